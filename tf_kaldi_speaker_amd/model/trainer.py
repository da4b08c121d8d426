"""Trainer with the reference's public surface (model/trainer.py:17-730):

    Trainer(params, model_dir, single_cpu=False)
    .build(mode in {"train","valid","predict"}, dim, loss_type=None, num_speakers=None, noupdate_var_list=None)
    .train(data, spklist, learning_rate, aux_data=None)       one epoch, resumes from the latest checkpoint
    .valid(data, spklist, batch_type="softmax", output_embeddings=False, aux_data=None) -> (loss, emb, labels)
    .predict(features [T,D] | [B,T,D]) -> [E] | [B,E]
    .save(step) / .load() -> step / .reset() / .close()
    attributes callers touch: .sess, .embeddings, .endpoints, .params, .model

The TF1 session/graph is replaced by the native MI355X engine (csrc/xv_engine.hip; forward, backward and update in
csrc/xv_engine_fwd / _bwd / _step.hip) reached through the C-ABI; this file is host logic only (loader, loop, logging, checkpoints, data parallelism).
Checkpoints: <model>/nnet/model-<step>.npz (variables by TF name + optimiser state) plus the
TF-format text index <model>/nnet/checkpoint that run_extract_embeddings.sh tests for.
"""
import logging
import os
import re
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

try:
    from .. import engine as E
    from .. import _lib, kinds
    from ..parallel import GradAllReduce, average_bn_statistics, broadcast_variables
    from ..dataset.data_loader import KaldiDataRandomQueue, KaldiDataSeqQueue, PlannedRandomQueue, DataOutOfRange
    from ..misc.utils import substring_in_list, read_checkpoint_state, write_checkpoint_state
    from ..misc import tf_checkpoint
    from .tdnn import tdnn, extended_tdnn, engine_config, collect_endpoints, check_params
    from . import loss as _loss
    from . import predict as _predict
except (ImportError, ValueError):      # drop-in layout: PYTHONPATH=$TF_KALDI_ROOT
    import engine as E
    import _lib
    import kinds
    from parallel import GradAllReduce, average_bn_statistics, broadcast_variables
    from dataset.data_loader import KaldiDataRandomQueue, KaldiDataSeqQueue, PlannedRandomQueue, DataOutOfRange
    from misc.utils import substring_in_list, read_checkpoint_state, write_checkpoint_state
    from misc import tf_checkpoint
    from model.tdnn import tdnn, extended_tdnn, engine_config, collect_endpoints, check_params
    from model import loss as _loss
    from model import predict as _predict

log = logging.getLogger("tf_kaldi_speaker_amd")


class _Session(object):
    """Stand-in for the tf.Session attribute some callers close explicitly."""

    def __init__(self, owner):
        self._owner = owner

    def close(self):
        self._owner._close_engine()


def _dist():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return dist
    except Exception:
        pass
    return None


class Trainer(object):
    def __init__(self, params, model_dir, single_cpu=False):
        self.network_type = params.network_type
        if params.network_type == "tdnn":
            self.network = tdnn
        elif params.network_type == "extended_tdnn":      # tdnn's layer recipe on params.tdnn_layers (no reference counterpart)
            self.network = extended_tdnn
        else:
            raise NotImplementedError("Not implement %s network" % params.network_type)
        self.loss_type = None
        self.loss_network = None
        self.params = params
        self.single_cpu = single_cpu       # accepted for signature parity; the engine always runs on the GPU
        self.model = os.path.join(model_dir, "nnet")
        self.sess = _Session(self)
        self.engine = None
        self.dim = None
        self.num_speakers = None
        self.global_step = None
        self.learning_rate = None
        self.embeddings = None
        self.endpoints = None
        self.optimizer = None
        self.total_loss = None
        self.train_op = None
        self.train_ops = {}
        self.valid_ops = {}
        self.saver = None
        self.is_built = False
        self.is_loaded = False
        self.modes = set()
        self.device = "cuda:%d" % _lib.local_device_index()

    # ------------------------------------------------------------------ lifecycle
    def _close_engine(self):
        if self.engine is not None:
            self.engine.close()
            self.engine = None

    def reset(self):
        """Drop the graph so a new one can be built (reference trainer.py:114-133)."""
        self._close_engine()
        self.is_built = False
        self.is_loaded = False
        self.modes = set()
        self.saver = None

    def close(self):
        self._close_engine()

    def _capacity(self):
        p = self.params.dict
        b = int(p.get("num_speakers_per_batch", 64)) * int(p.get("num_segments_per_speaker", 1))
        t = int(p.get("max_segment_len", 400))
        return max(b, 1), max(t, 15)

    def _make_engine(self, num_speakers, loss_type, max_batch, max_frames, max_rows=0, training_state=False):
        """The engine of this configuration and capacity; in the place of the present one (engine.rebuild: its variables carried over, with
        training_state also the optimiser state, the update count and the update filter), else new with initial values."""
        cfg = engine_config(self.params, self.dim, num_speakers or 0, loss_type or "softmax", max_batch, max_frames, max_rows)
        seed = int(self.params.dict.get("seed", 0))
        if self.engine is not None:
            old, self.engine = self.engine, None
            return E.rebuild(old, cfg, seed=seed, training_state=training_state)
        eng = E.Engine(cfg, device=self.device)
        eng.init_variables(seed=seed)
        return eng

    def _ensure_capacity(self, b, t, rows=0):
        """Grow the engine to hold b chunks of t frames.  rows > 0 (batched extraction): a capacity in rows = chunks x frames instead
        of the full b x t rectangle - many short utterances or a few long ones per batch."""
        eng = self.engine
        cfg = eng.config
        have_rows = cfg.max_rows if cfg.max_rows > 0 else cfg.max_batch * cfg.max_frames
        need_rows = rows if rows > 0 else b * t      # (rows given: b and t are the largest batch and the longest utterance of DIFFERENT batches)
        if b <= cfg.max_batch and t <= cfg.max_frames and need_rows <= have_rows:
            return
        nb, nt = max(b, cfg.max_batch), max(t, cfg.max_frames)
        if t > cfg.max_frames:
            nt = max(t, min(2 * cfg.max_frames, 20000))
        nrows = 0
        if rows > 0 or cfg.max_rows > 0:
            # row-bounded capacity: chunks and frames per chunk cost nothing beyond the rows, so take them generously once instead of
            # rebuilding the engine whenever a later window holds a slightly longer utterance or a slightly larger batch
            nrows = max(need_rows, cfg.max_rows)
            nb, nt = max(nb, self.PREDICT_CHUNKS), max(nt, 20000)
        self.engine = self._make_engine(self.num_speakers, self.loss_type, nb, nt, max_rows=nrows, training_state=True)

    # ------------------------------------------------------------------ build
    def build(self, mode, dim, loss_type=None, num_speakers=None, noupdate_var_list=None):
        assert (mode == "train" or mode == "valid" or mode == "predict")
        check_params(self.params)
        self.dim = int(dim)
        if mode == "predict":
            if "embedding_node" not in self.params.dict:
                raise KeyError("embedding_node")
            log.info("Extract embedding from node %s" % self.params.embedding_node)
            if self.engine is None:
                self.engine = self._make_engine(0, "softmax", 1, 400)
            self.embeddings = self.params.embedding_node
            self.modes.add(mode)
            self.is_built = True
            return

        self.params.dict["global_step"] = 0
        self.loss_type = loss_type
        if kinds.family(loss_type) == kinds.REFUSED:
            raise NotImplementedError("Not implement %s loss on the MI355X engine (outside the hot path)" % loss_type)
        self.loss_network = getattr(_loss, kinds.loss(loss_type).name)
        if mode == "train":
            if "optimizer" not in self.params.dict:
                self.params.dict["optimizer"] = "sgd"
            if self.params.optimizer == "sgd":
                if "momentum" in self.params.dict:
                    sys.exit("Using sgd as the optimizer and you should not specify the momentum.")
            elif self.params.optimizer not in ("momentum", "adam"):
                sys.exit("Optimizer %s is not supported." % self.params.optimizer)
            self.optimizer = self.params.optimizer
        self.num_speakers = int(num_speakers)
        b, t = self._capacity()
        if self.engine is None or self.engine.config.num_speakers != self.num_speakers:
            self.engine = self._make_engine(self.num_speakers, loss_type, b, t)
        self.embeddings = "output"          # valid embeddings = endpoints["output"], trainer.py:308
        self.modes.add(mode)
        self.is_built = True
        if mode == "train" and noupdate_var_list is not None:
            # fine-tuning (trainer.py:379-403): variables - and BN UPDATE_OPS - whose name contains one of the strings are left alone
            self._frozen = [n for n in self.engine.table if substring_in_list(n, noupdate_var_list)]
            for n in self.engine.table:
                log.info("[Info] Var %s will not be updated" % n if n in self._frozen else "[Info] Train %s" % n)
        self._apply_update_filter()

    def _apply_update_filter(self):
        if self.engine is not None:
            self.engine.set_update_filter(getattr(self, "_frozen", None) or ())

    # ------------------------------------------------------------------ checkpoints
    def save(self, step, sync_bn=True):
        """sync_bn: average the BN moving statistics over the ranks first - a COLLECTIVE, so every rank must make this call
        (the epoch loop does); sync_bn=False is for a caller that runs on one rank only (get_finetune_model on rank 0)."""
        dist = _dist()
        if dist is not None:
            if sync_bn:
                average_bn_statistics(dist, self.engine.variables, self.engine.n_train, dist.get_world_size())
            if dist.get_rank() != 0:
                return
        os.makedirs(self.model, exist_ok=True)
        path = os.path.join(self.model, "model-%d" % step)
        arrays = dict(self.engine.get_variables())
        arrays["__opt_state__"] = self.engine.opt_state.cpu().numpy()
        arrays["__update_count__"] = np.array([self.engine.update_count], np.int64)
        tmp = path + ".tmp.npz"
        np.savez(tmp, **arrays)
        os.replace(tmp, path + ".npz")
        if self.params.dict.get("save_tf_checkpoint", False):
            # the same variables as a TensorFlow V2 checkpoint (model-<step>.index / .data-00000-of-00001) the reference's
            # tf.train.Saver restores (trainer.py:142-158): an upstream user can pick the model up without this package
            tf_checkpoint.write_checkpoint(path, self.engine.get_variables())
        # the index keeps BASENAMES (TF's save_relative_paths form): the model directory can be moved or copied and pruning
        # / loading still find the payloads; entries written with a directory part by older runs are read by basename
        name = os.path.basename(path)
        _, listed = read_checkpoint_state(self.model)
        names = [n for n in (os.path.basename(q) for q in listed) if n != name] + [name]
        keep = int(self.params.dict.get("keep_checkpoint_max", 5))
        while keep > 0 and len(names) > keep:
            old = os.path.join(self.model, names.pop(0))
            for ext in (".npz", ".index", ".data-00000-of-00001"):
                if os.path.exists(old + ext):
                    os.remove(old + ext)
        write_checkpoint_state(self.model, name, names)

    def _set_variables_or_exit(self, stored, path):
        """The engine's table filled from a checkpoint's variables (either format); a checkpoint that lacks one ends the run."""
        missing = [k for k in self.engine.table if k not in stored]
        if missing:
            sys.exit("Checkpoint %s lacks variables: %s" % (path, ", ".join(missing[:5])))
        self.engine.set_variables({k: stored[k] for k in self.engine.table})

    def load(self):
        log.info("Reading checkpoints...")
        current, _ = read_checkpoint_state(self.model)
        if not current:
            sys.exit("Failed to find a checkpoint in {}".format(self.model))
        ckpt_name = os.path.basename(current)
        step = int(next(re.finditer(r"(\d+)(?!.*\d)", ckpt_name)).group(0))
        path = os.path.join(self.model, ckpt_name + ".npz")
        if not os.path.isfile(path):
            prefix = os.path.join(self.model, ckpt_name)
            if os.path.isfile(prefix + ".index"):
                # a checkpoint written by the reference's tf.train.Saver (trainer.py:318,444; the pretrained models of README.md:86-104):
                # same variable names and shapes, read without TensorFlow (misc/tf_checkpoint.py).  Optimiser slots are not taken over.
                self._set_variables_or_exit(tf_checkpoint.read_checkpoint(prefix), prefix + ".index")
                log.info("Succeed to load TensorFlow checkpoint {}".format(ckpt_name))
                self.is_loaded = True
                return step
            sys.exit("Failed to find a checkpoint in {}".format(self.model))
        data = np.load(path)
        self._set_variables_or_exit({k: data[k] for k in data.files if not k.startswith("__")}, path)
        if "__opt_state__" in data.files and data["__opt_state__"].size == self.engine.opt_state.numel():
            self.engine.opt_state.copy_(torch.from_numpy(data["__opt_state__"]))
        if "__update_count__" in data.files:
            self.engine.update_count = int(data["__update_count__"][0])
        log.info("Succeed to load checkpoint {}".format(ckpt_name))
        self.is_loaded = True
        return step

    # ------------------------------------------------------------------ training
    def _training_queue(self, data, spklist, gpu_decode=False):
        """The random queue of training batches.  KaldiDataRandomQueue = the C++ loader (libxvector_io.so: planning + decoding in native
        threads); XV_LOADER=python plans the batches in Python and only decodes natively (dataset/data_loader.py) - same rules, same batch
        contract.  gpu_decode (train() under XV_LOADER=gpu_decode): the native threads only gather the rows' 'CM ' bytes, the batch is
        decoded on the GPU (xv_cm_decode) - a quarter of the host memory traffic and PCIe bytes, bit-identical features ('CM ' archives only)."""
        p = self.params
        queue_cls = PlannedRandomQueue if os.environ.get("XV_LOADER", "native") == "python" else KaldiDataRandomQueue
        return queue_cls(data, spklist, num_parallel=p.num_parallel_datasets, max_qsize=p.max_queue_size,
                         num_speakers=p.num_speakers_per_batch, num_segments=p.num_segments_per_speaker,
                         min_len=p.min_segment_len, max_len=p.max_segment_len, shuffle=True, **({"packed": True} if gpu_decode else {}))

    def train(self, data, spklist, learning_rate, aux_data=None):
        """One epoch over `num_steps_per_epoch` random batches (reference trainer.py:451-520)."""
        assert "train" in self.modes, "call build('train', ...) first"
        p = self.params
        curr_step = 0
        if os.path.isfile(os.path.join(self.model, "checkpoint")):
            curr_step = self.load()
        dist = _dist()
        if dist is not None:
            broadcast_variables(dist, self.engine.variables, 0)
            self.engine.lib.xv_engine_invalidate_weights(self.engine.h)
        loader = self._training_queue(data, spklist, gpu_decode=os.environ.get("XV_LOADER") == "gpu_decode")
        loader.start()
        try:
            if hasattr(loader, "device_batches"):        # pinned staging + asynchronous H2D on a copy stream
                batches = loader.device_batches(self.device)
            else:
                batches = iter(loader.fetch, None)
            curr_step = self.train_batches(batches, learning_rate, curr_step)
        finally:
            loader.stop()
        self.save(curr_step)
        return

    def train_batches(self, batches, learning_rate, curr_step=0, num_steps=None):
        """The hot loop on an iterator of (features [B,T,D], labels [B]); returns the new global step.
        curr_step (the count of optimiser steps incl. resumed ones) feeds the lambda schedule."""
        p = self.params
        dist = _dist()
        allreduce = GradAllReduce(dist, dist.get_world_size()) if dist is not None else None
        rank0 = dist is None or dist.get_rank() == 0
        steps_per_epoch = int(p.num_steps_per_epoch) if num_steps is None else int(num_steps)
        epoch = int(curr_step / p.num_steps_per_epoch) if num_steps is None else 0
        first = curr_step % steps_per_epoch if num_steps is None else 0
        show = int(p.dict.get("show_training_progress", 100))
        save_every = int(p.dict.get("save_checkpoints_steps", 0) or 0)
        # data parallelism: BN moving statistics follow each rank's own batches (local batch statistics);
        # they are re-averaged every `bn_sync_steps` optimiser steps (one all-reduce of a few thousand floats) and before every
        # checkpoint, so replicas never drift further apart than that many moving-average updates
        bn_sync = int(p.dict.get("bn_sync_steps", 100) or 0) if dist is not None else 0
        for step in range(first, steps_per_epoch):
            try:
                start_time = time.time()
                features, labels = next(batches)
            except (DataOutOfRange, StopIteration):
                log.info("Finished reading features.")
                break
            self._ensure_capacity(features.shape[0], features.shape[1])
            verbose = show > 0 and step % show == 0
            losses = self.engine.train_step(features, labels, learning_rate, curr_step, allreduce=allreduce,
                                            fetch_losses=verbose)
            if verbose and rank0:
                raw, reg = losses
                self.train_ops = {"raw_loss": raw, "loss": raw + reg}
                log.info("Epoch: [%2d] step: [%2d/%2d] time: %.4f s/step, raw loss: %f, total loss: %f"
                         % (epoch, step, steps_per_epoch, time.time() - start_time, raw, raw + reg))
            if save_every > 0 and step % save_every == 0 and curr_step != 0:
                self.save(curr_step)
            elif bn_sync > 0 and (curr_step + 1) % bn_sync == 0:
                average_bn_statistics(dist, self.engine.variables, self.engine.n_train, dist.get_world_size())
            curr_step += 1
        return curr_step

    # ------------------------------------------------------------------ validation / inference
    def valid(self, data, spklist, batch_type="softmax", output_embeddings=False, aux_data=None):
        """Mean validation loss with the margin switched off (trainer.py:261-271) and BN in inference
        mode; optionally all "output" embeddings + labels in file order (trainer.py:592-706)."""
        assert "valid" in self.modes, "call build('valid', ...) first"
        assert batch_type == "softmax" or batch_type == "end2end", "The batch_type can only be softmax or end2end"
        p = self.params
        if batch_type == "end2end":
            # N speakers x M segments per batch, speaker-major, as the end-to-end validation loss needs them (trainer.py:667-680)
            assert "num_valid_speakers_per_batch" in p.dict and "num_valid_segments_per_speaker" in p.dict, \
                "Valid parameters should be set if E2E loss is selected"
            if kinds.family(self.loss_type) not in kinds.HEADS_WITHOUT_SPEAKERS:
                raise NotImplementedError("end2end validation batches belong to %s, not to %s"
                                          % (" / ".join(n for n in kinds.LOSSES if kinds.family(n) in kinds.HEADS_WITHOUT_SPEAKERS), self.loss_type))
        curr_step = 0
        if os.path.isfile(os.path.join(self.model, "checkpoint")):
            curr_step = self.load()
        else:
            log.info("[Warning] Cannot find model in %s. Random initialization is used in validation." % self.model)
        bsz = p.num_speakers_per_batch * p.num_segments_per_speaker
        embeddings_val, labels_val = None, None
        common = dict(num_parallel=2, max_qsize=10, min_len=p.min_segment_len, max_len=p.max_segment_len)
        if output_embeddings:
            embs, labs = [], []

            def keep_embeddings(features, labels):
                embs.append(self.engine.endpoint("output").cpu().numpy())
                labs.append(np.asarray(labels))
            self._inference_pass(KaldiDataSeqQueue(data, spklist, batch_size=bsz, shuffle=False, **common), keep_embeddings)
            if embs:
                embeddings_val, labels_val = np.concatenate(embs, 0), np.concatenate(labs, 0)
        if batch_type == "end2end":
            loader = KaldiDataRandomQueue(data, spklist, num_speakers=p.num_valid_speakers_per_batch,
                                          num_segments=p.num_valid_segments_per_speaker, shuffle=True, **common)
        else:
            loader = KaldiDataSeqQueue(data, spklist, batch_size=bsz, shuffle=True, **common)
        losses = []

        def keep_loss(features, labels):
            self.engine.loss(labels, curr_step, with_margin=False)
            self._last_valid_labels = np.asarray(labels)
            self._last_valid_features = features          # (the batch a test restates; a reference to what the loader returned)
            losses.append(self.engine.raw_loss())
        self._inference_pass(loader, keep_loss, int(p.valid_max_iterations))
        total, num_batches = sum(losses, 0.0), len(losses)
        loss = total / max(num_batches, 1)
        log.info("[Validation %d batches] valid loss: %f" % (num_batches, loss))
        return loss, embeddings_val, labels_val

    def _inference_pass(self, loader, each, limit=None):
        """each(features, labels) after an inference forward of every batch the loader gives - at most `limit`, else until it runs out;
        the loader is started here and stopped here, whatever happens."""
        loader.start()
        try:
            n = 0
            while limit is None or n < limit:
                try:
                    features, labels = loader.fetch()
                except DataOutOfRange:
                    break
                self._ensure_capacity(features.shape[0], features.shape[1])
                self.engine.forward(features, False)
                each(features, labels)
                n += 1
        finally:
            loader.stop()

    def _ensure_loaded(self):
        if not self.is_loaded:
            if os.path.isfile(os.path.join(self.model, "checkpoint")):
                self.load()
            else:
                sys.exit("Cannot find model in %s" % self.model)

    def predict(self, features):
        """Embedding(s) of `embedding_node` with BN in inference mode (trainer.py:708-726)."""
        self._ensure_loaded()
        features = np.asarray(features, np.float32)
        rank = len(features.shape)
        assert (rank == 2 or rank == 3)
        if rank == 2:
            features = np.expand_dims(features, axis=0)
        self._ensure_capacity(features.shape[0], features.shape[1])
        self.engine.forward(features, False)
        node = self.params.embedding_node
        emb = self.engine.endpoint(node)
        b = features.shape[0]
        if emb.shape[0] != b:
            emb = emb.view(b, emb.shape[0] // b, emb.shape[1])
        emb = emb.cpu().numpy()
        self.endpoints = OrderedDict([(node, emb)])
        if rank == 2:
            emb = np.squeeze(emb, axis=0)
        return emb

    # rows (chunks x frames) of one batched-extraction forward: about two S1 training batches - large enough for the GEMMs to run at
    # their training-pass rate, small enough that the activation arena stays at a few GB
    PREDICT_ROWS = 49152
    PREDICT_CHUNKS = 128

    def predict_batch(self, items, return_device=False, cmn_window=0, voiced=None):
        """Embeddings of MANY utterances of different lengths, [n, E] in the order given - the batched form of the loop
        extract.py:64-93 runs one predict() at a time.  items: float32 matrices [T_i, D] and / or kaldi_io.PackedMatrix ('CM '
        matrices as read from the archive, decoded on the GPU).  Utterances are sorted by length, padded to the longest of their
        batch (misc.utils.plan_length_batches) and run through xv_engine_forward_lengths, whose pooling sees only each utterance's
        own frames; the embedding node must be a segment-level one (tdnn6_dense, tdnn7_*, output).
        cmn_window / voiced: the recipe's feature pipe on the GPU (Engine.frontend) for items that are RAW features - sliding-window
        CMN over cmn_window frames (0 = off), then the frames whose entry in voiced[i] (one uint8 array per item; None = all) is
        non-zero.  An item may also be a kaldi_io.VoicedRows (raw utterance + mask + a range of its kept frames: extract.py's chunks).
        Lengths - the batch plan, the receptive-field check - then count the frames left after selection.
        Items of the third kind, kaldi_io.DeviceRows (all of them, then), are raw features and masks that are on the device already -
        extract.py's wav mode.  The path itself - plan, staging, batch loop - is model/predict.py."""
        self._ensure_loaded()
        return _predict.predict_batch(self, items, return_device, cmn_window, voiced)

    # ------------------------------------------------------------------ fine-tuning / diagnostics (trainer.py:522-590, 728-920)
    def set_trainable_variables(self, variable_list=None):
        """Only the trainable variables whose name contains one of the strings are optimised (None: all).  BN moving statistics
        keep updating (trainer.py:728-773)."""
        assert "train" in self.modes, "call build('train', ...) first"
        if variable_list is None:
            log.info("[Info] Add all trainable variables to the optimizer.")
            self._frozen = []
        else:
            self._frozen = []
            for n, (_, _, trainable) in self.engine.table.items():
                if not trainable:
                    continue
                if substring_in_list(n, variable_list):
                    log.info("[Info] Add %s to trainable list" % n)
                else:
                    self._frozen.append(n)
        self._apply_update_filter()

    def get_finetune_model(self, excluded_list):
        """Start from the pre-trained checkpoint in the model directory; variables whose name contains a string of `excluded_list`
        keep their default initialisation.  The pre-trained files are backed up (`.bak`) and the result is saved as step 0
        (trainer.py:775-819)."""
        assert self.engine is not None, "call build(...) first"
        self.engine.init_variables(seed=int(self.params.dict.get("seed", 0)))
        fresh = self.engine.get_variables()
        current, _ = read_checkpoint_state(self.model)
        if not current:
            sys.exit("Failed to find a checkpoint in {}".format(self.model))
        path = os.path.join(self.model, os.path.basename(current) + ".npz")
        data = np.load(path)
        values = {}
        for name in self.engine.table:
            if substring_in_list(name, excluded_list):
                log.info("[Info] Ignore %s when loading the checkpoint" % name)
                values[name] = fresh[name]
            elif name in data.files and tuple(data[name].shape) == tuple(fresh[name].shape):
                values[name] = data[name]
            else:
                sys.exit("Checkpoint %s lacks variable %s (exclude it to re-initialise it)" % (path, name))
        self.engine.set_variables(values)
        self.engine.opt_state.zero_()
        self.engine.update_count = 0
        import glob
        import shutil
        for filename in glob.glob(os.path.join(self.model, os.path.basename(current)) + "*"):
            if not filename.endswith(".bak"):
                shutil.copyfile(filename, filename + ".bak")
        self.save(0, sync_bn=False)      # no collective: nnet/lib/train.py calls this on rank 0 only (replicas are identical here)
        self.is_loaded = True

    def train_tune_lr(self, data, spklist, tune_period=100, aux_data=None, tune_times=None):
        """Learning-rate range test (trainer.py:522-590): lr = 1e-5 * 1.15^(step // tune_period), global_step fed as 0, the
        (step, lr, total loss) of the first step of every period written to <model>/learning_rate_tuning."""
        assert "train" in self.modes, "call build('train', ...) first"
        p = self.params
        if tune_times is None:      # the reference hard-codes 100 learning rates (trainer.py:556); XV_TUNE_TIMES shortens a smoke run
            tune_times = int(os.environ.get("XV_TUNE_TIMES", "100"))
        self.engine.init_variables(seed=int(p.dict.get("seed", 0)))
        if os.path.isfile(os.path.join(self.model, "checkpoint")):
            self.load()
        loader = self._training_queue(data, spklist)      # never the packed form: this loop fetches host batches
        loader.start()
        init_learning_rate, factor = 1e-5, 1.15
        os.makedirs(self.model, exist_ok=True)
        try:
            with open(os.path.join(self.model, "learning_rate_tuning"), "w") as fp_lr:
                for step in range(int(tune_period) * int(tune_times)):
                    lr = init_learning_rate * (factor ** (step // tune_period))
                    start_time = time.time()
                    features, labels = loader.fetch()
                    self._ensure_capacity(features.shape[0], features.shape[1])
                    first = step % tune_period == 0
                    losses = self.engine.train_step(features, labels, lr, 0, fetch_losses=first)
                    if first:
                        raw, reg = losses
                        log.info("Epoch: step: %2d, time: %.4f s/step, lr: %f, raw loss: %f, total loss: %f"
                                 % (step, time.time() - start_time, lr, raw, raw + reg))
                        fp_lr.write("%d %f %f\n" % (step, lr, raw + reg))
        finally:
            loader.stop()

    def insight(self, data, spklist, batch_type="softmax", output_embeddings=False, aux_data=None):
        """The reference's debugging pass (trainer.py:821-920) without its pdb breakpoint: validation loss, optional embeddings /
        labels in file order, and the accuracy of the last validation batch in the log."""
        loss, emb, labels = self.valid(data, spklist, batch_type=batch_type, output_embeddings=output_embeddings, aux_data=aux_data)
        try:
            logits = self.engine.endpoint("logits").cpu().numpy()
            lab = self._last_valid_labels
            log.info("Acc: %f" % (float(np.sum(np.argmax(logits[:, :self.num_speakers], axis=1) == lab)) / float(lab.shape[0])))
        except Exception:
            pass
        return loss, emb, labels
