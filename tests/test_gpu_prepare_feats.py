"""nnet/lib/prepare_feats.py (stage 4 of the recipe: CMN, voiced-frame selection and 'CM ' compression on the device) and
make_mfcc.py --compress true through the device encoder, on a real MI355X.  Six synthetic utterances of 80 ... 48 037 samples go through
make_mfcc.py, then prepare_feats.py --cmn-window 300 --vad scp:vad.scp.  The yardsticks are the unchanged host writer
kaldi_io.write_compressed_mat (byte equality) and the fp64 restatement tests/frontend_ref.py; the drivers run once for the module:
make_mfcc.py, prepare_feats.py with the defaults, and prepare_feats.py --cm-header quartiles --min-len on a VAD table with an all-zero
vector and a missing entry."""
import io
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from tests import frontend_ref as F
from tests import mfcc_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")
LENS = {"utt_a": 16000, "utt_b": 24000, "utt_c": 48037, "utt_d": 80, "utt_e": 32000, "utt_f": 20011}      # utt_d: one frame

def _driver(name, argv):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", name)] + argv, env=env, cwd=PKG, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    tmp = tmp_path_factory.mktemp("prepare_feats")
    rs = np.random.RandomState(47)
    with open(str(tmp / "wav.scp"), "w") as scp:
        for k, n in LENS.items():
            path = str(tmp / (k + ".wav"))
            with wave.open(path, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(16000)
                w.writeframes(R.signal(rs, n, 16000.0).astype("<i2").tobytes())
            scp.write("%s %s\n" % (k, path))
    p = lambda name: str(tmp / name)
    _driver("make_mfcc.py", ["--compress", "true", p("wav.scp"), "ark,scp:%s,%s" % (p("raw.ark"), p("raw.scp")), "ark,scp:%s,%s" % (p("vad.ark"), p("vad.scp"))])
    vads = dict(kaldi_io.read_vec_flt_scp(p("vad.scp")))
    assert all(v.any() for v in vads.values()), "every synthetic utterance has a voiced frame"
    log = _driver("prepare_feats.py", ["--cmn-window", "300", "--vad", "scp:" + p("vad.scp"), "--write-utt2num-frames", p("utt2num_frames"),
                                       "ark:" + p("raw.ark"), "ark,scp:%s,%s" % (p("out.ark"), p("out.scp"))])
    # the second run: utt_b's decisions all zero, utt_e without an entry, --min-len at utt_a's voiced count, Kaldi's header points
    min_len = int(np.count_nonzero(vads["utt_a"]))
    with open(p("vad2.ark"), "wb") as f:
        for k, v in vads.items():
            if k != "utt_e":
                kaldi_io.write_vec_flt(f, np.zeros_like(v) if k == "utt_b" else v, key=k)
    log2 = _driver("prepare_feats.py", ["--vad", "ark:" + p("vad2.ark"), "--cm-header", "quartiles", "--min-len", str(min_len),
                                        "--write-utt2num-frames", p("utt2num_frames2"), "ark:" + p("raw.ark"), "ark:" + p("out2.ark")])
    return dict(tmp=tmp, p=p, vads=vads, log=log, log2=log2, min_len=min_len, expected=_kernel_frontend(p("raw.ark"), vads))


def _kernel_frontend(raw_ark, vads):
    """{key: the kernels' own decode -> CMN(300) -> selection of the raw archive's matrix, copied to the host}: one ops.frontend call."""
    import torch
    from tf_kaldi_speaker_amd import ops
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    items = list(kaldi_io.read_mat_ark_packed(raw_ark))
    assert [k for k, _ in items] == list(LENS) and all(isinstance(m, kaldi_io.PackedMatrix) for _, m in items)
    dev = torch.device("cuda:0")
    rows = np.asarray([m.rows for _, m in items], np.int64)
    sizes = [len(m.payload) for _, m in items]
    packed = torch.from_numpy(np.concatenate([np.frombuffer(m.payload, np.uint8) for _, m in items])).to(dev)
    x = ops.cm_decode_ragged(packed, np.cumsum(sizes) - sizes, rows, int(rows.max()), 30)
    masks = [(vads[k] != 0).astype(np.uint8) for k, _ in items]
    assert [len(m) for m in masks] == list(rows)
    y, rows_out = ops.frontend(x, torch.from_numpy(rows.astype(np.int32)).to(dev), 300, torch.from_numpy(np.concatenate(masks)).to(dev),
                               torch.from_numpy((np.cumsum(rows) - rows).astype(np.int64)).to(dev))
    y, rows_out = y.cpu().numpy(), rows_out.cpu().numpy()
    assert list(rows_out) == [int(m.sum()) for m in masks]
    return {k: y[i, :rows_out[i]].copy() for i, (k, _) in enumerate(items)}


def _records(ark):
    """{key: the bytes of its record behind "key "} of a binary archive of 'CM ' matrices, cut with the image sizes."""
    raw, out, at = open(ark, "rb").read(), {}, 0
    while at < len(raw):
        sp = raw.index(b" ", at)
        assert raw[sp + 1:sp + 6] == b"\0BCM ", raw[sp + 1:sp + 6]
        rows, cols = np.frombuffer(raw[sp + 6 + 8:sp + 6 + 16], "<i4")
        size = 5 + 16 + 8 * cols + cols * rows
        out[raw[at:sp].decode()] = raw[sp + 1:sp + 1 + size]
        at = sp + 1 + size
    return out


def _host_record(m, header):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    buf = io.BytesIO()
    kaldi_io.write_compressed_mat(buf, m, key="", header=header)
    return buf.getvalue()


def test_archive_is_the_host_codec_image_of_the_kernel_front_end(run):
    """Every matrix the driver wrote == write_compressed_mat(header="uniform") of the kernels' own front-end output, byte for byte: the
    chain adds no error beyond the codec; utt2num_frames holds the voiced counts; the scp offsets point at the token."""
    p, vads, expected = run["p"], run["vads"], run["expected"]
    records = _records(p("out.ark"))
    assert list(records) == list(LENS)
    for k in LENS:
        assert records[k] == _host_record(expected[k], "uniform"), k
    assert [ln.split() for ln in open(p("utt2num_frames"))] == [[k, str(int(np.count_nonzero(vads[k])))] for k in LENS]
    raw = open(p("out.ark"), "rb").read()
    lines = [ln.split() for ln in open(p("out.scp"))]
    assert [k for k, _ in lines] == list(LENS)
    for k, rx in lines:
        path, at = rx.rsplit(":", 1)
        assert path == p("out.ark") and raw[int(at):int(at) + 5] == b"\0BCM " and raw[int(at) - len(k) - 1:int(at)] == (k + " ").encode()
    assert "Prepared 6 utterances" in run["log"]
    assert expected["utt_d"].shape == (1, 30)      # the one-frame utterance went through: a 'CM ' matrix of one row


def test_decoded_features_within_front_end_tolerance_plus_codec_step(run):
    """|decoded - ref| <= 2^-23 |ref| + 2^-32 A (tests/test_gpu_frontend.py: one fp32 rounding of a mean accumulated in double, A the raw
    utterance's max |x|) + (max - min) / 255 of the column (the step tests/test_gpu_make_mfcc.py allows the evenly spaced header), ref the
    fp64 restatement on the raw archive's own matrices and decisions."""
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    p, vads = run["p"], run["vads"]
    raw = dict(kaldi_io.read_mat_scp(p("raw.scp")))
    worst = 0.0
    for k, got in kaldi_io.read_mat_scp(p("out.scp")):
        ref = F.frontend(raw[k], 300, vads[k] != 0)
        assert got.shape == ref.shape
        tol = 2.0 ** -23 * np.abs(ref) + 2.0 ** -32 * float(np.abs(raw[k]).max()) + (ref.max(axis=0) - ref.min(axis=0))[None, :] / 255.0
        if len(ref) == 1:
            assert not ref.any() and not got.any()      # one frame: x - x
            continue
        ratio = float((np.abs(got.astype(np.float64) - ref) / tol).max())
        print("%s: %d of %d frames, worst error / tolerance %.3f" % (k, len(ref), len(raw[k]), ratio))
        worst = max(worst, ratio)
    assert worst <= 1.0, worst


def test_min_len_skips_and_quartile_header(run):
    """--min-len N drops exactly the utterances of N voiced frames or fewer; an all-zero VAD vector and a missing entry are skipped and named
    in the log; what stays equals write_compressed_mat(header="quartiles") of the kernels' front-end output."""
    p, vads, expected, n = run["p"], run["vads"], run["expected"], run["min_len"]
    voiced = {k: int(np.count_nonzero(v)) for k, v in vads.items()}
    keep = [k for k in LENS if k not in ("utt_b", "utt_e") and voiced[k] > n]
    assert voiced["utt_a"] == n and "utt_a" not in keep and "utt_d" not in keep and len(keep) >= 2
    records = _records(p("out2.ark"))
    assert list(records) == keep
    for k in keep:
        assert records[k] == _host_record(expected[k], "quartiles"), k
    assert [ln.split() for ln in open(p("utt2num_frames2"))] == [[k, str(voiced[k])] for k in keep]
    log = run["log2"]
    assert "Key utt_b has no voiced frame, skip." in log and "Key utt_e has no VAD entry, skip." in log
    assert "Key utt_a length too short, %d <= %d, skip." % (n, n) in log and "Key utt_d length too short, 1 <= %d, skip." % n in log


def test_wrong_vad_length_is_an_error_by_key(run, tmp_path):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    p, vads = run["p"], run["vads"]
    with open(str(tmp_path / "vad.ark"), "wb") as f:
        for k, v in vads.items():
            kaldi_io.write_vec_flt(f, v[:-1] if k == "utt_c" else v, key=k)
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", "prepare_feats.py"), "--vad", "ark:" + str(tmp_path / "vad.ark"),
                        "ark:" + p("raw.ark"), "ark:" + str(tmp_path / "out.ark")], env=env, cwd=PKG, capture_output=True, text=True, timeout=600)
    n = len(vads["utt_c"])
    assert r.returncode != 0 and "Key utt_c: %d frames but %d VAD decisions" % (n, n - 1) in r.stderr, r.stderr[-2000:]


def test_loaders_read_the_directory_after_filter_data_dir(run, tmp_path):
    """out.scp + utt2num_frames + a utt2spk, through misc/tools/filter_data_dir.py: FeatureReader and KaldiDataRandomQueue accept the result."""
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.dataset.data_loader import KaldiDataRandomQueue
    from tf_kaldi_speaker_amd.misc.tools import filter_data_dir
    p, vads, expected = run["p"], run["vads"], run["expected"]
    data = str(tmp_path / "train")
    os.makedirs(data)
    for name, src in (("feats.scp", "out.scp"), ("utt2num_frames", "utt2num_frames")):
        open(os.path.join(data, name), "w").write(open(p(src)).read())
    spk = {"utt_a": "spk1", "utt_b": "spk1", "utt_c": "spk2", "utt_d": "spk2", "utt_e": "spk2", "utt_f": "spk3"}
    open(os.path.join(data, "utt2spk"), "w").write("".join("%s %s\n" % (k, spk[k]) for k in reversed(list(LENS))))
    assert filter_data_dir.filter_data_dir(data, min_len=1, min_num_utts=2) == (4, 2)      # utt_d: one frame; spk3: one utterance
    assert open(os.path.join(data, "spk2utt")).read() == "spk1 utt_a utt_b\nspk2 utt_c utt_e\n"
    open(os.path.join(data, "spklist"), "w").write("spk1 0\nspk2 1\n")
    rd = kaldi_io.FeatureReader(data)
    assert rd.dim == 30
    for line in open(os.path.join(data, "feats.scp")):
        k = line.split()[0]
        m, _ = rd.read(line.strip())
        want = kaldi_io.read_mat(io.BytesIO(_host_record(expected[k], "uniform")))
        assert np.array_equal(m.view(np.uint32), want.view(np.uint32)), k
    rd.close()
    shortest = min(int(np.count_nonzero(vads[k])) for k in ("utt_a", "utt_b", "utt_c", "utt_e"))
    assert shortest > 30
    q = KaldiDataRandomQueue(data, os.path.join(data, "spklist"), num_parallel=1, max_qsize=2, num_speakers=2, num_segments=1, min_len=20, max_len=30, seed=1)
    q.start()
    f, labels = q.fetch()
    q.stop()
    assert f.shape[0] == 2 and 20 <= f.shape[1] <= 30 and f.shape[2] == 30 and sorted(labels) == [0, 1] and np.isfinite(f).all()


def test_make_mfcc_compress_true_equals_the_host_codec(run):
    """The archive make_mfcc.py --compress true wrote through the device encoder == write_compressed_mat(header="uniform") of
    FeatureExtractor.extract's float features, byte for byte; the encoded form of extract() gives the same images."""
    from tf_kaldi_speaker_amd.misc import features
    p = run["p"]
    waves = [features.read_wav(line.split(None, 1)[1].strip()) for line in open(p("wav.scp"))]
    fx = features.FeatureExtractor(workspace_bytes=1 << 20)      # 1 MB: several batches
    direct = fx.extract(waves)
    coded = fx.extract(waves, cm_header="uniform")
    records = _records(p("raw.ark"))
    assert list(records) == list(LENS)
    for k, (x, decisions), (image, decisions2) in zip(LENS, direct, coded):
        want = _host_record(x, "uniform")
        assert records[k] == want, k
        assert b"\0BCM " + bytes(image) == want and np.array_equal(decisions, decisions2), k
