"""Layer helpers with the reference's model/common.py names, evaluated on the GPU through the
C-ABI (no TensorFlow graph: calls execute eagerly on torch CUDA buffers)."""
from collections import OrderedDict

import numpy as np
import torch

try:
    from .. import ops, kinds
except (ImportError, ValueError):   # drop-in layout (PYTHONPATH=$TF_KALDI_ROOT)
    import ops
    import kinds


def shape_list(x):
    """Static shape as a list (reference common.py:7-24)."""
    return list(x.shape)


def to_device(x, dtype=torch.float32, device="cuda:0"):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    np_dtype = np.float32 if dtype == torch.float32 else np.int32
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np_dtype)).to(device)


def l2_scaling(x, scaling_factor, epsilon=1e-12, name="l2_norm"):
    """x * rsqrt(max(sum x^2, eps)) * scaling_factor along the last axis (reference common.py:45-58)."""
    if epsilon != 1e-12:
        raise NotImplementedError("l2_scaling: the HIP kernel fixes epsilon = 1e-12 (common.py:45)")
    x = to_device(x)
    flat = x.reshape(-1, x.shape[-1])
    return ops.l2_scaling_forward(flat, scaling_factor).reshape(x.shape)


class VariableStore(object):
    """The variables of one module-level scope, by their TF name: tf.get_variable's create / reuse with its two errors, and preset.  A new
    variable takes kinds.initial_value from RandomState(seed + the number of variables the store holds).  `variables` is the mapping itself
    (tests clear and read it); when a call may create and when it may reuse is the owning module's rule."""

    def __init__(self, to_device, getter="tf.get_variable()"):
        self.variables, self.seed, self.to_device, self.getter = OrderedDict(), 0, to_device, getter

    def reset(self, seed=0):
        self.variables.clear()
        self.seed = seed

    def preset(self, name, value):
        self.variables[name] = self.to_device(value)

    def get(self, name, shape, create=True, reuse=True, constant=None):
        shape = tuple(shape) or (1,)
        if name in self.variables:
            if not reuse:
                raise ValueError("Variable %s already exists, disallowed. Did you mean to set reuse=True?" % name)
            v = self.variables[name]
            assert tuple(v.shape) == shape, "variable %s has shape %s, requested %s" % (name, tuple(v.shape), shape)
            return v
        if not create:
            raise ValueError("Variable %s does not exist, or was not created with %s." % (name, self.getter))
        rs = np.random.RandomState(self.seed + len(self.variables))
        self.preset(name, kinds.initial_value(name.rsplit("/", 1)[-1], shape, rs, constant))
        return self.variables[name]


_ALPHA_STORE = VariableStore(lambda v: to_device(v))
_ALPHAS = _ALPHA_STORE.variables      # "<name>/alpha" -> device tensor (the tf.variable_scope(name) of common.py:35-39)


def prelu(x, name="prelu", shared=False):
    """relu(x) + alpha * (x - |x|) / 2 with a trainable alpha per channel (last axis), initialised to 0.01; one scalar alpha when
    `shared` (reference common.py:27-42).  The variable lives in a module-level store keyed by "<name>/alpha", created on first use."""
    x = to_device(x)
    c = x.shape[-1]
    key = name + "/alpha"
    alpha = _ALPHAS[key] if key in _ALPHAS else _ALPHA_STORE.get(key, (1 if shared else c,))
    if alpha.numel() == 1 and c > 1:
        alpha = alpha.expand(c).contiguous()
    return ops.prelu_forward(x.reshape(-1, c), alpha).reshape(x.shape)
