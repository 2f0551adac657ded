"""What the training ops share (attention.py, linear.py, layer.py, mlp.py, conv.py): the dtype table, the device check, the autocast
rule, the dropout draw state of a module and the normalisation of a dropout key, the weight-gradient output rule, and the small
helpers of the autograd functions and converters.

Dropout draw ids.  A module that drops (MultiheadSelfAttention, DeviceEncoderLayer) is a `DropoutDraws`: layer i of an encoder of L
layers gives its training-mode forward number `calls` the draw id  (calls * L + i) mod 2^32,  so no two (layer, training forward)
pairs of a run share a mask stream for 2^32 / L calls.  Each instance counts its own forwards; a forward that drops nothing does not
count.  `seed` is the run's 64-bit key, fixed from `sampling.noise_key()` (the CPU generator's state) at the first forward that drops
unless it was set; `seed` / `calls` may be set to replay a step.  Gradient checkpointing is out of scope: a re-forward advances
`calls` and would draw another mask than the forward it repeats.
"""
import torch

from . import _lib
from .sampling import noise_key

DTYPES = {torch.float32: _lib.BG_F32, torch.float16: _lib.BG_F16, torch.bfloat16: _lib.BG_BF16}
HALF = (torch.float16, torch.bfloat16)


def require_device(t, what):
    if not getattr(t, "is_cuda", False):
        raise _lib.BrepgenHipError(f"{what} runs on the MI355X only (a device tensor is required); there is no CPU fallback")


def require_devices(what, x, **named):
    """`require_device` for x under the name `what` and for every named tensor that is not None under `what (name)`"""
    require_device(x, what)
    for name, t in named.items():
        if t is not None:
            require_device(t, f"{what} ({name})")


def autocast_dtype():
    """the autocast dtype inside torch.autocast, None outside"""
    return torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None


def default_out_dtype(x):
    """the default output dtype of an op on x: the autocast dtype inside torch.autocast, x's dtype otherwise"""
    return autocast_dtype() or x.dtype


class DropoutDraws:
    """The dropout draw state of a module (module docstring).  The defaults are class attributes; an instance owns what it sets."""

    seed, calls, layer_index, n_layers, first_sample = None, 0, 0, 1, 0

    def next_draw_id(self):
        """draw_id of the next training-mode forward (advances the call counter)."""
        d = (self.calls * self.n_layers + self.layer_index) & 0xFFFFFFFF
        self.calls += 1
        return d

    def draw_key(self, drops):
        """(seed, draw_id) of this forward.  drops: whether it drops anything; if not, nothing advances and the draw id is 0."""
        if not drops:
            return self.seed or 0, 0
        if self.seed is None:
            self.seed = noise_key()
        return self.seed, self.next_draw_id()


def dropout_key(what, p, training, seed, draw_id, first_sample, B, p_name="p"):
    """(p, seed, draw_id, first_sample) as the kernels take them: p = 0 outside training, seed (default noise_key() when p > 0) and
    draw_id masked to 64 / 32 bits.  B: samples of the call, for the range of first_sample; None leaves that check to the kernel."""
    p = float(p) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{what}: {p_name} = {p} outside [0, 1)")
    if B is not None and not 0 <= int(first_sample) <= (1 << 44) - B:
        raise ValueError(f"{what}: first_sample = {first_sample}: first_sample + B must stay within 2^44")
    if seed is None:
        seed = noise_key() if p > 0.0 else 0
    return p, int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw_id) & 0xFFFFFFFF, int(first_sample)


def fp32(param):
    """detached, contiguous fp32 view (or copy) of a parameter: what the kernels read of an fp32 master or a 16-bit parameter"""
    t = param.detach()
    return (t if t.dtype == torch.float32 else t.float()).contiguous()


def workspace(nbytes, device):
    """`nbytes` of scratch for one launch (the allocator's alignment covers every kernel's), None for 0"""
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def grad_as(t, dtype):
    """a parameter gradient (or None) in the parameter's dtype"""
    return t if t is None or t.dtype == dtype else t.to(dtype)


def weight_grad(weight, dt, shape, need_w, need_b, nbytes, launch):
    """The output rule of a weight-gradient entry (bg_linear_wgrad, bg_conv_wgrad): dw of `shape` and db [shape[0]] come out of ONE
    launch in one dtype -- fp32 for an fp32 master `weight`, otherwise the operand dtype dt -- with `nbytes` of workspace;
    launch(dw, db, out dtype code, ws, nbytes) returns the entry's status.  db is allocated only for need_b; a frozen weight with a
    trained bias gets a scratch dw.  Returns (dw or None, db or None)."""
    odt = torch.float32 if weight.dtype == torch.float32 else dt
    dw = torch.empty(shape, dtype=odt, device=weight.device)
    db = torch.empty(shape[0], dtype=odt, device=weight.device) if need_b else None
    launch(dw, db, DTYPES[odt], workspace(nbytes, weight.device), nbytes)
    return (dw if need_w else None), db


def adopt(new, old, *names):
    """`new` shares old's members `names` (Parameter objects, sub-modules) and its training flag"""
    for name in names:
        setattr(new, name, getattr(old, name))
    return new.train(old.training)


def encoder_layers(encoder, who):
    if not hasattr(encoder, "layers"):
        raise ValueError(f"{who}: an nn.TransformerEncoder (an object with .layers) is required")
    return list(encoder.layers)
