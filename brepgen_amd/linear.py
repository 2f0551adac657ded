"""nn.Linear as a differentiable op on the device: forward and data gradient on bg_gemm_ex_fwd, weight and bias gradient on
bg_linear_wgrad, the 16-bit weight copies (plain for the forward, transposed for the data gradient) from bg_weight_cast --
csrc/linear_bwd.hip.

    linear(x, weight, bias=None, split=0)     F.linear's semantics for 16-bit x, a torch.autograd.Function
    DeviceLinear(in_features, out_features)   nn.Linear's parameters and state-dict keys, forward through `linear`
    use_device_linear(encoder)                swaps it into linear1 / linear2 / self_attn.out_proj (and the in_proj of a
                                              MultiheadSelfAttention) of every layer of an nn.TransformerEncoder

The trainers run under torch.autocast with fp32 master parameters: x arrives (or is cast, as autocast would) in fp16 / bf16, the
weight is cast per call by one launch, y and dX come out in x's dtype, and dW / db are written in fp32 straight from the fp32
accumulators (torch's autocast rounds dW to 16 bits and casts it back).  An fp32 product is not provided.  LayerNorm, ReLU and
dropout are layer.py's (layer.use_device_layer); the embed MLPs of the denoisers (first Linear K = 6 / 12 / 48, output Linear
N = 3 .. 48: no multiple of 128) are mlp.py's thin products (mlp.use_device_mlps).
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._train import DTYPES, HALF, adopt, autocast_dtype, encoder_layers, fp32, grad_as, require_devices, weight_grad

TILE = 128           # bg_linear_wgrad / bg_conv_wgrad: N % 128 == 0 and K (C) % 128 == 0


def _weight_cast(lib, w, dtype, transposed):
    """16-bit copy of w [R, C] ([C, R] if transposed) in one launch"""
    R, C = w.shape
    out = torch.empty((C, R) if transposed else (R, C), dtype=dtype, device=w.device)
    _lib.check(lib.bg_weight_cast(_lib.ptr(w), DTYPES[w.dtype], R, C, None if transposed else _lib.ptr(out),
                                  _lib.ptr(out) if transposed else None, DTYPES[dtype], _lib.stream()), "bg_weight_cast")
    return out


def _gemm(lib, a, w, bias, M, N, K):
    """a [M, K] . w [N, K]^T + bias (fp32 [N] or None) -> [M, N] in a's dtype"""
    out = torch.empty(M, N, dtype=a.dtype, device=a.device)
    d = _lib.GemmDesc()
    d.a, d.lda, d.w, d.bias, d.out, d.ldc = _lib.ptr(a), K, _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), N
    d.M, d.N, d.N_pad, d.K = M, N, N, K
    d.ab_dtype = d.out_dtype = DTYPES[a.dtype]
    d.act, d.add_div, d.add2_div, d.ln_eps = _lib.BG_ACT_NONE, 1, 1, 1e-5
    _lib.check(lib.bg_gemm_ex_fwd(d, _lib.stream()), "bg_gemm_ex_fwd")
    return out


def linear_backward(x2, weight, dy, need_x, need_w, need_b, bias_dtype, split=0):
    """The backward of y = x2 weight^T + bias for x2 [M, K] 16-bit and dy [M, N] (cast to x2's dtype): (dx [M, K] in x2's dtype,
    dw [N, K], db [N]), each None unless asked for.  dw / db come out of ONE launch in one dtype -- the weight's when that is fp32
    (the trainers' masters), otherwise x2's -- and db is cast to bias_dtype.  What `linear`'s autograd op runs; conv.py's 1x1
    shortcut calls it too."""
    lib = _lib.load()
    N, K = weight.shape
    M = x2.shape[0]
    dx = dw = db = None
    with torch.autocast(device_type="cuda", enabled=False):
        dy = dy.to(x2.dtype).reshape(M, N).contiguous()
        if need_x:
            wt = _weight_cast(lib, weight, x2.dtype, True)                   # W^T [K, N]: the data gradient's w
            dx = _gemm(lib, dy, wt, None, M, K, N)
        if need_w or need_b:
            dw, db = weight_grad(weight, x2.dtype, (N, K), need_w, need_b, lib.bg_linear_wgrad_workspace_bytes(M, N, K, split),
                                 lambda dw, db, odt, ws, nbytes: _lib.check(lib.bg_linear_wgrad(
                                     _lib.ptr(dy), N, _lib.ptr(x2), K, _lib.ptr(dw), _lib.ptr(db), M, N, K, DTYPES[x2.dtype], odt, split,
                                     _lib.ptr(ws), nbytes, _lib.stream()), "bg_linear_wgrad"))
    return dx, dw, grad_as(db, bias_dtype)


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, split):
        lib = _lib.load()
        N, K = weight.shape
        x2 = x.reshape(-1, K).contiguous()
        M = x2.shape[0]
        with torch.autocast(device_type="cuda", enabled=False):
            weight = weight.contiguous()
            w16 = weight if weight.dtype == x.dtype else _weight_cast(lib, weight, x.dtype, False)
            b32 = None if bias is None else fp32(bias)
            y = _gemm(lib, x2, w16.detach(), b32, M, N, K)
        ctx.save_for_backward(x2, weight)
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.x_shape, ctx.split = x.shape, split
        return y.view(*x.shape[:-1], N)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x2, weight = ctx.saved_tensors
        dx, dw, db = linear_backward(x2, weight, dy, ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                     ctx.bias_dtype is not None and ctx.needs_input_grad[2], ctx.bias_dtype, ctx.split)
        return None if dx is None else dx.view(ctx.x_shape), dw, db, None


def linear(x, weight, bias=None, split=0):
    """y = x weight^T + bias, differentiable.  x [..., K] fp16 / bf16 on the device; weight [N, K] fp32 or x's dtype; bias [N] fp32,
    x's dtype or None; N % 128 == 0 and K % 128 == 0.  Returns [..., N] in x's dtype.  Saves x and the weight for the backward, no
    activation-sized extra.  The backward gives dX in x's dtype and dW / db in the parameter's dtype -- fp32 parameters get the fp32
    sums unrounded.  split: bg_linear_wgrad's (0 = auto).  Works inside torch.autocast (nothing here is re-cast by it); enqueues on
    the current stream, no host synchronisation in forward or backward."""
    if x.dtype not in HALF:
        raise ValueError(f"linear: x of dtype {x.dtype} (fp16 or bf16: the trainers run under autocast; an fp32 product is not provided)")
    if weight.dim() != 2 or weight.dtype not in (torch.float32, x.dtype):
        raise ValueError(f"linear: weight must be [N, K] in fp32 or {x.dtype}, got {tuple(weight.shape)} {weight.dtype}")
    N, K = weight.shape
    if N % TILE or K % TILE or N < TILE or K < TILE:
        raise ValueError(f"linear: N = {N} and K = {K} must be multiples of {TILE}")
    if x.dim() < 1 or x.shape[-1] != K or x.numel() == 0:
        raise ValueError(f"linear: x must be [..., {K}] with at least one row, got {tuple(x.shape)}")
    if bias is not None and (tuple(bias.shape) != (N,) or bias.dtype not in (torch.float32, x.dtype)):
        raise ValueError(f"linear: bias must be [{N}] in fp32 or {x.dtype}, got {tuple(bias.shape)} {bias.dtype}")
    if not 0 <= int(split) <= 64:
        raise ValueError(f"linear: split = {split} outside [0, 64]")
    require_devices("linear", x, weight=weight, bias=bias)
    return _Linear.apply(x, weight, bias, int(split))


def linear_autocast(x, weight, bias, what="DeviceLinear"):
    """`linear` after casting a non-16-bit x to the autocast dtype, as autocast would for F.linear; outside autocast such an x raises"""
    if x.dtype not in HALF:
        dt = autocast_dtype()
        if dt is None:
            raise ValueError(f"{what}: input of dtype {x.dtype} outside torch.autocast (fp16 / bf16 input, or run under autocast)")
        x = x.to(dt)
    return linear(x, weight, bias)


class DeviceLinear(nn.Linear):
    """nn.Linear with the same parameters and state-dict keys whose forward and backward run on this library (`linear`)."""

    def __init__(self, in_features, out_features, bias=True, device=None, dtype=None):
        if in_features % TILE or out_features % TILE or in_features < TILE or out_features < TILE:
            raise ValueError(f"DeviceLinear: in_features = {in_features} and out_features = {out_features} must be multiples of {TILE}")
        super().__init__(in_features, out_features, bias=bias, device=device, dtype=dtype)

    def forward(self, input):
        return linear_autocast(input, self.weight, self.bias)


def _shared(old):
    return adopt(DeviceLinear(old.in_features, old.out_features, bias=old.bias is not None, device="meta"), old, "weight", "bias")


def use_device_linear(encoder):
    """Replace `linear1`, `linear2` and `self_attn.out_proj` of every layer of an nn.TransformerEncoder by DeviceLinear modules that
    SHARE the layers' Parameter objects (state_dict keys, the optimiser's parameter list and checkpoints are unchanged), and make a
    layer's MultiheadSelfAttention (attention.use_device_attention, called BEFORE this) run its in_proj through `linear` too.  With
    torch's own nn.MultiheadAttention in a layer, only the three nn.Linear modules are swapped (torch's attention reads out_proj's
    parameters itself).  The embed MLPs and fc_out of the denoisers are not touched: their shapes are no multiples of 128.  Returns the
    encoder."""
    from .attention import MultiheadSelfAttention
    for layer in encoder_layers(encoder, "use_device_linear"):
        for holder, name in ((layer, "linear1"), (layer, "linear2"), (layer.self_attn, "out_proj")):
            old = getattr(holder, name)
            if isinstance(old, DeviceLinear):
                continue
            if not isinstance(old, nn.Linear):
                raise ValueError(f"use_device_linear: {name} is a {type(old).__name__}, not an nn.Linear")
            setattr(holder, name, _shared(old))
        if isinstance(layer.self_attn, MultiheadSelfAttention):
            layer.self_attn.device_linear = True
    return encoder
