"""The denoisers' MLPs as differentiable ops on the device: nn.Sequential(Linear(k, 768), LayerNorm, SiLU, Linear(768, n)) -- the data
embeds (k = 6 / 12 / 48), time_embed (k = 768) and fc_out (n = 6 / 18 / 48) of SurfPosNet / SurfZNet / EdgePosNet / EdgeZNet
(network.py:1076-1099) -- csrc/mlp_train.hip behind bg_thin_expand / bg_thin_contract / bg_thin_wgrad / bg_ln_silu_train_fwd /
bg_ln_silu_bwd.

    thin_linear_in(x, weight, bias, out_dtype)     F.linear for in_features <= 48; x may be a column slice of wider rows
    thin_linear_out(a, weight, bias)               F.linear for out_features <= 48 and 16-bit a -> fp32
    ln_silu(x, weight, bias, eps, out_dtype)       SiLU(LayerNorm(x)) over 768 columns in one pass per direction
    DeviceMLP(mlp)                                 the four children of such a Sequential under their names, composed from the ops above
                                                   and linear.linear
    use_device_mlps(model)                         swaps it in for every such direct child of a denoiser

With training.use_device_training and training.mse_loss a training iteration of a reference-keyed denoiser leaves this library only for
what is NOT in scope here: the adds between the embeds, the `repeat` over edges, the class embedding and the sincos table (torch
autograd), fusing LN + SiLU into the thin contract (two launches), and the VAE trainers' backward.

The trainers run under torch.autocast with fp32 master parameters, and so do these ops: the thin weights must be fp32, the [M, 768]
activations between the Linears are 16-bit, dW / db come out in fp32 straight from the fp32 / fp64 sums.  Nothing synchronises.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._train import DTYPES, HALF, autocast_dtype, default_out_dtype, fp32, require_device, require_devices, workspace
from .layer import D_MODEL, row_layer_norm
from .linear import TILE, linear, linear_autocast

THIN = 48


def _rows2d(x, what):
    """(tensor, M, row stride): x [..., s] as M rows of a fixed stride, in place where the leading dimensions collapse, else a copy"""
    s = x.shape[-1]
    M = x.numel() // s if s else 0
    if x.stride(-1) != 1 and s > 1:
        x = x.contiguous()
    if x.dim() == 1:
        return x, M, s
    ld = x.stride(-2)
    ok = ld >= s
    for i in range(x.dim() - 2):
        ok = ok and (x.shape[i] == 1 or x.stride(i) == x.stride(i + 1) * x.shape[i + 1])
    if not ok or M <= 1:
        x = x.contiguous()
        ld = s
    return x, M, ld


def _thin_weight(what, weight, bias, thin_dim):
    """checks of a Linear with one side <= 48 and the other 768; thin_dim: the index of the thin side in weight.shape"""
    if weight.dim() != 2 or weight.dtype != torch.float32:
        raise ValueError(f"{what}: weight must be a 2-D fp32 master parameter, got {tuple(weight.shape)} {weight.dtype}")
    if not 1 <= weight.shape[thin_dim] <= THIN or weight.shape[1 - thin_dim] != D_MODEL:
        want = f"[{D_MODEL}, 1 .. {THIN}]" if thin_dim == 1 else f"[1 .. {THIN}, {D_MODEL}]"
        raise ValueError(f"{what}: weight must be {want}, got {tuple(weight.shape)}")
    if bias is not None and (tuple(bias.shape) != (weight.shape[0],) or bias.dtype != torch.float32):
        raise ValueError(f"{what}: bias must be fp32 [{weight.shape[0]}], got {tuple(bias.shape)} {bias.dtype}")


def _expand(lib, x, M, ldx, w, k_major, bias, out_dtype, s):
    y = torch.empty(M, D_MODEL, dtype=out_dtype, device=x.device)
    _lib.check(lib.bg_thin_expand(x.data_ptr(), DTYPES[x.dtype], ldx, _lib.ptr(w), int(k_major), _lib.ptr(bias), _lib.ptr(y), DTYPES[out_dtype],
                                  M, s, _lib.stream()), "bg_thin_expand")
    return y


def _wgrad(lib, t, M, ldt, u, transposed, colsum_of, s):
    """(g, colsum): g = t^T u as [s, 768] or [768, s]; colsum of u [768] (1), of t [s] (2) or None (0)"""
    g = torch.empty((D_MODEL, s) if transposed else (s, D_MODEL), dtype=torch.float32, device=u.device)
    cs = torch.empty(D_MODEL if colsum_of == 1 else s, dtype=torch.float32, device=u.device) if colsum_of else None
    nbytes = lib.bg_thin_wgrad_workspace_bytes(M, s)
    ws = workspace(nbytes, u.device)
    _lib.check(lib.bg_thin_wgrad(t.data_ptr(), DTYPES[t.dtype], ldt, _lib.ptr(u), DTYPES[u.dtype], _lib.ptr(g), int(transposed), _lib.ptr(cs),
                                 colsum_of, M, s, _lib.ptr(ws), nbytes, _lib.stream()), "bg_thin_wgrad")
    return g, cs


class _ThinIn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, out_dtype):
        lib = _lib.load()
        s = weight.shape[1]
        x2, M, ldx = _rows2d(x, "thin_linear_in")
        y = _expand(lib, x2, M, ldx, weight.detach().contiguous(), False, None if bias is None else fp32(bias), out_dtype, s)
        ctx.save_for_backward(x2)
        ctx.dims, ctx.has_bias = (M, ldx, s), bias is not None
        return y.view(*x.shape[:-1], D_MODEL)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x2, = ctx.saved_tensors
        M, ldx, s = ctx.dims
        need_w, need_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        if not (need_w or need_b):
            return None, None, None, None
        dy = dy.reshape(M, D_MODEL).contiguous()                  # 16-bit: the forward's out_dtype (thin_linear_in checks it)
        dw, db = _wgrad(_lib.load(), x2, M, ldx, dy, True, 1 if need_b else 0, s)
        return None, (dw if need_w else None), db, None


def thin_linear_in(x, weight, bias=None, out_dtype=None):
    """y = x weight^T + bias for in_features <= 48 and out_features = 768, differentiable in weight and bias.  x [..., s] fp32 / fp16 /
    bf16 on the device, any strided view whose last dimension is contiguous (edge[..., :12] of 18-wide rows is read in place where
    the leading dimensions collapse to one row stride); weight fp32 [768, s], bias fp32 [768] or None.  out_dtype: default = the
    autocast dtype inside torch.autocast, x's dtype otherwise.  Returns [..., 768].  dW [768, s] and db come back in fp32 from one
    launch (bg_thin_wgrad); that launch takes a 16-bit dY, so parameters that require a gradient need a 16-bit out_dtype.  The
    denoisers' inputs never need a gradient: an x that requires one raises ValueError."""
    what = "thin_linear_in"
    if x.requires_grad:
        raise ValueError(f"{what}: x requires a gradient; the data gradient of an embed's first Linear is not provided")
    if x.dtype not in DTYPES or x.dim() < 1:
        raise ValueError(f"{what}: x must be [..., s] in fp32, fp16 or bf16, got {tuple(x.shape)} {x.dtype}")
    _thin_weight(what, weight, bias, 1)
    if x.shape[-1] != weight.shape[1] or x.numel() == 0:
        raise ValueError(f"{what}: x must be [..., {weight.shape[1]}] with at least one row, got {tuple(x.shape)}")
    if out_dtype is None:
        out_dtype = default_out_dtype(x)
    if out_dtype not in DTYPES:
        raise ValueError(f"{what}: out_dtype {out_dtype} (fp32, fp16 or bf16)")
    trains = torch.is_grad_enabled() and (weight.requires_grad or (bias is not None and bias.requires_grad))
    if trains and out_dtype not in HALF:
        raise ValueError(f"{what}: the weight gradient takes a 16-bit dY: run under torch.autocast or pass a 16-bit out_dtype (got {out_dtype})")
    require_devices(what, x, weight=weight, bias=bias)
    return _ThinIn.apply(x, weight, bias, out_dtype)


class _ThinOut(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, weight, bias):
        lib = _lib.load()
        n = weight.shape[0]
        a2 = a.reshape(-1, D_MODEL).contiguous()
        M = a2.shape[0]
        w = weight.detach().contiguous()
        y = torch.empty(M, n, dtype=torch.float32, device=a.device)
        _lib.check(lib.bg_thin_contract(_lib.ptr(a2), DTYPES[a2.dtype], _lib.ptr(w), _lib.ptr(None if bias is None else fp32(bias)), _lib.ptr(y), M, n,
                                        _lib.stream()), "bg_thin_contract")
        ctx.save_for_backward(a2, weight)
        ctx.a_shape, ctx.has_bias = a.shape, bias is not None
        return y.view(*a.shape[:-1], n)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        a2, weight = ctx.saved_tensors
        lib = _lib.load()
        M, n = a2.shape[0], weight.shape[0]
        need_a, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dy = dy.float().reshape(M, n).contiguous()
        da = dw = db = None
        if need_a:                                                # dA = dY W: the thin expansion with W [n, 768] taken k-major
            da = _expand(lib, dy, M, n, weight.detach().contiguous(), True, None, a2.dtype, n).view(ctx.a_shape)
        if need_w or need_b:
            dw, db = _wgrad(lib, dy, M, n, a2, False, 2 if need_b else 0, n)
        return da, (dw if need_w else None), db


def thin_linear_out(a, weight, bias=None):
    """y = a weight^T + bias for in_features = 768 and out_features <= 48, differentiable.  a [..., 768] fp16 / bf16 on the device;
    weight fp32 [n, 768] (read as fp32: no 16-bit copy), bias fp32 [n] or None.  Returns fp32 [..., n].  The backward gives dA in a's
    dtype (bg_thin_expand) and dW / db in fp32 from one launch (bg_thin_wgrad)."""
    what = "thin_linear_out"
    if a.dtype not in HALF:
        raise ValueError(f"{what}: a of dtype {a.dtype} (fp16 or bf16: the trainers run under autocast)")
    _thin_weight(what, weight, bias, 0)
    if a.dim() < 1 or a.shape[-1] != D_MODEL or a.numel() == 0:
        raise ValueError(f"{what}: a must be [..., {D_MODEL}] with at least one row, got {tuple(a.shape)}")
    require_devices(what, a, weight=weight, bias=bias)
    return _ThinOut.apply(a, weight, bias)


def ln_silu(x, weight, bias, eps=1e-5, out_dtype=None):
    """SiLU(LayerNorm(x)) over the last dimension (768), differentiable, one launch per direction (two with dgamma / dbeta).  The rules
    for dtypes and autocast are layer.layer_norm's: x [..., 768] fp32 / fp16 / bf16; out_dtype default = the autocast dtype inside
    torch.autocast (what the next Linear's cast would make of torch's fp32 result, rounded once), x's dtype otherwise; a 16-bit x
    gives its own dtype or fp32.  Saves x and the rows' (mean, rstd); the backward recomputes LayerNorm(x)."""
    return row_layer_norm("ln_silu", x, weight, bias, eps, out_dtype, False, True)


def _fits(mlp):
    """None if `mlp` is not a Linear-LayerNorm-SiLU-Linear Sequential at all, else a string saying why it does not fit ('' = it fits)"""
    if not isinstance(mlp, nn.Sequential) or len(mlp) != 4:
        return None
    l0, ln, act, l3 = mlp[0], mlp[1], mlp[2], mlp[3]
    if not (isinstance(l0, nn.Linear) and isinstance(ln, nn.LayerNorm) and isinstance(act, nn.SiLU) and isinstance(l3, nn.Linear)):
        return None
    if tuple(ln.normalized_shape) != (D_MODEL,) or ln.weight is None or ln.bias is None:
        return f"its LayerNorm must be affine LayerNorm({D_MODEL}) with bias"
    if l0.out_features != D_MODEL or l3.in_features != D_MODEL:
        return f"its hidden width must be {D_MODEL}, got {l0.out_features} and {l3.in_features}"
    for side, v in (("in_features", l0.in_features), ("out_features", l3.out_features)):
        if not (1 <= v <= THIN or (v >= TILE and v % TILE == 0)):
            return f"{side} = {v} is neither 1 .. {THIN} nor a multiple of {TILE}"
    return ""


class DeviceMLP(nn.Sequential):
    """nn.Sequential(Linear(k, 768), LayerNorm(768), SiLU, Linear(768, n)) holding the SAME four children under the names 0 1 2 3
    (state-dict keys and Parameter objects are unchanged) whose forward and backward run on this library:
        thin_linear_in (k <= 48) or linear.linear_autocast (k a multiple of 128: time_embed)  ->  ln_silu  ->
        thin_linear_out (n <= 48) or linear.linear (n a multiple of 128)
    Runs under torch.autocast, like DeviceLinear; the output dtype is what autocast's last nn.Linear would hand the caller (the
    autocast dtype), outside autocast thin_linear_out's fp32."""

    def __init__(self, mlp):
        why = _fits(mlp)
        if why is None or why:
            raise ValueError(f"DeviceMLP: an nn.Sequential(Linear, LayerNorm({D_MODEL}), SiLU, Linear) is required" + (f": {why}" if why else ""))
        super().__init__()
        for i in range(4):
            self.add_module(str(i), mlp[i])
        self.train(mlp.training)

    def forward(self, input):
        l0, ln, l3 = self[0], self[1], self[3]
        require_device(input, "DeviceMLP")
        if l0.in_features <= THIN:
            h = thin_linear_in(input, l0.weight, l0.bias)
        else:
            h = linear_autocast(input, l0.weight, l0.bias, "DeviceMLP")
        h = ln_silu(h, ln.weight, ln.bias, ln.eps)
        if h.dtype not in HALF:
            raise ValueError(f"DeviceMLP: hidden activations of dtype {h.dtype} outside torch.autocast (fp16 / bf16 input, or run under autocast)")
        if l3.out_features > THIN:
            return linear(h, l3.weight, l3.bias)
        y = thin_linear_out(h, l3.weight, l3.bias)
        dt = autocast_dtype()
        return y if dt is None else y.to(dt)


def use_device_mlps(model):
    """Make every direct child of `model` that is an nn.Sequential(Linear, LayerNorm(768), SiLU, Linear) a DeviceMLP: the embeds,
    time_embed and fc_out of a reference-keyed denoiser (3 / 4 / 5 / 7 children for SurfPosNet / SurfZNet / EdgePosNet / EdgeZNet).
    Parameter objects, state_dict keys, the optimiser's parameter list and checkpoints are unchanged.  A child that is such a
    Sequential but does not fit (another width, a LayerNorm without affine parameters) raises ValueError before anything is
    converted.  Launches nothing.  Returns the model."""
    found = []
    for name, child in model.named_children():
        if isinstance(child, DeviceMLP):
            continue
        why = _fits(child)
        if why:
            raise ValueError(f"use_device_mlps: {name} looks like an embed MLP but does not fit: {why}")
        if why == "":
            found.append((name, child))
    for name, child in found:
        setattr(model, name, DeviceMLP(child))
    return model
