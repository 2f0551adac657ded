"""The VAEs' ResnetBlock2D in TRAINING: GroupNorm + SiLU + 3x3 convolution as differentiable ops on the device -- csrc/conv_train.hip
for the backward (bg_conv_wgrad, bg_conv_weight_pack, bg_gn_act_bwd), the VAE forward entries (bg_groupnorm_stats, bg_im2col,
bg_conv_gemm_fwd / bg_gemm_bias_act_fwd) for the forward and the data gradient.

    gn_act_conv(x, norm, conv, act="silu", res=None)    y = conv(act(GroupNorm(x))) + bias (+ res), a torch.autograd.Function
    DeviceResnetBlock2D(cin, cout, groups=32, eps=1e-6) diffusers' ResnetBlock2D (no time embedding, dropout 0, output scale 1) with its
                                                        parameter names; forward and backward as ONE autograd node
    use_device_resnets(module)                          swaps it in for every child with exactly that parameter structure
    conv_down(x, conv) / conv_up(x, conv)               diffusers' Downsample2D / Upsample2D convolutions (pad after + stride 2 | nearest x2 +
                                                        'same'), torch.autograd.Functions: bg_conv_wgrad_geom, bg_conv_down_dgrad /
                                                        bg_conv_weight_pack_down, bg_pool2x2_sum for the backward
    DeviceDownsample2D(c) / DeviceUpsample2D(c)         the two modules, parameter name `conv`
    DeviceBlock2D(resnets, downsamplers, upsamplers)    a DownEncoderBlock2D / UpDecoderBlock2D: the resnets, then the sampler
    use_device_blocks(module)                           use_device_resnets + the samplers + the blocks around them

Layout.  Everything here takes and returns CHANNELS-LAST fp32 activations: a dense [S, H, W, C] tensor (1-D: [S, L, C]), which is
`x.permute(0, 2, 3, 1).contiguous()` of torch's [S, C, H, W] -- not a torch memory format of a 4-D NCHW tensor.  A module converted by
use_device_resnets therefore has to be fed, and returns, that layout.

The trainers run under torch.autocast with fp32 master parameters: the normalised, activated input is rounded ONCE to fp16 / bf16, the
weights are cast per call by one launch (bg_conv_weight_pack), products accumulate in fp32, y / dx come out in fp32 and the parameter
gradients in fp32 straight from the fp32 sums.  Calls outside autocast, CPU tensors, strides other than 1, grids that are no powers
of two and channel counts the kernels do not take raise; nothing falls back to torch.

Not here (the rest of the VAE backward): conv_in / conv_out, the mid-block attention, the 1-D ResConvBlock composition and cubic
resamplers, the posterior's backward, a whole-VAE training step.  Nor is nearest x2 + 3x3 folded into four 2x2 class convolutions
with summed weights (16 instead of 36 tap-products per low-resolution pixel): that changes the rounding of a forward that inference
and the goldens share.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._train import DTYPES, HALF, adopt, autocast_dtype, fp32, grad_as, require_device, weight_grad, workspace
from .linear import TILE, linear, linear_backward

ACTS = {"none": 0, "silu": 1, "gelu": 2}         # bg_vae_act
_ZERO = {}


def _zero_page(device):
    """one pixel of zeros for bg_conv_gemm_fwd's padded taps (>= 2 * C bytes for any C <= 32768)"""
    if device not in _ZERO:
        _ZERO[device] = torch.zeros(1 << 16, dtype=torch.uint8, device=device)
    return _ZERO[device]


def _pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def _implicit_ok(S, H, W, C, N, taps):
    """would bg_conv_gemm_fwd take this convolution?  (vae_exec.hip's conv_implicit_ok: its argument checks + the >= 64 tiles rule)"""
    rows = S * H * W
    return taps > 1 and C % 64 == 0 and _pow2(C // 64) and N % 128 == 0 and rows < 1 << 31 and (rows + 127) // 128 * (N // 128) >= 64


def _norm_act_cast(lib, x, S, H, W, C, dt, gn=None, act=0):
    """act(GroupNorm(x)) (or x itself) rounded to `dt`: [S*H*W, C].  gn = (stats, gamma, beta, G)"""
    out = torch.empty(S * H * W, C, dtype=dt, device=x.device)
    st, ga, be, G = gn if gn is not None else (None, None, None, 1)
    _lib.check(lib.bg_im2col(_lib.ptr(x), _lib.ptr(out), DTYPES[dt], S, H, W, C, 1, 1, 0, 1, 0, 0, H, W, _lib.ptr(st), _lib.ptr(ga),
                             _lib.ptr(be), G, act, None, _lib.stream()), "bg_im2col")
    return out


def _conv_same(lib, src32, src16, S, H, W, C, kh, kw, w16, N, bias, res, gn=None, act=0):
    """'same' stride-1 convolution of the channels-last [S, H, W, C] activations with the packed weight w16 [N, kh*kw*C] -> fp32
    [S*H*W, N] (+ bias, + res).  src16: the 16-bit operand (already normalised / activated); src32: its fp32 source, which the
    materialised-im2col path gathers (and normalises with gn / act) itself.  The implicit GEMM where its 64-tile rule holds,
    else im2col + GEMM: vae_exec.hip's choice."""
    dt, dev = src16.dtype, src16.device
    M, K = S * H * W, kh * kw * C
    out = torch.empty(M, N, dtype=torch.float32, device=dev)
    if _implicit_ok(S, H, W, C, N, kh * kw):
        d = _lib.ConvDesc()
        d.x, d.S, d.H, d.W, d.C = _lib.ptr(src16), S, H, W, C
        d.kh, d.kw, d.up = kh, kw, 0
        d.w, d.bias, d.N = _lib.ptr(w16), _lib.ptr(bias), N
        d.out, d.ldc = _lib.ptr(out), N
        d.add, d.ld_add = _lib.ptr(res), N
        d.dtype, d.zero_page = DTYPES[dt], _lib.ptr(_zero_page(dev))
        _lib.check(lib.bg_conv_gemm_fwd(d, _lib.stream()), "bg_conv_gemm_fwd")
        return out
    if kh * kw > 1:
        col = torch.empty(M, K, dtype=dt, device=dev)
        st, ga, be, G = gn if gn is not None else (None, None, None, 1)
        _lib.check(lib.bg_im2col(_lib.ptr(src32), _lib.ptr(col), DTYPES[dt], S, H, W, C, kh, kw, 0, 1, kh // 2, kw // 2, H, W, _lib.ptr(st),
                                 _lib.ptr(ga), _lib.ptr(be), G, act, None, _lib.stream()), "bg_im2col")
    else:
        col = src16
    _lib.check(lib.bg_gemm_bias_act_fwd(_lib.ptr(col), K, _lib.ptr(w16), _lib.ptr(bias), _lib.ptr(out), N, M, N, N, K, DTYPES[dt],
                                        _lib.BG_F32, _lib.BG_ACT_NONE, _lib.ptr(res), N if res is not None else 0, 1, _lib.stream()),
               "bg_gemm_bias_act_fwd")
    return out


def _pack(lib, weight, kh, kw, dt, fwd):
    """the forward pack [N, kh*kw*C] (fwd) or the data-gradient pack [C, kh*kw*N] of a conv weight [N, C, kh, kw] / [N, C, kw]"""
    N, C = weight.shape[:2]
    w = weight.detach().contiguous()
    out = torch.empty((N, kh * kw * C) if fwd else (C, kh * kw * N), dtype=dt, device=w.device)
    _lib.check(lib.bg_conv_weight_pack(_lib.ptr(w), DTYPES[w.dtype], N, C, kh, kw, _lib.ptr(out) if fwd else None,
                                       None if fwd else _lib.ptr(out), DTYPES[dt], _lib.stream()), "bg_conv_weight_pack")
    return out


class _Layer:
    """What one y = conv(act(GroupNorm(x))) + bias (+ res) keeps between forward and backward: x (fp32), the 16-bit a = act(GN(x)),
    the statistics, and the parameters."""

    def forward(self, x, S, H, W, gamma, beta, G, eps, act, weight, bias, res, dt):
        lib = _lib.load()
        self.S, self.H, self.W, self.dt, self.act, self.G = S, H, W, dt, act, G
        self.N, self.C = weight.shape[:2]
        self.kh, self.kw = (1, weight.shape[2]) if weight.dim() == 3 else tuple(weight.shape[2:])
        self.x, self.weight, self.gn = x, weight, None
        if gamma is not None:
            stats = torch.empty(S, G, 2, dtype=torch.float32, device=x.device)
            _lib.check(lib.bg_groupnorm_stats(_lib.ptr(x), _lib.ptr(stats), S, H * W, self.C, G, eps, _lib.stream()), "bg_groupnorm_stats")
            self.gn = (stats, fp32(gamma), fp32(beta), G)
        self.a = _norm_act_cast(lib, x, S, H, W, self.C, dt, self.gn, act if self.gn else 0)
        w16 = _pack(lib, weight, self.kh, self.kw, dt, True)
        return _conv_same(lib, x, self.a, S, H, W, self.C, self.kh, self.kw, w16, self.N, None if bias is None else fp32(bias), res, self.gn,
                          act if self.gn else 0)

    def backward(self, dy, need_x, need_gn, need_w, need_b, dskip=None, dy16=None):
        """dy fp32 [S*H*W, N] -> (dx fp32 [S*H*W, C] (+ dskip), dgamma, dbeta, dw in the weight's layout, db, dy16)"""
        lib = _lib.load()
        S, H, W, N, C, kh, kw, dt = self.S, self.H, self.W, self.N, self.C, self.kh, self.kw, self.dt
        dev = dy.device
        if dy16 is None:
            dy16 = _norm_act_cast(lib, dy, S, H, W, N, dt)
        dx = dgamma = dbeta = dw = db = None
        if need_w or need_b:
            dwp, db = weight_grad(self.weight, dt, (N, kh * kw * C), need_w, need_b, lib.bg_conv_wgrad_workspace_bytes(S, H, W, N, C, kh, kw, 0),
                                  lambda dwp, db, odt, ws, nbytes: _lib.check(lib.bg_conv_wgrad(
                                      _lib.ptr(dy16), N, _lib.ptr(self.a), C, _lib.ptr(dwp), _lib.ptr(db), S, H, W, N, C, kh, kw, DTYPES[dt], odt, 0,
                                      _lib.ptr(ws), nbytes, _lib.stream()), "bg_conv_wgrad"))
            if need_w:                                     # tap-major [N, kh, kw, C] -> the parameter's [N, C, kh, kw] / [N, C, kw]
                dw = (dwp.view(N, kw, C).permute(0, 2, 1) if self.weight.dim() == 3 else dwp.view(N, kh, kw, C).permute(0, 3, 1, 2)).contiguous()
        if need_x or (need_gn and self.gn):
            wd = _pack(lib, self.weight, kh, kw, dt, False)
            da = _conv_same(lib, dy, dy16, S, H, W, N, kh, kw, wd, C, None, None)
            if self.gn:
                stats, ga, be, G = self.gn
                dx = torch.empty(S * H * W, C, dtype=torch.float32, device=dev)
                if need_gn:
                    dgamma, dbeta = torch.empty(C, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
                nbytes = lib.bg_gn_act_bwd_workspace_bytes(S, H * W, C, G)
                ws = workspace(nbytes, dev)
                _lib.check(lib.bg_gn_act_bwd(_lib.ptr(da), _lib.ptr(self.x), _lib.ptr(stats), _lib.ptr(ga), _lib.ptr(be), _lib.ptr(dskip),
                                             _lib.ptr(dx), _lib.ptr(dgamma), _lib.ptr(dbeta), S, H * W, C, G, self.act, _lib.ptr(ws), nbytes,
                                             _lib.stream()), "bg_gn_act_bwd")
            else:
                dx = da if dskip is None else da + dskip
        return dx, dgamma, dbeta, dw, db, dy16


class _GnActConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, weight, bias, res, G, eps, act, dt):
        S, H, W = (x.shape[0], 1, x.shape[1]) if x.dim() == 3 else x.shape[:3]
        with torch.autocast(device_type="cuda", enabled=False):
            L = _Layer()
            y = L.forward(x.contiguous(), S, H, W, gamma, beta, G, eps, act, weight, bias,
                          None if res is None else res.contiguous(), dt)
        ctx.layer, ctx.params = L, (gamma, beta, weight, bias)
        return y.view(*x.shape[:-1], L.N)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        L = ctx.layer
        gamma, beta, weight, bias = ctx.params
        need = ctx.needs_input_grad
        with torch.autocast(device_type="cuda", enabled=False):
            dy = dy.float().contiguous()
            dx, dgamma, dbeta, dw, db, _ = L.backward(dy.view(-1, L.N), need[0], need[1] or need[2], need[3], bias is not None and need[4])
        dx = None if dx is None or not need[0] else dx.view(L.x.shape)
        return (dx, grad_as(dgamma, gamma.dtype) if need[1] else None, grad_as(dbeta, beta.dtype) if need[2] else None,
                grad_as(dw, weight.dtype), grad_as(db, bias.dtype) if bias is not None else None, dy if need[5] else None, None, None, None, None)


def _autocast_dtype(what):
    dt = autocast_dtype()
    if dt is None:
        raise ValueError(f"{what}: called outside torch.autocast (the trainers run under fp16 / bf16 autocast; an fp32 product is not provided)")
    if dt not in HALF:
        raise ValueError(f"{what}: autocast dtype {dt} (fp16 or bf16)")
    return dt


def _check_input(x, what):
    if x.dtype != torch.float32 or x.dim() not in (3, 4) or x.numel() == 0:
        raise ValueError(f"{what}: x must be fp32 channels-last [S, H, W, C] or [S, L, C], got {tuple(x.shape)} {x.dtype}")
    H, W = (1, x.shape[1]) if x.dim() == 3 else x.shape[1:3]
    if not (_pow2(H) and _pow2(W)):
        raise ValueError(f"{what}: the grid {H} x {W} must be powers of two")


def _check_conv(conv, dims, what):
    kind = nn.Conv1d if dims == 1 else nn.Conv2d
    if not isinstance(conv, kind):
        raise ValueError(f"{what}: a {kind.__name__} is required for a {dims}-D input, got {type(conv).__name__}")
    k, one, zero = tuple(conv.kernel_size), (1,) * dims, (0,) * dims
    if tuple(conv.stride) != one or tuple(conv.dilation) != one or conv.groups != 1 or conv.padding_mode != "zeros":
        raise ValueError(f"{what}: stride {tuple(conv.stride)}, dilation {tuple(conv.dilation)}, groups {conv.groups} (stride 1, no dilation, one group)")
    if any(v % 2 == 0 or v > 5 for v in k) or conv.padding not in ("same", tuple(v // 2 for v in k)) or tuple(conv.output_padding) != zero:
        raise ValueError(f"{what}: window {k} with padding {conv.padding} (odd, at most 5, 'same' zero padding)")
    N, C = conv.out_channels, conv.in_channels
    if N % TILE or C % TILE:
        raise ValueError(f"{what}: in_channels = {C} and out_channels = {N} must be multiples of {TILE}")
    if conv.weight.dtype not in (torch.float32,) + HALF:
        raise ValueError(f"{what}: weight dtype {conv.weight.dtype}")


def _check_norm(norm, C, what):
    if not isinstance(norm, nn.GroupNorm) or not norm.affine:
        raise ValueError(f"{what}: norm must be an affine nn.GroupNorm or None, got {type(norm).__name__}")
    if norm.num_channels != C or (C // norm.num_groups) % 4:
        raise ValueError(f"{what}: GroupNorm({norm.num_groups}, {norm.num_channels}) on {C} channels (channels per group: a multiple of 4)")


def gn_act_conv(x, norm, conv, act="silu", res=None):
    """y = conv(act(GroupNorm(x))) + bias (+ res), differentiable.  x: fp32 channels-last [S, H, W, Cin] ([S, L, Cin] with an
    nn.Conv1d) on the device, H and W powers of two; norm: an nn.GroupNorm, or None for a plain convolution (`act` is then not
    applied); conv: an nn.Conv2d / nn.Conv1d with stride 1, 'same' zero padding, an odd window of at most 5 per side, Cin and Cout
    multiples of 128; act: "silu", "gelu" (erf) or "none"; res: fp32 [S, H, W, Cout], added in the GEMM's epilogue.  Returns fp32
    channels-last [S, H, W, Cout].  Must run under fp16 / bf16 torch.autocast; anything outside these rules raises.

    Saves for the backward: x (fp32), the 16-bit a = act(GroupNorm(x)) and the statistics -- 2 + 4 bytes per activation element
    per convolution.  The backward gives dx (fp32), dgamma, dbeta, dW (in the parameter's [Cout, Cin, kh, kw] layout) and db -- fp32
    for fp32 master parameters, unrounded from the fp32 sums -- and dres = dy.  Enqueues on the current stream, no host
    synchronisation."""
    what = "gn_act_conv"
    _check_input(x, what)
    _check_conv(conv, x.dim() - 2, what)
    if x.shape[-1] != conv.in_channels:
        raise ValueError(f"{what}: x has {x.shape[-1]} channels, the convolution takes {conv.in_channels}")
    if act not in ACTS:
        raise ValueError(f"{what}: act = {act!r} (one of {sorted(ACTS)})")
    if norm is not None:
        _check_norm(norm, x.shape[-1], what)
    if res is not None and (res.dtype != torch.float32 or tuple(res.shape) != (*x.shape[:-1], conv.out_channels)):
        raise ValueError(f"{what}: res must be fp32 {(*x.shape[:-1], conv.out_channels)}, got {tuple(res.shape)} {res.dtype}")
    for t in (x, conv.weight, conv.bias, res) + ((norm.weight, norm.bias) if norm is not None else ()):
        if t is not None:
            require_device(t, what)
    dt = _autocast_dtype(what)
    gamma, beta, G, eps = (norm.weight, norm.bias, norm.num_groups, norm.eps) if norm is not None else (None, None, 1, 0.0)
    return _GnActConv.apply(x, gamma, beta, conv.weight, conv.bias, res, G, float(eps), ACTS[act], dt)


class _Resnet(torch.autograd.Function):
    """out = conv2(silu(norm2(conv1(silu(norm1(x)))))) + shortcut(x) as one node, so that the shortcut's gradient enters
    norm1's backward through dskip instead of a separate add."""

    @staticmethod
    def forward(ctx, x, dt, g1, b1, w1, c1, g2, b2, w2, c2, ws, cs, G, eps):
        S, H, W, C = x.shape
        with torch.autocast(device_type="cuda", enabled=False):
            x = x.contiguous()
            L1, L2 = _Layer(), _Layer()
            h = L1.forward(x, S, H, W, g1, b1, G, eps, ACTS["silu"], w1, c1, None, dt)
            N = L1.N
            sc = x.view(-1, C)
            if ws is not None:
                x16 = _norm_act_cast(_lib.load(), x, S, H, W, C, dt)
                sc = linear(x16, ws.view(N, C), cs).float()
            out = L2.forward(h, S, H, W, g2, b2, G, eps, ACTS["silu"], w2, c2, sc, dt)
        ctx.layers, ctx.params, ctx.dt = (L1, L2), (g1, b1, w1, c1, g2, b2, w2, c2, ws, cs), dt
        return out.view(S, H, W, N)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        L1, L2 = ctx.layers
        g1, b1, w1, c1, g2, b2, w2, c2, ws, cs = ctx.params
        need = ctx.needs_input_grad
        S, H, W, C, N = L1.S, L1.H, L1.W, L1.C, L1.N
        with torch.autocast(device_type="cuda", enabled=False):
            dy = dy.float().contiguous().view(-1, N)
            dh, dg2, db2, dw2, dc2, dy16 = L2.backward(dy, True, need[6] or need[7], need[8], need[9])
            dskip, dws, dcs = dy, None, None
            if ws is not None:
                x16 = _norm_act_cast(_lib.load(), L1.x, S, H, W, C, ctx.dt)
                dsc, dws, dcs = linear_backward(x16, ws.view(N, C), dy16, need[0], need[10], cs is not None and need[11],
                                                None if cs is None else cs.dtype)
                dskip = None if dsc is None else dsc.float()
                dws = None if dws is None else dws.view(ws.shape)
            dx, dg1, db1, dw1, dc1, _ = L1.backward(dh, need[0], need[2] or need[3], need[4], need[5], dskip=dskip if need[0] else None)
        grads = [dx.view(S, H, W, C) if need[0] else None, None]
        for g, p, n in ((dg1, g1, 2), (db1, b1, 3), (dw1, w1, 4), (dc1, c1, 5), (dg2, g2, 6), (db2, b2, 7), (dw2, w2, 8), (dc2, c2, 9),
                        (dws, ws, 10), (dcs, cs, 11)):
            grads.append(grad_as(g, p.dtype) if p is not None and need[n] else None)
        return (*grads, None, None)


class DeviceResnetBlock2D(nn.Module):
    """diffusers' ResnetBlock2D without a time embedding, with dropout 0 and output scale 1 -- the VAEs' block -- on the device, forward
    and backward: parameter names norm1, conv1, norm2, conv2 and, for cin != cout, conv_shortcut (a 1x1 nn.Conv2d, run by
    brepgen_amd.linear's kernels).  forward(x): fp32 CHANNELS-LAST [S, H, W, cin] -> [S, H, W, cout] (module docstring), under
    fp16 / bf16 autocast; H, W powers of two, cin and cout multiples of 128.  The whole block is one autograd node: the shortcut's
    gradient is merged into norm1's backward pass (bg_gn_act_bwd's dskip)."""

    def __init__(self, cin, cout, groups=32, eps=1e-6, device=None, dtype=None):
        super().__init__()
        if cin % TILE or cout % TILE or cin < TILE or cout < TILE:
            raise ValueError(f"DeviceResnetBlock2D: cin = {cin} and cout = {cout} must be multiples of {TILE}")
        kw = {"device": device, "dtype": dtype}
        self.norm1 = nn.GroupNorm(groups, cin, eps=eps, **kw)
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1, **kw)
        self.norm2 = nn.GroupNorm(groups, cout, eps=eps, **kw)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1, **kw)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1, **kw)

    def forward(self, x):
        what = "DeviceResnetBlock2D"
        _check_input(x, what)
        if x.dim() != 4 or x.shape[-1] != self.conv1.in_channels:
            raise ValueError(f"{what}: x must be channels-last [S, H, W, {self.conv1.in_channels}], got {tuple(x.shape)}")
        sc = getattr(self, "conv_shortcut", None)
        for conv in (self.conv1, self.conv2) + (() if sc is None else (sc,)):
            _check_conv(conv, 2, what)
        _check_norm(self.norm1, self.conv1.in_channels, what)
        _check_norm(self.norm2, self.conv2.in_channels, what)
        if self.norm1.num_groups != self.norm2.num_groups or self.norm1.eps != self.norm2.eps:
            raise ValueError(f"{what}: norm1 and norm2 differ in groups or eps")
        for t in (x, *self.parameters()):
            require_device(t, what)
        dt = _autocast_dtype(what)
        return _Resnet.apply(x, dt, self.norm1.weight, self.norm1.bias, self.conv1.weight, self.conv1.bias, self.norm2.weight,
                             self.norm2.bias, self.conv2.weight, self.conv2.bias, None if sc is None else sc.weight,
                             None if sc is None else sc.bias, self.norm1.num_groups, float(self.norm1.eps))


_KEYS = {f"{m}.{p}" for m in ("norm1", "conv1", "norm2", "conv2") for p in ("weight", "bias")}
_SHORTCUT = {"conv_shortcut.weight", "conv_shortcut.bias"}


def _is_resnet(m):
    """exactly a ResnetBlock2D's parameter structure, with the geometry DeviceResnetBlock2D runs"""
    keys = {k for k, _ in m.named_parameters()}
    if isinstance(m, DeviceResnetBlock2D) or keys not in (_KEYS, _KEYS | _SHORTCUT):
        return False
    convs = [m.conv1, m.conv2] + ([m.conv_shortcut] if keys != _KEYS else [])
    if not all(isinstance(c, nn.Conv2d) for c in convs) or not all(isinstance(n, nn.GroupNorm) for n in (m.norm1, m.norm2)):
        return False
    if any(isinstance(c, nn.Dropout) and c.p > 0 for c in m.children()):
        return False
    cin, cout = m.conv1.in_channels, m.conv1.out_channels
    return (m.conv1.kernel_size == (3, 3) and m.conv2.kernel_size == (3, 3) and m.conv2.in_channels == cout and m.conv2.out_channels == cout
            and (keys == _KEYS) == (cin == cout) and (keys == _KEYS or m.conv_shortcut.kernel_size == (1, 1)))


def use_device_resnets(module):
    """Replace every descendant of `module` that has exactly a ResnetBlock2D's parameter structure (norm1, conv1, norm2, conv2 and,
    for cin != cout, a 1x1 conv_shortcut; diffusers' block without a time embedding, and the package's own vae._Resnet2D containers)
    by a DeviceResnetBlock2D that SHARES the block's norm / conv sub-modules, hence its Parameter objects: state_dict keys, the
    optimiser's parameter list and checkpoints are unchanged.  Launches nothing.  A replaced block takes and returns CHANNELS-LAST
    fp32 [S, H, W, C] (module docstring) -- the caller's walk has to feed it that layout.  Blocks whose channels are no multiples of
    128 raise.  Returns the module."""
    for name, child in list(module.named_children()):
        if _is_resnet(child):
            cin, cout = child.conv1.in_channels, child.conv1.out_channels
            new = DeviceResnetBlock2D(cin, cout, child.norm1.num_groups, child.norm1.eps, device="meta")
            names = ("norm1", "conv1", "norm2", "conv2") + (("conv_shortcut",) if cin != cout else ())
            setattr(module, name, adopt(new, child, *names))
        else:
            use_device_resnets(child)
    return module


# ---------------------------------------------------------------------------------------------------------------------------------
# Downsample2D / Upsample2D: the two 3x3 resampling convolutions, and whole down / up blocks
# ---------------------------------------------------------------------------------------------------------------------------------
def _gemm(lib, col, K, w16, bias, M, N, dt):
    out = torch.empty(M, N, dtype=torch.float32, device=col.device)
    _lib.check(lib.bg_gemm_bias_act_fwd(_lib.ptr(col), K, _lib.ptr(w16), _lib.ptr(bias), _lib.ptr(out), N, M, N, N, K, DTYPES[dt], _lib.BG_F32,
                                        _lib.BG_ACT_NONE, None, 0, 1, _lib.stream()), "bg_gemm_bias_act_fwd")
    return out


def _gather(lib, x, S, H, W, C, dt, up, stride, pad, Ho, Wo):
    """the im2col matrix [S*Ho*Wo, 9C] of a 3x3 window over x fp32 [S, H, W, C], rounded to dt: bg_im2col's `up`, `stride` and before-padding"""
    col = torch.empty(S * Ho * Wo, 9 * C, dtype=dt, device=x.device)
    _lib.check(lib.bg_im2col(_lib.ptr(x), _lib.ptr(col), DTYPES[dt], S, H, W, C, 3, 3, up, stride, pad, pad, Ho, Wo, None, None, None, 1, 0, None,
                             _lib.stream()), "bg_im2col")
    return col


def _wgrad_geom(lib, dy16, a, weight, S, H, W, geom, dt, need_w, need_b):
    """(dw in the parameter's [N, C, 3, 3] layout, db) of a resampling convolution; H x W: the grid of the 16-bit a [S*H*W, C]"""
    N, C = weight.shape[:2]
    dwp, db = weight_grad(weight, dt, (N, 9 * C), need_w, need_b, lib.bg_conv_wgrad_geom_workspace_bytes(S, H, W, N, C, 3, 3, geom, 0),
                          lambda dwp, db, odt, ws, nbytes: _lib.check(lib.bg_conv_wgrad_geom(
                              _lib.ptr(dy16), N, _lib.ptr(a), C, _lib.ptr(dwp), _lib.ptr(db), S, H, W, N, C, 3, 3, geom, DTYPES[dt], odt, 0,
                              _lib.ptr(ws), nbytes, _lib.stream()), "bg_conv_wgrad_geom"))
    return (dwp.view(N, 3, 3, C).permute(0, 3, 1, 2).contiguous() if need_w else None), db


def _pack_down(lib, weight, dt):
    """the class-ordered pack of bg_conv_down_dgrad (9*C*N elements) of a conv weight [N, C, 3, 3]"""
    N, C = weight.shape[:2]
    w = weight.detach().contiguous()
    out = torch.empty(9 * C * N, dtype=dt, device=w.device)
    _lib.check(lib.bg_conv_weight_pack_down(_lib.ptr(w), DTYPES[w.dtype], N, C, None, _lib.ptr(out), DTYPES[dt], _lib.stream()),
               "bg_conv_weight_pack_down")
    return out


def _down_dgrad(lib, dy16, pack, S, H, W, N, C, dt):
    """dx fp32 [S, H, W, C] of the stride-2 convolution from dy16 [S*H/2*W/2, N]"""
    dx = torch.empty(S, H, W, C, dtype=torch.float32, device=dy16.device)
    nbytes = lib.bg_conv_down_dgrad_workspace_bytes(S, H, W, N, C)
    ws = workspace(nbytes, dy16.device)
    _lib.check(lib.bg_conv_down_dgrad(_lib.ptr(dy16), N, _lib.ptr(pack), _lib.ptr(dx), S, H, W, N, C, DTYPES[dt], _lib.ptr(ws), nbytes,
                                      _lib.stream()), "bg_conv_down_dgrad")
    return dx


def _pool2x2(lib, u, S, H, W, C, add=None):
    """y fp32 [S, H, W, C]: the 2 x 2 sums of u [S*2H*2W, C] (+ add)"""
    y = torch.empty(S, H, W, C, dtype=torch.float32, device=u.device)
    _lib.check(lib.bg_pool2x2_sum(_lib.ptr(u), _lib.ptr(add), _lib.ptr(y), S, H, W, C, _lib.stream()), "bg_pool2x2_sum")
    return y


def _up_fwd(lib, x, a, S, H, W, C, w16, N, bias, dt):
    """conv 3x3 'same' on the nearest-x2 grid of x [S, H, W, C] -> fp32 [S*2H*2W, N]: the implicit GEMM (up = 1) on the 16-bit a where its
    64-tile rule holds, else im2col (up = 1) from x + GEMM -- vae_exec.hip's choice"""
    Ho, Wo = 2 * H, 2 * W
    if not _implicit_ok(S, Ho, Wo, C, N, 9):
        return _gemm(lib, _gather(lib, x, S, H, W, C, dt, 1, 1, 1, Ho, Wo), 9 * C, w16, bias, S * Ho * Wo, N, dt)
    out = torch.empty(S * Ho * Wo, N, dtype=torch.float32, device=a.device)
    d = _lib.ConvDesc()
    d.x, d.S, d.H, d.W, d.C = _lib.ptr(a), S, H, W, C
    d.kh, d.kw, d.up = 3, 3, 1
    d.w, d.bias, d.N = _lib.ptr(w16), _lib.ptr(bias), N
    d.out, d.ldc = _lib.ptr(out), N
    d.add, d.ld_add = None, N
    d.dtype, d.zero_page = DTYPES[dt], _lib.ptr(_zero_page(a.device))
    _lib.check(lib.bg_conv_gemm_fwd(d, _lib.stream()), "bg_conv_gemm_fwd")
    return out


class _Resample(torch.autograd.Function):
    """conv_down (down=True) / conv_up: keeps the 16-bit cast of x -- for conv_up the LOW-resolution one -- and the parameters"""

    @staticmethod
    def forward(ctx, x, weight, bias, down, dt):
        S, H, W, C = x.shape
        N = weight.shape[0]
        with torch.autocast(device_type="cuda", enabled=False):
            lib = _lib.load()
            x = x.contiguous()
            a = _norm_act_cast(lib, x, S, H, W, C, dt)
            w16 = _pack(lib, weight, 3, 3, dt, True)
            b32 = None if bias is None else fp32(bias)
            if down:
                Ho, Wo = H // 2, W // 2
                y = _gemm(lib, _gather(lib, x, S, H, W, C, dt, 0, 2, 0, Ho, Wo), 9 * C, w16, b32, S * Ho * Wo, N, dt)
            else:
                Ho, Wo = 2 * H, 2 * W
                y = _up_fwd(lib, x, a, S, H, W, C, w16, N, b32, dt)
        ctx.a, ctx.params, ctx.geo = a, (weight, bias), (S, H, W, C, N, Ho, Wo, down, dt)
        return y.view(S, Ho, Wo, N)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        S, H, W, C, N, Ho, Wo, down, dt = ctx.geo
        weight, bias = ctx.params
        need = ctx.needs_input_grad
        need_b = bias is not None and need[2]
        dx = dw = db = None
        with torch.autocast(device_type="cuda", enabled=False):
            lib = _lib.load()
            dy = dy.float().contiguous()
            dy16 = _norm_act_cast(lib, dy, S, Ho, Wo, N, dt)
            if need[1] or need_b:
                dw, db = _wgrad_geom(lib, dy16, ctx.a, weight, S, H, W, _lib.BG_CONV_DOWN2 if down else _lib.BG_CONV_UP2, dt, need[1], need_b)
            if need[0] and down:
                dx = _down_dgrad(lib, dy16, _pack_down(lib, weight, dt), S, H, W, N, C, dt)
            elif need[0]:
                da_up = _conv_same(lib, dy, dy16, S, Ho, Wo, N, 3, 3, _pack(lib, weight, 3, 3, dt, False), C, None, None)
                dx = _pool2x2(lib, da_up, S, H, W, C)
        return dx, grad_as(dw, weight.dtype), grad_as(db, bias.dtype) if bias is not None else None, None, None


def _check_resample(x, conv, down, what):
    if x.dtype != torch.float32 or x.dim() != 4 or x.numel() == 0:
        raise ValueError(f"{what}: x must be fp32 channels-last [S, H, W, C], got {tuple(x.shape)} {x.dtype}")
    H, W = x.shape[1:3]
    if not (_pow2(H) and _pow2(W)) or (down and (H < 2 or W < 2)):
        raise ValueError(f"{what}: the grid {H} x {W} must be powers of two" + (", each at least 2" if down else ""))
    if not isinstance(conv, nn.Conv2d):
        raise ValueError(f"{what}: an nn.Conv2d is required, got {type(conv).__name__}")
    stride, padding = ((2, 2), ((0, 0),)) if down else ((1, 1), ((1, 1), "same"))
    if tuple(conv.kernel_size) != (3, 3) or tuple(conv.dilation) != (1, 1) or conv.groups != 1 or conv.padding_mode != "zeros":
        raise ValueError(f"{what}: window {tuple(conv.kernel_size)}, dilation {tuple(conv.dilation)}, groups {conv.groups} (3 x 3, no dilation, one group)")
    if tuple(conv.stride) != stride or conv.padding not in padding:
        raise ValueError(f"{what}: stride {tuple(conv.stride)} with padding {conv.padding} (stride {stride[0]}, padding {padding[0][0]}: "
                         f"{'the pad after the grid is part of the op' if down else 'on the nearest x2 grid'})")
    N, C = conv.out_channels, conv.in_channels
    if N % TILE or C % TILE:
        raise ValueError(f"{what}: in_channels = {C} and out_channels = {N} must be multiples of {TILE}")
    if x.shape[-1] != C:
        raise ValueError(f"{what}: x has {x.shape[-1]} channels, the convolution takes {C}")
    if conv.weight.dtype not in (torch.float32,) + HALF:
        raise ValueError(f"{what}: weight dtype {conv.weight.dtype}")
    for t in (x, conv.weight, conv.bias):
        if t is not None:
            require_device(t, what)
    return _autocast_dtype(what)


def conv_down(x, conv):
    """diffusers' Downsample2D: y = conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2) + b, differentiable.  x: fp32 channels-last [S, H, W, C] on
    the device, H and W powers of two >= 2; conv: a 3x3 nn.Conv2d with stride 2 and padding 0 (the pad after the grid is part of the op),
    channels multiples of 128.  Returns fp32 [S, H/2, W/2, N].  Must run under fp16 / bf16 torch.autocast; anything else raises.  Saves
    the 16-bit cast of x for the backward, which gives dx (fp32, bg_conv_down_dgrad), dW in the parameter's layout and db (fp32 for
    fp32 masters, bg_conv_wgrad_geom).  Enqueues on the current stream, no host synchronisation."""
    dt = _check_resample(x, conv, True, "conv_down")
    return _Resample.apply(x, conv.weight, conv.bias, True, dt)


def conv_up(x, conv):
    """diffusers' Upsample2D: y = conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1) + b, differentiable.  x: fp32
    channels-last [S, H, W, C] on the device, H and W powers of two; conv: a 3x3 nn.Conv2d with stride 1 and padding 1, channels
    multiples of 128.  Returns fp32 [S, 2H, 2W, N].  Must run under fp16 / bf16 torch.autocast; anything else raises.  Saves the 16-bit
    cast of the LOW-resolution x (S*H*W*C elements, not four times that); the backward's dx is the 2 x 2 sum (bg_pool2x2_sum) of the
    stride-1 data gradient on the 2H x 2W grid."""
    dt = _check_resample(x, conv, False, "conv_up")
    return _Resample.apply(x, conv.weight, conv.bias, False, dt)


def _sampler_channels(c, what):
    if c % TILE or c < TILE:
        raise ValueError(f"{what}: c = {c} must be a multiple of {TILE}")


class DeviceDownsample2D(nn.Module):
    """diffusers' Downsample2D (a 3x3 convolution, stride 2, padded after the grid), parameter name `conv`: forward(x) = conv_down(x, conv)"""

    def __init__(self, c, device=None, dtype=None):
        super().__init__()
        _sampler_channels(c, "DeviceDownsample2D")
        self.conv = nn.Conv2d(c, c, 3, stride=2, padding=0, device=device, dtype=dtype)

    def forward(self, x):
        return conv_down(x, self.conv)


class DeviceUpsample2D(nn.Module):
    """diffusers' Upsample2D (nearest x2, then a 3x3 'same' convolution), parameter name `conv`: forward(x) = conv_up(x, conv)"""

    def __init__(self, c, device=None, dtype=None):
        super().__init__()
        _sampler_channels(c, "DeviceUpsample2D")
        self.conv = nn.Conv2d(c, c, 3, padding=1, device=device, dtype=dtype)

    def forward(self, x):
        return conv_up(x, self.conv)


_SAMPLERS = {"downsamplers": DeviceDownsample2D, "upsamplers": DeviceUpsample2D}


class DeviceBlock2D(nn.Module):
    """diffusers' DownEncoderBlock2D / UpDecoderBlock2D with their keys: `resnets`, then optionally `downsamplers` or `upsamplers` (not
    both).  forward(x): fp32 CHANNELS-LAST [S, H, W, cin], the resnets, then the sampler.  The children are taken as given (shared)."""

    def __init__(self, resnets, downsamplers=None, upsamplers=None):
        super().__init__()
        if downsamplers is not None and upsamplers is not None:
            raise ValueError("DeviceBlock2D: downsamplers or upsamplers, not both")
        self.resnets = resnets if isinstance(resnets, nn.ModuleList) else nn.ModuleList(resnets)
        for name, members in (("downsamplers", downsamplers), ("upsamplers", upsamplers)):
            if members is not None:
                setattr(self, name, members if isinstance(members, nn.ModuleList) else nn.ModuleList(members))

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        for name in _SAMPLERS:
            for m in getattr(self, name, ()):
                x = m(x)
        return x


def _is_sampler(m, name):
    """exactly {conv.weight, conv.bias}, a 3x3 nn.Conv2d with the geometry of the list it sits in"""
    if isinstance(m, _SAMPLERS[name]) or {k for k, _ in m.named_parameters()} != {"conv.weight", "conv.bias"}:
        return False
    c = getattr(m, "conv", None)
    stride, padding = ((2, 2), (0, 0)) if name == "downsamplers" else ((1, 1), (1, 1))
    return (isinstance(c, nn.Conv2d) and tuple(c.kernel_size) == (3, 3) and tuple(c.stride) == stride and c.padding == padding
            and tuple(c.dilation) == (1, 1) and c.groups == 1 and c.padding_mode == "zeros" and c.in_channels == c.out_channels)


def _swap_samplers(module):
    for name, child in module.named_children():
        if name in _SAMPLERS and isinstance(child, nn.ModuleList):
            for i, m in enumerate(child):
                if _is_sampler(m, name):
                    child[i] = adopt(_SAMPLERS[name](m.conv.in_channels, device="meta"), m, "conv")
        else:
            _swap_samplers(child)


def _is_block(m):
    """`resnets` and at most one sampler list, nothing else, every member on the device path"""
    kids = dict(m.named_children())
    if isinstance(m, DeviceBlock2D) or "resnets" not in kids or not set(kids) <= {"resnets", *_SAMPLERS} or len(kids) > 2:
        return False
    if any(True for _ in m.parameters(recurse=False)) or not all(isinstance(k, nn.ModuleList) for k in kids.values()):
        return False
    return (all(isinstance(r, DeviceResnetBlock2D) for r in kids["resnets"])
            and all(isinstance(s, _SAMPLERS[n]) for n in _SAMPLERS for s in kids.get(n, ())))


def _wrap(m):
    kids = dict(m.named_children())
    return DeviceBlock2D(kids["resnets"], kids.get("downsamplers"), kids.get("upsamplers")).train(m.training)


def _wrap_blocks(module):
    for name, child in list(module.named_children()):
        if _is_block(child):
            setattr(module, name, _wrap(child))
        elif not isinstance(child, DeviceBlock2D):
            _wrap_blocks(child)


def use_device_blocks(module):
    """use_device_resnets(module), then: every member of a ModuleList named `downsamplers` / `upsamplers` whose only parameters are
    conv.weight / conv.bias of a 3x3 nn.Conv2d with stride 2 / padding 0 (downsamplers) or stride 1 / padding 1 (upsamplers) becomes a
    DeviceDownsample2D / DeviceUpsample2D that SHARES the conv, and every descendant whose children are `resnets` and at most one of the
    two sampler lists (diffusers' DownEncoderBlock2D / UpDecoderBlock2D, vae._DownBlock2D / _UpBlock2D) becomes a DeviceBlock2D that
    shares those lists.  Parameter objects and state_dict keys are unchanged; idempotent; launches nothing.  Modules with other
    children -- a mid block with its attention, conv_in, conv_norm_out, conv_out -- stay what they are (a mid block's resnets are
    swapped by use_device_resnets all the same).  Returns the module -- or, when `module` ITSELF is such a block, the DeviceBlock2D
    around its children.  Converted blocks take and return CHANNELS-LAST fp32 [S, H, W, C]."""
    use_device_resnets(module)
    _swap_samplers(module)
    _wrap_blocks(module)
    return _wrap(module) if _is_block(module) else module
