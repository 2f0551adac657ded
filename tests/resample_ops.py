"""ctypes wrappers and case builders of the resampling-convolution entries (bg_conv_wgrad_geom and its plan helpers,
bg_conv_weight_pack_down, bg_conv_down_dgrad, bg_pool2x2_sum), and the two torch expressions they are held against.  TEST
INFRASTRUCTURE."""
import torch
import torch.nn.functional as F

from brepgen_amd import _lib
from tests.hip_ops import DT, NAME, _p, _stream  # noqa: F401
from tests.linear_ops import wgrad_call, workspace_formula  # noqa: F401
from tests.resample_restate import DOWN, UP, out_grid


def torch_fwd(x_nchw, w, b, geom):
    """diffusers' Downsample2D / Upsample2D in NCHW, from stock torch"""
    if geom == DOWN:
        return F.conv2d(F.pad(x_nchw, (0, 1, 0, 1)), w, b, stride=2)
    return F.conv2d(F.interpolate(x_nchw, scale_factor=2, mode="nearest"), w, b, padding=1)


def auto_split(S, H, W, N, C, geom, kh=3, kw=3):
    return _lib.load().bg_conv_wgrad_geom_split(S, H, W, N, C, kh, kw, geom)


def workspace_bytes(S, H, W, N, C, geom, split, kh=3, kw=3):
    return _lib.load().bg_conv_wgrad_geom_workspace_bytes(S, H, W, N, C, kh, kw, geom, split)


def wgrad(dy, a, S, H, W, N, C, geom, out_dtype=torch.float32, split=0, bias=True, ld_dy=None, ld_a=None, dw=None, db=None, kh=3, kw=3):
    """dy / a: tensors (or strided views) holding [S*Ho*Wo, N] / [S*H*W, C] pixels; dw / db may be given (guarded views) -> (dw, db)"""
    return wgrad_call("bg_conv_wgrad_geom", (S, H, W, N, C, kh, kw, geom), dy, a, N if ld_dy is None else ld_dy, C if ld_a is None else ld_a,
                      (N, kh * kw * C), out_dtype, split, bias, dw, db)


def pack_down(w, dtype, fwd=False, down=True, out_f=None, out_d=None):
    """w [N, C, 3, 3] -> (fwd [N, 9C] or None, the class-ordered pack [9*C*N] or None) in `dtype`"""
    N, C = w.shape[:2]
    if fwd and out_f is None:
        out_f = torch.empty(N, 9 * C, dtype=dtype, device=w.device)
    if down and out_d is None:
        out_d = torch.empty(9 * C * N, dtype=dtype, device=w.device)
    _lib.check(_lib.load().bg_conv_weight_pack_down(_p(w), DT[w.dtype], N, C, _p(out_f) if fwd else None, _p(out_d) if down else None, DT[dtype],
                                                    _stream()), "bg_conv_weight_pack_down")
    return (out_f if fwd else None), (out_d if down else None)


def down_dgrad(dy16, pack, S, H, W, N, C, dx=None, ld_dy=None):
    """dy16 [S*H/2*W/2, N] (or a strided view), the class-ordered pack -> dx fp32 [S*H*W, C] (may be given: a guarded view)"""
    lib = _lib.load()
    dx = torch.empty(S * H * W, C, dtype=torch.float32, device=pack.device) if dx is None else dx
    nbytes = lib.bg_conv_down_dgrad_workspace_bytes(S, H, W, N, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pack.device)
    _lib.check(lib.bg_conv_down_dgrad(_p(dy16), N if ld_dy is None else ld_dy, _p(pack), _p(dx), S, H, W, N, C, DT[pack.dtype], _p(ws), nbytes,
                                      _stream()), "bg_conv_down_dgrad")
    return dx


def pool(u, S, H, W, C, add=None, y=None):
    """u fp32 [S, 2H, 2W, C] -> y fp32 [S*H*W, C] (may be given: a guarded view)"""
    y = torch.empty(S * H * W, C, dtype=torch.float32, device=u.device) if y is None else y
    _lib.check(_lib.load().bg_pool2x2_sum(_p(u), _p(add), _p(y), S, H, W, C, _stream()), "bg_pool2x2_sum")
    return y


def draw(S, H, W, N, C, geom, dtype, seed, device="cuda"):
    """standard-normal dy [S, Ho, Wo, N] and a [S, H, W, C] rounded to `dtype`"""
    Ho, Wo = out_grid(H, W, geom)
    g = torch.Generator(device="cpu").manual_seed(seed)
    dy = torch.randn(S, Ho, Wo, N, generator=g).to(dtype).to(device)
    a = torch.randn(S, H, W, C, generator=g).to(dtype).to(device)
    return dy, a
