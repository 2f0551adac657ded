"""ctypes wrappers and case builders of the conv-layer backward entries (bg_conv_wgrad / bg_conv_weight_pack / bg_gn_act_bwd and the
host-side plan helpers) and of the forward entries the data gradient runs on.  TEST INFRASTRUCTURE."""
import torch

from brepgen_amd import _lib
from brepgen_amd import conv as CV
from tests.hip_ops import DT, NAME, _p, _stream  # noqa: F401
from tests.linear_ops import draw_pair, wgrad_call, workspace_formula  # noqa: F401

ACT = CV.ACTS


def auto_split(S, H, W, N, C, kh, kw):
    return _lib.load().bg_conv_wgrad_split(S, H, W, N, C, kh, kw)


def workspace_bytes(S, H, W, N, C, kh, kw, split):
    return _lib.load().bg_conv_wgrad_workspace_bytes(S, H, W, N, C, kh, kw, split)


def wgrad(dy, a, S, H, W, N, C, kh, kw, out_dtype=torch.float32, split=0, bias=True, ld_dy=None, ld_a=None, dw=None, db=None):
    """dy / a: tensors (or strided views) holding [S*H*W, N] / [S*H*W, C] pixels; dw / db may be given (guarded views) -> (dw, db)"""
    return wgrad_call("bg_conv_wgrad", (S, H, W, N, C, kh, kw), dy, a, N if ld_dy is None else ld_dy, C if ld_a is None else ld_a,
                      (N, kh * kw * C), out_dtype, split, bias, dw, db)


def weight_pack(w, dtype, fwd=True, dgrad=True, out_f=None, out_d=None):
    """w [N, C, kh, kw] -> (fwd [N, kh*kw*C], dgrad [C, kh*kw*N]) in `dtype`"""
    N, C, kh, kw = w.shape
    if fwd and out_f is None:
        out_f = torch.empty(N, kh * kw * C, dtype=dtype, device=w.device)
    if dgrad and out_d is None:
        out_d = torch.empty(C, kh * kw * N, dtype=dtype, device=w.device)
    _lib.check(_lib.load().bg_conv_weight_pack(_p(w), DT[w.dtype], N, C, kh, kw, _p(out_f) if fwd else None, _p(out_d) if dgrad else None,
                                               DT[dtype], _stream()), "bg_conv_weight_pack")
    return out_f, out_d


def gn_stats(x, G, eps):
    """bg_groupnorm_stats of x [S, P, C] -> [S, G, 2]"""
    S, P, C = x.shape
    st = torch.empty(S, G, 2, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().bg_groupnorm_stats(_p(x), _p(st), S, P, C, G, eps, _stream()), "bg_groupnorm_stats")
    return st


def gn_act_bwd(da, x, stats, gamma, beta, G, act, dskip=None, params=True, dx=None, dgamma=None, dbeta=None):
    S, P, C = x.shape
    dev = x.device
    dx = torch.empty(S, P, C, dtype=torch.float32, device=dev) if dx is None else dx
    if params:
        dgamma = torch.empty(C, dtype=torch.float32, device=dev) if dgamma is None else dgamma
        dbeta = torch.empty(C, dtype=torch.float32, device=dev) if dbeta is None else dbeta
    nbytes = _lib.load().bg_gn_act_bwd_workspace_bytes(S, P, C, G)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().bg_gn_act_bwd(_p(da), _p(x), _p(stats), _p(gamma), _p(beta), _p(dskip), _p(dx), _p(dgamma) if params else None,
                                         _p(dbeta) if params else None, S, P, C, G, ACT[act], _p(ws), nbytes, _stream()), "bg_gn_act_bwd")
    return dx, dgamma, dbeta


def data_grad(dy, w, dtype):
    """the data gradient of a 'same' convolution with the nn.Conv2d weight w [N, C, kh, kw] for dy fp32 channels-last [S, H, W, N], the
    way conv.py runs it: -> (da fp32 [S, H, W, C], whether the implicit GEMM took it)"""
    lib = _lib.load()
    S, H, W, N = dy.shape
    C, kh, kw = w.shape[1:]
    dy16 = CV._norm_act_cast(lib, dy, S, H, W, N, dtype)
    wd = CV._pack(lib, w, kh, kw, dtype, False)
    da = CV._conv_same(lib, dy, dy16, S, H, W, N, kh, kw, wd, C, None, None)
    return da.view(S, H, W, C), CV._implicit_ok(S, H, W, N, C, kh * kw)


def draw(S, H, W, N, C, dtype, seed, device="cuda"):
    """standard-normal dy [S, H, W, N] and a [S, H, W, C] rounded to `dtype`"""
    return draw_pair((S, H, W), N, C, dtype, seed, device)
