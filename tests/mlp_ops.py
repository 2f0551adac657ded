"""ctypes wrappers of the denoiser-MLP training entries (csrc/mlp_train.hip: bg_thin_expand / bg_thin_contract / bg_thin_wgrad /
bg_ln_silu_train_fwd / bg_ln_silu_bwd / bg_masked_mse_bwd) and the host-side plan of bg_thin_wgrad restated in Python.
TEST INFRASTRUCTURE.  Outputs (and workspaces) may be given, e.g. guarded views."""
import torch

from brepgen_amd import _lib
from tests.hip_ops import DT, NAME, _p, _stream  # noqa: F401
from tests.layer_ops import ln_bwd, ln_fwd
from tests.layer_ops import workspace_bytes as ln_workspace_bytes

C = 768
HALF = (torch.float16, torch.bfloat16)


def wgrad_plan(M, s):
    """(s8, R rows per fp32 chain, chunks, W row workgroups) of bg_thin_wgrad (include/brepgen_hip.h)"""
    kgroups = (s + 7) // 8
    cap = 256 // kgroups
    R = min(max((M + 8 * cap - 1) // (8 * cap), 4), 64)
    chunks = (M + 8 * R - 1) // (8 * R)
    return 8 * kgroups, R, chunks, min(chunks, cap)


def wgrad_workspace_formula(M, s):
    if M <= 0 or not 1 <= s <= 48:
        return 0
    s8, _, _, W = wgrad_plan(M, s)
    return W * (s8 * C + C + s8) * 8


def wgrad_workspace_bytes(M, s):
    return _lib.load().bg_thin_wgrad_workspace_bytes(M, s)


def thin_expand(x, w, b, y_dtype, k_major=False, y=None):
    """x [M, s] (a view with a row stride), w fp32 [768, s] ([s, 768] if k_major), b fp32 [768] or None -> y [M, 768]"""
    M, s = x.shape
    y = torch.empty(M, C, dtype=y_dtype, device=x.device) if y is None else y
    _lib.check(_lib.load().bg_thin_expand(_p(x), DT[x.dtype], x.stride(0) if M > 1 else max(x.stride(0), s), _p(w), int(k_major), _p(b), _p(y),
                                          DT[y.dtype], M, s, _stream()), "bg_thin_expand")
    return y


def thin_contract(a, w, b, y=None):
    """a [M, 768] 16-bit, w fp32 [n, 768], b fp32 [n] or None -> y fp32 [M, n]"""
    M, n = a.shape[0], w.shape[0]
    y = torch.empty(M, n, dtype=torch.float32, device=a.device) if y is None else y
    _lib.check(_lib.load().bg_thin_contract(_p(a), DT[a.dtype], _p(w), _p(b), _p(y), M, n, _stream()), "bg_thin_contract")
    return y


def thin_wgrad(t, u, transposed=False, colsum_of=0, g=None, colsum=None, ws=None):
    """t [M, s] (row-strided view), u [M, 768] 16-bit -> (g fp32 [s, 768] or [768, s], colsum fp32 [768] (1) / [s] (2) / None (0))"""
    M, s = t.shape
    dev = u.device
    g = torch.empty((C, s) if transposed else (s, C), dtype=torch.float32, device=dev) if g is None else g
    if colsum_of and colsum is None:
        colsum = torch.empty(C if colsum_of == 1 else s, dtype=torch.float32, device=dev)
    nbytes = wgrad_workspace_bytes(M, s)
    if ws is None and nbytes:
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().bg_thin_wgrad(_p(t), DT[t.dtype], t.stride(0) if M > 1 else max(t.stride(0), s), _p(u), DT[u.dtype], _p(g),
                                         int(transposed), _p(colsum) if colsum_of else None, colsum_of, M, s, _p(ws), nbytes, _stream()),
               "bg_thin_wgrad")
    return g, (colsum if colsum_of else None)


def ln_silu_fwd(x, gamma, beta, h_dtype, eps=1e-5, h=None, stats=None):
    return ln_fwd(x, gamma, beta, h_dtype, eps, h, stats, entry="bg_ln_silu_train_fwd")


def ln_silu_bwd(dh, x, stats, gamma, beta, grads=True, dx=None, dgamma=None, dbeta=None, ws=None):
    assert _lib.load().bg_ln_silu_bwd_workspace_bytes(x.shape[0]) == ln_workspace_bytes(x.shape[0])
    return ln_bwd(dh, x, stats, gamma, beta, grads, dx, dgamma, dbeta, ws, entry="bg_ln_silu_bwd")


def masked_mse(pred, target, mask, cols):
    """-> out3 (mean, row-mean sum, valid rows) of bg_masked_mse: the forward whose out3 the backward reads"""
    rows, ld = pred.shape
    scratch = torch.empty(1024, dtype=torch.float64, device=pred.device)
    out3 = torch.empty(3, dtype=torch.float32, device=pred.device)
    _lib.check(_lib.load().bg_masked_mse(_p(pred), _p(target), _p(mask), rows, ld, cols[0], cols[1] - cols[0], _p(scratch), _p(out3), _stream()),
               "bg_masked_mse")
    return out3


def masked_mse_bwd(pred, target, mask, cols, out3, g, dpred=None):
    rows, ld = pred.shape
    dpred = torch.empty_like(pred) if dpred is None else dpred
    _lib.check(_lib.load().bg_masked_mse_bwd(_p(pred), _p(target), _p(mask), rows, ld, cols[0], cols[1] - cols[0], _p(out3), g.data_ptr(), _p(dpred),
                                             _stream()), "bg_masked_mse_bwd")          # g: a 0-d device scalar
    return dpred
