"""ctypes wrappers of the encoder-layer glue entries (csrc/layer_train.hip: bg_ln_train_fwd / bg_ln_bwd / bg_dropout_add_fwd /
bg_dropout_bwd / bg_relu_dropout_fwd / bg_relu_dropout_bwd / bg_dropout_mask) and the host-side plan of bg_ln_bwd restated in Python.
TEST INFRASTRUCTURE."""
import torch

from brepgen_amd import _lib
from tests.hip_ops import DT, NAME, _p, _stream  # noqa: F401

C_LN = 768
LN_PAIRS = ((torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float32, torch.bfloat16),
            (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16))                                  # (x, y)
U24 = 2.0 ** -24
MAX_WGS, SLOTS = 2048, 8


def chain_rows(M):
    """R: rows per fp32 column-sum chain of bg_ln_bwd (include/brepgen_hip.h)"""
    return min(max((M + 8191) // 8192, 4), 64)


def workgroups(M):
    return min((M + SLOTS * chain_rows(M) - 1) // (SLOTS * chain_rows(M)), MAX_WGS)


def workspace_formula(M):
    return 0 if M <= 0 else workgroups(M) * 2 * C_LN * 8


def workspace_bytes(M):
    return _lib.load().bg_ln_bwd_workspace_bytes(M)


def ln_fwd(x, gamma, beta, y_dtype, eps=1e-5, y=None, stats=None, entry="bg_ln_train_fwd"):
    """x [M, 768] -> (y [M, 768] in y_dtype, stats fp32 [M, 2]); y / stats may be given (guarded views).  entry: bg_ln_train_fwd or
    mlp_train.hip's bg_ln_silu_train_fwd (tests/mlp_ops.py)"""
    M = x.shape[0]
    y = torch.empty(M, C_LN, dtype=y_dtype, device=x.device) if y is None else y
    stats = torch.empty(M, 2, dtype=torch.float32, device=x.device) if stats is None else stats
    _lib.check(getattr(_lib.load(), entry)(_p(x), DT[x.dtype], _p(gamma), _p(beta), _p(y), DT[y.dtype], _p(stats), M, eps, _stream()), entry)
    return y, stats


def ln_bwd(dy, x, stats, gamma, dskip=None, grads=True, dx=None, dgamma=None, dbeta=None, ws=None, entry="bg_ln_bwd"):
    """-> (dx, dgamma, dbeta); grads=False: dgamma / dbeta NULL, no workspace.  Outputs and workspace may be given (guarded views).
    entry: bg_ln_bwd, or bg_ln_silu_bwd (tests/mlp_ops.py), which takes beta where bg_ln_bwd takes dskip"""
    lib = _lib.load()
    M, dev = x.shape[0], x.device
    dx = torch.empty(M, C_LN, dtype=x.dtype, device=dev) if dx is None else dx
    nbytes = 0
    if grads:
        dgamma = torch.empty(C_LN, dtype=torch.float32, device=dev) if dgamma is None else dgamma
        dbeta = torch.empty(C_LN, dtype=torch.float32, device=dev) if dbeta is None else dbeta
        nbytes = getattr(lib, entry + "_workspace_bytes")(M)
        if ws is None and nbytes:
            ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    _lib.check(getattr(lib, entry)(_p(dy), DT[dy.dtype], _p(x), DT[x.dtype], _p(stats), _p(gamma), _p(dskip), _p(dx),
                                   _p(dgamma) if grads else None, _p(dbeta) if grads else None, M, _p(ws) if grads else None, nbytes,
                                   _stream()), entry)
    return dx, (dgamma if grads else None), (dbeta if grads else None)


def dropout_add_fwd(branch, skip, B, p, seed=0, draw=0, site=1, first=0, out=None):
    M, C = branch.shape
    out = torch.empty_like(skip) if out is None else out
    _lib.check(_lib.load().bg_dropout_add_fwd(_p(branch), DT[branch.dtype], _p(skip), _p(out), DT[skip.dtype], M, C, B, p, seed, draw, site,
                                              first, _stream()), "bg_dropout_add_fwd")
    return out


def dropout_bwd(dout, branch_dtype, B, p, seed=0, draw=0, site=1, first=0, dbranch=None):
    M, C = dout.shape
    dbranch = torch.empty(M, C, dtype=branch_dtype, device=dout.device) if dbranch is None else dbranch
    _lib.check(_lib.load().bg_dropout_bwd(_p(dout), DT[dout.dtype], _p(dbranch), DT[branch_dtype], M, C, B, p, seed, draw, site, first,
                                          _stream()), "bg_dropout_bwd")
    return dbranch


def relu_dropout_fwd(x, B, p, seed=0, draw=0, site=2, first=0, h=None):
    M, C = x.shape
    h = torch.empty_like(x) if h is None else h
    _lib.check(_lib.load().bg_relu_dropout_fwd(_p(x), _p(h), DT[x.dtype], M, C, B, p, seed, draw, site, first, _stream()),
               "bg_relu_dropout_fwd")
    return h


def relu_dropout_bwd(h, dh, p, dx=None):
    M, C = h.shape
    dx = torch.empty_like(h) if dx is None else dx
    _lib.check(_lib.load().bg_relu_dropout_bwd(_p(h), _p(dh), _p(dx), DT[h.dtype], M, C, p, _stream()), "bg_relu_dropout_bwd")
    return dx


def dropout_mask(M, C, B, p, seed=0, draw=0, site=1, first=0, mask=None, device="cuda"):
    mask = torch.empty(M, C, dtype=torch.uint8, device=device) if mask is None else mask
    _lib.check(_lib.load().bg_dropout_mask(_p(mask), M, C, B, p, seed, draw, site, first, _stream()), "bg_dropout_mask")
    return mask
