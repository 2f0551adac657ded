"""ctypes wrappers and case builders of the Linear-backward entries (bg_linear_wgrad / bg_weight_cast and the host-side plan
helpers), plus the slicing rule restated in Python.  TEST INFRASTRUCTURE."""
import torch

from brepgen_amd import _lib
from tests.hip_ops import DT, NAME, _p, _stream  # noqa: F401

ROW_STEP = 32                       # rows of M a workgroup stages per step (include/brepgen_hip.h: bg_linear_wgrad)
LAYERS = {"in_proj": (2304, 768), "out_proj": (768, 768), "linear1": (1024, 768), "linear2": (768, 1024)}      # (N, K)
U24 = 2.0 ** -24


def auto_split(M, N, K):
    return _lib.load().bg_linear_wgrad_split(M, N, K)


def workspace_bytes(M, N, K, split):
    return _lib.load().bg_linear_wgrad_workspace_bytes(M, N, K, split)


def workspace_formula(N, K, S):
    """the header's formula: 0 for S = 1, else the fp32 partials [S][N][K] + [S][N] rounded up to 256 bytes"""
    return 0 if S <= 1 else (4 * S * N * (K + 1) + 255) // 256 * 256


def slices(M, S):
    """the slicing rule: [(first row, end row)] of the S slices -- whole row steps, equal but for the last"""
    steps = (M + ROW_STEP - 1) // ROW_STEP
    rows = (steps + S - 1) // S * ROW_STEP
    return [(s * rows, min(M, (s + 1) * rows)) for s in range(S)]


def wgrad_call(entry, lead, dy, b, ld_dy, ld_b, shape, out_dtype, split, bias, dw, db, ws=None):
    """The weight-gradient entry `entry` (bg_linear_wgrad, lead = (M, N, K) | bg_conv_wgrad, lead = (S, H, W, N, C, kh, kw)) on dy and
    its second operand b with their strides; dw (of `shape`) / db / ws may be given (guarded views).  -> (dw, db)"""
    lib, dev = _lib.load(), dy.device
    dw = torch.empty(shape, dtype=out_dtype, device=dev) if dw is None else dw
    if bias and db is None:
        db = torch.empty(shape[0], dtype=out_dtype, device=dev)
    nbytes = getattr(lib, entry + "_workspace_bytes")(*lead, split)
    if ws is None and nbytes:
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    _lib.check(getattr(lib, entry)(_p(dy), ld_dy, _p(b), ld_b, _p(dw), _p(db) if bias else None, *lead, DT[dy.dtype], DT[out_dtype], split,
                                   _p(ws), nbytes, _stream()), entry)
    return dw, (db if bias else None)


def wgrad(dy, x, M, N, K, out_dtype=torch.float32, split=0, bias=True, ld_dy=None, ld_x=None, dw=None, db=None, ws=None):
    """dy / x: tensors (or strided views) holding [M, N] / [M, K] rows; dw / db / ws may be given (guarded views).  -> (dw, db)"""
    return wgrad_call("bg_linear_wgrad", (M, N, K), dy, x, N if ld_dy is None else ld_dy, K if ld_x is None else ld_x, (N, K), out_dtype, split,
                      bias, dw, db, ws)


def weight_cast(src, dtype, dst=True, dst_t=True, out=None, out_t=None):
    R, C = src.shape
    if dst and out is None:
        out = torch.empty(R, C, dtype=dtype, device=src.device)
    if dst_t and out_t is None:
        out_t = torch.empty(C, R, dtype=dtype, device=src.device)
    _lib.check(_lib.load().bg_weight_cast(_p(src), DT[src.dtype], R, C, _p(out) if dst else None, _p(out_t) if dst_t else None, DT[dtype],
                                          _stream()), "bg_weight_cast")
    return out, out_t


def draw_pair(lead, N, K, dtype, seed, device="cuda"):
    """standard-normal dy [*lead, N] and second operand [*lead, K] rounded to `dtype`"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    dy = torch.randn(*lead, N, generator=g).to(dtype).to(device)
    b = torch.randn(*lead, K, generator=g).to(dtype).to(device)
    return dy, b


def draw(M, N, K, dtype, seed, device="cuda"):
    """standard-normal dy [M, N], x [M, K] rounded to `dtype`"""
    return draw_pair((M,), N, K, dtype, seed, device)


def reference(dy, x):
    """fp64 from the rounded values: (dw, db, sum |dy| |x|, sum |dy|)"""
    d, xx = dy.double(), x.double()
    return d.t() @ xx, d.sum(0), d.abs().t() @ xx.abs(), d.abs().sum(0)
