"""ctypes wrappers and case builders of the training attention entries (bg_attn_train_fwd / bg_attn_bwd / bg_attn_dropout_mask), plus
the same math written with torch ops (torch's autograd differentiates it): the fp64 cross-check of tests/attn_bwd_restate.py on the
CPU and the fp64 reference of the one long case on the device.  TEST INFRASTRUCTURE."""
import numpy as np
import torch

from brepgen_amd import _lib
from tests.hip_ops import DT, _p, _stream

H, DH, D = 12, 64, 768
MASK_KINDS = ("none", "tail", "scattered", "one_empty")


def train_fwd(qkv, key_pad, B, N, scale=0.125, p=0.0, seed=0, draw=0, first=0, out=None, lse=None):
    """qkv: any tensor holding [B*N, 2304] rows (dense) -> (out [B*N, 768], lse [B, 12, N]); out / lse may be given (guarded views)."""
    out = torch.empty(B * N, D, dtype=qkv.dtype, device=qkv.device) if out is None else out
    lse = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device) if lse is None else lse
    _lib.check(_lib.load().bg_attn_train_fwd(_p(qkv), _p(key_pad), _p(out), _p(lse), B, N, DT[qkv.dtype], scale, p, seed, draw, first,
                                             _stream()), "bg_attn_train_fwd")
    return out, lse


def workspace(B, N, dtype, device="cuda"):
    n = _lib.load().bg_attn_bwd_workspace_bytes(B, N, DT[dtype])
    return torch.empty(max(n, 4) // 4, dtype=torch.float32, device=device), n


def bwd(qkv, key_pad, lse, dout, B, N, scale=0.125, p=0.0, seed=0, draw=0, first=0, dqkv=None, ws=None, variant=_lib.BG_ATTN_BWD_GENERAL):
    dqkv = torch.empty(B * N, 3 * D, dtype=qkv.dtype, device=qkv.device) if dqkv is None else dqkv
    if ws is None:
        ws = workspace(B, N, qkv.dtype, qkv.device)
    _lib.check(_lib.load().bg_attn_bwd(_p(qkv), _p(key_pad), _p(lse), _p(dout), _p(dqkv), B, N, DT[qkv.dtype], scale, p, seed,
                                       draw, first, variant, _p(ws[0]), ws[1], _stream()), "bg_attn_bwd")
    return dqkv


def dropout_mask(B, N, p, seed, draw, first=0, device="cuda"):
    m = torch.empty(B, H, N, N, dtype=torch.uint8, device=device)
    _lib.check(_lib.load().bg_attn_dropout_mask(_p(m), B, N, p, seed, draw, first, _stream()), "bg_attn_dropout_mask")
    return m


def key_padding(B, N, kind, rng):
    """bool [B, N] (True = padded) or None.  tail: another length per sample; scattered: ~30 % of the keys anywhere (one kept);
    one_empty: the tail mask with every key of the LAST sample padded."""
    if kind == "none":
        return None
    m = np.zeros((B, N), dtype=bool)
    if kind in ("tail", "one_empty"):
        for b in range(B):
            m[b, max(1, (N * (b + 2)) // (B + 2)):] = True
        if kind == "one_empty":
            m[B - 1] = True
    else:
        m = rng.random((B, N)) < 0.3
        m[:, rng.integers(0, N)] = False
    return m


def make_case(B, N, kind, seed, dtype):
    """Operands drawn N(0, 1), q and k scaled by sqrt(2) so that the scores 0.125 q.k have a standard deviation of about 2, rounded to
    `dtype` (the kernels, torch and the fp64 references all see the same rounded values).  -> dict of host arrays."""
    rng = np.random.default_rng(seed)
    qkv = rng.standard_normal((B, N, 3 * D))
    qkv[..., :2 * D] *= np.sqrt(2.0)
    dout = rng.standard_normal((B, N, D))
    qkv_t, dout_t = torch.from_numpy(qkv).to(dtype), torch.from_numpy(dout).to(dtype)
    return dict(B=B, N=N, qkv_t=qkv_t, dout_t=dout_t, qkv=qkv_t.double().numpy(), dout=dout_t.double().numpy(),
                key_pad=key_padding(B, N, kind, rng))


def torch_attention(qkv, key_pad, scale, keep=None, rp=1.0):
    """The restatement's forward in torch ops: qkv [B, N, 2304] (any float dtype / device, requires_grad allowed), key_pad bool [B, N] or
    None without an all-padded sample, keep [B, 12, N, N] or None -> out [B, N, 768]."""
    B, N, _ = qkv.shape
    q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(B, N, H, DH).transpose(1, 2) for i in range(3))
    s = scale * (q @ k.transpose(-1, -2))
    if key_pad is not None:
        s = s.masked_fill(key_pad[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * (keep.to(p.dtype) * rp)
    return (p @ v).transpose(1, 2).reshape(B, N, D)


def torch_grads(qkv, dout, key_pad, scale, keep=None, rp=1.0):
    """(out, dqkv) of torch_attention by torch's autograd."""
    x = qkv.detach().clone().requires_grad_(True)
    out = torch_attention(x, key_pad, scale, keep, rp)
    out.backward(dout)
    return out.detach(), x.grad
