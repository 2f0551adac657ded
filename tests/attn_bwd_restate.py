"""Numpy fp64 restatement of the training attention core (csrc/attn_train.hip): forward, row log-sum-exp, the three gradients and the
dropout keep mask, from the formulas of include/brepgen_hip.h.  TEST INFRASTRUCTURE: nothing here is on the product path.

    S = scale q k^T (-inf on padded keys);  P = softmax(S);  lse = max + log(sum exp);  O = (P o M rp) V
    delta_i = sum_d dO_id O_id;  dV = (P o M rp)^T dO;  dP = (dO V^T) o M rp;  dS = P o (dP - delta);  dQ = scale dS K;  dK = scale dS^T Q
A sample whose keys are all padded: out = 0, lse = 0, gradients 0.
"""
import numpy as np

from oracle.philox import philox4x32_10

H, DH, D = 12, 64, 768
TAG = 0xAD700000


def threshold(p):
    return int(np.floor(float(p) * 4294967296.0))


def rp_of(p):
    """1 / (1 - p) as the kernels hold it: rounded to fp32."""
    return float(np.float32(1.0 / (1.0 - float(p))))


def keep_mask(B, N, p, seed, draw_id, first_sample=0):
    """uint8 [B, 12, N, N], 1 = kept: one Philox block per (global sample, head, query, 4 consecutive keys)."""
    nkb = (N + 3) // 4
    g = (int(first_sample) + np.arange(B, dtype=np.uint64))[:, None, None, None]
    head = np.arange(H, dtype=np.uint64)[None, :, None, None]
    q = np.arange(N, dtype=np.uint64)[None, None, :, None]
    kb = np.arange(nkb, dtype=np.uint64)[None, None, None, :]
    c = np.zeros((B, H, N, nkb, 4), dtype=np.uint32)
    c[..., 0] = ((q << np.uint64(16)) | kb).astype(np.uint32)
    c[..., 1] = np.broadcast_to(g & np.uint64(0xFFFFFFFF), c.shape[:-1]).astype(np.uint32)
    c[..., 2] = np.uint32(draw_id)
    c[..., 3] = (np.uint64(TAG) | (head << np.uint64(12)) | ((g >> np.uint64(32)) & np.uint64(0xFFF))).astype(np.uint32)
    words = philox4x32_10(c, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    keep = (words >= np.uint32(threshold(p))).astype(np.uint8)
    return keep.reshape(B, H, N, nkb * 4)[..., :N]


def _split(qkv):
    B, N, _ = qkv.shape
    q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(B, N, H, DH).transpose(0, 2, 1, 3).astype(np.float64) for i in range(3))
    return q, k, v


def _probs(q, k, key_pad, scale):
    B, _, N, _ = q.shape
    s = scale * np.einsum("bhid,bhjd->bhij", q, k)
    dead = np.zeros((B, 1, 1, N), dtype=bool) if key_pad is None else np.asarray(key_pad, dtype=bool)[:, None, None, :]
    s = np.where(dead, -np.inf, s)
    m = s.max(-1, keepdims=True)
    empty = ~np.isfinite(m)                                  # every key padded
    m = np.where(empty, 0.0, m)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    p = np.where(empty, 0.0, e / np.where(l > 0, l, 1.0))
    lse = np.where(empty[..., 0], 0.0, m[..., 0] + np.log(np.where(l[..., 0] > 0, l[..., 0], 1.0)))
    return p, lse


def forward(qkv, key_pad=None, scale=0.125, keep=None, p=0.0):
    """qkv [B, N, 2304] -> (out [B, N, 768], lse [B, 12, N]) in fp64.  keep: uint8 [B, 12, N, N] or None."""
    q, k, v = _split(np.asarray(qkv))
    B, _, N, _ = q.shape
    pr, lse = _probs(q, k, key_pad, scale)
    pt = pr if keep is None else pr * keep * rp_of(p)
    out = np.einsum("bhij,bhjd->bhid", pt, v).transpose(0, 2, 1, 3).reshape(B, N, D)
    return out, lse


def backward(qkv, dout, key_pad=None, scale=0.125, keep=None, p=0.0):
    """-> dqkv [B, N, 2304] fp64 (dq | dk | dv)."""
    q, k, v = _split(np.asarray(qkv))
    B, _, N, _ = q.shape
    do = np.asarray(dout).reshape(B, N, H, DH).transpose(0, 2, 1, 3).astype(np.float64)
    pr, _ = _probs(q, k, key_pad, scale)
    mk = 1.0 if keep is None else keep * rp_of(p)
    pt = pr * mk
    o = np.einsum("bhij,bhjd->bhid", pt, v)
    delta = (do * o).sum(-1, keepdims=True)
    dv = np.einsum("bhij,bhid->bhjd", pt, do)
    dp = np.einsum("bhid,bhjd->bhij", do, v) * mk
    ds = pr * (dp - delta)
    dq = scale * np.einsum("bhij,bhjd->bhid", ds, k)
    dk = scale * np.einsum("bhij,bhid->bhjd", ds, q)
    return np.concatenate([t.transpose(0, 2, 1, 3).reshape(B, N, D) for t in (dq, dk, dv)], -1)
