"""Restatement of csrc/layer_train.hip for the tests: the elementwise dropout mask from oracle.philox.philox4x32_10 (numpy), the
elementwise ops as their fp32 expressions (torch, any device), and the LayerNorm forward / backward in the kernels' OWN summation order
(numpy float32 for the chains and row sums, float64 where the kernels use fp64).  TEST INFRASTRUCTURE.

The derived bound of the gamma / beta gradients (`dgamma_dbeta_bounds`), u = 2^-24, R = rows per fp32 chain (<= 64):

  dbeta[c]  = sum_m dy[m, c]: R - 1 fp32 additions per chain, fp64 additions across chains and workgroups (2^-53 each: below 1e-6 of
              the rest for the at most 8 + 64 + 32 of them per path), one rounding to fp32:    |dbeta - ref| <= (R + 3) u sum_m |dy|.
  dgamma[c] = sum_m dy[m, c] xhat[m, c]: one more rounding for the product, and the kernel's xhat is not the reference's:
              |dgamma - ref| <= (R + 3) u sum_m |dy| |xhat|  +  sum_m |dy| E[m, c],     E >= |xhat_kernel - xhat_fp64|.
  E, first order in u, from the forward's two passes over a row of 768 = 32 lanes x 3 chunks x 8 (a sum passes 3 pairwise levels,
  2 chunk additions and 5 butterfly steps = 10 additions, then the product with the rounded constant 1 / 768: 12 roundings):
      |mean_k - mean| <= e_mu = 12 u mean_c |x|;
      d_k = fl(x - mean_k):  |d_k - d| <= e_mu + u |d|;
      var_k: the squares (1 rounding each), the same 12 roundings, + eps (1), and  sum (d + e)^2 - sum d^2 <= 2 sqrt(sum d^2) sqrt(sum e^2)
             + sum e^2  give a relative error of var + eps of at most  2 (e_mu r + u) + 14 u,   r = rstd = 1 / sqrt(var + eps);
      rstd_k = 1 / sqrtf(.): half of that plus 2 roundings (sqrtf and the division):  |rstd_k - r| / r <= e_mu r + 10 u;
      xhat_k = fl(d_k rstd_k):  E = |xhat| (e_mu r + 10 u + 2 u) + e_mu r.
  Rows with |mean| >> std make e_mu r large: that is the price of ANY fp32 mean, not of this summation order."""
import math

import numpy as np
import torch

from oracle.philox import philox4x32_10
from tests import layer_ops as ops

TAG = 0xD4090000
f32 = np.float32
_M32 = np.uint64(0xFFFFFFFF)


def rp_of(p):
    return float(np.float32(1.0 / (1.0 - p)))


def threshold(p):
    return int(math.floor(p * 65536.0))


def keep_mask(M, C, B, p, seed, draw_id, site, first_sample=0):
    """uint8 [M, C] (1 = kept): row r = token r // B of sample r % B, global sample g = first_sample + r % B (brepgen_hip.h)"""
    assert C % 8 == 0 and M % B == 0
    CB = C // 8
    r = np.arange(M, dtype=np.uint64)
    n, g = r // np.uint64(B), np.uint64(first_sample) + r % np.uint64(B)
    c = np.zeros((M, CB, 4), dtype=np.uint32)
    c[..., 0] = ((n[:, None] * np.uint64(CB) + np.arange(CB, dtype=np.uint64)[None]) & _M32).astype(np.uint32)
    c[..., 1] = (g & _M32).astype(np.uint32)[:, None]
    c[..., 2] = np.uint32(draw_id)
    c[..., 3] = (np.uint64(TAG | (site << 12)) | ((g >> np.uint64(32)) & np.uint64(0xFFF))).astype(np.uint32)[:, None]
    w = philox4x32_10(c, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))                  # [M, CB, 4]
    hw = np.stack([w & np.uint32(0xFFFF), w >> np.uint32(16)], -1).reshape(M, C)          # element j: half j & 1 of word j >> 1
    return (hw >= threshold(p)).astype(np.uint8)


# ---- the elementwise ops: fp32 expressions, rounded once (keep: bool tensor like the operands, or None = no mask) ----
def dropout_add(branch, skip, keep, rp):
    kept = skip.float() + branch.float() * rp
    return (kept if keep is None else torch.where(keep, kept, skip.float())).to(skip.dtype)


def dropout_bwd(dout, keep, rp, branch_dtype):
    kept = dout.float() * rp
    return (kept if keep is None else torch.where(keep, kept, torch.zeros_like(kept))).to(branch_dtype)


def relu_dropout(x, keep, rp):
    xf = x.float()
    passes = ~(xf <= 0) if keep is None else keep & ~(xf <= 0)
    return torch.where(passes, xf * rp, torch.zeros_like(xf)).to(x.dtype)


def relu_dropout_bwd(h, dh, rp):
    return torch.where(h.float() > 0, dh.float() * rp, torch.zeros_like(dh.float())).to(h.dtype)


# ---- LayerNorm in the kernels' order ----
def _sum8(a):
    return ((a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])) + ((a[..., 4] + a[..., 5]) + (a[..., 6] + a[..., 7]))


def row_sum(v):
    """v float32 [M, 768] -> [M]: chunk (l + 32 j) of lane l; 8 values pairwise, the lane's chunks in order, 32-lane butterfly"""
    c = _sum8(v.reshape(v.shape[0], 3, 32, 8))                     # [M, j, l]
    s = (c[:, 0] + c[:, 1]) + c[:, 2]                              # 0 + c0 is c0
    lane = np.arange(32)
    for o in (16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, 0]


def ln_fwd(x, gamma, beta, eps=1e-5):
    """x, gamma, beta float32 arrays -> (y float32 before the rounding to y's dtype, stats [M, 2])"""
    x, inv = x.astype(f32), f32(1.0 / 768.0)
    mean = row_sum(x) * inv
    d = x - mean[:, None]
    rstd = f32(1.0) / np.sqrt(row_sum(d * d) * inv + f32(eps))
    return d * rstd[:, None] * gamma.astype(f32) + beta.astype(f32), np.stack([mean, rstd], 1).astype(f32)


def ln_bwd(dy, x, stats, gamma, dskip=None):
    """float32 arrays (16-bit operands: their values) -> (dx float32 before the rounding to x's dtype, dgamma, dbeta float32 [768])"""
    dy, x, gamma = dy.astype(f32), x.astype(f32), gamma.astype(f32)
    M, inv = x.shape[0], f32(1.0 / 768.0)
    xh = (x - stats[:, :1]) * stats[:, 1:2]
    g = gamma[None] * dy
    c1, c2 = row_sum(g) * inv, row_sum(g * xh) * inv
    dx = stats[:, 1:2] * ((g - c1[:, None]) - xh * c2[:, None]) + (f32(0.0) if dskip is None else dskip.astype(f32))
    R, G = ops.chain_rows(M), ops.workgroups(M)
    part = np.zeros((G, 2, 768), dtype=np.float64)
    prod = dy * xh
    for chunk in range((M + 8 * R - 1) // (8 * R)):
        for slot in range(8):
            ag, ab = np.zeros(768, f32), np.zeros(768, f32)
            for i in range(R):
                row = chunk * 8 * R + 8 * i + slot
                if row >= M:
                    break
                ag, ab = ag + prod[row], ab + dy[row]
            part[chunk % G, 0] += ag.astype(np.float64)
            part[chunk % G, 1] += ab.astype(np.float64)
    per = (G + 31) // 32
    groups = [part[k * per:min(G, (k + 1) * per)] for k in range(32)]
    tot = np.zeros((2, 768), dtype=np.float64)
    for grp in groups:
        s = np.zeros((2, 768), dtype=np.float64)
        for w in range(grp.shape[0]):
            s = s + grp[w]
        tot = tot + s
    return dx.astype(f32), tot[0].astype(f32), tot[1].astype(f32)


def dgamma_dbeta_bounds(dy, x, M, eps=1e-5):
    """(bound of |dgamma - ref|, bound of |dbeta - ref|), float64 tensors [768]: the module docstring.  dy, x: torch tensors [M, 768]."""
    u, R = ops.U24, ops.chain_rows(M)
    d, xx = dy.double().abs(), x.double()
    mean = xx.mean(1, keepdim=True)
    r = 1.0 / torch.sqrt(((xx - mean) ** 2).mean(1, keepdim=True) + eps)
    xhat = ((xx - mean) * r).abs()
    e_mu_r = 12 * u * xx.abs().mean(1, keepdim=True) * r
    E = xhat * (e_mu_r + 12 * u) + e_mu_r
    return (R + 3) * u * (d * xhat).sum(0) + (d * E).sum(0), (R + 3) * u * d.sum(0)
