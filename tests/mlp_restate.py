"""Restatement of csrc/mlp_train.hip for the tests, in numpy: the three thin products and bg_masked_mse_bwd in the kernels' OWN order
of operations (float32, with the fused multiply-add emulated exactly; float64 where the kernels use fp64) -- the GPU tests compare
them bit for bit -- and LN + SiLU on tests/layer_restate.py's LayerNorm (numpy's exp is not the device's expf: compared by error, not
by bits).  `mlp` strings them into the whole Sequential, forward and backward.  TEST INFRASTRUCTURE."""
import numpy as np

from tests import layer_restate as LR
from tests import mlp_ops as ops

f32, f64 = np.float32, np.float64
C = 768


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, elementwise on float32 arrays.  The product of two float32 is exact in float64; the sum is
    formed in float64 rounded TO ODD (the rounding error from TwoSum decides), after which the rounding to float32 is the correct
    one (53 >= 24 + 2 bits)."""
    p = np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)
    c = np.asarray(c, f32).astype(f64)
    p, c = np.broadcast_arrays(p, c)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        odd = (np.ascontiguousarray(s).view(np.int64) & 1) == 1
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ~odd
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def thin_expand(x, w_kc, b=None):
    """x [M, s], w_kc [s, 768] (W as (k, column)), b [768] or None -> float32 [M, 768] before the rounding to y's dtype:
    acc = b; acc = fma(x[m, k], W(k, c), acc), k ascending"""
    x, w_kc = np.asarray(x, f32), np.asarray(w_kc, f32)
    acc = np.broadcast_to(np.zeros(C, f32) if b is None else np.asarray(b, f32), (x.shape[0], C)).copy()
    for k in range(x.shape[1]):
        acc = fma32(x[:, k:k + 1], w_kc[k][None], acc)
    return acc


def thin_contract(a, w, b=None):
    """a [M, 768], w [n, 768], b [n] or None -> float32 [M, n]: lane l's chain over columns 8 (l + 32 j) + e (j, then e, ascending),
    the 32-lane butterfly, + b"""
    a, w = np.asarray(a, f32), np.asarray(w, f32)
    M, n = a.shape[0], w.shape[0]
    A, W = a.reshape(M, 1, 3, 32, 8), w.reshape(1, n, 3, 32, 8)
    p = np.zeros((M, n, 32), f32)
    for j in range(3):
        for e in range(8):
            p = fma32(A[:, :, j, :, e], W[:, :, j, :, e], p)
    lane = np.arange(32)
    for o in (16, 8, 4, 2, 1):
        p = p + p[..., lane ^ o]
    y = p[..., 0]
    return y if b is None else y + np.asarray(b, f32)[None]


def thin_wgrad(t, u):
    """t [M, s], u [M, 768] -> (g [s, 768], column sums of u [768], column sums of t [s]), float32, in the plan's order
    (tests/mlp_ops.py wgrad_plan): fp32 chains of R rows per half-wave (8 rows for the column sums), the 8 chains of a chunk in fp64 in slot order, the chunks of a
    workgroup in order, the workgroups in index order, rounded once"""
    t, u = np.asarray(t, f32), np.asarray(u, f32)
    M, s = t.shape
    _, R, chunks, W = ops.wgrad_plan(M, s)
    pg, pu, pt = np.zeros((W, s, C), f64), np.zeros((W, C), f64), np.zeros((W, s), f64)
    for chunk in range(chunks):
        acc, au, at = np.zeros((8, s, C), f32), np.zeros((8, C), f32), np.zeros((8, s), f32)
        dau, dat = np.zeros((8, C), f64), np.zeros((8, s), f64)                # the column sums: fp32 chains of 8 rows, folded in fp64
        for i in range(R):
            rows = chunk * 8 * R + 8 * i + np.arange(8)
            live = rows < M
            if not live.any():
                break
            rr = np.minimum(rows, M - 1)
            tv, uv = t[rr], u[rr]
            acc = np.where(live[:, None, None], fma32(tv[:, :, None], uv[:, None, :], acc), acc)
            au = np.where(live[:, None], au + uv, au)
            at = np.where(live[:, None], at + tv, at)
            if i % 8 == 7:
                dau, dat, au, at = dau + au.astype(f64), dat + at.astype(f64), np.zeros_like(au), np.zeros_like(at)
        dau, dat = dau + au.astype(f64), dat + at.astype(f64)
        w = chunk % W
        for slot in range(8):
            pg[w] += acc[slot].astype(f64)
            pu[w] += dau[slot]
            pt[w] += dat[slot]
    g, cu, ct = np.zeros((s, C), f64), np.zeros(C, f64), np.zeros(s, f64)
    for w in range(W):
        g, cu, ct = g + pg[w], cu + pu[w], ct + pt[w]
    return g.astype(f32), cu.astype(f32), ct.astype(f32)


def silu(v):
    v = np.asarray(v, f32)
    return v / (f32(1.0) + np.exp(-v))


def silu_grad(v):
    v = np.asarray(v, f32)
    sg = f32(1.0) / (f32(1.0) + np.exp(-v))
    return sg + v * sg * (f32(1.0) - sg)


def ln_silu_fwd(x, gamma, beta, eps=1e-5):
    """-> (h float32 before the rounding to h's dtype, stats [M, 2])"""
    y, stats = LR.ln_fwd(np.asarray(x, f32), gamma, beta, eps)
    return silu(y), stats


def ln_silu_bwd(dh, x, stats, gamma, beta):
    """-> (dx, dgamma, dbeta): v recomputed as the forward formed it, dv = dh * SiLU'(v), then the LayerNorm backward on dv"""
    x, gamma, beta = np.asarray(x, f32), np.asarray(gamma, f32), np.asarray(beta, f32)
    v = (x - stats[:, :1]) * stats[:, 1:2] * gamma + beta
    return LR.ln_bwd(np.asarray(dh, f32) * silu_grad(v), x, stats, gamma)


def masked_mse_bwd(pred, target, mask, cols, valid, g):
    """pred / target float32 [rows, ld], mask uint8 [rows] or None, valid = out3[2], g the upstream scalar -> dpred float32"""
    pred, target = np.asarray(pred, f32), np.asarray(target, f32)
    out = np.zeros_like(pred)
    if not valid > 0:
        return out
    coef = (f32(2.0) * f32(g)) / (f32(valid) * f32(cols[1] - cols[0]))
    rows = np.ones(pred.shape[0], bool) if mask is None else np.asarray(mask) == 0
    with np.errstate(invalid="ignore"):
        d = (pred[:, cols[0]:cols[1]] - target[:, cols[0]:cols[1]]) * coef
    out[:, cols[0]:cols[1]] = np.where(rows[:, None], d, f32(0.0))
    return out


def mlp(x, p, dy, eps=1e-5):
    """The Sequential(Linear(k, 768), LayerNorm, SiLU, Linear(768, n)) with parameters p = (W0, b0, gamma, beta, W3, b3), forward and
    backward for the output gradient dy, all in float32 with no rounding to 16 bits between the pieces: a thin side runs the restated
    kernel, a wide one (768) a float64 matrix product.  -> (y, {name: gradient}) with torch's parameter names."""
    W0, b0, gamma, beta, W3, b3 = (np.asarray(v, f32) for v in p)
    x, dy = np.asarray(x, f32), np.asarray(dy, f32)
    k, n = W0.shape[1], W3.shape[0]
    z = thin_expand(x, W0.T, b0) if k <= 48 else (x.astype(f64) @ W0.T.astype(f64) + b0).astype(f32)
    h, stats = ln_silu_fwd(z, gamma, beta, eps)
    y = thin_contract(h, W3, b3) if n <= 48 else (h.astype(f64) @ W3.T.astype(f64) + b3).astype(f32)
    if n <= 48:
        dh = thin_expand(dy, W3)                                  # dA = dY W3: W3 [n, 768] is already (k, column)
        dW3, _, db3 = thin_wgrad(dy, h)
    else:
        dh = (dy.astype(f64) @ W3.astype(f64)).astype(f32)
        dW3, db3 = (dy.astype(f64).T @ h.astype(f64)).astype(f32), dy.astype(f64).sum(0).astype(f32)
    dz, dgamma, dbeta = ln_silu_bwd(dh, z, stats, gamma, beta)
    if k <= 48:
        g, db0, _ = thin_wgrad(x, dz)
        dW0 = g.T                                                 # the kernel writes this layout itself (g_transposed)
    else:
        dW0, db0 = (dz.astype(f64).T @ x.astype(f64)).astype(f32), dz.astype(f64).sum(0).astype(f32)
    return y, {"0.weight": dW0, "0.bias": db0, "1.weight": dgamma, "1.bias": dbeta, "3.weight": dW3, "3.bias": db3}
