"""The contract of brepgen_amd/optim.py (csrc/optim.hip) in numpy: the reference's last four lines of a trainer iteration

    scaler.scale(loss).backward(); clip_grad_norm_(params, max_norm); scaler.step(optimizer); scaler.update()

as the library computes them -- the order in which the gradient norm is summed, the per-element fp32 arithmetic with one rounding per
operation, the skip rule and GradScaler's state machine.  What the device produces has to equal this file bit for bit
(tests/test_gpu_optim.py); tests/test_optim_cpu.py holds it against torch on the CPU.  `Trainer(dtype=np.float64)` is the fp64 twin:
the same formulas with every fp32 rounding removed (the skip decisions stay those of the fp32 data).
"""
import math

import numpy as np

CHUNK, MAX_BLOCKS, THREADS, WAVE = 4096, 2048, 256, 64
_LANES = np.arange(WAVE)


def chunk_list(numels):
    """[(tensor, first element)] per CHUNK elements, tensors in order; the last chunk of a tensor is short, an empty tensor has none."""
    return [(i, first) for i, n in enumerate(numels) for first in range(0, int(n), CHUNK)]


def _butterfly(v):
    """64 fp64 lanes: v += v[lane ^ o] for o = 32, 16, .. 1 (every lane ends with the total; lane 0 is returned)."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[_LANES ^ o]
    return v[0]


def grad_partials(grads):
    """Launch 1.  grads: fp32 arrays (any shape).  -> (sumsq fp64 [G], maxabs fp32 [G], nonfinite bool [G]) for G = min(chunks,
    MAX_BLOCKS) workgroups.  Thread t of a workgroup owns elements 4 (t + 256 j) + e of each of its chunks and adds their exact fp64
    squares in the order chunk, j, e; then the butterfly per wave and ((w0 + w1) + w2) + w3."""
    flat = [np.ascontiguousarray(g, dtype=np.float32).reshape(-1) for g in grads]
    chunks = chunk_list([g.size for g in flat])
    G = min(len(chunks), MAX_BLOCKS)
    sumsq, maxabs, bad = np.zeros(G, np.float64), np.zeros(G, np.float32), np.zeros(G, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(G):
            acc = np.zeros(THREADS, np.float64)
            for i, first in chunks[b::G]:
                g = np.zeros(CHUNK, np.float32)
                part = flat[i][first:first + CHUNK]
                g[:part.size] = part
                fin = np.isfinite(part)
                bad[b] |= not fin.all()
                if fin.any():
                    maxabs[b] = max(maxabs[b], np.abs(part[fin]).max())
                sq = (g.astype(np.float64) ** 2).reshape(4, THREADS, 4)
                for j in range(4):
                    for e in range(4):
                        acc = acc + sq[j, :, e]
            w = [_butterfly(acc[k * WAVE:(k + 1) * WAVE]) for k in range(THREADS // WAVE)]
            sumsq[b] = ((w[0] + w[1]) + w[2]) + w[3]
    return sumsq, maxabs, bad


def reduce_partials(sumsq, maxabs, bad):
    """What launches 2 and 3 do first: lane l adds partials l, l + 64, .. in order, then the butterfly.  -> (sum, maxabs, nonfinite)"""
    s = np.zeros(WAVE, np.float64)
    pad = np.zeros(-len(sumsq) % WAVE, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for row in np.concatenate([sumsq, pad]).reshape(-1, WAVE):
            s = s + row
        total = _butterfly(s)
    return total, (np.float32(maxabs.max()) if len(maxabs) else np.float32(0)), bool(bad.any())


def verdict(grads, max_norm=None, scale=None):
    """(total_norm fp32, c fp32, r fp32, found_inf) of one set of gradients: c = min(1, max_norm / (norm + 1e-6)) or 1 without
    max_norm, r = float(1 / double(scale)) or 1 without a scaler, found_inf = a non-finite gradient, or the largest finite |g| not
    finite after both multiplications (rounding is monotonic, so no smaller one can overflow if it does not)."""
    total, maxabs, bad = reduce_partials(*grad_partials(grads))
    with np.errstate(invalid="ignore", over="ignore"):
        norm = np.float32(np.sqrt(total))
        c = np.float32(1.0)
        if max_norm is not None:
            q = np.float32(max_norm) / (norm + np.float32(1e-6))
            c = q if q < np.float32(1.0) else np.float32(1.0)
        r = np.float32(1.0) if scale is None else np.float32(np.float64(1.0) / np.float64(np.float32(scale)))
        big = np.float32(np.float32(maxabs * c) * r)
    return norm, c, r, bool(bad or not np.isfinite(big))


def adamw_elements(p, g, m, v, c, r, lr, weight_decay, betas, eps, beta1_pow, beta2_pow, dtype=np.float32):
    """The per-element update of step number (successful steps so far) + 1; beta_pow = beta ** (successful steps so far) as the running
    fp64 product.  dtype float32: one rounding per operation, in this order; float64: the twin.  -> (p, m, v), new arrays."""
    f = dtype
    b1, b2 = betas
    p, g, m, v = (np.asarray(a).astype(f) for a in (p, g, m, v))
    bc1, bc2 = 1.0 - beta1_pow * b1, 1.0 - beta2_pow * b2
    gg = (g * f(c)) * f(r)
    if weight_decay != 0:
        p = p * f(1.0 - lr * weight_decay)
    m = m + (gg - m) * f(1.0 - b1)
    v = v * f(b2) + f(1.0 - b2) * (gg * gg)
    denom = np.sqrt(v) / f(math.sqrt(bc2)) + f(eps)
    p = p - f(lr / bc1) * (m / denom)
    return p, m, v


class Trainer:
    """Optimiser + scaler state of one parameter list; `update(grads, max_norm)` is one scaler.step(opt, max_norm) + scaler.update().
    groups: [(indices of params, lr, weight_decay)], default one group of everything.  scale=None: no scaler (AdamW.step())."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, scale=65536.0, growth_factor=2.0,
                 backoff_factor=0.5, growth_interval=2000, groups=None, dtype=np.float32):
        self.dtype = dtype
        self.p = [np.array(p, dtype=dtype) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.groups = [[list(range(len(self.p))), lr, weight_decay]] if groups is None else [list(g) for g in groups]
        self.betas, self.eps = betas, eps
        self.step, self.beta1_pow, self.beta2_pow = 0, 1.0, 1.0
        self.scale = None if scale is None else np.float32(scale)
        self.growth_tracker = 0
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, growth_interval
        self.total_norm, self.found_inf, self.skipped = np.float32(0), False, []

    def update(self, grads, max_norm=None):
        """grads: one fp32 array or None per parameter (None: left out of this step).  The gradients are what backward() of the SCALED
        loss left behind."""
        live = [i for i, g in enumerate(grads) if g is not None]
        norm, c, r, found_inf = verdict([grads[i] for i in live], max_norm, self.scale)
        self.total_norm, self.found_inf = norm, found_inf
        if self.dtype == np.float64 and not found_inf:              # the twin: norm, c and r without their fp32 roundings
            total = sum(float((np.asarray(grads[i], np.float64) ** 2).sum()) for i in live)
            c = 1.0 if max_norm is None else min(1.0, max_norm / (math.sqrt(total) + 1e-6))
            r = 1.0 if self.scale is None else 1.0 / float(self.scale)
        if not found_inf:
            for idx, lr, wd in self.groups:
                for i in idx:
                    if grads[i] is None:
                        continue
                    g = np.asarray(grads[i], np.float32).reshape(self.p[i].shape)
                    self.p[i], self.m[i], self.v[i] = adamw_elements(self.p[i], g, self.m[i], self.v[i], c, r, lr, wd, self.betas, self.eps,
                                                                     self.beta1_pow, self.beta2_pow, self.dtype)
        # bg_optim_finish == torch's _amp_update_scale_ + the step counter
        if found_inf:
            self.skipped.append(True)
            if self.scale is not None:
                self.scale, self.growth_tracker = np.float32(np.float64(self.scale) * self.backoff_factor), 0
            return
        self.skipped.append(False)
        self.step += 1
        self.beta1_pow *= self.betas[0]
        self.beta2_pow *= self.betas[1]
        if self.scale is not None:
            self.growth_tracker += 1
            if self.growth_tracker == self.growth_interval:
                with np.errstate(over="ignore"):
                    grown = np.float32(np.float64(self.scale) * self.growth_factor)
                if np.isfinite(grown):
                    self.scale = grown
                self.growth_tracker = 0


def beta_pow(beta, step):
    """beta ** step as `step` fp64 multiplications (what the device state holds; load_state_dict rebuilds it this way)."""
    x = 1.0
    for _ in range(int(step)):
        x *= beta
    return x
