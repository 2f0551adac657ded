"""The formulas include/brepgen_hip.h documents for the conv-layer backward (bg_conv_wgrad, bg_conv_weight_pack, bg_gn_act_bwd and the
data gradient as a forward convolution), restated in plain fp64 tensor arithmetic -- explicit shifts and sums, no torch.nn.functional
convolution or normalisation and no autograd -- so that the CPU tests can hold them against torch.autograd and the GPU tests against the
kernels.  TEST INFRASTRUCTURE.  Activations are channels-last [S, H, W, C]."""
import math

import torch


def taps(kh, kw):
    """[(tap, dy, dx)]: tap = ky * kw + kx reads the pixel shifted by (ky - kh // 2, kx - kw // 2)"""
    return [(ky * kw + kx, ky - kh // 2, kx - kw // 2) for ky in range(kh) for kx in range(kw)]


def shifted(a, dy, dx):
    """b[s, y, x] = a[s, y + dy, x + dx], zero outside the sample's own grid"""
    S, H, W, C = a.shape
    b = torch.zeros_like(a)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y1 > y0 and x1 > x0:
        b[:, y0:y1, x0:x1] = a[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return b


def pack_fwd(w):
    """[N, C, kh, kw] -> [N, kh*kw*C]: fwd[n, tap, c] = w[n, c, tap]"""
    N, C, kh, kw = w.shape
    return w.permute(0, 2, 3, 1).reshape(N, kh * kw * C)


def pack_dgrad(w):
    """[N, C, kh, kw] -> [C, kh*kw*N]: dgrad[c, T - 1 - tap, n] = w[n, c, tap]"""
    N, C, kh, kw = w.shape
    return w.flip(2, 3).permute(1, 2, 3, 0).reshape(C, kh * kw * N)


def unpack_dw(dwp, kh, kw):
    """the tap-major dw [N, kh*kw*C] in the parameter's layout [N, C, kh, kw]"""
    N = dwp.shape[0]
    return dwp.reshape(N, kh, kw, -1).permute(0, 3, 1, 2)


def conv_same(x, wp, kh, kw):
    """'same' stride-1 convolution of channels-last x [S, H, W, C] with a packed weight wp [N, kh*kw*C] -> [S, H, W, N]"""
    C = x.shape[-1]
    out = 0
    for tap, dy, dx in taps(kh, kw):
        out = out + shifted(x, dy, dx) @ wp[:, tap * C:(tap + 1) * C].t()
    return out


def wgrad(dy, a, kh, kw, absolute=False):
    """dw [N, kh*kw*C] and db [N] of bg_conv_wgrad from dy [S, H, W, N] and a [S, H, W, C] (absolute: of |dy|, |a|)"""
    if absolute:
        dy, a = dy.abs(), a.abs()
    N = dy.shape[-1]
    d2 = dy.reshape(-1, N)
    cols = [d2.t() @ shifted(a, sy, sx).reshape(d2.shape[0], -1) for _, sy, sx in taps(kh, kw)]
    return torch.cat(cols, 1), d2.sum(0)


def act_and_derivative(v, act):
    if act == "silu":
        sg = 1 / (1 + torch.exp(-v))
        return v * sg, sg * (1 + v * (1 - sg))
    if act == "gelu":
        cdf = 0.5 * (1 + torch.erf(v / math.sqrt(2.0)))
        return v * cdf, cdf + v * torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)
    return v, torch.ones_like(v)


def gn_stats(x, G, eps):
    """(mean, rstd) [S, G] of x [S, P, C]"""
    S, P, C = x.shape
    xg = x.reshape(S, P, G, C // G)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    return mean, 1 / torch.sqrt(var + eps)


def gn_act(x, gamma, beta, G, eps, act):
    S, P, C = x.shape
    mean, rstd = gn_stats(x, G, eps)
    rep = C // G
    xh = (x - mean.repeat_interleave(rep, 1)[:, None]) * rstd.repeat_interleave(rep, 1)[:, None]
    return act_and_derivative(xh * gamma + beta, act)[0]


def gn_act_bwd(da, x, gamma, beta, G, eps, act, dskip=None, stats=None):
    """(dx, dgamma, dbeta) of a = act(GroupNorm(x)) by the header's formulas.  x, da [S, P, C]; stats: (mean, rstd) [S, G] or None"""
    S, P, C = x.shape
    rep = C // G
    mean, rstd = gn_stats(x, G, eps) if stats is None else stats
    mean_c, rstd_c = mean.repeat_interleave(rep, 1)[:, None], rstd.repeat_interleave(rep, 1)[:, None]      # [S, 1, C]
    xh = (x - mean_c) * rstd_c
    dv = da * act_and_derivative(xh * gamma + beta, act)[1]
    s1, s2 = dv.sum(1), (dv * xh).sum(1)                                    # [S, C]
    dbeta, dgamma = s1.sum(0), s2.sum(0)
    m1 = (s1 * gamma).reshape(S, G, rep).sum(2) / (P * rep)
    m2 = (s2 * gamma).reshape(S, G, rep).sum(2) / (P * rep)
    dx = rstd_c * (dv * gamma - m1.repeat_interleave(rep, 1)[:, None] - xh * m2.repeat_interleave(rep, 1)[:, None])
    if dskip is not None:
        dx = dx + dskip
    return dx, dgamma, dbeta
