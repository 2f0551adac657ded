"""The formulas include/brepgen_hip.h documents for the two resampling convolutions in training (bg_conv_wgrad_geom, bg_conv_down_dgrad,
bg_conv_weight_pack_down, bg_pool2x2_sum), restated in plain fp64 tensor arithmetic -- explicit shifts, slices and sums, no
torch.nn.functional convolution, padding or interpolation and no autograd -- so that the CPU tests can hold them against torch.autograd
and the GPU tests against the kernels.  TEST INFRASTRUCTURE.  Activations are channels-last [S, H, W, C]; weights [N, C, 3, 3].

    DOWN  y = conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)                           Ho = H / 2, Wo = W / 2
    UP    y = conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)   Ho = 2H,    Wo = 2W
"""
import torch

from tests.conv_restate import conv_same, pack_dgrad, shifted

DOWN, UP = 1, 2                                              # bg_conv_geom
TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]      # tap = ky * 3 + kx
# the class-ordered pack: taps of the parity classes (iy odd, ix odd) | (odd, even) | (even, odd) | (even, even) of dx
CLASS_TAPS = (((1, 1),), ((1, 0), (1, 2)), ((0, 1), (2, 1)), ((0, 0), (0, 2), (2, 0), (2, 2)))
CLASS_PARITY = ((1, 1), (1, 0), (0, 1), (0, 0))


def out_grid(H, W, geom):
    return (H // 2, W // 2) if geom == DOWN else (2 * H, 2 * W) if geom == UP else (H, W)


def down_tap(a, ky, kx):
    """g[s, j, i] = a[s, 2j + ky, 2i + kx] where 2j + ky < H and 2i + kx < W, else 0"""
    S, H, W, C = a.shape
    g = torch.zeros(S, H // 2, W // 2, C, dtype=a.dtype, device=a.device)
    part = a[:, ky:H:2, kx:W:2]
    g[:, :part.shape[1], :part.shape[2]] = part
    return g


def up_tap(a, ky, kx):
    """g[s, y, x] = a[s, uy >> 1, ux >> 1] where 0 <= uy = y + ky - 1 < 2H and 0 <= ux = x + kx - 1 < 2W, else 0"""
    S, H, W, C = a.shape
    u = a[:, torch.arange(2 * H, device=a.device) >> 1][:, :, torch.arange(2 * W, device=a.device) >> 1]      # u[s, uy, ux] = a[s, uy >> 1, ux >> 1]
    return shifted(u, ky - 1, kx - 1)                        # the range test on the 2H x 2W grid, before any shift


def tap_of(geom):
    return down_tap if geom == DOWN else up_tap


def fwd(x, w, b, geom):
    """y [S, Ho, Wo, N]"""
    y = 0
    for ky, kx in TAPS:
        y = y + tap_of(geom)(x, ky, kx) @ w[:, :, ky, kx].t()
    return y + b


def wgrad(dy, a, geom, absolute=False):
    """dw tap-major [N, 9C] and db [N] of bg_conv_wgrad_geom from dy [S, Ho, Wo, N] and a [S, H, W, C] (absolute: of |dy|, |a|)"""
    if absolute:
        dy, a = dy.abs(), a.abs()
    d2 = dy.reshape(-1, dy.shape[-1])
    cols = [d2.t() @ tap_of(geom)(a, ky, kx).reshape(d2.shape[0], -1) for ky, kx in TAPS]
    return torch.cat(cols, 1), d2.sum(0)


def pack_down(w):
    """[N, C, 3, 3] -> the class-ordered pack, 9*C*N elements: block k = [C, T_k, N], block[c, t, n] = w[n, c, tap_k[t]]"""
    return torch.cat([torch.stack([w[:, :, ky, kx].t() for ky, kx in taps], 1).reshape(-1) for taps in CLASS_TAPS])


def class_operand(dy, k):
    """[S, Ho, Wo, T_k * N]: for each tap of class k the dy pixel it meets -- (j, i) for tap index 0 / 1, one back for tap index 2 -- or 0"""
    return torch.cat([shifted(dy, -(ky // 2), -(kx // 2)) for ky, kx in CLASS_TAPS[k]], -1)


def down_dgrad(dy, pack, C):
    """dx [S, 2Ho, 2Wo, C] of DOWN from dy [S, Ho, Wo, N] and the class-ordered pack: four class products, interleaved by parity"""
    S, Ho, Wo, N = dy.shape
    dx = torch.zeros(S, 2 * Ho, 2 * Wo, C, dtype=dy.dtype, device=dy.device)
    at = 0
    for k, taps in enumerate(CLASS_TAPS):
        blk = pack[at:at + C * len(taps) * N].reshape(C, len(taps) * N)
        at += C * len(taps) * N
        py, px = CLASS_PARITY[k]
        dx[:, py::2, px::2] = class_operand(dy, k) @ blk.t()
    return dx


def pool2x2(u, add=None):
    """(u[2Y, 2X] + u[2Y, 2X+1]) + (u[2Y+1, 2X] + u[2Y+1, 2X+1]) (+ add), in that association"""
    y = (u[:, 0::2, 0::2] + u[:, 0::2, 1::2]) + (u[:, 1::2, 0::2] + u[:, 1::2, 1::2])
    return y if add is None else y + add


def up_dgrad(dy, w):
    """dx [S, H, W, C] of UP: the 2 x 2 sums of the stride-1 'same' data gradient on the 2H x 2W grid"""
    return pool2x2(conv_same(dy, pack_dgrad(w), 3, 3))
