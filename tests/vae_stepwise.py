"""Step-by-step Python driver of the VAE primitives (the round-1 execution path): the same convolution-net steps the product
runs as ONE bg_vae_run program (brepgen_amd/vae.py), issued one C call at a time with torch-allocated intermediates.  Test
infrastructure only -- it cross-checks the program / the implicit-GEMM convolutions bit for bit
(tests/test_gpu_round2.py::test_vae_program_equals_step_by_step, ::test_vae_implicit_gemm_equals_materialised_im2col) and
serves tools/vae_bench.py as the A/B baseline.

    from vae_stepwise import stepwise
    y = stepwise(module, x, implicit_gemm=True)      # module: one of the four Fast VAE modules (or the widened encoder of a full one), x as module.forward takes it
"""
import ctypes

import torch

from brepgen_amd import _lib
import hip_ops as ops
from brepgen_amd._lib import BG_F32, check, ptr, stream
from brepgen_amd.vae import ACT_NONE, VAE_OUT, VOP_UP1D, _Blocks, _CODE, _pow2

IM2COL_BUDGET = 1 << 32        # bytes of im2col scratch per chunk of samples


class _Steps(_Blocks):
    """The second executor of a module's walk (`m._program`): every primitive runs its C entry point at once on torch-allocated tensors.
    A slot is a (tensor, shape) pair, shape = (S, H, W, C) of the channels-last tensor."""

    def __init__(self, m, implicit_gemm=True):
        self.m, self.implicit_gemm = m, implicit_gemm
        self.input = self.out = None                   # the chunk a walk starts from / what its last step wrote

    def free(self, *slots):                            # torch owns the intermediates
        pass

    def conv(self, src, conv, kh, kw, up=0, norm=None, act=ACT_NONE, res=None, stride=1, pad_mode=0, dst=None, n_out=None, pad16=64):
        out, shape = self._conv(*src, self.packs.conv(conv, pad16), kh, kw, up, norm, act, None if res is None else res[0], stride,
                                (0, 0) if pad_mode == 1 else None)
        if n_out is not None:
            out, shape = out[:, :n_out], (*shape[:3], n_out)
        if dst == VAE_OUT:
            self.out = out.reshape(shape)
        return out, shape

    def _stats(self, x, S, P, C, norm):
        st = torch.empty(S, norm.num_groups, 2, device=x.device, dtype=torch.float32)
        check(_lib.load().bg_groupnorm_stats(ptr(x), ptr(st), S, P, C, norm.num_groups, norm.eps, stream()),
              "bg_groupnorm_stats")
        return st

    def _conv(self, x, shape, pk, kh, kw, up=0, norm=None, act=ACT_NONE, residual=None, stride=1, pad=None):
        """conv (kh x kw) on channels-last x; pad=None: 'same' (kh//2, kw//2); pad=(py, px): zeros before only."""
        S, H, W, C = shape
        lib = _lib.load()
        Hl, Wl = H << up, W << up
        if pad is None:
            py, px = kh // 2, kw // 2
            Ho, Wo = (Hl + 2 * py - kh) // stride + 1, (Wl + 2 * px - kw) // stride + 1
        else:                                          # Downsample2D: F.pad(x, (0,1,0,1)) then stride-2 conv, no padding
            py, px = pad
            Ho, Wo = (Hl + 1 - kh) // stride + 1 if kh > 1 else Hl, (Wl + 1 - kw) // stride + 1
        rows = S * Ho * Wo
        st = self._stats(x, S, H * W, C, norm) if norm is not None else None
        g = norm.weight.detach().float().contiguous() if norm is not None else None
        b = norm.bias.detach().float().contiguous() if norm is not None else None
        implicit = (self.implicit_gemm and pk.dtype != torch.float32 and kh * kw > 1 and stride == 1 and pad is None
                    and C % 64 == 0 and _pow2(C // 64) and _pow2(Ho) and _pow2(Wo) and pk.n % 128 == 0
                    and pk.w.shape[0] == pk.n and ((rows + 127) // 128) * (pk.n // 128) >= 64 and rows < 2 ** 31)
        if implicit:
            # normalise + activate + cast ONCE (a 1x1 "im2col"), then let the GEMM's loader walk the window
            xn = torch.empty(S * H * W, C, device=x.device, dtype=pk.dtype)
            check(lib.bg_im2col(ptr(x), ptr(xn), _CODE[pk.dtype], S, H, W, C, 1, 1, 0, 1, 0, 0, H, W, ptr(st), ptr(g), ptr(b),
                                norm.num_groups if norm is not None else 1, act, None, stream()), "bg_im2col[norm+act+cast]")
            out = torch.empty(rows, pk.n, device=x.device, dtype=torch.float32)
            res = residual.contiguous() if residual is not None else None
            d = _lib.ConvDesc()
            d.x, d.S, d.H, d.W, d.C = ptr(xn), S, H, W, C
            d.kh, d.kw, d.up = kh, kw, up
            d.w, d.bias, d.N = ptr(pk.w), ptr(pk.b), pk.n
            d.out, d.ldc = ptr(out), pk.n
            d.add, d.ld_add = ptr(res), pk.n
            d.dtype, d.zero_page = _CODE[pk.dtype], ptr(self.m._zero_page(x.device))
            check(lib.bg_conv_gemm_fwd(ctypes.byref(d), stream()), "bg_conv_gemm_fwd")
            return out, (S, Ho, Wo, pk.n)
        a = torch.empty(rows, kh * kw * C, device=x.device, dtype=pk.dtype)
        check(lib.bg_im2col(ptr(x), ptr(a), _CODE[pk.dtype], S, H, W, C, kh, kw, up, stride, py, px, Ho, Wo,
                            ptr(st), ptr(g), ptr(b), norm.num_groups if norm is not None else 1, act, None, stream()),
              "bg_im2col")
        out = ops.linear(a, pk.w, pk.b, out_dtype=torch.float32, add=residual, add_div=1, n_valid=pk.n)
        return out, (S, Ho, Wo, pk.n)

    def norm_act_add(self, src, norm, act, res):
        h, (S, H, W, C) = src
        st = self._stats(h, S, H * W, C, norm)
        y = torch.empty(S * H * W, C, device=h.device, dtype=torch.float32)
        check(_lib.load().bg_im2col(ptr(h), ptr(y), BG_F32, S, H, W, C, 1, 1, 0, 1, 0, 0, H, W, ptr(st),
                                    ptr(norm.weight.detach().float().contiguous()), ptr(norm.bias.detach().float().contiguous()),
                                    norm.num_groups, act, ptr(res[0].contiguous()), stream()), "bg_im2col[norm+act+residual]")
        return y, src[1]

    def attn(self, src, at, heads, scale):
        """diffusers Attention over the H*W tokens of a sample: fused q|k|v GEMM, bg_small_attn, projection GEMM + residual."""
        x, shape = src
        S, H, W, C = shape
        qkv, proj = self.packs.attn(at)
        t, _ = self._conv(x, shape, qkv, 1, 1, norm=at.group_norm)
        o = torch.empty(S * H * W, C, device=x.device, dtype=proj.dtype)
        check(_lib.load().bg_small_attn(ptr(t), 3 * C, ptr(o), _CODE[o.dtype], S, H * W, C, heads, scale, stream()), "bg_small_attn")
        return ops.linear(o, proj.w, proj.b, out_dtype=torch.float32, add=x, n_valid=C), shape

    def resample1d(self, src, op):
        x, (S, _, L, C) = src
        name, Lo = ("bg_upsample1d_cubic", 2 * L) if op == VOP_UP1D else ("bg_downsample1d_cubic", L // 2)
        y = torch.empty(S * Lo, C, device=x.device, dtype=torch.float32)
        check(getattr(_lib.load(), name)(ptr(x), ptr(y), S, L, C, stream()), name)
        return y, (S, 1, Lo, C)

    def run(self, x_cl, dt):
        """One chunk x_cl [S, (H,) W, C] through the module's walk -> its output, channels-last [S, (H,) W, C']."""
        self.input = (x_cl, (x_cl.shape[0], 1, *x_cl.shape[1:]) if x_cl.dim() == 3 else tuple(x_cl.shape))
        self.m._program(self, self.m._pack(dt))
        return self.out if x_cl.dim() == 4 else self.out.squeeze(1)


def stepwise(m, x, implicit_gemm=True, im2col_budget=IM2COL_BUDGET):
    """module.forward(x) through the step-by-step driver (chunked against `im2col_budget` like the round-1 path).  The layout and the chunk
    estimate go by the module's class name: the widened encoder of a full VAE (`full._runners[0]`) is an instance of the Fast encoder class."""
    st = _Steps(m, implicit_gemm)
    dt = m._dtype()
    cls = type(m).__name__
    es = 4 if dt == torch.float32 else 2
    x = x.detach().to(torch.float32)
    two_d = cls in ("AutoencoderKLFastDecode", "AutoencoderKLFastEncode")
    x_cl = (x.permute(0, 2, 3, 1) if two_d else x.permute(0, 2, 1)).contiguous()
    n = x_cl.shape[0]
    side = x_cl.shape[1]
    worst = {"AutoencoderKLFastDecode": (side * 2 ** (len(m.block_out) - 1)) ** 2 * 9 * m.block_out[0] * 2 * es,
             "AutoencoderKL1DFastDecode": side * 2 ** len(m.block_out) * 5 * m.block_out[-1] * es,
             "AutoencoderKLFastEncode": side * side * 9 * m.block_out[0] * es,
             "AutoencoderKL1DFastEncode": side * 5 * m.block_out[-1] * es}[cls]     # bytes of one sample's largest im2col matrix
    step = max(1, min(n, im2col_budget // max(1, worst)))
    outs = [st.run(x_cl[i:i + step].contiguous(), dt) for i in range(0, n, step)]
    y = torch.cat(outs) if len(outs) > 1 else outs[0]
    return (y.permute(0, 3, 1, 2) if two_d else y.permute(0, 2, 1)).contiguous()
