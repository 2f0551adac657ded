"""Drop-in mirrors of the two VAE *decoders* BrepGen samples with, on the HIP path.

``AutoencoderKLFastDecode`` (network.py:948-1040, built at sample.py:72-84) and ``AutoencoderKL1DFastDecode``
(network.py:786-858, built at sample.py:86-99): same constructor keywords, same ``forward(z)`` -> decoded points,
and the diffusers checkpoint key layout, so ``load_state_dict(torch.load(vae.pt), strict=False)`` works as at
sample.py:83,98 (the file also holds ``encoder.*`` / ``quant_conv.*``, which are ignored).

Execution: channels-last fp32 activations; every convolution = ``bg_im2col`` (GroupNorm + SiLU/GELU and the nearest
x2 up-sampling folded into the gather) + the MFMA GEMM with bias / residual fused in its epilogue; mid-block
attention = one fused q|k|v GEMM + ``bg_small_attn`` + projection GEMM; ``Upsample1d("cubic")`` = ``bg_upsample1d_cubic``.
The nn.Module tree below only holds parameters.  Like the denoisers, bf16 operands inside autocast, exact fp32 outside.

A pass is ONE C call: each module compiles itself (once per dtype) into a flat ``bg_vae_op`` program and ``bg_vae_run``
enqueues every launch of it, chunking the batch against a caller-owned workspace.

Each network's layer order is written once, in its class's ``_program(pg, P)``: a walk that names sub-modules and calls the primitives
of its executor ``pg`` (``conv``, ``norm_act_add``, ``attn``, ``resample1d``, ``free``; the two residual blocks are compositions of them in
``_Blocks``).  ``_Program`` records the calls as program steps; ``P`` (``_pack(dt)``) packs a sub-module's weights the first time the walk
names it.  The second executor, tests/vae_stepwise.py, runs every primitive at once from Python -- the cross-check of ``bg_vae_run``.

Below the decoders: the Fast encoders (posterior mean only), and the full ``AutoencoderKL`` / ``AutoencoderKL1D`` the VAE trainers build
(trainer.py:20-30, 150-160), which run the same two programs with one ``bg_vae_posterior`` launch (``DiagonalGaussianDistribution``:
sample + KL) in between.
"""
import ctypes
import math

import torch
import torch.nn as nn

from . import _lib
from ._lib import BG_BF16, BG_F16, BG_F32, check, ptr, stream

_CODE = {torch.bfloat16: BG_BF16, torch.float16: BG_F16, torch.float32: BG_F32}

CUBIC2 = [2 * v for v in (-0.01171875, -0.03515625, 0.11328125, 0.43359375, 0.43359375, 0.11328125, -0.03515625,
                          -0.01171875)]
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2


# --------------------------------------------------------------------------------------------------
# parameter containers (diffusers key layout)
# --------------------------------------------------------------------------------------------------
class _Resnet2D(nn.Module):
    def __init__(self, cin, cout, groups):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, cin, eps=1e-6)
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1)
        self.norm2 = nn.GroupNorm(groups, cout, eps=1e-6)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)


class _Attn2D(nn.Module):
    def __init__(self, c, groups):
        super().__init__()
        self.group_norm = nn.GroupNorm(groups, c, eps=1e-6)
        self.to_q, self.to_k, self.to_v = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)
        self.to_out = nn.ModuleList([nn.Linear(c, c), nn.Dropout(0.0)])


class _Up2D(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, padding=1)


class _UpBlock2D(nn.Module):
    def __init__(self, cin, cout, n, groups, upsample):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet2D(cin if i == 0 else cout, cout, groups) for i in range(n)])
        if upsample:
            self.upsamplers = nn.ModuleList([_Up2D(cout)])


class _Mid2D(nn.Module):
    def __init__(self, c, groups):
        super().__init__()
        self.attentions = nn.ModuleList([_Attn2D(c, groups)])
        self.resnets = nn.ModuleList([_Resnet2D(c, c, groups), _Resnet2D(c, c, groups)])


class _Decoder2D(nn.Module):
    def __init__(self, latent, out_ch, block_out, layers_per_block, groups):
        super().__init__()
        top = block_out[-1]
        self.conv_in = nn.Conv2d(latent, top, 3, padding=1)
        self.mid_block = _Mid2D(top, groups)
        rev = list(reversed(block_out))
        blocks, prev = [], rev[0]
        for i, ch in enumerate(rev):
            blocks.append(_UpBlock2D(prev, ch, layers_per_block + 1, groups, upsample=i != len(rev) - 1))
            prev = ch
        self.up_blocks = nn.ModuleList(blocks)
        self.conv_norm_out = nn.GroupNorm(groups, block_out[0], eps=1e-6)
        self.conv_out = nn.Conv2d(block_out[0], out_ch, 3, padding=1)


class _ResConv(nn.Module):
    def __init__(self, cin, mid, cout):
        super().__init__()
        if cin != cout:
            self.conv_skip = nn.Conv1d(cin, cout, 1, bias=False)
        self.conv_1 = nn.Conv1d(cin, mid, 5, padding=2)
        self.group_norm_1 = nn.GroupNorm(1, mid)
        self.conv_2 = nn.Conv1d(mid, cout, 5, padding=2)
        self.group_norm_2 = nn.GroupNorm(1, cout)


class _Attn1D(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.group_norm = nn.GroupNorm(1, c)
        self.query, self.key, self.value, self.proj_attn = (nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c),
                                                            nn.Linear(c, c))


class _Cubic(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("kernel", torch.tensor(CUBIC2))


class _UpBlock1D(nn.Module):                       # network.py:30-48
    def __init__(self, cin, cout):
        super().__init__()
        self.resnets = nn.ModuleList([_ResConv(cin, cin, cin), _ResConv(cin, cin, cin), _ResConv(cin, cin, cout)])
        self.up = _Cubic()


class _Mid1D(nn.Module):                           # network.py:51-83
    def __init__(self, c):
        super().__init__()
        self.attentions = nn.ModuleList([_Attn1D(c) for _ in range(6)])
        self.resnets = nn.ModuleList([_ResConv(c, c, c) for _ in range(6)])


class _Decoder1D(nn.Module):                       # network.py:188-244
    def __init__(self, latent, out_ch, block_out, groups):
        super().__init__()
        top = block_out[-1]
        self.conv_in = nn.Conv1d(latent, top, 3, padding=1)
        self.mid_block = _Mid1D(top)
        rev = list(reversed(block_out))
        blocks, prev = [], rev[0]
        for ch in rev:
            blocks.append(_UpBlock1D(prev, ch))
            prev = ch
        self.up_blocks = nn.ModuleList(blocks)
        self.conv_norm_out = nn.GroupNorm(groups, block_out[0], eps=1e-6)
        self.conv_out = nn.Conv1d(block_out[0], out_ch, 3, padding=1)


# --------------------------------------------------------------------------------------------------
# execution helpers
# --------------------------------------------------------------------------------------------------
class _Packed:
    """One convolution / linear as a GEMM: weight [n_pad, K] (compute dtype, or fp32 when K % 64 != 0), fp32 bias."""
    __slots__ = ("w", "b", "n", "k", "dtype")


def _pow2(v):
    return v > 0 and (v & (v - 1)) == 0


VOP_CONV, VOP_NORM_ACT_ADD, VOP_ATTN, VOP_UP1D, VOP_DOWN1D = 0, 1, 2, 3, 4
VAE_OUT = 255


def _check(t, what):
    if not t.is_cuda:
        raise _lib.BrepgenHipError(f"brepgen_amd VAE {what} runs on the MI355X only (tensor on {t.device})")


class _Blocks:
    """The residual blocks of the four networks, written once over the primitives of whoever executes a walk (`_program`): `_Program`
    below records each as a bg_vae_op step, tests/vae_stepwise.py runs each at once.  A walk names modules; their weights come
    from `packs`, the `_Packs` the walk was given."""
    PRIMITIVES = ("conv", "norm_act_add", "attn", "resample1d", "free")
    packs = None

    def resnet2d(self, x, r):                          # diffusers ResnetBlock2D
        h = self.conv(x, r.conv1, 3, 3, norm=r.norm1, act=ACT_SILU)
        sc = self.conv(x, r.conv_shortcut, 1, 1) if hasattr(r, "conv_shortcut") else x
        out = self.conv(h, r.conv2, 3, 3, norm=r.norm2, act=ACT_SILU, res=sc)
        self.free(h, x, sc)
        return out

    def resconv(self, x, r):
        # diffusers ResConvBlock: conv k5 -> GroupNorm(1) -> GELU -> conv k5 -> GroupNorm(1) -> GELU, + (1x1) skip.  group_norm_1 + GELU
        # fold into the gather of conv_2; the trailing group_norm_2 + GELU cannot fold into the next consumer (the residual add sits in
        # between), so it is one pass of its own with the add fused.
        h1 = self.conv(x, r.conv_1, 1, 5)
        h2 = self.conv(h1, r.conv_2, 1, 5, norm=r.group_norm_1, act=ACT_GELU)
        self.free(h1)
        sk = self.conv(x, r.conv_skip, 1, 1) if hasattr(r, "conv_skip") else x
        out = self.norm_act_add(h2, r.group_norm_2, ACT_GELU, sk)
        self.free(h2, x, sk)
        return out


class _Program(_Blocks):
    """A flat bg_vae_op program under construction: steps + a free-list slot allocator (slot 0 = the input)."""
    input = 0

    def __init__(self):
        self.steps, self.keep, self._free, self.n_slots = [], [], [], 1
        self.ops = None

    def new(self):
        if self._free:
            return self._free.pop()
        self.n_slots += 1
        return self.n_slots - 1

    def free(self, *slots):
        self._free.extend(s for s in dict.fromkeys(slots) if s > 0 and s not in self._free)

    def step(self, op, src, dst, res=None):
        o = _lib.VaeOp()
        o.op, o.src, o.res = op, src, -1 if res is None else res
        o.dst = self.new() if dst is None else dst
        o.stride = 1
        self.steps.append(o)
        return o

    def norm(self, o, norm, act):
        g, b = norm.weight.detach().float().contiguous(), norm.bias.detach().float().contiguous()
        self.keep += [g, b]
        o.gn_gamma, o.gn_beta, o.gn_groups, o.gn_eps, o.act = ptr(g), ptr(b), norm.num_groups, norm.eps, act

    def conv(self, src, conv, kh, kw, up=0, norm=None, act=ACT_NONE, res=None, stride=1, pad_mode=0, dst=None, n_out=None, pad16=64):
        pk = self.packs.conv(conv, pad16)
        o = self.step(VOP_CONV, src, dst, res)
        o.kh, o.kw, o.up, o.stride, o.pad_mode = kh, kw, up, stride, pad_mode
        o.n_out, o.n_pad, o.w_dtype = pk.n if n_out is None else n_out, pk.w.shape[0], _CODE[pk.dtype]
        o.w, o.bias = ptr(pk.w), ptr(pk.b)
        if norm is not None:
            self.norm(o, norm, act)
        return o.dst

    def norm_act_add(self, src, norm, act, res):
        o = self.step(VOP_NORM_ACT_ADD, src, None, res)
        self.norm(o, norm, act)
        return o.dst

    def attn(self, src, at, heads, scale):
        qkv, proj = self.packs.attn(at)
        o = self.step(VOP_ATTN, src, None)
        o.n_pad, o.w_dtype, o.w, o.bias = qkv.w.shape[0], _CODE[qkv.dtype], ptr(qkv.w), ptr(qkv.b)
        o.n_pad2, o.w2_dtype, o.w2, o.bias2 = proj.w.shape[0], _CODE[proj.dtype], ptr(proj.w), ptr(proj.b)
        o.heads, o.scale = heads, scale
        self.norm(o, at.group_norm, ACT_NONE)
        self.free(src)
        return o.dst

    def resample1d(self, x, op):
        o = self.step(op, x, None)
        self.free(x)
        return o.dst

    def finish(self):
        assert self.steps[-1].dst == VAE_OUT and self.n_slots <= 8
        self.ops = (_lib.VaeOp * len(self.steps))(*self.steps)
        return self


class _HipVAE(nn.Module):
    WS_BUDGET = 8 << 30            # bytes of bg_vae_run workspace (activation slots + scratch) per chunk of samples
    TWO_STREAMS_MIN = 2048         # samples from which a pass is cut into two concurrent halves (below: launch-bound, nothing to overlap)

    def __init__(self):
        super().__init__()
        self.compute_dtype = None
        # 16-bit modes: the 3x3 / k5 convolutions run as IMPLICIT GEMMs inside bg_vae_run: GroupNorm + activation + cast in one
        # elementwise pass, then the GEMM gathers the window itself -- the kh*kw-fold im2col matrix is never written (fp32 and
        # tiny batches take the materialised im2col path, bit-identical).  The step-by-step Python driver of the same
        # primitives that cross-checks the program lives in tests/vae_stepwise.py.
        self._packs = {}
        self._programs = {}
        self._zero = None
        self._ws = {}                  # (device, stream) -> workspace kept between passes (a fresh multi-GiB hipMalloc costs more than the pass)
        self.two_streams = True        # large batches: two halves of a pass in flight on forked streams (bit-identical; _run)
        self._side = None

    def _apply(self, fn, *a, **k):
        self._packs, self._programs, self._ws = {}, {}, {}
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packs, self._programs = {}, {}
        return super().load_state_dict(*a, **k)

    def __setattr__(self, name, value):
        # switches of earlier versions: an nn.Module would accept the assignment silently and nothing would change
        if name in ("executor", "implicit_gemm"):
            raise AttributeError(f"{type(self).__name__}.{name} no longer exists: every pass is one bg_vae_run program; the "
                                 "step-by-step driver of the same kernels is tests/vae_stepwise.py")
        super().__setattr__(name, value)

    def release_workspace(self):
        """Drop the cached bg_vae_run workspaces (up to WS_BUDGET bytes per (device, stream) this module has decoded on)."""
        self._ws = {}

    def _zero_page(self, device):
        if self._zero is None or self._zero.device != device:
            self._zero = torch.zeros(1 << 16, dtype=torch.uint8, device=device)  # >= 2 * C bytes (one pixel of zeros) for any C <= 32768
        return self._zero

    def _run(self, x_cl, out_shape, dt):
        """bg_vae_run over the whole batch x_cl [n, (H,) W, C] -> [n, *out_shape]; chunks sized to WS_BUDGET.  Large batches are cut into
        two halves that run CONCURRENTLY -- the first on the caller's stream, the second on a forked helper stream, joined before the
        call returns (`two_streams`; each stream has its own workspace): a pass alternates MFMA-bound convolutions with HBM-bound
        GroupNorm / activation passes and tile-round tails, and two of them in flight fill each other's gaps, exactly like the sample
        groups of the denoisers (n_split).  Samples are independent and chunk boundaries do not change a sample's bits (tests), so
        the result is bit-identical."""
        if dt not in self._programs:
            self._programs[dt] = self._program(_Program(), self._pack(dt)).finish()
        n = x_cl.shape[0]
        out = torch.empty(n, *out_shape, device=x_cl.device, dtype=torch.float32)
        self._zero_page(x_cl.device)                                    # (created on the caller's stream, BEFORE the fork below orders the helper behind it)
        if self.two_streams and n >= self.TWO_STREAMS_MIN and not torch.cuda.is_current_stream_capturing():
            h = (n // 2 + 63) // 64 * 64                                # (whole 64-sample groups per half)
            cur = torch.cuda.current_stream(x_cl.device)
            side = self._side_stream(x_cl.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._run_into(x_cl[h:], out[h:], dt)
            self._run_into(x_cl[:h], out[:h], dt)
            cur.wait_stream(side)
        else:
            self._run_into(x_cl, out, dt)
        return out

    def _side_stream(self, device):
        if self._side is None or self._side.device != device:
            self._side = torch.cuda.Stream(device=device)
        return self._side

    def _run_into(self, x_cl, out, dt):
        pg, lib = self._programs[dt], _lib.load()
        n = x_cl.shape[0]
        h, w, c = (1, *x_cl.shape[1:]) if x_cl.dim() == 3 else x_cl.shape[1:]
        size = lambda n_, chunk: lib.bg_vae_workspace_bytes(pg.ops, len(pg.steps), pg.n_slots, h, w, c, n_, chunk)
        ref = min(n, 4096)
        per_sample = max(1, size(ref, ref) // ref)
        chunk = max(1, min(n, self.WS_BUDGET // per_sample))
        need = size(n, chunk)
        if need == 0:
            raise _lib.BrepgenHipError("bg_vae_workspace_bytes: malformed VAE program")
        key = (x_cl.device, stream())
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            self._ws[key] = None                                     # release the smaller one first
            ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=x_cl.device)
        check(lib.bg_vae_run(pg.ops, len(pg.steps), pg.n_slots, h, w, c, ptr(x_cl), n, chunk, ptr(out),
                             ptr(self._zero_page(x_cl.device)), ptr(ws), ws.numel(), stream()), "bg_vae_run")

    def _dtype(self):
        if self.compute_dtype is not None:
            return self.compute_dtype
        if torch.is_autocast_enabled():
            dt = torch.get_autocast_dtype('cuda')
            return dt if dt in (torch.bfloat16, torch.float16) else torch.bfloat16
        return torch.float32

    # ---- packing ----
    def _pack(self, dt):
        """The module's weights in compute dtype `dt`, packed as a walk asks for them; kept (with the programs that point into them) until
        the parameters move or change."""
        if dt not in self._packs:
            self._packs[dt] = _Packs(dt)
        return self._packs[dt]

    @staticmethod
    def _pack_gemm(weight2d, bias, dt, pad16=64):
        n, k = weight2d.shape
        p = _Packed()
        use = dt if (dt == torch.float32 or k % 64 == 0) else torch.float32
        w = weight2d.detach().to(torch.float32)
        pad = 1 if use == torch.float32 else pad16
        if n % pad:
            w = torch.cat([w, w.new_zeros((-n) % pad, k)])
        p.w = w.to(use).contiguous()
        b = torch.zeros(n, device=w.device) if bias is None else bias.detach().to(torch.float32)
        if b.numel() % pad:
            b = torch.cat([b, b.new_zeros((-b.numel()) % pad)])
        p.b, p.n, p.k, p.dtype = b.contiguous(), n, k, use
        return p

    @staticmethod
    def _pack_conv(conv, dt, pad16=64):
        """pad16: rows the 16-bit weight matrix is zero-padded to a multiple of.  128 for a NARROW windowed convolution (conv_out:
        3 output channels): the implicit GEMM then takes it as one 128-column tile that stores only the real columns, instead of
        materialising the 9-fold / 3-fold im2col matrix of the largest activation of the pass for the generic kernel."""
        w = conv.weight.detach()
        if w.dim() == 3:                               # Conv1d [Cout, Cin, k] -> [Cout, k*Cin] (tap-major)
            w2 = w.permute(0, 2, 1).reshape(w.shape[0], -1)
        else:                                          # Conv2d [Cout, Cin, kh, kw] -> [Cout, kh*kw*Cin]
            w2 = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
        return _HipVAE._pack_gemm(w2, conv.bias, dt, pad16)


class _Packs(dict):
    """One module's pack cache for one compute dtype: sub-module -> what `_pack_conv` / `_pack_gemm` made of it, packed the first time a
    walk names the sub-module."""

    def __init__(self, dt):
        super().__init__()
        self.dt = dt

    def conv(self, conv, pad16=64):
        if conv not in self:
            self[conv] = _HipVAE._pack_conv(conv, self.dt, pad16)
        return self[conv]

    def attn(self, at):
        """-> (fused q|k|v, output projection) of a diffusers Attention (2-D mid block) or AttentionBlock (1-D mid block)."""
        if at not in self:
            q, k, v, proj = (at.to_q, at.to_k, at.to_v, at.to_out[0]) if hasattr(at, "to_q") else (at.query, at.key, at.value, at.proj_attn)
            self[at] = (_HipVAE._pack_gemm(torch.cat([q.weight, k.weight, v.weight]), torch.cat([q.bias, k.bias, v.bias]), self.dt),
                        _HipVAE._pack_gemm(proj.weight, proj.bias, self.dt))
        return self[at]


class AutoencoderKLFastDecode(_HipVAE):
    """Surface-VAE decoder: z [F,3,4,4] -> points [F,3,32,32]  (network.py:948-1040)."""

    def __init__(self, in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",),
                 up_block_types=("UpDecoderBlock2D",), block_out_channels=(64,), layers_per_block=1, act_fn="silu",
                 latent_channels=4, norm_num_groups=32, sample_size=32, scaling_factor=0.18215, force_upcast=True):
        super().__init__()
        if act_fn != "silu":
            raise NotImplementedError("BrepGen builds its VAEs with act_fn='silu'")
        self.block_out = tuple(block_out_channels)
        self.groups, self.latent, self.out_ch = norm_num_groups, latent_channels, out_channels
        self.decoder = _Decoder2D(latent_channels, out_channels, self.block_out, layers_per_block, norm_num_groups)
        self.post_quant_conv = nn.Conv2d(latent_channels, latent_channels, 1)

    def _program(self, pg, P):
        pg.packs, d = P, self.decoder
        x = pg.conv(pg.input, self.post_quant_conv, 1, 1)
        x2 = pg.conv(x, d.conv_in, 3, 3)
        pg.free(x)
        x = pg.resnet2d(x2, d.mid_block.resnets[0])
        x = pg.attn(x, d.mid_block.attentions[0], 1, 1.0 / math.sqrt(self.block_out[-1]))
        x = pg.resnet2d(x, d.mid_block.resnets[1])
        for blk in d.up_blocks:
            for r in blk.resnets:
                x = pg.resnet2d(x, r)
            if hasattr(blk, "upsamplers"):
                x2 = pg.conv(x, blk.upsamplers[0].conv, 3, 3, up=1)
                pg.free(x)
                x = x2
        pg.conv(x, d.conv_out, 3, 3, norm=d.conv_norm_out, act=ACT_SILU, dst=VAE_OUT, pad16=128)
        return pg

    def forward(self, z, return_dict=True, generator=None):
        _check(z, "decode")
        z_cl = z.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()
        return self._decode_cl(z_cl).permute(0, 3, 1, 2).contiguous()

    def _decode_cl(self, z_cl):
        """Channels-last latents [F,4,4,3] -> channels-last point grids [F,32,32,3] (the layout the kernels use)."""
        dt = self._dtype()
        side = z_cl.shape[1] * 2 ** (len(self.block_out) - 1)
        return self._run(z_cl, (side, side, self.out_ch), dt)

    def decode_tokens(self, surfZ):
        """Token-layout latents [..., 16*3] (position-major, channel-minor: what SurfZNet denoises) -> point grids
        [..., 32, 32, 3].  Equals sample.py:289-290's `vae(z.unflatten(-1,(16,3)).flatten(0,1).permute(0,2,1)
        .unflatten(-1,(4,4))).permute(0,2,3,1).unflatten(0,(B,S))` without the two NCHW round trips: the token
        layout already is the channels-last layout."""
        _check(surfZ, "decode")
        lead = surfZ.shape[:-1]
        if surfZ.numel() == 0:                                       # a rank that owns no sample of a sharded batch
            return surfZ.new_zeros((*lead, *self._decode_cl_shape()), dtype=torch.float32)
        z_cl = surfZ.detach().to(torch.float32).reshape(-1, 4, 4, self.latent).contiguous()
        return self._decode_cl(z_cl).reshape(*lead, *self._decode_cl_shape())

    def _decode_cl_shape(self):
        side = 4 * 2 ** (len(self.block_out) - 1)
        return (side, side, self.out_ch)


class AutoencoderKL1DFastDecode(_HipVAE):
    """Edge-VAE decoder: z [G,3,4] -> points [G,3,32]  (network.py:786-858)."""

    def __init__(self, in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",),
                 up_block_types=("UpDecoderBlock2D",), block_out_channels=(64,), layers_per_block=1, act_fn="silu",
                 latent_channels=4, norm_num_groups=32, sample_size=32, scaling_factor=0.18215):
        super().__init__()
        self.block_out = tuple(block_out_channels)
        self.groups, self.latent, self.out_ch = norm_num_groups, latent_channels, out_channels
        self.decoder = _Decoder1D(latent_channels, out_channels, self.block_out, norm_num_groups)
        self.post_quant_conv = nn.Conv1d(latent_channels, latent_channels, 1)

    def _program(self, pg, P):
        pg.packs, d = P, self.decoder
        x = pg.conv(pg.input, self.post_quant_conv, 1, 1)
        x2 = pg.conv(x, d.conv_in, 1, 3)
        pg.free(x)
        x = x2
        c = self.block_out[-1]
        for r, at in zip(d.mid_block.resnets, d.mid_block.attentions):
            x = pg.resconv(x, r)
            x = pg.attn(x, at, c // 32, 1.0 / math.sqrt(32))
        for blk in d.up_blocks:
            for r in blk.resnets:
                x = pg.resconv(x, r)
            x = pg.resample1d(x, VOP_UP1D)
        pg.conv(x, d.conv_out, 1, 3, norm=d.conv_norm_out, act=ACT_SILU, dst=VAE_OUT, pad16=128)
        return pg

    def forward(self, z, return_dict=True):
        _check(z, "decode")
        z_cl = z.detach().to(torch.float32).permute(0, 2, 1).contiguous()          # [G, L, 3]
        return self._decode_cl(z_cl).permute(0, 2, 1).contiguous()

    def _decode_cl(self, z_cl):
        """Channels-last latents [G,4,3] -> channels-last polylines [G,32,3]."""
        dt = self._dtype()
        length = z_cl.shape[1] * 2 ** len(self.block_out)
        return self._run(z_cl, (length, self.out_ch), dt)

    def decode_tokens(self, edgeZ):
        """Token-layout latents [..., 4*3] (the first 12 of EdgeZNet's 18 channels) -> polylines [..., 32, 3]; equals
        sample.py:293-294's `vae(z.unflatten(-1,(4,3)).reshape(-1,4,3).permute(0,2,1)).permute(0,2,1).reshape(B,S,E,32,3)`."""
        _check(edgeZ, "decode")
        lead = edgeZ.shape[:-1]
        if edgeZ.numel() == 0:
            return edgeZ.new_zeros((*lead, 4 * 2 ** len(self.block_out), self.out_ch), dtype=torch.float32)
        z_cl = edgeZ.detach().to(torch.float32).reshape(-1, 4, self.latent).contiguous()
        out = self._decode_cl(z_cl)
        return out.reshape(*lead, out.shape[1], out.shape[2])


# --------------------------------------------------------------------------------------------------
# encoders (training-time API surface of the path: trainer.py:521,925 call FastEncode under no_grad)
# --------------------------------------------------------------------------------------------------
class _Down2D(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, stride=2, padding=0)


class _DownBlock2D(nn.Module):
    def __init__(self, cin, cout, n, groups, downsample):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet2D(cin if i == 0 else cout, cout, groups) for i in range(n)])
        if downsample:
            self.downsamplers = nn.ModuleList([_Down2D(cout)])


class _Encoder2D(nn.Module):
    def __init__(self, in_ch, latent, block_out, layers_per_block, groups):
        super().__init__()
        self.conv_in = nn.Conv2d(in_ch, block_out[0], 3, padding=1)
        blocks, prev = [], block_out[0]
        for i, ch in enumerate(block_out):
            blocks.append(_DownBlock2D(prev, ch, layers_per_block, groups, downsample=i != len(block_out) - 1))
            prev = ch
        self.down_blocks = nn.ModuleList(blocks)
        self.mid_block = _Mid2D(block_out[-1], groups)
        self.conv_norm_out = nn.GroupNorm(groups, block_out[-1], eps=1e-6)
        self.conv_out = nn.Conv2d(block_out[-1], 2 * latent, 3, padding=1)


class _CubicDown(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("kernel", torch.tensor(CUBIC2) / 2)


class _DownBlock1D(nn.Module):                     # diffusers DownBlock1D(out_channels, in_channels)
    def __init__(self, cin, cout):
        super().__init__()
        self.down = _CubicDown()
        self.resnets = nn.ModuleList([_ResConv(cin, cout, cout), _ResConv(cout, cout, cout), _ResConv(cout, cout, cout)])


class _Encoder1D(nn.Module):                       # network.py:86-185
    def __init__(self, in_ch, latent, block_out, groups):
        super().__init__()
        self.conv_in = nn.Conv1d(in_ch, block_out[0], 3, padding=1)
        blocks, prev = [], block_out[0]
        for ch in block_out:
            blocks.append(_DownBlock1D(prev, ch))
            prev = ch
        self.down_blocks = nn.ModuleList(blocks)
        self.mid_block = _Mid1D(block_out[-1])
        self.conv_norm_out = nn.GroupNorm(groups, block_out[-1], eps=1e-6)
        self.conv_out = nn.Conv1d(block_out[-1], 2 * latent, 3, padding=1)


class AutoencoderKLFastEncode(_HipVAE):
    """Surface-VAE encoder: points [F,3,32,32] -> posterior mode [F,3,4,4]  (network.py:861-945)."""

    def __init__(self, in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",),
                 up_block_types=("UpDecoderBlock2D",), block_out_channels=(64,), layers_per_block=1, act_fn="silu",
                 latent_channels=4, norm_num_groups=32, sample_size=32, scaling_factor=0.18215, force_upcast=True):
        super().__init__()
        self.block_out, self.latent, self.in_ch = tuple(block_out_channels), latent_channels, in_channels
        self.n_out = latent_channels      # columns of quant_conv the program writes: the mean (AutoencoderKL: all 2 * latent moments)
        self.encoder = _Encoder2D(in_channels, latent_channels, self.block_out, layers_per_block, norm_num_groups)
        self.quant_conv = nn.Conv2d(2 * latent_channels, 2 * latent_channels, 1)

    def _program(self, pg, P):
        pg.packs, e = P, self.encoder
        x = pg.conv(pg.input, e.conv_in, 3, 3)
        for blk in e.down_blocks:
            for r in blk.resnets:
                x = pg.resnet2d(x, r)
            if hasattr(blk, "downsamplers"):                  # Downsample2D: pad (0,1,0,1), conv 3x3 stride 2
                x2 = pg.conv(x, blk.downsamplers[0].conv, 3, 3, stride=2, pad_mode=1)
                pg.free(x)
                x = x2
        x = pg.resnet2d(x, e.mid_block.resnets[0])
        x = pg.attn(x, e.mid_block.attentions[0], 1, 1.0 / math.sqrt(self.block_out[-1]))
        x = pg.resnet2d(x, e.mid_block.resnets[1])
        x2 = pg.conv(x, e.conv_out, 3, 3, norm=e.conv_norm_out, act=ACT_SILU, pad16=128)
        pg.free(x)
        pg.conv(x2, self.quant_conv, 1, 1, dst=VAE_OUT, n_out=self.n_out)   # n_out = latent: DiagonalGaussianDistribution(moments).mode() = mean
        return pg

    def forward(self, x, return_dict=True):
        _check(x, "encode")
        x_cl = x.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()
        return self._encode_cl(x_cl).permute(0, 3, 1, 2).contiguous()

    def _encode_cl(self, x_cl):
        """Channels-last point grids [F,32,32,3] -> channels-last latent modes [F,4,4,3]."""
        dt = self._dtype()
        lat = x_cl.shape[1] >> (len(self.block_out) - 1)
        return self._run(x_cl, (lat, lat, self.n_out), dt)

    def encode_tokens(self, surfPnt):
        """Point grids [..., 32, 32, 3] (the datasets' layout) -> token-layout latents [..., 48]; equals trainer.py:519-524
        `vae(p.flatten(0,1).permute(0,3,1,2)).unflatten(0,(B,-1)).flatten(-2,-1).permute(0,1,3,2).flatten(-2,-1)` without
        the NCHW round trips."""
        _check(surfPnt, "encode")
        lead = surfPnt.shape[:-3]
        x_cl = surfPnt.detach().to(torch.float32).reshape(-1, *surfPnt.shape[-3:]).contiguous()
        z = self._encode_cl(x_cl)                                  # [F, 4, 4, latent]
        return z.reshape(*lead, z.shape[1] * z.shape[2] * z.shape[3])


class AutoencoderKL1DFastEncode(_HipVAE):
    """Edge-VAE encoder: points [G,3,32] -> posterior mode [G,3,4]  (network.py:690-783)."""

    def __init__(self, in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",),
                 up_block_types=("UpDecoderBlock2D",), block_out_channels=(64,), layers_per_block=1, act_fn="silu",
                 latent_channels=4, norm_num_groups=32, sample_size=32, scaling_factor=0.18215):
        super().__init__()
        self.block_out, self.latent, self.in_ch = tuple(block_out_channels), latent_channels, in_channels
        self.n_out = latent_channels      # (see AutoencoderKLFastEncode)
        self.encoder = _Encoder1D(in_channels, latent_channels, self.block_out, norm_num_groups)
        self.quant_conv = nn.Conv1d(2 * latent_channels, 2 * latent_channels, 1)

    def _program(self, pg, P):
        pg.packs, e = P, self.encoder
        x = pg.conv(pg.input, e.conv_in, 1, 3)
        for blk in e.down_blocks:
            x = pg.resample1d(x, VOP_DOWN1D)
            for r in blk.resnets:
                x = pg.resconv(x, r)
        c = self.block_out[-1]
        for r, at in zip(e.mid_block.resnets, e.mid_block.attentions):
            x = pg.resconv(x, r)
            x = pg.attn(x, at, c // 32, 1.0 / math.sqrt(32))
        x2 = pg.conv(x, e.conv_out, 1, 3, norm=e.conv_norm_out, act=ACT_SILU, pad16=128)
        pg.free(x)
        pg.conv(x2, self.quant_conv, 1, 1, dst=VAE_OUT, n_out=self.n_out)
        return pg

    def forward(self, sample, sample_posterior=False, return_dict=True, generator=None):
        _check(sample, "encode")
        x_cl = sample.detach().to(torch.float32).permute(0, 2, 1).contiguous()
        return self._encode_cl(x_cl).permute(0, 2, 1).contiguous()

    def _encode_cl(self, x_cl):
        """Channels-last polylines [G,32,3] -> channels-last latent modes [G,4,3]."""
        dt = self._dtype()
        return self._run(x_cl, (x_cl.shape[1] >> len(self.block_out), self.n_out), dt)

    def encode_tokens(self, edgePnt):
        """Polylines [..., 32, 3] -> token-layout latents [..., 12]; equals trainer.py:924-929
        `vae(p.flatten(0,1).flatten(0,1).permute(0,2,1)) ... .permute(0,1,2,4,3).flatten(-2,-1)`."""
        _check(edgePnt, "encode")
        lead = edgePnt.shape[:-2]
        x_cl = edgePnt.detach().to(torch.float32).reshape(-1, *edgePnt.shape[-2:]).contiguous()
        z = self._encode_cl(x_cl)                                  # [G, 4, latent]
        return z.reshape(*lead, z.shape[1] * z.shape[2])


# --------------------------------------------------------------------------------------------------
# full auto-encoders (what SurfVAETrainer / EdgeVAETrainer train, validate and save: trainer.py:20-30, 150-160)
# --------------------------------------------------------------------------------------------------
class AutoencoderKLOutput:
    def __init__(self, latent_dist):
        self.latent_dist = latent_dist


class DecoderOutput:
    def __init__(self, sample):
        self.sample = sample


def _to_ref(t_cl):
    """Channels-last [n, *spatial, C] -> the reference's [n, C, *spatial]."""
    return t_cl.movedim(-1, 1).contiguous()


def _to_cl(t):
    return t.movedim(1, -1).contiguous()


class DiagonalGaussianDistribution:
    """The posterior ``encode`` returns (diffusers' class of that name, network.py:513-514): ``parameters`` [n, 2L, ...] = mean | log-variance.

    ``sample`` and ``kl`` -- what the trainers call -- are ONE ``bg_vae_posterior`` launch on the channels-last moments the encode
    program wrote; the launch that samples also leaves the clamped log-variance and the KL behind, so ``kl()`` after ``sample()`` costs
    nothing.  ``mean`` / ``logvar`` / ``std`` / ``var`` are the reference's attributes for callers that read them (``logvar`` is the kernel's
    clamped output, ``std`` / ``var`` its exponentials); nothing on the package's own paths does."""

    def __init__(self, parameters, deterministic=False):
        if deterministic:
            raise NotImplementedError("BrepGen never builds a deterministic posterior")
        self._init_cl(_to_cl(parameters.detach().to(torch.float32)))

    @classmethod
    def _from_cl(cls, moments_cl):
        self = cls.__new__(cls)
        self._init_cl(moments_cl)
        return self

    def _init_cl(self, moments_cl):
        self._mom = moments_cl                                     # [n, *spatial, 2L] fp32
        self.latent = moments_cl.shape[-1] // 2
        self._lv_cl = self._kl = None

    def _launch(self, noise, seed, draw_id, first_sample):
        m = self._mom
        if not m.is_cuda:
            raise _lib.BrepgenHipError(f"brepgen_amd VAE posterior runs on the MI355X only (tensor on {m.device})")
        n, L = m.shape[0], self.latent
        P = math.prod(m.shape[1:-1])
        if noise is not None:
            if tuple(noise.shape) != (n, L, *m.shape[1:-1]):
                raise ValueError(f"noise has shape {tuple(noise.shape)}, the posterior's mean {(n, L, *m.shape[1:-1])}")
            noise = noise.detach().to(device=m.device, dtype=torch.float32).contiguous()
        z = torch.empty(*m.shape[:-1], L, device=m.device, dtype=torch.float32)
        lv, kl = torch.empty_like(z), torch.empty(n, device=m.device, dtype=torch.float32)
        check(_lib.load().bg_vae_posterior(ptr(m), ptr(noise), n, P, L, int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw_id) & 0xFFFFFFFF,
                                           int(first_sample), ptr(z), ptr(lv), ptr(kl), stream()), "bg_vae_posterior")
        self._lv_cl, self._kl = lv, kl                              # (neither depends on the noise)
        return z

    def _sample_cl(self, generator=None, noise=None, seed=None, draw_id=0, first_sample=0):
        if noise is None and seed is None:
            from .sampling import noise_key
            seed = noise_key(generator)
        return self._launch(noise, 0 if seed is None else seed, draw_id, first_sample)

    def sample(self, generator=None, *, noise=None, seed=None, draw_id=0, first_sample=0):
        """z = mean + std * eps, [n, L, ...].  ``noise`` [n, L, ...] given: it is eps (the parity mode -- the reference draws from the device's
        global RNG, which no other platform reproduces).  Otherwise the kernel draws eps itself: element e of row b is
        ``sampling.device_randn``'s value for (key, draw_id, first_sample + b, e), key = ``seed`` or else ``sampling.noise_key(generator)``
        -- the generator's STATE, which this call does not advance: successive draws under one key take successive ``draw_id``s.  A rank
        that owns rows [lo, hi) of a batch passes first_sample = lo and gets those rows of the single-GPU draw."""
        return _to_ref(self._sample_cl(generator, noise, seed, draw_id, first_sample))

    def mode(self):
        return self.mean

    def kl(self, other=None):
        """0.5 * sum(mean^2 + var - 1 - logvar) over every non-batch dimension, [n] (trainer.py:84; EdgeVAETrainer's hand-written
        sum over [1, 2], trainer.py:211-214, is the same quantity)."""
        if other is not None:
            raise NotImplementedError("BrepGen only takes the KL to N(0, I)")
        if self._kl is None:
            self._launch(None, 0, 0, 0)                             # (the draw is discarded: one launch yields z, logvar and kl)
        return self._kl

    @property
    def parameters(self):
        return _to_ref(self._mom)

    @property
    def mean(self):
        return _to_ref(self._mom[..., :self.latent])

    @property
    def logvar(self):
        if self._lv_cl is None:
            self._launch(None, 0, 0, 0)
        return _to_ref(self._lv_cl)

    @property
    def std(self):
        return torch.exp(0.5 * self.logvar)

    @property
    def var(self):
        return torch.exp(self.logvar)


def _on_runners(name):
    """An attribute of the full module that lives on its two program runners."""
    def get(self):
        return getattr(self._runners[0], name)

    def put(self, value):
        for r in self._runners:
            setattr(r, name, value)
    return property(get, put)


class _FullVAE(nn.Module):
    """encoder + quant_conv + post_quant_conv + decoder under the checkpoint's own keys.  The networks are not written again: the
    module owns one Fast encoder (widened to all 2 * latent moments) and one Fast decoder as its two program runners and registers
    THEIR sub-modules as its own, so a full checkpoint loads ``strict=True`` and ``state_dict()`` is what the Fast classes load."""
    _ENC = _DEC = None

    def _build(self, cfg):
        enc, dec = self._ENC(**cfg), self._DEC(**cfg)
        enc.n_out = 2 * enc.latent
        self.latent, self.in_ch = enc.latent, enc.in_ch
        self.encoder, self.quant_conv = enc.encoder, enc.quant_conv
        self.decoder, self.post_quant_conv = dec.decoder, dec.post_quant_conv
        self._runners = (enc, dec)                                   # (a tuple: not registered, no keys of their own)

    def _stale(self, workspaces):
        for r in self._runners:
            r._packs, r._programs = {}, {}
            if workspaces:
                r._ws = {}

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._stale(True)
        return out

    def load_state_dict(self, *a, **k):
        self._stale(False)
        return super().load_state_dict(*a, **k)

    def release_workspace(self):
        for r in self._runners:
            r.release_workspace()

    # switches of _HipVAE, set on both runners
    compute_dtype, WS_BUDGET, two_streams = _on_runners("compute_dtype"), _on_runners("WS_BUDGET"), _on_runners("two_streams")

    def _points_cl(self, x):
        """Points in the datasets' layout [..., (32,) 32, 3] or the trainers' permuted [n, 3, (32,) 32] -> (channels-last [N, (32,) 32, 3],
        restore), restore(y_cl) giving y in x's layout.  The last dimension decides: in_channels long = the datasets' layout."""
        _check(x, "encode")
        rank = self._RANK
        x = x.detach().to(torch.float32)
        if x.shape[-1] == self.in_ch and x.dim() >= rank + 1:
            lead = x.shape[:-(rank + 1)]
            return x.reshape(-1, *x.shape[-(rank + 1):]).contiguous(), lambda y: y.reshape(*lead, *y.shape[1:])
        if x.dim() != rank + 2 or x.shape[1] != self.in_ch:
            raise ValueError(f"{type(self).__name__}: points of shape {tuple(x.shape)}")
        return _to_cl(x), _to_ref

    def _encode_cl(self, x_cl):
        return DiagonalGaussianDistribution._from_cl(self._runners[0]._encode_cl(x_cl))

    def _decode_cl(self, z_cl):
        return self._runners[1]._decode_cl(z_cl)

    def encode(self, x, return_dict=True):
        _check(x, "encode")
        posterior = self._encode_cl(_to_cl(x.detach().to(torch.float32)))
        return AutoencoderKLOutput(posterior) if return_dict else (posterior,)

    def decode(self, z, return_dict=True):
        _check(z, "decode")
        dec = _to_ref(self._decode_cl(_to_cl(z.detach().to(torch.float32))))
        return DecoderOutput(dec) if return_dict else (dec,)

    def forward(self, sample, sample_posterior=False, return_dict=True, generator=None, *, noise=None):
        """network.py:660-687: encode, sample the posterior (or take its mode), decode -- the encode program, one bg_vae_posterior and the
        decode program on the current stream, channels-last in between."""
        _check(sample, "forward")
        posterior = self._encode_cl(_to_cl(sample.detach().to(torch.float32)))
        if sample_posterior:
            z_cl = posterior._sample_cl(generator, noise)
        else:
            z_cl = posterior._mom[..., :self.latent].contiguous()
        dec = _to_ref(self._decode_cl(z_cl))
        return DecoderOutput(dec) if return_dict else (dec,)


class AutoencoderKL(_FullVAE):
    """Surface VAE (trainer.py:20-30; network.py AutoencoderKL): points [F,3,32,32] <-> posterior over [F,3,4,4]."""
    _ENC, _DEC, _RANK = AutoencoderKLFastEncode, AutoencoderKLFastDecode, 2

    def __init__(self, in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",),
                 up_block_types=("UpDecoderBlock2D",), block_out_channels=(64,), layers_per_block=1, act_fn="silu",
                 latent_channels=4, norm_num_groups=32, sample_size=32, scaling_factor=0.18215, force_upcast=True):
        super().__init__()
        self._build(dict(in_channels=in_channels, out_channels=out_channels, down_block_types=down_block_types,
                         up_block_types=up_block_types, block_out_channels=block_out_channels, layers_per_block=layers_per_block,
                         act_fn=act_fn, latent_channels=latent_channels, norm_num_groups=norm_num_groups, sample_size=sample_size,
                         scaling_factor=scaling_factor, force_upcast=force_upcast))


class AutoencoderKL1D(_FullVAE):
    """Edge VAE (trainer.py:150-160; network.py AutoencoderKL1D): points [G,3,32] <-> posterior over [G,3,4]."""
    _ENC, _DEC, _RANK = AutoencoderKL1DFastEncode, AutoencoderKL1DFastDecode, 1

    def __init__(self, in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",),
                 up_block_types=("UpDecoderBlock2D",), block_out_channels=(64,), layers_per_block=1, act_fn="silu",
                 latent_channels=4, norm_num_groups=32, sample_size=32, scaling_factor=0.18215):
        super().__init__()
        self._build(dict(in_channels=in_channels, out_channels=out_channels, down_block_types=down_block_types,
                         up_block_types=up_block_types, block_out_channels=block_out_channels, layers_per_block=layers_per_block,
                         act_fn=act_fn, latent_channels=latent_channels, norm_num_groups=norm_num_groups, sample_size=sample_size,
                         scaling_factor=scaling_factor))
