"""CPU-side checks of the resampling convolutions in training (csrc/conv_train.hip: bg_conv_wgrad_geom, bg_conv_down_dgrad,
bg_conv_weight_pack_down, bg_pool2x2_sum; brepgen_amd/conv.py: conv_down, conv_up, the modules, use_device_blocks): the ABI boundary,
argument validation, the host-side split plan, the module swap, and the documented formulas (tests/resample_restate.py) against
torch.autograd in fp64.  No kernel is launched.  The entries are ADDED ones: BG_ABI_VERSION stays 7."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import brepgen_amd as bga
from brepgen_amd import _lib
from brepgen_amd import conv as CV
from brepgen_amd.vae import _Decoder2D, _DownBlock2D, _Encoder2D, _UpBlock2D
from tests import resample_ops as ops
from tests import resample_restate as R
from tests.conv_restate import pack_fwd, unpack_dw
from tests.train_cpu import BF, F16, F32, FAKE, assert_exported, explained, resource_usage, vp

NEW = ("bg_conv_wgrad_geom", "bg_conv_wgrad_geom_workspace_bytes", "bg_conv_wgrad_geom_split", "bg_conv_weight_pack_down",
       "bg_conv_down_dgrad_workspace_bytes", "bg_conv_down_dgrad", "bg_pool2x2_sum")
DOWN, UP = R.DOWN, R.UP


def test_entries_are_exported_with_the_declared_argtypes():
    assert_exported(NEW)
    i, z = C.c_int, C.c_size_t
    assert _lib._SIGNATURES["bg_conv_wgrad_geom"] == (i, [vp, i, vp, i, vp, vp] + [i] * 11 + [vp, z, vp])
    assert _lib._SIGNATURES["bg_conv_wgrad_geom_workspace_bytes"] == (z, [i] * 9)
    assert _lib._SIGNATURES["bg_conv_wgrad_geom_split"] == (i, [i] * 8)
    assert _lib._SIGNATURES["bg_conv_weight_pack_down"] == (i, [vp, i, i, i, vp, vp, i, vp])
    assert _lib._SIGNATURES["bg_conv_down_dgrad_workspace_bytes"] == (z, [i] * 5)
    assert _lib._SIGNATURES["bg_conv_down_dgrad"] == (i, [vp, i, vp, vp] + [i] * 6 + [vp, z, vp])
    assert _lib._SIGNATURES["bg_pool2x2_sum"] == (i, [vp, vp, vp, i, i, i, i, vp])
    assert (_lib.BG_CONV_SAME, _lib.BG_CONV_DOWN2, _lib.BG_CONV_UP2) == (0, 1, 2)
    for name in ("conv_down", "conv_up", "DeviceDownsample2D", "DeviceUpsample2D", "DeviceBlock2D", "use_device_blocks"):
        assert name in bga.__all__ and getattr(bga, name) is getattr(CV, name)


def _wgrad(dy=FAKE, ld_dy=128, a=FAKE, ld_a=128, dw=FAKE, db=FAKE, S=3, H=8, W=8, N=128, C=128, kh=3, kw=3, geom=DOWN, dtype=BF, out_dtype=F32,
           split=1, ws=None, ws_bytes=0):
    return _lib.load().bg_conv_wgrad_geom(dy, ld_dy, a, ld_a, dw, db, S, H, W, N, C, kh, kw, geom, dtype, out_dtype, split, ws, ws_bytes, None)


@pytest.mark.parametrize("geom", [DOWN, UP])
@pytest.mark.parametrize("kw, code, word", [
    (dict(N=192, ld_dy=192), _lib.BG_E_SHAPE, b"multiples of 128"),
    (dict(C=64), _lib.BG_E_SHAPE, b"multiples of 128"),
    (dict(N=0), _lib.BG_E_SHAPE, b"multiples of 128"),
    (dict(H=6), _lib.BG_E_SHAPE, b"powers of two"),
    (dict(W=0), _lib.BG_E_SHAPE, b"powers of two"),
    (dict(S=-1), _lib.BG_E_SHAPE, b"powers of two"),
    (dict(kh=1, kw=1), _lib.BG_E_SHAPE, b"window"),
    (dict(kh=5), _lib.BG_E_SHAPE, b"window"),
    (dict(kw=1), _lib.BG_E_SHAPE, b"window"),
    (dict(dy=FAKE + 8), _lib.BG_E_ALIGN, b"alignment"),
    (dict(dw=FAKE + 4), _lib.BG_E_ALIGN, b"alignment"),
    (dict(ld_a=132), _lib.BG_E_ALIGN, b"multiples of 8"),
    (dict(ld_dy=120), _lib.BG_E_ALIGN, b"ld_dy"),
    (dict(out_dtype=F16), _lib.BG_E_DTYPE, b"out_dtype"),
    (dict(dtype=F32), _lib.BG_E_DTYPE, b"operand dtype"),
    (dict(split=65), _lib.BG_E_ARG, b"split"),
    (dict(split=-1), _lib.BG_E_ARG, b"split"),
    (dict(split=3, ws=FAKE, ws_bytes=256), _lib.BG_E_ARG, b"workspace"),
    (dict(split=3), _lib.BG_E_ARG, b"workspace"),                       # NULL workspace
    (dict(dw=None), _lib.BG_E_ARG, b"null"),
    (dict(a=None), _lib.BG_E_ARG, b"null"),
    (dict(dy=None), _lib.BG_E_ARG, b"null"),
])
def test_wgrad_geom_argument_errors_are_negative_and_explained(kw, code, word, geom):
    explained(_wgrad(**{"geom": geom, **kw}), code, word)


def test_wgrad_geom_rules_of_its_own():
    explained(_wgrad(geom=3), _lib.BG_E_ARG, b"geom")
    explained(_wgrad(geom=-1), _lib.BG_E_ARG, b"geom")
    explained(_wgrad(geom=DOWN, H=1), _lib.BG_E_SHAPE, b"at least 2")           # DOWN2 halves the grid
    explained(_wgrad(geom=DOWN, W=1), _lib.BG_E_SHAPE, b"at least 2")
    explained(_wgrad(geom=UP, H=1, split=65), _lib.BG_E_ARG, b"split")          # UP2 takes a 1 x 1 grid: the next rule answers
    # geom = 0 is bg_conv_wgrad with its rules and its words: another window is its business, a 1 x 5 one passes on to the split rule
    explained(_wgrad(geom=0, kh=1, kw=5, split=65), _lib.BG_E_ARG, b"bg_conv_wgrad: split")
    explained(_wgrad(geom=0, kh=2), _lib.BG_E_SHAPE, b"bg_conv_wgrad: window")


def _dgrad(dy=FAKE, ld_dy=128, pack=FAKE, dx=FAKE, S=2, H=4, W=4, N=128, C=128, dtype=BF, ws=FAKE, ws_bytes=1 << 30):
    return _lib.load().bg_conv_down_dgrad(dy, ld_dy, pack, dx, S, H, W, N, C, dtype, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(N=192, ld_dy=192), _lib.BG_E_SHAPE, b"multiples of 128"),
    (dict(C=64), _lib.BG_E_SHAPE, b"multiples of 128"),
    (dict(H=6), _lib.BG_E_SHAPE, b"powers of two"),
    (dict(H=1), _lib.BG_E_SHAPE, b"at least 2"),
    (dict(W=1), _lib.BG_E_SHAPE, b"at least 2"),
    (dict(S=0), _lib.BG_E_SHAPE, b"samples"),
    (dict(dtype=F32), _lib.BG_E_DTYPE, b"operand dtype"),
    (dict(dy=None), _lib.BG_E_ARG, b"null"),
    (dict(pack=None), _lib.BG_E_ARG, b"null"),
    (dict(dx=None), _lib.BG_E_ARG, b"null"),
    (dict(ld_dy=120), _lib.BG_E_ALIGN, b"ld_dy"),
    (dict(ld_dy=132), _lib.BG_E_ALIGN, b"ld_dy"),
    (dict(dy=FAKE + 8), _lib.BG_E_ALIGN, b"alignment"),
    (dict(dx=FAKE + 4), _lib.BG_E_ALIGN, b"alignment"),
    (dict(ws=None), _lib.BG_E_ARG, b"workspace"),
    (dict(ws_bytes=1024), _lib.BG_E_ARG, b"workspace"),
])
def test_down_dgrad_argument_errors_are_negative_and_explained(kw, code, word):
    explained(_dgrad(**kw), code, word)


@pytest.mark.parametrize("args, code, word", [
    ((FAKE, F32, 128, 128, None, None, BF), _lib.BG_E_ARG, b"at least one output"),
    ((None, F32, 128, 128, None, FAKE, BF), _lib.BG_E_ARG, b"null"),
    ((FAKE, F32, 100, 128, None, FAKE, BF), _lib.BG_E_SHAPE, b"multiples of 32"),
    ((FAKE, F32, 128, 48, FAKE, None, BF), _lib.BG_E_SHAPE, b"multiples of 32"),
    ((FAKE + 2, BF, 128, 128, None, FAKE, BF), _lib.BG_E_ALIGN, b"alignment"),
    ((FAKE, F32, 128, 128, FAKE, FAKE + 8, BF), _lib.BG_E_ALIGN, b"alignment"),
    ((FAKE, F16, 128, 128, None, FAKE, BF), _lib.BG_E_DTYPE, b"source dtype"),
    ((FAKE, F32, 128, 128, None, FAKE, F32), _lib.BG_E_DTYPE, b"target dtype"),
])
def test_pack_down_argument_errors_are_negative_and_explained(args, code, word):
    explained(_lib.load().bg_conv_weight_pack_down(*args, None), code, word)


@pytest.mark.parametrize("args, code, word", [
    ((FAKE, None, FAKE, 2, 4, 4, 126), _lib.BG_E_SHAPE, b"multiple of 4"),
    ((FAKE, None, FAKE, 2, 4, 4, 0), _lib.BG_E_SHAPE, b"multiple of 4"),
    ((FAKE, None, FAKE, 0, 4, 4, 128), _lib.BG_E_SHAPE, b"samples"),
    ((FAKE, None, FAKE, 2, 0, 4, 128), _lib.BG_E_SHAPE, b"samples"),
    ((None, None, FAKE, 2, 4, 4, 128), _lib.BG_E_ARG, b"null"),
    ((FAKE, None, None, 2, 4, 4, 128), _lib.BG_E_ARG, b"null"),
    ((FAKE + 4, None, FAKE, 2, 4, 4, 128), _lib.BG_E_ALIGN, b"alignment"),
    ((FAKE, FAKE + 8, FAKE, 2, 4, 4, 128), _lib.BG_E_ALIGN, b"alignment"),
])
def test_pool_argument_errors_are_negative_and_explained(args, code, word):
    explained(_lib.load().bg_pool2x2_sum(*args, None), code, word)


# (S, H, W, N, C, geom): the SurfVAE trainer's six resampling convolutions at its batch of 512, and the GPU tests' small ones
SHAPES = ((512, 32, 32, 128, 128, DOWN), (512, 16, 16, 256, 256, DOWN), (512, 8, 8, 512, 512, DOWN), (512, 4, 4, 512, 512, UP),
          (512, 8, 8, 512, 512, UP), (512, 16, 16, 256, 256, UP), (1, 2, 2, 128, 128, DOWN), (3, 4, 4, 128, 256, DOWN), (2, 8, 8, 256, 128, DOWN),
          (2, 2, 8, 128, 128, DOWN), (1, 1, 1, 128, 128, UP), (3, 2, 2, 128, 256, UP), (2, 4, 4, 256, 128, UP), (2, 1, 4, 128, 128, UP))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_plan_and_workspace_are_consistent(shape):
    S, H, W, N, Cc, geom = shape
    Ho, Wo = R.out_grid(H, W, geom)
    M, K = S * Ho * Wo, 9 * Cc                                                # M from the OUTPUT grid
    sp = ops.auto_split(*shape)
    assert 1 <= sp <= 64
    assert sp == _lib.load().bg_linear_wgrad_split(M, N, K)
    steps = (M + 31) // 32
    rows = (steps + sp - 1) // sp * 32
    assert (sp - 1) * rows < M                                                # no empty slice
    assert ops.workspace_bytes(*shape, 0) == ops.workspace_formula(N, K, sp)
    for forced in (1, 2, 3, 64):
        assert ops.workspace_bytes(*shape, forced) == ops.workspace_formula(N, K, forced)
    assert ops.workspace_bytes(*shape, 65) == 0
    assert ops.workspace_bytes(S, H, W, N + 1, Cc, geom, 2) == 0 and ops.auto_split(S, 3, W, N, Cc, geom) == 1
    assert ops.workspace_bytes(S, H, W, N, Cc, geom, 2, kh=1, kw=5) == 0 and ops.workspace_bytes(S, H, W, N, Cc, 3, 2) == 0
    # geom = 0 is bg_conv_wgrad's plan
    lib = _lib.load()
    assert ops.auto_split(S, H, W, N, Cc, 0) == lib.bg_conv_wgrad_split(S, H, W, N, Cc, 3, 3)
    assert ops.workspace_bytes(S, H, W, N, Cc, 0, 0) == lib.bg_conv_wgrad_workspace_bytes(S, H, W, N, Cc, 3, 3, 0)


def test_down_plan_needs_a_grid_to_halve_and_dgrad_workspace_formula():
    assert ops.auto_split(512, 1, 8, 128, 128, DOWN) == 1 and ops.workspace_bytes(512, 1, 8, 128, 128, DOWN, 2) == 0
    al = lambda v: (v + 255) // 256 * 256
    lib = _lib.load()
    for S, H, W, N, Cc in ((2, 4, 4, 128, 256), (3, 2, 2, 128, 128), (4, 32, 32, 128, 128), (512, 32, 32, 128, 128), (1, 2, 8, 256, 128)):
        M = S * (H // 2) * (W // 2)
        assert lib.bg_conv_down_dgrad_workspace_bytes(S, H, W, N, Cc) == 2 * al(4 * M * N) + al(8 * M * N) + al(16 * M * Cc)
    assert lib.bg_conv_down_dgrad_workspace_bytes(2, 1, 4, 128, 128) == 0 and lib.bg_conv_down_dgrad_workspace_bytes(2, 4, 4, 128, 64) == 0


@pytest.mark.parametrize("geom, H, W", [(DOWN, 2, 2), (DOWN, 4, 4), (DOWN, 2, 8), (UP, 1, 1), (UP, 2, 2), (UP, 1, 4)])
def test_restatement_equals_autograd(geom, H, W):
    g = torch.Generator().manual_seed(3 * H + W + geom)
    S, N, Cc = 2, 6, 5
    Ho, Wo = R.out_grid(H, W, geom)
    w = torch.randn(N, Cc, 3, 3, generator=g, dtype=torch.float64).requires_grad_()
    b = torch.randn(N, generator=g, dtype=torch.float64).requires_grad_()
    x = torch.randn(S, Cc, H, W, generator=g, dtype=torch.float64).requires_grad_()
    dy = torch.randn(S, N, Ho, Wo, generator=g, dtype=torch.float64)
    y = ops.torch_fwd(x, w, b, geom)
    assert y.shape == (S, N, Ho, Wo)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), dy)
    x_cl, dy_cl, wd = x.detach().permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1), w.detach()
    close = lambda p, q: torch.allclose(p, q, rtol=1e-12, atol=1e-12)
    assert close(R.fwd(x_cl, wd, b.detach(), geom), y.detach().permute(0, 2, 3, 1))
    dwp, rb = R.wgrad(dy_cl, x_cl, geom)
    assert dwp.shape == (N, 9 * Cc) and close(unpack_dw(dwp, 3, 3), dw) and close(rb, db)
    assert torch.equal(pack_fwd(unpack_dw(dwp, 3, 3)), dwp)                   # the forward pack's layout
    if geom == DOWN:
        pack = R.pack_down(wd)
        assert pack.shape == (9 * Cc * N,)
        assert close(R.down_dgrad(dy_cl, pack, Cc), dx.permute(0, 2, 3, 1))
    else:
        assert close(R.up_dgrad(dy_cl, wd), dx.permute(0, 2, 3, 1))


def test_restated_class_ordered_pack_and_pool():
    g = torch.Generator().manual_seed(9)
    N, Cc = 4, 3
    w = torch.randn(N, Cc, 3, 3, generator=g, dtype=torch.float64)
    pack = R.pack_down(w)
    # block k starts at C * N * {0, 1, 3, 5}; block[c, t, n] = w[n, c, tap_k[t]]
    starts = [0, 1, 3, 5]
    assert [len(t) for t in R.CLASS_TAPS] == [1, 2, 2, 4] and sorted(t for ts in R.CLASS_TAPS for t in ts) == R.TAPS
    for k, taps in enumerate(R.CLASS_TAPS):
        blk = pack[starts[k] * Cc * N:(starts[k] + len(taps)) * Cc * N].reshape(Cc, len(taps), N)
        for t, (ky, kx) in enumerate(taps):
            assert torch.equal(blk[:, t], w[:, :, ky, kx].t())
            assert (ky % 2, kx % 2) == R.CLASS_PARITY[k]                      # tap 1 meets odd coordinates, taps 0 and 2 even ones
    # the 2 x 2 sum is the backward of nearest x2 up-sampling
    x = torch.randn(2, 3, 2, 4, generator=g, dtype=torch.float64).requires_grad_()
    du = torch.randn(2, 3, 4, 8, generator=g, dtype=torch.float64)
    (dx,) = torch.autograd.grad(torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest"), x, du)
    cl = lambda t: t.permute(0, 2, 3, 1)
    assert torch.allclose(R.pool2x2(cl(du)), cl(dx), rtol=1e-12, atol=1e-12)
    add = torch.randn(2, 2, 4, 3, generator=g, dtype=torch.float64)
    assert torch.equal(R.pool2x2(cl(du), add), R.pool2x2(cl(du)) + add)


def _ids(m):
    return {k: id(p) for k, p in m.named_parameters()}


def test_use_device_blocks_keeps_parameter_identity_key_order_and_is_idempotent():
    enc, dec = _Encoder2D(3, 3, (128, 256), 2, 32), _Decoder2D(3, 3, (128, 256), 2, 32)
    for m in (enc, dec):
        before, keys = _ids(m), list(m.state_dict())
        kept = {n: getattr(m, n) for n in ("conv_in", "mid_block", "conv_norm_out", "conv_out")}
        assert bga.use_device_blocks(m) is m
        assert _ids(m) == before and list(m.state_dict()) == keys
        blocks = list(m.down_blocks if m is enc else m.up_blocks)
        bga.use_device_blocks(m)                                              # idempotent
        assert _ids(m) == before and list(m.state_dict()) == keys
        assert all(p is q for p, q in zip(blocks, m.down_blocks if m is enc else m.up_blocks))
        assert all(getattr(m, n) is v for n, v in kept.items())               # left alone (the mid block's resnets: use_device_resnets)
        assert type(m.conv_in) is nn.Conv2d and type(m.conv_out) is nn.Conv2d and type(m.conv_norm_out) is nn.GroupNorm
        assert all(isinstance(r, CV.DeviceResnetBlock2D) for r in m.mid_block.resnets) and not isinstance(m.mid_block, CV.DeviceBlock2D)
    assert all(isinstance(b, CV.DeviceBlock2D) for b in list(enc.down_blocks) + list(dec.up_blocks))
    assert isinstance(enc.down_blocks[0].downsamplers[0], CV.DeviceDownsample2D) and not hasattr(enc.down_blocks[1], "downsamplers")
    assert isinstance(dec.up_blocks[0].upsamplers[0], CV.DeviceUpsample2D) and not hasattr(dec.up_blocks[1], "upsamplers")
    assert all(isinstance(r, CV.DeviceResnetBlock2D) for b in list(enc.down_blocks) + list(dec.up_blocks) for r in b.resnets)
    assert not hasattr(enc.down_blocks[0], "upsamplers")


def test_use_device_blocks_on_a_block_and_what_it_leaves_alone():
    for blk, name in ((_DownBlock2D(128, 256, 2, 32, True), "downsamplers"), (_UpBlock2D(256, 128, 3, 32, True), "upsamplers")):
        before, keys = _ids(blk), list(blk.state_dict())
        dev = bga.use_device_blocks(blk)
        assert isinstance(dev, CV.DeviceBlock2D) and _ids(dev) == before and list(dev.state_dict()) == keys
        assert isinstance(getattr(dev, name)[0], CV._SAMPLERS[name]) and bga.use_device_blocks(dev) is dev
    # a 1 x 1 convolution among the downsamplers, a stride-1 one, an up-sampler with padding 0: left alone, and so is their block
    class Odd(nn.Module):
        def __init__(self, conv):
            super().__init__()
            self.conv = conv

    for name, conv in (("downsamplers", nn.Conv2d(128, 128, 1, stride=2)), ("downsamplers", nn.Conv2d(128, 128, 3, stride=1, padding=0)),
                       ("downsamplers", nn.Conv2d(128, 128, 3, stride=2, padding=1)), ("upsamplers", nn.Conv2d(128, 128, 3, padding=0)),
                       ("upsamplers", nn.Conv2d(128, 128, 3, stride=2, padding=1))):
        blk = _DownBlock2D(128, 128, 1, 32, False)
        odd = Odd(conv)
        setattr(blk, name, nn.ModuleList([odd]))
        holder = nn.ModuleList([blk])
        bga.use_device_blocks(holder)
        assert holder[0] is blk and getattr(blk, name)[0] is odd and isinstance(blk.resnets[0], CV.DeviceResnetBlock2D)
    # extra parameters beside conv: not a sampler
    extra = Odd(nn.Conv2d(128, 128, 3, stride=2))
    extra.scale = nn.Parameter(torch.ones(1))
    blk = _DownBlock2D(128, 128, 1, 32, False)
    blk.downsamplers = nn.ModuleList([extra])
    bga.use_device_blocks(nn.ModuleList([blk]))
    assert blk.downsamplers[0] is extra
    # use_device_resnets still leaves the samplers alone
    up = bga.use_device_resnets(_UpBlock2D(256, 128, 2, 32, True))
    assert not isinstance(up.upsamplers[0], CV.DeviceUpsample2D)


def test_python_surface_raises_without_a_device_and_on_bad_arguments():
    """argument rules first, then the device (the call outside autocast needs one: tests/test_gpu_conv_resample.py)"""
    x = torch.zeros(2, 4, 4, 128)
    down, up = nn.Conv2d(128, 128, 3, stride=2), nn.Conv2d(128, 128, 3, padding=1)
    assert sorted(CV.DeviceDownsample2D(128).state_dict()) == ["conv.bias", "conv.weight"] == sorted(CV.DeviceUpsample2D(128).state_dict())
    assert CV.DeviceDownsample2D(128).conv.stride == (2, 2) and CV.DeviceDownsample2D(128).conv.padding == (0, 0)
    assert CV.DeviceUpsample2D(256).conv.stride == (1, 1) and CV.DeviceUpsample2D(256).conv.padding == (1, 1)
    for cls in (CV.DeviceDownsample2D, CV.DeviceUpsample2D):
        with pytest.raises(ValueError, match="multiple of 128"):
            cls(96)
    with pytest.raises(ValueError, match="not both"):
        CV.DeviceBlock2D([], [], [])
    with pytest.raises(_lib.BrepgenHipError):
        CV.conv_down(x, down)                                                  # CPU tensors: no fallback
    with pytest.raises(_lib.BrepgenHipError):
        CV.conv_up(x, up)
    with pytest.raises(_lib.BrepgenHipError):
        CV.DeviceBlock2D([], [CV.DeviceDownsample2D(128)])(x)
    with pytest.raises(ValueError, match="stride"):
        CV.conv_down(x, up)
    with pytest.raises(ValueError, match="stride"):
        CV.conv_up(x, down)
    with pytest.raises(ValueError, match="padding"):
        CV.conv_down(x, nn.Conv2d(128, 128, 3, stride=2, padding=1))
    with pytest.raises(ValueError, match="window"):
        CV.conv_up(x, nn.Conv2d(128, 128, 5, padding=2))
    with pytest.raises(ValueError, match="powers of two"):
        CV.conv_down(torch.zeros(2, 6, 4, 128), down)
    with pytest.raises(ValueError, match="at least 2"):
        CV.conv_down(torch.zeros(2, 1, 4, 128), down)
    with pytest.raises(ValueError, match="powers of two"):
        CV.conv_up(torch.zeros(2, 4, 12, 128), up)
    with pytest.raises(ValueError, match="multiples of 128"):
        CV.conv_up(torch.zeros(2, 4, 4, 64), nn.Conv2d(64, 128, 3, padding=1))
    with pytest.raises(ValueError, match="channels"):
        CV.conv_down(torch.zeros(2, 4, 4, 256), down)
    with pytest.raises(ValueError, match="fp32"):
        CV.conv_up(x.half(), up)
    with pytest.raises(ValueError, match="Conv2d"):
        CV.conv_down(x, nn.Conv1d(128, 128, 3))
    with pytest.raises(ValueError, match="channels-last"):
        CV.conv_up(torch.zeros(2, 8, 128), up)


def test_resampling_kernels_do_not_spill():
    """the new kernels of conv_train.hip: the two geometries of the tile kernel (6 instantiations each), the class-ordered pack (3), the
    gather, the interleave and the 2 x 2 sum"""
    names, scratch, spills, _ = resource_usage("conv_train.hip")
    geom = [n for n in names if "cw_wgrad_kernel" in n]
    assert len(geom) == 18, geom                                              # 6 of round 18 + 2 x 6
    for word, count in (("cd_pack_kernel", 3), ("cd_gather_kernel", 1), ("cd_interleave_kernel", 1), ("pool2x2_sum_kernel", 1)):
        assert sum(word in n for n in names) == count, (word, names)
    assert all(v == 0 for v in scratch + spills), list(zip(names, scratch, spills))
