"""CPU-side checks of the conv-layer backward (csrc/conv_train.hip, brepgen_amd/conv.py): the ABI boundary, argument validation, the
host-side split plan, the module swap, and the documented formulas (tests/conv_restate.py) against torch.autograd in fp64.  No kernel is
launched.  The entries are ADDED ones: BG_ABI_VERSION stays 7 (see tests/test_linear_bwd_cpu.py)."""
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import brepgen_amd as bga
from brepgen_amd import _lib
from brepgen_amd import conv as CV
from brepgen_amd.vae import _UpBlock2D
from tests import conv_ops as ops
from tests import conv_restate as R
from tests.train_cpu import BF, F16, F32, FAKE, assert_exported, explained, resource_usage, vp

NEW = ("bg_conv_wgrad", "bg_conv_wgrad_workspace_bytes", "bg_conv_wgrad_split", "bg_conv_weight_pack", "bg_gn_act_bwd_workspace_bytes",
       "bg_gn_act_bwd")


def test_entries_are_exported_with_the_declared_argtypes():
    assert_exported(NEW)
    i, z = C.c_int, C.c_size_t
    assert _lib._SIGNATURES["bg_conv_wgrad"] == (i, [vp, i, vp, i, vp, vp] + [i] * 10 + [vp, z, vp])
    assert _lib._SIGNATURES["bg_conv_wgrad_workspace_bytes"] == (z, [i] * 8)
    assert _lib._SIGNATURES["bg_conv_wgrad_split"] == (i, [i] * 7)
    assert _lib._SIGNATURES["bg_conv_weight_pack"] == (i, [vp, i, i, i, i, i, vp, vp, i, vp])
    assert _lib._SIGNATURES["bg_gn_act_bwd_workspace_bytes"] == (z, [i] * 4)
    assert _lib._SIGNATURES["bg_gn_act_bwd"] == (i, [vp] * 9 + [i] * 5 + [vp, z, vp])
    from brepgen_amd import build as b
    assert "conv_train.hip" in b.SOURCES


def _wgrad(dy=FAKE, ld_dy=128, a=FAKE, ld_a=128, dw=FAKE, db=FAKE, S=3, H=8, W=8, N=128, C=128, kh=3, kw=3, dtype=BF, out_dtype=F32, split=1,
           ws=None, ws_bytes=0):
    return _lib.load().bg_conv_wgrad(dy, ld_dy, a, ld_a, dw, db, S, H, W, N, C, kh, kw, dtype, out_dtype, split, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(N=192, ld_dy=192), _lib.BG_E_SHAPE, b"multiples of 128"),
    (dict(C=64), _lib.BG_E_SHAPE, b"multiples of 128"),
    (dict(N=0), _lib.BG_E_SHAPE, b"multiples of 128"),
    (dict(H=6), _lib.BG_E_SHAPE, b"powers of two"),
    (dict(W=0), _lib.BG_E_SHAPE, b"powers of two"),
    (dict(S=-1), _lib.BG_E_SHAPE, b"powers of two"),
    (dict(kh=2), _lib.BG_E_SHAPE, b"window"),
    (dict(kw=7), _lib.BG_E_SHAPE, b"window"),
    (dict(kh=0), _lib.BG_E_SHAPE, b"window"),
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
])
def test_wgrad_argument_errors_are_negative_and_explained(kw, code, word):
    explained(_wgrad(**kw), code, word)


@pytest.mark.parametrize("args, code, word", [
    ((FAKE, F32, 128, 128, 3, 3, None, None, BF), _lib.BG_E_ARG, b"at least one output"),
    ((None, F32, 128, 128, 3, 3, FAKE, None, BF), _lib.BG_E_ARG, b"null"),
    ((FAKE, F32, 100, 128, 3, 3, FAKE, None, BF), _lib.BG_E_SHAPE, b"multiples of 32"),
    ((FAKE, F32, 128, 48, 3, 3, FAKE, None, BF), _lib.BG_E_SHAPE, b"multiples of 32"),
    ((FAKE, F32, 128, 128, 3, 4, FAKE, None, BF), _lib.BG_E_SHAPE, b"window"),
    ((FAKE, F32, 128, 128, 7, 1, FAKE, None, BF), _lib.BG_E_SHAPE, b"window"),
    ((FAKE + 2, BF, 128, 128, 3, 3, FAKE, None, BF), _lib.BG_E_ALIGN, b"alignment"),
    ((FAKE, F32, 128, 128, 3, 3, FAKE, FAKE + 8, BF), _lib.BG_E_ALIGN, b"alignment"),
    ((FAKE, F16, 128, 128, 3, 3, FAKE, None, BF), _lib.BG_E_DTYPE, b"source dtype"),
    ((FAKE, F32, 128, 128, 3, 3, FAKE, None, F32), _lib.BG_E_DTYPE, b"target dtype"),
])
def test_weight_pack_argument_errors_are_negative_and_explained(args, code, word):
    explained(_lib.load().bg_conv_weight_pack(*args, None), code, word)


def _gn(da=FAKE, x=FAKE, stats=FAKE, gamma=FAKE, beta=FAKE, dskip=None, dx=FAKE, dgamma=FAKE, dbeta=FAKE, S=2, P=16, C=128, G=32, act=1,
        ws=FAKE, ws_bytes=1 << 30):
    return _lib.load().bg_gn_act_bwd(da, x, stats, gamma, beta, dskip, dx, dgamma, dbeta, S, P, C, G, act, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(C=126), _lib.BG_E_SHAPE, b"multiple of 4"),
    (dict(G=24), _lib.BG_E_SHAPE, b"multiple of 4"),
    (dict(G=0), _lib.BG_E_SHAPE, b"multiple of 4"),
    (dict(P=0), _lib.BG_E_SHAPE, b"positions"),
    (dict(S=0), _lib.BG_E_SHAPE, b"samples"),
    (dict(S=70000), _lib.BG_E_SHAPE, b"samples"),
    (dict(act=3), _lib.BG_E_ARG, b"act"),
    (dict(da=None), _lib.BG_E_ARG, b"null"),
    (dict(dx=None), _lib.BG_E_ARG, b"null"),
    (dict(dgamma=None), _lib.BG_E_ARG, b"both or neither"),
    (dict(x=FAKE + 4), _lib.BG_E_ALIGN, b"alignment"),
    (dict(dskip=FAKE + 8), _lib.BG_E_ALIGN, b"alignment"),
    (dict(stats=FAKE + 4), _lib.BG_E_ALIGN, b"alignment"),
    (dict(ws=None), _lib.BG_E_ARG, b"workspace"),
    (dict(ws_bytes=1024), _lib.BG_E_ARG, b"workspace"),
])
def test_gn_act_bwd_argument_errors_are_negative_and_explained(kw, code, word):
    explained(_gn(**kw), code, word)


def test_gn_act_bwd_workspace_formula():
    al = lambda v: (v + 255) // 256 * 256
    for S, P, Cc, G in ((1, 1, 128, 32), (3, 16, 128, 32), (5, 65, 256, 32), (512, 1024, 128, 32), (2, 8, 12, 3)):
        want = al(S * ((P + 63) // 64) * 3 * Cc * 8) + al(S * 3 * Cc * 8) + al(S * G * 4 * 4)
        assert _lib.load().bg_gn_act_bwd_workspace_bytes(S, P, Cc, G) == want
    assert _lib.load().bg_gn_act_bwd_workspace_bytes(2, 8, 126, 1) == 0 and _lib.load().bg_gn_act_bwd_workspace_bytes(0, 8, 128, 1) == 0


SHAPES = ((1, 4, 4, 128, 128, 3, 3), (3, 4, 4, 128, 256, 3, 3), (2, 8, 8, 256, 128, 3, 3), (3, 1, 8, 128, 128, 1, 5), (2, 2, 2, 128, 128, 3, 3),
          (512, 32, 32, 128, 128, 3, 3), (512, 8, 8, 512, 512, 3, 3), (512, 4, 4, 512, 512, 3, 3), (512, 1, 32, 256, 256, 1, 5))


@pytest.mark.parametrize("shape", SHAPES)
def test_split_plan_and_workspace_are_consistent(shape):
    S, H, W, N, Cc, kh, kw = shape
    M, K = S * H * W, kh * kw * Cc
    sp = ops.auto_split(*shape)
    assert 1 <= sp <= 64
    assert sp == _lib.load().bg_linear_wgrad_split(M, N, K)                 # the Linear entry's plan on the same M, N, K
    steps = (M + 31) // 32
    rows = (steps + sp - 1) // sp * 32
    assert (sp - 1) * rows < M                                              # no empty slice
    assert ops.workspace_bytes(*shape, 0) == ops.workspace_formula(N, K, sp)
    for forced in (1, 2, 3, 64):
        assert ops.workspace_bytes(*shape, forced) == ops.workspace_formula(N, K, forced)
    assert ops.workspace_bytes(*shape, 65) == 0
    assert ops.workspace_bytes(S, H, W, N + 1, Cc, kh, kw, 2) == 0 and ops.auto_split(S, 3, W, N, Cc, kh, kw) == 1


@pytest.mark.parametrize("act", ["none", "silu", "gelu"])
@pytest.mark.parametrize("S, P, Cc, G", [(2, 6, 16, 4), (3, 5, 8, 1), (1, 1, 12, 3)])
def test_restated_gn_act_backward_equals_autograd(act, S, P, Cc, G):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(S, P, Cc, generator=g, dtype=torch.float64) * 2 + 3).requires_grad_()
    gamma = (1 + 0.3 * torch.randn(Cc, generator=g, dtype=torch.float64)).requires_grad_()
    beta = (0.3 * torch.randn(Cc, generator=g, dtype=torch.float64)).requires_grad_()
    da = torch.randn(S, P, Cc, generator=g, dtype=torch.float64)
    dskip = torch.randn(S, P, Cc, generator=g, dtype=torch.float64)
    v = F.group_norm(x.permute(0, 2, 1), G, gamma, beta, 1e-6).permute(0, 2, 1)
    a = {"none": lambda t: t, "silu": F.silu, "gelu": F.gelu}[act](v)
    assert torch.allclose(R.gn_act(x.detach(), gamma.detach(), beta.detach(), G, 1e-6, act), a.detach(), rtol=1e-12, atol=1e-12)
    dx, dg, db = torch.autograd.grad(a, (x, gamma, beta), da)
    rx, rg, rb = R.gn_act_bwd(da, x.detach(), gamma.detach(), beta.detach(), G, 1e-6, act)
    assert torch.allclose(rx, dx, rtol=1e-10, atol=1e-11) and torch.allclose(rg, dg, rtol=1e-10, atol=1e-11)
    assert torch.allclose(rb, db, rtol=1e-10, atol=1e-11)
    assert torch.equal(R.gn_act_bwd(da, x.detach(), gamma.detach(), beta.detach(), G, 1e-6, act, dskip)[0], rx + dskip)


@pytest.mark.parametrize("kh, kw", [(3, 3), (1, 5), (1, 1)])
def test_restated_packs_and_layouts_equal_autograd(kh, kw):
    g = torch.Generator().manual_seed(7)
    S, H, W, N, Cc = 2, (1 if kh == 1 else 4), 8, 6, 5
    w = torch.randn(N, Cc, kh, kw, generator=g, dtype=torch.float64).requires_grad_()
    x = torch.randn(S, Cc, H, W, generator=g, dtype=torch.float64).requires_grad_()
    dy = torch.randn(S, N, H, W, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, padding=(kh // 2, kw // 2))
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    x_cl, dy_cl = x.detach().permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1)
    # the forward pack is the forward's weight
    assert torch.allclose(R.conv_same(x_cl, R.pack_fwd(w.detach()), kh, kw), y.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    # a 'same' forward convolution of dy with the reversed-tap pack is the data gradient
    assert torch.allclose(R.conv_same(dy_cl, R.pack_dgrad(w.detach()), kh, kw), dx.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    # the tap-major dw permutes to autograd's weight gradient; db is the pixel sum
    dwp, db = R.wgrad(dy_cl, x_cl, kh, kw)
    assert dwp.shape == (N, kh * kw * Cc)
    assert torch.allclose(R.unpack_dw(dwp, kh, kw), dw, rtol=1e-12, atol=1e-12)
    assert torch.allclose(db, dy.sum((0, 2, 3)), rtol=1e-12, atol=1e-12)
    # and it is the layout of the forward pack
    assert torch.equal(R.pack_fwd(R.unpack_dw(dwp, kh, kw)), dwp)


def _ref_block(cin, cout):
    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.norm1, self.conv1 = nn.GroupNorm(32, cin, eps=1e-6), nn.Conv2d(cin, cout, 3, padding=1)
            self.norm2, self.conv2 = nn.GroupNorm(32, cout, eps=1e-6), nn.Conv2d(cout, cout, 3, padding=1)
            self.nonlinearity, self.dropout = nn.SiLU(), nn.Dropout(0.0)
            if cin != cout:
                self.conv_shortcut = nn.Conv2d(cin, cout, 1)
    return Block()


def test_use_device_resnets_keeps_parameter_identity_and_state_dict_keys():
    seq = nn.Sequential(_ref_block(128, 128), _ref_block(128, 256), nn.Conv2d(256, 256, 3, padding=1))
    up = _UpBlock2D(256, 128, 2, 32, True)
    for m in (seq, up):
        before = {k: id(p) for k, p in m.named_parameters()}
        keys = list(m.state_dict())
        assert bga.use_device_resnets(m) is m
        assert {k: id(p) for k, p in m.named_parameters()} == before and list(m.state_dict()) == keys
        bga.use_device_resnets(m)                                             # idempotent
        assert {k: id(p) for k, p in m.named_parameters()} == before
    assert isinstance(seq[0], CV.DeviceResnetBlock2D) and isinstance(seq[1], CV.DeviceResnetBlock2D) and type(seq[2]) is nn.Conv2d
    assert hasattr(seq[1], "conv_shortcut") and not hasattr(seq[0], "conv_shortcut")
    assert all(isinstance(r, CV.DeviceResnetBlock2D) for r in up.resnets) and not isinstance(up.upsamplers[0], CV.DeviceResnetBlock2D)
    # other structures are left alone: a time-embedding projection, a strided block
    odd = _ref_block(128, 128)
    odd.time_emb_proj = nn.Linear(16, 128)
    holder = nn.ModuleList([odd])
    bga.use_device_resnets(holder)
    assert holder[0] is odd
    assert bga.gn_act_conv is CV.gn_act_conv and bga.DeviceResnetBlock2D is CV.DeviceResnetBlock2D


def test_python_surface_raises_without_a_device_and_on_bad_arguments():
    """argument rules first, then the device (the call outside autocast needs one: tests/test_gpu_conv_train.py)"""
    x = torch.zeros(2, 4, 4, 128)
    norm, conv = nn.GroupNorm(32, 128), nn.Conv2d(128, 128, 3, padding=1)
    blk = CV.DeviceResnetBlock2D(128, 256)
    assert sorted(k.split(".")[0] for k in blk.state_dict()) == sorted(["conv1", "conv2", "conv_shortcut", "norm1", "norm2"] * 2)
    with pytest.raises(ValueError):
        CV.DeviceResnetBlock2D(96, 128)
    with pytest.raises(_lib.BrepgenHipError):
        CV.gn_act_conv(x, norm, conv)                                          # CPU tensors: no fallback
    with pytest.raises(_lib.BrepgenHipError):
        blk(x)
    with pytest.raises(ValueError, match="stride"):
        CV.gn_act_conv(x, norm, nn.Conv2d(128, 128, 3, padding=1, stride=2))
    with pytest.raises(ValueError, match="powers of two"):
        CV.gn_act_conv(torch.zeros(2, 6, 4, 128), norm, conv)
    with pytest.raises(ValueError, match="powers of two"):
        blk(torch.zeros(2, 4, 12, 128))
    with pytest.raises(ValueError, match="multiples of 128"):
        CV.gn_act_conv(torch.zeros(2, 4, 4, 64), nn.GroupNorm(32, 64), nn.Conv2d(64, 128, 3, padding=1))
    with pytest.raises(ValueError, match="multiples of 128"):
        CV.gn_act_conv(x, norm, nn.Conv2d(128, 192, 3, padding=1))
    with pytest.raises(ValueError, match="padding"):
        CV.gn_act_conv(x, norm, nn.Conv2d(128, 128, 3, padding=0))
    with pytest.raises(ValueError, match="window"):
        CV.gn_act_conv(x, norm, nn.Conv2d(128, 128, 7, padding=3))
    with pytest.raises(ValueError, match="Conv1d"):
        CV.gn_act_conv(torch.zeros(2, 8, 128), None, conv)
    with pytest.raises(ValueError, match="act"):
        CV.gn_act_conv(x, norm, conv, act="relu")
    with pytest.raises(ValueError, match="channels"):
        CV.gn_act_conv(x, nn.GroupNorm(32, 256), conv)
    with pytest.raises(ValueError, match="fp32"):
        CV.gn_act_conv(x.half(), norm, conv)
    with pytest.raises(ValueError, match="res"):
        CV.gn_act_conv(x, norm, conv, res=torch.zeros(2, 4, 4, 64))


def test_conv_train_kernels_do_not_spill():
    """the check tests/test_abi_cpu.py::test_hand_scheduled_kernels_do_not_spill makes for its files"""
    names, scratch, spills, _ = resource_usage("conv_train.hip")
    assert len(names) >= 17                                                   # 6 tile kernels, 3 packs, 3 + 3 GroupNorm passes, 2 merges
    assert all(v == 0 for v in scratch + spills), list(zip(names, scratch, spills))
