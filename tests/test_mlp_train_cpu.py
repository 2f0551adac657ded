"""CPU-side checks of the denoiser-MLP training ops (csrc/mlp_train.hip, brepgen_amd/mlp.py, training.mse_loss): the ABI boundary,
argument validation, the module swap on the reference-keyed denoisers, the compiler's resource report, and the restatement the GPU
tests compare against (tests/mlp_restate.py) held against torch's fp64 autograd of the same Sequential and of
mse_loss(pred[~mask], target[~mask]).  No kernel is launched."""
import ctypes as C
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import brepgen_amd as bga
from brepgen_amd import _lib, layer, linear, mlp, training
from oracle.ref_formulation import RefDenoiser
from tests import mlp_ops as ops
from tests import mlp_restate as R
from tests.train_cpu import BF, F16, F32, FAKE, assert_exported, resource_usage, vp
from tests.train_cpu import explained as _explained

NEW = ("bg_thin_expand", "bg_thin_contract", "bg_thin_wgrad_workspace_bytes", "bg_thin_wgrad", "bg_ln_silu_train_fwd",
       "bg_ln_silu_bwd_workspace_bytes", "bg_ln_silu_bwd", "bg_masked_mse_bwd")


def test_entries_are_exported_with_the_declared_argtypes():
    assert_exported(NEW)
    i, z, f, ll = C.c_int, C.c_size_t, C.c_float, C.c_longlong
    assert _lib._SIGNATURES["bg_thin_expand"] == (i, [vp, i, i, vp, i, vp, vp, i, i, i, vp])
    assert _lib._SIGNATURES["bg_thin_contract"] == (i, [vp, i, vp, vp, vp, i, i, vp])
    assert _lib._SIGNATURES["bg_thin_wgrad_workspace_bytes"] == (z, [i, i])
    assert _lib._SIGNATURES["bg_thin_wgrad"] == (i, [vp, i, i, vp, i, vp, i, vp, i, i, i, vp, z, vp])
    assert _lib._SIGNATURES["bg_ln_silu_train_fwd"] == _lib._SIGNATURES["bg_ln_train_fwd"]
    assert _lib._SIGNATURES["bg_ln_silu_bwd_workspace_bytes"] == (z, [i])
    assert _lib._SIGNATURES["bg_ln_silu_bwd"] == (i, [vp, i, vp, i, vp, vp, vp, vp, vp, vp, i, vp, z, vp])
    assert _lib._SIGNATURES["bg_masked_mse_bwd"] == (i, [vp, vp, vp, ll, i, i, i, vp, vp, vp, vp])


def _expand(x=FAKE, xd=F32, ldx=18, w=FAKE, km=0, b=FAKE, y=FAKE, yd=BF, M=5, s=12):
    return _lib.load().bg_thin_expand(x, xd, ldx, w, km, b, y, yd, M, s, None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(x=None), _lib.BG_E_ARG, b"null"),
    (dict(w=None), _lib.BG_E_ARG, b"null"),
    (dict(y=None), _lib.BG_E_ARG, b"null"),
    (dict(s=0), _lib.BG_E_SHAPE, b"outside 1 .. 48"),
    (dict(s=49, ldx=64), _lib.BG_E_SHAPE, b"outside 1 .. 48"),
    (dict(ldx=11), _lib.BG_E_SHAPE, b"ldx = 11 is below s = 12"),
    (dict(M=-1), _lib.BG_E_SHAPE, b"negative"),
    (dict(xd=5), _lib.BG_E_DTYPE, b"dtype"),
    (dict(y=FAKE + 8), _lib.BG_E_ALIGN, b"alignment"),
    (dict(x=FAKE + 2), _lib.BG_E_ALIGN, b"alignment"),
])
def test_thin_expand_argument_errors_are_negative_and_explained(kw, code, word):
    _explained(_expand(**kw), code, word)
    assert _expand(M=0, x=None, w=None, y=None) == 0                       # no rows: no launch, nothing is looked at
    assert _expand(b=None, M=0) == 0 and _expand(x=FAKE + 2, xd=BF, M=0) == 0


def _contract(a=FAKE, ad=BF, w=FAKE, b=FAKE, y=FAKE, M=5, n=18):
    return _lib.load().bg_thin_contract(a, ad, w, b, y, M, n, None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(a=None), _lib.BG_E_ARG, b"null"),
    (dict(y=None), _lib.BG_E_ARG, b"null"),
    (dict(n=0), _lib.BG_E_SHAPE, b"outside 1 .. 48"),
    (dict(n=49), _lib.BG_E_SHAPE, b"outside 1 .. 48"),
    (dict(M=-2), _lib.BG_E_SHAPE, b"negative"),
    (dict(ad=F32), _lib.BG_E_DTYPE, b"dtype"),
    (dict(a=FAKE + 8), _lib.BG_E_ALIGN, b"alignment"),
])
def test_thin_contract_argument_errors_are_negative_and_explained(kw, code, word):
    _explained(_contract(**kw), code, word)
    assert _contract(M=0) == 0


def _wgrad(t=FAKE, td=F32, ldt=18, u=FAKE, ud=BF, g=FAKE, tr=0, cs=None, of=0, M=300, s=12, ws=FAKE, ws_bytes=1 << 30):
    return _lib.load().bg_thin_wgrad(t, td, ldt, u, ud, g, tr, cs, of, M, s, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(t=None), _lib.BG_E_ARG, b"null"),
    (dict(u=None), _lib.BG_E_ARG, b"null"),
    (dict(g=None), _lib.BG_E_ARG, b"null"),
    (dict(s=0), _lib.BG_E_SHAPE, b"outside 1 .. 48"),
    (dict(s=49, ldt=49), _lib.BG_E_SHAPE, b"outside 1 .. 48"),
    (dict(ldt=11), _lib.BG_E_SHAPE, b"ldt = 11 is below s = 12"),
    (dict(ws=None), _lib.BG_E_ARG, b"workspace"),
    (dict(ws_bytes=ops.wgrad_workspace_formula(300, 12) - 1), _lib.BG_E_ARG, b"workspace"),
    (dict(of=1), _lib.BG_E_ARG, b"colsum"),
    (dict(cs=FAKE), _lib.BG_E_ARG, b"colsum"),
    (dict(of=3, cs=FAKE), _lib.BG_E_ARG, b"colsum"),
    (dict(ud=F32), _lib.BG_E_DTYPE, b"u dtype"),
    (dict(td=9), _lib.BG_E_DTYPE, b"t dtype"),
    (dict(u=FAKE + 4), _lib.BG_E_ALIGN, b"alignment"),
    (dict(M=-1), _lib.BG_E_SHAPE, b"negative"),
])
def test_thin_wgrad_argument_errors_are_negative_and_explained(kw, code, word):
    _explained(_wgrad(**kw), code, word)


def test_thin_wgrad_workspace_plan():
    for s in (1, 6, 8, 9, 12, 18, 48):
        for M in (1, 31, 32, 33, 257, 1000, 8192, 15360, 32777, 96000, 2_000_000):
            s8, Rr, chunks, W = ops.wgrad_plan(M, s)
            assert s8 % 8 == 0 and s <= s8 < s + 8 and 4 <= Rr <= 64 and 1 <= W <= 256 // (s8 // 8)
            assert ops.wgrad_workspace_bytes(M, s) == ops.wgrad_workspace_formula(M, s) == W * (s8 * 768 + 768 + s8) * 8
            assert ops.wgrad_workspace_bytes(M, s) <= 14 << 20
    for M, s in ((0, 6), (-3, 6), (5, 0), (5, 49)):
        assert ops.wgrad_workspace_bytes(M, s) == 0
    # the rule's intent at the trainers' shapes: about three workgroups per CU (3 slabs x k groups x W)
    assert all(512 <= 3 * ((s + 7) // 8) * ops.wgrad_plan(M, s)[3] <= 768 for M in (15360, 96000) for s in (6, 12, 18, 48))


def _ln_silu_bwd(dh=FAKE, hd=BF, x=FAKE, xd=BF, stats=FAKE, g=FAKE, b=FAKE, dx=FAKE, dg=FAKE, db=FAKE, M=200, ws=FAKE, ws_bytes=1 << 30):
    return _lib.load().bg_ln_silu_bwd(dh, hd, x, xd, stats, g, b, dx, dg, db, M, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(dh=None), _lib.BG_E_ARG, b"null"),
    (dict(b=None), _lib.BG_E_ARG, b"null"),
    (dict(dg=None), _lib.BG_E_ARG, b"together"),
    (dict(ws=None), _lib.BG_E_ARG, b"workspace"),
    (dict(ws_bytes=_lib.load().bg_ln_bwd_workspace_bytes(200) - 1), _lib.BG_E_ARG, b"workspace"),
    (dict(xd=BF, hd=F16), _lib.BG_E_DTYPE, b"dtype pair"),
    (dict(b=FAKE + 4), _lib.BG_E_ALIGN, b"alignment"),
    (dict(M=-3), _lib.BG_E_SHAPE, b"negative"),
])
def test_ln_silu_argument_errors_are_negative_and_explained(kw, code, word):
    _explained(_ln_silu_bwd(**kw), code, word)
    assert b"bg_ln_silu_bwd" in _lib.load().bg_last_error()
    lib = _lib.load()
    _explained(lib.bg_ln_silu_train_fwd(None, F32, FAKE, FAKE, FAKE, BF, FAKE, 5, 1e-5, None), _lib.BG_E_ARG, b"bg_ln_silu_train_fwd: null")
    _explained(lib.bg_ln_silu_train_fwd(FAKE, F16, FAKE, FAKE, FAKE, BF, FAKE, 5, 1e-5, None), _lib.BG_E_DTYPE, b"dtype pair")
    assert all(lib.bg_ln_silu_bwd_workspace_bytes(M) == lib.bg_ln_bwd_workspace_bytes(M) for M in (-1, 0, 1, 257, 32777, 96000))


def _mse_bwd(p=FAKE, t=FAKE, m=None, rows=5, ld=18, c0=0, nc=12, out3=FAKE, g=FAKE, d=FAKE):
    return _lib.load().bg_masked_mse_bwd(p, t, m, rows, ld, c0, nc, out3, g, d, None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(p=None), _lib.BG_E_ARG, b"null"),
    (dict(out3=None), _lib.BG_E_ARG, b"null"),
    (dict(g=None), _lib.BG_E_ARG, b"null"),
    (dict(d=None), _lib.BG_E_ARG, b"null"),
    (dict(c0=12, nc=7), _lib.BG_E_SHAPE, b"bad shape"),
    (dict(nc=0), _lib.BG_E_SHAPE, b"bad shape"),
    (dict(rows=-1), _lib.BG_E_SHAPE, b"bad shape"),
])
def test_masked_mse_bwd_argument_errors_are_negative_and_explained(kw, code, word):
    _explained(_mse_bwd(**kw), code, word)
    assert _mse_bwd(rows=0) == 0


def test_python_surface_raises_without_a_device_and_on_bad_arguments():
    w0, b0, w3, b3 = torch.zeros(768, 12), torch.zeros(768), torch.zeros(18, 768), torch.zeros(18)
    g, be = torch.ones(768), torch.zeros(768)
    x, a = torch.zeros(2, 3, 12), torch.zeros(2, 3, 768, dtype=torch.bfloat16)
    with pytest.raises(_lib.BrepgenHipError):
        mlp.thin_linear_in(x, w0, b0)                                       # CPU tensors: no fallback
    with pytest.raises(_lib.BrepgenHipError):
        mlp.thin_linear_out(a, w3, b3)
    with pytest.raises(_lib.BrepgenHipError):
        mlp.ln_silu(a, g, be)
    with pytest.raises(_lib.BrepgenHipError):
        training.mse_loss(torch.zeros(2, 3, 18), torch.zeros(2, 3, 18))
    with pytest.raises(ValueError, match="requires a gradient"):
        mlp.thin_linear_in(x.clone().requires_grad_(True), w0, b0)
    with pytest.raises(ValueError, match="16-bit dY"):
        mlp.thin_linear_in(x, w0.clone().requires_grad_(True), b0)          # fp32 output outside autocast, and a gradient asked for
    with pytest.raises(ValueError):
        mlp.thin_linear_in(x, torch.zeros(768, 49), b0)
    with pytest.raises(ValueError):
        mlp.thin_linear_in(x, w0.to(torch.bfloat16), b0)                    # fp32 masters only
    with pytest.raises(ValueError):
        mlp.thin_linear_in(torch.zeros(2, 3, 6), w0, b0)
    with pytest.raises(ValueError):
        mlp.thin_linear_out(a.float(), w3, b3)                              # 16-bit a
    with pytest.raises(ValueError):
        mlp.thin_linear_out(a, torch.zeros(49, 768), None)
    with pytest.raises(ValueError):
        mlp.thin_linear_out(a, w3, torch.zeros(17))
    with pytest.raises(ValueError):
        mlp.ln_silu(torch.zeros(5, 512), g, be)
    with pytest.raises(ValueError):
        mlp.ln_silu(a.to(torch.float16), g, be, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        mlp.ln_silu(a, g, be, eps=-1.0)
    dev = torch.device("meta")
    with pytest.raises(ValueError, match="target requires"):
        training.mse_loss(torch.zeros(2, 18, device=dev), torch.zeros(2, 18, device=dev, requires_grad=True))
    for name in ("thin_linear_in", "thin_linear_out", "ln_silu", "DeviceMLP", "use_device_mlps"):
        assert getattr(bga, name) is getattr(mlp, name) and name in bga.__all__
    for name in ("mse_loss", "use_device_training"):
        assert getattr(bga, name) is getattr(training, name) and name in bga.__all__


def test_existing_error_messages_of_linear_and_layer_norm_are_untouched():
    x16 = torch.zeros(5, 6, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=re.escape("linear: N = 768 and K = 6 must be multiples of 128")):
        linear.linear(x16, torch.zeros(768, 6))
    with pytest.raises(ValueError, match=re.escape("linear: N = 18 and K = 768 must be multiples of 128")):
        linear.linear(torch.zeros(5, 768, dtype=torch.bfloat16), torch.zeros(18, 768))
    with pytest.raises(ValueError, match=re.escape("linear: x of dtype torch.float32 (fp16 or bf16: the trainers run under autocast; an fp32 product "
                                                   "is not provided)")):
        linear.linear(torch.zeros(5, 768), torch.zeros(768, 768))
    with pytest.raises(ValueError, match=re.escape("layer_norm: x must be [..., 768], got (5, 512)")):
        layer.layer_norm(torch.zeros(5, 512), torch.ones(768), torch.zeros(768))
    with pytest.raises(ValueError, match=re.escape("layer_norm: dtype torch.float64 (fp32, fp16 or bf16)")):
        layer.layer_norm(torch.zeros(5, 768, dtype=torch.float64), torch.ones(768), torch.zeros(768))
    with pytest.raises(_lib.BrepgenHipError, match=re.escape("layer_norm runs on the MI355X only (a device tensor is required); there is no CPU fallback")):
        layer.layer_norm(torch.zeros(5, 768), torch.ones(768), torch.zeros(768))
    lib = _lib.load()
    assert lib.bg_ln_bwd(None, BF, FAKE, F32, FAKE, FAKE, None, FAKE, FAKE, FAKE, 200, FAKE, 1 << 30, None) == _lib.BG_E_ARG
    assert lib.bg_last_error() == b"bg_ln_bwd: null pointer (dy, x, stats, gamma, dx)"
    assert lib.bg_ln_train_fwd(FAKE, F16, FAKE, FAKE, FAKE, BF, FAKE, 5, 1e-5, None) == _lib.BG_E_DTYPE
    assert lib.bg_last_error() == b"bg_ln_train_fwd: dtype pair x 1 -> y 2 (x fp32: any y; x 16-bit: y of the same dtype or fp32)"
    assert lib.bg_ln_bwd(FAKE, BF, FAKE, F32, FAKE, FAKE, None, FAKE, FAKE + 4, FAKE, 200, FAKE, 1 << 30, None) == _lib.BG_E_ALIGN
    assert lib.bg_last_error() == (b"bg_ln_bwd: 16-byte alignment of dy / x / gamma / dskip / dx / dgamma / dbeta / workspace, 8-byte alignment "
                                   b"of stats")


KINDS = {"SurfPosNet": 3, "SurfZNet": 4, "EdgePosNet": 5, "EdgeZNet": 7}


@pytest.mark.parametrize("use_cf", [False, True])
@pytest.mark.parametrize("kind", list(KINDS))
def test_use_device_mlps_keeps_parameter_identity_and_state_dict_keys(kind, use_cf):
    with torch.device("meta"):
        m = RefDenoiser(kind, use_cf)
    before = {k: id(p) for k, p in m.named_parameters()}
    keys = list(m.state_dict().keys())
    assert mlp.use_device_mlps(m) is m
    converted = [n for n, c in m.named_children() if isinstance(c, mlp.DeviceMLP)]
    assert len(converted) == KINDS[kind] and "time_embed" in converted and "fc_out" in converted
    assert {k: id(p) for k, p in m.named_parameters()} == before and list(m.state_dict().keys()) == keys
    assert isinstance(m.net.layers[0], nn.TransformerEncoderLayer)             # the encoder is use_device_layer's, untouched here
    for n in converted:
        c = getattr(m, n)
        assert isinstance(c, nn.Sequential) and [type(v) for v in c] == [nn.Linear, nn.LayerNorm, nn.SiLU, nn.Linear] and c.training
    mlp.use_device_mlps(m)                                                     # idempotent
    assert {k: id(p) for k, p in m.named_parameters()} == before
    m.eval()
    assert not m.fc_out.training
    assert training.use_device_training(m, seed=9) is m
    assert isinstance(m.net.layers[0], layer.DeviceEncoderLayer) and m.net.layers[3].seed == 9
    assert {k: id(p) for k, p in m.named_parameters()} == before and list(m.state_dict().keys()) == keys


def test_use_device_mlps_refuses_what_does_not_fit_and_leaves_the_rest_alone():
    class Net(nn.Module):
        def __init__(self, bad):
            super().__init__()
            self.good = nn.Sequential(nn.Linear(6, 768), nn.LayerNorm(768), nn.SiLU(), nn.Linear(768, 768))
            self.other = nn.Sequential(nn.Linear(6, 768), nn.ReLU())           # not an embed MLP: left alone
            self.bad = bad
    for bad in (nn.Sequential(nn.Linear(6, 512), nn.LayerNorm(512), nn.SiLU(), nn.Linear(512, 768)),
                nn.Sequential(nn.Linear(64, 768), nn.LayerNorm(768), nn.SiLU(), nn.Linear(768, 768)),
                nn.Sequential(nn.Linear(6, 768), nn.LayerNorm(768), nn.SiLU(), nn.Linear(768, 100)),
                nn.Sequential(nn.Linear(6, 768), nn.LayerNorm(768, elementwise_affine=False), nn.SiLU(), nn.Linear(768, 768))):
        net = Net(bad)
        with pytest.raises(ValueError, match="bad looks like an embed MLP but does not fit"):
            mlp.use_device_mlps(net)
        assert not isinstance(net.good, mlp.DeviceMLP)                         # nothing was converted before the refusal
    net = Net(nn.Identity())
    mlp.use_device_mlps(net)
    assert isinstance(net.good, mlp.DeviceMLP) and not isinstance(net.other, mlp.DeviceMLP)
    with pytest.raises(ValueError):
        mlp.DeviceMLP(net.other)
    with pytest.raises(ValueError):
        training.use_device_training(nn.Linear(3, 3))
    with pytest.raises(_lib.BrepgenHipError):
        net.good(torch.zeros(4, 6))


def test_mlp_train_kernels_use_no_scratch_and_do_not_spill():
    names, scratch, spills, sspills = resource_usage("mlp_train.hip")
    # 3 expansions, 2 contractions, 2 weight gradients and their reduction, 7 + 14 LN + SiLU row kernels, the loss gradient
    assert len(names) == 30, names
    assert all(v == 0 for v in scratch + spills + sspills), list(zip(names, scratch, spills, sspills))
    assert not any("lt_ln_reduce" in n for n in names)                         # the fp64 merge of the LayerNorm sums stays layer_train.hip's


# ---- the restatement ----

def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(np.float32)
    b = (rng.standard_normal(4000) * 2.0 ** rng.integers(-30, 30, 4000)).astype(np.float32)
    c = (-a * b * (1 + rng.integers(-3, 4, 4000) * 2.0 ** -24)).astype(np.float32)           # cancellation: the product's low bits decide
    c[::3] = (rng.standard_normal(4000) * 2.0 ** rng.integers(-40, 40, 4000)).astype(np.float32)[::3]
    # double-rounding traps: a * b + c one float64 ulp off a float32 tie
    a[:4], b[:4] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23)
    c[:4] = np.float32([2.0 ** 30, -2.0 ** 30, 2.0 ** 29 * 3, 2.0 ** -60])
    got = R.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                                         # Fraction -> float is correctly rounded; float32 of it may double-round
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        errs = [abs(Fraction(float(v)) - exact) for v in cands]
        best = min(errs)
        winners = [v for v, e in zip(cands, errs) if e == best]
        if len(winners) > 1:                                                  # a true tie: the even mantissa
            winners = [v for v in winners if (np.float32(v).view(np.uint32) & 1) == 0]
        assert got[i].view(np.uint32) == np.float32(winners[0]).view(np.uint32), (i, a[i], b[i], c[i], got[i], winners)


def _params(k, n, gen):
    W0, b0 = torch.randn(768, k, generator=gen) / k ** 0.5, 0.1 * torch.randn(768, generator=gen)
    gamma, beta = 1.0 + 0.1 * torch.randn(768, generator=gen), 0.1 * torch.randn(768, generator=gen)
    W3, b3 = torch.randn(n, 768, generator=gen) / 768 ** 0.5, 0.1 * torch.randn(n, generator=gen)
    return W0, b0, gamma, beta, W3, b3


@pytest.mark.parametrize("k, n, M", [(6, 768, 37), (48, 768, 5), (768, 768, 3), (768, 6, 37), (768, 18, 70), (12, 48, 33)])
def test_restated_mlp_against_fp64_autograd_of_the_same_sequential(k, n, M):
    """fp32 restatement, no 16-bit rounding between the pieces, against torch's fp64 autograd: every output and gradient within
    2e-5 of its own scale (fp32 sums of up to 768 terms carry a few 1e-6 relative)"""
    gen = torch.Generator().manual_seed(100 * k + n)
    p = _params(k, n, gen)
    x, dy = torch.randn(M, k, generator=gen), torch.randn(M, n, generator=gen)
    y, grads = R.mlp(x.numpy(), [v.numpy() for v in p], dy.numpy(), 1e-5)
    seq = nn.Sequential(nn.Linear(k, 768), nn.LayerNorm(768), nn.SiLU(), nn.Linear(768, n)).double()
    with torch.no_grad():
        for name, v in zip(("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias"), p):
            seq.get_parameter(name).copy_(v.double())
    out = seq(x.double())
    out.backward(dy.double())

    def close(got, ref, what):
        err, scale = float((torch.from_numpy(np.ascontiguousarray(got)).double() - ref).abs().max()), float(ref.abs().max())
        assert err <= 2e-5 * scale, (what, err, scale)
    close(y, out.detach(), "y")
    for name, q in seq.named_parameters():
        assert grads[name].shape == tuple(q.shape), name
        close(grads[name], q.grad, name)


@pytest.mark.parametrize("valid", ["all", "some", "one", "none"])
@pytest.mark.parametrize("cols", [(0, 12), (12, 18), (0, 18)])
def test_restated_mse_backward_against_autograd_of_the_indexed_loss(valid, cols):
    gen = torch.Generator().manual_seed(7)
    rows, ld, g = 23, 18, 65536.0
    pred, target = torch.randn(rows, ld, generator=gen), torch.randn(rows, ld, generator=gen)
    mask = {"all": torch.zeros(rows, dtype=torch.bool), "some": torch.rand(rows, generator=gen) < 0.4,
            "one": torch.arange(rows) != 11, "none": torch.ones(rows, dtype=torch.bool)}[valid]
    pd = pred.double().requires_grad_(True)
    loss = F.mse_loss(pd[~mask][:, cols[0]:cols[1]], target.double()[~mask][:, cols[0]:cols[1]])
    if valid == "none":
        want = torch.zeros(rows, ld, dtype=torch.float64)                      # torch's mean of nothing is NaN; the kernels say 0 (brepgen_hip.h)
    else:
        (loss * g).backward()
        want = pd.grad
    poisoned = pred.clone()
    poisoned[mask] = float("nan")                                              # masked rows and unused columns are never read
    poisoned[:, :cols[0]] = float("inf")
    poisoned[:, cols[1]:] = float("nan")
    got = R.masked_mse_bwd(poisoned.numpy(), target.numpy(), mask.to(torch.uint8).numpy(), cols, float((~mask).sum()), g)
    got = torch.from_numpy(got).double()
    assert bool(torch.isfinite(got).all())
    assert float((got - want).abs().max()) <= 4 * 2.0 ** -24 * max(float(want.abs().max()), 1e-30)
    assert bool((got[mask] == 0).all()) and bool((got[:, :cols[0]] == 0).all()) and bool((got[:, cols[1]:] == 0).all())
