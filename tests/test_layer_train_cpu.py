"""CPU-side checks of the encoder-layer glue (csrc/layer_train.hip, brepgen_amd/layer.py): the ABI boundary, argument validation, the
module swap, the compiler's resource report, and the restatement the GPU tests compare against (tests/layer_restate.py) -- the mask's
statistics and key separation, and the LayerNorm backward in the kernels' summation order against torch's fp64 autograd, held to HALF
the bound the GPU test asserts.  No kernel is launched.

The ABI number stays 7 (the entries are added ones; the suite's existing files pin it): what is asserted is that header, binding and
library agree."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import brepgen_amd as bga
from brepgen_amd import _lib
from brepgen_amd import layer as L
from tests import layer_ops as ops
from tests import layer_restate as R
from tests.train_cpu import BF, F16, F32, FAKE, ROOT, assert_exported, resource_usage, vp
from tests.train_cpu import explained as _explained

NEW = ("bg_ln_train_fwd", "bg_ln_bwd_workspace_bytes", "bg_ln_bwd", "bg_dropout_add_fwd", "bg_dropout_bwd", "bg_relu_dropout_fwd",
       "bg_relu_dropout_bwd", "bg_dropout_mask")


def test_entries_are_exported_with_the_declared_argtypes():
    assert_exported(NEW)
    i, z, d, f, u64, u32, ll = C.c_int, C.c_size_t, C.c_double, C.c_float, C.c_ulonglong, C.c_uint, C.c_longlong
    key = [d, u64, u32, i, ll]
    assert _lib._SIGNATURES["bg_ln_train_fwd"] == (i, [vp, i, vp, vp, vp, i, vp, i, f, vp])
    assert _lib._SIGNATURES["bg_ln_bwd_workspace_bytes"] == (z, [i])
    assert _lib._SIGNATURES["bg_ln_bwd"] == (i, [vp, i, vp, i, vp, vp, vp, vp, vp, vp, i, vp, z, vp])
    assert _lib._SIGNATURES["bg_dropout_add_fwd"] == (i, [vp, i, vp, vp, i, i, i, i] + key + [vp])
    assert _lib._SIGNATURES["bg_dropout_bwd"] == (i, [vp, i, vp, i, i, i, i] + key + [vp])
    assert _lib._SIGNATURES["bg_relu_dropout_fwd"] == (i, [vp, vp, i, i, i, i] + key + [vp])
    assert _lib._SIGNATURES["bg_relu_dropout_bwd"] == (i, [vp, vp, vp, i, i, i, d, vp])
    assert _lib._SIGNATURES["bg_dropout_mask"] == (i, [vp, i, i, i] + key + [vp])
    assert "0xD409" in open(os.path.join(ROOT, "brepgen_amd", "csrc", "philox.h")).read().split("#pragma once")[0]      # the tag list


def _ln_fwd(x=FAKE, xd=F32, g=FAKE, b=FAKE, y=FAKE, yd=BF, stats=FAKE, M=5, eps=1e-5):
    return _lib.load().bg_ln_train_fwd(x, xd, g, b, y, yd, stats, M, eps, None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(x=None), _lib.BG_E_ARG, b"null"),
    (dict(stats=None), _lib.BG_E_ARG, b"null"),
    (dict(x=FAKE + 8), _lib.BG_E_ALIGN, b"alignment"),
    (dict(stats=FAKE + 4), _lib.BG_E_ALIGN, b"alignment"),
    (dict(xd=F16, yd=BF), _lib.BG_E_DTYPE, b"dtype pair"),
    (dict(xd=7), _lib.BG_E_DTYPE, b"dtype pair"),
    (dict(M=-1), _lib.BG_E_SHAPE, b"negative"),
    (dict(eps=-1.0), _lib.BG_E_ARG, b"eps"),
])
def test_ln_fwd_argument_errors_are_negative_and_explained(kw, code, word):
    _explained(_ln_fwd(**kw), code, word)


def _ln_bwd(dy=FAKE, yd=BF, x=FAKE, xd=F32, stats=FAKE, g=FAKE, dskip=None, dx=FAKE, dg=FAKE, db=FAKE, M=200, ws=FAKE, ws_bytes=1 << 30):
    return _lib.load().bg_ln_bwd(dy, yd, x, xd, stats, g, dskip, dx, dg, db, M, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(dy=None), _lib.BG_E_ARG, b"null"),
    (dict(dx=None), _lib.BG_E_ARG, b"null"),
    (dict(dg=None), _lib.BG_E_ARG, b"together"),
    (dict(db=None), _lib.BG_E_ARG, b"together"),
    (dict(ws=None), _lib.BG_E_ARG, b"workspace"),
    (dict(ws_bytes=ops.workspace_formula(200) - 1), _lib.BG_E_ARG, b"workspace"),
    (dict(dskip=FAKE + 2), _lib.BG_E_ALIGN, b"alignment"),
    (dict(dg=FAKE + 4), _lib.BG_E_ALIGN, b"alignment"),
    (dict(xd=BF, yd=F16), _lib.BG_E_DTYPE, b"dtype pair"),
    (dict(M=-3), _lib.BG_E_SHAPE, b"negative"),
])
def test_ln_bwd_argument_errors_are_negative_and_explained(kw, code, word):
    _explained(_ln_bwd(**kw), code, word)


def test_ln_bwd_workspace_plan():
    for M in (1, 3, 31, 32, 33, 257, 1000, 8192, 8193, 15360, 30720, 96000, 524288, 524289, 2_000_000):
        Rr, G = ops.chain_rows(M), ops.workgroups(M)
        assert 4 <= Rr <= 64 and 1 <= G <= ops.MAX_WGS
        assert ops.workspace_bytes(M) == ops.workspace_formula(M) == G * 1536 * 8
        if G < ops.MAX_WGS:
            assert G * 8 * Rr >= M > (G - 1) * 8 * Rr                  # one chunk per workgroup, none empty
    assert ops.workspace_bytes(0) == 0 and ops.workspace_bytes(-5) == 0
    # the rule's intent at the trainers' shapes: every one of the 256 CUs has a workgroup, and about four at most
    assert all(256 <= ops.workgroups(M) <= 1100 for M in (15360, 30720, 96000))


KEY = dict(M=6, C=768, B=3, p=0.1, seed=77, draw=5, site=1, first=0)


def _call(name, **kw):
    a = dict(KEY, **kw)
    lib = _lib.load()
    key = (a["p"], a["seed"], a["draw"], a["site"], a["first"], None)
    p1, p2, p3 = a.get("p1", FAKE), a.get("p2", FAKE), a.get("p3", FAKE)
    if name == "bg_dropout_add_fwd":
        return lib.bg_dropout_add_fwd(p1, a.get("bd", BF), p2, p3, a.get("sd", F32), a["M"], a["C"], a["B"], *key)
    if name == "bg_dropout_bwd":
        return lib.bg_dropout_bwd(p1, a.get("sd", F32), p2, a.get("bd", BF), a["M"], a["C"], a["B"], *key)
    if name == "bg_relu_dropout_fwd":
        return lib.bg_relu_dropout_fwd(p1, p2, a.get("bd", BF), a["M"], a["C"], a["B"], *key)
    if name == "bg_relu_dropout_bwd":
        return lib.bg_relu_dropout_bwd(p1, p2, p3, a.get("bd", BF), a["M"], a["C"], a["p"], None)
    return lib.bg_dropout_mask(p1, a["M"], a["C"], a["B"], *key)


KEYED = ("bg_dropout_add_fwd", "bg_dropout_bwd", "bg_relu_dropout_fwd", "bg_dropout_mask")


@pytest.mark.parametrize("name", KEYED + ("bg_relu_dropout_bwd",))
@pytest.mark.parametrize("kw, code, word", [
    (dict(p1=None), _lib.BG_E_ARG, b"null"),
    (dict(p1=FAKE + 4), _lib.BG_E_ALIGN, b"alignment"),
    (dict(C=772), _lib.BG_E_SHAPE, b"multiple of 8"),
    (dict(C=0), _lib.BG_E_SHAPE, b"multiple of 8"),
    (dict(M=-6), _lib.BG_E_SHAPE, b"M = -6"),
    (dict(p=1.0), _lib.BG_E_ARG, b"outside [0, 1)"),
    (dict(p=-0.1), _lib.BG_E_ARG, b"outside [0, 1)"),
    (dict(p=float("nan")), _lib.BG_E_ARG, b"outside [0, 1)"),
    (dict(M=1 << 30, C=1024, B=1), _lib.BG_E_SHAPE, b"32 bits"),
])
def test_dropout_argument_errors_are_negative_and_explained(name, kw, code, word):
    _explained(_call(name, **kw), code, word)


@pytest.mark.parametrize("name", KEYED)
@pytest.mark.parametrize("kw, code, word", [
    (dict(site=4), _lib.BG_E_ARG, b"site"),
    (dict(site=-1), _lib.BG_E_ARG, b"site"),
    (dict(B=4), _lib.BG_E_SHAPE, b"multiple of B"),
    (dict(B=0), _lib.BG_E_SHAPE, b"multiple of B"),
    (dict(first=-1), _lib.BG_E_ARG, b"first_sample"),
    (dict(first=(1 << 44) - 2), _lib.BG_E_ARG, b"first_sample"),
])
def test_dropout_key_errors_are_negative_and_explained(name, kw, code, word):
    _explained(_call(name, **kw), code, word)
    assert _call(name, M=0, first=(1 << 44) - 3) == 0                  # the largest first_sample; M == 0: no launch


@pytest.mark.parametrize("name, kw, word", [
    ("bg_dropout_add_fwd", dict(bd=F32), b"branch dtype"),
    ("bg_dropout_add_fwd", dict(bd=BF, sd=F16), b"stream dtype"),
    ("bg_dropout_bwd", dict(bd=F16, sd=BF), b"stream dtype"),
    ("bg_dropout_bwd", dict(bd=F32), b"branch dtype"),
    ("bg_relu_dropout_fwd", dict(bd=F32), b"dtype"),
    ("bg_relu_dropout_bwd", dict(bd=9), b"dtype"),
])
def test_dropout_dtype_pairs(name, kw, word):
    _explained(_call(name, **kw), _lib.BG_E_DTYPE, word)


def test_python_surface_raises_without_a_device_and_on_bad_arguments():
    w, b = torch.ones(768), torch.zeros(768)
    x, x16 = torch.zeros(5, 3, 768), torch.zeros(5, 3, 768, dtype=torch.float16)
    with pytest.raises(_lib.BrepgenHipError):
        L.layer_norm(x, w, b)                                              # CPU tensors: no fallback
    with pytest.raises(_lib.BrepgenHipError):
        L.dropout_add(x16, x, 0.1, True, seed=1)
    with pytest.raises(_lib.BrepgenHipError):
        L.relu_dropout(x16, 0.1, True, seed=1)
    with pytest.raises(ValueError):
        L.layer_norm(torch.zeros(5, 512), w, b)                            # width
    with pytest.raises(ValueError):
        L.layer_norm(x.double(), w, b)                                     # dtype
    with pytest.raises(ValueError):
        L.layer_norm(x, w[:100], b)
    with pytest.raises(ValueError):
        L.layer_norm(x16, w, b, out_dtype=torch.bfloat16)                  # a 16-bit x gives its own dtype or fp32
    with pytest.raises(ValueError):
        L.layer_norm(x, w, b, eps=-1.0)
    with pytest.raises(ValueError):
        L.dropout_add(x, x, 0.1, True)                                     # fp32 branch
    with pytest.raises(ValueError):
        L.dropout_add(x16, x.to(torch.bfloat16), 0.1, True)                # skip neither fp32 nor branch's dtype
    with pytest.raises(ValueError):
        L.dropout_add(x16, x[:4], 0.1, True)                               # shapes
    with pytest.raises(ValueError):
        L.dropout_add(x16, x, 1.0, True)                                   # p
    with pytest.raises(ValueError):
        L.dropout_add(x16, x, 0.1, True, site=4)
    with pytest.raises(ValueError):
        L.dropout_add(x16, x, 0.1, True, first_sample=-1)
    with pytest.raises(ValueError):
        L.relu_dropout(x, 0.1, True)                                       # fp32
    with pytest.raises(ValueError):
        L.relu_dropout(torch.zeros(5, 3, 100, dtype=torch.float16), 0.1, True)      # C % 8
    with pytest.raises(ValueError):
        L.relu_dropout(x16, -0.5, True)
    with pytest.raises(ValueError):
        L.DeviceLayerNorm(512)
    m = L.DeviceLayerNorm(768)
    assert sorted(m.state_dict()) == ["bias", "weight"] and isinstance(m, nn.LayerNorm)
    with pytest.raises(_lib.BrepgenHipError):
        m(x)
    for name in ("layer_norm", "dropout_add", "relu_dropout", "DeviceLayerNorm", "DeviceEncoderLayer", "use_device_layer"):
        assert getattr(bga, name) is getattr(L, name) and name in bga.__all__


def _stock(dropout=0.1, layers=2, norm=True, **kw):
    return nn.TransformerEncoder(nn.TransformerEncoderLayer(768, 12, 1024, dropout=dropout, norm_first=True, **kw), layers,
                                 norm=nn.LayerNorm(768) if norm else None, enable_nested_tensor=False)


@pytest.mark.parametrize("prepared", [False, True], ids=["stock", "attention_and_linear_done"])
@pytest.mark.parametrize("norm", [False, True], ids=["no_final_norm", "final_norm"])
def test_use_device_layer_keeps_parameter_identity_and_state_dict_keys(norm, prepared):
    enc = _stock(norm=norm)
    before = {k: id(p) for k, p in enc.named_parameters()}
    keys = list(enc.state_dict())
    if prepared:
        bga.use_device_linear(bga.use_device_attention(enc))
    assert L.use_device_layer(enc, seed=77) is enc
    assert {k: id(p) for k, p in enc.named_parameters()} == before
    assert list(enc.state_dict()) == keys
    for i, layer in enumerate(enc.layers):
        assert isinstance(layer, L.DeviceEncoderLayer) and (layer.layer_index, layer.n_layers, layer.seed, layer.calls) == (i, 2, 77, 0)
        assert isinstance(layer.self_attn, bga.MultiheadSelfAttention) and layer.self_attn.device_linear and layer.self_attn.seed == 77
        assert isinstance(layer.linear1, bga.DeviceLinear) and isinstance(layer.linear2, bga.DeviceLinear)
        assert layer.self_attn.batch_first is False and layer.training
        assert (layer.dropout1.p, layer.dropout.p, layer.dropout2.p) == (0.1, 0.1, 0.1)
    if norm:
        assert isinstance(enc.norm, L.DeviceLayerNorm) and enc.norm.out_dtype == torch.float32
    else:
        assert enc.norm is None
    L.use_device_layer(enc)                                                   # idempotent; the seed stays
    assert {k: id(p) for k, p in enc.named_parameters()} == before and enc.layers[1].seed == 77
    assert enc.layers[0].next_draw_id() == 0 and enc.layers[0].next_draw_id() == 2 and enc.layers[1].next_draw_id() == 1
    enc.eval()
    assert not enc.layers[0].training and not enc.layers[0].self_attn.training
    # nn.TransformerEncoder.forward accepts the layer class and reaches it (which then refuses the CPU tensor); masks it does not provide raise
    with pytest.raises(_lib.BrepgenHipError):
        enc(torch.zeros(5, 3, 768), src_key_padding_mask=torch.zeros(3, 5, dtype=torch.bool))
    with pytest.raises(NotImplementedError):
        enc.layers[0](torch.zeros(5, 3, 768), src_mask=torch.zeros(5, 5))
    with pytest.raises(NotImplementedError):
        enc.layers[0](torch.zeros(5, 3, 768), is_causal=True)


def test_use_device_layer_refuses_what_it_does_not_run():
    with pytest.raises(ValueError):
        L.use_device_layer(nn.Linear(768, 768))
    with pytest.raises(ValueError):
        L.use_device_layer(nn.TransformerEncoder(nn.TransformerEncoderLayer(768, 12, 1024, norm_first=False), 1, enable_nested_tensor=False))
    with pytest.raises(ValueError):
        L.use_device_layer(_stock(activation="gelu"))
    with pytest.raises(ValueError):
        L.use_device_layer(nn.TransformerEncoder(nn.TransformerEncoderLayer(512, 8, 1024, norm_first=True), 1, enable_nested_tensor=False))
    enc = _stock()
    enc.norm = nn.LayerNorm(768, elementwise_affine=False)
    with pytest.raises(ValueError):
        L.use_device_layer(enc)
    assert isinstance(enc.layers[0], nn.TransformerEncoderLayer)              # nothing was converted before the refusal


def test_dropout_draw_state_of_the_attention_module_and_the_layer():
    """_train.DropoutDraws, the one draw state of MultiheadSelfAttention and DeviceEncoderLayer: draw_id = (calls * n_layers +
    layer_index) mod 2^32, a forward that drops nothing leaves it alone, seed / calls replay it, every instance counts for itself."""
    from brepgen_amd import _train
    enc = L.use_device_layer(_stock(layers=3), seed=5)
    layer, attn = enc.layers[1], enc.layers[1].self_attn
    assert isinstance(layer, _train.DropoutDraws) and isinstance(attn, _train.DropoutDraws)
    for m in (layer, attn):
        assert (m.seed, m.calls, m.layer_index, m.n_layers, m.first_sample) == (5, 0, 1, 3, 0)
    fresh = bga.MultiheadSelfAttention()
    assert (fresh.seed, fresh.calls, fresh.layer_index, fresh.n_layers, fresh.first_sample) == (None, 0, 0, 1, 0)
    assert layer.draw_key(False) == (5, 0) and fresh.draw_key(False) == (0, 0) and (layer.calls, fresh.calls, fresh.seed) == (0, 0, None)
    assert [layer.draw_key(True) for _ in range(3)] == [(5, 1), (5, 4), (5, 7)] and layer.calls == 3
    assert attn.calls == 0 and enc.layers[0].calls == 0 and attn.draw_key(True) == (5, 1) and layer.calls == 3      # counters of their own
    layer.seed, layer.calls = 9, 1                                             # replay from the second forward, under another seed
    assert [layer.draw_key(True) for _ in range(2)] == [(9, 4), (9, 7)]
    # the wrap: calls just below 2^32 / n_layers
    layer.calls = 2 ** 32 // 3 - 1                                             # 3 * (calls + 1) + 1 == 2^32
    assert [layer.next_draw_id() for _ in range(3)] == [2 ** 32 - 3, 0, 3] and layer.calls == 2 ** 32 // 3 + 2
    # the default seed is fixed at the first forward that drops, from the CPU generator's state
    torch.manual_seed(1234)
    from brepgen_amd.sampling import noise_key
    assert fresh.draw_key(True) == (noise_key(), 0) and fresh.seed == noise_key() and fresh.draw_key(True) == (fresh.seed, 1)
    # the three converters refuse an object without .layers alike
    for convert in (bga.use_device_attention, bga.use_device_linear, L.use_device_layer):
        with pytest.raises(ValueError, match=r"an object with \.layers"):
            convert(nn.Linear(768, 768))


def test_layer_train_kernels_use_no_scratch_and_do_not_spill():
    """the check tests/test_abi_cpu.py::test_hand_scheduled_kernels_do_not_spill makes for its files"""
    names, scratch, spills, sspills = resource_usage("layer_train.hip")
    assert len(names) == 45, names       # 7 LayerNorm forwards, 14 backwards, the reduction, 8 + 8 dropout add / backward, 4 + 2 ReLU-dropout, the mask
    assert all(v == 0 for v in scratch + spills + sspills), list(zip(names, scratch, spills, sspills))


SHAPES = [(5, 3, 768, 0.1), (33, 3, 1024, 0.1), (1, 1, 768, 0.5), (7, 3, 768, 0.1), (64, 4, 1024, 0.25)]      # (N, B, C, p)
FIRST = 2 ** 33 + 3


@pytest.mark.parametrize("N, B, C, p", SHAPES)
def test_restated_mask_drops_the_stated_fraction(N, B, C, p):
    m = R.keep_mask(N * B, C, B, p, 77, 5, 1, FIRST)
    q = R.threshold(p) / 65536.0
    sigma = math.sqrt(q * (1.0 - q) / m.size)
    assert abs((1.0 - m.mean()) - q) <= 5.0 * sigma, ((1.0 - m.mean()), q, sigma)
    assert R.threshold(0.1) == 6553 and R.threshold(0.5) == 32768 and R.threshold(0.0) == 0


def test_restated_masks_of_other_keys_differ_and_shards_reproduce_their_rows():
    N, B, C, p = 7, 3, 768, 0.1
    base = R.keep_mask(N * B, C, B, p, 77, 5, 1, FIRST)
    for kw in (dict(site=2), dict(site=0), dict(draw_id=6), dict(seed=78), dict(seed=77 + (1 << 32)), dict(first_sample=FIRST + 1),
               dict(first_sample=FIRST + (1 << 32))):
        a = dict(seed=77, draw_id=5, site=1, first_sample=FIRST)
        a.update(kw)
        assert not np.array_equal(R.keep_mask(N * B, C, B, p, **a), base), kw
    full = base.reshape(N, B, C)
    assert not np.array_equal(full[:, 0], full[:, 1]) and not np.array_equal(full[0], full[1])       # samples and tokens differ
    for lo, hi in ((0, 1), (1, 3), (2, 3)):                                   # a rank that owns samples [lo, hi)
        part = R.keep_mask(N * (hi - lo), C, hi - lo, p, 77, 5, 1, FIRST + lo).reshape(N, hi - lo, C)
        assert np.array_equal(part, full[:, lo:hi])
    assert R.keep_mask(N * B, C, B, 0.0, 77, 5, 1, FIRST).all()               # threshold 0: everything kept


@pytest.mark.parametrize("dskip", (False, True), ids=("no_dskip", "dskip"))
@pytest.mark.parametrize("M", (1, 3, 4, 5, 63, 64, 65, 129, 257, 1000))
def test_restated_ln_backward_meets_half_the_derived_bound(M, dskip):
    """the kernels' summation order in numpy float32 against torch's fp64 autograd: dgamma / dbeta within HALF the bound the GPU test
    asserts (the bound is one the summation order alone satisfies, with headroom for the device's sqrt and division), dx and y close"""
    eps = float(np.float32(1e-5))
    g = torch.Generator(device="cpu").manual_seed(M)
    x = (0.5 + 1.5 * torch.randn(M, 768, generator=g)).to(torch.float16 if M % 2 else torch.float32).float()
    dy = torch.randn(M, 768, generator=g).to(torch.bfloat16).float()
    sk = torch.randn(M, 768, generator=g) if dskip else None
    gamma, beta = 1.0 + 0.1 * torch.randn(768, generator=g), 0.1 * torch.randn(768, generator=g)
    y, stats = R.ln_fwd(x.numpy(), gamma.numpy(), beta.numpy(), eps)
    dx, dg, db = R.ln_bwd(dy.numpy(), x.numpy(), stats, gamma.numpy(), None if sk is None else sk.numpy())
    xd, gd, bd = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    yd = F.layer_norm(xd, (768,), gd, bd, eps)
    yd.backward(dy.double())
    want_dx = xd.grad if sk is None else xd.grad + sk.double()
    bg, bb = R.dgamma_dbeta_bounds(dy, x, M, eps)
    assert bool(((torch.from_numpy(dg).double() - gd.grad).abs() <= 0.5 * bg).all())
    assert bool(((torch.from_numpy(db).double() - bd.grad).abs() <= 0.5 * bb).all())
    assert float((torch.from_numpy(y).double() - yd.detach()).abs().max()) <= 4e-6
    assert float((torch.from_numpy(dx).double() - want_dx).abs().max()) <= 4e-6
    assert float((torch.from_numpy(stats[:, 0]).double() - x.double().mean(1)).abs().max()) <= 1e-6
