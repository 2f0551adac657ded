"""CPU-side checks of the Linear-backward entries (csrc/linear_bwd.hip, brepgen_amd/linear.py): the ABI boundary, argument
validation, the host-side split plan and the module swap.  No kernel is launched.

The ABI number: the entries are ADDED ones, and the suite's existing files pin `BG_ABI_VERSION == 7` for added entries
(tests/test_optim_cpu.py, test_dedup_cpu.py, test_dataset_cpu.py, test_metrics_cpu.py, test_vae_full_cpu.py, test_attn_bwd_cpu.py), so
the number stays; what is asserted here is that header, binding and library agree."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import brepgen_amd as bga
from brepgen_amd import _lib
from brepgen_amd import linear as L
from tests import linear_ops as ops
from tests.train_cpu import BF, F32, FAKE, assert_exported, explained, resource_usage, vp

NEW = ("bg_linear_wgrad", "bg_linear_wgrad_workspace_bytes", "bg_linear_wgrad_split", "bg_weight_cast")


def test_entries_are_exported_with_the_declared_argtypes():
    assert_exported(NEW)
    i, z = C.c_int, C.c_size_t
    assert _lib._SIGNATURES["bg_linear_wgrad"] == (i, [vp, i, vp, i, vp, vp, i, i, i, i, i, i, vp, z, vp])
    assert _lib._SIGNATURES["bg_linear_wgrad_workspace_bytes"] == (z, [i, i, i, i])
    assert _lib._SIGNATURES["bg_linear_wgrad_split"] == (i, [i, i, i])
    assert _lib._SIGNATURES["bg_weight_cast"] == (i, [vp, i, i, i, vp, vp, i, vp])


def _wgrad(dy=FAKE, ld_dy=128, x=FAKE, ld_x=128, dw=FAKE, db=FAKE, M=200, N=128, K=128, dtype=BF, out_dtype=F32, split=1, ws=None, ws_bytes=0):
    return _lib.load().bg_linear_wgrad(dy, ld_dy, x, ld_x, dw, db, M, N, K, dtype, out_dtype, split, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, code, word", [
    (dict(N=192, ld_dy=192), _lib.BG_E_SHAPE, b"multiples of 128"),
    (dict(K=64), _lib.BG_E_SHAPE, b"multiples of 128"),
    (dict(N=0), _lib.BG_E_SHAPE, b"multiples of 128"),
    (dict(M=-1), _lib.BG_E_SHAPE, b"negative"),
    (dict(dy=FAKE + 8), _lib.BG_E_ALIGN, b"alignment"),
    (dict(dw=FAKE + 4), _lib.BG_E_ALIGN, b"alignment"),
    (dict(ld_x=132), _lib.BG_E_ALIGN, b"multiples of 8"),
    (dict(ld_dy=120), _lib.BG_E_ALIGN, b"ld_dy"),
    (dict(out_dtype=_lib.BG_F16), _lib.BG_E_DTYPE, b"out_dtype"),
    (dict(dtype=F32), _lib.BG_E_DTYPE, b"operand dtype"),
    (dict(split=65), _lib.BG_E_ARG, b"split"),
    (dict(split=-1), _lib.BG_E_ARG, b"split"),
    (dict(split=64), _lib.BG_E_ARG, b"empty slice"),                    # 200 rows are 7 row steps
    (dict(split=3, ws=FAKE, ws_bytes=256), _lib.BG_E_ARG, b"workspace"),
    (dict(split=3), _lib.BG_E_ARG, b"workspace"),                       # NULL workspace
    (dict(dw=None), _lib.BG_E_ARG, b"null"),
    (dict(x=None), _lib.BG_E_ARG, b"null"),
])
def test_wgrad_argument_errors_are_negative_and_explained(kw, code, word):
    explained(_wgrad(**kw), code, word)


@pytest.mark.parametrize("args, code, word", [
    ((FAKE, F32, 64, 64, None, None, BF), _lib.BG_E_ARG, b"dst and dst_t"),
    ((None, F32, 64, 64, FAKE, None, BF), _lib.BG_E_ARG, b"null"),
    ((FAKE, F32, 96, 64, FAKE, None, BF), _lib.BG_E_SHAPE, b"multiples of 64"),
    ((FAKE, F32, 64, 100, FAKE, None, BF), _lib.BG_E_SHAPE, b"multiples of 64"),
    ((FAKE + 2, BF, 64, 64, FAKE, None, BF), _lib.BG_E_ALIGN, b"alignment"),
    ((FAKE, F32, 64, 64, FAKE, FAKE + 8, BF), _lib.BG_E_ALIGN, b"alignment"),
    ((FAKE, _lib.BG_F16, 64, 64, FAKE, None, BF), _lib.BG_E_DTYPE, b"source dtype"),
    ((FAKE, F32, 64, 64, FAKE, None, F32), _lib.BG_E_DTYPE, b"target dtype"),
])
def test_weight_cast_argument_errors_are_negative_and_explained(args, code, word):
    explained(_lib.load().bg_weight_cast(*args, None), code, word)


M_GRID = (1, 31, 64, 65, 1000, 15360, 25600, 96000)
SHAPES = tuple(ops.LAYERS.values()) + ((128, 128),)


@pytest.mark.parametrize("N, K", SHAPES)
def test_split_plan_properties(N, K):
    for M in M_GRID:
        S = ops.auto_split(M, N, K)
        assert 1 <= S <= 64, (M, S)
        if M <= ops.ROW_STEP:
            assert S == 1, (M, S)
        sl = ops.slices(M, S)
        assert all(b > a for a, b in sl), (M, S, sl)                      # no empty slice
        assert sl[0][0] == 0 and sl[-1][1] == M and all(sl[i][1] == sl[i + 1][0] for i in range(S - 1))
        assert all(a % ops.ROW_STEP == 0 for a, _ in sl)                  # boundaries on whole row steps
        assert ops.workspace_bytes(M, N, K, 0) == ops.workspace_formula(N, K, S)
        for forced in (1, 2, 3, 7, 64):
            assert ops.workspace_bytes(M, N, K, forced) == ops.workspace_formula(N, K, forced)
    assert ops.workspace_bytes(1000, N, K, 65) == 0 and ops.workspace_bytes(1000, N + 1, K, 2) == 0


def test_split_plan_fills_the_chip_at_the_trainers_shapes():
    """the rule's intent: at least one workgroup per CU and at most ~two, wherever the rows allow it"""
    for N, K in ops.LAYERS.values():
        for M in (15360, 25600, 96000):
            wgs = ops.auto_split(M, N, K) * (N // 128) * (K // 128)
            assert 256 <= wgs <= 512, (M, N, K, wgs)


def test_python_surface_raises_without_a_device_and_on_bad_arguments():
    w = torch.zeros(256, 128)
    x16 = torch.zeros(3, 128, dtype=torch.float16)
    with pytest.raises(_lib.BrepgenHipError):
        L.linear(x16, w)                                                   # CPU tensors: no fallback
    with pytest.raises(ValueError):
        L.linear(torch.zeros(3, 128), w)                                   # fp32 input
    with pytest.raises(ValueError):
        L.linear(torch.zeros(3, 96, dtype=torch.float16), torch.zeros(256, 96))     # K % 128
    with pytest.raises(ValueError):
        L.linear(torch.zeros(3, 128, dtype=torch.float16), torch.zeros(200, 128))   # N % 128
    with pytest.raises(ValueError):
        L.linear(x16, w, torch.zeros(255))                                 # bias shape
    with pytest.raises(ValueError):
        L.linear(x16, w.to(torch.bfloat16))                                # weight neither fp32 nor x's dtype
    with pytest.raises(ValueError):
        L.linear(x16, w, split=65)
    with pytest.raises(ValueError):
        L.DeviceLinear(100, 128)
    m = L.DeviceLinear(128, 256)
    assert sorted(m.state_dict()) == ["bias", "weight"] and isinstance(m, nn.Linear)
    with pytest.raises(ValueError):
        m(torch.zeros(3, 128))                                             # fp32 input outside autocast
    with pytest.raises(_lib.BrepgenHipError):
        m(x16)                                                             # CPU
    with pytest.raises(ValueError):
        L.use_device_linear(nn.Linear(128, 128))
    bad = nn.TransformerEncoder(nn.TransformerEncoderLayer(96, 4, 128, norm_first=True), 1, enable_nested_tensor=False)
    with pytest.raises(ValueError):
        L.use_device_linear(bad)
    assert bga.DeviceLinear is L.DeviceLinear and bga.use_device_linear is L.use_device_linear


@pytest.mark.parametrize("with_attention", [False, True])
def test_use_device_linear_keeps_parameter_identity_and_state_dict_keys(with_attention):
    enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(768, 12, 1024, dropout=0.0, norm_first=True), 2, enable_nested_tensor=False)
    before = {k: id(p) for k, p in enc.named_parameters()}
    keys = list(enc.state_dict())
    if with_attention:
        bga.use_device_attention(enc)
    assert L.use_device_linear(enc) is enc
    assert {k: id(p) for k, p in enc.named_parameters()} == before
    assert list(enc.state_dict()) == keys
    for layer in enc.layers:
        assert isinstance(layer.linear1, L.DeviceLinear) and isinstance(layer.linear2, L.DeviceLinear)
        assert isinstance(layer.self_attn.out_proj, L.DeviceLinear)
        assert getattr(layer.self_attn, "device_linear", False) is with_attention
    assert bga.attention.MultiheadSelfAttention.device_linear is False       # off by default
    L.use_device_linear(enc)                                                  # idempotent
    assert {k: id(p) for k, p in enc.named_parameters()} == before


def test_linear_bwd_kernels_do_not_spill():
    """the check tests/test_abi_cpu.py::test_hand_scheduled_kernels_do_not_spill makes for its files"""
    names, scratch, spills, sspills = resource_usage("linear_bwd.hip")
    assert len(names) >= 13                                                   # 6 tile kernels, 4 reductions, 3 casts
    assert all(v == 0 for v in scratch + spills + sspills), list(zip(names, scratch, spills, sspills))
