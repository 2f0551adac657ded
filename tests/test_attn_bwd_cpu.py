"""CPU-side checks of the training attention core (no kernel is launched): the fp64 restatement against torch's own autograd, the
module's parameter surface, the ABI's argument checks, the header against the binding, and the new kernels' resource usage.

Torch references of the restatement: nn.MultiheadAttention with copied weights (dropout = 0, key-padding mask) and
F.scaled_dot_product_attention with an explicit boolean mask tensor (dropout = 0).  F.scaled_dot_product_attention has no way to be
handed a dropout mask, so the dropout case is checked against the same formula written with torch ops (softmax, mask product, matmul:
tests/attn_train_ops.py torch_attention) and differentiated by torch's autograd."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import brepgen_amd as bga
from brepgen_amd import _lib, attention
from tests import attn_bwd_restate as R
from tests import attn_train_ops as ops
from tests.train_cpu import BF, FAKE, ROOT, assert_exported, resource_usage

NEW = ("bg_attn_train_fwd", "bg_attn_bwd_workspace_bytes", "bg_attn_bwd", "bg_attn_dropout_mask")


def _case(N, seed):
    """B = 3 with a padded tail of another length per sample (the all-padded sample is appended by the tests that exclude it)."""
    rng = np.random.default_rng(seed)
    B = 3
    qkv = rng.standard_normal((B, N, 2304))
    qkv[..., :1536] *= np.sqrt(2.0)
    dout = rng.standard_normal((B, N, 768))
    return qkv, dout, ops.key_padding(B, N, "tail", rng)


@pytest.mark.parametrize("N", [1, 5, 33])
def test_restatement_equals_torch_autograd_fp64(N):
    qkv, dout, kp = _case(N, 10 + N)
    out, lse = R.forward(qkv, kp)
    dqkv = R.backward(qkv, dout, kp)
    tq, td, tk = torch.from_numpy(qkv), torch.from_numpy(dout), torch.from_numpy(kp)
    # (1) the formula in torch ops, torch's autograd
    o1, g1 = ops.torch_grads(tq, td, tk, 0.125)
    assert np.abs(out - o1.numpy()).max() <= 1e-12 and np.abs(dqkv - g1.numpy()).max() <= 1e-12
    # (2) F.scaled_dot_product_attention with an explicit mask tensor (True = attend)
    x = tq.clone().requires_grad_(True)
    q, k, v = (x[..., i * 768:(i + 1) * 768].reshape(3, N, 12, 64).transpose(1, 2) for i in range(3))
    o2 = F.scaled_dot_product_attention(q, k, v, attn_mask=~tk[:, None, None, :], scale=0.125).transpose(1, 2).reshape(3, N, 768)
    o2.backward(td)
    assert np.abs(out - o2.detach().numpy()).max() <= 1e-12 and np.abs(dqkv - x.grad.numpy()).max() <= 1e-12
    # lse against torch.logsumexp of the masked scores
    s = 0.125 * (q.detach() @ k.detach().transpose(-1, -2)).masked_fill(tk[:, None, None, :], float("-inf"))
    assert np.abs(lse - torch.logsumexp(s, -1).numpy()).max() <= 1e-12
    # an all-padded sample next to them: zeros, and the other samples unchanged
    qkv4, dout4 = np.concatenate([qkv, qkv[:1]]), np.concatenate([dout, dout[:1]])
    kp4 = np.concatenate([kp, np.ones((1, N), dtype=bool)])
    out4, lse4 = R.forward(qkv4, kp4)
    d4 = R.backward(qkv4, dout4, kp4)
    assert np.array_equal(out4[:3], out) and np.array_equal(d4[:3], dqkv) and not out4[3].any() and not d4[3].any() and not lse4[3].any()


@pytest.mark.parametrize("N", [1, 5, 33])
def test_restatement_equals_multihead_attention_fp64(N):
    """nn.MultiheadAttention (dropout 0) with the weights copied: its in_proj output is the qkv the restatement starts from."""
    qkv_unused, dout, kp = _case(N, 20 + N)
    torch.manual_seed(N)
    mha = nn.MultiheadAttention(768, 12, dropout=0.0).double()
    x = torch.randn(N, 3, 768, dtype=torch.float64, requires_grad=True)
    y, _ = mha(x, x, x, key_padding_mask=torch.from_numpy(kp), need_weights=False)
    # the core's input and upstream gradient as torch sees them
    qkv = F.linear(x, mha.in_proj_weight, mha.in_proj_bias).transpose(0, 1).detach()            # [B, N, 2304]
    out, _ = R.forward(qkv.numpy(), kp)
    y_r = F.linear(torch.from_numpy(out).transpose(0, 1), mha.out_proj.weight, mha.out_proj.bias)
    assert float((y_r - y.detach()).abs().max()) <= 1e-12
    dy = torch.from_numpy(dout).transpose(0, 1)
    y.backward(dy)
    d_core = (dy @ mha.out_proj.weight).transpose(0, 1)                                          # d loss / d out  [B, N, 768]
    dqkv = torch.from_numpy(R.backward(qkv.numpy(), d_core.detach().numpy(), kp)).transpose(0, 1)   # [N, B, 2304]
    gw = torch.einsum("nbo,nbi->oi", dqkv, x.detach())
    assert float((gw - mha.in_proj_weight.grad).abs().max()) <= 1e-12 * max(1.0, float(mha.in_proj_weight.grad.abs().max()))
    assert float((dqkv @ mha.in_proj_weight.detach() - x.grad).abs().max()) <= 1e-12 * max(1.0, float(x.grad.abs().max()))


@pytest.mark.parametrize("N", [1, 5, 33])
def test_restatement_with_dropout_equals_torch_autograd_fp64(N):
    qkv, dout, kp = _case(N, 30 + N)
    p = 0.3
    keep = R.keep_mask(3, N, p, 0x1234567890ABCDEF, 7, first_sample=5)
    assert keep.shape == (3, 12, N, N) and set(np.unique(keep)) <= {0, 1}
    out, _ = R.forward(qkv, kp, keep=keep, p=p)
    dqkv = R.backward(qkv, dout, kp, keep=keep, p=p)
    o1, g1 = ops.torch_grads(torch.from_numpy(qkv), torch.from_numpy(dout), torch.from_numpy(kp), 0.125, torch.from_numpy(keep), R.rp_of(p))
    assert np.abs(out - o1.numpy()).max() <= 1e-12 and np.abs(dqkv - g1.numpy()).max() <= 1e-12


def test_keep_mask_is_per_sample_and_per_draw():
    a = R.keep_mask(5, 9, 0.5, 99, 3)
    assert np.array_equal(a[2:5], R.keep_mask(3, 9, 0.5, 99, 3, first_sample=2))
    assert not np.array_equal(a, R.keep_mask(5, 9, 0.5, 99, 4)) and not np.array_equal(a, R.keep_mask(5, 9, 0.5, 98, 3))
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[0, 0], a[0, 1])
    assert R.keep_mask(2, 6, 0.0, 1, 1).all() and R.threshold(0.5) == 1 << 31


def test_module_has_multihead_attention_keys_and_shapes():
    ref = nn.MultiheadAttention(768, 12, dropout=0.1)
    mod = bga.MultiheadSelfAttention(768, 12, dropout=0.1)
    a, b = ref.state_dict(), mod.state_dict()
    assert list(a) == list(b) == ["in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"]
    assert all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)
    mod.load_state_dict(a, strict=True)
    assert (mod.batch_first, mod._qkv_same_embed_dim, mod.num_heads, mod.embed_dim) == (False, True, 12, 768)
    with pytest.raises(ValueError):
        bga.MultiheadSelfAttention(512, 8)


def test_use_device_attention_keeps_keys_and_parameter_identity():
    enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(768, 12, 1024, dropout=0.1, norm_first=True), 2, nn.LayerNorm(768))
    keys, params = list(enc.state_dict()), list(enc.parameters())
    opt = torch.optim.AdamW(enc.parameters())
    assert bga.use_device_attention(enc, seed=5) is enc
    assert list(enc.state_dict()) == keys
    after = list(enc.parameters())
    assert len(after) == len(params) and all(x is y for x, y in zip(after, params))
    assert all(x is y for x, y in zip(opt.param_groups[0]["params"], after))
    mods = [l.self_attn for l in enc.layers]
    assert all(isinstance(m, attention.MultiheadSelfAttention) and m.dropout == 0.1 and m.seed == 5 and m.n_layers == 2 for m in mods)
    assert [m.layer_index for m in mods] == [0, 1]
    # draw ids: no two (layer, call) pairs share one
    ids = [m.next_draw_id() for _ in range(4) for m in mods]
    assert len(set(ids)) == 8 and ids[:4] == [0, 1, 2, 3]
    bga.use_device_attention(enc)                              # idempotent
    assert [l.self_attn for l in enc.layers] == mods and list(enc.state_dict()) == keys


def test_unsupported_calls_and_cpu_tensors_raise():
    mod = bga.MultiheadSelfAttention()
    x = torch.zeros(4, 2, 768)
    with pytest.raises(NotImplementedError):
        mod(x, x.clone(), x, need_weights=False)
    with pytest.raises(NotImplementedError):
        mod(x, x, x, attn_mask=torch.zeros(4, 4), need_weights=False)
    with pytest.raises(NotImplementedError):
        mod(x, x, x, need_weights=True)
    with pytest.raises(_lib.BrepgenHipError):
        mod(x, x, x, need_weights=False)
    with pytest.raises(_lib.BrepgenHipError):
        bga.self_attention(torch.zeros(2, 4, 2304))


def test_argument_errors_are_negative_and_explained():
    lib = _lib.load()
    f = FAKE                                         # aligned, never dereferenced: validation fails before any launch

    def fwd(qkv=f, out=f, lse=f, B=2, N=8, dt=BF, scale=0.125, p=0.0, first=0):
        return lib.bg_attn_train_fwd(qkv, None, out, lse, B, N, dt, scale, p, 1, 0, first, None)

    def bwd(qkv=f, lse=f, dout=f, dqkv=f, B=2, N=8, dt=BF, scale=0.125, p=0.0, ws=f, nbytes=1 << 20, variant=0, first=0):
        return lib.bg_attn_bwd(qkv, None, lse, dout, dqkv, B, N, dt, scale, p, 1, 0, first, variant, ws, nbytes, None)

    def mask(m=f, B=2, N=8, p=0.1):
        return lib.bg_attn_dropout_mask(m, B, N, p, 1, 0, 0, None)

    bad = [(lambda: fwd(N=0), -1, b"N = 0"), (lambda: fwd(dt=9), -4, b"dtype"), (lambda: fwd(p=1.0), -1, b"dropout_p"),
           (lambda: fwd(p=-0.1), -1, b"dropout_p"), (lambda: fwd(p=float("nan")), -1, b"dropout_p"),
           (lambda: fwd(qkv=None), -1, b"null"), (lambda: fwd(lse=None), -1, b"null"), (lambda: fwd(out=f + 2), -5, b"alignment"),
           (lambda: fwd(B=-1), -1, b"B = -1"), (lambda: fwd(first=-1), -1, b"first_sample"), (lambda: fwd(scale=float("inf")), -1, b"scale"),
           (lambda: fwd(N=70000, p=0.1), -2, b"dropout counter"),
           (lambda: bwd(N=0), -1, b"N = 0"), (lambda: bwd(dt=9), -4, b"dtype"), (lambda: bwd(p=1.5), -1, b"dropout_p"),
           (lambda: bwd(dout=None), -1, b"null"), (lambda: bwd(dqkv=None), -1, b"null"), (lambda: bwd(qkv=f + 4), -5, b"alignment"),
           (lambda: bwd(ws=None), -3, b"workspace"), (lambda: bwd(nbytes=16), -3, b"workspace"),
           (lambda: bwd(dt=_lib.BG_F32, N=6000, nbytes=1 << 22), -2, b"too long"),
           (lambda: bwd(variant=3), -1, b"variant"), (lambda: bwd(variant=2, N=65), -2, b"short-sequence"),
           (lambda: bwd(variant=2, dt=_lib.BG_F32), -2, b"short-sequence"), (lambda: bwd(first=(1 << 44) - 1), -1, b"2^44"),
           (lambda: fwd(first=1 << 44, B=1), -1, b"2^44"),
           (lambda: mask(N=0), -1, b"N = 0"), (lambda: mask(m=None), -1, b"null"), (lambda: mask(p=1.0), -1, b"dropout_p"),
           (lambda: mask(B=-2), -1, b"negative")]
    for call, code, text in bad:
        rc = call()
        assert rc == code and text in lib.bg_last_error(), (rc, code, text, lib.bg_last_error())
    # B == 0: nothing to do, no launch
    assert fwd(B=0) == 0 and bwd(B=0) == 0 and mask(B=0) == 0
    # the workspace: delta [B, 12, N] fp32 (fp32: + row maximum and row sum), rounded up to 256 bytes; 0 for arguments bg_attn_bwd rejects
    w = lib.bg_attn_bwd_workspace_bytes
    assert w(2, 8, BF) == 768 and w(3, 50, _lib.BG_F16) == 7424 and w(3, 50, _lib.BG_F32) == 21760 and w(0, 8, BF) == 0 and w(2, 0, BF) == 0 and w(2, 8, 9) == 0


def test_header_prototypes_match_the_binding():
    lib = _lib.load()
    src = open(os.path.join(ROOT, "include", "brepgen_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ctype = {"const void*": C.c_void_p, "void*": C.c_void_p, "const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p, "float*": C.c_void_p,
             "const float*": C.c_void_p, "int": C.c_int, "float": C.c_float, "double": C.c_double, "unsigned long long": C.c_ulonglong,
             "unsigned": C.c_uint, "long long": C.c_longlong, "size_t": C.c_size_t, "bg_stream_t": C.c_void_p}
    for name in NEW:
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        args = [ctype[a.strip().rsplit(" ", 1)[0].strip()] for a in m.group(2).split(",")]
        res, want = _lib._SIGNATURES[name]
        assert args == want, (name, args, want)
        assert res is (C.c_int if m.group(1) == "int" else C.c_size_t)
        assert getattr(lib, name).argtypes == want
    assert_exported(NEW)


def test_training_attention_kernels_use_no_scratch():
    """Every kernel of csrc/attn_train.hip: no scratch memory and no spilled VGPR (the backward kernels keep up to 64 accumulators, 32
    score registers and 32 operand registers live; a spill would put scratch traffic into the tile loop)."""
    names, scratch, spills, _ = resource_usage("attn_train.hip")
    assert len(names) == 23, names                   # 4 forward + 8 general + 4 short backward 16-bit, 2 + 4 fp32, the mask kernel
    assert all(v == 0 for v in scratch + spills), list(zip(names, scratch, spills))
