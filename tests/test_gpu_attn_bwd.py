"""The training attention core on the device (csrc/attn_train.hip, brepgen_amd/attention.py) against its fp64 restatement
(tests/attn_bwd_restate.py), with torch's own result on the same GPU as the yardstick of every tolerance.

Accuracy.  For every (dtype, N) the cases B in {1, 3} x {no mask, ragged tail, scattered padding, one all-padded sample} are run;
the absolute errors against fp64 of this op and of torch (autograd of F.scaled_dot_product_attention, math backend, same dtype, same
GPU, same rounded inputs) are pooled over those eight cases, and this op's max and mean error must be <= 2 x torch's, separately for
out, dQ, dK and dV.  All-padded samples are left out of the pooled errors (torch gives NaN there) and must be exactly 0 here.
lse has no torch counterpart: a score is a sum of 64 exact products of magnitude <= ~128 accumulated in fp32 (<= 64 * 2^-24 * 128 =
5e-4 in the worst case) and the log of a sum of fast exponentials adds ~1e-6, so |lse - fp64| <= 1e-3.
The one long case (B = 2, N = 1500) takes its fp64 reference from the same formula in torch ops on the device
(tests/attn_train_ops.py torch_grads, pinned to the restatement at 1e-12 by tests/test_attn_bwd_cpu.py).
With dropout the yardstick is at the same level as the math backend's: that formula (softmax, explicit keep mask, matmul) evaluated
in fp32 from the same 16-bit inputs under torch's autograd, results rounded once to the dtype.
Every N <= 64 runs the general path AND, for the 16-bit dtypes, the short-sequence kernel (bg_attn_bwd's `variant`), each against the
same bounds.  lse: 1e-3 for the 16-bit kernels (above); the fp32 kernel accumulates a score in fp64 and rounds once (half an ulp of
|S| <= 16: 1e-6), the sum of exponentials and its log add a few 1e-7 and lse itself (|lse| <= 16) rounds by 1e-6: 1e-5.
BG_ATTN_PARITY_JSON=<path> makes the run write the measured pairs there (profiles/r13/attn_bwd_parity.json is such a run)."""
import copy
import json

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.attention import SDPBackend, sdpa_kernel

import brepgen_amd as bga
from brepgen_amd import optim  # noqa: F401
from tests import attn_bwd_restate as R
from tests import attn_train_ops as ops
from tests import hip_ops
from tests.guarded import guarded
from tests.train_check import Parity, encoder, encoder_grads, errs, same_bits

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
NS = [1, 2, 5, 31, 32, 33, 50, 63, 64, 65, 96, 127, 128, 129, 200]
PARTS = ("out", "dq", "dk", "dv")
GENERAL, SHORT = ops._lib.BG_ATTN_BWD_GENERAL, ops._lib.BG_ATTN_BWD_SHORT
VNAME = {GENERAL: "general", SHORT: "short"}
HALF = [torch.float16, torch.bfloat16]
LSE_TOL = {torch.float32: 1e-5, torch.float16: 1e-3, torch.bfloat16: 1e-3}
_PAIRS = {}


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t if dtype is None else t.to(dtype)).cuda()


def _kernel(case, dtype, p=0.0, seed=0, draw=0, first=0, variant=GENERAL):
    B, N = case["B"], case["N"]
    qkv, dout = case["qkv_t"].cuda().reshape(B * N, 2304), case["dout_t"].cuda().reshape(B * N, 768)
    kp = None if case["key_pad"] is None else _dev(case["key_pad"].astype(np.uint8))
    out, lse = ops.train_fwd(qkv, kp, B, N, 0.125, p, seed, draw, first)
    dqkv = ops.bwd(qkv, kp, lse, dout, B, N, 0.125, p, seed, draw, first, variant=variant)
    return out.reshape(B, N, 768), lse, dqkv.reshape(B, N, 2304)


def _torch_sdpa(case, live):
    """(out, dqkv) of F.scaled_dot_product_attention (math backend) on the live samples, in the case's dtype."""
    B, N = len(live), case["N"]
    x = case["qkv_t"][live].cuda().requires_grad_(True)
    q, k, v = (x[..., i * 768:(i + 1) * 768].reshape(B, N, 12, 64).transpose(1, 2) for i in range(3))
    am = None if case["key_pad"] is None else ~_dev(case["key_pad"][live])[:, None, None, :]
    with sdpa_kernel(SDPBackend.MATH):
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=am, scale=0.125).transpose(1, 2).reshape(B, N, 768)
    o.backward(case["dout_t"][live].cuda())
    return o.detach(), x.grad


def _split_err(out, dqkv, ref_out, ref_dqkv):
    """absolute errors against fp64 as flat fp64 arrays, by part"""
    e = {"out": (out.double().cpu().numpy() - ref_out)}
    d = dqkv.double().cpu().numpy() - ref_dqkv
    e["dq"], e["dk"], e["dv"] = d[..., :768], d[..., 768:1536], d[..., 1536:]
    return {k: np.abs(v).reshape(-1) for k, v in e.items()}


def _pool_and_assert(tag, mine, theirs):
    rec = {}
    for part in PARTS:
        m, t = np.concatenate(mine[part]), np.concatenate(theirs[part])
        rec[part] = dict(max=float(m.max()), mean=float(m.mean()), torch_max=float(t.max()), torch_mean=float(t.mean()))
    _PAIRS[tag] = rec
    print(tag, json.dumps(rec))
    for part in PARTS:
        r = rec[part]
        assert r["max"] <= 2 * r["torch_max"] and r["mean"] <= 2 * r["torch_mean"], (tag, part, r)


ACC_CASES = [(d, n, GENERAL) for d in DTYPES for n in NS] + [(d, n, SHORT) for d in HALF for n in NS if n <= 64]


@pytest.mark.parametrize("dtype,N,variant", ACC_CASES, ids=[f"{str(d)[6:]}-{n}-{VNAME[v]}" for d, n, v in ACC_CASES])
def test_accuracy_against_fp64_within_twice_torch(dtype, N, variant):
    mine = {k: [] for k in PARTS}
    theirs = {k: [] for k in PARTS}
    for B in (1, 3):
        for ki, kind in enumerate(ops.MASK_KINDS):
            case = ops.make_case(B, N, kind, 1000 * N + 10 * B + ki, dtype)
            kp = case["key_pad"]
            out, lse, dqkv = _kernel(case, dtype, variant=variant)
            ref_out, ref_lse = R.forward(case["qkv"], kp)
            ref_d = R.backward(case["qkv"], case["dout"], kp)
            assert np.isfinite(lse.cpu().numpy()).all() and np.abs(lse.cpu().numpy() - ref_lse).max() <= LSE_TOL[dtype]
            if variant == SHORT:                                    # the short kernel's dQ is the general path's, bit for bit
                assert torch.equal(dqkv[..., :768].contiguous().view(torch.uint8),
                                   _kernel(case, dtype)[2][..., :768].contiguous().view(torch.uint8))
            live = [b for b in range(B) if kp is None or not kp[b].all()]
            for b in set(range(B)) - set(live):                     # all-padded: exactly 0, never NaN
                assert not out[b].any() and not dqkv[b].any() and not lse[b].any()
            if not live:
                continue
            t_out, t_d = _torch_sdpa(case, live)
            em = _split_err(out[live], dqkv[live], ref_out[live], ref_d[live])
            et = _split_err(t_out, t_d, ref_out[live], ref_d[live])
            for part in PARTS:
                mine[part].append(em[part])
                theirs[part].append(et[part])
            if kp is not None:                                      # padded keys: dK and dV rows exactly 0
                dead = _dev(kp)
                assert not dqkv[..., 768:][dead].any()
    _pool_and_assert(f"p0/{str(dtype)[6:]}/N{N}" + ("/short" if variant == SHORT else ""), mine, theirs)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
def test_accuracy_at_the_edge_trainers_bound(dtype):
    """B = 2, N = 1500 (50 faces x 30 edges), ragged tail mask."""
    case = ops.make_case(2, 1500, "tail", 77, dtype)
    kp = _dev(case["key_pad"])
    out, lse, dqkv = _kernel(case, dtype)
    ref_out, ref_d = ops.torch_grads(case["qkv_t"].cuda().double(), case["dout_t"].cuda().double(), kp, 0.125)
    t_out, t_d = _torch_sdpa(case, [0, 1])
    ref_out, ref_d = ref_out.cpu().numpy(), ref_d.cpu().numpy()
    em, et = _split_err(out, dqkv, ref_out, ref_d), _split_err(t_out, t_d, ref_out, ref_d)
    assert not dqkv[..., 768:][kp].any() and torch.isfinite(lse).all()
    _pool_and_assert(f"p0/{str(dtype)[6:]}/N1500", {k: [v] for k, v in em.items()}, {k: [v] for k, v in et.items()})


@pytest.mark.parametrize("first", [0, 2 ** 32 + 3])
@pytest.mark.parametrize("N", [5, 64, 130])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_mask_equals_the_restatement_bit_for_bit(p, N, first):
    B, seed, draw = 2, 0xC0FFEE1234567, 41
    m = ops.dropout_mask(B, N, p, seed, draw, first).cpu().numpy()
    assert np.array_equal(m, R.keep_mask(B, N, p, seed, draw, first))
    n = m.size
    assert abs(m.mean() - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n)


DROP_CASES = [(d, p, n, GENERAL) for d in DTYPES for p in (0.1, 0.5) for n in (5, 64, 130)] + \
             [(d, p, n, SHORT) for d in HALF for p in (0.1, 0.5) for n in (5, 64)]


@pytest.mark.parametrize("dtype,p,N,variant", DROP_CASES, ids=[f"{str(d)[6:]}-{p}-{n}-{VNAME[v]}" for d, p, n, v in DROP_CASES])
def test_dropout_accuracy_with_the_restated_mask(dtype, p, N, variant):
    """The kernels regenerate the mask (forward, dQ and dK/dV kernel, short kernel, each on its own): with the restated mask fed to the
    fp64 restatement, out and dqkv stay within twice the error of the formula evaluated in fp32 and rounded once (the level of the
    p = 0 yardstick); the same mask serves every dtype and both backward paths."""
    B, seed, draw, first = 3, 0xABCDEF0123, 9, 6
    case = ops.make_case(B, N, "tail", 5000 + N, dtype)
    kp = case["key_pad"]
    keep = R.keep_mask(B, N, p, seed, draw, first)
    out, lse, dqkv = _kernel(case, dtype, p, seed, draw, first, variant=variant)
    ref_out, ref_lse = R.forward(case["qkv"], kp, keep=keep, p=p)
    ref_d = R.backward(case["qkv"], case["dout"], kp, keep=keep, p=p)
    assert np.abs(lse.cpu().numpy() - ref_lse).max() <= LSE_TOL[dtype]     # lse does not see the mask
    t_out, t_d = ops.torch_grads(case["qkv_t"].cuda().float(), case["dout_t"].cuda().float(), _dev(kp), 0.125, _dev(keep), R.rp_of(p))
    t_out, t_d = t_out.to(dtype), t_d.to(dtype)
    em, et = _split_err(out, dqkv, ref_out, ref_d), _split_err(t_out, t_d, ref_out, ref_d)
    _pool_and_assert(f"p{p}/{str(dtype)[6:]}/N{N}" + ("/short" if variant == SHORT else ""), {k: [v] for k, v in em.items()}, {k: [v] for k, v in et.items()})


INV_CASES = [(d, n, GENERAL) for d in DTYPES for n in (50, 130)] + [(d, 50, SHORT) for d in HALF]


@pytest.mark.parametrize("dtype,N,variant", INV_CASES, ids=[f"{str(d)[6:]}-{n}-{VNAME[v]}" for d, n, v in INV_CASES])
def test_bitwise_invariants(dtype, N, variant):
    p, seed, draw = 0.1, 31337, 2
    case = ops.make_case(5, N, "one_empty", 9000 + N, dtype)
    kp = case["key_pad"]
    a = _kernel(case, dtype, p, seed, draw, variant=variant)
    b = _kernel(case, dtype, p, seed, draw, variant=variant)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))          # two identical calls
    out, lse, dqkv = a
    assert not dqkv[..., 768:][_dev(kp)].any()                                                       # padded keys: dK = dV = 0
    assert not out[4].any() and not dqkv[4].any() and not lse[4].any()                               # the all-padded sample
    # the other samples replaced: sample 1 keeps its bits
    other = ops.make_case(5, N, "one_empty", 9500 + N, dtype)
    for k in ("qkv_t", "dout_t"):
        other[k][1] = case[k][1]
    other["key_pad"][1] = kp[1]
    o2, l2, d2 = _kernel(other, dtype, p, seed, draw, variant=variant)
    assert torch.equal(o2[1].view(torch.uint8), out[1].view(torch.uint8)) and torch.equal(d2[1].view(torch.uint8), dqkv[1].view(torch.uint8))
    assert torch.equal(l2[1], lse[1]) and not torch.equal(d2[0].view(torch.uint8), dqkv[0].view(torch.uint8))
    # rows [2:5] of the B = 5 call = a B = 3 call with first_sample = 2
    sub = dict(case, B=3, qkv_t=case["qkv_t"][2:], dout_t=case["dout_t"][2:], key_pad=kp[2:])
    o3, l3, d3 = _kernel(sub, dtype, p, seed, draw, first=2, variant=variant)
    assert torch.equal(o3.view(torch.uint8), out[2:].view(torch.uint8)) and torch.equal(d3.view(torch.uint8), dqkv[2:].view(torch.uint8))
    o4, _, _ = _kernel(sub, dtype, p, seed, draw, first=0)                                            # ... and not with another one
    assert not torch.equal(o4.view(torch.uint8), out[2:].view(torch.uint8))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("N", [5, 33, 64])
@pytest.mark.parametrize("dtype", HALF, ids=["fp16", "bf16"])
def test_short_and_general_backward_agree_on_dq_bit_for_bit(dtype, N, p):
    """The one-launch kernel forms dQ by the general path's arithmetic in the same order (its helpers in csrc/attn_tile.h restate the
    general kernel's own text): the same bytes, with and without dropout, with an all-padded sample in the batch.  (dK and dV are
    rounded through LDS images there: not compared.)"""
    case = ops.make_case(3, N, "one_empty", 7000 + N, dtype)
    short = _kernel(case, dtype, p, 99, 4, variant=SHORT)[2]
    general = _kernel(case, dtype, p, 99, 4, variant=GENERAL)[2]
    assert same_bits(short[..., :768], general[..., :768], typed=False)


@pytest.mark.parametrize("N", [5, 33, 64])
@pytest.mark.parametrize("dtype", HALF, ids=["fp16", "bf16"])
def test_training_forward_equals_the_inference_kernel_bit_for_bit(dtype, N):
    """bg_attn_train_fwd with scale 1 and no dropout is bg_attn_fwd (which expects q pre-scaled): the same bytes of `out`.  N <= 64:
    longer sequences take attn16_long_kernel, whose deferred maximum differs by design."""
    B = 3
    case = ops.make_case(B, N, "tail", 8000 + N, dtype)
    qkv = case["qkv_t"].cuda().reshape(B * N, 2304)
    kp = _dev(case["key_pad"].astype(np.uint8))
    out_train, _ = ops.train_fwd(qkv, kp, B, N, 1.0, 0.0)
    assert same_bits(out_train, hip_ops.attention(qkv, kp, B, N), typed=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("N", [5, 65, 130])
def test_guarded_buffers(dtype, N):
    """out, lse, dqkv and the workspace's delta are fully written, guards untouched; qkv / out / dout rows beyond B * N hold NaN
    sentinels and never reach a result."""
    B, p, seed = 3, 0.1, 5
    case = ops.make_case(B, N, "tail", 400 + N, dtype)
    kp = _dev(case["key_pad"].astype(np.uint8))
    gq, gdo = guarded((B * N + 2, 2304), dtype, "cuda"), guarded((B * N + 2, 768), dtype, "cuda")
    gq.view[:B * N].copy_(case["qkv_t"].reshape(B * N, 2304))
    gdo.view[:B * N].copy_(case["dout_t"].reshape(B * N, 768))
    go, gl, gd = guarded((B * N, 768), dtype, "cuda"), guarded((B * 12, N), torch.float32, "cuda"), guarded((B * N, 2304), dtype, "cuda")
    nbytes = ops._lib.load().bg_attn_bwd_workspace_bytes(B, N, ops.DT[dtype])
    gw = guarded((1, nbytes // 4), torch.float32, "cuda")
    ops.train_fwd(gq.view, kp, B, N, 0.125, p, seed, 1, 0, out=go.view, lse=gl.view)
    ops.bwd(gq.view, kp, gl.view, gdo.view, B, N, 0.125, p, seed, 1, 0, dqkv=gd.view, ws=(gw.view, nbytes))
    torch.cuda.synchronize()
    for g, what in ((go, "out"), (gl, "lse"), (gd, "dqkv")):
        g.assert_fully_written(what)
        g.assert_untouched(what)
    gw.assert_untouched("workspace")
    assert gw.written_mask()[0, :B * 12 * N * (3 if dtype == torch.float32 else 1)].all()
    for g in (gq, gdo):
        g.assert_untouched("input")
    if dtype in HALF and N <= 64:                                   # the short kernel: every element of dqkv again, same guards
        gs = guarded((B * N, 2304), dtype, "cuda")
        ops.bwd(gq.view, kp, gl.view, gdo.view, B, N, 0.125, p, seed, 1, 0, dqkv=gs.view, ws=(gw.view, nbytes), variant=SHORT)
        torch.cuda.synchronize()
        gs.assert_fully_written("dqkv (short)")
        gs.assert_untouched("dqkv (short)")
        assert torch.isfinite(gs.view.float()).all()
        assert torch.equal(gs.view[:, :768].contiguous().view(torch.uint8), gd.view[:, :768].contiguous().view(torch.uint8))
    ref = _kernel(case, dtype, p, seed, 1, 0)
    assert torch.equal(go.view.view(torch.uint8), ref[0].reshape(B * N, 768).view(torch.uint8))
    assert torch.equal(gd.view.view(torch.uint8), ref[2].reshape(B * N, 2304).view(torch.uint8))
    assert torch.isfinite(go.view.float()).all() and torch.isfinite(gd.view.float()).all() and torch.isfinite(gl.view).all()


def test_autograd_under_autocast_with_a_scaled_loss():
    """MultiheadSelfAttention against nn.MultiheadAttention with the same weights under fp16 autocast and a GradScaler-scaled loss: the
    weight gradients' error against fp64 is within twice torch's own."""
    torch.manual_seed(3)
    N, B = 50, 4
    ref64 = nn.MultiheadAttention(768, 12, dropout=0.0).cuda().double()
    with torch.no_grad():
        ref64.in_proj_weight.mul_(3.0)                        # scores with a standard deviation of ~1 instead of ~0.3
    x64 = torch.randn(N, B, 768, dtype=torch.float64, device="cuda")
    w64 = torch.randn(N, B, 768, dtype=torch.float64, device="cuda")
    kpm = torch.zeros(B, N, dtype=torch.bool, device="cuda")
    kpm[1, 30:] = True
    kpm[3, 7:] = True
    y, _ = ref64(x64, x64, x64, key_padding_mask=kpm, need_weights=False)
    (y * w64).mean().backward()
    tor = copy.deepcopy(ref64).float()
    mine = bga.MultiheadSelfAttention(768, 12)
    mine.load_state_dict(tor.state_dict())
    mine = mine.cuda()
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    grads = {}
    for name, mod in (("torch", tor), ("mine", mine)):
        mod.zero_grad()
        x = x64.float()
        with torch.autocast("cuda", torch.float16):
            y, none = mod(x, x, x, key_padding_mask=kpm, need_weights=False)
            loss = (y.float() * w64.float()).mean()
        assert none is None
        scaler.scale(loss).backward()
        grads[name] = {k: getattr(mod, k).grad / 65536.0 for k in ("in_proj_weight",)}
        grads[name]["out_proj.weight"] = mod.out_proj.weight.grad / 65536.0
    for k, ref in (("in_proj_weight", ref64.in_proj_weight.grad), ("out_proj.weight", ref64.out_proj.weight.grad)):
        (mm, ma), (tm, ta) = errs(grads["mine"][k], ref), errs(grads["torch"][k], ref)
        print("autocast", k, mm, ma, tm, ta)
        assert torch.isfinite(grads["mine"][k]).all() and mm <= 2 * tm and ma <= 2 * ta, (k, mm, ma, tm, ta)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
def test_an_inf_in_dout_reaches_the_gradients_of_its_sample_only(dtype):
    case = ops.make_case(3, 40, "tail", 123, dtype)
    qkv = case["qkv_t"].cuda().requires_grad_(True)
    out = bga.self_attention(qkv, _dev(case["key_pad"]))
    dout = case["dout_t"].cuda().clone()
    dout[1, 3, 100] = float("inf")
    out.backward(dout)
    g = qkv.grad
    assert not torch.isfinite(g[1]).all() and torch.isfinite(g[0]).all() and torch.isfinite(g[2]).all()


def test_two_layer_encoder_forward_and_backward_fp32():
    enc = encoder(0.0, 11)
    torch.manual_seed(12)
    x, w = torch.randn(7, 3, 768, device="cuda"), torch.randn(7, 3, 768, device="cuda") / 64
    kpm = torch.zeros(3, 7, dtype=torch.bool, device="cuda")
    kpm[0, 5:] = True
    kpm[2, 2:] = True
    _, g64 = encoder_grads(copy.deepcopy(enc).double(), x.double(), kpm, w.double(), fp64=False)
    y_t, g_t = encoder_grads(enc, x, kpm, w, fp64=False)
    keys = list(enc.state_dict())
    bga.use_device_attention(enc)
    assert list(enc.state_dict()) == keys
    y_m, g_m = encoder_grads(enc, x, kpm, w, fp64=False)
    assert float((y_m - y_t).abs().max()) <= 1e-4
    L = 2
    for k in g64:
        (mm, ma), (tm, ta) = errs(g_m[k], g64[k]), errs(g_t[k], g64[k])
        assert mm <= 2 * L * tm + 1e-30 and ma <= 2 * L * ta + 1e-30, (k, mm, ma, tm, ta)


def test_two_layer_encoder_dropout_streams():
    enc = bga.use_device_attention(encoder(0.1, 11), seed=77)
    torch.manual_seed(13)
    x, w = torch.randn(7, 3, 768, device="cuda"), torch.randn(7, 3, 768, device="cuda") / 64
    kpm = torch.zeros(3, 7, dtype=torch.bool, device="cuda")
    kpm[1, 4:] = True
    mods = [l.self_attn for l in enc.layers]

    def run(calls):
        torch.manual_seed(99)                                  # the layers' own nn.Dropout draws from torch's generator
        for m in mods:
            m.calls = calls
        return encoder_grads(enc, x, kpm, w, fp64=False)

    enc.train()
    y0, g0 = run(0)
    y1, g1 = run(1)                                            # only the attention's call counter differs
    y0b, g0b = run(0)
    assert not torch.equal(y0, y1)
    assert torch.equal(y0, y0b) and all(torch.equal(g0[k], g0b[k]) for k in g0)
    assert [m.calls for m in mods] == [1, 1]
    # eval(): no mask anywhere -- the bits of an encoder built with dropout = 0
    enc.eval()
    y_e, g_e = encoder_grads(enc, x, kpm, w, fp64=False)
    plain = bga.use_device_attention(encoder(0.0, 11))
    plain.load_state_dict(enc.state_dict())
    plain.train()
    y_p, g_p = encoder_grads(plain, x, kpm, w, fp64=False)
    assert torch.equal(y_e, y_p) and all(torch.equal(g_e[k], g_p[k]) for k in g_e)


def test_eval_and_no_grad_forward_of_the_converted_encoder():
    """eval() / no_grad of the surrounding torch layers still works after the swap (the fast-path check reads the module's attributes)
    and gives the stock encoder's result."""
    enc = encoder(0.1, 11).eval()
    torch.manual_seed(14)
    x = torch.randn(7, 3, 768, device="cuda")
    kpm = torch.zeros(3, 7, dtype=torch.bool, device="cuda")
    kpm[1, 4:] = True
    with torch.no_grad():
        y_t = enc(x, src_key_padding_mask=kpm)
        bga.use_device_attention(enc)
        y_m = enc(x, src_key_padding_mask=kpm)
        y_u = enc(x)                                               # no mask at all
    assert y_m.shape == y_t.shape and torch.isfinite(y_m).all() and torch.isfinite(y_u).all()
    assert float((y_m - y_t)[:, 0].abs().max()) <= 1e-4 and float((y_m - y_t)[:4, 1].abs().max()) <= 1e-4


def test_zz_write_parity_pairs():
    """Not a check of its own: writes the pairs measured above where BG_ATTN_PARITY_JSON points."""
    if _PAIRS:
        Parity("BG_ATTN_PARITY_JSON", "absolute error against fp64, pooled over B in {1, 3} x four masks per (dtype, N); torch = autograd of "
               "F.scaled_dot_product_attention (math backend) for p0, of the explicit-mask formula for dropout").write(_PAIRS)
