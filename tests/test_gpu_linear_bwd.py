"""The Linear layers' backward on the device (csrc/linear_bwd.hip, brepgen_amd/linear.py) against fp64 evaluated from the same rounded
inputs, with two kinds of bound:

(a) derived, fp32 output: a product of two 16-bit values is exact in fp32, every output is a sum of M of them in at most M + S fp32
    additions, so  |dw - ref| <= (M + S + 2) 2^-24 sum_m |dy[m,n]| |x[m,k]|  and  |db - ref| <= (M + S + 2) 2^-24 sum_m |dy[m,n]|;
(b) the project's yardstick (tests/test_gpu_attn_bwd.py): pooled max and mean absolute error <= 2 x torch's on the same GPU from the
    same inputs -- `dy.t() @ x` in the 16-bit dtype for the 16-bit output, `dy.float().t() @ x.float()` for the fp32 output.  db has
    no asserted torch ratio (a tree reduction and a row walk grow their errors differently); the pair is recorded.

BG_LINEAR_PARITY_JSON=<path> makes the run write the measured pairs there (profiles/r14/linear_bwd_parity.json is such a run)."""
import copy
import functools
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import brepgen_amd as bga
from brepgen_amd import linear as L
from tests import linear_ops as ops
from tests.guarded import guarded, strided_input
from tests.train_check import Parity, encoder_grads, errs

pytestmark = pytest.mark.gpu
DTYPES = (torch.float16, torch.bfloat16)
NAME = ops.NAME
PARITY = Parity("BG_LINEAR_PARITY_JSON")
record, within_2x, _parity_json = PARITY.record, PARITY.within_2x, PARITY.fixture()


@functools.lru_cache(maxsize=None)
def case(M, N, K, dtype, seed=0):
    """inputs, the fp64 reference and torch's two results -- computed once, shared, never modified"""
    dy, x = ops.draw(M, N, K, dtype, 1000 * seed + M)
    ref_w, ref_b, abs_w, abs_b = ops.reference(dy, x)
    t16 = errs(dy.t() @ x, ref_w)
    t32 = errs(dy.float().t() @ x.float(), ref_w)
    tb16, tb32 = errs(dy.sum(0), ref_b), errs(dy.float().sum(0), ref_b)
    return dy, x, ref_w, ref_b, abs_w, abs_b, {torch.float32: (t32, tb32), dtype: (t16, tb16)}


def check_bound_a(dw, db, M, S, ref_w, ref_b, abs_w, abs_b, what):
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), what
    f = (M + S + 2) * ops.U24
    ew, eb = (dw.double() - ref_w).abs(), (db.double() - ref_b).abs()
    worst_w, worst_b = float((ew / (f * abs_w).clamp_min(1e-300)).max()), float((eb / (f * abs_b).clamp_min(1e-300)).max())
    print(f"{what}: bound (a) used to {worst_w:.3f} (dw), {worst_b:.3f} (db)")
    assert bool((ew <= f * abs_w).all()), (what, "dw", worst_w)
    assert bool((eb <= f * abs_b).all()), (what, "db", worst_b)


SMALL_M = (1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 200, 1000)
WGRAD_CASES = [(M, 128, 128) for M in SMALL_M] + [(M, N, K) for (N, K) in ((256, 128), (128, 256), (768, 1024), (2304, 768)) for M in (65, 1000)]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("M, N, K", WGRAD_CASES)
def test_wgrad_accuracy(M, N, K, dtype):
    dy, x, ref_w, ref_b, abs_w, abs_b, torchs = case(M, N, K, dtype)
    for split in (1, 0) + ((3, 7) if M >= 200 else ()):
        S = split or ops.auto_split(M, N, K)
        for odt in (torch.float32, dtype):
            tag = f"wgrad M={M} N={N} K={K} {NAME[dtype]}->{NAME[odt]} split={split}(S={S})"
            dw, db = ops.wgrad(dy, x, M, N, K, odt, split)
            if odt == torch.float32:
                check_bound_a(dw, db, M, S, ref_w, ref_b, abs_w, abs_b, tag)
            record(tag, "db", errs(db, ref_b), torchs[odt][1])
            within_2x(tag, "dw", errs(dw, ref_w), torchs[odt][0])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_wgrad_bits(dtype):
    M, N, K = 1000, 256, 128
    dy, x, ref_w, ref_b, abs_w, abs_b, _ = case(M, N, K, dtype)
    for split in (1, 3, 0):
        a, b = ops.wgrad(dy, x, M, N, K, torch.float32, split), ops.wgrad(dy, x, M, N, K, torch.float32, split)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), split                 # two calls, identical bits
    (w1, b1), (w3, b3) = ops.wgrad(dy, x, M, N, K, torch.float32, 1), ops.wgrad(dy, x, M, N, K, torch.float32, 3)
    # each is within (a) of the reference (test_wgrad_accuracy), so they agree within the sum of their bounds
    f = ((M + 1 + 2) + (M + 3 + 2)) * ops.U24
    assert bool(((w1.double() - w3.double()).abs() <= f * abs_w).all()) and bool(((b1.double() - b3.double()).abs() <= f * abs_b).all())
    # the workgroup order is a placement choice only: plain block order (BG_LINEAR_WGRAD_WALK=plain, read at every call) gives the same bits
    for split in (1, 3):
        xcd = ops.wgrad(dy, x, M, N, K, torch.float32, split)
        try:
            os.environ["BG_LINEAR_WGRAD_WALK"] = "plain"
            plain = ops.wgrad(dy, x, M, N, K, torch.float32, split)
        finally:
            os.environ.pop("BG_LINEAR_WGRAD_WALK", None)
        assert torch.equal(xcd[0], plain[0]) and torch.equal(xcd[1], plain[1]), split
    # a row of dw depends on its own dy column alone
    n0 = 77
    dy2 = dy.clone()
    dy2[:, n0] = dy2[:, n0] * 0.5 + 1.0
    for split in (1, 3):
        (wa, ba), (wb, bb) = ops.wgrad(dy, x, M, N, K, torch.float32, split), ops.wgrad(dy2, x, M, N, K, torch.float32, split)
        others = torch.arange(N, device=dy.device) != n0
        assert torch.equal(wa[others], wb[others]) and torch.equal(ba[others], bb[others])
        assert not torch.equal(wa[n0], wb[n0]) and not torch.equal(ba[n0], bb[n0])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("M, split", [(1, 1), (65, 1), (65, 3), (129, 1), (129, 3), (129, 0)])
def test_wgrad_guarded(M, split, dtype):
    """ld > columns, NaN-sentinel padding and guard bands around dy / x: a padding column or a row >= M in any product makes the
    result NaN.  dw / db / workspace: every promised element written, nothing outside."""
    N, K = 256, 128
    dy, x, ref_w, ref_b, abs_w, abs_b, _ = case(M, N, K, dtype)
    dys, xs = strided_input(dy, N + 8), strided_input(x, K + 24)
    S = split or ops.auto_split(M, N, K)
    for odt in (torch.float32, dtype):
        gw, gb = guarded((N, K), odt, "cuda"), guarded((N,), odt, "cuda")
        nws = ops.workspace_bytes(M, N, K, S) // 4
        assert (nws > 0) == (S > 1)
        gws = guarded((max(nws, 1),), torch.float32, "cuda")
        ops.wgrad(dys, xs, M, N, K, odt, split, ld_dy=N + 8, ld_x=K + 24, dw=gw.view, db=gb.view, ws=gws.view if nws else None)
        for g, what in ((gw, "dw"), (gb, "db"), (gws, "workspace")):
            g.assert_untouched(what)
        gw.assert_fully_written("dw")
        gb.assert_fully_written("db")
        if nws:
            gws.assert_fully_written("workspace")
        else:
            assert not bool(gws.written_mask().any())
        dw, db = gw.view.clone(), gb.view.reshape(N).clone()
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
        if odt == torch.float32:
            check_bound_a(dw, db, M, S, ref_w, ref_b, abs_w, abs_b, f"guarded M={M} split={split}")
    # no bias requested: db is not touched, in either path
    gb = guarded((N,), torch.float32, "cuda")
    _lib_call = ops._lib.load().bg_linear_wgrad
    nbytes = ops.workspace_bytes(M, N, K, S)
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device="cuda")
    dw = torch.empty(N, K, dtype=torch.float32, device="cuda")
    ops._lib.check(_lib_call(dys.data_ptr(), N + 8, xs.data_ptr(), K + 24, dw.data_ptr(), None, M, N, K, ops.DT[dtype], ops.DT[torch.float32], split,
                             ws.data_ptr() if nbytes else None, nbytes, ops._stream()), "bg_linear_wgrad")
    gb.assert_untouched("db (NULL)")
    assert bool(((dw.double() - ref_w).abs() <= (M + S + 2) * ops.U24 * abs_w).all())


def test_wgrad_zero_rows_write_zeros():
    gw, gb = guarded((128, 128), torch.float32, "cuda"), guarded((128,), torch.float32, "cuda")
    ops.wgrad(torch.empty(0, 128, dtype=torch.float16, device="cuda"), torch.empty(0, 128, dtype=torch.float16, device="cuda"), 0, 128, 128,
              torch.float32, 0, dw=gw.view, db=gb.view)
    gw.assert_untouched("dw"), gb.assert_untouched("db")
    assert not bool(gw.view.any()) and not bool(gb.view.any())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("src_dtype", ("fp32", "same"))
@pytest.mark.parametrize("R, C", [(64, 64), (768, 1024), (2304, 768)])
def test_weight_cast_guarded(R, C, src_dtype, dtype):
    g = torch.Generator(device="cpu").manual_seed(R + C)
    src = torch.randn(R, C, generator=g).cuda()
    if src_dtype == "same":
        src = src.to(dtype)
    src = strided_input(src, C)                                             # dense, NaN guard bands before and behind
    want = src.to(dtype)
    for dst, dst_t in ((True, True), (True, False), (False, True)):
        go, gt = guarded((R, C), dtype, "cuda"), guarded((C, R), dtype, "cuda")
        ops.weight_cast(src, dtype, dst, dst_t, out=go.view, out_t=gt.view)
        go.assert_untouched("dst"), gt.assert_untouched("dst_t")
        if dst:
            go.assert_fully_written("dst")
            assert torch.equal(go.view.view(torch.int16), want.view(torch.int16))
        else:
            assert not bool(go.written_mask().any())
        if dst_t:
            gt.assert_fully_written("dst_t")
            assert torch.equal(gt.view.view(torch.int16), want.t().contiguous().view(torch.int16))
        else:
            assert not bool(gt.written_mask().any())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("split", (1, 3))
def test_wgrad_overflow_marks_its_row_only(split, dtype):
    M, N, K = 200, 256, 128
    dy, x = (t.clone() for t in case(M, N, K, dtype)[:2])
    m0, n0 = 131, 200
    dy[m0, n0] = float("inf")
    for odt in (torch.float32, dtype):
        dw, db = ops.wgrad(dy, x, M, N, K, odt, split)
        fin_w, fin_b = torch.isfinite(dw), torch.isfinite(db)
        assert not bool(fin_w[n0].any()) and not bool(fin_b[n0])
        others = torch.arange(N, device="cuda") != n0
        assert bool(fin_w[others].all()) and bool(fin_b[others].all())


# ---- the autograd op ----

def _linear_case(shape, N, dtype, bias=True, seed=0):
    """x, W, b, dy: standard-normal draws ROUNDED to dtype (the fp32 parameters hold rounded values: autocast's cast is exact, and the
    fp64 reference sees exactly what both implementations see)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    K = shape[-1]
    x = torch.randn(*shape, generator=g).to(dtype).cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype).float().cuda()
    b = torch.randn(N, generator=g).to(dtype).float().cuda() if bias else None
    dy = torch.randn(*shape[:-1], N, generator=g).to(dtype).cuda()
    return x, w, b, dy


def _run(fn, x, w, b, dy, dtype, grads=(True, True, True), autocast=True):
    x = x.detach().clone().requires_grad_(grads[0])
    w = w.detach().clone().requires_grad_(grads[1])
    b = None if b is None else b.detach().clone().requires_grad_(grads[2])
    with torch.autocast("cuda", dtype=dtype, enabled=autocast):
        y = fn(x, w, b)
    y.backward(dy.to(y.dtype))
    return y.detach(), x.grad, w.grad, (None if b is None else b.grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
@pytest.mark.parametrize("shape, N", [((3, 5, 768), 1024), ((2, 33, 1024), 768)])
def test_linear_autograd_against_fp64(shape, N, dtype):
    x, w, b, dy = _linear_case(shape, N, dtype)
    ref = _run(F.linear, x.double(), w.double(), b.double(), dy.double(), dtype, autocast=False)
    ours = _run(L.linear, x, w, b, dy, dtype)
    tors = _run(F.linear, x, w, b, dy, dtype)
    assert ours[0].dtype == dtype and ours[1].dtype == dtype and ours[2].dtype == torch.float32 and ours[3].dtype == torch.float32
    tag = f"linear {tuple(shape)}->{N} {NAME[dtype]}"
    for what, o, t, r in zip(("y", "dx", "dw", "db"), ours, tors, ref):
        assert o.shape == r.shape
        within_2x(tag, what, errs(o, r), errs(t, r))
    # needs_input_grad: frozen weight, no bias, x without grad -- what is computed equals the full run bit for bit
    y, dx, dw, db = _run(L.linear, x, w, b, dy, dtype, grads=(True, False, True))
    assert dw is None and torch.equal(dx, ours[1]) and torch.equal(db, ours[3]) and torch.equal(y, ours[0])
    y, dx, dw, db = _run(L.linear, x, w, b, dy, dtype, grads=(False, True, True))
    assert dx is None and torch.equal(dw, ours[2]) and torch.equal(db, ours[3])
    y, dx, dw, db = _run(L.linear, x, w, None, dy, dtype)
    assert db is None and torch.equal(dw, ours[2]) and torch.equal(dx, ours[1])
    refn = _run(F.linear, x.double(), w.double(), None, dy.double(), dtype, autocast=False)
    within_2x(tag + " no bias", "y", errs(y, refn[0]), errs(_run(F.linear, x, w, None, dy, dtype)[0], refn[0]))
    # 16-bit parameters outside autocast: gradients in the parameters' dtype
    y, dx, dw, db = _run(L.linear, x, w.to(dtype), b.to(dtype), dy, dtype, autocast=False)
    assert dw.dtype == dtype and db.dtype == dtype and torch.equal(y, ours[0]) and torch.equal(dx, ours[1])
    # DeviceLinear casts an fp32 input as autocast would, and raises outside autocast
    m = L.DeviceLinear(shape[-1], N).cuda()
    with torch.no_grad():
        m.weight.copy_(w), m.bias.copy_(b)
    with torch.autocast("cuda", dtype=dtype):
        assert torch.equal(m(x.float()), ours[0])
    with pytest.raises(ValueError):
        m(x.float())


# ---- in the encoder layer ----

@pytest.mark.parametrize("with_attention", (False, True), ids=("torch_attention", "device_attention"))
@pytest.mark.parametrize("N", (5, 33))
def test_linear_in_the_encoder_layer(N, with_attention):
    B, scale = 3, 2.0 ** 10
    torch.manual_seed(N)
    base = nn.TransformerEncoder(nn.TransformerEncoderLayer(768, 12, 1024, dropout=0.0, norm_first=True), 1, enable_nested_tensor=False).cuda().train()
    x = torch.randn(N, B, 768, device="cuda")
    g = torch.randn(N, B, 768, device="cuda", dtype=torch.float64) / (N * B)
    mask = torch.zeros(B, N, dtype=torch.bool, device="cuda")
    for b in range(B):
        mask[b, max(1, (N * (b + 2)) // (B + 2)):] = True                    # ragged: another length per sample
    g = g * (~mask).t().unsqueeze(-1)                                       # padded tokens carry no loss, as in the trainers
    ref = encoder_grads(copy.deepcopy(base).double(), x, mask, g, 1.0, None)[1]
    plain = encoder_grads(copy.deepcopy(base), x, mask, g, scale, torch.float16)[1]
    enc = copy.deepcopy(base)
    if with_attention:
        bga.use_device_attention(enc)
    assert L.use_device_linear(enc) is enc
    ours = encoder_grads(enc, x, mask, g, scale, torch.float16)[1]
    assert list(ours) == list(ref)
    for k in ref:
        assert enc.get_parameter(k).grad.dtype == torch.float32
        within_2x(f"layer N={N} {'device' if with_attention else 'torch'} attention", k, errs(ours[k], ref[k]), errs(plain[k], ref[k]))
    # one AdamW step on the converted encoder changes the Parameter objects the next forward reads
    params = list(enc.parameters())
    assert any(p is enc.layers[0].linear1.weight for p in params) and any(p is enc.layers[0].self_attn.out_proj.weight for p in params)
    with torch.autocast("cuda", dtype=torch.float16), torch.no_grad():
        y0 = enc(x, src_key_padding_mask=mask).clone()
    before = [p.detach().clone() for p in params]
    bga.optim.AdamW(params, lr=1e-2).step()
    assert all(not torch.equal(a, p) for a, p in zip(before, params))
    with torch.autocast("cuda", dtype=torch.float16), torch.no_grad():
        y1 = enc(x, src_key_padding_mask=mask)
    assert not torch.equal(y0, y1)
