"""The glue of an encoder layer on the device (csrc/layer_train.hip, brepgen_amd/layer.py) against fp64 evaluated from the same rounded
inputs.

(a) The project's yardstick: absolute errors pooled over M in {1, 3, 4, 5, 63, 64, 65, 129, 257, 1000} per (x dtype -> y dtype) pair, max
    and mean <= 2 x torch's on the same GPU from the same inputs.  Torch's side is torch.native_layer_norm in fp32 (its output rounded to
    y's dtype, as autocast's cast does) and its autograd.  Forward rows include fp32 x = 100 + 0.1 N(0, 1) / 16-bit x = 8 + N(0, 1)
    (|mean| >> std) and a constant row (var = 0).
(b) dgamma / dbeta: the bound derived in tests/layer_restate.py from the summation order the kernels have,
        |dbeta - ref| <= (R + 3) 2^-24 sum_m |dy|,    |dgamma - ref| <= (R + 3) 2^-24 sum_m |dy| |xhat| + sum_m |dy| E[m, c],
    R = rows per fp32 chain (4 at these M; <= 64 always), E = the bound of the kernel's xhat against the reference's.  tests/
    test_layer_train_cpu.py holds the restated kernel order to HALF of it against torch's fp64 autograd.  The torch pair is recorded, not
    asserted: a row walk in short chains and torch's tree reduction grow their errors differently (tests/test_gpu_linear_bwd.py, db).
(c) bits: the elementwise ops and the mask equal their restatement bit for bit; every entry gives the same bits twice.

BG_LAYER_PARITY_JSON=<path> makes the run write the measured pairs there (profiles/r15/layer_train_parity.json is such a run)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import brepgen_amd as bga
from brepgen_amd import layer as L
from tests import attn_train_ops as aops
from tests import layer_ops as ops
from tests import layer_restate as R
from tests.guarded import guarded, strided_input
from tests.train_check import Parity, bits, encoder, encoder_grads, errs, pooled, same_bits

pytestmark = pytest.mark.gpu
NAME = ops.NAME
MS = (1, 3, 4, 5, 63, 64, 65, 129, 257, 1000)
EPS = float(np.float32(1e-5))          # what the kernels and torch's fp32 LayerNorm both use
PAIR_IDS = [f"{NAME[a]}-{NAME[b]}" for a, b in ops.LN_PAIRS]
FIRSTS = (0, 2 ** 33 + 3)


PARITY = Parity("BG_LAYER_PARITY_JSON", "absolute error against fp64 from the same rounded inputs; LayerNorm pairs are pooled over M in "
                f"{list(MS)}; torch = torch.native_layer_norm in fp32 and its autograd, or stock autocast for the encoder")
record, within_2x, _parity_json = PARITY.record, PARITY.within_2x, PARITY.fixture()


@functools.lru_cache(maxsize=None)
def affine():
    g = torch.Generator(device="cpu").manual_seed(768)
    return (1.0 + 0.1 * torch.randn(768, generator=g)).cuda(), (0.1 * torch.randn(768, generator=g)).cuda()


@functools.lru_cache(maxsize=None)
def ln_case(M, xdt, ydt, hostile):
    """x (rounded to xdt), dy (ydt), dskip (xdt) and the fp64 reference of forward and backward -- computed once, shared, never modified"""
    g = torch.Generator(device="cpu").manual_seed(100 * M + 7 * ops.DT[xdt] + ops.DT[ydt])
    x = 0.5 + 1.5 * torch.randn(M, 768, generator=g)
    if hostile and M >= 3:
        x[1] = (100.0 + 0.1 * torch.randn(768, generator=g)) if xdt == torch.float32 else (8.0 + torch.randn(768, generator=g))
        x[2] = 3.0
    x = x.to(xdt).cuda()
    dy = torch.randn(M, 768, generator=g).to(ydt).cuda()
    dskip = torch.randn(M, 768, generator=g).to(xdt).cuda()
    gamma, beta = affine()
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mean = xd.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(1, keepdim=True) + EPS)
    y = (xd - mean) * rstd * gd + bd
    y.backward(dy.double())
    ref = dict(y=y.detach(), mean=mean.detach().reshape(M), rstd=rstd.detach().reshape(M), dx=xd.grad, dx_skip=xd.grad + dskip.double(),
               dgamma=gd.grad, dbeta=bd.grad)
    # torch: fp32 LayerNorm and its autograd from the same rounded values
    xt = x.float().clone().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yt, mt, rt = torch.native_layer_norm(xt, (768,), gt, bt, 1e-5)
    yt.backward(dy.float())
    tor = dict(y=yt.detach().to(ydt), mean=mt.detach().reshape(M), rstd=rt.detach().reshape(M), dx=xt.grad.to(xdt),
               dx_skip=(xt.grad + dskip.float()).to(xdt), dgamma=gt.grad, dbeta=bt.grad)
    return x, dy, dskip, ref, tor


# ---- LayerNorm ----

@pytest.mark.parametrize("xdt, ydt", ops.LN_PAIRS, ids=PAIR_IDS)
def test_ln_forward_within_twice_torch(xdt, ydt):
    gamma, beta = affine()
    mine, theirs = {k: [] for k in ("y", "mean", "rstd")}, {k: [] for k in ("y", "mean", "rstd")}
    for M in MS:
        x, _, _, ref, tor = ln_case(M, xdt, ydt, True)
        y, stats = ops.ln_fwd(x, gamma, beta, ydt)
        assert y.dtype == ydt and bool(torch.isfinite(y).all()) and bool(torch.isfinite(stats).all())
        got = dict(y=y, mean=stats[:, 0], rstd=stats[:, 1])
        for k in mine:
            mine[k].append((got[k].double() - ref[k]).abs())
            theirs[k].append((tor[k].double() - ref[k]).abs())
        if M >= 3:                                                  # the constant row: var = 0 exactly, y = beta rounded
            assert same_bits(y[2], beta.to(ydt))
    for k in mine:
        within_2x(f"ln_fwd {NAME[xdt]}->{NAME[ydt]}", k, pooled(mine[k]), pooled(theirs[k]))


@pytest.mark.parametrize("xdt, ydt", ops.LN_PAIRS, ids=PAIR_IDS)
def test_ln_backward_within_twice_torch_and_the_derived_bound(xdt, ydt):
    gamma, beta = affine()
    mine, theirs = {k: [] for k in ("dx", "dx_skip")}, {k: [] for k in ("dx", "dx_skip")}
    for M in MS:
        x, dy, dskip, ref, tor = ln_case(M, xdt, ydt, False)
        _, stats = ops.ln_fwd(x, gamma, beta, ydt)
        dx, dg, db = ops.ln_bwd(dy, x, stats, gamma)
        dxs, dg2, db2 = ops.ln_bwd(dy, x, stats, gamma, dskip)
        dxn, none_g, none_b = ops.ln_bwd(dy, x, stats, gamma, grads=False)
        assert dx.dtype == xdt and none_g is None and none_b is None
        assert same_bits(dxn, dx) and same_bits(dg2, dg) and same_bits(db2, db)       # dx does not depend on whether the sums are asked for
        for k, got in (("dx", dx), ("dx_skip", dxs)):
            assert bool(torch.isfinite(got).all())
            mine[k].append((got.double() - ref[k]).abs())
            theirs[k].append((tor[k].double() - ref[k]).abs())
        bg, bb = R.dgamma_dbeta_bounds(dy, x, M, EPS)
        eg, eb = (dg.double() - ref["dgamma"]).abs(), (db.double() - ref["dbeta"]).abs()
        tag = f"ln_bwd M={M} {NAME[xdt]}->{NAME[ydt]}"
        print(f"{tag}: bound (b) used to {float((eg / bg.clamp_min(1e-300)).max()):.3f} (dgamma), {float((eb / bb.clamp_min(1e-300)).max()):.3f} (dbeta)")
        record(tag, "dgamma", errs(dg, ref["dgamma"]), errs(tor["dgamma"], ref["dgamma"]))
        record(tag, "dbeta", errs(db, ref["dbeta"]), errs(tor["dbeta"], ref["dbeta"]))
        assert bool(torch.isfinite(dg).all()) and bool(torch.isfinite(db).all())
        assert bool((eg <= bg).all()), (tag, "dgamma")
        assert bool((eb <= bb).all()), (tag, "dbeta")
    for k in mine:
        within_2x(f"ln_bwd {NAME[xdt]}->{NAME[ydt]}", k, pooled(mine[k]), pooled(theirs[k]))


@pytest.mark.parametrize("xdt, ydt", ops.LN_PAIRS, ids=PAIR_IDS)
def test_ln_bits(xdt, ydt):
    gamma, beta = affine()
    for M in (5, 257):
        x, dy, dskip, _, _ = ln_case(M, xdt, ydt, False)
        y, stats = ops.ln_fwd(x, gamma, beta, ydt)
        y2, stats2 = ops.ln_fwd(x, gamma, beta, ydt)
        assert same_bits(y, y2) and same_bits(stats, stats2)                            # two calls, identical bits
        a, b = ops.ln_bwd(dy, x, stats, gamma, dskip), ops.ln_bwd(dy, x, stats, gamma, dskip)
        assert all(same_bits(p, q) for p, q in zip(a, b))
        # dskip = 0 and no dskip
        assert same_bits(ops.ln_bwd(dy, x, stats, gamma, torch.zeros_like(dskip))[0], ops.ln_bwd(dy, x, stats, gamma)[0])
        # a row of y / dx depends on its own row alone
        r0 = M // 2
        others = torch.arange(M, device="cuda") != r0
        xp, dyp = x.clone(), dy.clone()
        xp[r0] = xp[r0].flip(0)                                    # (LayerNorm undoes an affine change of a row)
        dyp[r0] = (dyp[r0].float() * 0.5 + 1.0).to(ydt)
        yp, statsp = ops.ln_fwd(xp, gamma, beta, ydt)
        assert same_bits(yp[others], y[others]) and same_bits(statsp[others], stats[others]) and not same_bits(yp[r0], y[r0])
        dxp = ops.ln_bwd(dyp, x, stats, gamma, dskip)[0]
        assert same_bits(dxp[others], a[0][others]) and not same_bits(dxp[r0], a[0][r0])
        # a column of dgamma / dbeta depends on its own column alone
        c0 = 77
        cols = torch.arange(768, device="cuda") != c0
        dyc = dy.clone()
        dyc[:, c0] = (dyc[:, c0].float() * 0.5 + 1.0).to(ydt)
        _, dgc, dbc = ops.ln_bwd(dyc, x, stats, gamma, dskip)
        assert same_bits(dgc[cols], a[1][cols]) and same_bits(dbc[cols], a[2][cols])
        assert not same_bits(dgc[c0], a[1][c0]) and not same_bits(dbc[c0], a[2][c0])


def test_ln_bwd_zero_rows_write_zeros():
    gamma, _ = affine()
    gg, gb = guarded((768,), torch.float32, "cuda"), guarded((768,), torch.float32, "cuda")
    e16 = torch.empty(0, 768, dtype=torch.float16, device="cuda")
    ops.ln_bwd(e16, e16, torch.empty(0, 2, device="cuda"), gamma, dgamma=gg.view, dbeta=gb.view)
    gg.assert_untouched("dgamma"), gb.assert_untouched("dbeta")
    assert not bool(gg.view.any()) and not bool(gb.view.any())
    assert ops.workspace_bytes(0) == 0


@pytest.mark.parametrize("xdt, ydt", ops.LN_PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("M", (1, 5, 65, 257))
def test_ln_guarded(M, xdt, ydt):
    """NaN guard bands around every input (a read before the first or past the last row makes a result NaN); every output and the
    workspace: all promised elements written, nothing outside -- the workspace is exactly bg_ln_bwd_workspace_bytes long"""
    gamma, beta = affine()
    x, dy, dskip, ref, _ = ln_case(M, xdt, ydt, False)
    xs, dys, sks = strided_input(x, 768), strided_input(dy, 768), strided_input(dskip, 768)
    gs, bs = strided_input(gamma[None], 768).reshape(768), strided_input(beta[None], 768).reshape(768)
    gy, gst = guarded((M, 768), ydt, "cuda"), guarded((M, 2), torch.float32, "cuda")
    ops.ln_fwd(xs, gs, bs, ydt, y=gy.view, stats=gst.view)
    for g, what in ((gy, "y"), (gst, "stats")):
        g.assert_untouched(what), g.assert_fully_written(what)
    assert bool(torch.isfinite(gy.view).all()) and bool(torch.isfinite(gst.view).all())
    stats = strided_input(gst.view.clone(), 2)
    nbytes = ops.workspace_bytes(M)
    assert nbytes == ops.workspace_formula(M) > 0
    for sk in (None, sks):
        gdx, gdg, gdb = guarded((M, 768), xdt, "cuda"), guarded((768,), torch.float32, "cuda"), guarded((768,), torch.float32, "cuda")
        gws = guarded((nbytes // 8,), torch.float64, "cuda")
        ops.ln_bwd(dys, xs, stats, gs, sk, dx=gdx.view, dgamma=gdg.view, dbeta=gdb.view, ws=gws.view)
        for g, what in ((gdx, "dx"), (gdg, "dgamma"), (gdb, "dbeta"), (gws, "workspace")):
            g.assert_untouched(what), g.assert_fully_written(what)
        assert all(bool(torch.isfinite(g.view).all()) for g in (gdx, gdg, gdb, gws))
        bg, bb = R.dgamma_dbeta_bounds(dy, x, M, EPS)
        assert bool(((gdg.view.reshape(768).double() - ref["dgamma"]).abs() <= bg).all())
        assert bool(((gdb.view.reshape(768).double() - ref["dbeta"]).abs() <= bb).all())
    # dgamma / dbeta NULL: neither they nor a workspace are touched
    gdx, gdg, gws = guarded((M, 768), xdt, "cuda"), guarded((768,), torch.float32, "cuda"), guarded((nbytes // 8,), torch.float64, "cuda")
    ops._lib.check(ops._lib.load().bg_ln_bwd(dys.data_ptr(), ops.DT[ydt], xs.data_ptr(), ops.DT[xdt], stats.data_ptr(), gs.data_ptr(), None,
                                             gdx.view.data_ptr(), None, None, M, gws.view.data_ptr(), nbytes, ops._stream()), "bg_ln_bwd")
    gdx.assert_untouched("dx"), gdx.assert_fully_written("dx"), gdg.assert_untouched("dgamma"), gws.assert_untouched("workspace")
    assert not bool(gws.written_mask().any())


@pytest.mark.parametrize("xdt, ydt", ops.LN_PAIRS, ids=PAIR_IDS)
def test_an_inf_in_dy_reaches_its_row_and_its_column_only(xdt, ydt):
    gamma, beta = affine()
    M, m0, c0 = 129, 70, 300
    x, dy, dskip, _, _ = ln_case(M, xdt, ydt, False)
    dy = dy.clone()
    dy[m0, c0] = float("inf")
    _, stats = ops.ln_fwd(x, gamma, beta, ydt)
    dx, dg, db = ops.ln_bwd(dy, x, stats, gamma, dskip)
    rows, cols = torch.arange(M, device="cuda") != m0, torch.arange(768, device="cuda") != c0
    assert not bool(torch.isfinite(dx[m0]).any()) and bool(torch.isfinite(dx[rows]).all())
    assert not bool(torch.isfinite(dg[c0])) and not bool(torch.isfinite(db[c0]))
    assert bool(torch.isfinite(dg[cols]).all()) and bool(torch.isfinite(db[cols]).all())


def test_a_grad_scaler_sees_the_inf_through_dgamma():
    w, b = (t.clone().requires_grad_(True) for t in affine())
    x = torch.randn(7, 3, 768, device="cuda", requires_grad=True)
    with torch.autocast("cuda", torch.float16):
        y = L.layer_norm(x, w, b)
    assert y.dtype == torch.float16
    dy = torch.ones_like(y)
    dy[2, 1, 5] = float("inf")
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    opt = torch.optim.SGD([w, b], lr=0.1)
    scaler.scale(torch.zeros((), device="cuda"))                 # (initialises the scaler's device state)
    y.backward(dy)
    assert w.grad.dtype == torch.float32 and b.grad.dtype == torch.float32 and x.grad.dtype == torch.float32
    before = w.detach().clone()
    scaler.step(opt)                                              # unscales, finds the inf, skips the step
    scaler.update()
    assert torch.equal(w.detach(), before) and scaler.get_scale() == 512.0
    assert bool(torch.isfinite(x.grad[torch.arange(7, device="cuda") != 2]).all())


# ---- the mask and the elementwise ops ----

@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("p", (0.1, 0.5))
@pytest.mark.parametrize("M, C, B", [(1, 768, 1), (15, 768, 3), (99, 1024, 3)])
def test_mask_equals_the_restatement(M, C, B, p, first):
    seen = []
    for site in range(4):
        got = ops.dropout_mask(M, C, B, p, 77, 5, site, first)
        want = R.keep_mask(M, C, B, p, 77, 5, site, first)
        assert np.array_equal(got.cpu().numpy(), want), site
        assert same_bits(got, ops.dropout_mask(M, C, B, p, 77, 5, site, first))
        seen.append(want)
    assert all(not np.array_equal(seen[i], seen[j]) for i in range(4) for j in range(i))
    # a rank that owns samples [lo, hi) reproduces its rows of the single-GPU mask
    if B == 3:
        full = seen[1].reshape(M // B, B, C)
        part = ops.dropout_mask(M // B * 2, C, 2, p, 77, 5, 1, first + 1).cpu().numpy().reshape(M // B, 2, C)
        assert np.array_equal(part, full[:, 1:3])


def _elementwise_case(M, C, dtype, sdt, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    branch = torch.randn(M, C, generator=g).to(dtype).cuda()
    skip = torch.randn(M, C, generator=g).to(sdt).cuda()
    dout = torch.randn(M, C, generator=g).to(sdt).cuda()
    return branch, skip, dout


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("p", (0.1, 0.5))
@pytest.mark.parametrize("stream", ("fp32_stream", "16bit_stream"))
@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), ids=lambda d: NAME[d])
@pytest.mark.parametrize("M, C, B", [(15, 768, 3), (99, 1024, 3)])
def test_elementwise_ops_equal_their_fp32_expressions(M, C, B, dtype, stream, p, first):
    sdt = torch.float32 if stream == "fp32_stream" else dtype
    branch, skip, dout = _elementwise_case(M, C, dtype, sdt, M + C)
    rp = R.rp_of(p)
    for site in (1, 3):
        keep = torch.from_numpy(R.keep_mask(M, C, B, p, 77, 5, site, first)).cuda().bool()
        out = ops.dropout_add_fwd(branch, skip, B, p, 77, 5, site, first)
        assert same_bits(out, R.dropout_add(branch, skip, keep, rp))
        assert torch.equal(bits(out)[~keep], bits(skip)[~keep])                       # dropped elements: skip's bits
        assert same_bits(out, ops.dropout_add_fwd(branch, skip, B, p, 77, 5, site, first))
        assert same_bits(ops.dropout_bwd(dout, dtype, B, p, 77, 5, site, first), R.dropout_bwd(dout, keep, rp, dtype))
    keep = torch.from_numpy(R.keep_mask(M, C, B, p, 77, 5, 2, first)).cuda().bool()
    h = ops.relu_dropout_fwd(branch, B, p, 77, 5, 2, first)
    assert same_bits(h, R.relu_dropout(branch, keep, rp)) and not bool((h < 0).any())
    assert bool(((h > 0) == (keep & (branch > 0))).all())                             # h > 0 marks exactly what passes
    dh = dout.to(dtype)
    assert same_bits(ops.relu_dropout_bwd(h, dh, p), R.relu_dropout_bwd(h, dh, rp))
    # p = 0: no mask, plain add / relu
    assert same_bits(ops.dropout_add_fwd(branch, skip, B, 0.0, 77, 5, 1, first), (skip.float() + branch.float()).to(sdt))
    assert same_bits(ops.dropout_bwd(dout, dtype, B, 0.0, 77, 5, 1, first), dout.to(dtype))
    assert same_bits(ops.relu_dropout_fwd(branch, B, 0.0, 77, 5, 2, first), torch.relu(branch))


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), ids=lambda d: NAME[d])
def test_relu_dropout_non_finite_inputs(dtype):
    M, C, B, p = 15, 1024, 3, 0.5
    keep = torch.from_numpy(R.keep_mask(M, C, B, p, 77, 5, 2, 0)).cuda().bool()
    x = _elementwise_case(M, C, dtype, dtype, 3)[0]
    x[::2] = float("nan")
    x[1, :100] = float("inf")
    x[1, 100:200] = float("-inf")
    h = ops.relu_dropout_fwd(x, B, p, 77, 5, 2, 0)
    nan = torch.isnan(x)
    assert bool((torch.isnan(h) == (nan & keep)).all())                               # a kept NaN propagates, a dropped one is 0
    assert not bool(h[~keep].any())
    assert bool((h[1, :100][keep[1, :100]] == float("inf")).all()) and not bool(h[1, 100:200].any())


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), ids=lambda d: NAME[d])
def test_python_ops_and_their_autograd(dtype):
    N, B, p, first = 5, 3, 0.1, 2 ** 33 + 3
    branch, skip, dout = (t.view(N, B, 768) for t in _elementwise_case(N * B, 768, dtype, torch.float32, 11))
    b_, s_ = branch.clone().requires_grad_(True), skip.clone().requires_grad_(True)
    out = L.dropout_add(b_, s_, p, True, seed=77, draw_id=5, site=3, first_sample=first)
    assert same_bits(out.detach().view(-1, 768), ops.dropout_add_fwd(branch.view(-1, 768), skip.view(-1, 768), B, p, 77, 5, 3, first))
    out.backward(dout)
    assert same_bits(s_.grad, dout) and same_bits(b_.grad.view(-1, 768), ops.dropout_bwd(dout.view(-1, 768), dtype, B, p, 77, 5, 3, first))
    # training=False or p = 0: no mask
    plain = (skip.float() + branch.float())
    assert same_bits(L.dropout_add(branch, skip, p, False), plain) and same_bits(L.dropout_add(branch, skip, 0.0, True), plain)
    x = _elementwise_case(N * B, 1024, dtype, dtype, 12)[0].view(N, B, 1024)
    assert same_bits(L.relu_dropout(x, p, False), torch.relu(x))
    x_ = x.clone().requires_grad_(True)
    h = L.relu_dropout(x_, p, True, seed=77, draw_id=5, first_sample=first)
    assert same_bits(h.detach().view(-1, 1024), ops.relu_dropout_fwd(x.view(-1, 1024), B, p, 77, 5, 2, first))
    dh = torch.randn(N, B, 1024, device="cuda").to(dtype)
    h.backward(dh)
    assert same_bits(x_.grad.view(-1, 1024), ops.relu_dropout_bwd(h.detach().view(-1, 1024), dh.view(-1, 1024), p))
    # layer_norm: an unused output arrives as None; the skip gradient is merged in the backward's own pass
    w, b = (t.clone().requires_grad_(True) for t in affine())
    xs = skip.clone().requires_grad_(True)
    y, s = L.layer_norm(xs, w, b, out_dtype=dtype, return_skip=True)
    assert y.dtype == dtype and s.dtype == torch.float32 and same_bits(s.detach(), skip)
    (s * dout).sum().backward()
    assert same_bits(xs.grad, dout) and w.grad is None and b.grad is None
    xs.grad = None
    y, s = L.layer_norm(xs, w, b, out_dtype=dtype, return_skip=True)
    dy = torch.randn(N, B, 768, device="cuda").to(dtype)
    torch.autograd.backward([y, s], [dy, dout])
    _, stats = ops.ln_fwd(skip.view(-1, 768), w.detach(), b.detach(), dtype)
    dx, dg, db = ops.ln_bwd(dy.view(-1, 768), skip.view(-1, 768), stats, w.detach(), dout.view(-1, 768))
    assert same_bits(xs.grad.view(-1, 768), dx) and same_bits(w.grad, dg) and same_bits(b.grad, db)


@pytest.mark.parametrize("stream", ("fp32_stream", "16bit_stream"))
@pytest.mark.parametrize("M", (1, 5, 65, 257))
def test_elementwise_guarded(M, stream):
    dtype, C, p = torch.bfloat16, 768, 0.1
    B = 5 if M % 5 == 0 else 1
    sdt = torch.float32 if stream == "fp32_stream" else dtype
    branch, skip, dout = (strided_input(t, C) for t in _elementwise_case(M, C, dtype, sdt, M))
    outs = []
    g = guarded((M, C), sdt, "cuda")
    ops.dropout_add_fwd(branch, skip, B, p, 77, 5, 1, 0, out=g.view)
    outs.append((g, "out"))
    g = guarded((M, C), dtype, "cuda")
    ops.dropout_bwd(dout, dtype, B, p, 77, 5, 1, 0, dbranch=g.view)
    outs.append((g, "dbranch"))
    gh = guarded((M, C), dtype, "cuda")
    ops.relu_dropout_fwd(branch, B, p, 77, 5, 2, 0, h=gh.view)
    outs.append((gh, "h"))
    g = guarded((M, C), dtype, "cuda")
    ops.relu_dropout_bwd(strided_input(gh.view.clone(), C), branch, p, dx=g.view)
    outs.append((g, "dx"))
    for g, what in outs:
        g.assert_untouched(what), g.assert_fully_written(what)
        assert bool(torch.isfinite(g.view).all()), what
    gm = guarded((M, C), torch.uint8, "cuda")
    ops.dropout_mask(M, C, B, p, 77, 5, 1, 0, mask=gm.view)
    gm.assert_untouched("mask")
    assert bool((gm.view <= 1).all())                                                  # every element written (the sentinel is 0xA5)


# ---- in the encoder ----

def _inputs(N, B):
    x = torch.randn(N, B, 768, device="cuda")
    g = torch.randn(N, B, 768, device="cuda", dtype=torch.float64) / (N * B)
    mask = torch.zeros(B, N, dtype=torch.bool, device="cuda")
    for b in range(B):
        mask[b, max(1, (N * (b + 2)) // (B + 2)):] = True                    # ragged: another length per sample
    return x, g * (~mask).t().unsqueeze(-1), mask                           # padded tokens carry no loss, as in the trainers


@pytest.mark.parametrize("stream", ("fp32_stream", "fp16_stream"))
@pytest.mark.parametrize("N", (5, 33))
def test_layer_in_the_encoder_without_dropout(N, stream):
    B, scale = 3, 2.0 ** 10
    base = encoder(0.0, N, jitter_norms=True)
    x, g, mask = _inputs(N, B)
    if stream == "fp16_stream":
        x = x.half()
    _, ref = encoder_grads(copy.deepcopy(base).double(), x, mask, g, 1.0, None)
    _, plain = encoder_grads(copy.deepcopy(base), x, mask, g, scale, torch.float16)
    enc = copy.deepcopy(base)
    assert L.use_device_layer(enc) is enc
    assert all(isinstance(l, L.DeviceEncoderLayer) for l in enc.layers) and isinstance(enc.norm, L.DeviceLayerNorm)
    out, ours = encoder_grads(enc, x, mask, g, scale, torch.float16)
    assert list(ours) == list(ref) and out.dtype == torch.float32
    for k in ref:
        assert enc.get_parameter(k).grad.dtype == torch.float32
        within_2x(f"encoder N={N} {stream} no dropout", k, errs(ours[k], ref[k]), errs(plain[k], ref[k]))
    if stream == "fp16_stream":
        return
    # one AdamW step on the converted encoder changes the Parameter objects the next forward reads
    params = list(enc.parameters())
    assert any(p is enc.layers[0].norm1.weight for p in params) and any(p is enc.norm.weight for p in params)
    with torch.autocast("cuda", dtype=torch.float16), torch.no_grad():
        y0 = enc(x, src_key_padding_mask=mask).clone()
    before = [p.detach().clone() for p in params]
    bga.optim.AdamW(params, lr=1e-2).step()
    assert all(not torch.equal(a, p) for a, p in zip(before, params))
    with torch.autocast("cuda", dtype=torch.float16), torch.no_grad():
        y1 = enc(x, src_key_padding_mask=mask)
    assert not torch.equal(y0, y1)


def _masked_model(P, x, key_pad, masks, rp):
    """the 2-layer pre-norm encoder + final norm in torch ops with EXPLICIT keep masks: P name -> tensor, masks[i] = (attn [B, 12, N, N],
    site 1, site 2, site 3 [N, B, C]) in P's dtype"""
    for i, (ka, k1, k2, k3) in enumerate(masks):
        pre = f"layers.{i}."
        y = F.layer_norm(x, (768,), P[pre + "norm1.weight"], P[pre + "norm1.bias"], 1e-5)
        qkv = F.linear(y, P[pre + "self_attn.in_proj_weight"], P[pre + "self_attn.in_proj_bias"]).transpose(0, 1)
        a = aops.torch_attention(qkv, key_pad, 0.125, ka, rp).transpose(0, 1)
        a = F.linear(a, P[pre + "self_attn.out_proj.weight"], P[pre + "self_attn.out_proj.bias"])
        x = x + a * (k1 * rp)
        y = F.layer_norm(x, (768,), P[pre + "norm2.weight"], P[pre + "norm2.bias"], 1e-5)
        h = torch.relu(F.linear(y, P[pre + "linear1.weight"], P[pre + "linear1.bias"])) * (k2 * rp)
        x = x + F.linear(h, P[pre + "linear2.weight"], P[pre + "linear2.bias"]) * (k3 * rp)
    return F.layer_norm(x, (768,), P["norm.weight"], P["norm.bias"], 1e-5)


def _masked_grads(base, x, key_pad, masks, rp, g, scale, dtype):
    wd = torch.float64 if dtype is None else torch.float32
    P = {k: p.detach().to(wd).clone().requires_grad_(True) for k, p in base.named_parameters()}
    mk = [tuple(m.to(wd) for m in ms) for ms in masks]
    if dtype is None:
        out = _masked_model(P, x.double(), key_pad, mk, rp)
    else:
        with torch.autocast("cuda", dtype=dtype):
            out = _masked_model(P, x, key_pad, mk, rp)
    ((out.double() * g).sum() * scale).backward()
    return {k: p.grad.double() / scale for k, p in P.items()}


def _reset_calls(enc, calls):
    for layer in enc.layers:
        layer.calls = layer.self_attn.calls = calls


@pytest.mark.parametrize("N", (5, 33))
def test_layer_in_the_encoder_with_dropout(N):
    B, scale, p, seed = 3, 2.0 ** 10, 0.1, 77
    base0 = encoder(0.0, N, jitter_norms=True)
    base = encoder(p, N, jitter_norms=True)
    base.load_state_dict(base0.state_dict())
    x, g, mask = _inputs(N, B)
    enc = L.use_device_layer(copy.deepcopy(base), seed=seed)
    out, ours = encoder_grads(enc, x, mask, g, scale, torch.float16)
    assert all(l.calls == 1 and l.self_attn.calls == 1 for l in enc.layers)
    # the masks of that step: layer i drew draw_id = 0 * 2 + i, in its attention module and in its three dropouts
    masks = []
    for i in range(2):
        ka = aops.dropout_mask(B, N, p, seed, i)
        ks = [ops.dropout_mask(N * B, C, B, p, seed, i, site).view(N, B, C) for site, C in ((1, 768), (2, 1024), (3, 768))]
        masks.append((ka, *ks))
    rp = R.rp_of(p)
    ref = _masked_grads(base, x, mask, masks, rp, g, 1.0, None)
    plain = _masked_grads(base, x, mask, masks, rp, g, scale, torch.float16)
    assert list(ours) == list(ref)
    for k in ref:
        assert enc.get_parameter(k).grad.dtype == torch.float32
        within_2x(f"encoder N={N} dropout {p}", k, errs(ours[k], ref[k]), errs(plain[k], ref[k]))
    # resetting the call counters replays the step bit for bit; another counter value draws other masks
    _reset_calls(enc, 0)
    out2, again = encoder_grads(enc, x, mask, g, scale, torch.float16)
    assert same_bits(out2, out) and all(torch.equal(again[k], ours[k]) for k in ours)
    _reset_calls(enc, 5)
    out3, _ = encoder_grads(enc, x, mask, g, scale, torch.float16)
    assert not same_bits(out3, out)
    # eval(): no mask -- the bits of an encoder built with dropout = 0
    enc0 = L.use_device_layer(copy.deepcopy(base0))
    with torch.autocast("cuda", dtype=torch.float16), torch.no_grad():
        assert same_bits(enc.eval()(x, src_key_padding_mask=mask), enc0(x, src_key_padding_mask=mask))
        assert same_bits(enc(x, src_key_padding_mask=mask), enc0.eval()(x, src_key_padding_mask=mask))
