"""The denoisers' MLPs and masked-MSE gradient on the device (csrc/mlp_train.hip, brepgen_amd/mlp.py, training.mse_loss).

(a) bits: the three thin products (their order of operations is stated in include/brepgen_hip.h, fused multiply-adds included), the
    column sums of bg_thin_wgrad and bg_masked_mse_bwd equal tests/mlp_restate.py bit for bit; every entry gives the same bits twice;
    outputs and workspaces sit in guard bands (tests/guarded.py), strided inputs carry NaN in the columns that must not be read.
(b) the project's yardstick: absolute errors against fp64 evaluated from the same rounded inputs, pooled over the row counts of a case,
    max and mean <= 2 x stock torch's on the same GPU -- torch under the same autocast dtype for 16-bit outputs, in fp32 for fp32 outputs.
(c) modules: DeviceMLP against the nn.Sequential it adopted, and two whole reference-keyed denoisers after training.use_device_training
    with training.mse_loss against the stock model with loss_fn(pred[~mask], noise[~mask]), every parameter's gradient.

Row counts follow the kernels' plans: bg_thin_expand 64-row tiles (8 slots x 8), bg_thin_contract 64-row tiles (32 half-waves x 2 rows),
bg_thin_wgrad chains of 4 rows and chunks of 32 at these M; the large M make a workgroup walk more than one tile / chunk.

BG_MLP_PARITY_JSON=<path> makes the run write the measured pairs there (profiles/r17/mlp_train_parity.json is such a run)."""
import copy
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from brepgen_amd import mlp, training
from oracle.ref_formulation import RefDenoiser
from tests import mlp_ops as ops
from tests import mlp_restate as R
from tests.guarded import guarded
from tests.layer_ops import LN_PAIRS
from tests.train_check import Parity, errs, pooled, same_bits

pytestmark = pytest.mark.gpu
NAME = ops.NAME
HALF = ops.HALF
EPS = float(np.float32(1e-5))
MS_THIN = (1, 2, 3, 31, 32, 33, 63, 64, 65, 257)          # one row; around a chain / chunk of bg_thin_wgrad (4 x 8) and a tile (64); ragged tail
MS_LN = (1, 31, 32, 33, 257)

PARITY = Parity("BG_MLP_PARITY_JSON", "absolute error against fp64 from the same rounded inputs, pooled over the row counts of a case; torch = "
                "stock torch on the same GPU, under the same autocast dtype for 16-bit outputs and in fp32 for fp32 outputs")
record, within_2x, _parity_json = PARITY.record, PARITY.within_2x, PARITY.fixture()


def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def thin_weights(s):
    """(W [768, s], W3 [s, 768], b [768], b3 [s]) fp32 on the device"""
    g = torch.Generator(device="cpu").manual_seed(1000 + s)
    return ((torch.randn(768, s, generator=g) / s ** 0.5).cuda(), (torch.randn(s, 768, generator=g) / 768 ** 0.5).cuda(),
            (0.1 * torch.randn(768, generator=g)).cuda(), (0.1 * torch.randn(s, generator=g)).cuda())


def strided(t, ld, col0):
    """a copy of t [M, s] as columns [col0, col0 + s) of an ld-wide buffer whose other columns hold NaN"""
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, col0:col0 + t.shape[1]] = t
    return buf[:, col0:col0 + t.shape[1]]


def np32(t):
    return t.detach().float().cpu().numpy()


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)


# ---- bg_thin_expand ----

@pytest.mark.parametrize("s", (6, 12, 48))
@pytest.mark.parametrize("ydt", (torch.float32, torch.float16, torch.bfloat16), ids=lambda d: NAME[d])
def test_thin_expand_bits_and_within_twice_torch(ydt, s):
    W, W3, b, _ = thin_weights(s)
    mine, theirs = [], []
    for M in MS_THIN + (16391,):                                   # 16391: 257 tiles for 256 row workgroups
        big = M > 1000
        xdt = torch.float32 if (M % 2 or ydt == torch.float32) else ydt
        x = torch.randn(M, s, generator=_gen("ex", M, s)).to(xdt).cuda()
        out = guarded((M, 768), ydt, "cuda")
        y = ops.thin_expand(x, W, b, ydt, y=out.view)
        out.assert_untouched(f"thin_expand M={M}"), out.assert_fully_written(f"thin_expand M={M}")
        assert same_bits(ops.thin_expand(x, W, b, ydt), y.contiguous())                      # twice the same bits
        if s in (6, 12):                                           # the columns 0:12 / 12:18 of 18-wide rows, in place
            xs = strided(x, 18, 0 if s == 12 else 12)
            assert same_bits(ops.thin_expand(xs, W, b, ydt), y.contiguous())
        ref = x.double() @ W.double().t() + b.double()
        if ydt == torch.float32:
            tor = F.linear(x.float(), W, b)
        else:
            with torch.autocast("cuda", dtype=ydt):
                tor = F.linear(x, W, b)
        assert tor.dtype == ydt
        mine.append((y.double() - ref).abs()), theirs.append((tor.double() - ref).abs())
        if not big:
            want = dev(R.thin_expand(np32(x), np32(W).T, np32(b)), ydt)
            assert same_bits(y.contiguous(), want), (M, s)
            # W taken k-major ([s, 768]: fc_out's data gradient), no bias
            y2 = ops.thin_expand(x, W3, None, ydt, k_major=True)
            assert same_bits(y2, dev(R.thin_expand(np32(x), np32(W3)), ydt)), (M, s)
    within_2x(f"thin_expand s={s}", f"y {NAME[ydt]}", pooled(mine), pooled(theirs))


# ---- bg_thin_contract ----

@pytest.mark.parametrize("n", (6, 18, 48))
@pytest.mark.parametrize("adt", HALF, ids=lambda d: NAME[d])
def test_thin_contract_bits_and_within_twice_torch(adt, n):
    _, W3, _, b3 = thin_weights(n)
    mine, theirs = [], []
    for M in MS_THIN + (16391,):                                   # 16391: 257 tiles for 256 workgroups
        a = torch.randn(M, 768, generator=_gen("co", M, n)).to(adt).cuda()
        out = guarded((M, n), torch.float32, "cuda")
        y = ops.thin_contract(a, W3, b3, y=out.view)
        out.assert_untouched(f"thin_contract M={M}"), out.assert_fully_written(f"thin_contract M={M}")
        assert same_bits(ops.thin_contract(a, W3, b3), y.contiguous())
        ref = a.double() @ W3.double().t() + b3.double()
        tor = F.linear(a.float(), W3, b3)
        mine.append((y.double() - ref).abs()), theirs.append((tor.double() - ref).abs())
        if M <= 257:
            assert same_bits(y.contiguous(), dev(R.thin_contract(np32(a), np32(W3), np32(b3)))), (M, n)
        if M == 33:
            assert same_bits(ops.thin_contract(a, W3, None), dev(R.thin_contract(np32(a), np32(W3))))
    within_2x(f"thin_contract n={n}", f"y from {NAME[adt]}", pooled(mine), pooled(theirs))


# ---- bg_thin_wgrad ----

@pytest.mark.parametrize("s", (6, 12, 18, 48))
@pytest.mark.parametrize("udt", HALF, ids=lambda d: NAME[d])
def test_thin_wgrad_bits_and_within_twice_torch(udt, s):
    mine, theirs = {k: [] for k in ("g", "colsum_u", "colsum_t")}, {k: [] for k in ("g", "colsum_u", "colsum_t")}
    big_M = 8 * 64 * (256 // ((s + 7) // 8)) + 77                  # past 64-row chains for every row workgroup: workgroups walk two chunks
    for M in (1, 3, 4, 5, 31, 32, 33, 257) + ((big_M,) if s in (18, 48) else ()):
        big = M > 1000
        tdt = torch.float32 if M % 2 else udt
        t = torch.randn(M, s, generator=_gen("wt", M, s)).to(tdt).cuda()
        u = torch.randn(M, 768, generator=_gen("wu", M, s)).to(udt).cuda()
        if s in (6, 12):
            t = strided(t, 18, 0 if s == 12 else 12)
        nws = ops.wgrad_workspace_bytes(M, s) // 8
        gout, cout, ws = guarded((s, 768), torch.float32, "cuda"), guarded((1, 768), torch.float32, "cuda"), guarded((1, nws), torch.float64, "cuda")
        g, cu = ops.thin_wgrad(t, u, False, 1, g=gout.view, colsum=cout.view.view(768), ws=ws.view)
        for buf, what in ((gout, "g"), (cout, "colsum"), (ws, "workspace")):
            buf.assert_untouched(f"thin_wgrad M={M} {what}")
        gout.assert_fully_written("g"), cout.assert_fully_written("colsum")
        gt_out, ct_out = guarded((768, s), torch.float32, "cuda"), guarded((1, s), torch.float32, "cuda")
        gt, ct = ops.thin_wgrad(t, u, True, 2, g=gt_out.view, colsum=ct_out.view.view(s))
        gt_out.assert_untouched("g transposed"), ct_out.assert_untouched("colsum of t"), gt_out.assert_fully_written("g transposed")
        assert same_bits(gt.t().contiguous(), g.contiguous())                                 # the layout option moves no bit
        g0, none = ops.thin_wgrad(t, u, False, 0)
        assert none is None and same_bits(g0, g.contiguous())
        g1, cu1 = ops.thin_wgrad(t, u, False, 1)
        assert same_bits(g1, g.contiguous()) and same_bits(cu1, cu.contiguous())              # twice the same bits
        ref = dict(g=t.double().t() @ u.double(), colsum_u=u.double().sum(0), colsum_t=t.double().sum(0))
        tor = dict(g=t.float().t() @ u.float(), colsum_u=u.float().sum(0), colsum_t=t.float().sum(0))
        got = dict(g=g, colsum_u=cu.reshape(768), colsum_t=ct.reshape(s))
        for k in mine:
            mine[k].append((got[k].double() - ref[k]).abs()), theirs[k].append((tor[k].double() - ref[k]).abs())
        if not big:
            wg, wu, wt = R.thin_wgrad(np32(t), np32(u))
            assert same_bits(g.contiguous(), dev(wg)) and same_bits(cu.contiguous().reshape(768), dev(wu)), (M, s)
            assert same_bits(ct.contiguous().reshape(s), dev(wt)), (M, s)
    for k in mine:
        within_2x(f"thin_wgrad s={s}", f"{k} {NAME[udt]}", pooled(mine[k]), pooled(theirs[k]))


# ---- bg_ln_silu_train_fwd / bg_ln_silu_bwd ----

@functools.lru_cache(maxsize=None)
def affine():
    g = torch.Generator(device="cpu").manual_seed(768)
    return (1.0 + 0.1 * torch.randn(768, generator=g)).cuda(), (0.1 * torch.randn(768, generator=g)).cuda()


def _ln_silu_sides(x, dh, wd):
    """(h, dx, dgamma, dbeta) of SiLU(LayerNorm(x)) and its autograd in the working dtype wd, from the rounded x / dh"""
    gamma, beta = affine()
    xw = x.to(wd).clone().requires_grad_(True)
    gw, bw = gamma.to(wd).clone().requires_grad_(True), beta.to(wd).clone().requires_grad_(True)
    h = F.silu(F.layer_norm(xw, (768,), gw, bw, EPS))
    h.backward(dh.to(wd))
    return h.detach(), xw.grad, gw.grad, bw.grad


@pytest.mark.parametrize("xdt, hdt", LN_PAIRS, ids=[f"{NAME[a]}-{NAME[b]}" for a, b in LN_PAIRS])
def test_ln_silu_within_twice_torch(xdt, hdt):
    gamma, beta = affine()
    keys = ("h", "dx", "dgamma", "dbeta")
    mine, theirs = {k: [] for k in keys}, {k: [] for k in keys}
    for M in MS_LN + (32777,):                                     # 32777: the chain plan leaves its minimum of 4 rows
        x = (0.5 + 1.5 * torch.randn(M, 768, generator=_gen("lx", M))).to(xdt).cuda()
        dh = torch.randn(M, 768, generator=_gen("ld", M)).to(hdt).cuda()
        hout, sout, dxout = guarded((M, 768), hdt, "cuda"), guarded((M, 2), torch.float32, "cuda"), guarded((M, 768), xdt, "cuda")
        h, stats = ops.ln_silu_fwd(x, gamma, beta, hdt, h=hout.view, stats=sout.view)
        stats = stats.contiguous()
        nws = ops.ln_workspace_bytes(M) // 8
        ws, dgo, dbo = guarded((1, nws), torch.float64, "cuda"), guarded((1, 768), torch.float32, "cuda"), guarded((1, 768), torch.float32, "cuda")
        dx, dg, db = ops.ln_silu_bwd(dh, x, stats, gamma, beta, dx=dxout.view, dgamma=dgo.view.view(768), dbeta=dbo.view.view(768), ws=ws.view)
        for buf in (hout, sout, dxout, ws, dgo, dbo):
            buf.assert_untouched(f"ln_silu M={M}")
        for buf in (hout, sout, dxout, dgo, dbo):
            buf.assert_fully_written(f"ln_silu M={M}")
        h2, stats2 = ops.ln_silu_fwd(x, gamma, beta, hdt)
        dx2, dg2, db2 = ops.ln_silu_bwd(dh, x, stats2, gamma, beta)
        dx3, none_g, none_b = ops.ln_silu_bwd(dh, x, stats2, gamma, beta, grads=False)
        assert same_bits(h2, h.contiguous()) and same_bits(stats2, stats) and same_bits(dx2, dx.contiguous()) and same_bits(dx3, dx2)
        assert same_bits(dg2, dg.contiguous()) and same_bits(db2, db.contiguous()) and none_g is None and none_b is None
        ref = _ln_silu_sides(x, dh, torch.float64)
        th, tdx, tdg, tdb = _ln_silu_sides(x, dh, torch.float32)
        tor = (th.to(hdt), tdx.to(xdt), tdg, tdb)                  # autocast's casts: h for the next Linear, dx back to x's dtype
        assert h.dtype == hdt and dx.dtype == xdt and bool(torch.isfinite(h).all()) and bool(torch.isfinite(dx).all())
        for k, got, r, t in zip(keys, (h, dx, dg, db), ref, tor):
            mine[k].append((got.double() - r).abs()), theirs[k].append((t.double() - r).abs())
        if M == 33:                                                # the restatement: numpy's exp is not expf -- by error, with the LN order's slack
            rh, rstats = R.ln_silu_fwd(np32(x), np32(gamma), np32(beta), EPS)
            assert float((dev(rh).double() - ref[0]).abs().max()) <= 4e-6
            assert float((h.double() - dev(rh).double()).abs().max()) <= (4e-6 if hdt == torch.float32 else 2.0 ** -8 * 8)
    for k in keys:
        within_2x(f"ln_silu {NAME[xdt]}->{NAME[hdt]}", k, pooled(mine[k]), pooled(theirs[k]))


# ---- bg_masked_mse_bwd ----

@pytest.mark.parametrize("valid", ("all", "some", "one", "none"))
@pytest.mark.parametrize("cols", ((0, 12), (12, 18)))
def test_masked_mse_backward_bits_and_zeros(valid, cols):
    rows, ld, scale = 2 * 3 * 5 * 7 + 1, 18, 65536.0
    gen = _gen("mse", valid, cols)
    pred, target = torch.randn(rows, ld, generator=gen), torch.randn(rows, ld, generator=gen)
    mask = {"all": torch.zeros(rows, dtype=torch.bool), "some": torch.rand(rows, generator=gen) < 0.4,
            "one": torch.arange(rows) != 101, "none": torch.ones(rows, dtype=torch.bool)}[valid]
    poisoned = pred.clone()
    poisoned[mask] = float("nan")
    poisoned[:, :cols[0]] = float("inf")
    poisoned[:, cols[1]:] = float("nan")
    p, t, m = poisoned.cuda(), target.cuda(), mask.to(torch.uint8).cuda()
    g = torch.tensor(scale, device="cuda")
    out3 = ops.masked_mse(p, t, m, cols)
    out = guarded((rows, ld), torch.float32, "cuda")
    d = ops.masked_mse_bwd(p, t, m, cols, out3, g, dpred=out.view)
    out.assert_untouched("masked_mse_bwd"), out.assert_fully_written("masked_mse_bwd")
    assert same_bits(ops.masked_mse_bwd(p, t, m, cols, out3, g), d.contiguous())
    n_valid = int((~mask).sum())
    assert float(out3[2]) == n_valid
    want = dev(R.masked_mse_bwd(poisoned.numpy(), target.numpy(), m.cpu().numpy(), cols, float(n_valid), scale))
    assert same_bits(d.contiguous(), want)
    dz = d.contiguous()
    assert bool((dz[m.bool()] == 0).all()) and bool((dz[:, :cols[0]] == 0).all()) and bool((dz[:, cols[1]:] == 0).all())
    if valid == "none":
        assert float(out3[0]) == 0.0 and bool((dz == 0).all())
        return
    # against autograd of the indexed loss in fp64
    pd = pred.double().cuda().requires_grad_(True)
    (F.mse_loss(pd[~mask.cuda()][:, cols[0]:cols[1]], t.double()[~mask.cuda()][:, cols[0]:cols[1]]) * scale).backward()
    assert float((dz.double() - pd.grad).abs().max()) <= 4 * 2.0 ** -24 * float(pd.grad.abs().max())
    if valid == "all":                                             # no mask at all is the all-valid mask
        assert same_bits(ops.masked_mse_bwd(p, t, None, cols, out3, g), dz)


def test_mse_loss_is_differentiable_without_indexing():
    gen = _gen("loss")
    pred = torch.randn(2, 3, 5, 18, generator=gen).cuda().requires_grad_(True)
    noise = torch.randn(2, 3, 5, 18, generator=gen).cuda()
    face_mask = torch.tensor([[False, False, True], [False, True, True]]).cuda()             # over faces: broadcast over the edges
    loss = training.mse_loss(pred, noise, face_mask, cols=(0, 12))
    (loss * 1024.0).backward()
    row_mask = face_mask.unsqueeze(-1).expand(2, 3, 5)
    pd = pred.detach().double().requires_grad_(True)
    want = F.mse_loss(pd[~row_mask][:, :12], noise.double()[~row_mask][:, :12])
    (want * 1024.0).backward()
    assert loss.dim() == 0 and abs(float(loss.detach()) - float(want.detach())) <= 1e-6 * float(want.detach())
    assert float((pred.grad.double() - pd.grad).abs().max()) <= 4 * 2.0 ** -24 * float(pd.grad.abs().max())
    assert bool((pred.grad[row_mask] == 0).all()) and bool((pred.grad[..., 12:] == 0).all())
    with pytest.raises(ValueError):
        training.mse_loss(pred, noise.requires_grad_(True))


# ---- DeviceMLP against the nn.Sequential it adopted ----

def _mlp_grads(seq, x, g, scale, dtype):
    """(out, {name: gradient / scale}) of sum(out * g) * scale; dtype None: the module's own precision (the fp64 copy)"""
    seq.zero_grad(set_to_none=True)
    if dtype is None:
        out = seq(x.double())
    else:
        with torch.autocast("cuda", dtype=dtype):
            out = seq(x)
    ((out.double() * g).sum() * scale).backward()
    return out.detach(), {k: p.grad.double() / scale for k, p in seq.named_parameters()}


@pytest.mark.parametrize("k, n, lead", [(6, 768, (2, 35)), (48, 768, (2, 35)), (768, 768, (3,)), (768, 6, (2, 35)), (768, 18, (2, 35))],
                         ids=["6-768", "48-768", "time_embed", "768-6", "768-18"])
@pytest.mark.parametrize("dtype", HALF, ids=lambda d: NAME[d])
def test_device_mlp_against_the_sequential_it_adopted(dtype, k, n, lead):
    torch.manual_seed(17 * k + n)
    base = nn.Sequential(nn.Linear(k, 768), nn.LayerNorm(768), nn.SiLU(), nn.Linear(768, n)).cuda()
    with torch.no_grad():
        base[1].weight.add_(0.1 * torch.randn_like(base[1].weight)), base[1].bias.add_(0.1 * torch.randn_like(base[1].bias))
    gen = _gen("mlp", k, n)
    x = torch.randn(*lead, k, generator=gen).cuda()
    g = torch.randn(*lead, n, generator=gen).double().cuda()
    scale = 1024.0 if dtype == torch.float16 else 1.0
    ref_out, ref = _mlp_grads(copy.deepcopy(base).double(), x, g, 1.0, None)
    plain_out, plain = _mlp_grads(copy.deepcopy(base), x, g, scale, dtype)
    ours_mod = mlp.DeviceMLP(copy.deepcopy(base))
    out, ours = _mlp_grads(ours_mod, x, g, scale, dtype)
    assert out.dtype == plain_out.dtype == dtype and out.shape == plain_out.shape and list(ours) == list(ref)
    case = f"DeviceMLP {k}->{n} {NAME[dtype]}"
    within_2x(case, "out", errs(out, ref_out), errs(plain_out, ref_out))
    for name in ref:
        assert ours_mod.get_parameter(name).grad.dtype == torch.float32
        within_2x(case, name, errs(ours[name], ref[name]), errs(plain[name], ref[name]))
    out2, again = _mlp_grads(ours_mod, x, g, scale, dtype)
    assert same_bits(out2, out) and all(torch.equal(again[name], ours[name]) for name in ours)


# ---- whole denoisers ----

def _small(kind, use_cf, seed):
    torch.manual_seed(seed)
    m = RefDenoiser(kind, use_cf)
    m.net.layers = nn.ModuleList(list(m.net.layers)[:2])
    m.net.num_layers = 2
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, nn.MultiheadAttention):
            mod.dropout = 0.0
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.LayerNorm):
                mod.weight.add_(0.1 * torch.randn_like(mod.weight)), mod.bias.add_(0.1 * torch.randn_like(mod.bias))
    return m.cuda().train()


def _net_case(kind):
    gen = _gen("net", kind)
    r = lambda *shape: torch.randn(*shape, generator=gen).cuda()      # noqa: E731
    if kind == "SurfZNet":
        B, S = 3, 7
        mask = torch.zeros(B, S, dtype=torch.bool)
        mask[0, 5:], mask[2, 3:] = True, True
        t = torch.tensor([10, 500, 990]).cuda()
        return (r(B, S, 48), t, r(B, S, 6), mask.cuda(), None), r(B, S, 48), mask.cuda(), 0
    B, S, E = 2, 3, 5
    mask = torch.zeros(B, S, E, dtype=torch.bool)
    mask[0, 1, 3:], mask[1, 2, :], mask[1, 0, 4:] = True, True, True
    t = torch.tensor([10, 900]).cuda()
    cl = torch.tensor([[3], [7]]).cuda()
    return (r(B, S, E, 18), t, r(B, S, E, 6), r(B, S, 6), r(B, S, 48), mask.cuda(), cl), r(B, S, E, 18), mask.cuda(), 0


def _fp64_copy(model):
    """the model in fp64; its sincos table stays the fp32 one every side reads (cast at time_embed's door)"""
    m = copy.deepcopy(model).double()
    m.time_embed.register_forward_pre_hook(lambda mod, a: (a[0].double(),))
    return m


def _to64(args):
    return tuple(a.double() if torch.is_tensor(a) and a.is_floating_point() else a for a in args)


def _net_grads(model, args, noise, mask, scale, dtype, device_loss):
    model.zero_grad(set_to_none=True)
    if dtype is None:
        pred = model(*_to64(args))
        loss = F.mse_loss(pred[~mask], noise.double()[~mask])
    else:
        with torch.autocast("cuda", dtype=dtype):
            pred = model(*args)
            loss = training.mse_loss(pred, noise, mask) if device_loss else F.mse_loss(pred[~mask], noise[~mask])
    (loss * scale).backward()
    return pred.detach(), {k: p.grad.double() / scale for k, p in model.named_parameters()}


@pytest.mark.parametrize("kind, use_cf", [("SurfZNet", False), ("EdgeZNet", True)], ids=["SurfZNet", "EdgeZNet_cf"])
@pytest.mark.parametrize("dtype", HALF, ids=lambda d: NAME[d])
def test_whole_denoiser_after_use_device_training(dtype, kind, use_cf):
    base = _small(kind, use_cf, 5)
    args, noise, mask, _ = _net_case(kind)
    scale = 1024.0 if dtype == torch.float16 else 1.0
    ref_pred, ref = _net_grads(_fp64_copy(base), args, noise, mask, 1.0, None, False)
    plain_model = copy.deepcopy(base)
    plain_pred, plain = _net_grads(plain_model, args, noise, mask, scale, dtype, False)
    ours_model = copy.deepcopy(base)
    keys = list(ours_model.state_dict().keys())
    assert training.use_device_training(ours_model, seed=3) is ours_model and list(ours_model.state_dict().keys()) == keys
    n_mlps = sum(isinstance(c, mlp.DeviceMLP) for c in ours_model.children())
    assert n_mlps == {"SurfZNet": 4, "EdgeZNet": 7}[kind]
    pred, ours = _net_grads(ours_model, args, noise, mask, scale, dtype, True)
    case = f"{kind} {NAME[dtype]}"
    assert list(ours) == list(ref) and pred.dtype == plain_pred.dtype == dtype
    within_2x(case, "pred", errs(pred[~mask], ref_pred[~mask]), errs(plain_pred[~mask], ref_pred[~mask]))
    # The loss value.  One scalar's error against one scalar's error is the ratio of two draws of the same distribution (each is a sum
    # of ~1000 signed terms 2 (p - t) dp / n that mostly cancel; 2e-7 and 2e-4 both occur), so the yardstick is applied to the errors
    # pooled over 8 targets: the step's own noise and 7 more draws against the same three predictions.
    mine, theirs = [], []
    for i in range(8):
        tgt = noise if i == 0 else torch.randn(noise.shape, generator=_gen("loss", kind, i)).cuda()
        want = F.mse_loss(ref_pred[~mask], tgt.double()[~mask])
        got = training.mse_loss(pred, tgt, mask)
        assert got.dim() == 0 and got.dtype == torch.float32
        mine.append((got.double() - want).abs().reshape(1)), theirs.append((F.mse_loss(plain_pred[~mask].float(), tgt[~mask]).double() - want).abs().reshape(1))
        # the loss kernel alone, against fp64 from the SAME prediction: fp32 sums of a row's <= 48 squares, fp64 across, one rounding
        exact = F.mse_loss(pred.double()[~mask], tgt.double()[~mask])
        assert abs(float(got) - float(exact)) <= (noise.shape[-1] + 3) * 2.0 ** -24 * float(exact)
    within_2x(case, "loss, 8 targets", pooled(mine), pooled(theirs))
    for k in ref:
        assert ours_model.get_parameter(k).grad.dtype == torch.float32
        within_2x(case, k, errs(ours[k], ref[k]), errs(plain[k], ref[k]))
    # eval(): the converted model returns what the stock model returns
    with torch.no_grad():
        ref_out = _fp64_copy(base).eval()(*_to64(args))
        with torch.autocast("cuda", dtype=dtype):
            before, after = plain_model.eval()(*args), ours_model.eval()(*args)
    assert after.dtype == before.dtype and after.shape == before.shape
    valid = ~mask
    within_2x(case, "eval output", errs(after[valid], ref_out[valid]), errs(before[valid], ref_out[valid]))
