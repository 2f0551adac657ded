"""The conv-layer backward on the device (csrc/conv_train.hip, brepgen_amd/conv.py) against fp64 evaluated from the same operands on
the device.  The yardstick is the project's (tests/train_check.py, Parity.within_2x): pooled max and mean absolute error <= 2 x the
errors of stock torch computing the same thing under the same autocast dtype, from the same inputs on the same GPU.  For the weight
gradient with fp32 output the derived bound of tests/test_gpu_linear_bwd.py holds as well: products of two 16-bit values are exact in
fp32 and an output is a sum of at most M of them in at most M + S additions, so |dw - ref| <= (M + S + 2) 2^-24 sum |dy| |a|.

BG_CONV_PARITY_JSON=<path> makes the run write the measured pairs there (profiles/r18/conv_train_parity.json is such a run)."""
import copy
import functools

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
from tests.guarded import guarded, strided_input
from tests.train_check import Parity, errs, same_bits

pytestmark = pytest.mark.gpu
DTYPES = (torch.float16, torch.bfloat16)
NAME = ops.NAME
U24 = 2.0 ** -24
PARITY = Parity("BG_CONV_PARITY_JSON")
record, within_2x, _parity_json = PARITY.record, PARITY.within_2x, PARITY.fixture()
by_name = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])


def nchw(t):
    return t.permute(0, 3, 1, 2)


def cl(t):
    return t.permute(0, 2, 3, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# bg_conv_wgrad
# ---------------------------------------------------------------------------------------------------------------------------------
WGRAD_CASES = [(1, 4, 4, 128, 128, 3, 3), (3, 4, 4, 128, 256, 3, 3), (2, 8, 8, 256, 128, 3, 3), (3, 1, 8, 128, 128, 1, 5), (2, 2, 2, 128, 128, 3, 3)]


@functools.lru_cache(maxsize=None)
def wcase(shape, dtype):
    """inputs, the fp64 reference and torch's conv2d weight / bias gradient in the 16-bit dtype (what autocast runs) -- computed once"""
    S, H, W, N, C, kh, kw = shape
    dy, a = ops.draw(S, H, W, N, C, dtype, 1000 * S + H * W + N)
    ref_w, ref_b = R.wgrad(dy.double(), a.double(), kh, kw)
    abs_w, abs_b = R.wgrad(dy.double(), a.double(), kh, kw, absolute=True)
    w = torch.zeros(N, C, kh, kw, dtype=dtype, device="cuda", requires_grad=True)
    b = torch.zeros(N, dtype=dtype, device="cuda", requires_grad=True)
    F.conv2d(nchw(a), w, b, padding=(kh // 2, kw // 2)).backward(nchw(dy))
    tw = R.pack_fwd(w.grad)
    return dy, a, ref_w, ref_b, abs_w, abs_b, errs(tw, ref_w), errs(b.grad, ref_b)


def check_bound_a(dw, db, M, S, ref_w, ref_b, abs_w, abs_b, what):
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), what
    f = (M + S + 2) * U24
    ew, eb = (dw.double() - ref_w).abs(), (db.double() - ref_b).abs()
    assert bool((ew <= f * abs_w).all()), (what, "dw", float((ew / (f * abs_w).clamp_min(1e-300)).max()))
    assert bool((eb <= f * abs_b).all()), (what, "db", float((eb / (f * abs_b).clamp_min(1e-300)).max()))


@by_name
@pytest.mark.parametrize("shape", WGRAD_CASES, ids=lambda s: "x".join(map(str, s)))
def test_wgrad_accuracy(shape, dtype):
    S, H, W, N, C, kh, kw = shape
    dy, a, ref_w, ref_b, abs_w, abs_b, tw, tb = wcase(shape, dtype)
    for split in (1, 3, 0):
        sp = split or ops.auto_split(*shape)
        for odt in (torch.float32, dtype):
            tag = f"conv_wgrad {'x'.join(map(str, shape))} {NAME[dtype]}->{NAME[odt]} split={split}(S={sp})"
            dw, db = ops.wgrad(dy, a, *shape, odt, split)
            if odt == torch.float32:
                check_bound_a(dw, db, S * H * W, sp, ref_w, ref_b, abs_w, abs_b, tag)
            record(tag, "db", errs(db, ref_b), tb)
            within_2x(tag, "dw", errs(dw, ref_w), tw)


@by_name
def test_wgrad_bits(dtype):
    shape = (2, 8, 8, 256, 128, 3, 3)
    S, H, W, N, C, kh, kw = shape
    dy, a = wcase(shape, dtype)[:2]
    for split in (1, 3, 0):
        p, q = ops.wgrad(dy, a, *shape, torch.float32, split), ops.wgrad(dy, a, *shape, torch.float32, split)
        assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]), split                 # two calls, identical bits
    # a row of dw depends on its own dy column alone
    n0 = 77
    others = torch.arange(N, device="cuda") != n0
    dy2 = dy.clone()
    dy2[..., n0] = dy2[..., n0] * 0.5 + 1.0
    for split in (1, 3):
        (wa, ba), (wb, bb) = ops.wgrad(dy, a, *shape, torch.float32, split), ops.wgrad(dy2, a, *shape, torch.float32, split)
        assert torch.equal(wa[others], wb[others]) and torch.equal(ba[others], bb[others])
        assert not torch.equal(wa[n0], wb[n0]) and not torch.equal(ba[n0], bb[n0])
    # overflow in one dy column marks that row of dw and db, and only that row
    dy3 = dy.clone()
    dy3[1, 3, 5, n0] = float("inf")
    for split in (1, 3):
        for odt in (torch.float32, dtype):
            dw, db = ops.wgrad(dy3, a, *shape, odt, split)
            assert not bool(torch.isfinite(dw[n0]).any()) and not bool(torch.isfinite(db[n0]))
            assert bool(torch.isfinite(dw[others]).all()) and bool(torch.isfinite(db[others]).all())


@by_name
@pytest.mark.parametrize("S, H, W, split", [(1, 2, 2, 1), (1, 2, 2, 3), (3, 4, 4, 1), (3, 4, 4, 0), (2, 8, 8, 1), (2, 8, 8, 3), (2, 8, 8, 0)])
def test_wgrad_guarded(S, H, W, split, dtype):
    """pixel strides > channels, NaN-sentinel padding and guard bands around dy / a: a padding column or a pixel outside the tensors in any
    product makes the result NaN.  dw / db: every promised element written, nothing outside.  M = 4, 48, 128."""
    N, C, kh, kw = 256, 128, 3, 3
    shape = (S, H, W, N, C, kh, kw)
    dy, a, ref_w, ref_b, abs_w, abs_b = wcase(shape, dtype)[:6]
    M = S * H * W
    dys, a_s = strided_input(dy.reshape(M, N), N + 8), strided_input(a.reshape(M, C), C + 24)
    sp = split or ops.auto_split(*shape)
    for odt in (torch.float32, dtype):
        gw, gb = guarded((N, kh * kw * C), odt, "cuda"), guarded((N,), odt, "cuda")
        ops.wgrad(dys, a_s, *shape, odt, split, ld_dy=N + 8, ld_a=C + 24, dw=gw.view, db=gb.view)
        for g, what in ((gw, "dw"), (gb, "db")):
            g.assert_untouched(what)
            g.assert_fully_written(what)
        if odt == torch.float32:
            check_bound_a(gw.view.clone(), gb.view.reshape(N).clone(), M, sp, ref_w, ref_b, abs_w, abs_b, f"guarded {shape} split={split}")
    gb = guarded((N,), torch.float32, "cuda")                                  # no bias requested: db is not touched
    dw, _ = ops.wgrad(dys, a_s, *shape, torch.float32, split, bias=False, ld_dy=N + 8, ld_a=C + 24)
    gb.assert_untouched("db (NULL)")
    assert bool(((dw.double() - ref_w).abs() <= (M + sp + 2) * U24 * abs_w).all())


@by_name
@pytest.mark.parametrize("H, W, kh, kw", [(4, 4, 3, 3), (2, 2, 3, 3), (1, 8, 1, 5)])
def test_wgrad_border_pixels_do_not_read_the_neighbouring_sample(H, W, kh, kw, dtype):
    """samples 0 and 2 hold a huge finite `a` and a zero dy: they contribute exactly zero, unless a border tap of sample 1 reads across"""
    S, N, C = 3, 128, 128
    dy, a = ops.draw(S, H, W, N, C, dtype, 42)
    huge = 3.0e4 if dtype == torch.float16 else 1.0e30
    a[0], a[2] = huge, -huge
    dy[0], dy[2] = 0, 0
    ref_w, ref_b = R.wgrad(dy[1:2].double(), a[1:2].double(), kh, kw)
    abs_w, abs_b = R.wgrad(dy[1:2].double(), a[1:2].double(), kh, kw, absolute=True)
    for split in (1, 3):
        dw, db = ops.wgrad(dy, a, S, H, W, N, C, kh, kw, torch.float32, split)
        check_bound_a(dw, db, S * H * W, split, ref_w, ref_b, abs_w, abs_b, f"neighbour {H}x{W} split={split}")


# ---------------------------------------------------------------------------------------------------------------------------------
# bg_conv_weight_pack
# ---------------------------------------------------------------------------------------------------------------------------------
@by_name
@pytest.mark.parametrize("N, C, kh, kw", [(128, 128, 3, 3), (256, 128, 1, 5), (128, 256, 1, 1), (32, 64, 5, 5)])
def test_weight_pack_bits(N, C, kh, kw, dtype):
    g = torch.Generator(device="cpu").manual_seed(N + C + kh)
    w32 = torch.randn(N, C, kh, kw, generator=g).cuda()
    for src in (w32, w32.to(dtype)):
        want_f, want_d = R.pack_fwd(src).to(dtype).contiguous(), R.pack_dgrad(src).to(dtype).contiguous()
        gf, gd = guarded((N, kh * kw * C), dtype, "cuda"), guarded((C, kh * kw * N), dtype, "cuda")
        ops.weight_pack(src, dtype, out_f=gf.view, out_d=gd.view)
        for gq, what in ((gf, "fwd"), (gd, "dgrad")):
            gq.assert_untouched(what)
            gq.assert_fully_written(what)
        assert same_bits(gf.view.clone(), want_f) and same_bits(gd.view.clone(), want_d)
        only_f, none_d = ops.weight_pack(src, dtype, dgrad=False)
        none_f, only_d = ops.weight_pack(src, dtype, fwd=False)
        assert none_d is None and none_f is None and same_bits(only_f, want_f) and same_bits(only_d, want_d)


# ---------------------------------------------------------------------------------------------------------------------------------
# the data gradient: a forward convolution of dy with the reversed-tap pack
# ---------------------------------------------------------------------------------------------------------------------------------
@by_name
@pytest.mark.parametrize("S, H, W, implicit", [(2, 4, 4, False), (4, 32, 32, True)])
def test_data_gradient(S, H, W, implicit, dtype):
    """dy with 128 channels -> dx with 256: the im2col + GEMM path at (2, 4, 4), the implicit GEMM at (4, 32, 32) = 64 tiles"""
    N, C, kh, kw = 128, 256, 3, 3
    g = torch.Generator(device="cpu").manual_seed(S * H)
    dy = torch.randn(S, H, W, N, generator=g).to(dtype).cuda()
    w = (torch.randn(N, C, kh, kw, generator=g) / (kh * kw * N) ** 0.5).to(dtype).cuda()
    ref = R.conv_same(dy.double(), R.pack_dgrad(w.double()), kh, kw)
    x = torch.zeros(S, C, H, W, dtype=dtype, device="cuda", requires_grad=True)
    F.conv2d(x, w, padding=1).backward(nchw(dy))
    da, took_implicit = ops.data_grad(dy.float(), w.float(), dtype)
    assert took_implicit is implicit
    within_2x(f"conv_dgrad {S}x{H}x{W} {N}->{C} {NAME[dtype]} {'implicit' if implicit else 'im2col'}", "dx", errs(da, ref), errs(cl(x.grad), ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# bg_gn_act_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
GN_CASES = [(1, 1, 128, 32), (3, 16, 128, 32), (2, 64, 512, 32), (2, 8, 128, 1), (5, 65, 256, 32)]
TORCH_ACT = {"none": lambda t: t, "silu": F.silu, "gelu": F.gelu}


def gn_torch(x, gamma, beta, da, G, eps, act):
    """(dx, dgamma, dbeta) by torch.autograd on F.group_norm + activation, in the dtype of the arguments; x [S, P, C]"""
    x, gamma, beta = (t.detach().clone().requires_grad_() for t in (x, gamma, beta))
    a = TORCH_ACT[act](F.group_norm(x.permute(0, 2, 1), G, gamma, beta, eps)).permute(0, 2, 1)
    return torch.autograd.grad(a, (x, gamma, beta), da)


@functools.lru_cache(maxsize=None)
def gcase(shape, act, hostile):
    S, P, C, G = shape
    g = torch.Generator(device="cpu").manual_seed(S * P + C + G)
    x = torch.randn(S, P, C, generator=g)
    if hostile:                                              # |mean| = 50 std in every group
        x = x + 50.0 * (1 - 2 * (torch.arange(C) // (C // G) % 2)).float()
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    da, dskip = torch.randn(S, P, C, generator=g), torch.randn(S, P, C, generator=g)
    x, gamma, beta, da, dskip = (t.cuda() for t in (x, gamma, beta, da, dskip))
    ref = gn_torch(x.double(), gamma.double(), beta.double(), da.double(), G, 1e-6, act)
    tor = gn_torch(x, gamma, beta, da, G, 1e-6, act)
    return x, gamma, beta, da, dskip, ref, tuple(errs(t, r) for t, r in zip(tor, ref))


@pytest.mark.parametrize("hostile", [False, True], ids=["friendly", "hostile"])
@pytest.mark.parametrize("act", ["none", "silu", "gelu"])
@pytest.mark.parametrize("shape", GN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_gn_act_bwd(shape, act, hostile):
    S, P, C, G = shape
    x, gamma, beta, da, dskip, ref, tor = gcase(shape, act, hostile)
    stats = ops.gn_stats(x, G, 1e-6)
    tag = f"gn_act_bwd {'x'.join(map(str, shape))} {act} {'hostile' if hostile else 'friendly'}"
    gx, gg, gb = guarded((S * P, C), torch.float32, "cuda"), guarded((C,), torch.float32, "cuda"), guarded((C,), torch.float32, "cuda")
    ops.gn_act_bwd(da, x, stats, gamma, beta, G, act, dx=gx.view, dgamma=gg.view, dbeta=gb.view)
    for gq, what in ((gx, "dx"), (gg, "dgamma"), (gb, "dbeta")):
        gq.assert_untouched(what)
        gq.assert_fully_written(what)
    dx, dg, db = gx.view.clone().view(S, P, C), gg.view.reshape(C).clone(), gb.view.reshape(C).clone()
    for what, got, r, t in (("dx", dx, ref[0], tor[0]), ("dgamma", dg, ref[1], tor[1]), ("dbeta", db, ref[2], tor[2])):
        within_2x(tag, what, errs(got, r), t)
    # two calls, the same bits; without dgamma / dbeta the same dx
    dx2, dg2, db2 = ops.gn_act_bwd(da, x, stats, gamma, beta, G, act)
    assert same_bits(dx2, dx) and same_bits(dg2, dg) and same_bits(db2, db)
    assert same_bits(ops.gn_act_bwd(da, x, stats, gamma, beta, G, act, params=False)[0], dx)
    # with dskip: the bits of the call without it plus one fp32 add
    dxs, dgs, dbs = ops.gn_act_bwd(da, x, stats, gamma, beta, G, act, dskip=dskip)
    assert same_bits(dxs, dx + dskip) and same_bits(dgs, dg) and same_bits(dbs, db)


# ---------------------------------------------------------------------------------------------------------------------------------
# gn_act_conv and DeviceResnetBlock2D
# ---------------------------------------------------------------------------------------------------------------------------------
class RefBlock(nn.Module):
    """diffusers' ResnetBlock2D without a time embedding (dropout 0, output scale 1), NCHW, from stock modules"""

    def __init__(self, cin, cout, groups=32):
        super().__init__()
        self.norm1, self.conv1 = nn.GroupNorm(groups, cin, eps=1e-6), nn.Conv2d(cin, cout, 3, padding=1)
        self.norm2, self.conv2 = nn.GroupNorm(groups, cout, eps=1e-6), nn.Conv2d(cout, cout, 3, padding=1)
        self.nonlinearity = nn.SiLU()
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)

    def forward(self, x):
        h = self.conv1(self.nonlinearity(self.norm1(x)))
        h = self.conv2(self.nonlinearity(self.norm2(h)))
        return (self.conv_shortcut(x) if hasattr(self, "conv_shortcut") else x) + h


def jitter_norms(m, gen):
    with torch.no_grad():
        for q in m.modules():
            if isinstance(q, nn.GroupNorm):
                q.weight.add_(0.1 * torch.randn(q.weight.shape, generator=gen)), q.bias.add_(0.1 * torch.randn(q.bias.shape, generator=gen))


def grads_of(module, x, g, scale, run):
    """(out, dx, {name: gradient}) / scale of the loss sum(out * g) * scale in fp64; run(module, x) -> out"""
    module.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_()
    out = run(module, x)
    ((out.double() * g).sum() * scale).backward()
    return out.detach(), x.grad.double() / scale, {k: p.grad.double() / scale for k, p in module.named_parameters()}


def compare(tag, ours, tor, ref, permute_out):
    (o_out, o_dx, o_g), (t_out, t_dx, t_g), (r_out, r_dx, r_g) = ours, tor, ref
    within_2x(tag, "out", errs(permute_out(o_out), r_out), errs(t_out, r_out))
    within_2x(tag, "dx", errs(permute_out(o_dx), r_dx), errs(t_dx, r_dx))
    assert set(o_g) == set(r_g)
    for k in r_g:
        assert o_g[k].shape == r_g[k].shape and bool(torch.isfinite(o_g[k]).all()), k
        within_2x(tag, f"d {k}", errs(o_g[k], r_g[k]), errs(t_g[k], r_g[k]))


@by_name
@pytest.mark.parametrize("scale", [1.0, 65536.0], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("cin, cout, hw", [(128, 128, 4), (128, 256, 4), (128, 128, 8), (128, 256, 8)])
def test_resnet_block(cin, cout, hw, scale, dtype):
    S = 3
    gen = torch.Generator(device="cpu").manual_seed(cin + cout + hw)
    torch.manual_seed(cin + cout + hw)
    ref32 = RefBlock(cin, cout)
    jitter_norms(ref32, gen)
    ref32 = ref32.cuda()
    ref64 = copy.deepcopy(ref32).double()
    dev = bga.use_device_resnets(nn.ModuleList([copy.deepcopy(ref32)]))[0]
    assert isinstance(dev, CV.DeviceResnetBlock2D) and dev.conv1.weight.dtype == torch.float32
    x = torch.randn(S, cin, hw, hw, generator=gen).cuda()
    g = (torch.randn(S, cout, hw, hw, generator=gen) * 1e-3).double().cuda()

    def autocast(m, t):
        with torch.autocast("cuda", dtype=dtype):
            return m(t)

    ref = grads_of(ref64, x.double(), g, 1.0, lambda m, t: m(t))
    tor = grads_of(ref32, x, g, scale, autocast)
    ours = grads_of(dev, cl(x).contiguous(), cl(g).contiguous(), scale, autocast)
    assert ours[0].dtype == torch.float32 and ours[0].shape == (S, hw, hw, cout)
    assert all(v.dtype == torch.float32 for v in (p.grad for p in dev.parameters()))
    compare(f"resnet {cin}->{cout} {S}x{hw}x{hw} {NAME[dtype]} scale={scale:g}", ours, tor, ref, nchw)


@by_name
def test_gn_act_conv_1d(dtype):
    """the 1-D blocks' layer: GroupNorm(1, C) + GELU + Conv1d k5 at L = 8, with a residual"""
    S, L, C, N = 3, 8, 128, 128
    gen = torch.Generator(device="cpu").manual_seed(11)
    torch.manual_seed(11)

    class Ref(nn.Module):
        def __init__(self):
            super().__init__()
            self.norm, self.conv = nn.GroupNorm(1, C, eps=1e-5), nn.Conv1d(C, N, 5, padding=2)

        def forward(self, x):
            return self.conv(F.gelu(self.norm(x)))

    ref32 = Ref()
    jitter_norms(ref32, gen)
    ref32 = ref32.cuda()
    ref64, dev = copy.deepcopy(ref32).double(), copy.deepcopy(ref32)
    x = torch.randn(S, C, L, generator=gen).cuda()
    res = torch.randn(S, N, L, generator=gen).cuda()
    g = (torch.randn(S, N, L, generator=gen) * 1e-3).double().cuda()
    ncl = lambda t: t.permute(0, 2, 1)

    def autocast(m, t):
        with torch.autocast("cuda", dtype=dtype):
            return m(t) + res

    def ours_run(m, t):
        with torch.autocast("cuda", dtype=dtype):
            return bga.gn_act_conv(t, m.norm, m.conv, act="gelu", res=ncl(res).contiguous())

    ref = grads_of(ref64, x.double(), g, 1.0, lambda m, t: m(t) + res.double())
    tor = grads_of(ref32, x, g, 1.0, autocast)
    ours = grads_of(dev, ncl(x).contiguous(), ncl(g).contiguous(), 1.0, ours_run)
    compare(f"gn_act_conv 1-D k5 L={L} {NAME[dtype]}", ours, tor, ref, ncl)
    # dres = dy; a plain convolution (norm=None) runs too
    r = ncl(res).contiguous().requires_grad_()
    with torch.autocast("cuda", dtype=dtype):
        y = bga.gn_act_conv(ncl(x).contiguous(), None, dev.conv, res=r)
    dy = torch.randn_like(y)
    y.backward(dy)
    assert torch.equal(r.grad, dy)
    plain = (F.conv1d(x.double(), ref64.conv.weight, ref64.conv.bias, padding=2) + res.double()).detach()
    with torch.autocast("cuda", dtype=dtype):
        t_plain = (ref32.conv(x) + res).detach()
    within_2x(f"gn_act_conv 1-D plain {NAME[dtype]}", "out", errs(ncl(y.detach()), plain), errs(t_plain, plain))


def test_use_device_resnets_and_rules():
    seq = nn.Sequential(RefBlock(128, 128), RefBlock(128, 256)).cuda()
    up = _UpBlock2D(256, 128, 2, 32, True).cuda()
    for m in (seq, up):
        before = {k: id(p) for k, p in m.named_parameters()}
        keys = list(m.state_dict())
        assert bga.use_device_resnets(m) is m
        assert {k: id(p) for k, p in m.named_parameters()} == before and list(m.state_dict()) == keys
    assert all(isinstance(b, CV.DeviceResnetBlock2D) for b in list(seq) + list(up.resnets))
    x = torch.randn(3, 4, 4, 128, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = seq(x)
        chained = seq[1](seq[0](x))
        z = up.resnets[1](up.resnets[0](torch.randn(3, 4, 4, 256, device="cuda")))
    assert y.shape == (3, 4, 4, 256) and z.shape == (3, 4, 4, 128) and same_bits(y, chained) and bool(torch.isfinite(y).all())
    # outside the kernels' rules: raises, no fallback
    norm, conv = nn.GroupNorm(32, 128).cuda(), nn.Conv2d(128, 128, 3, padding=1).cuda()
    with pytest.raises(ValueError, match="autocast"):
        bga.gn_act_conv(x, norm, conv)
    with pytest.raises(ValueError, match="autocast"):
        seq[0](x)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(_lib.BrepgenHipError):
            bga.gn_act_conv(x.cpu(), norm, conv)
        with pytest.raises(ValueError, match="stride"):
            bga.gn_act_conv(x, norm, nn.Conv2d(128, 128, 3, padding=1, stride=2).cuda())
        with pytest.raises(ValueError, match="powers of two"):
            bga.gn_act_conv(torch.randn(2, 6, 4, 128, device="cuda"), norm, conv)
        with pytest.raises(ValueError, match="multiples of 128"):
            bga.gn_act_conv(torch.randn(2, 4, 4, 64, device="cuda"), nn.GroupNorm(32, 64).cuda(), nn.Conv2d(64, 128, 3, padding=1).cuda())
