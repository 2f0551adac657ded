"""The resampling convolutions in training on the device (csrc/conv_train.hip: bg_conv_wgrad_geom, bg_conv_down_dgrad,
bg_conv_weight_pack_down, bg_pool2x2_sum; brepgen_amd/conv.py: conv_down, conv_up, DeviceBlock2D) against fp64 evaluated from the same
operands on the device.  The yardsticks are the project's: Parity.within_2x (tests/train_check.py) -- pooled max and mean absolute error
<= 2 x the errors of stock torch computing the same thing under the same autocast dtype -- and, for an fp32 weight gradient, the derived
bound of tests/test_gpu_conv_train.py, |dw - ref| <= (M + split + 2) 2^-24 sum |dy| |a| with M = S*Ho*Wo.

BG_RESAMPLE_PARITY_JSON=<path> makes the run write the measured pairs there (profiles/r19/conv_resample_parity.json is such a run)."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

import brepgen_amd as bga
from brepgen_amd import conv as CV
from brepgen_amd.vae import _DownBlock2D, _UpBlock2D
from tests import conv_ops
from tests import resample_ops as ops
from tests import resample_restate as R
from tests.conv_restate import pack_fwd
from tests.guarded import guarded, strided_input
from tests.train_check import Parity, errs, same_bits

pytestmark = pytest.mark.gpu
DTYPES = (torch.float16, torch.bfloat16)
NAME = ops.NAME
U24 = 2.0 ** -24
DOWN, UP = R.DOWN, R.UP
GEOM = {DOWN: "down2", UP: "up2"}
PARITY = Parity("BG_RESAMPLE_PARITY_JSON")
record, within_2x, _parity_json = PARITY.record, PARITY.within_2x, PARITY.fixture()
by_name = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])


def nchw(t):
    return t.permute(0, 3, 1, 2)


def cl(t):
    return t.permute(0, 2, 3, 1)


def huge_of(dtype):
    return 3.0e4 if dtype == torch.float16 else 1.0e30


# ---------------------------------------------------------------------------------------------------------------------------------
# bg_conv_wgrad_geom
# ---------------------------------------------------------------------------------------------------------------------------------
# (S, H, W, N, C, geom), H x W the grid of a
WGRAD_CASES = [(1, 2, 2, 128, 128, DOWN), (3, 4, 4, 128, 256, DOWN), (2, 8, 8, 256, 128, DOWN), (2, 2, 8, 128, 128, DOWN),
               (1, 1, 1, 128, 128, UP), (3, 2, 2, 128, 256, UP), (2, 4, 4, 256, 128, UP), (2, 1, 4, 128, 128, UP)]
case_id = lambda s: "x".join(map(str, s[:5])) + "-" + GEOM[s[5]]


def rows_of(shape):
    S, H, W, _, _, geom = shape
    Ho, Wo = R.out_grid(H, W, geom)
    return S * Ho * Wo


@functools.lru_cache(maxsize=None)
def wcase(shape, dtype):
    """inputs, the fp64 reference and torch's weight / bias gradient of the geometry's torch expression in the 16-bit dtype -- computed once"""
    S, H, W, N, C, geom = shape
    dy, a = ops.draw(*shape, dtype, 1000 * S + H * W + N + geom)
    ref_w, ref_b = R.wgrad(dy.double(), a.double(), geom)
    abs_w, abs_b = R.wgrad(dy.double(), a.double(), geom, absolute=True)
    w = torch.zeros(N, C, 3, 3, dtype=dtype, device="cuda", requires_grad=True)
    b = torch.zeros(N, dtype=dtype, device="cuda", requires_grad=True)
    ops.torch_fwd(nchw(a), w, b, geom).backward(nchw(dy))
    return dy, a, ref_w, ref_b, abs_w, abs_b, errs(pack_fwd(w.grad), ref_w), errs(b.grad, ref_b)


def check_bound_a(dw, db, M, S, ref_w, ref_b, abs_w, abs_b, what):
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), what
    f = (M + S + 2) * U24
    ew, eb = (dw.double() - ref_w).abs(), (db.double() - ref_b).abs()
    assert bool((ew <= f * abs_w).all()), (what, "dw", float((ew / (f * abs_w).clamp_min(1e-300)).max()))
    assert bool((eb <= f * abs_b).all()), (what, "db", float((eb / (f * abs_b).clamp_min(1e-300)).max()))


@by_name
@pytest.mark.parametrize("shape", WGRAD_CASES, ids=case_id)
def test_wgrad_geom_accuracy(shape, dtype):
    dy, a, ref_w, ref_b, abs_w, abs_b, tw, tb = wcase(shape, dtype)
    M = rows_of(shape)
    for split in (1, 3, 0):
        sp = split or ops.auto_split(*shape)
        for odt in (torch.float32, dtype):
            tag = f"conv_wgrad_geom {case_id(shape)} {NAME[dtype]}->{NAME[odt]} split={split}(S={sp})"
            dw, db = ops.wgrad(dy, a, *shape, odt, split)
            if odt == torch.float32:
                check_bound_a(dw, db, M, sp, ref_w, ref_b, abs_w, abs_b, tag)
            record(tag, "db", errs(db, ref_b), tb)
            within_2x(tag, "dw", errs(dw, ref_w), tw)


@by_name
@pytest.mark.parametrize("shape", [(2, 8, 8, 256, 128, DOWN), (2, 4, 4, 256, 128, UP)], ids=case_id)
def test_wgrad_geom_bits(shape, dtype):
    S, H, W, N, C, geom = shape
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
    dy3[1, 1, 2, n0] = float("inf")
    for split in (1, 3):
        for odt in (torch.float32, dtype):
            dw, db = ops.wgrad(dy3, a, *shape, odt, split)
            assert not bool(torch.isfinite(dw[n0]).any()) and not bool(torch.isfinite(db[n0]))
            assert bool(torch.isfinite(dw[others]).all()) and bool(torch.isfinite(db[others]).all())


@by_name
def test_wgrad_geom_same_is_bg_conv_wgrad(dtype):
    S, H, W, N, C = 2, 8, 8, 256, 128
    dy, a = conv_ops.draw(S, H, W, N, C, dtype, 5)
    for split in (1, 3, 0):
        for odt in (torch.float32, dtype):
            p, q = conv_ops.wgrad(dy, a, S, H, W, N, C, 3, 3, odt, split), ops.wgrad(dy, a, S, H, W, N, C, 0, odt, split)
            assert same_bits(p[0], q[0]) and same_bits(p[1], q[1]), (split, odt)
    dy, a = conv_ops.draw(3, 1, 8, 128, 128, dtype, 6)                                     # its other windows too
    p, q = conv_ops.wgrad(dy, a, 3, 1, 8, 128, 128, 1, 5), ops.wgrad(dy, a, 3, 1, 8, 128, 128, 0, kh=1, kw=5)
    assert same_bits(p[0], q[0]) and same_bits(p[1], q[1])


@by_name
@pytest.mark.parametrize("S, H, W, geom, split", [(1, 2, 2, DOWN, 1), (1, 2, 2, DOWN, 3), (3, 4, 4, DOWN, 0), (2, 8, 8, DOWN, 1), (2, 8, 8, DOWN, 3),
                                                  (1, 1, 1, UP, 1), (1, 1, 1, UP, 3), (3, 2, 2, UP, 0), (2, 4, 4, UP, 1), (2, 4, 4, UP, 3)])
def test_wgrad_geom_guarded(S, H, W, geom, split, dtype):
    """pixel strides > channels, NaN-sentinel padding and guard bands around dy / a: a padding column or a pixel outside the tensors in any
    product makes the result NaN.  dw / db: every promised element written, nothing outside."""
    N, C = 256, 128
    shape = (S, H, W, N, C, geom)
    dy, a, ref_w, ref_b, abs_w, abs_b = wcase(shape, dtype)[:6]
    M = rows_of(shape)
    dys, a_s = strided_input(dy.reshape(M, N), N + 8), strided_input(a.reshape(S * H * W, C), C + 24)
    sp = split or ops.auto_split(*shape)
    for odt in (torch.float32, dtype):
        gw, gb = guarded((N, 9 * C), odt, "cuda"), guarded((N,), odt, "cuda")
        ops.wgrad(dys, a_s, *shape, odt, split, ld_dy=N + 8, ld_a=C + 24, dw=gw.view, db=gb.view)
        for g, what in ((gw, "dw"), (gb, "db")):
            g.assert_untouched(what)
            g.assert_fully_written(what)
        if odt == torch.float32:
            check_bound_a(gw.view.clone(), gb.view.reshape(N).clone(), M, sp, ref_w, ref_b, abs_w, abs_b, f"guarded {case_id(shape)} split={split}")
    gb = guarded((N,), torch.float32, "cuda")                                  # no bias requested: db is not touched
    dw, _ = ops.wgrad(dys, a_s, *shape, torch.float32, split, bias=False, ld_dy=N + 8, ld_a=C + 24)
    gb.assert_untouched("db (NULL)")
    assert bool(((dw.double() - ref_w).abs() <= (M + sp + 2) * U24 * abs_w).all())


@by_name
@pytest.mark.parametrize("H, W, geom", [(2, 2, DOWN), (4, 4, DOWN), (1, 1, UP), (2, 2, UP)])
def test_wgrad_geom_border_taps_do_not_read_the_neighbours(H, W, geom, dtype):
    """samples 0 and 2 hold a huge finite `a` and a zero dy: they contribute exactly zero, unless a padded tap of sample 1 reads the
    next grid row or sample, or an up-sampling tap at uy = -1 lands on row -1 >> 1 = -1 (the sample before) or (-1) / 2 = 0"""
    S, N, C = 3, 128, 128
    shape = (S, H, W, N, C, geom)
    dy, a = ops.draw(*shape, dtype, 42)
    a[0], a[2] = huge_of(dtype), -huge_of(dtype)
    dy[0], dy[2] = 0, 0
    ref_w, ref_b = R.wgrad(dy[1:2].double(), a[1:2].double(), geom)
    abs_w, abs_b = R.wgrad(dy[1:2].double(), a[1:2].double(), geom, absolute=True)
    for split in (1, 3):
        dw, db = ops.wgrad(dy, a, *shape, torch.float32, split)
        check_bound_a(dw, db, rows_of(shape), split, ref_w, ref_b, abs_w, abs_b, f"neighbour {H}x{W} {GEOM[geom]} split={split}")


# ---------------------------------------------------------------------------------------------------------------------------------
# bg_conv_weight_pack_down and bg_conv_down_dgrad
# ---------------------------------------------------------------------------------------------------------------------------------
@by_name
@pytest.mark.parametrize("N, C", [(128, 128), (256, 128), (32, 64)])
def test_pack_down_bits(N, C, dtype):
    g = torch.Generator(device="cpu").manual_seed(N + C)
    w32 = torch.randn(N, C, 3, 3, generator=g).cuda()
    for src in (w32, w32.to(dtype)):
        want_f, want_d = pack_fwd(src).to(dtype).contiguous(), R.pack_down(src).to(dtype).contiguous()
        gf, gd = guarded((N, 9 * C), dtype, "cuda"), guarded((9 * C * N,), dtype, "cuda")
        ops.pack_down(src, dtype, fwd=True, out_f=gf.view, out_d=gd.view.reshape(-1))
        for gq, what in ((gf, "fwd"), (gd, "down")):
            gq.assert_untouched(what)
            gq.assert_fully_written(what)
        assert same_bits(gf.view.clone(), want_f) and same_bits(gd.view.reshape(-1).clone(), want_d)
        none_f, only_d = ops.pack_down(src, dtype)
        only_f, none_d = ops.pack_down(src, dtype, fwd=True, down=False)
        assert none_f is None and none_d is None and same_bits(only_d, want_d) and same_bits(only_f, want_f)


DGRAD_CASES = [(2, 4, 4, 128, 256), (3, 2, 2, 128, 128), (4, 32, 32, 128, 128)]


@by_name
@pytest.mark.parametrize("S, H, W, N, C", DGRAD_CASES, ids=lambda v: str(v))
def test_down_dgrad(S, H, W, N, C, dtype):
    Ho, Wo = H // 2, W // 2
    g = torch.Generator(device="cpu").manual_seed(S * H + C)
    dy = torch.randn(S, Ho, Wo, N, generator=g).to(dtype).cuda()
    w = (torch.randn(N, C, 3, 3, generator=g) / (9 * N) ** 0.5).to(dtype).cuda()
    ref = R.down_dgrad(dy.double(), R.pack_down(w.double()), C)
    x = torch.zeros(S, C, H, W, dtype=dtype, device="cuda", requires_grad=True)
    ops.torch_fwd(x, w, None, DOWN).backward(nchw(dy))
    pack = ops.pack_down(w, dtype)[1]
    dys = strided_input(dy.reshape(-1, N), N + 8)                              # a pixel stride > N, NaN padding
    gx = guarded((S * H * W, C), torch.float32, "cuda")
    ops.down_dgrad(dys, pack, S, H, W, N, C, dx=gx.view, ld_dy=N + 8)
    gx.assert_untouched("dx")
    gx.assert_fully_written("dx")
    dx = gx.view.clone().view(S, H, W, C)
    within_2x(f"conv_down_dgrad {S}x{H}x{W} {N}->{C} {NAME[dtype]}", "dx", errs(dx, ref), errs(cl(x.grad), ref))
    again = ops.down_dgrad(dy.reshape(-1, N), pack, S, H, W, N, C)            # dense dy, a second call: the same bits
    assert same_bits(again.view(S, H, W, C), dx)


@by_name
@pytest.mark.parametrize("H, W", [(2, 2), (4, 4), (4, 8)])
def test_down_dgrad_neighbours_contribute_exactly_zero(H, W, dtype):
    """a sample with a zero dy between two samples with a huge one has dx == 0 exactly; inside a sample, input pixel (0, 0) meets dy pixel
    (0, 0) alone -- not the last pixel of the row or the sample before it"""
    S, N, C = 3, 128, 128
    Ho, Wo = H // 2, W // 2
    g = torch.Generator(device="cpu").manual_seed(H * W)
    w = (torch.randn(N, C, 3, 3, generator=g) / (9 * N) ** 0.5).to(dtype).cuda()
    pack = ops.pack_down(w, dtype)[1]
    dy = torch.full((S, Ho, Wo, N), huge_of(dtype)).to(dtype).cuda()
    dy[1] = 0
    dx = ops.down_dgrad(dy.reshape(-1, N), pack, S, H, W, N, C).view(S, H, W, C)
    assert bool((dx[1] == 0).all()) and bool(torch.isfinite(dx).all()) and bool((dx[0] != 0).any())
    dy[:, 0, 0] = 0                                                           # every sample: pixel (0, 0) zero, the rest huge
    dx = ops.down_dgrad(dy.reshape(-1, N), pack, S, H, W, N, C).view(S, H, W, C)
    assert bool((dx[0, 0, 0] == 0).all()) and bool((dx[2, 0, 0] == 0).all()) and bool((dx[:, 1, 1] == 0).all())
    # odd input pixels (1, 1) meet tap (1, 1) at dy (0, 0) alone; even ones past the first meet their predecessors too
    assert Wo == 1 or bool((dx[0, 0, 2] != 0).any())


# ---------------------------------------------------------------------------------------------------------------------------------
# bg_pool2x2_sum
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S, H, W, C", [(1, 1, 1, 4), (3, 2, 4, 128), (2, 16, 16, 256)])
def test_pool2x2_sum_bits(S, H, W, C):
    g = torch.Generator(device="cpu").manual_seed(S + H + C)
    u = torch.randn(S, 2 * H, 2 * W, C, generator=g).cuda()
    add = torch.randn(S, H, W, C, generator=g).cuda()
    for ad in (None, add):
        gy = guarded((S * H * W, C), torch.float32, "cuda")
        ops.pool(u, S, H, W, C, add=ad, y=gy.view)
        gy.assert_untouched("y")
        gy.assert_fully_written("y")
        assert same_bits(gy.view.clone().view(S, H, W, C), R.pool2x2(u, ad))   # fp32, the same association: the same bits


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_down / conv_up, the modules and the blocks
# ---------------------------------------------------------------------------------------------------------------------------------
class Sampler(nn.Module):
    """diffusers' Downsample2D / Upsample2D from stock modules, NCHW"""

    def __init__(self, cin, cout, geom):
        super().__init__()
        self.geom = geom
        self.conv = nn.Conv2d(cin, cout, 3, stride=2) if geom == DOWN else nn.Conv2d(cin, cout, 3, padding=1)

    def forward(self, x):
        return ops.torch_fwd(x, self.conv.weight, self.conv.bias, self.geom)


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


def three_ways(ref32, dev, x, g, scale, dtype, ours_run=None):
    """(ours, torch under autocast, fp64) of the NCHW module ref32 and its channels-last device twin"""
    def autocast(m, t):
        with torch.autocast("cuda", dtype=dtype):
            return m(t)

    ref = grads_of(copy.deepcopy(ref32).double(), x.double(), g, 1.0, lambda m, t: m(t))
    tor = grads_of(ref32, x, g, scale, autocast)
    ours = grads_of(dev, cl(x).contiguous(), cl(g).contiguous(), scale, ours_run or autocast)
    return ours, tor, ref


def sampler_case(S, H, W, cin, cout, geom, scale, dtype):
    gen = torch.Generator(device="cpu").manual_seed(cin + cout + H + geom)
    torch.manual_seed(cin + cout + H + geom)
    ref32 = Sampler(cin, cout, geom).cuda()
    dev = copy.deepcopy(ref32)
    Ho, Wo = R.out_grid(H, W, geom)
    x = torch.randn(S, cin, H, W, generator=gen).cuda()
    g = (torch.randn(S, cout, Ho, Wo, generator=gen) * 1e-3).double().cuda()

    def ours_run(m, t):
        with torch.autocast("cuda", dtype=dtype):
            return (bga.conv_down if geom == DOWN else bga.conv_up)(t, m.conv)

    ours, tor, ref = three_ways(ref32, dev, x, g, scale, dtype, ours_run)
    assert ours[0].dtype == torch.float32 and ours[0].shape == (S, Ho, Wo, cout) and ours[1].shape == (S, H, W, cin)
    assert all(p.grad.dtype == torch.float32 and p.grad.shape == p.shape for p in dev.parameters())
    compare(f"conv_{GEOM[geom]} {cin}->{cout} {S}x{H}x{W} {NAME[dtype]} scale={scale:g}", ours, tor, ref, nchw)


@by_name
@pytest.mark.parametrize("S, H, W, C, implicit", [(2, 2, 2, 128, False), (4, 16, 16, 256, True)])
def test_conv_up_forward_paths(S, H, W, C, implicit, dtype):
    """im2col + GEMM at (2, 2, 2); at (4, 16, 16) x 256 channels the 32 x 32 grid gives 64 tiles: the forward (up = 1) and the
    data gradient's 'same' convolution both take the implicit GEMM"""
    assert CV._implicit_ok(S, 2 * H, 2 * W, C, C, 9) is implicit
    sampler_case(S, H, W, C, C, UP, 1.0, dtype)


@by_name
@pytest.mark.parametrize("scale", [1.0, 65536.0], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("S, H, W, C, geom", [(3, 8, 8, 128, DOWN), (3, 4, 4, 256, DOWN), (3, 4, 4, 128, UP), (3, 2, 2, 256, UP)],
                         ids=lambda v: str(v))
def test_autograd_ops(S, H, W, C, geom, scale, dtype):
    sampler_case(S, H, W, C, C, geom, scale, dtype)


class RefResnet(nn.Module):
    """diffusers' ResnetBlock2D without a time embedding (dropout 0, output scale 1), NCHW, from stock modules"""

    def __init__(self, cin, cout, groups=32):
        super().__init__()
        self.norm1, self.conv1 = nn.GroupNorm(groups, cin, eps=1e-6), nn.Conv2d(cin, cout, 3, padding=1)
        self.norm2, self.conv2 = nn.GroupNorm(groups, cout, eps=1e-6), nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)

    def forward(self, x):
        h = self.conv1(nn.functional.silu(self.norm1(x)))
        h = self.conv2(nn.functional.silu(self.norm2(h)))
        return (self.conv_shortcut(x) if hasattr(self, "conv_shortcut") else x) + h


class RefBlock2D(nn.Module):
    """DownEncoderBlock2D / UpDecoderBlock2D with vae._DownBlock2D's / _UpBlock2D's keys, NCHW, from stock modules"""

    def __init__(self, cin, cout, n, geom):
        super().__init__()
        self.resnets = nn.ModuleList([RefResnet(cin if i == 0 else cout, cout) for i in range(n)])
        setattr(self, "downsamplers" if geom == DOWN else "upsamplers", nn.ModuleList([Sampler(cout, cout, geom)]))

    def forward(self, x):
        for m in list(self.resnets) + list(getattr(self, "downsamplers", [])) + list(getattr(self, "upsamplers", [])):
            x = m(x)
        return x


@by_name
@pytest.mark.parametrize("geom", [DOWN, UP], ids=lambda v: GEOM[v])
def test_blocks(geom, dtype):
    S = 3
    cin, cout, n, hw = (128, 256, 2, 8) if geom == DOWN else (256, 128, 3, 4)
    gen = torch.Generator(device="cpu").manual_seed(cin + hw)
    torch.manual_seed(cin + hw)
    ref32 = RefBlock2D(cin, cout, n, geom)
    with torch.no_grad():
        for q in ref32.modules():
            if isinstance(q, nn.GroupNorm):
                q.weight.add_(0.1 * torch.randn(q.weight.shape, generator=gen)), q.bias.add_(0.1 * torch.randn(q.bias.shape, generator=gen))
    ref32 = ref32.cuda()
    holder = (_DownBlock2D(cin, cout, n, 32, True) if geom == DOWN else _UpBlock2D(cin, cout, n, 32, True)).cuda()
    keys = list(holder.state_dict())
    assert keys == list(ref32.state_dict())
    holder.load_state_dict(ref32.state_dict())
    dev = bga.use_device_blocks(holder)
    assert isinstance(dev, CV.DeviceBlock2D) and list(dev.state_dict()) == keys
    Ho, Wo = R.out_grid(hw, hw, geom)
    x = torch.randn(S, cin, hw, hw, generator=gen).cuda()
    g = (torch.randn(S, cout, Ho, Wo, generator=gen) * 1e-3).double().cuda()
    ours, tor, ref = three_ways(ref32, dev, x, g, 1.0, dtype)
    assert ours[0].dtype == torch.float32 and ours[0].shape == (S, Ho, Wo, cout)
    assert all(p.grad.dtype == torch.float32 for p in dev.parameters())
    compare(f"block {GEOM[geom]} {cin}->{cout} x{n} {S}x{hw}x{hw} {NAME[dtype]}", ours, tor, ref, nchw)
    # outside the rules: raises, no fallback
    with pytest.raises(ValueError, match="autocast"):
        dev(cl(x).contiguous())
    with torch.autocast("cuda", dtype=dtype):
        with pytest.raises(ValueError, match="powers of two"):
            dev(torch.randn(S, 6, 4, cin, device="cuda"))
