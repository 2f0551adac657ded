"""The trainer update on the device (brepgen_amd/optim.py, csrc/optim.hip) against its numpy restatement (tests/optim_restate.py):
parameters, moments, scale, tracker, step counter and norm bit for bit; guard bands, padding and gradients untouched.  Parameters and
moments live in tests/guarded.py buffers; the whole file stays under a million elements.
"""
import numpy as np
import pytest
import torch

import brepgen_amd as bga
from brepgen_amd import optim
from tests import optim_restate as R
from tests.guarded import guarded

pytestmark = pytest.mark.gpu

C = optim.CHUNK
# numel 0 .. 5 and around 1024: the 16-byte path's tails; around CHUNK: the chunk list's; [768, 48]: nine full chunks
SHAPES = [(0,), (1,), (3,), (4,), (5,), (1023,), (1024,), (1025,), (C - 1,), (C,), (C + 1,), (2 * C + 7,), (768, 48), (1027,), (9,), (2051,)]
MISALIGNED_P, NO_GRAD, MISALIGNED_G = 13, 14, 15      # a view 4 bytes into its storage; .grad is None; a gradient 4 bytes into its storage
LDM = dict(lr=5e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-6)
VAE = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
SIGMA = (0.05, 1.0, 0.1, 2.0, 0.02, 0.5, 0.1, 3.0)      # norm ~ 250 sigma over 62 k elements: clipped at 50 iff sigma > 0.2


def bits(t):
    return t.detach().cpu().contiguous().numpy().reshape(-1).view(np.int32)


def same_bits(t, a):
    return np.array_equal(bits(t), np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.int32))


def make_grads(rng, sigma, shapes=SHAPES, no_grad=(NO_GRAD,)):
    return [None if i in no_grad else (rng.standard_normal(s) * sigma).astype(np.float32) for i, s in enumerate(shapes)]


class Rig:
    """The tensor set on the device (p, exp_avg, exp_avg_sq in guarded buffers), an AdamW + GradScaler over it, and the restatement."""

    def __init__(self, hyper=LDM, seed=0, groups=None, shapes=SHAPES, misaligned=(MISALIGNED_P,), scaler=None, **scaler_kw):
        rng = np.random.default_rng(seed)
        self.shapes, self.host_p = shapes, [rng.standard_normal(s).astype(np.float32) for s in shapes]
        self.bufs, self.params, self.moments = [], [], []
        for i, (s, hp) in enumerate(zip(shapes, self.host_p)):
            off = 1 if i in misaligned else 0
            trio = []
            for k in range(3):
                lead, n = s[:-1], s[-1]
                buf = guarded(lead + (n + off,), torch.float32, "cuda") if not off else guarded(n + off, torch.float32, "cuda")
                t = buf.view.reshape(-1)[off:].reshape(s)
                assert t.is_contiguous() and t.data_ptr() % 16 == 4 * off
                t.copy_(torch.from_numpy(hp)) if k == 0 else t.zero_()
                self.bufs.append((buf, off))
                trio.append(t)
            self.params.append(trio[0])
            self.moments.append(trio[1:])
        spec = self.params if groups is None else [dict(params=[self.params[i] for i in idx], lr=lr, weight_decay=wd) for idx, lr, wd in groups]
        self.opt = optim.AdamW(spec, **hyper)
        for p, (m, v) in zip(self.params, self.moments):
            self.opt.state[p] = {"exp_avg": m, "exp_avg_sq": v}
        self.scaler = optim.GradScaler(**scaler_kw) if scaler is None else scaler
        sk = {"scale": scaler_kw.get("init_scale", 65536.0), **{k: v for k, v in scaler_kw.items() if k != "init_scale"}}
        self.r = R.Trainer(self.host_p, groups=groups, **hyper, **sk)
        torch.cuda.synchronize()

    def set_grads(self, grads):
        self.dev_grads = []
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                p.grad = None
            elif i == MISALIGNED_G and len(self.shapes) > MISALIGNED_G:
                store = torch.zeros(g.size + 1, dtype=torch.float32, device="cuda")
                p.grad = store[1:].reshape(g.shape)
                p.grad.copy_(torch.from_numpy(g))
                assert p.grad.data_ptr() % 16 == 4
            else:
                p.grad = torch.from_numpy(g).cuda()
            self.dev_grads.append(p.grad)

    def update(self, grads, max_norm=None):
        self.set_grads(grads)
        self.scaler.step(self.opt, max_norm=max_norm)
        self.scaler.update()
        self.r.update(grads, max_norm)

    def check(self, grads=None, what=""):
        for i, (p, (m, v)) in enumerate(zip(self.params, self.moments)):
            for name, t, a in (("p", p, self.r.p[i]), ("exp_avg", m, self.r.m[i]), ("exp_avg_sq", v, self.r.v[i])):
                if not same_bits(t, a):
                    bad = np.nonzero(bits(t) != a.reshape(-1).view(np.int32))[0]
                    raise AssertionError(f"{what}: {name} of tensor {i} {self.shapes[i]}: {bad.size} elements differ, first at {bad[0]}: "
                                         f"{t.reshape(-1)[int(bad[0])].item()!r} vs {a.reshape(-1)[bad[0]]!r}")
        for buf, off in self.bufs:
            buf.assert_untouched(what)
            if off:
                assert not bool(buf.written_mask()[0, 0]), f"{what}: the element before a misaligned view was written"
        if grads is not None:
            for g, d in zip(grads, self.dev_grads):
                assert (g is None and d is None) or same_bits(d, g), f"{what}: a gradient was written"
        info, sc = self.opt.last_step_info(), self.scaler.state_dict()
        assert info["step"] == self.r.step and info["found_inf"] == self.r.found_inf, (what, info, self.r.step, self.r.found_inf)
        assert np.float32(sc["scale"]) == self.r.scale and sc["_growth_tracker"] == self.r.growth_tracker, (what, sc, self.r.scale)
        if not self.r.found_inf:
            assert np.float32(info["total_norm"]).view(np.int32) == np.float32(self.r.total_norm).view(np.int32), (what, info, self.r.total_norm)


def test_trajectory_bit_for_bit():
    """8 steps, growth_interval 2, max_norm 50 (clipped on the steps with sigma > 0.2): an inf at step 2 in the LAST chunk of the
    [768, 48] matrix -- every tensor before it, and every other chunk, is clean --, a NaN at step 5 in the one-element tensor."""
    rig = Rig(LDM, seed=1, growth_interval=2)
    rng = np.random.default_rng(11)
    clipped, scales = [], []
    for k, sigma in enumerate(SIGMA):
        grads = make_grads(rng, sigma)
        if k == 2:
            grads[12][767, 40] = np.inf
        if k == 5:
            grads[1][0] = np.nan
        before = [[bits(t) for t in (p, m, v)] for p, (m, v) in zip(rig.params, rig.moments)]
        rig.update(grads, max_norm=50.0)
        rig.check(grads, f"step {k}")
        after = [[bits(t) for t in (p, m, v)] for p, (m, v) in zip(rig.params, rig.moments)]
        unchanged = [all(np.array_equal(x, y) for x, y in zip(a, b)) for a, b in zip(before, after)]
        if k in (2, 5):
            assert rig.r.found_inf and all(unchanged), k
        else:
            assert not rig.r.found_inf and not any(u for u, s in zip(unchanged, SHAPES) if s != (0,) and s != SHAPES[NO_GRAD]), k
            clipped.append(bool(rig.r.total_norm > 50.0))
        assert unchanged[NO_GRAD]
        scales.append(float(rig.r.scale))
    assert True in clipped and False in clipped
    assert scales[:3] == [65536.0, 131072.0, 65536.0] and scales[-1] == 131072.0 and rig.r.step == 6      # grew, backed off, grew again


def test_norm_within_an_ulp_and_reproducible():
    rng = np.random.default_rng(3)
    grads = make_grads(rng, 0.7)
    rig = Rig(seed=2)
    exact = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads if g is not None))
    want = R.verdict([g for g in grads if g is not None], 1e30)
    norms = []
    for _ in range(2):
        rig.set_grads(grads)
        norms.append(optim.clip_grad_norm_(rig.params, 1e30))          # c = 1: the gradients keep their bits
    a, b = (np.float32(n.item()) for n in norms)
    assert norms[0].shape == () and norms[0].is_cuda and a.view(np.int32) == b.view(np.int32) == want[0].view(np.int32)
    assert abs(float(a) - exact) <= float(np.spacing(np.float32(exact))), (a, exact)
    for g, d in zip(grads, rig.dev_grads):
        assert g is None or same_bits(d, g)
    norm = optim.clip_grad_norm_(rig.params, 5.0)                      # clipped: g * c, one rounding
    c = R.verdict([g for g in grads if g is not None], 5.0)[1]
    assert c < 1 and np.float32(norm.item()).view(np.int32) == a.view(np.int32)
    for g, d in zip(grads, rig.dev_grads):
        assert g is None or same_bits(d, g * c)


def test_overflow_through_unscaling_skips_the_step():
    """No clipping, scale 2^-10, one gradient of 1e36: every input is finite, 1e36 * 2^10 is not -- the step is skipped, the scale halved."""
    rig = Rig(seed=3, init_scale=2.0 ** -10)
    grads = make_grads(np.random.default_rng(4), 1.0)
    grads[11][C + 5] = 1e36
    before = [bits(p) for p in rig.params]
    rig.update(grads, max_norm=None)
    rig.check(grads, "overflow")
    assert rig.r.found_inf and rig.scaler.get_scale() == 2.0 ** -11 and rig.opt.last_step_info()["step"] == 0
    assert all(np.array_equal(a, bits(p)) for a, p in zip(before, rig.params))
    grads[11][C + 5] = 1e10                                            # finite after unscaling: the next step runs
    rig.update(grads, max_norm=None)
    rig.check(grads, "after overflow")
    assert not rig.r.found_inf and rig.opt.last_step_info()["step"] == 1


def test_fused_step_equals_the_reference_four_lines():
    fused, literal = Rig(seed=5, growth_interval=2), Rig(seed=5, growth_interval=2)
    rng = np.random.default_rng(6)
    for k, sigma in enumerate((1.0, 0.05, 2.0)):
        grads = make_grads(rng, sigma)
        fused.update(grads, max_norm=50.0)
        literal.set_grads(grads)
        norm = optim.clip_grad_norm_(literal.params, 50.0)
        literal.scaler.step(literal.opt)
        literal.scaler.update()
        for i in range(len(SHAPES)):
            for a, b in zip((fused.params[i], *fused.moments[i]), (literal.params[i], *literal.moments[i])):
                assert np.array_equal(bits(a), bits(b)), (k, i)
        assert np.float32(norm.item()) == fused.r.total_norm and fused.scaler.get_scale() == literal.scaler.get_scale()
        fused.check(grads, f"fused {k}")
    for buf, _ in literal.bufs:
        buf.assert_untouched("literal")


SMALL = [(5,), (1025,), (C + 1,), (37, 48)]


@pytest.mark.parametrize("case", ["ldm", "vae", "no_decay", "two_groups", "lr_schedule"])
def test_hyper_parameters(case):
    hyper, max_norm, groups = LDM, 50.0, None
    if case == "vae":
        hyper, max_norm = VAE, 5.0
    elif case == "no_decay":
        hyper = dict(LDM, weight_decay=0.0)
    elif case == "two_groups":
        groups = [([0, 2], 5e-4, 1e-6), ([1, 3], 1e-3, 0.0)]
    rig = Rig(hyper, seed=7, groups=groups, shapes=SMALL, misaligned=(1,))
    rng = np.random.default_rng(8)
    for k, sigma in enumerate((0.5, 0.01, 0.3)):
        if case == "lr_schedule" and k > 0:
            rig.opt.param_groups[0]["lr"] = rig.r.groups[0][1] = 5e-4 * (1.0 - 0.3 * k)
        grads = make_grads(rng, sigma, SMALL, ())
        rig.update(grads, max_norm=max_norm)
        rig.check(grads, f"{case} step {k}")
    assert rig.r.step == 3
    if case == "lr_schedule":                      # the schedule is seen: a fixed lr gives other bits
        fixed = Rig(hyper, seed=7, shapes=SMALL, misaligned=(1,))
        rng = np.random.default_rng(8)
        for sigma in (0.5, 0.01, 0.3):
            fixed.update(make_grads(rng, sigma, SMALL, ()), max_norm=max_norm)
        assert not np.array_equal(bits(fixed.params[2]), bits(rig.params[2]))


def test_step_without_a_scaler():
    """AdamW.step(): r = 1, no clipping, a NaN still skips; the counter advances on the good steps only."""
    rig = Rig(VAE, seed=9, shapes=SMALL, misaligned=(1,))
    rig.r.scale = None
    rng = np.random.default_rng(10)
    for k in range(3):
        grads = make_grads(rng, 0.1, SMALL, ())
        if k == 1:
            grads[3][36, 47] = np.nan
        rig.set_grads(grads)
        rig.opt.step()
        rig.r.update(grads, None)
        for i in range(len(SMALL)):
            assert same_bits(rig.params[i], rig.r.p[i]) and same_bits(rig.moments[i][0], rig.r.m[i]) and same_bits(rig.moments[i][1], rig.r.v[i]), (k, i)
        info = rig.opt.last_step_info()
        assert info["step"] == rig.r.step and info["found_inf"] == (k == 1)
    rig.opt.zero_grad()
    assert all(p.grad is None for p in rig.params)
    rig.opt.step()                                 # no gradient anywhere: nothing happens
    assert rig.opt.last_step_info()["step"] == 2


def test_state_round_trip():
    """3 steps, state_dict() into a fresh AdamW + GradScaler, 2 more steps == 5 uninterrupted steps, bit for bit; the same state in
    torch.optim.AdamW on the CPU, continued with torch's own clip / scaler, stays as close to the fp64 twin as tests/test_optim_cpu.py
    asks of the restatement: the device's error at most 2 x torch's own."""
    rng = np.random.default_rng(12)
    all_grads = [make_grads(rng, s, SMALL, ()) for s in (0.5, 0.02, 1.0, 0.3, 0.05)]
    whole = Rig(LDM, seed=13, shapes=SMALL, misaligned=(1,), growth_interval=2)
    for g in all_grads:
        whole.update(g, max_norm=5.0)
    first = Rig(LDM, seed=13, shapes=SMALL, misaligned=(1,), growth_interval=2)
    for g in all_grads[:3]:
        first.update(g, max_norm=5.0)
    sd, ssd = first.opt.state_dict(), first.scaler.state_dict()
    assert all(float(st["step"]) == 3.0 for st in sd["state"].values()) and len(sd["state"]) == len(SMALL)
    second = Rig(dict(LDM, lr=1.0), seed=99, shapes=SMALL, misaligned=(1,))          # other values everywhere until the state is loaded
    for p, q in zip(second.params, first.params):
        p.copy_(q)
    second.opt.load_state_dict(sd)
    second.scaler.load_state_dict(ssd)
    for p, (m, v) in zip(second.params, second.moments):                              # the loaded moments, back in guarded buffers
        m.copy_(second.opt.state[p]["exp_avg"])
        v.copy_(second.opt.state[p]["exp_avg_sq"])
        second.opt.state[p] = {"exp_avg": m, "exp_avg_sq": v}
    # torch on the CPU and the fp64 twin start from the same state
    tp = [torch.nn.Parameter(p.detach().cpu().clone()) for p in first.params]
    topt = torch.optim.AdamW(tp, foreach=False)
    topt.load_state_dict(sd)
    assert all(st["exp_avg"].device.type == "cpu" for st in topt.state.values()) and topt.param_groups[0]["lr"] == LDM["lr"]
    tscaler = torch.amp.GradScaler("cpu")
    tscaler.load_state_dict(ssd)
    twin = R.Trainer([p.detach().cpu().numpy() for p in first.params], dtype=np.float64, scale=ssd["scale"], growth_interval=2, **LDM)
    twin.m = [m.cpu().numpy().astype(np.float64) for m, _ in first.moments]
    twin.v = [v.cpu().numpy().astype(np.float64) for _, v in first.moments]
    twin.step, twin.growth_tracker = 3, ssd["_growth_tracker"]
    twin.beta1_pow, twin.beta2_pow = R.beta_pow(LDM["betas"][0], 3), R.beta_pow(LDM["betas"][1], 3)
    for g in all_grads[3:]:
        second.set_grads(g)
        second.scaler.step(second.opt, max_norm=5.0)
        second.scaler.update()
        tscaler.scale(torch.zeros(()))
        for p, a in zip(tp, g):
            p.grad = torch.from_numpy(a.copy())
        torch.nn.utils.clip_grad_norm_(tp, max_norm=5.0)
        tscaler.step(topt)
        tscaler.update()
        twin.update(g, 5.0)
    for i in range(len(SMALL)):
        for a, b in zip((whole.params[i], *whole.moments[i]), (second.params[i], *second.moments[i])):
            assert np.array_equal(bits(a), bits(b)), i
    for buf, _ in second.bufs:
        buf.assert_untouched("resumed")
    assert second.scaler.state_dict() == whole.scaler.state_dict() and second.opt.last_step_info() == whole.opt.last_step_info()
    assert float(tscaler.get_scale()) == second.scaler.get_scale()
    for name, mine, theirs, ref in (("p", second.params, [p.detach() for p in tp], twin.p),
                                    ("exp_avg", [m for m, _ in second.moments], [topt.state[p]["exp_avg"] for p in tp], twin.m),
                                    ("exp_avg_sq", [v for _, v in second.moments], [topt.state[p]["exp_avg_sq"] for p in tp], twin.v)):
        e_mine = max(float(np.abs(a.cpu().numpy().astype(np.float64) - r).max()) for a, r in zip(mine, ref))
        e_torch = max(float(np.abs(a.cpu().numpy().astype(np.float64) - r).max()) for a, r in zip(theirs, ref))
        print(f"{name}: max |device - fp64 twin| = {e_mine:.3e}, max |torch CPU - fp64 twin| = {e_torch:.3e}")
        assert e_torch > 0.0 and e_mine <= 2.0 * e_torch, (name, e_mine, e_torch)


def test_more_chunks_than_workgroups():
    """2100 tensors of 1 .. 7 elements, 5 floats apart in one buffer (every alignment): more chunks than the 2048 workgroups of a launch,
    so some walk two; the gaps between the tensors stay as they were."""
    rng = np.random.default_rng(14)
    n_t, pitch = 2100, 13
    sizes = [1 + i % 7 for i in range(n_t)]
    flat = {k: torch.full((n_t * pitch,), float("nan"), device="cuda") for k in "pmv"}
    params, host_p = [], []
    opt_state = {}
    for i, n in enumerate(sizes):
        hp = rng.standard_normal(n).astype(np.float32)
        p, m, v = (flat[k][i * pitch:i * pitch + n] for k in "pmv")
        p.copy_(torch.from_numpy(hp))
        m.zero_()
        v.zero_()
        params.append(p)
        host_p.append(hp)
        opt_state[p] = {"exp_avg": m, "exp_avg_sq": v}
    opt = optim.AdamW(params, **LDM)
    opt.state.update(opt_state)
    scaler = optim.GradScaler()
    r = R.Trainer(host_p, **LDM)
    gflat = torch.from_numpy((rng.standard_normal(n_t * pitch) * 3.0).astype(np.float32)).cuda()
    grads = []
    for i, (p, n) in enumerate(zip(params, sizes)):
        p.grad = gflat[i * pitch + 2:i * pitch + 2 + n]
        grads.append(p.grad.cpu().numpy())
    assert len(R.chunk_list(sizes)) == n_t > optim.MAX_BLOCKS
    scaler.step(opt, max_norm=50.0)
    scaler.update()
    r.update(grads, 50.0)
    assert r.total_norm > 50.0 and not r.found_inf
    got = {k: flat[k].cpu().numpy().reshape(n_t, pitch) for k in "pmv"}
    for k, want in (("p", r.p), ("m", r.m), ("v", r.v)):
        for i, n in enumerate(sizes):
            assert np.array_equal(got[k][i, :n].view(np.int32), want[i].view(np.int32)), (k, i)
            assert np.isnan(got[k][i, n:]).all(), (k, i)
    info = opt.last_step_info()
    assert info["step"] == 1 and np.float32(info["total_norm"]) == r.total_norm


def test_owners_are_invalidated():
    """SurfPosNet caches packed copies of its parameters: with owners=(net,) the next forward sees the step, and equals -- bit for bit --
    a fresh module loaded with the updated state_dict."""
    torch.manual_seed(0)
    net = bga.SurfPosNet(False).to("cuda").eval()
    net.compute_dtype = torch.float32
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 6, 6, generator=g).cuda()
    t = torch.tensor([249]).cuda()
    with torch.no_grad():
        before = net(x, t, None).clone()
    params = [p for p in net.parameters()]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).cuda()
    opt = optim.AdamW(params, lr=1e-2, owners=(net,))
    opt.step()
    with torch.no_grad():
        after = net(x, t, None).clone()
        fresh = bga.SurfPosNet(False)
        fresh.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
        fresh = fresh.to("cuda").eval()
        fresh.compute_dtype = torch.float32
        want = fresh(x, t, None).clone()
    info = opt.last_step_info()
    assert info["step"] == 1 and not info["found_inf"] and info["total_norm"] > 0
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
    assert np.array_equal(bits(after), bits(want))
