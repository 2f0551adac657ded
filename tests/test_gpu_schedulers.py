"""-m gpu: the scheduler kernels (csrc/elementwise.hip: DDPM, PNDM, add_noise) and `brepgen_amd/schedulers.py` around them.

  1. timestep idioms: a device timestep is taken by VALUE under every way a caller can hold one, bit-equal to host timesteps, with
     the number of device-to-host reads the feature promises (`_timestep_reads`);
  2. the reference's loops (sample.py:126-153: PNDM [:158] -> DDPM [-250:] on reused scheduler objects, then a full PNDM schedule),
     teacher-forced by the fp32 oracle: every single step against the oracle's, at the project's single-step bounds;
  3. the same loops free-running, device and oracle each against the fp64 restatement (tests/sched_restate.py);
  4. kernel edges through the C ABI against the fp64 restatement of one launch: past the grid cap, misaligned operands, a coarser
     schedule, non-finite inputs.
Bounds (from test_gpu_parity.py's single-step tests), times max(1, |ref|max): DDPM 1e-6, guided 2e-6; PNDM 2e-6, guided 4e-6."""
import gc
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(3, 30, 6), (3, 7, 6)]                          # 540 elements: float4 path; 126 = 4 * 31 + 2: scalar path
KW = dict(num_train_timesteps=1000, beta_schedule="linear", prediction_type="epsilon", beta_start=0.0001, beta_end=0.02)
TOL = {("ddpm", False): 1e-6, ("ddpm", True): 2e-6, ("pndm", False): 2e-6, ("pndm", True): 4e-6}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import brepgen_amd as bga
    import guarded
    import sched_restate as sr
    from brepgen_amd import _lib
    from oracle import schedulers as osch

    class Env:
        pass
    e = Env()
    e.bga, e.sr, e.lib, e._lib, e.osch, e.guarded = bga, sr, _lib.load(), _lib, osch, guarded
    return e


def _make(env, kind):
    return env.bga.DDPMScheduler(clip_sample=True, clip_sample_range=3, **KW) if kind == "ddpm" else env.bga.PNDMScheduler(**KW)


# ---- 1. timestep idioms ------------------------------------------------------------------------------------------------------------
WALK = {"ddpm": (1000, slice(-250, None)), "pndm": (200, slice(None, 158))}


def _walk(s, kind, ts, x0, eps, noise):
    """Closed loop over the timesteps `ts` (any form) with fixed per-step eps / noise: -> every step's output, stacked."""
    x, outs = x0, []
    for i, t in enumerate(ts):
        x = (s.step(eps[i], t, x, noise=noise[i]) if kind == "ddpm" else s.step(eps[i], t, x)).prev_sample
        outs.append(x)
    return torch.stack(outs)


@pytest.fixture(scope="module")
def idiom_data(env):
    """Per (kind, shape): start, per-step eps and noise on the device, and the run with HOST timesteps (computed once, never changed)."""
    data = {}
    for kind, (n, sl) in WALK.items():
        for shape in SHAPES:
            g = torch.Generator().manual_seed(11)
            steps = len(range(*sl.indices(1000 if kind == "ddpm" else 209)))
            x0 = torch.randn(*shape, generator=g).to(DEV)
            eps = torch.randn(steps, *shape, generator=g).to(DEV)
            noise = torch.randn(steps, *shape, generator=g).to(DEV)
            s = _make(env, kind)
            s.set_timesteps(n)
            host = _walk(s, kind, s.timesteps[sl], x0, eps, noise)
            assert s._timestep_reads == 0
            data[(kind, shape)] = (x0, eps, noise, host, steps)
    return data


def _form_own_device(s, n, sl):
    s.set_timesteps(n, device=DEV)
    return s.timesteps[sl]


def _form_copy_then_slice(s, n, sl):
    s.set_timesteps(n)
    return s.timesteps.to(DEV)[sl]


def _form_slice_then_copy(s, n, sl):
    s.set_timesteps(n)
    return s.timesteps[sl].to(DEV)


def _form_one_element_views(s, n, sl):
    s.set_timesteps(n)
    d = s.timesteps.to(DEV)
    return [d[i:i + 1] for i in range(*sl.indices(d.numel()))]


def _form_fresh_scalars(s, n, sl):
    s.set_timesteps(n)
    return (torch.tensor(int(t), device=DEV) for t in s.timesteps[sl])


FORMS = [(_form_own_device, 0), (_form_copy_then_slice, 1), (_form_slice_then_copy, 1), (_form_one_element_views, 1),
         (_form_fresh_scalars, None)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["ddpm", "pndm"])
def test_device_timesteps_in_every_form_equal_host_timesteps(env, idiom_data, kind, shape):
    """DDPM walks [-250:] (where position and value differ: position 0 of the schedule is t = 999), PNDM [:158]."""
    x0, eps, noise, host, steps = idiom_data[(kind, shape)]
    n, sl = WALK[kind]
    for form, reads in FORMS:
        s = _make(env, kind)
        got = _walk(s, kind, form(s, n, sl), x0, eps, noise)
        assert torch.equal(got, host), (form.__name__, int((got != host).flatten(1).any(1).nonzero()[0]))
        assert s._timestep_reads == (steps if reads is None else reads), (form.__name__, s._timestep_reads)


def _host_walk(env, ts, x0, eps, noise):
    s = _make(env, "ddpm")
    s.set_timesteps(1000)
    return _walk(s, "ddpm", ts, x0, eps, noise)


def test_timestep_memo_strided_out_of_order_walk(env, idiom_data):
    x0, eps, noise, _, _ = idiom_data[("ddpm", SHAPES[1])]
    s = _make(env, "ddpm")
    s.set_timesteps(1000)
    d = s.timesteps.to(DEV)
    order = [5, 2, 9, 0, 26, 13]                           # of d[::37]: t = 999 - 37 * k
    got = _walk(s, "ddpm", [d[::37][k] for k in order], x0, eps, noise)
    assert torch.equal(got, _host_walk(env, [999 - 37 * k for k in order], x0, eps, noise))
    assert s._timestep_reads == 1


def test_timestep_memo_does_not_outlive_its_tensor(env, idiom_data):
    """A foreign tensor is freed and another of the same size takes its place -- with the caching allocator, most likely at the same
    address: the walk uses the new values (the memo knows the tensor object, not its address)."""
    x0, eps, noise, _, _ = idiom_data[("ddpm", SHAPES[1])]
    s = _make(env, "ddpm")
    s.set_timesteps(1000)
    first, second = [900, 500, 100], [899, 2, 640]
    a = torch.tensor(first, device=DEV)
    addr = a.data_ptr()
    x = _walk(s, "ddpm", list(a), x0, eps, noise)
    del a
    gc.collect()
    b = torch.tensor(second, device=DEV)
    print("address reused:", b.data_ptr() == addr)
    y = _walk(s, "ddpm", list(b), x[-1], eps[3:], noise[3:])
    assert torch.equal(torch.cat([x, y]), _host_walk(env, first + second, x0, eps, noise))
    assert s._timestep_reads == 2


def test_timestep_memo_rereads_a_tensor_written_in_place(env, idiom_data):
    x0, eps, noise, _, _ = idiom_data[("ddpm", SHAPES[1])]
    s = _make(env, "ddpm")
    s.set_timesteps(1000)
    d = torch.tensor([700, 300], device=DEV)
    x = s.step(eps[0], d[0], x0, noise=noise[0]).prev_sample
    d.add_(1)
    y = s.step(eps[1], d[1], x, noise=noise[1]).prev_sample
    assert torch.equal(torch.stack([x, y]), _host_walk(env, [700, 301], x0, eps, noise))
    assert s._timestep_reads == 2
    own = _make(env, "ddpm")                               # the scheduler's own device schedule, written: no longer trusted, read
    own.set_timesteps(1000, device=DEV)
    t = own.timesteps[299]
    own.timesteps.add_(1)
    z = own.step(eps[0], t, x0, noise=noise[0]).prev_sample
    assert torch.equal(z, _host_walk(env, [701], x0, eps, noise)[0]) and own._timestep_reads == 1


# ---- 2 + 3. the reference's loops --------------------------------------------------------------------------------------------------
class DeviceSide:
    """brepgen_amd's schedulers on the GPU, with HOST timesteps (what CascadeSampler and bench.py pass)."""
    def __init__(self, env):
        self.s = {"pndm": _make(env, "pndm"), "ddpm": _make(env, "ddpm")}

    def begin(self, kind, n):
        self.s[kind].set_timesteps(n)
        return [int(t) for t in self.s[kind].timesteps]

    put = staticmethod(lambda x: x.to(DEV))
    get32 = staticmethod(lambda x: x.cpu())
    get = staticmethod(lambda x: x.double().cpu().numpy())

    def step(self, kind, eps, t, x, noise, guidance):
        kw = dict(noise=noise.to(DEV)) if kind == "ddpm" else {}
        return self.s[kind].step(eps, t, x, guidance=guidance, **kw).prev_sample


CASES = [(shape, w) for shape in SHAPES for w in (None, 0.6)]


@pytest.mark.parametrize("shape,w", CASES)
def test_reference_loops_teacher_forced_by_the_oracle(env, shape, w):
    """The oracle runs the three stages closed-loop; at every step the device gets the oracle's (eps, t, x) -- the raw 2B eps and
    `guidance=` in the guided cases, t as a view of a device copy of the schedule -- and its prev_sample is held against the oracle's.
    No error accumulates, so the single-step bounds hold at every one of the 617 steps; |x| reaches ~ 150 early in PNDM, hence
    the scaling by max(1, |ref|max)."""
    sr = env.sr
    orc, dev = sr.OracleSide(), DeviceSide(env)
    got, want, x = [], [], None
    for st in sr.loop_inputs(shape, w):
        kind = st["kind"]
        full = orc.begin(kind, st["n"])
        assert dev.begin(kind, st["n"]) == full
        ts_dev = torch.tensor(full, device=DEV)[st["sl"]]
        if st["x0"] is not None:
            x = st["x0"]
        for i, t in enumerate(full[st["sl"]]):
            eps = sr.pseudo_net(x, st["model_noise"][i], w)
            z = st["step_noise"][i] if kind == "ddpm" else None
            got.append((kind, t, dev.step(kind, eps.to(DEV), ts_dev[i], x.to(DEV), z, w)))
            x = orc.step(kind, eps, t, x, z, w)
            want.append(x)
    assert len(got) == 617
    worst = {}
    for i, ((kind, t, g), r) in enumerate(zip(got, want)):
        err = float((g.cpu() - r).abs().max()) / max(1.0, float(r.abs().max()))
        worst[kind] = max(worst.get(kind, 0.0), err)
        assert err <= TOL[(kind, bool(w))], (i, kind, t, err)
    print("teacher-forced", shape, w, worst)
    assert dev.s["ddpm"]._timestep_reads == 1 and dev.s["pndm"]._timestep_reads == 2      # one copy per device schedule


def _record(path, key, value):
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        d = {}
    d[key] = value
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def restated(env):
    return {c: env.sr.free_run(env.sr.RestateSide(), *c) for c in CASES}


@pytest.mark.parametrize("shape,w", CASES)
def test_reference_loops_free_running_are_as_close_to_fp64_as_the_oracle(env, restated, shape, w):
    """Device and fp32 oracle each closed-loop from the same start, the pseudo-model in fp32 on the CPU for both; per step
    max|x - x64| / max(1, |x64|max) against the fp64 restatement's own closed loop; pooled over the 617 steps, the device's max and
    mean are within twice the oracle's.  The oracle's own error is 9e-5 max (the fp32 rounding of 1 - acp_t / acp_prev at small t,
    which the device shares bit for bit), so this says the loop as a whole is as good as upstream's formulation; the sharp test of
    the kernels is the teacher-forced one.  BG_SCHED_PARITY_JSON=<path> records both sides' figures."""
    sr = env.sr
    e_dev = sr.loop_errors(sr.free_run(DeviceSide(env), shape, w), restated[(shape, w)])
    e_orc = sr.loop_errors(sr.free_run(sr.OracleSide(), shape, w), restated[(shape, w)])
    rec = {"device": e_dev, "oracle": e_orc, "ratio_max": e_dev["loop"][0] / e_orc["loop"][0],
           "ratio_mean": e_dev["loop"][1] / e_orc["loop"][1]}
    print("free-running", shape, w, rec)
    if os.environ.get("BG_SCHED_PARITY_JSON"):
        _record(os.environ["BG_SCHED_PARITY_JSON"], f"shape={'x'.join(map(str, shape))} guidance={w}", rec)
    assert e_dev["loop"][0] <= 2 * e_orc["loop"][0] and e_dev["loop"][1] <= 2 * e_orc["loop"][1], rec


# ---- 4. kernel edges, through the C ABI --------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else t.data_ptr()


def _ddpm_abi(env, ec, eu, w, x, z, out, n, c, clip):
    env._lib.check(env.lib.bg_cfg_ddpm_step(_p(ec), _p(eu), w, _p(x), _p(z), _p(out), n, float(c["sqrt_alpha_prod"]),
                                            float(c["sqrt_beta_prod"]), float(c["x0_coeff"]), float(c["xt_coeff"]),
                                            float(c["sigma"]), clip, env._lib.stream()), "bg_cfg_ddpm_step")


def _coeffs(env, t, n_inference=1000):
    """The oracle's fp32 scalars of step t under the kernel's argument names (exact in fp64: they are the launch's inputs)."""
    o = env.osch.OracleDDPM(clip_sample_range=3)
    o.set_timesteps(n_inference)
    c = o.coefficients(t)
    return dict(sqrt_alpha_prod=c["sqrt_alpha_prod_t"], sqrt_beta_prod=c["sqrt_beta_prod_t"], x0_coeff=c["x0_coeff"],
                xt_coeff=c["xt_coeff"], sigma=c["sigma"])


def _close(got, want64, tol, what):
    got = got.detach().double().cpu().numpy().reshape(-1)
    want64 = np.asarray(want64).reshape(-1)
    d = np.abs(got - want64)
    assert np.isfinite(got).all(), what
    i = int(d.argmax())
    assert d[i] <= tol * max(1.0, float(np.abs(want64).max())), (what, i, float(d[i]))


def _guard_out(env, n):
    return env.guarded.guarded((1, n), torch.float32, DEV)


def _check_out(g, what):
    torch.cuda.synchronize()
    g.assert_untouched(what)
    g.assert_fully_written(what)


W = 0.6                                                   # the ABI takes float: the reference gets the same fp32 value
W32 = float(np.float32(W))


@pytest.mark.parametrize("n", [2048 * 256 * 4 + 4, 2048 * 256 + 3])
def test_ddpm_past_the_grid_cap(env, n):
    """2048 blocks x 256 threads is one pass of the grid-stride loop: n = cap * 4 + 4 leaves ONE float4 for a second pass of the
    vector kernel, n = cap + 3 three elements for a second pass of the scalar kernel (n % 4 = 3).  Guided, with noise, every
    element compared."""
    g = torch.Generator().manual_seed(n % 1000)
    ec, eu, x, z = (torch.randn(n, generator=g) for _ in range(4))
    c = _coeffs(env, 249)
    out = _guard_out(env, n)
    d = [t.to(DEV) for t in (ec, eu, x, z)]
    _ddpm_abi(env, d[0], d[1], W, d[2], d[3], out.view, n, c, 3.0)
    _check_out(out, f"ddpm n={n}")
    want = env.sr.ddpm_update(env.sr.guided(torch.cat([ec, eu]), W32, n), x, z, clip=3.0, **c)
    _close(out.view, want, TOL[("ddpm", True)], f"ddpm n={n}")
    _close(out.view.reshape(-1)[-8:], want[-8:], TOL[("ddpm", True)], f"ddpm n={n}: the second pass")


def _pndm_abi(env, ec, eu, w, x, store, acc, acc_out, so, se, ce, ca, hist, ch, sc, epc, out, n):
    hist = list(hist) + [None] * (3 - len(hist))
    ch = list(ch) + [0.0] * (3 - len(ch))
    env._lib.check(env.lib.bg_pndm_step(_p(ec), _p(eu), w, _p(x), _p(store), _p(acc), _p(acc_out), so, se, ce, ca,
                                        *[_p(h) for h in hist], *ch, sc, epc, _p(out), n, env._lib.stream()), "bg_pndm_step")


F = lambda v: float(np.float32(v))                         # noqa: E731  (a scalar as the float ABI receives it)
PLMS4 = (F(55 / 24), [F(-59 / 24), F(37 / 24), F(-9 / 24)])


@pytest.mark.parametrize("mode", ["prk1", "plms"])
def test_pndm_past_the_grid_cap(env, mode):
    """4096 x 256 elements are one pass: n = cap + 1.  A Runge-Kutta evaluation that accumulates in place (r = 1) and the four-term
    linear multistep, guided; prev_sample and every side output compared."""
    n = 4096 * 256 + 1
    g = torch.Generator().manual_seed(5)
    ec, eu, x, acc, h0, h1, h2 = (torch.randn(n, generator=g) for _ in range(7))
    sc, epc = F(1.0123), F(0.0456)
    e64 = env.sr.guided(torch.cat([ec, eu]), W32, n)
    d = {k: v.to(DEV) for k, v in dict(ec=ec, eu=eu, x=x, h0=h0, h1=h1, h2=h2).items()}
    out = _guard_out(env, n)
    tol = TOL[("pndm", True)]
    if mode == "prk1":
        acc_g = _guard_out(env, n)
        acc_g.view.copy_(acc.reshape(1, n))
        _pndm_abi(env, d["ec"], d["eu"], W, d["x"], None, acc_g.view, acc_g.view, 1.0, F(1 / 3), 1.0, 0.0, [], [], sc, epc,
                  out.view, n)
        _check_out(out, "pndm prk1")
        _check_out(acc_g, "pndm prk1 acc")
        want, _, want_acc = env.sr.pndm_update(e64, x, acc, 1.0, 0.0, [], [], sc, epc, 1.0, F(1 / 3))
        _close(acc_g.view, want_acc, tol, "pndm prk1 acc")
    else:
        store = _guard_out(env, n)
        _pndm_abi(env, d["ec"], d["eu"], W, d["x"], store.view, None, None, 0.0, 0.0, PLMS4[0], 0.0,
                  [d["h0"], d["h1"], d["h2"]], PLMS4[1], sc, epc, out.view, n)
        _check_out(out, "pndm plms")
        _check_out(store, "pndm plms e_store")
        want, want_e, _ = env.sr.pndm_update(e64, x, None, PLMS4[0], 0.0, [h0, h1, h2], PLMS4[1], sc, epc)
        _close(store.view, want_e, tol, "pndm plms e_store")
    _close(out.view, want, tol, f"pndm {mode}")
    _close(out.view.reshape(-1)[-4:], want[-4:], tol, f"pndm {mode}: the second pass")


def test_add_noise_past_the_grid_cap(env):
    """B = 3, per = 349 527: n = 4096 * 256 + 5, so the last five elements (of sample 2) belong to the second pass.  Two roundings of
    products below 8 and one of the sum: 1e-6 as in test_add_noise_writes_b_times_per_sample."""
    B, per = 3, 349527
    assert B * per == 4096 * 256 + 5
    g = torch.Generator().manual_seed(8)
    x0, z = torch.randn(B, per, generator=g) * 1.5, torch.randn(B, per, generator=g)
    sa, sb = torch.rand(B, generator=g), torch.rand(B, generator=g)
    out = env.guarded.guarded((B, per), torch.float32, DEV)
    d = [t.to(DEV) for t in (x0, z, sa, sb)]
    env._lib.check(env.lib.bg_add_noise(*[t.data_ptr() for t in d], out.view.data_ptr(), B, per, env._lib.stream()), "bg_add_noise")
    _check_out(out, "add_noise")
    want = sa.double()[:, None] * x0.double() + sb.double()[:, None] * z.double()
    _close(out.view, want.numpy(), 1e-6, "add_noise")


@pytest.mark.parametrize("which", ["eps_c", "eps_u", "x", "noise", "out"])
def test_ddpm_one_operand_off_16_byte_alignment(env, which):
    """n % 4 == 0, four operands 16-byte aligned, one 4 bytes off (a contiguous [1:] view): the launch must take the scalar kernel.
    Every operand sits between NaN-sentinel guard bands, so a 16-byte access rounded down to its aligned address reads or writes
    a sentinel."""
    n = 1028                                               # five blocks of the scalar kernel
    g = torch.Generator().manual_seed(21)
    host = {k: torch.randn(n, generator=g) for k in ("eps_c", "eps_u", "x", "noise")}
    bufs = {k: env.guarded.guarded((1, n + 4), torch.float32, DEV) for k in ("eps_c", "eps_u", "x", "noise", "out")}
    off = {k: (1 if k == which else 0) for k in bufs}
    view = {k: b.view.reshape(-1)[off[k]:off[k] + n] for k, b in bufs.items()}
    for k, v in host.items():
        view[k].copy_(v)
    assert all((view[k].data_ptr() % 16 == 0) == (k != which) for k in view) and view[which].data_ptr() % 16 == 4
    c = _coeffs(env, 249)
    _ddpm_abi(env, view["eps_c"], view["eps_u"], W, view["x"], view["noise"], view["out"], n, c, 3.0)
    torch.cuda.synchronize()
    bufs["out"].assert_untouched(f"ddpm misaligned {which}")
    written = bufs["out"].written_mask().reshape(-1)
    lo = off["out"]
    assert bool(written[lo:lo + n].all()) and not bool(written[:lo].any()) and not bool(written[lo + n:].any()), which
    want = env.sr.ddpm_update(env.sr.guided(torch.cat([host["eps_c"], host["eps_u"]]), W32, n), host["x"], host["noise"],
                              clip=3.0, **c)
    _close(view["out"], want, TOL[("ddpm", True)], f"ddpm misaligned {which}")


@pytest.mark.parametrize("shape", SHAPES)
def test_ddpm_with_fewer_inference_steps(env, shape):
    """set_timesteps(50) on the device: prev_t = t - 20, and at the last step (t = 0) prev_t < 0 -> alpha_prod_prev = 1, no noise.
    Reference: the fp64 update with the ORACLE's scalars of (t, 50 steps), which are a launch's exact inputs; that those scalars
    are the fp64 ones rounded is test_schedulers_cpu.py's business."""
    s = env.bga.DDPMScheduler(clip_sample=True, clip_sample_range=3, **KW)
    s.set_timesteps(50, device=DEV)
    assert s.timesteps.tolist() == list(range(980, -1, -20))
    g = torch.Generator().manual_seed(50)
    for i in (0, 1, 25, 48, 49):
        t = 980 - 20 * i
        x, eps, z = (torch.randn(*shape, generator=g) for _ in range(3))
        got = s.step(eps.to(DEV), s.timesteps[i], x.to(DEV), noise=z.to(DEV)).prev_sample
        want = env.sr.ddpm_update(eps, x, z, clip=3.0, **_coeffs(env, t, 50))
        _close(got, want, TOL[("ddpm", False)], f"ddpm 50 steps t={t}")
        if t == 0:
            assert torch.equal(got, s.step(eps.to(DEV), 0, x.to(DEV), noise=2 * z.to(DEV)).prev_sample)    # no noise at t = 0
    assert s._timestep_reads == 0


def _same_class(got, want):
    """NaN where the oracle has NaN, +-inf where it has +-inf, finite elsewhere: -> mask of the finite elements."""
    got, want = got.cpu(), want.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], want[inf])
    return torch.isfinite(want)


NONFINITE = [("eps", float("nan")), ("eps", float("inf")), ("eps", float("-inf")), ("x", float("nan")),
             ("eps_uncond", float("nan"))]


@pytest.mark.parametrize("where,value", NONFINITE)
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_ddpm_non_finite_inputs_come_out_as_the_oracle_has_them(env, shape, clip, where, value):
    """torch.clamp keeps NaN and sends +-inf to the bound (oracle/schedulers.py, upstream): a NaN in eps -- an overflowed fp16
    evaluation -- must reach prev_sample as NaN with clip_sample on as well, not as the clip value.  Both kernels (540 elements:
    float4; 126: scalar).  Every element that the non-finite value does not touch is bit-equal to the run without it."""
    guided = where == "eps_uncond"
    B = shape[0]
    g = torch.Generator().manual_seed(77)
    x, z = torch.randn(*shape, generator=g) * 1.5, torch.randn(*shape, generator=g)
    eps = torch.randn(*((2 * B,) + shape[1:] if guided else shape), generator=g)
    hit = torch.zeros(shape, dtype=torch.bool)
    hit.view(-1)[[0, 5, 41, hit.numel() - 1]] = True       # first and last element, both halves of a float4
    bad_x, bad_eps = x.clone(), eps.clone()
    if where == "x":
        bad_x[hit] = value
    elif guided:
        bad_eps[B:][hit] = value
    else:
        bad_eps[hit] = value
    w = 0.6 if guided else None
    t = 249
    o = env.osch.OracleDDPM(clip_sample=clip, clip_sample_range=3)
    o.set_timesteps(1000)
    want = o.step(bad_eps[:B] * (1 + w) - bad_eps[B:] * w if guided else bad_eps, t, bad_x, noise=z)
    assert bool((~torch.isfinite(want[hit])).all()) or (clip and value in (float("inf"), float("-inf")))
    if clip and where != "x":
        assert bool(torch.isnan(want[hit]).all()) == (value != value)       # NaN stays NaN; +-inf is clipped to a finite value
    s = env.bga.DDPMScheduler(clip_sample=clip, clip_sample_range=3, **KW)
    s.set_timesteps(1000)
    run = lambda e, xx: s.step(e.to(DEV), t, xx.to(DEV), noise=z.to(DEV), guidance=w).prev_sample     # noqa: E731
    got, clean = run(bad_eps, bad_x), run(eps, x)
    fin = _same_class(got, want)
    err = float((got.cpu()[fin] - want[fin]).abs().max())
    assert err <= TOL[("ddpm", guided)] * max(1.0, float(want[fin].abs().max())), err
    assert torch.equal(got.cpu()[~hit], clean.cpu()[~hit])


def test_pndm_and_add_noise_propagate_nan(env):
    """Plain arithmetic: a NaN in the PLMS history / in the noise comes out at its own element and nowhere else."""
    n = 126
    g = torch.Generator().manual_seed(9)
    ec, x, h0, h1, h2 = (torch.randn(n, generator=g) for _ in range(5))
    hit = [0, 57, n - 1]
    bad = h1.clone()
    bad[hit] = float("nan")
    outs = []
    for h in (bad, h1):
        out = _guard_out(env, n)
        d = [t.to(DEV) for t in (ec, x, h0, h, h2)]
        _pndm_abi(env, d[0], None, 0.0, d[1], None, None, None, 0.0, 0.0, PLMS4[0], 0.0, d[2:], PLMS4[1], F(1.0123), F(0.0456),
                  out.view, n)
        _check_out(out, "pndm nan")
        outs.append(out.view.reshape(-1).cpu())
    mask = torch.zeros(n, dtype=torch.bool)
    mask[hit] = True
    assert torch.equal(torch.isnan(outs[0]), mask) and torch.equal(outs[0][~mask], outs[1][~mask])
    want = env.sr.pndm_update(ec, x, None, PLMS4[0], 0.0, [h0, h1, h2], PLMS4[1], F(1.0123), F(0.0456))[0]
    _close(outs[1], want, TOL[("pndm", False)], "pndm plms")

    s = env.bga.DDPMScheduler(**KW)
    x0, z = torch.randn(3, 7, 6, generator=g), torch.randn(3, 7, 6, generator=g)
    zb = z.clone()
    zb[1, 3, 2] = float("nan")
    ts = torch.tensor([10, 500, 999])
    got, clean = s.add_noise(x0.to(DEV), zb.to(DEV), ts).cpu(), s.add_noise(x0.to(DEV), z.to(DEV), ts).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(zb)) and torch.equal(got[~torch.isnan(zb)], clean[~torch.isnan(zb)])
    want = env.osch.OracleDDPM().add_noise(x0.double(), z.double(), ts)
    _close(clean, want.numpy(), 1e-6, "add_noise")
