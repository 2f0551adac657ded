"""brepgen_amd/optim.py without a device: the numpy restatement (tests/optim_restate.py) against torch on the CPU, the C ABI of
csrc/optim.hip, the host-side validation and the state_dict layout.  No kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import brepgen_amd as bga
from brepgen_amd import _lib, optim

from tests import optim_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("bg_mt_grad_stats", "bg_mt_adamw_step", "bg_optim_finish", "bg_mt_scale_grads")

SHAPES = ((5,), (1025,), (768, 48), (4097,))
HYPER = dict(lr=5e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-6)       # the LDM trainers' setting
MAX_NORM, STEPS, INF_STEP, NAN_STEP = 50.0, 8, 2, 5


def trajectory_inputs(seed=0):
    """Parameters and 8 sets of (scaled) gradients: norms on both sides of MAX_NORM, an inf at step 2, a NaN at step 5."""
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    sigma = (0.05, 1.0, 0.1, 2.0, 0.02, 0.5, 0.2, 3.0)                         # norm ~ 203 sigma over 41 991 elements: clip iff sigma > 0.25
    grads = [[(rng.standard_normal(s) * sg).astype(np.float32) for s in SHAPES] for sg in sigma]
    grads[INF_STEP][2][100, 7] = np.inf
    grads[NAN_STEP][0][3] = np.nan
    return params, grads


def test_restatement_against_torch_on_the_cpu(capsys):
    """8 steps of the reference's four lines with stock torch on the CPU (single-tensor AdamW, GradScaler, clip_grad_norm_) next to the
    restatement: scale, growth tracker, every step counter and the skipped iterations are torch's exactly; for p, exp_avg and
    exp_avg_sq the restatement's largest error against its fp64 twin is at most 2 x that of torch's own fp32 result (the two differ
    in the grouping of three or four roundings per element and in a norm a few ulp apart).
    Measured (max over the trajectory, torch / restatement): p 5.93e-07 / 5.93e-07, exp_avg 2.89e-13 / 1.48e-13, exp_avg_sq
    1.69e-19 / 6.98e-20 ("The trainer update")."""
    params, grads = trajectory_inputs()
    kw = dict(scale=65536.0, growth_interval=2, **HYPER)
    r32, r64 = R.Trainer(params, **kw), R.Trainer(params, dtype=np.float64, **kw)
    tp = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in params]
    opt = torch.optim.AdamW(tp, foreach=False, **HYPER)
    scaler = torch.amp.GradScaler("cpu", init_scale=65536.0, growth_interval=2)
    err = {k: [0.0, 0.0] for k in ("p", "exp_avg", "exp_avg_sq")}
    clipped = []
    for k in range(STEPS):
        before = [p.detach().clone() for p in tp]
        scaler.scale(torch.zeros(()))                                             # torch creates its scale tensor here
        for p, g in zip(tp, grads[k]):
            p.grad = torch.from_numpy(g.copy())
        torch.nn.utils.clip_grad_norm_(tp, max_norm=MAX_NORM)
        scaler.step(opt)
        scaler.update()
        r32.update(grads[k], MAX_NORM)
        r64.update(grads[k], MAX_NORM)
        skipped = all(torch.equal(a, b) for a, b in zip(before, tp))
        assert r32.skipped[-1] == r64.skipped[-1] == skipped, k
        assert float(scaler.get_scale()) == float(r32.scale) and int(scaler._growth_tracker) == r32.growth_tracker, k
        steps = {int(opt.state[p]["step"]) for p in tp if p in opt.state and "step" in opt.state[p]}
        assert steps <= {r32.step} and (steps or r32.step == 0), (k, steps, r32.step)
        if not skipped:
            clipped.append(bool(r32.total_norm > MAX_NORM))
            for i, p in enumerate(tp):
                for name, mine32, mine64, theirs in (("p", r32.p[i], r64.p[i], p.detach()), ("exp_avg", r32.m[i], r64.m[i], opt.state[p]["exp_avg"]),
                                                     ("exp_avg_sq", r32.v[i], r64.v[i], opt.state[p]["exp_avg_sq"])):
                    err[name][0] = max(err[name][0], float(np.abs(theirs.numpy().astype(np.float64) - mine64).max()))
                    err[name][1] = max(err[name][1], float(np.abs(mine32.astype(np.float64) - mine64).max()))
    assert r32.skipped == [k in (INF_STEP, NAN_STEP) for k in range(STEPS)]
    assert True in clipped and False in clipped
    assert float(r32.scale) != 65536.0 and r32.step == STEPS - 2
    with capsys.disabled():
        for name, (e_torch, e_mine) in err.items():
            print(f"\n  {name}: max |torch fp32 - fp64 twin| = {e_torch:.3e}, max |restatement - fp64 twin| = {e_mine:.3e}", end="")
        print()
    for name, (e_torch, e_mine) in err.items():
        assert e_torch > 0.0 and e_mine <= 2.0 * e_torch, (name, e_torch, e_mine)


def test_norm_of_the_restatement_is_within_an_ulp_of_the_fp64_norm():
    _, grads = trajectory_inputs(1)
    for gs in grads[:2] + grads[3:5]:
        norm = R.verdict(gs)[0]
        exact = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in gs))
        assert abs(float(norm) - exact) <= float(np.spacing(np.float32(exact))), (norm, exact)
    assert R.verdict([np.zeros(0, np.float32)], 5.0) == (np.float32(0), np.float32(1), np.float32(1), False)
    # overflow through unscaling alone: every input is finite
    assert R.verdict([np.array([1e36], np.float32)], None, 2.0 ** -10)[3] and not R.verdict([np.array([1e36], np.float32)], None, 1.0)[3]


def test_chunk_lists_agree():
    numels = [0, 1, 4095, 4096, 4097, 2 * 4096 + 7, 0, 36864]
    mine = optim._chunks_of(numels)
    assert [(int(c["tensor"]), int(c["first"])) for c in mine] == R.chunk_list(numels)
    assert (optim.CHUNK, optim.MAX_BLOCKS) == (R.CHUNK, R.MAX_BLOCKS) == (4096, 2048)
    for b, n in ((0.95, 7), (0.9, 0), (0.999, 1000), (0.95, 333)):
        assert R.beta_pow(b, n) == optim._beta_pow(b, n)


def test_new_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "brepgen_hip.h")).read()
    lib = _lib.load()
    vp = _lib.vp
    want = {"bg_mt_grad_stats": [vp, vp, C.c_int, vp, vp],
            "bg_mt_adamw_step": [vp, vp, C.c_int, vp, vp, vp, C.c_float, C.c_double, C.c_double, C.c_double, vp],
            "bg_optim_finish": [vp, C.c_int, vp, vp, C.c_float, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, vp],
            "bg_mt_scale_grads": [vp, vp, C.c_int, vp, C.c_float, _lib.fp, vp]}
    for name in NEW_ENTRIES:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name][1] == want[name] and getattr(lib, name).restype is C.c_int
    assert int(re.search(r"#define BG_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.bg_abi_version() == 7
    assert int(re.search(r"#define BG_OPTIM_CHUNK (\d+)", header).group(1)) == optim.CHUNK
    assert int(re.search(r"#define BG_OPTIM_MAX_BLOCKS (\d+)", header).group(1)) == optim.MAX_BLOCKS
    assert "optim.hip" in __import__("brepgen_amd.build", fromlist=["SOURCES"]).SOURCES
    assert [C.sizeof(t) for t in (_lib.MtRow, _lib.MtChunk, _lib.OptimState, _lib.ScalerState)] == [56, 16, 32, 8]
    assert _lib.MtRow.lr.offset == 40 and _lib.OptimState.step.offset == 16 and _lib.OptimState.found_inf.offset == 24
    assert bga.optim is optim and "optim" in bga.__all__


def test_entries_validate_before_they_launch():
    lib = _lib.load()
    fake = 0x10000                                   # aligned, never dereferenced: validation fails first
    assert lib.bg_mt_grad_stats(None, None, 0, None, None) == 0 and lib.bg_mt_adamw_step(None, None, 0, None, None, None, -1.0, 0.9, 0.999, 1e-8, None) == 0
    assert lib.bg_mt_grad_stats(fake, fake, -1, fake, None) == _lib.BG_E_SHAPE
    assert lib.bg_mt_grad_stats(None, fake, 3, fake, None) == _lib.BG_E_ARG and lib.bg_last_error()
    assert lib.bg_mt_grad_stats(fake, fake + 8, 3, fake, None) == _lib.BG_E_ALIGN
    assert lib.bg_mt_adamw_step(fake, fake, 3, fake, None, None, -1.0, 0.9, 0.999, 1e-8, None) == _lib.BG_E_ARG          # no state
    assert lib.bg_mt_adamw_step(fake, fake, 3, fake, fake, None, -1.0, 1.0, 0.999, 1e-8, None) == _lib.BG_E_ARG          # beta1 = 1
    assert lib.bg_mt_adamw_step(fake, fake, 3, fake, fake + 4, None, -1.0, 0.9, 0.999, 1e-8, None) == _lib.BG_E_ALIGN
    assert lib.bg_optim_finish(fake, 3, None, None, -1.0, 0.9, 0.999, 2.0, 0.5, 2000, None) == _lib.BG_E_ARG
    assert lib.bg_optim_finish(fake, 3, fake, fake, -1.0, 0.9, 0.999, 2.0, 0.5, 0, None) == _lib.BG_E_ARG                # growth_interval = 0
    assert lib.bg_optim_finish(fake + 8, 3, fake, None, -1.0, 0.9, 0.999, 2.0, 0.5, 1, None) == _lib.BG_E_ALIGN
    assert lib.bg_mt_scale_grads(fake, fake, 3, fake, -1.0, None, None) == _lib.BG_E_ARG                                  # no max_norm
    assert lib.bg_mt_scale_grads(fake, fake, 3, None, 1.0, None, None) == _lib.BG_E_ARG


def test_validation_without_a_device():
    p = torch.nn.Parameter(torch.zeros(7))
    p.grad = torch.ones(7)
    opt = optim.AdamW([p])                           # like the package's modules: built anywhere, runs on the device only
    with pytest.raises(_lib.BrepgenHipError, match="no CPU fallback"):
        opt.step()
    with pytest.raises(_lib.BrepgenHipError, match="no CPU fallback"):
        optim.GradScaler().step(opt, max_norm=5.0)
    with pytest.raises(_lib.BrepgenHipError, match="no CPU fallback"):
        optim.clip_grad_norm_([p], 5.0)
    with pytest.raises(_lib.BrepgenHipError, match="no CPU fallback"):
        optim.GradScaler().scale(torch.zeros(()))
    with pytest.raises(ValueError, match="float32"):
        optim.AdamW([torch.zeros(4, dtype=torch.bfloat16)])
    with pytest.raises(ValueError, match="contiguous"):
        optim.AdamW([torch.zeros(4, 6).t()])
    a, b = torch.zeros(3), torch.zeros(3)
    with pytest.raises(ValueError, match="betas"):
        optim.AdamW([{"params": [a], "betas": (0.9, 0.999)}, {"params": [b], "betas": (0.95, 0.999)}])
    with pytest.raises(ValueError, match="eps"):
        optim.AdamW([{"params": [a]}, {"params": [b], "eps": 1e-6}])
    with pytest.raises(ValueError):
        optim.AdamW([{"params": [a]}, {"params": [a]}])
    two = optim.AdamW([{"params": [a], "lr": 1e-3}, {"params": [b], "lr": 1e-4, "weight_decay": 0.0}], betas=(0.95, 0.999))
    assert [g["lr"] for g in two.param_groups] == [1e-3, 1e-4] and two.param_groups[1]["betas"] == (0.95, 0.999)
    with pytest.raises(RuntimeError):
        optim.GradScaler().update()                  # nothing was stepped
    with pytest.raises(ValueError):
        optim.clip_grad_norm_([p], 5.0, norm_type=1.0)
    opt.zero_grad()
    assert p.grad is None
    assert optim.GradScaler(init_scale=4.0).state_dict() == {"scale": 4.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000,
                                                             "_growth_tracker": 0}
    assert set(optim.GradScaler().state_dict()) == set(torch.amp.GradScaler("cpu").state_dict())


def test_state_dict_layout_is_torch_adamw():
    """A torch.optim.AdamW continues from our state_dict and we load torch's: the round trip through this optimiser changes nothing of
    what a torch optimiser computes next."""
    params, grads = trajectory_inputs(2)

    def torch_opt(groups=True):
        tp = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in params]
        spec = [{"params": tp[:2], "lr": 1e-3}, {"params": tp[2:], "weight_decay": 0.0}] if groups else tp
        return tp, torch.optim.AdamW(spec, foreach=False, **HYPER)

    def run(tp, opt, ks):
        for k in ks:
            for p, g in zip(tp, grads[k]):
                p.grad = torch.from_numpy(g.copy())
            opt.step()

    tp_a, opt_a = torch_opt()
    run(tp_a, opt_a, (0, 1, 3))                      # (2 and 5 carry the inf and the NaN)
    tp_m = [torch.nn.Parameter(p.detach().clone()) for p in tp_a]
    mine = optim.AdamW([{"params": tp_m[:2]}, {"params": tp_m[2:]}])
    mine.load_state_dict(opt_a.state_dict())
    assert mine._step == 3 and mine.param_groups[0]["lr"] == 1e-3 and mine.param_groups[1]["weight_decay"] == 0.0
    assert mine.param_groups[0]["betas"] == HYPER["betas"]
    sd, ref = mine.state_dict(), opt_a.state_dict()
    assert set(sd) == set(ref) and [set(g) for g in sd["param_groups"]] == [set(g) for g in ref["param_groups"]]
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in ref["param_groups"]] and set(sd["state"]) == set(ref["state"])
    for i in sd["state"]:
        assert set(sd["state"][i]) == set(ref["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(sd["state"][i]["step"]) == 3.0 and sd["state"][i]["step"].dtype == ref["state"][i]["step"].dtype
        assert torch.equal(sd["state"][i]["exp_avg"], ref["state"][i]["exp_avg"]) and torch.equal(sd["state"][i]["exp_avg_sq"], ref["state"][i]["exp_avg_sq"])
    tp_b, opt_b = torch_opt(groups=False)            # a fresh torch optimiser, other hyper-parameters until it loads ours
    for b, a in zip(tp_b, tp_a):
        b.data.copy_(a.data)
    opt_b = torch.optim.AdamW([{"params": tp_b[:2]}, {"params": tp_b[2:]}], foreach=False)
    opt_b.load_state_dict(sd)
    run(tp_a, opt_a, (4, 6))
    run(tp_b, opt_b, (4, 6))
    for a, b in zip(tp_a, tp_b):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    with pytest.raises(ValueError, match="steps differ"):
        bad = opt_a.state_dict()
        bad["state"][0]["step"] = torch.tensor(9.0)
        mine.load_state_dict(bad)
    fresh = optim.AdamW([torch.zeros(3)]).state_dict()
    assert fresh["state"] == {} and fresh["param_groups"][0]["params"] == [0] and fresh["param_groups"][0]["decoupled_weight_decay"] is True
