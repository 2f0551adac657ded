"""-m gpu: round-3 additions -- the 256 x 256 persistent GEMM (bit-identical to the 128 x 128 kernel, alone and as the
256 + 128 hybrid, host- and device-side row counts), the free-running PNDM chain against the fp32 oracle, the VAE passes at
sizes that take the implicit-GEMM + chunked path against the oracle and against torch autocast of the oracle, and the
per-call key of the device-side ancestral noise.  Measured numbers go to gpurun_out/parity_r03.json (copied to profiles/)."""
import json
import os

import pytest
import torch

from gpu_check import tune  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pc():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import parity_cases
    return parity_cases


def _record(key, value):
    """Measured parity numbers of this run -> gpurun_out/parity_r03.json (merged)."""
    path = os.path.join(ROOT, "gpurun_out", "parity_r03.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        d = {}
    d[key] = value
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


# ---- the 256 x 256 persistent GEMM -------------------------------------------------------------------------------------
def _gemm_cases(M, dt, seed=0):
    import hip_ops as ops
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(M, 768) * 2
    a = x.to(dt).cuda()
    grp = x.reshape(M, 12, 64)
    stats = torch.stack([grp.sum(-1), (grp * grp).sum(-1)], -1).permute(1, 0, 2).contiguous().cuda()
    cases = {}
    for name, N, act in (("qkv", 2304, 0), ("ffn1", 1024, 1)):
        w, b = (rn(N, 768) * 0.04).to(dt).cuda(), rn(N).cuda()
        cs = w.float().sum(1).contiguous()
        cases[name + " plain"] = lambda a=a, w=w, b=b, act=act: ops.linear(a, w, b, out_dtype=dt, act=act)
        cases[name + " nobias"] = lambda a=a, w=w: ops.linear(a, w, None, out_dtype=dt)
        cases[name + " fold"] = lambda a=a, w=w, b=b, act=act, cs=cs: ops.linear_ex(a, w, b, act=act, stats_in=stats, colsum=cs)["out"]
    return cases


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("M", [1037, 1038, 256 * 7, 130, 17294])
def test_p256_gemm_is_bit_identical_to_the_128_kernel(pc, tune, dt, M):
    """Plain and LayerNorm-fold epilogues, ragged row counts, the 256 kernel alone (P256_MODE = 1) and as the 256 + 128 hybrid
    (P256_MODE = 0; at M = 17 294 the QKV launch splits into two full rounds on the 256 kernel + 12 row panels on the 128
    kernel).  Odd M: the fold launches stay on the 128 kernel (the 256 kernel fetches the row statistics two rows per DMA
    element).  Repeated: a race in the 8-phase K loop would not necessarily show the first time."""
    for name, fn in _gemm_cases(M, dt).items():
        tune("P256_MODE", 2)
        ref = fn().clone()
        for mode in (1, 0):
            tune("P256_MODE", mode)
            for _ in range(3):
                got = fn()
                torch.cuda.synchronize()
                assert torch.equal(ref, got), (name, M, dt, mode)


@pytest.mark.parametrize("n_split", [1, 2])
def test_p256_inside_the_denoiser_with_device_side_row_counts(pc, tune, n_split):
    """SurfZNet at the headline shape (512 x 60, ragged mask -> the compacted row count only exists on the device): the
    eps-prediction with the 256 + 128 hybrid GEMMs equals the one computed by the 128 kernel alone, bit for bit, dense
    and variable-length."""
    for varlen in (True, False):
        m, _ = pc.build_net("SurfZNet", 5, False, BF16, varlen=varlen)
        m.n_split = n_split
        args = [a.cuda() if torch.is_tensor(a) else a for a in pc.synth_inputs("SurfZNet", 512, 60, 1, False)]
        with torch.no_grad():
            tune("P256_MODE", 2)
            ref = m(*args).clone()
            tune("P256_MODE", 0)
            got = m(*args)
            tune("P256_MODE", 1)
            got1 = m(*args)
        assert torch.isfinite(ref).all() and torch.equal(ref, got) and torch.equal(ref, got1)


# ---- the PNDM chain (what SurfZ / EdgeZ and 158 of the position steps run) ----------------------------------------------
@pytest.mark.parametrize("dt,bound", [(F32, 1e-5), (BF16, 6e-3), (F16, 6e-4)])
def test_pndm_chain_free_running_vs_fp32_oracle(pc, dt, bound):
    """B = 1, N = 60 SurfZNet, the full 209-evaluation PNDM schedule (PRK warm-up, then PLMS), nothing injected: the HIP
    chain (16-bit operands) and the fp32 oracle chain each follow their own trajectory.  With random-init weights the
    trajectory is not a denoising one -- |x| grows to several hundred -- so the error is reported (and asserted) relative
    to max(1, |x|_max) of the oracle's state at the same step: max over the 209 steps measured 1.3e-6 (fp32), 1.9e-3
    (bf16), 1.7e-4 (fp16) (profiles/r03/parity_r03.json); asserted at ~3x that."""
    import brepgen_amd as bga
    from oracle import denoisers as orc
    from oracle.schedulers import OraclePNDM
    m, sd = pc.build_net("SurfZNet", 21, False, dt, varlen=True)
    z, _, pos, mask, _ = pc.synth_inputs("SurfZNet", 1, 60, 1, False, seed=77)
    kw = dict(num_train_timesteps=1000, beta_schedule="linear", prediction_type="epsilon", beta_start=0.0001, beta_end=0.02)
    sch, osch = bga.PNDMScheduler(**kw), OraclePNDM()
    sch.set_timesteps(200)
    osch.set_timesteps(200)
    assert torch.equal(sch.timesteps, osch.timesteps) and len(sch.timesteps) == 209
    x, xo = z.cuda(), z.clone()
    posd, maskd = pos.cuda(), mask.cuda()
    valid = ~mask[0]
    errs, rels, tf_rel = [], [], []
    with torch.no_grad():
        for i, t in enumerate(sch.timesteps):
            eps_o = pc.oracle_on_device(orc.surfz_forward, sd, xo, t.reshape(-1), pos, mask)
            eps = m(x, t.reshape(-1).cuda(), posd, maskd, None)
            # (teacher-forced eps error at this step, on the oracle's trajectory: how far ONE evaluation is off)
            tf = float((m(xo.cuda(), t.reshape(-1).cuda(), posd, maskd, None).cpu() - eps_o)[0][valid].abs().max())
            tf_rel.append(tf / max(1.0, float(eps_o[0][valid].abs().max())))
            x = sch.step(eps, t, x).prev_sample
            xo = osch.step(eps_o, t, xo)
            errs.append(float((x.cpu() - xo)[0][valid].abs().max()))
            rels.append(errs[-1] / max(1.0, float(xo[0][valid].abs().max())))
    _record(f"pndm_chain_surfz_b1_n60_{str(dt)[6:]}", {
        "x_rel_err_max_over_steps": max(rels), "x_rel_err_at_steps_0_11_50_100_150_208": [float("%.3g" % rels[i]) for i in (0, 11, 50, 100, 150, 208)],
        "x_abs_err_last": errs[-1], "x_abs_max_last": float(xo.abs().max()),
        "eps_rel_err_teacher_forced_max": max(tf_rel)})
    assert all(e == e for e in errs) and max(rels) < bound


# ---- VAE passes at sizes that take the implicit-GEMM + chunked path ----------------------------------------------------
@pytest.mark.parametrize("kind,n", [("surf", 64), ("edge", 512)])
@pytest.mark.parametrize("dt", [BF16, F16])
def test_vae_decode_large_vs_oracle_and_torch_autocast(pc, kind, n, dt):
    """>= 64 faces / >= 512 edges: bg_vae_run takes the implicit-GEMM convolutions (>= 64 tiles per layer) -- the product
    default at the cascade's sizes.  Compared with oracle/vae.py run in fp32 on the device, next to torch.autocast of the
    same oracle (how sample.py:121 runs the reference), like the denoisers: err(HIP) <= 1.25 x err(autocast)."""
    import brepgen_amd as bga
    from oracle import vae as ov
    g = torch.Generator().manual_seed(123)
    if kind == "surf":
        sd = ov.seeded_state_dict(ov.surf_decoder_spec(), 31)
        m = bga.AutoencoderKLFastDecode(**pc.SURF_CFG)
        z = torch.randn(n, 3, 4, 4, generator=g)
        ref_fn = ov.surf_decode
    else:
        sd = ov.seeded_state_dict(ov.edge_decoder_spec(), 41)
        m = bga.AutoencoderKL1DFastDecode(**pc.EDGE_CFG)
        z = torch.randn(n, 3, 4, generator=g)
        ref_fn = ov.edge_decode
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    sdd = {k: v.cuda() for k, v in sd.items()}
    zd = z.cuda()
    with torch.no_grad():
        want = ref_fn(sdd, zd).float()
        with torch.autocast("cuda", dtype=dt):
            auto = ref_fn(sdd, zd).float()
        m.compute_dtype = dt
        got = m(zd).float()
        m.compute_dtype = F32
        got32 = m(zd).float()
    e = lambda a: (float((a - want).abs().max()), float((a - want).abs().mean()))
    hip, ac, f32 = e(got), e(auto), e(got32)
    ref_max = float(want.abs().max())
    _record(f"vae_{kind}_decode_n{n}_{str(dt)[6:]}", {"hip_max": hip[0], "hip_mean": hip[1], "autocast_max": ac[0], "autocast_mean": ac[1],
                                                      "hip_fp32_max": f32[0], "ref_absmax": ref_max})
    assert torch.isfinite(got).all()
    assert f32[0] < 2e-4 * max(1.0, ref_max)
    assert hip[0] <= 1.25 * ac[0] + 1e-6 and hip[1] <= 1.25 * ac[1] + 1e-7


# ---- per-call key of the device-side ancestral noise ---------------------------------------------------
def test_successive_sample_calls_draw_different_ancestral_noise(pc, monkeypatch):
    import brepgen_amd.sampling as smp
    from test_gpu_round2 import SCHED, _build_sampler
    seen = []
    real = smp.device_randn
    monkeypatch.setattr(smp, "device_randn", lambda shape, seed, draw, first, dev: (seen.append((seed, draw)), real(shape, seed, draw, first, dev))[1])
    sampler = _build_sampler(None, False, "device")
    gen = torch.Generator().manual_seed(31)
    a = sampler.sample(2, 6, 5, generator=gen, stop_after="surfPos", **SCHED)
    n1 = len(seen)
    b = sampler.sample(2, 6, 5, generator=gen, stop_after="surfPos", **SCHED)
    keys1, keys2 = {s for s, _ in seen[:n1]}, {s for s, _ in seen[n1:]}
    assert n1 > 0 and len(keys1) == 1 and len(keys2) == 1 and keys1 != keys2          # one key per call, a new one per call
    again = sampler.sample(2, 6, 5, generator=torch.Generator().manual_seed(31), stop_after="surfPos", **SCHED)
    assert torch.equal(a["surfPos"], again["surfPos"]) and not torch.equal(a["surfPos"], b["surfPos"])
