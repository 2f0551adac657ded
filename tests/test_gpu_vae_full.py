"""-m gpu: the full auto-encoders (AutoencoderKL / AutoencoderKL1D), the posterior kernel bg_vae_posterior and the VAE trainers' forward
(training.vae_loss / vae_validation) against fp64 restatements, the Fast classes (bit for bit) and the CPU oracle (oracle/vae.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def pc():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import parity_cases
    return parity_cases


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def posterior(mom, noise, P, L, seed=0, draw=0, first=0, z=None, lv=True, kl=True):
    """bg_vae_posterior on channels-last moments [n, P, 2L] (device); noise [n, L, P] or None.  -> (z [n,P,L], lv [n,P,L] | None, kl [n] | None)."""
    from brepgen_amd import _lib
    n = mom.shape[0]
    z = torch.empty(n, P, L, device="cuda") if z is None else z
    lv = torch.empty(n, P, L, device="cuda") if lv is True else (None if lv is False else lv)
    kl = torch.empty(n, device="cuda") if kl is True else (None if kl is False else kl)
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.load().bg_vae_posterior(mom.data_ptr(), p(noise), n, P, L, seed, draw, first, p(z), p(lv), p(kl), _lib.stream()),
               "bg_vae_posterior")
    return z, lv, kl


def moments(n, P, L, seed):
    """Seeded moments [n, P, 2L]: means up to 1e3, log-variances that make both clamps act; noise [n, L, P]."""
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(n, P, L, generator=g) * torch.tensor([1.0, 30.0, 1e3])[torch.randint(0, 3, (n, 1, 1), generator=g)]
    logvar = torch.randn(n, P, L, generator=g) * 3
    special = torch.tensor([-50.0, -30.0, 0.0, 20.0, 35.0, -30.000002, 20.000002, 1e-4])
    flat = logvar.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:max(len(special), flat.numel() // 3)]
    flat[idx] = special[torch.arange(idx.numel()) % len(special)]
    return torch.cat([mean, logvar], -1).contiguous(), torch.randn(n, L, P, generator=g)


SHAPES = [(5, 16, 3), (7, 4, 3), (3, 5, 3), (1000, 4, 3)]


@pytest.mark.parametrize("n,P,L", SHAPES)
def test_posterior_kernel_vs_fp64(pc, n, P, L):
    mom, eps = moments(n, P, L, 11 + n)
    assert {-50.0, -30.0, 0.0, 20.0, 35.0} <= set(mom[..., L:].reshape(-1).tolist())
    z, lv, kl = posterior(mom.cuda(), eps.cuda(), P, L)
    z2, lv2, kl2 = posterior(mom.cuda(), eps.cuda(), P, L)
    assert torch.equal(z, z2) and torch.equal(lv, lv2) and torch.equal(kl, kl2)              # no atomics: the same bits again
    z, lv, kl = z.cpu(), lv.cpu(), kl.cpu()
    mean, want_lv = mom[..., :L], torch.clamp(mom[..., L:], -30.0, 20.0)
    assert torch.equal(lv.view(torch.int32), want_lv.view(torch.int32))                      # the clamp, bit for bit
    e = eps.transpose(1, 2).double()                                                         # [n, P, L]
    std64 = torch.exp(0.5 * want_lv.double())
    z64 = mean.double() + std64 * e
    budget = 4 * ULP * (mean.double().abs() + std64 * e.abs())                               # <= 2 ulp expf, 1/2 product, 1/2 sum
    over = (z.double() - z64).abs() - budget
    print(f"posterior {n, P, L}: max |z - z64| / budget = {float(((z.double() - z64).abs() / budget).max()):.3f}")
    assert float(over.max()) <= 0
    kl64 = 0.5 * (mean.double() ** 2 + torch.expm1(want_lv.double()) - want_lv.double()).sum((1, 2))
    rel = ((kl.double() - kl64).abs() / kl64.abs()).max()
    print(f"posterior {n, P, L}: max |kl - kl64| / |kl64| = {float(rel):.3e} (bound {ULP:.3e})")
    assert float(rel) <= ULP                                                                 # one rounding of an fp64 result


@pytest.mark.parametrize("n,P,L", SHAPES)
def test_posterior_kernel_draws_device_randn(pc, n, P, L):
    from brepgen_amd import sampling
    mom = moments(n, P, L, 3)[0].cuda()
    seed, draw, first = 0x1234567890ABCDEF, 7, 5
    eps = sampling.device_randn((n, L, P), seed, draw, first, "cuda")
    want = posterior(mom, eps, P, L)
    got = posterior(mom, None, P, L, seed, draw, first)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    lo, hi = n // 3, n - 1                                                                   # a rank's rows of the same draw
    part = posterior(mom[lo:hi].contiguous(), None, P, L, seed, draw, first + lo)
    assert all(torch.equal(a, b[lo:hi]) for a, b in zip(part, got))
    other = posterior(mom, None, P, L, seed, draw + 1, first)
    assert not torch.equal(other[0], got[0]) and torch.equal(other[1], got[1]) and torch.equal(other[2], got[2])


@pytest.mark.parametrize("n,P,L", SHAPES)
def test_posterior_kernel_writes_its_outputs_only(pc, n, P, L):
    from guarded import guarded
    mom, eps = moments(n, P, L, 5)
    mom, eps = mom.cuda(), eps.cuda()
    want = posterior(mom, eps, P, L)
    for noise in (eps, None):
        z, lv, kl = (guarded(s, F32, "cuda") for s in ((n, P * L), (n, P * L), (n,)))
        posterior(mom, noise, P, L, 9, 1, 2, z=z.view.view(n, P, L), lv=lv.view.view(n, P, L), kl=kl.view.view(n))
        torch.cuda.synchronize()
        for name, g in (("z_out", z), ("logvar_out", lv), ("kl_out", kl)):
            g.assert_fully_written(name)
            g.assert_untouched(name)
        assert torch.equal(lv.view.view(n, P, L), want[1]) and torch.equal(kl.view.view(n), want[2])
        if noise is not None:
            assert torch.equal(z.view.view(n, P, L), want[0])
    z = guarded((n, P * L), F32, "cuda")                                                     # the optional outputs left out
    posterior(mom, eps, P, L, z=z.view.view(n, P, L), lv=False, kl=False)
    torch.cuda.synchronize()
    z.assert_fully_written("z_out alone")
    z.assert_untouched("z_out alone")
    assert torch.equal(z.view.view(n, P, L), want[0])


# ---- the modules -----------------------------------------------------------------------------------------------------------------
_CASE = {}


def case(pc, kind):
    """Seeded full checkpoint (the union of the oracle's encoder and decoder specs, as parity_cases.vae_case seeds them), the full
    module and the two Fast modules with the same weights on the device, inputs, and the oracle's moments / decoded sample (CPU, once)."""
    if kind in _CASE:
        return _CASE[kind]
    import brepgen_amd as bga
    from oracle import vae as ov
    surf = kind == "surf"
    n = 2 if surf else 6
    cfg = pc.SURF_CFG if surf else pc.EDGE_CFG
    spec = {**(ov.surf_encoder_spec() if surf else ov.edge_encoder_spec()), **(ov.surf_decoder_spec() if surf else ov.edge_decoder_spec())}
    sd = ov.seeded_state_dict(spec, 71 if surf else 81)
    full = (bga.AutoencoderKL if surf else bga.AutoencoderKL1D)(**cfg)
    full.load_state_dict(sd, strict=True)
    enc = (bga.AutoencoderKLFastEncode if surf else bga.AutoencoderKL1DFastEncode)(**cfg)
    dec = (bga.AutoencoderKLFastDecode if surf else bga.AutoencoderKL1DFastDecode)(**cfg)
    enc.load_state_dict(full.state_dict(), strict=False)
    dec.load_state_dict(full.state_dict(), strict=False)
    g = pc.gen(200 + surf)
    x = torch.randn(n, 3, 32, 32, generator=g) if surf else torch.randn(n, 3, 32, generator=g)
    e = torch.randn(n, 3, 4, 4, generator=g) if surf else torch.randn(n, 3, 4, generator=g)
    with torch.no_grad():
        mom = (ov.surf_encode if surf else ov.edge_encode)(sd, x, latent=6)
        z = mom[:, :3] + torch.exp(0.5 * torch.clamp(mom[:, 3:], -30.0, 20.0)) * e
        out = (ov.surf_decode if surf else ov.edge_decode)(sd, z)
    c = _CASE[kind] = dict(full=full.cuda().eval(), enc=enc.cuda().eval(), dec=dec.cuda().eval(), sd=sd, x=x, e=e, mom=mom, out=out, n=n)
    return c


def _set_dtype(c, dt):
    for m in (c["full"], c["enc"], c["dec"]):
        m.compute_dtype = dt


@pytest.mark.parametrize("kind", ["surf", "edge"])
def test_full_vae_moments_vs_oracle_fp32(pc, kind):
    c = case(pc, kind)
    _set_dtype(c, F32)
    with torch.no_grad():
        got = c["full"].encode(c["x"].cuda()).latent_dist.parameters
    assert got.shape == c["mom"].shape
    e = pc._err(got, c["mom"])
    print(f"{kind} moments fp32: {e}")
    assert e["finite"] and e["max_abs"] < 2e-4 * max(1.0, e["ref_absmax"])                     # the bound of test_vae_encode_fp32


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("kind", ["surf", "edge"])
def test_full_vae_equals_the_fast_classes_bit_for_bit(pc, kind, dt):
    c = case(pc, kind)
    _set_dtype(c, dt)
    m, x, e = c["full"], c["x"].cuda(), c["e"].cuda()
    with torch.no_grad():
        dist = m.encode(x).latent_dist
        assert m.encode(x, return_dict=False)[0].parameters.shape == c["mom"].shape
        assert torch.equal(dist.mode(), c["enc"](x))
        z = dist.sample(noise=e)
        assert torch.equal(m.decode(z).sample, c["dec"](z)) and torch.equal(m.decode(z, return_dict=False)[0], c["dec"](z))
        assert torch.equal(m(x).sample, m.decode(dist.mode()).sample)
        assert torch.equal(m(x, sample_posterior=True, noise=e).sample, m.decode(z).sample)
        assert torch.equal(m(x, True, False, noise=e)[0], m.decode(z).sample)
        assert not torch.equal(z, dist.mode()) and torch.equal(dist.logvar, torch.clamp(dist.parameters[:, 3:], -30.0, 20.0))


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("kind,n", [("surf", 20), ("edge", 96)])
def test_full_vae_encode_program_equals_step_by_step(pc, kind, n, dt):
    """The widened encoder (all 2 * latent moments) through bg_vae_run and through the step-by-step driver of the same walk: the same bits
    (the batch sizes of test_gpu_round2.py::test_vae_program_equals_step_by_step)."""
    from vae_stepwise import stepwise
    c = case(pc, kind)
    _set_dtype(c, dt)
    enc = c["full"]._runners[0]
    x = torch.randn(n, *c["x"].shape[1:], generator=pc.gen(300 + n)).cuda()
    with torch.no_grad():
        a = c["full"].encode(x).latent_dist.parameters
        b = stepwise(enc, x)
    assert a.shape == b.shape == (n, 6, *c["mom"].shape[2:]) and torch.isfinite(a).all() and torch.equal(a, b)


# (max abs, mean abs) error of the fp32 chain encode -> sample(noise) -> decode against the oracle's own chain (|ref|max 3.08 / 2.00), and
# the relative error of vae_loss's (mse, kl) against the oracle chain's values (mse 1.361 / 1.873, kl 12.49 / 7.741): measured once on the
# MI355X with these seeds (every run prints its figures) and asserted at 2x, the convention of test_vae_decode_bf16.  The chain is
# deterministic on both sides, so the figures repeat; the two below 6e-8 are under one fp32 rounding of the returned value.
E2E_MEASURED = {"surf": (1.3247e-05, 2.1609e-06, 1.5859e-08, 5.3705e-07), "edge": (5.8413e-06, 1.1200e-06, 2.0362e-07, 5.7551e-09)}


def e2e_figures(pc, kind):
    from brepgen_amd import training
    c = case(pc, kind)
    _set_dtype(c, F32)
    x, e = c["x"], c["e"]
    with torch.no_grad():
        got = c["full"](x.cuda(), sample_posterior=True, noise=e.cuda()).sample
        r = training.vae_loss(c["full"], x.cuda(), noise=e.cuda())
    err = pc._err(got, c["out"])
    mom = c["mom"].double()
    lv = torch.clamp(mom[:, 3:], -30.0, 20.0)
    dims = tuple(range(1, mom.dim()))
    kl = (0.5 * (mom[:, :3] ** 2 + torch.exp(lv) - 1.0 - lv).sum(dims)).mean()
    mse = ((c["out"].double() - x.double()) ** 2).mean()
    return {"max_abs": err["max_abs"], "mean_abs": err["mean_abs"], "ref_absmax": err["ref_absmax"], "finite": err["finite"],
            "mse_rel": abs(float(r["mse"]) - float(mse)) / float(mse), "kl_rel": abs(float(r["kl"]) - float(kl)) / float(kl),
            "mse": float(mse), "kl": float(kl)}


@pytest.mark.parametrize("kind", ["surf", "edge"])
def test_full_vae_end_to_end_vs_oracle_fp32(pc, kind):
    f = e2e_figures(pc, kind)
    print(f"{kind} end to end fp32: {f}")
    max_abs, mean_abs, mse_rel, kl_rel = E2E_MEASURED[kind]                                  # measured: see E2E_MEASURED; asserted at 2x
    assert f["finite"]
    assert f["max_abs"] < 2 * max_abs and f["mean_abs"] < 2 * mean_abs
    assert f["mse_rel"] < 2 * mse_rel and f["kl_rel"] < 2 * kl_rel


@pytest.mark.parametrize("kind", ["surf", "edge"])
def test_vae_loss_reductions(pc, kind):
    """vae_loss / vae_validation against the trainers' formulas (trainer.py:84-86, 122, 211-216, 252) in fp64 torch on the module's own
    dec, parameters and x; the nets themselves are pinned by the tests above."""
    from brepgen_amd import training
    c = case(pc, kind)
    _set_dtype(c, F32)
    m, x, e, n = c["full"], c["x"].cuda(), c["e"].cuda(), c["n"]
    with torch.no_grad():
        r = training.vae_loss(m, x, noise=e)
        v = training.vae_validation(m, x, noise=e)
        p = m.encode(x).latent_dist.parameters.double()
    dec, xd = r["dec"].double(), x.double()
    dims = tuple(range(1, x.dim()))
    mean, logvar = p[:, :3], torch.clamp(p[:, 3:], -30.0, 20.0)
    kl_ps = 0.5 * torch.sum(torch.pow(mean, 2) + torch.exp(logvar) - 1.0 - logvar, dim=dims)
    mse, kl = float(((dec - xd) ** 2).mean()), float(kl_ps.mean())
    mse_sum = float(((dec - xd) ** 2).mean(dims).sum())
    print(f"{kind} losses: mse {float(r['mse'])!r} vs {mse!r}, kl {float(r['kl'])!r} vs {kl!r}, mse_sum {float(v['mse_sum'])!r} vs {mse_sum!r}")
    assert r["dec"].shape == x.shape and r["kl_per_sample"].shape == (n,) and v["count"] == n
    assert abs(float(r["mse"]) - mse) <= 1e-6 * mse and abs(float(r["kl"]) - kl) <= 1e-6 * kl
    assert float((r["kl_per_sample"].double() - kl_ps).abs().max()) <= 1e-6 * kl
    assert abs(float(r["total"]) - (mse + 1e-6 * kl)) <= 1e-6 * (mse + 1e-6 * kl)
    assert abs(float(v["mse_sum"]) - mse_sum) <= 1e-6 * n
    assert float(r["total"]) == float(r["mse"] + 1e-6 * r["kl"])
    with torch.no_grad():
        # the datasets' layout (points last) is the same computation
        rl = training.vae_loss(m, x.movedim(1, -1).contiguous(), noise=e)
        assert torch.equal(rl["dec"], r["dec"].movedim(1, -1)) and float(rl["total"]) == float(r["total"])
        # kernel-drawn noise: the key is the generator's state
        a = training.vae_loss(m, x, generator=pc.gen(5))
        b = training.vae_loss(m, x, generator=pc.gen(5))
        d = training.vae_loss(m, x, generator=pc.gen(6))
        va, vb = training.vae_validation(m, x, generator=pc.gen(5)), training.vae_validation(m, x, generator=pc.gen(5))
    assert torch.equal(a["dec"], b["dec"]) and float(a["total"]) == float(b["total"]) and float(va["mse_sum"]) == float(vb["mse_sum"])
    assert not torch.equal(a["dec"], d["dec"]) and torch.equal(a["kl_per_sample"], d["kl_per_sample"])


def test_full_vae_chunked_forward_is_batch_independent(pc):
    """The pattern of test_vae_decode_batch_independence for the whole chain with kernel-drawn noise: chunk boundaries change no bit, and
    a row run alone under its global index reproduces its row of the batch."""
    import brepgen_amd as bga
    from oracle import vae as ov
    sd = ov.seeded_state_dict({**ov.edge_encoder_spec(), **ov.edge_decoder_spec()}, 77)
    m = bga.AutoencoderKL1D(**pc.EDGE_CFG)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.compute_dtype = F32
    x = torch.randn(40, 3, 32, generator=pc.gen(3)).cuda()
    g = pc.gen(9)
    with torch.no_grad():
        full = m(x, sample_posterior=True, generator=g).sample
        m.WS_BUDGET = 1 << 22                           # force several chunks inside bg_vae_run
        m.release_workspace()
        chunked = m(x, sample_posterior=True, generator=g).sample
        one = m.decode(m.encode(x[17:18]).latent_dist.sample(generator=g, first_sample=17)).sample
        shifted = m.decode(m.encode(x[17:18]).latent_dist.sample(generator=g, first_sample=16)).sample
    assert torch.isfinite(full).all() and torch.equal(full, chunked)
    assert float((full[17:18] - one).abs().max()) < 1e-5 < float((full[17:18] - shifted).abs().max())
