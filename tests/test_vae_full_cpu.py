"""The full auto-encoders (brepgen_amd.vae.AutoencoderKL / AutoencoderKL1D), their posterior entry bg_vae_posterior and the two VAE
trainers' forward (brepgen_amd.training.vae_loss / vae_validation): everything that can be checked without a GPU -- the checkpoint
key layout, the ABI declaration, the argument checks, the programs' shape, and that nothing falls back to the CPU."""
import ctypes as C
import os
import re

import pytest
import torch

import brepgen_amd as bga
from brepgen_amd import _lib, training, vae
from brepgen_amd.pipeline import EDGE_VAE_CFG, SURF_VAE_CFG
from oracle import vae as ov

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("AutoencoderKL", SURF_VAE_CFG, ov.surf_encoder_spec, ov.surf_decoder_spec, "AutoencoderKLFastEncode", "AutoencoderKLFastDecode"),
         ("AutoencoderKL1D", EDGE_VAE_CFG, ov.edge_encoder_spec, ov.edge_decoder_spec, "AutoencoderKL1DFastEncode",
          "AutoencoderKL1DFastDecode")]


@pytest.mark.parametrize("cls,cfg,enc_spec,dec_spec,fast_enc,fast_dec", CASES)
def test_full_vae_keys_are_the_union_of_the_encoder_and_decoder_checkpoints(cls, cfg, enc_spec, dec_spec, fast_enc, fast_dec):
    m = getattr(bga, cls)(**cfg)
    spec = {**enc_spec(), **dec_spec()}
    sd = m.state_dict()
    assert set(sd) == set(spec)
    for k, shape in spec.items():
        assert tuple(sd[k].shape) == tuple(shape), k
    assert {n for n, _ in m.named_children()} == {"encoder", "decoder", "quant_conv", "post_quant_conv"}
    ckpt = ov.seeded_state_dict(spec, 5)
    m.load_state_dict(ckpt, strict=True)
    assert all(torch.equal(m.state_dict()[k], ckpt[k]) for k in ckpt)
    for fast in (fast_enc, fast_dec):                              # sample.py:83,98 and trainer.py:521,925 load the same file strict=False
        r = getattr(bga, fast)(**cfg).load_state_dict(m.state_dict(), strict=False)
        assert not r.missing_keys and r.unexpected_keys


@pytest.mark.parametrize("cls,cfg,shape", [("AutoencoderKL", SURF_VAE_CFG, (32, 32, 3)), ("AutoencoderKL1D", EDGE_VAE_CFG, (1, 32, 3))])
def test_full_vae_encode_program_writes_all_moments(cls, cfg, shape):
    """The full classes run the Fast encoder's program with the last convolution widened from `latent` to 2 * latent columns."""
    m = getattr(bga, cls)(**cfg)
    enc, dec = m._runners
    fast = type(enc)(**cfg)
    assert fast.n_out == fast.latent == 3 and enc.n_out == 6
    pg, pg_fast = (e._program(vae._Program(), e._pack(torch.float32)).finish() for e in (enc, fast))
    assert len(pg.steps) == len(pg_fast.steps)
    assert pg.steps[-1].n_out == 6 and pg_fast.steps[-1].n_out == 3 and pg.steps[-1].dst == vae.VAE_OUT
    assert [(a.op, a.src, a.dst, a.n_out) for a in pg.steps[:-1]] == [(a.op, a.src, a.dst, a.n_out) for a in pg_fast.steps[:-1]]
    assert _lib.load().bg_vae_workspace_bytes(pg.ops, len(pg.steps), pg.n_slots, *shape, 8, 8) > 0
    # the switches of the program runners are set through the full module
    m.compute_dtype, m.WS_BUDGET = torch.bfloat16, 1 << 22
    assert all(r.compute_dtype == torch.bfloat16 and r.WS_BUDGET == 1 << 22 for r in (enc, dec))
    m.load_state_dict(m.state_dict())
    assert not enc._packs and not enc._programs


_CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "bg_stream_t": C.c_void_p, "long long": C.c_longlong, "int": C.c_int,
          "unsigned long long": C.c_ulonglong, "unsigned": C.c_uint}


def test_posterior_entry_is_exported_with_the_headers_signature():
    assert "bg_vae_posterior" in _lib.EXPORTS and hasattr(_lib.load(), "bg_vae_posterior")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "brepgen_hip.h")).read(), flags=re.S)
    ret, params = re.search(r"(\w+)\s+bg_vae_posterior\s*\(([^)]*)\)\s*;", src).groups()
    types = [re.sub(r"\s+", " ", re.sub(r"\w+\s*$", "", p.strip())).strip() for p in params.split(",")]
    res, args = _lib._SIGNATURES["bg_vae_posterior"]
    assert ret == "int" and res is C.c_int
    assert [_CTYPE[t] for t in types] == args
    assert _lib.ABI_VERSION == 7                                   # an added entry: no bump


def test_posterior_argument_errors_are_negative_and_explained():
    lib = _lib.load()
    fake = 0x10000                                                 # never dereferenced: validation fails (or n == 0 returns) first

    def f(moments=fake, noise=None, n=4, P=16, L=3, first=0, z=fake):
        return lib.bg_vae_posterior(moments, noise, n, P, L, 1, 0, first, z, None, None, None)

    for kw in (dict(moments=None), dict(z=None)):
        assert f(**kw) == _lib.BG_E_ARG and b"null" in lib.bg_last_error(), kw
    for kw in (dict(n=-1), dict(P=0), dict(L=0), dict(P=-4), dict(first=-1)):
        assert f(**kw) == _lib.BG_E_SHAPE and b"bad shape" in lib.bg_last_error(), kw
    assert f(P=70000, L=70000) == _lib.BG_E_SHAPE and b"Philox" in lib.bg_last_error()
    assert f(P=1 << 30, L=2) == _lib.BG_E_SHAPE
    assert f(n=0) == 0 and f(n=0, noise=fake) == 0                 # nothing to do: no launch


def test_posterior_object_keeps_the_reference_layout():
    p = torch.randn(2, 6, 4, 4, generator=torch.Generator().manual_seed(0))
    d = bga.DiagonalGaussianDistribution(p)
    assert torch.equal(d.parameters, p) and torch.equal(d.mean, p[:, :3]) and torch.equal(d.mode(), p[:, :3])
    p1 = torch.randn(5, 6, 4, generator=torch.Generator().manual_seed(1))
    d1 = bga.DiagonalGaussianDistribution(p1)
    assert torch.equal(d1.parameters, p1) and torch.equal(d1.mean, p1[:, :3])


def test_full_vae_has_no_cpu_fallback():
    surf, edge = bga.AutoencoderKL(**SURF_VAE_CFG), bga.AutoencoderKL1D(**EDGE_VAE_CFG)
    for m, x, z in ((surf, torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 4, 4)), (edge, torch.zeros(2, 3, 32), torch.zeros(2, 3, 4))):
        for call in (lambda: m.encode(x), lambda: m.decode(z), lambda: m(x), lambda: m(x, sample_posterior=True),
                     lambda: training.vae_loss(m, x), lambda: training.vae_validation(m, x),
                     lambda: training.vae_loss(m, x.movedim(1, -1)), lambda: training.vae_validation(m, x.movedim(1, -1))):
            with pytest.raises(_lib.BrepgenHipError):
                call()
    d = bga.DiagonalGaussianDistribution(torch.zeros(2, 6, 4, 4))
    for call in (lambda: d.sample(), lambda: d.sample(noise=torch.zeros(2, 3, 4, 4)), lambda: d.sample(seed=3), lambda: d.kl(),
                 lambda: d.logvar):
        with pytest.raises(_lib.BrepgenHipError):
            call()
