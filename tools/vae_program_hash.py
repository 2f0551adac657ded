#!/usr/bin/env python
"""What the VAE modules compile themselves into, as one line per network and dtype: step count, slot count and a SHA-256 over the
whole bg_vae_op program -- every non-pointer field of every step in declaration order and, for each pointer field, the bytes of the
tensor it points to (found by data_ptr() among the program's `keep` list and the module's packs; a pointer nothing owns is counted
and fails the run).  Two trees whose outputs are equal hand bg_vae_run the same programs over the same weights.  Last line: host time of
compiling the surface decoder in bf16 from a cold pack cache (median of 5; on stderr, so that the outputs diff clean).  Needs neither a GPU nor the built library.

    python tools/vae_program_hash.py > after.txt        # and the same on the other tree; diff the two
"""
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import brepgen_amd as bga  # noqa: E402
from brepgen_amd import _lib, vae  # noqa: E402
from brepgen_amd.pipeline import EDGE_VAE_CFG, SURF_VAE_CFG  # noqa: E402  (= tests/parity_cases.SURF_CFG / EDGE_CFG)

POINTERS = ("w", "bias", "gn_gamma", "gn_beta", "w2", "bias2")
CASES = [("AutoencoderKLFastDecode", SURF_VAE_CFG, False), ("AutoencoderKL1DFastDecode", EDGE_VAE_CFG, False),
         ("AutoencoderKLFastEncode", SURF_VAE_CFG, False), ("AutoencoderKL1DFastEncode", EDGE_VAE_CFG, False),
         ("AutoencoderKLFastEncode", SURF_VAE_CFG, True), ("AutoencoderKL1DFastEncode", EDGE_VAE_CFG, True)]


def _tensors(v):
    """Every tensor a pack cache holds, whatever its keys and however it groups the packs of one module."""
    if isinstance(v, torch.Tensor):
        yield v
    elif isinstance(v, vae._Packed):
        yield v.w
        yield v.b
    elif isinstance(v, dict):
        for x in v.values():
            yield from _tensors(x)
    elif isinstance(v, (tuple, list)):
        for x in v:
            yield from _tensors(x)


def program_hash(m, pg, packs):
    owner = {t.data_ptr(): t for t in [*_tensors(packs), *pg.keep]}
    h, unresolved = hashlib.sha256(), 0
    for o in pg.steps:
        for name, _ in _lib.VaeOp._fields_:
            v = getattr(o, name)
            if name not in POINTERS:
                h.update(f"{name}={v!r};".encode())
            elif not v:
                h.update(f"{name}=null;".encode())
            elif v in owner:
                t = owner[v]
                h.update(f"{name}={t.dtype}{tuple(t.shape)}:".encode())
                h.update(t.contiguous().view(torch.uint8).numpy().tobytes())
            else:
                unresolved += 1
    return h.hexdigest(), unresolved


def main():
    bad = 0
    for cls, cfg, widened in CASES:
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            torch.manual_seed(0)
            m = getattr(bga, cls)(**cfg)
            if widened:
                m.n_out = 2 * m.latent
            packs = m._pack(dt)
            pg = m._program(vae._Program(), packs).finish()
            digest, unresolved = program_hash(m, pg, packs)
            bad += unresolved
            print(f"{cls}{'[n_out=2*latent]' if widened else ''} {str(dt).split('.')[1]}: steps {len(pg.steps)} n_slots {pg.n_slots} "
                  f"sha256 {digest} unresolved {unresolved}")
    torch.manual_seed(0)
    m = bga.AutoencoderKLFastDecode(**SURF_VAE_CFG)
    times = []
    for _ in range(5):
        m._packs = {}
        t0 = time.perf_counter()
        m._program(vae._Program(), m._pack(torch.bfloat16)).finish()
        times.append(time.perf_counter() - t0)
    print(f"# AutoencoderKLFastDecode bf16 _program(_Program(), _pack(dt)), cold pack cache, median of 5: {statistics.median(times) * 1e3:.1f} ms",
          file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
