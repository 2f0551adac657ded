#!/usr/bin/env python
"""Surface sampling (bg_mesh_sample, csrc/mesh_sample.hip) on a synthetic evaluation set: `--meshes` triangle soups of about `--triangles`
triangles each, `--points` points per mesh, in ONE call of brepgen_amd.sample_points.sample_meshes.  Beside the time: the bytes such a call
has to move at the nominal HBM rate, and the wall time of a numpy restatement of the same sampler on this host for the same set.

    python tools/mesh_sample_bench.py [--meshes 3000 --triangles 5000 --points 2000 --repeats 5 --out mesh_sample.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_NOMINAL = 8.0e12                        # MI355X datasheet rate, B/s
LDS_TABLE_CAP = 6144                        # csrc/mesh_sample.hip MS_CAP: larger meshes keep their running sum in the workspace


def numpy_sampler(tri, u):
    """fp64 areas and running sum, searchsorted, trimesh's reflected placement in fp32 (what tests/test_gpu_mesh_sample.py compares with)."""
    t = tri.astype(np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    cdf = np.cumsum(0.5 * np.sqrt((n * n).sum(1)))
    face = np.minimum(np.searchsorted(cdf, u[:, 0] * cdf[-1], side="right"), len(tri) - 1)
    r1, r2 = u[:, 1].astype(np.float32), u[:, 2].astype(np.float32)
    flip = (r1 + r2) > np.float32(1.0)
    r1, r2 = np.where(flip, np.float32(1.0) - r1, r1)[:, None], np.where(flip, np.float32(1.0) - r2, r2)[:, None]
    a = tri[face, 0]
    return (a + r1 * (tri[face, 1] - a)) + r2 * (tri[face, 2] - a), face


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=3000)
    ap.add_argument("--triangles", type=int, default=5000, help="mean; sizes are uniform in [0.8, 1.2] x this")
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the record to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_sample_bench needs the GPU: a CPU run measures nothing")
    from brepgen_amd import _lib, sample_points
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(1)
    sizes = rng.integers(int(0.8 * args.triangles), int(1.2 * args.triangles) + 1, size=args.meshes)
    gen = torch.Generator(device=dev).manual_seed(2)
    meshes = list(torch.randn(int(sizes.sum()), 3, 3, device=dev, generator=gen).split(sizes.tolist()))
    T, M, P = int(sizes.sum()), args.meshes, args.points

    sample_points.sample_meshes(meshes[:8], P, seed=3)                              # code object, allocator
    first = sample_points.sample_meshes(meshes, P, seed=3)                          # one full-size warm-up
    torch.cuda.synchronize()
    call_s, kernel_ms = [], []
    for _ in range(max(5, args.repeats)):
        with _lib.profile() as prof:
            t0 = time.perf_counter()
            out = sample_points.sample_meshes(meshes, P, seed=3)                    # ends in a device read (the area check)
            torch.cuda.synchronize()
            call_s.append(time.perf_counter() - t0)
        kernel_ms.append(sum(r["total_ms"] for r in prof.rows))
        assert torch.equal(out[0], first[0]) and torch.equal(out[1], first[1]), "the clouds changed between two runs"
    med = lambda v: sorted(v)[len(v) // 2]

    host = [m.cpu().numpy() for m in meshes]
    u = rng.random((M, P, 3))
    t0 = time.perf_counter()
    ref = [numpy_sampler(host[i], u[i]) for i in range(M)]
    numpy_s = time.perf_counter() - t0
    given = sample_points.sample_meshes(meshes[:16], P, uniforms=u[:16])
    same = all(np.array_equal(given[1][i].cpu().numpy(), ref[i][1]) and given[0][i].cpu().numpy().tobytes() == ref[i][0].tobytes()
               for i in range(16))

    must_move = 36.0 * T + 16.0 * T + 28.0 * M * P
    in_ws = int(sizes[sizes > LDS_TABLE_CAP].sum())
    rec = {"meshes": M, "triangles_total": T, "triangles_per_mesh": [int(sizes.min()), int(sizes.max())], "points_per_mesh": P,
           "device": torch.cuda.get_device_name(dev),
           "sample_meshes_call_s": round(med(call_s), 5), "sample_meshes_call_all_repeats_s": [round(v, 5) for v in call_s],
           "call_timing": "host clock around sample_meshes on device tensors (concatenation, offsets, allocation, the launch, the area "
                          "check that reads the device) + synchronize; one full-size warm-up, median of the repeats",
           "bg_mesh_sample_kernel_ms": round(med(kernel_ms), 4), "bg_mesh_sample_kernel_all_repeats_ms": [round(v, 4) for v in kernel_ms],
           "kernel_timing": "hipEvent pair around the launch (bg_profile_begin / bg_profile_end), same repeats",
           "bytes_the_call_must_move": must_move,
           "bytes_formula": "36 B per triangle read + 16 B per triangle of workspace traffic + 28 B per point written",
           "triangles_whose_table_goes_through_the_workspace": in_ws,
           "time_at_nominal_8TBps_ms": round(must_move / HBM_NOMINAL * 1e3, 4),
           "kernel_fraction_of_that_rate": round(must_move / HBM_NOMINAL / (med(kernel_ms) / 1e3), 4),
           "numpy_restatement_same_host_s": round(numpy_s, 3),
           "numpy_restatement": "one thread: per mesh np.cross / cumsum / searchsorted / fp32 placement, meshes already in host memory",
           "first_16_clouds_equal_numpy_bitwise_with_given_uniforms": bool(same),
           "note": "none of these figures existed before bg_mesh_sample: nothing in the project preceded this kernel"}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
