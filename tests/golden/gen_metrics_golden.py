#!/usr/bin/env python
"""Generate the evaluation-metric fixtures ``tests/golden/metrics_*.npz`` from the REFERENCE's own ``pc_metric.py``.

Runs on the CPU where the reference checkout is (the ``BREPGEN_REFERENCE`` environment variable names it), like gen_golden.py.
``pc_metric.py`` imports two packages that are not installable here; both are stubbed in ``sys.modules``:

    plyfile            never called by the functions used here
    chamfer_distance   ``ChamferDistance()(a, b)`` delegates to the reference's OWN pure-torch ``distChamfer`` (pc_metric.py:32-42),
                       which states the same quantity; (dl, dr) = (min over b per a point, min over a per b point)

Per case the file holds the input clouds (points on random boxes through the reference's ``normalize_pc``, stored as fp32), the
reference's [S, R] Chamfer matrix, MMD, COV, occupancy counters, entropy and JSD, the direct-form matrix in fp64 and ``ref_dev``, the
largest relative deviation of the reference's fp32 matrix from the fp64 one -- the yardstick of tests/test_gpu_metrics.py.
The ``cloud_counts`` (the reference's grid_bernoulli_rvars, which it does not return) are recounted here with the reference's grid
and the same sklearn nearest-neighbour search.

The generator asserts on its own inputs: (1) in fp64 every row's and column's best-to-second-best gap is >= 1000 x ref_dev
(relative), so fp32 cannot legitimately flip an argmin; (2) 0 < COV < 1.

    BREPGEN_REFERENCE=<reference checkout> python tests/golden/gen_metrics_golden.py
"""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("BREPGEN_REFERENCE", "")
OUT = os.path.join(ROOT, "tests", "golden")
RESOLUTION = 28

# (name, seed, S, R, Pa, Pb): more reference clouds than samples keeps COV < 1
CASES = [("metrics_p2000", 11, 4, 8, 2000, 2000),
         ("metrics_p256", 12, 12, 20, 256, 256),
         ("metrics_mixed", 13, 5, 7, 300, 500)]          # Pa != Pb: distChamfer does not cover it -> fp64 only


def import_reference():
    assert os.path.isdir(REF), "set BREPGEN_REFERENCE to the reference checkout"
    ply = types.ModuleType("plyfile")
    ply.PlyData = object
    sys.modules["plyfile"] = ply
    class ChamferDistance:
        def __call__(self, a, b):
            over_a, over_b = sys.modules["pc_metric"].distChamfer(a, b)      # min over a per b point, min over b per a point
            return over_b, over_a, None, None

    cd = types.ModuleType("chamfer_distance")
    cd.ChamferDistance = ChamferDistance
    sys.modules["chamfer_distance"] = cd
    sys.path.insert(0, REF)
    import pc_metric
    return pc_metric


def box_cloud(rng, n):
    """n points on the surface of a random axis-aligned box, somewhere off the origin (normalize_pc centres and scales it)."""
    half = rng.uniform(0.15, 1.0, size=3)
    centre = rng.uniform(-0.5, 0.5, size=3)
    pts = rng.uniform(-1.0, 1.0, size=(n, 3)) * half
    face = rng.integers(0, 3, size=n)
    pts[np.arange(n), face] = np.where(rng.random(n) < 0.5, -1.0, 1.0) * half[face]
    return pts + centre


def chamfer_fp64(a, b):
    out = np.zeros((len(a), len(b)))
    for i, x in enumerate(a.astype(np.float64)):
        for j, y in enumerate(b.astype(np.float64)):
            d = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
            out[i, j] = d.min(1).mean() + d.min(0).mean()
    return out


def smallest_relative_gap(m):
    """Over all rows and columns: (second best - best) / best."""
    gaps = []
    for mat in (m, m.T):
        s = np.sort(mat, axis=1)
        gaps.append(((s[:, 1] - s[:, 0]) / s[:, 0]).min())
    return float(min(gaps))


def cloud_counts(pm, clouds):
    """grid_bernoulli_rvars of pc_metric.py:128-139 (the reference computes it but returns only what it derives from it)."""
    from sklearn.neighbors import NearestNeighbors
    grid = pm.unit_cube_grid_point_cloud(RESOLUTION, False)[0].reshape(-1, 3)
    nn = NearestNeighbors(n_neighbors=1).fit(grid)
    out = np.zeros(len(grid), dtype=np.int64)
    for pc in clouds:
        out[np.unique(nn.kneighbors(pc)[1])] += 1
    return out


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps: the same arrays give the same file, byte for byte."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(1)
    pm = import_reference()
    for name, seed, S, R, Pa, Pb in CASES:
        rng = np.random.default_rng(seed)
        sample = np.stack([pm.normalize_pc(box_cloud(rng, Pa)) for _ in range(S)]).astype(np.float32)
        ref = np.stack([pm.normalize_pc(box_cloud(rng, Pb)) for _ in range(R)]).astype(np.float32)
        fp64 = chamfer_fp64(sample, ref)
        arrays = {"sample": sample, "ref": ref, "cd_fp64": fp64}
        gap = smallest_relative_gap(fp64)
        if Pa == Pb:
            with torch.no_grad():
                ts, tr = torch.from_numpy(sample), torch.from_numpy(ref)
                cd_ref = pm._pairwise_CD(ts, tr, 64).numpy()
                res = pm.compute_cov_mmd(ts, tr, 64)
            ref_dev = float((np.abs(cd_ref.astype(np.float64) - fp64) / fp64).max())
            assert gap >= 1000 * ref_dev, (name, gap, ref_dev)
            assert 0 < res["COV-CD"] < 1, (name, res)
            assert np.float32(len(np.unique(fp64.argmin(1))) / R) == np.float32(res["COV-CD"]), name     # fp64 agrees on the matches
            arrays.update(cd_ref=cd_ref, ref_dev=np.float64(ref_dev), mmd=np.float64(res["MMD-CD"]), cov=np.float64(res["COV-CD"]))
        else:
            ref_dev = None
        ent_s, cnt_s = pm.entropy_of_occupancy_grid(sample, RESOLUTION, False)
        ent_r, cnt_r = pm.entropy_of_occupancy_grid(ref, RESOLUTION, False)
        jsd = pm.jsd_between_point_cloud_sets(sample, ref, False, RESOLUTION)
        arrays.update(resolution=np.int64(RESOLUTION), entropy_sample=np.float64(ent_s), entropy_ref=np.float64(ent_r),
                      point_counts_sample=cnt_s.astype(np.int64), point_counts_ref=cnt_r.astype(np.int64),
                      cloud_counts_sample=cloud_counts(pm, sample), cloud_counts_ref=cloud_counts(pm, ref), jsd=np.float64(jsd))
        # normalize_pc on a raw (un-normalised) cloud, for the CPU test of brepgen_amd.metrics.normalize_pc
        raw = box_cloud(rng, 64) * 3.0 + 0.25
        arrays.update(raw=raw, raw_normalized=pm.normalize_pc(raw))
        path = os.path.join(OUT, name + ".npz")
        save_npz(path, arrays)
        print(f"{name}: S={S} R={R} Pa={Pa} Pb={Pb}  ref_dev={ref_dev}  smallest gap={gap:.3e}  jsd={float(jsd):.6f}  "
              f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
