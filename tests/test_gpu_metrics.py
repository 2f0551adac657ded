"""-m gpu: the evaluation metrics on the device (csrc/metrics.hip through brepgen_amd/metrics.py).

ACCURACY RULE of the Chamfer matrix -- no invented tolerance; the yardstick is the reference's own fp32 formulation
(|x|^2 + |y|^2 - 2 x.y, pc_metric.py:32-42) on the same inputs:

    |out - fp64| / fp64  <=  max(ref_dev, 64 * 2^-24)        for every entry

ref_dev = largest relative deviation of that fp32 formulation from the direct form in fp64: stored in the fixtures
(tests/golden/gen_metrics_golden.py), recomputed here for the live cases.  64 * 2^-24 is the floor that keeps the rule meaningful where the
reference happens to be exact (P = 1): <= 5 roundings per direct-form distance plus a summation tree of depth <= 59.  fp64 == 0 (identical
clouds) demands exactly 0.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FLOOR = 64 * 2.0 ** -24


@pytest.fixture(scope="module")
def m():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from brepgen_amd import metrics
    return metrics


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def chamfer_fp64(a, b):
    """Direct form in fp64 on the CPU."""
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    out = np.zeros((len(a), len(b)))
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            rows, cols = [], torch.full((len(y),), float("inf"), dtype=torch.float64)
            for p0 in range(0, len(x), 512):
                d = (x[p0:p0 + 512, None, :] - y[None, :, :]).pow(2).sum(-1)
                rows.append(d.min(1).values)
                cols = torch.minimum(cols, d.min(0).values)
            out[i, j] = float(torch.cat(rows).mean() + cols.mean())
    return out


def reference_fp32(a, b):
    """The reference's formulation restated (fp32, CPU): expanded squared distances, then the two minima."""
    a, b = torch.as_tensor(a, dtype=torch.float32), torch.as_tensor(b, dtype=torch.float32)
    out = np.zeros((len(a), len(b)), np.float32)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            P = (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2 * (x @ y.T)
            out[i, j] = float(P.min(1).values.mean() + P.min(0).values.mean())
    return out


def check_rule(what, out, fp64, ref_dev):
    out = np.asarray(out, dtype=np.float64)
    zero = fp64 == 0
    dev = float((np.abs(out - fp64)[~zero] / fp64[~zero]).max()) if (~zero).any() else 0.0
    bound = max(float(ref_dev), FLOOR)
    print(f"{what}: max relative deviation from fp64 = {dev:.3e}  (ref_dev {float(ref_dev):.3e}, bound {bound:.3e})")
    assert np.all(out[zero] == 0.0), what
    assert np.isfinite(out).all() and dev <= bound, (what, dev, bound)
    return dev


def clouds(rng, n, P):
    pts = rng.uniform(-1.0, 1.0, size=(n, P, 3))
    return (pts / np.abs(pts).max(axis=(1, 2), keepdims=True)).astype(np.float32)


# ---- 1. golden matrices, COV, MMD ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["metrics_p2000", "metrics_p256"])
def test_golden_matrix_cov_mmd(m, name):
    g = golden(name)
    out = m.pairwise_chamfer(g["sample"], g["ref"])
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (len(g["sample"]), len(g["ref"]))
    check_rule(name, out.cpu().numpy(), g["cd_fp64"], g["ref_dev"])
    res = m.compute_cov_mmd(torch.from_numpy(g["sample"]), torch.from_numpy(g["ref"]), batch_size=64)
    assert set(res) == {"MMD-CD", "COV-CD"}
    mmd64 = g["cd_fp64"].min(0).mean()
    print(f"{name}: COV {res['COV-CD']!r} (reference {float(g['cov'])!r})  MMD {res['MMD-CD']!r} (reference {float(g['mmd'])!r}, fp64 {mmd64!r})")
    assert res["COV-CD"] == float(g["cov"])                                           # exactly the reference's
    assert abs(res["MMD-CD"] - mmd64) / mmd64 <= max(float(g["ref_dev"]), FLOOR)
    assert m.compute_cov_mmd(g["sample"], g["ref"]) == res                            # numpy input, no batch_size: the same


def test_golden_matrix_unequal_point_counts(m):
    g = golden("metrics_mixed")
    a, b = g["sample"], g["ref"]
    assert a.shape[1] != b.shape[1]
    check_rule("metrics_mixed", m.pairwise_chamfer(a, b).cpu().numpy(), g["cd_fp64"], 0.0)


# ---- 2. live shapes against fp64 ------------------------------------------------------------------------------------------------
LIVE = [(1, 1, 1, 1), (7, 1, 63, 63), (1, 5, 64, 64), (5, 9, 65, 65), (3, 17, 257, 257), (2, 3, 2049, 2049),      # (S, R, Pa, Pb)
        (3, 4, 100, 257), (4, 3, 1, 300), (3, 2, 300, 1), (33, 65, 64, 63), (2, 3, 2047, 2050), (2, 2, 2048, 4097), (2, 3, 2049, 500),
        (3, 2, 500, 2049), (1, 2, 4100, 2048)]


@pytest.mark.parametrize("S,R,Pa,Pb", LIVE)
def test_live_shapes_against_fp64(m, S, R, Pa, Pb):
    rng = np.random.default_rng(1000 * S + 100 * R + Pa + 7 * Pb)
    a, b = clouds(rng, S, Pa), clouds(rng, R, Pb)
    fp64 = chamfer_fp64(a, b)
    ref = reference_fp32(a, b).astype(np.float64)
    ref_dev = float((np.abs(ref - fp64) / fp64).max())
    check_rule(f"S={S} R={R} Pa={Pa} Pb={Pb}", m.pairwise_chamfer(a, b).cpu().numpy(), fp64, ref_dev)


@pytest.mark.parametrize("P", [65, 300, 2100])
def test_duplicated_points_and_identical_clouds(m, P):
    rng = np.random.default_rng(P)
    a = clouds(rng, 4, P)
    a[1, P // 2:] = a[1, :P - P // 2]                    # a cloud whose second half repeats its first half
    a[2, :] = a[2, 0]                                    # one point, P times
    b = np.concatenate([a, clouds(rng, 2, P)])           # b_0 .. b_3 ARE a_0 .. a_3
    out = m.pairwise_chamfer(a, b).cpu().numpy()
    assert np.all(np.diagonal(out) == 0.0), np.diagonal(out)          # identical clouds: exactly 0
    fp64 = chamfer_fp64(a, b)
    ref_dev = float(np.nanmax(np.where(fp64 > 0, np.abs(reference_fp32(a, b) - fp64) / np.where(fp64 > 0, fp64, 1), 0)))
    check_rule(f"duplicates P={P}", out, fp64, ref_dev)


def test_more_pairs_than_one_launch_carries(m):
    """bg_chamfer_pairwise slices S * R into launches of 2^22 cloud pairs: 2050 x 2050 pairs of two-point clouds cross that seam.  Every
    entry against fp64 (numpy, vectorised), and rows on both sides of the seam bitwise against a call of their own."""
    rng = np.random.default_rng(2050)
    a, b = clouds(rng, 2050, 2), clouds(rng, 2050, 2)
    assert a.shape[0] * b.shape[0] > 1 << 22
    d = ((a.astype(np.float64)[:, None, :, None, :] - b.astype(np.float64)[None, :, None, :, :]) ** 2).sum(-1)      # [S, R, 2, 2]
    fp64 = d.min(3).mean(2) + d.min(2).mean(2)
    out = m.pairwise_chamfer(a, b).cpu()
    check_rule("2050 x 2050 clouds of 2 points", out.numpy(), fp64, 0.0)
    seam = (1 << 22) // 2050                              # the row the second launch starts in
    assert torch.equal(m.pairwise_chamfer(a[seam - 1:seam + 2], b).cpu(), out[seam - 1:seam + 2])
    assert torch.equal(m.pairwise_chamfer(a[-3:], b[-5:]).cpu(), out[-3:, -5:])


# ---- 3. / 4. bitwise batch independence and determinism -------------------------------------------------------------------------
@pytest.mark.parametrize("Pa,Pb", [(300, 300), (257, 100), (2100, 700)])
def test_entries_depend_on_their_two_clouds_only(m, Pa, Pb):
    rng = np.random.default_rng(Pa + Pb)
    S, R = (9, 11) if Pa < 2048 else (4, 5)
    a, b = clouds(rng, S, Pa), clouds(rng, R, Pb)
    full = m.pairwise_chamfer(a, b).cpu()
    assert torch.equal(m.pairwise_chamfer(a[2:4], b).cpu(), full[2:4])                    # row slice
    assert torch.equal(m.pairwise_chamfer(a, b[1:4]).cpu(), full[:, 1:4])                 # column slice
    assert torch.equal(m.pairwise_chamfer(a[3:4], b[4:5]).cpu(), full[3:4, 4:5])          # one pair on its own
    pr, pc = rng.permutation(S), rng.permutation(R)
    assert torch.equal(m.pairwise_chamfer(a[pr], b[pc]).cpu(), full[pr][:, pc])           # another order
    both = np.concatenate([a[:, :min(Pa, Pb)], b[:, :min(Pa, Pb)]])
    sq = m.pairwise_chamfer(both, both).cpu()
    assert torch.equal(torch.diagonal(sq), torch.zeros(len(both)))


def test_run_to_run_determinism_on_two_streams(m):
    g = golden("metrics_p2000")
    a, b = torch.from_numpy(g["sample"]).cuda(), torch.from_numpy(g["ref"]).cuda()
    first = m.pairwise_chamfer(a, b)
    second = m.pairwise_chamfer(a, b)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third = m.pairwise_chamfer(a, b)
    side.synchronize()
    assert torch.equal(first, second) and torch.equal(first, third)


# ---- 5. / 6. occupancy counts, entropy, JSD -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["metrics_p2000", "metrics_p256", "metrics_mixed"])
def test_occupancy_counts_entropy_and_jsd_equal_the_reference(m, name):
    g = golden(name)
    res = int(g["resolution"])
    for which in ("sample", "ref"):
        points, per_cloud = m.occupancy_counts(g[which], res)
        assert np.array_equal(points, g["point_counts_" + which]) and np.array_equal(per_cloud, g["cloud_counts_" + which])
        ent, counters = m.entropy_of_occupancy_grid(g[which], res)
        assert counters.dtype == np.float64 and np.array_equal(counters, g["point_counts_" + which])
        assert abs(ent - float(g["entropy_" + which])) <= 1e-12 * float(g["entropy_" + which])
    jsd = m.jsd_between_point_cloud_sets(g["sample"], g["ref"], in_unit_sphere=False, resolution=res)
    print(f"{name}: JSD {jsd!r} (reference {float(g['jsd'])!r})")
    assert abs(jsd - float(g["jsd"])) <= 1e-12 * float(g["jsd"])
    assert m.jsd_between_point_cloud_sets(torch.from_numpy(g["sample"]), torch.from_numpy(g["ref"])) == jsd     # resolution=28 default


def brute_force_counts(pts, res):
    """Nearest node of the full res^3 grid in fp64, first (lowest) index on a tie."""
    from brepgen_amd.metrics import grid_axis
    ax = grid_axis(res).astype(np.float64)
    grid = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    points, per_cloud = np.zeros(res ** 3, np.int64), np.zeros(res ** 3, np.int64)
    for cloud in pts.astype(np.float64):
        cells = np.concatenate([((cloud[p0:p0 + 8, None, :] - grid[None]) ** 2).sum(-1).argmin(1) for p0 in range(0, len(cloud), 8)])
        np.add.at(points, cells, 1)
        per_cloud[np.unique(cells)] += 1
    return points, per_cloud


@pytest.mark.parametrize("res", [2, 28, 64])
def test_occupancy_counts_equal_a_brute_force_search(m, res):
    from brepgen_amd.metrics import grid_axis
    rng = np.random.default_rng(res)
    ax = grid_axis(res)
    n, P = 3, 96
    pts = rng.uniform(-1.0, 1.0, size=(n, P, 3)).astype(np.float32)
    pts[0, :8] = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)     # the cube's corners
    pts[0, 8:16] = ax[rng.integers(0, res, size=(8, 3))]                                                       # exactly on nodes
    pts[1, :8, 0] = ((ax[:-1].astype(np.float64) + ax[1:].astype(np.float64)) / 2).astype(np.float32)[rng.integers(0, res - 1, size=8)]
    pts[1, 8:12] = np.float32(1.0005) * np.sign(pts[1, 8:12])                                                  # a hair outside the cube
    pts[2, :] = pts[2, 0]                                                                                      # one cell, P times
    points, per_cloud = m.occupancy_counts(pts, res)
    want_points, want_cloud = brute_force_counts(pts, res)
    assert points.sum() == n * P and np.array_equal(points, want_points) and np.array_equal(per_cloud, want_cloud)
    assert points.max() >= P and per_cloud.max() <= n


# ---- 7. argument errors -----------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(m):
    from brepgen_amd import _lib
    lib = _lib.load()
    a = torch.rand(2, 5, 3, device="cuda")
    out = torch.full((2, 2), -7.0, device="cuda")
    axis = torch.from_numpy(m.grid_axis(28)).cuda()
    counts = torch.zeros(2, 64 ** 3, dtype=torch.int32, device="cuda")
    s = _lib.stream()
    bad_cd = [(None, 2, 5, a.data_ptr(), 2, 5, out.data_ptr()), (a.data_ptr(), 2, 5, None, 2, 5, out.data_ptr()),
              (a.data_ptr(), 2, 5, a.data_ptr(), 2, 5, None), (a.data_ptr(), 2, 0, a.data_ptr(), 2, 5, out.data_ptr()),
              (a.data_ptr(), 2, 5, a.data_ptr(), 2, 0, out.data_ptr()), (a.data_ptr(), 0, 5, a.data_ptr(), 2, 5, out.data_ptr())]
    for args in bad_cd:
        assert lib.bg_chamfer_pairwise(*args, s) < 0 and lib.bg_last_error(), args
    c0, c1 = counts[0].data_ptr(), counts[1].data_ptr()
    bad_oc = [(None, 2, 5, axis.data_ptr(), 28, c0, c1), (a.data_ptr(), 2, 5, None, 28, c0, c1), (a.data_ptr(), 2, 5, axis.data_ptr(), 28, None, c1),
              (a.data_ptr(), 2, 5, axis.data_ptr(), 28, c0, None), (a.data_ptr(), 2, 0, axis.data_ptr(), 28, c0, c1),
              (a.data_ptr(), 2, 5, axis.data_ptr(), 65, c0, c1), (a.data_ptr(), 2, 5, axis.data_ptr(), 0, c0, c1)]
    for args in bad_oc:
        assert lib.bg_occupancy_counts(*args, s) < 0 and lib.bg_last_error(), args
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and int(counts.abs().sum()) == 0
    with pytest.raises(ValueError):
        m.occupancy_counts(a, 65)
    with pytest.raises(ValueError):
        m.pairwise_chamfer(a[0], a)
    with pytest.raises(ValueError):
        m.jsd_between_point_cloud_sets(a, a, in_unit_sphere=True)
