"""CPU-side checks of the evaluation metrics (brepgen_amd/metrics.py, csrc/metrics.hip): the ABI boundary, the host halves
(PLY reader, normalisation, counts -> entropy / JSD) against the reference's stored results (tests/golden/metrics_*.npz,
written by tests/golden/gen_metrics_golden.py from the reference's own pc_metric.py), and the command line.  No kernel is launched."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import brepgen_amd as bga
from brepgen_amd import _lib, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ["metrics_p2000", "metrics_p256", "metrics_mixed"]


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def test_library_exports_both_symbols_and_the_signatures_load():
    lib = _lib.load()
    for name in ("bg_chamfer_pairwise", "bg_occupancy_counts"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name][1]
    assert lib.bg_abi_version() == _lib.ABI_VERSION == 7
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        assert " T bg_chamfer_pairwise" in nm.stdout and " T bg_occupancy_counts" in nm.stdout


def test_argument_errors_need_no_device():
    lib = _lib.load()
    fake = 0x10000                                    # never dereferenced: validation fails first
    assert lib.bg_chamfer_pairwise(None, 1, 1, fake, 1, 1, fake, None) == _lib.BG_E_ARG and b"null" in lib.bg_last_error()
    assert lib.bg_chamfer_pairwise(fake, 1, 1, None, 1, 1, fake, None) == _lib.BG_E_ARG
    assert lib.bg_chamfer_pairwise(fake, 1, 1, fake, 1, 1, None, None) == _lib.BG_E_ARG
    for S, Pa, R, Pb in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-3, 1, 1, 1), (1 << 16, 1, 1 << 15, 1)):
        assert lib.bg_chamfer_pairwise(fake, S, Pa, fake, R, Pb, fake, None) == _lib.BG_E_SHAPE, (S, Pa, R, Pb)
        assert lib.bg_last_error()
    assert lib.bg_occupancy_counts(None, 1, 1, fake, 28, fake, fake, None) == _lib.BG_E_ARG and b"null" in lib.bg_last_error()
    assert lib.bg_occupancy_counts(fake, 1, 1, None, 28, fake, fake, None) == _lib.BG_E_ARG
    assert lib.bg_occupancy_counts(fake, 1, 1, fake, 28, None, fake, None) == _lib.BG_E_ARG
    assert lib.bg_occupancy_counts(fake, 1, 1, fake, 28, fake, None, None) == _lib.BG_E_ARG
    assert lib.bg_occupancy_counts(fake, 1, 0, fake, 28, fake, fake, None) == _lib.BG_E_SHAPE
    assert lib.bg_occupancy_counts(fake, 0, 5, fake, 28, fake, fake, None) == _lib.BG_E_SHAPE
    assert lib.bg_occupancy_counts(fake, 1, 5, fake, 65, fake, fake, None) == _lib.BG_E_SHAPE and b"res" in lib.bg_last_error()
    assert lib.bg_occupancy_counts(fake, 1, 5, fake, 0, fake, fake, None) == _lib.BG_E_SHAPE


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # also where the suite runs next to a GPU
    g = golden("metrics_p256")
    a, b = g["sample"][:2], g["ref"][:3]
    for call in (lambda: metrics.pairwise_chamfer(a, b), lambda: metrics.compute_cov_mmd(torch.from_numpy(a), torch.from_numpy(b), 64),
                 lambda: metrics.entropy_of_occupancy_grid(a, 28), lambda: metrics.jsd_between_point_cloud_sets(a, b),
                 lambda: bga.compute_cov_mmd(a, b)):
        with pytest.raises(_lib.BrepgenHipError):
            call()


def test_sphere_clipped_grid_is_refused():
    a = np.zeros((1, 4, 3), np.float32)
    with pytest.raises(ValueError):
        metrics.jsd_between_point_cloud_sets(a, a, in_unit_sphere=True)
    with pytest.raises(ValueError):
        metrics.entropy_of_occupancy_grid(a, 28, in_sphere=True)


def test_package_reexports_the_reference_names():
    for name in ("pairwise_chamfer", "compute_cov_mmd", "entropy_of_occupancy_grid", "jsd_between_point_cloud_sets", "normalize_pc",
                 "read_ply"):
        assert getattr(bga, name) is getattr(metrics, name) and name in bga.__all__


def _write_ply(path, pts, fmt, dtype):
    """sample_points.py:write_ply's layout: a vertex element with x, y, z."""
    ply_type = {"f4": "float", "f8": "double"}[dtype]
    header = ["ply", f"format {fmt} 1.0", "comment written by the test", f"element vertex {len(pts)}",
              f"property {ply_type} x", f"property {ply_type} y", f"property {ply_type} z", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode())
        if fmt == "ascii":
            for p in pts:
                f.write((" ".join(repr(float(v)) for v in p) + "\n").encode())
        else:
            f.write(np.asarray(pts, dtype="<" + dtype).tobytes())


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
@pytest.mark.parametrize("dtype", ["f4", "f8"])
def test_ply_reader_round_trip(tmp_path, fmt, dtype):
    pts = np.random.default_rng(3).normal(size=(37, 3)).astype(dtype)
    path = tmp_path / "cloud.ply"
    _write_ply(path, pts, fmt, dtype)
    got = metrics.read_ply(str(path))
    assert got.shape == (37, 3) and got.dtype == np.dtype(dtype) and np.array_equal(got, pts)


def test_ply_reader_skips_other_vertex_properties_and_later_elements(tmp_path):
    path = tmp_path / "mesh.ply"
    header = ["ply", "format binary_little_endian 1.0", "element vertex 2", "property float x", "property float y", "property float z",
              "property uchar red", "element face 1", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode())
        f.write(struct.pack("<fffB", 1.0, 2.0, 3.0, 7) + struct.pack("<fffB", 4.0, 5.0, 6.0, 8))
        f.write(struct.pack("<Biii", 3, 0, 1, 0))
    assert np.array_equal(metrics.read_ply(str(path)), np.array([[1, 2, 3], [4, 5, 6]], np.float32))
    bad = tmp_path / "bad.ply"
    bad.write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    with pytest.raises(ValueError):
        metrics.read_ply(str(bad))


@pytest.mark.parametrize("name", CASES)
def test_normalize_pc_matches_the_reference(name):
    g = golden(name)
    assert np.array_equal(metrics.normalize_pc(g["raw"]), g["raw_normalized"])
    s = g["sample"]
    assert np.abs(s).max() == 1.0                       # the fixture's clouds came through it: some coordinate sits exactly on a node


@pytest.mark.parametrize("name", CASES)
def test_host_half_of_jsd_and_entropy_match_the_reference(name):
    """counts -> value: with the reference's own counters as input the numpy float64 formulas give the reference's JSD and entropy
    (scipy sums in another order: 1e-12 relative)."""
    g = golden(name)
    jsd = metrics.jensen_shannon_divergence(g["point_counts_sample"].astype(np.float64), g["point_counts_ref"].astype(np.float64))
    assert abs(jsd - float(g["jsd"])) <= 1e-12 * float(g["jsd"])
    for which in ("sample", "ref"):
        ent = metrics.entropy_from_cloud_counts(g["cloud_counts_" + which], len(g[which]))
        assert abs(ent - float(g["entropy_" + which])) <= 1e-12 * float(g["entropy_" + which])
        assert g["point_counts_" + which].sum() == g[which].shape[0] * g[which].shape[1]


def test_grid_axis_is_the_reference_grid():
    """i * spacing - 1 in double, rounded to fp32 (pc_metric.py:152-170), and the separable nearest-node rule of the kernel -- restated
    here in numpy -- reproduces the reference's stored counters."""
    axis = metrics.grid_axis(28)
    assert axis.dtype == np.float32 and axis[0] == -1.0 and axis[-1] == 1.0 and np.all(np.diff(axis) > 0)
    spacing = 1.0 / 27.0 * 2
    assert all(axis[i] == np.float32(i * spacing - 1.0) for i in range(28))
    g = golden("metrics_p256")
    idx = np.abs(g["sample"].astype(np.float64)[..., None] - axis.astype(np.float64)).argmin(-1)      # argmin: the lower index on a tie
    cells = (idx[..., 0] * 28 + idx[..., 1]) * 28 + idx[..., 2]
    assert np.array_equal(np.bincount(cells.ravel(), minlength=28 ** 3), g["point_counts_sample"])


def test_cli_parser_accepts_the_evaluation_script_invocation():
    """eval.sh: python pc_metric.py --fake <dir> --real <dir>; plus pc_metric.py:287-295's options and --seed."""
    p = metrics.build_parser()
    a = p.parse_args(["--fake", "samples/deepcad", "--real", "data/test_pcd"])
    assert (a.fake, a.real, a.n_test, a.multi, a.times, a.batch_size, a.seed) == ("samples/deepcad", "data/test_pcd", 1000, 3, 10, 64, None)
    a = p.parse_args(["--fake", "f", "--real", "r", "--n_test", "10", "--multi", "2", "--times", "1", "--batch_size", "8", "--seed", "5"])
    assert (a.n_test, a.multi, a.times, a.batch_size, a.seed) == (10, 2, 1, 8, 5)


def test_chamfer_kernel_keeps_its_instruction_mix_and_does_not_spill():
    """tools/metrics_bench.py and DESIGN.md count 7 lane-ops per point pair: 3 sub + 1 mul + 2 fma + two halves of a v_min3_f32 (hipcc
    fuses the row-minimum and the column-partial chains of fminf pairwise).  Pin that in the ISA: per unrolled 8 x 4 block 16 + 16
    v_min3_f32 in the one-pass loop and 16 in each of the two rows-only loops, no two-operand float minimum, no scratch."""
    import re
    from tests.train_cpu import resource_usage
    _, scratch, spills, _, asm = resource_usage("metrics.hip", asm=True)
    body = re.search(r"^_ZN2bg23chamfer_pairwise_kernel\w*:.*?^\.Lfunc_end\d+:", asm, flags=re.S | re.M).group(0)
    assert len(re.findall(r"\bv_min3_f32\b", body)) == 64 and not re.findall(r"\bv_min_f32", body)
    assert len(re.findall(r"\bv_sub_f32", body)) == 3 * 96 and len(re.findall(r"\bds_min_u32\b", body)) == 1
    assert len(scratch) == 2 and not any(scratch) and not any(spills), (scratch, spills)
