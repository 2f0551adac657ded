"""CPU-side checks of the surface sampler (brepgen_amd/sample_points.py, csrc/mesh_sample.hip): the STL reader and the PLY writer, the ABI
boundary of bg_mesh_sample, and the host restatement of the device's uniform draw (`drawn_uniforms`, which tests/test_gpu_mesh_sample.py
compares the kernel against bit for bit) -- run here through the numpy restatement of the whole sampler on the cube.  No kernel is launched."""
import struct

import numpy as np
import pytest
import torch

import brepgen_amd as bga
from brepgen_amd import _lib, metrics, sample_points
from oracle.philox import philox4x32_10

TAG = 0x5A3D                    # csrc/mesh_sample.hip: MS_TAG >> 16
CUBE_SEED, CUBE_POINTS = 2024, 2000


def drawn_uniforms(M, P, seed, draw_id=0, first_mesh=0):
    """[M, P, 3] float64: what bg_mesh_sample draws when `uniforms` is NULL.  One Philox4x32-10 block per point, key = seed, counter =
    (p, low 32 bits of g, draw_id, TAG << 16 | bits 32..47 of g) with g = first_mesh + m;  u0 = (top 52 bits of word0:word1 + 0.5) * 2^-52
    in fp64, u1 / u2 = ((word >> 9) + 0.5) * 2^-23 in fp32 of words 2 / 3."""
    g = np.uint64(first_mesh) + np.arange(M, dtype=np.uint64)
    c = np.zeros((M, P, 4), dtype=np.uint32)
    c[..., 0] = np.arange(P, dtype=np.uint32)[None, :]
    c[..., 1] = (g & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    c[..., 2] = np.uint32(draw_id)
    c[..., 3] = (np.uint64(TAG << 16) | ((g >> np.uint64(32)) & np.uint64(0xFFFF))).astype(np.uint32)[:, None]
    w = philox4x32_10(c, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    top52 = ((w[..., 0].astype(np.uint64) << np.uint64(32)) | w[..., 1].astype(np.uint64)) >> np.uint64(12)
    u = np.empty((M, P, 3), dtype=np.float64)
    u[..., 0] = (top52.astype(np.float64) + 0.5) * 2.0 ** -52
    for j in (1, 2):
        u[..., j] = ((w[..., 1 + j] >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 8388608.0)
    return u


def test_drawn_uniforms_are_exact_and_open():
    u = drawn_uniforms(3, 4000, seed=(7 << 32) | 5, draw_id=2, first_mesh=(1 << 33) + 1)
    assert u.min() > 0.0 and u.max() < 1.0
    k = u[..., 0] * 2.0 ** 52 - 0.5                         # the 52-bit grid, exactly
    assert np.array_equal(k, np.floor(k)) and k.max() > 2.0 ** 51
    assert np.array_equal(u[..., 1:], u[..., 1:].astype(np.float32).astype(np.float64))
    assert abs(u.mean() - 0.5) < 0.01
    # the counter carries every index: another mesh, draw or seed is another stream, and a shard is a slice
    assert np.array_equal(drawn_uniforms(3, 50, 9, 1, 4)[1:], drawn_uniforms(2, 50, 9, 1, 5))
    base = drawn_uniforms(1, 50, 9, 1, 4)
    for other in (drawn_uniforms(1, 50, 10, 1, 4), drawn_uniforms(1, 50, 9, 2, 4), drawn_uniforms(1, 50, 9, 1, 4 + (1 << 32))):
        assert not np.array_equal(base, other)


def test_cube_statistics_of_the_committed_seed():
    """The cube case of tests/test_gpu_mesh_sample.py on the host: numpy restatement of the sampler + the restated draw.  The sequence is a
    fixed fact of the seed, so the chi-square condition of the GPU test is settled here."""
    import test_gpu_mesh_sample as g
    tri = g.cube()
    u = drawn_uniforms(1, CUBE_POINTS, CUBE_SEED)[0]
    ref = g.restate(tri, u)
    assert ref["area"] == 6.0 and np.array_equal(ref["face"], np.searchsorted(ref["cdf"], u[:, 0] * 6.0, side="right"))
    chi2, counts = g.check_cube(g.place(tri, ref["face"], u))
    print("cube side counts", counts.tolist(), "chi-square", chi2)
    assert chi2 < 20.5


# ---- STL / PLY --------------------------------------------------------------------------------------------------------------------

def write_binary_stl(path, tri):
    with open(path, "wb") as f:
        f.write(b"binary stl written by the test".ljust(80, b" ") + struct.pack("<I", len(tri)))
        for t in np.asarray(tri, dtype="<f4"):
            f.write(struct.pack("<3f", 0.0, 0.0, 0.0) + t.tobytes() + struct.pack("<H", 0))


def write_ascii_stl(path, tri, vertices_per_facet=3):
    lines = ["solid test"]
    for t in np.asarray(tri, dtype=np.float32):
        lines += [" facet normal 0 0 0", "  outer loop"]
        lines += [f"   vertex {float(v[0])!r} {float(v[1])!r} {float(v[2])!r}" for v in t[:vertices_per_facet]]
        lines += ["  endloop", " endfacet"]
    lines.append("endsolid test")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def small_mesh(n=7, seed=11):
    return np.random.default_rng(seed).normal(size=(n, 3, 3)).astype(np.float32)


def test_read_stl_binary_and_ascii_agree(tmp_path):
    tri = small_mesh()
    write_binary_stl(tmp_path / "b.stl", tri)
    write_ascii_stl(tmp_path / "a.stl", tri)
    b, a = sample_points.read_stl(str(tmp_path / "b.stl")), sample_points.read_stl(str(tmp_path / "a.stl"))
    assert b.dtype == a.dtype == np.float32 and b.shape == a.shape == (7, 3, 3)
    assert np.array_equal(b, tri) and np.array_equal(a, tri)


def test_read_stl_rejects_truncated_and_malformed_files(tmp_path):
    tri = small_mesh()
    write_binary_stl(tmp_path / "b.stl", tri)
    whole = (tmp_path / "b.stl").read_bytes()
    (tmp_path / "cut.stl").write_bytes(whole[:-13])
    with pytest.raises(ValueError, match="cut.stl"):
        sample_points.read_stl(str(tmp_path / "cut.stl"))
    write_ascii_stl(tmp_path / "two.stl", tri, vertices_per_facet=2)
    with pytest.raises(ValueError, match="two.stl"):
        sample_points.read_stl(str(tmp_path / "two.stl"))
    write_ascii_stl(tmp_path / "a.stl", tri)
    text = (tmp_path / "a.stl").read_text()
    (tmp_path / "half.stl").write_text(text[:len(text) // 2])
    with pytest.raises(ValueError, match="half.stl"):
        sample_points.read_stl(str(tmp_path / "half.stl"))


def test_write_ply_round_trips_through_the_metrics_reader(tmp_path):
    pts = np.random.default_rng(5).normal(size=(123, 3)).astype(np.float32)
    pts[0, 0], pts[1, 1] = np.float32(1e-42), np.float32(-0.0)             # a subnormal and a signed zero travel too
    for name, value in (("n.ply", pts), ("t.ply", torch.from_numpy(pts))):
        sample_points.write_ply(value, str(tmp_path / name))
        got = metrics.read_ply(str(tmp_path / name))
        assert got.dtype == np.float32 and got.tobytes() == pts.tobytes()
    with pytest.raises(ValueError):
        sample_points.write_ply(np.zeros((4, 2), np.float32), str(tmp_path / "bad.ply"))


# ---- the ABI boundary -------------------------------------------------------------------------------------------------------------

def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # also where the suite runs next to a GPU
    tri = torch.from_numpy(small_mesh())
    with pytest.raises(_lib.BrepgenHipError):
        sample_points.sample_meshes([tri], 10)
    with pytest.raises(_lib.BrepgenHipError):
        bga.sample_surface(tri.reshape(-1, 3), torch.arange(21).reshape(7, 3), 10)


def test_argument_errors_need_no_device():
    lib = _lib.load()
    assert "bg_mesh_sample" in _lib.EXPORTS and lib.bg_mesh_sample.argtypes == _lib._SIGNATURES["bg_mesh_sample"][1]
    fake = 0x10000                                    # never dereferenced: validation fails first
    ok = dict(tri=fake, off=fake, M=2, P=5, seed=1, draw=0, first=0, uni=None, ws=fake, pts=fake, face=fake, area=fake)

    def call(**kw):
        a = {**ok, **kw}
        return lib.bg_mesh_sample(a["tri"], a["off"], a["M"], a["P"], a["seed"], a["draw"], a["first"], a["uni"], a["ws"], a["pts"],
                                  a["face"], a["area"], None)

    assert call(tri=None) == _lib.BG_E_ARG and b"null" in lib.bg_last_error()
    for name in ("off", "ws", "pts", "face", "area"):
        assert call(**{name: None}) == _lib.BG_E_ARG and b"null" in lib.bg_last_error(), name
    for kw in (dict(P=0), dict(P=-4), dict(M=-1), dict(first=-1), dict(P=0x7fffffff)):
        assert call(**kw) == _lib.BG_E_SHAPE and lib.bg_last_error(), kw
    assert call(M=0, tri=None, pts=None) == 0          # nothing to do


def test_package_exports_the_sampler():
    for name in ("sample_surface", "sample_meshes", "read_stl", "write_ply"):
        assert getattr(bga, name) is getattr(sample_points, name) and name in bga.__all__
    a = sample_points.build_parser().parse_args(["--in_dir", "samples", "--out_dir", "pcd"])
    assert (a.in_dir, a.out_dir, a.n_points, a.seed) == ("samples", "pcd", 2000, 0)
