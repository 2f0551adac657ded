"""-m gpu: surface sampling on the device (csrc/mesh_sample.hip through brepgen_amd/sample_points.py).

The yardstick is the numpy restatement below: fp64 areas and np.cumsum, fp32 placement op for op.  No tolerance on the points: for the
face the kernel chose, `points` must equal the restatement bitwise.

FACE AGREEMENT RULE.  The kernel's running sum and np.cumsum associate differently, so face k is accepted iff

    cdf64[k - 1] - tol  <=  x  <  cdf64[k] + tol        tol = T * 2^-52 * area,   x = u0 * area[m] (the kernel's own area, in fp64)

which bounds the reordering error of T fp64 additions on either side; area[m] is checked against cdf64[-1] to the same tol.  A chosen face
must have positive area, always.  The number of picks that differ from np.searchsorted's answer is printed before anything is asserted
(expected: 0 for these inputs)."""
import os

import numpy as np
import pytest
import torch

from test_sample_points_cpu import CUBE_POINTS, CUBE_SEED, drawn_uniforms, write_ascii_stl, write_binary_stl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 300


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from brepgen_amd import sample_points
    return sample_points


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

def restate(tri, u):
    """tri [T, 3, 3] fp32, u [P, 3] fp64 -> areas, cdf (np.cumsum), area and the face of every point, all in fp64."""
    t = tri.astype(np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    areas = 0.5 * np.sqrt((n * n).sum(1))
    cdf = np.cumsum(areas)
    area = cdf[-1]
    face = np.searchsorted(cdf, u[:, 0] * area, side="right")
    face = np.where(face >= len(tri), np.searchsorted(cdf, area, side="left"), face)      # rounding left none: the last that raised the sum
    return {"areas": areas, "cdf": cdf, "area": area, "face": face}


def place(tri, face, u):
    """fp32, op for op: two subtractions, two products, (a + first) + second; trimesh's reflection before."""
    r1, r2 = u[:, 1].astype(np.float32), u[:, 2].astype(np.float32)
    flip = (r1 + r2) > np.float32(1.0)
    r1, r2 = np.where(flip, np.float32(1.0) - r1, r1)[:, None], np.where(flip, np.float32(1.0) - r2, r2)[:, None]
    a = tri[face, 0]
    e1, e2 = tri[face, 1] - a, tri[face, 2] - a
    out = (a + r1 * e1) + r2 * e2
    assert out.dtype == np.float32
    return out


def check_mesh(tri, u, points, face, area, label):
    """The agreement rule on one mesh; returns the number of picks that differ from np.searchsorted."""
    ref = restate(tri, u)
    T = len(tri)
    tol = T * 2.0 ** -52 * ref["area"]
    differ = int((face != ref["face"]).sum())
    print(f"{label}: T={T} area={area!r} |area - cumsum|={abs(area - ref['area']):.3e} tol={tol:.3e} picks differing from searchsorted={differ}")
    assert abs(area - ref["area"]) <= tol
    assert face.min() >= 0 and face.max() < T
    assert np.all(ref["areas"][face] > 0), "a zero-area triangle was picked"
    x = u[:, 0] * area
    below = np.where(face > 0, ref["cdf"][np.maximum(face - 1, 0)], 0.0)
    assert np.all(below - tol <= x) and np.all(x < ref["cdf"][face] + tol)
    assert points.dtype == np.float32 and points.tobytes() == place(tri, face, u).tobytes()
    return differ


def random_mesh(T, seed):
    return np.random.default_rng(seed).normal(size=(T, 3, 3)).astype(np.float32)


def uniforms(n, seed):
    return np.random.default_rng(seed).random((n, 3))


def run(sp, meshes, u, **kw):
    points, face, area = sp.sample_meshes(meshes, u.shape[1], uniforms=u, **kw)
    assert points.is_cuda and points.dtype == torch.float32 and face.dtype == torch.int32 and area.dtype == torch.float64
    return points.cpu().numpy(), face.cpu().numpy(), area.cpu().numpy()


# ---- supplied uniforms ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 2047, 2048, 2049, 6144, 6145, 40000])
def test_single_mesh_against_the_restatement(sp, T):
    """The scan's edges: one thread's eight entries (<= 8), a partial / full / just-started chunk of 256 x 8 (2047, 2048, 2049), the last
    table that stays in LDS and the first that goes through the workspace (6144, 6145), and 40 000 -- above anything LDS could hold."""
    tri, u = random_mesh(T, 100 + T), uniforms(P, 7 * T)[None]
    points, face, area = run(sp, [tri], u)
    assert check_mesh(tri, u[0], points[0], face[0], area[0], f"T={T}") == 0


def test_batch_of_mixed_sizes_in_one_call(sp):
    sizes = [1, 257, 3, 40000, 64]
    meshes = [random_mesh(T, 900 + i) for i, T in enumerate(sizes)]
    u = uniforms(len(sizes) * P, 3).reshape(len(sizes), P, 3)
    points, face, area = run(sp, meshes, u)
    assert sum(check_mesh(meshes[i], u[i], points[i], face[i], area[i], f"batch[{i}]") for i in range(len(sizes))) == 0
    # torch tensors on the device are taken as they are
    again = sp.sample_meshes([torch.from_numpy(t).cuda() for t in meshes], P, uniforms=torch.from_numpy(u))
    assert torch.equal(again[0].cpu(), torch.from_numpy(points)) and torch.equal(again[1].cpu(), torch.from_numpy(face))


def test_areas_over_twelve_orders_of_magnitude(sp):
    T = 600
    tri = random_mesh(T, 41)
    scale = (10.0 ** (-6.0 * np.random.default_rng(42).random(T))).astype(np.float32)          # edge 1 .. 1e-6: area 1 .. 1e-12
    tri = (tri[:, :1] + (tri - tri[:, :1]) * scale[:, None, None]).astype(np.float32)
    tri[::7, 1] = tri[::7, 0]                                                                   # and exact zeros among them
    ref = restate(tri, uniforms(1, 0))
    positive = ref["areas"][ref["areas"] > 0]
    assert positive.max() / positive.min() > 1e12 and (ref["areas"] == 0).sum() >= T // 7
    # half of the picks aimed INTO the tiny triangles: u0 just inside their own slice of the running sum
    u = uniforms(P, 43)[None]
    tiny = np.argsort(ref["areas"] + (ref["areas"] == 0) * 1e9)[:P // 2]
    u[0, :P // 2, 0] = (ref["cdf"][tiny] - 0.5 * ref["areas"][tiny]) / ref["area"]
    points, face, area = run(sp, [tri], u)
    check_mesh(tri, u[0], points[0], face[0], area[0], "twelve orders")
    # (a slice of 1e-12 of the sum is a few ulps of the running sum wide, the smallest ones less than one: not every aimed pick can hit)
    print(f"aimed picks that hit their tiny triangle: {int((face[0, :P // 2] == tiny).sum())} of {P // 2}")


@pytest.mark.parametrize("T", [40, 5000, 9000])
def test_zero_area_triangles_are_never_picked(sp, T):
    """Zero-area triangles at the front, in the middle and at the end (LDS table, several chunks, workspace table); u0 on the very values
    of the running sum next to them, and just below 1."""
    tri = random_mesh(T, 60 + T)
    zero = np.zeros(T, bool)
    zero[:3], zero[T // 2 - 2:T // 2 + 2], zero[-5:] = True, True, True
    zero[np.random.default_rng(T).random(T) < 0.2] = True
    tri[zero, 2] = tri[zero, 1]
    ref = restate(tri, uniforms(1, 0))
    assert np.array_equal(ref["areas"] == 0, zero)
    last_positive = int(np.nonzero(~zero)[0][-1])
    u = uniforms(P, 61)[None]
    edges = ref["cdf"][np.nonzero(zero)[0][:100]] / ref["area"]                  # boundaries that zero-area triangles sit on
    u[0, :len(edges), 0] = np.minimum(edges, 1.0 - 2.0 ** -53)
    near_one = 1.0 - 2.0 ** -53 * np.arange(1, 41)
    u[0, -40:, 0] = near_one
    points, face, area = run(sp, [tri], u)
    check_mesh(tri, u[0], points[0], face[0], area[0], f"zeros T={T}")
    assert np.all(face[0, -40:] == last_positive), face[0, -40:]


# ---- drawn uniforms, sharding ---------------------------------------------------------------------------------------------------------

def test_drawn_uniforms_equal_the_host_restatement(sp):
    meshes = [random_mesh(T, 70 + T) for T in (5, 300, 7000)]
    seed, draw, first = (0x1234 << 32) | 0x9ABCDEF0, 3, (1 << 32) + 5           # every key and counter word in use
    drawn = sp.sample_meshes(meshes, 1000, seed=seed, draw_id=draw, first_mesh=first)
    given = sp.sample_meshes(meshes, 1000, uniforms=drawn_uniforms(3, 1000, seed, draw, first))
    assert torch.equal(drawn[1], given[1]) and drawn[0].cpu().numpy().tobytes() == given[0].cpu().numpy().tobytes()
    assert torch.equal(drawn[2], given[2])


def test_a_shard_reproduces_its_clouds_and_the_keys_matter(sp):
    A, B, C = random_mesh(30, 1), random_mesh(700, 2), random_mesh(6500, 3)
    whole = sp.sample_meshes([A, B, C], 500, seed=11, draw_id=1, first_mesh=0)
    shard = sp.sample_meshes([B], 500, seed=11, draw_id=1, first_mesh=1)
    assert torch.equal(whole[0][1], shard[0][0]) and torch.equal(whole[1][1], shard[1][0]) and torch.equal(whole[2][1], shard[2][0])
    for kw in (dict(seed=12, draw_id=1, first_mesh=1), dict(seed=11, draw_id=2, first_mesh=1), dict(seed=11, draw_id=1, first_mesh=2)):
        other = sp.sample_meshes([B], 500, **kw)
        assert not torch.equal(other[0], shard[0]) and not torch.equal(other[1], shard[1]), kw


# ---- the cube -------------------------------------------------------------------------------------------------------------------------

def cube():
    """12 triangles of the cube [-0.5, 0.5]^3, two per side."""
    tris = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for s in (-0.5, 0.5):
            corner = np.zeros((4, 3), np.float32)
            corner[:, axis] = s
            corner[:, u] = [-0.5, 0.5, 0.5, -0.5]
            corner[:, v] = [-0.5, -0.5, 0.5, 0.5]
            tris += [corner[[0, 1, 2]], corner[[0, 2, 3]]]
    return np.stack(tris).astype(np.float32)


def check_cube(points):
    """Every point on a side, inside it; -> (chi-square of the six side counts against P / 6, the counts)."""
    assert np.all(np.abs(points) <= 0.5)
    on_side = np.abs(points) == 0.5
    assert np.all(on_side.any(1))
    side = 2 * on_side.argmax(1) + (points[np.arange(len(points)), on_side.argmax(1)] > 0)
    counts = np.bincount(side, minlength=6)
    expect = len(points) / 6.0
    return float(((counts - expect) ** 2 / expect).sum()), counts


def test_cube_points_lie_on_the_sides_evenly(sp):
    tri = cube()
    faces = np.arange(36).reshape(12, 3)
    points, face = sp.sample_surface(tri.reshape(36, 3), faces, CUBE_POINTS, seed=CUBE_SEED)
    assert points.shape == (CUBE_POINTS, 3) and face.shape == (CUBE_POINTS,) and face.dtype == torch.int64
    chi2, counts = check_cube(points.cpu().numpy())
    print("cube side counts", counts.tolist(), "chi-square", chi2)
    assert chi2 < 20.5                                     # 0.1 % point of chi-square with 5 degrees of freedom
    assert np.array_equal(np.bincount(face.cpu().numpy() // 2, minlength=6), counts)
    u = drawn_uniforms(1, CUBE_POINTS, CUBE_SEED)[0]
    assert points.cpu().numpy().tobytes() == place(tri, restate(tri, u)["face"], u).tobytes()      # the very sequence the CPU test judged


# ---- degenerate meshes ------------------------------------------------------------------------------------------------------------------

def test_degenerate_meshes_inside_a_batch(sp):
    A, C = random_mesh(100, 5), random_mesh(6200, 6)
    flat = random_mesh(9, 7)
    flat[:, 1], flat[:, 2] = flat[:, 0], flat[:, 0]                               # area exactly 0
    empty = np.zeros((0, 3, 3), np.float32)
    nan = random_mesh(300, 8)
    nan[17, 1, 2] = np.nan
    inf = random_mesh(12, 9)
    inf[3, 0, 0] = np.inf
    batch = [A, flat, empty, C, nan, inf]
    points, face, area = sp._launch(batch, 200, 4, 0, 0, None)
    points, face, area = points.cpu().numpy(), face.cpu().numpy(), area.cpu().numpy()
    for i in (1, 2, 4, 5):
        assert np.all(face[i] == -1) and np.all(np.isnan(points[i])), i
    assert area[1] == 0.0 and area[2] == 0.0 and np.isnan(area[4]) and not np.isfinite(area[5])
    for i, mesh in ((0, A), (3, C)):                                              # the neighbours: as if sampled alone
        alone = sp.sample_meshes([mesh], 200, seed=4, first_mesh=i)
        assert np.array_equal(alone[1][0].cpu().numpy(), face[i]) and alone[0][0].cpu().numpy().tobytes() == points[i].tobytes()
        assert np.all(np.isfinite(points[i]))
    with pytest.raises(ValueError, match="mesh 1 "):
        sp.sample_meshes(batch, 200, seed=4)
    with pytest.raises(ValueError, match="mesh 0 "):
        sp.sample_meshes([empty], 200)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------

def test_command_line_writes_the_clouds_of_sample_meshes(sp, tmp_path):
    from brepgen_amd import metrics
    src, dst = tmp_path / "stl", tmp_path / "ply"
    (src / "sub").mkdir(parents=True)
    meshes = {"b_mesh.stl": random_mesh(20, 1), os.path.join("sub", "a_mesh.stl"): random_mesh(300, 2), "c_mesh.stl": cube()}
    write_binary_stl(src / "b_mesh.stl", meshes["b_mesh.stl"])
    write_ascii_stl(src / "sub" / "a_mesh.stl", meshes[os.path.join("sub", "a_mesh.stl")])
    write_binary_stl(src / "c_mesh.stl", meshes["c_mesh.stl"])
    (src / "notes.txt").write_text("not a mesh")
    written = sp.main(["--in_dir", str(src), "--out_dir", str(dst), "--n_points", "500", "--seed", "9", "--batch", "2"])
    assert len(written) == 3
    assert sorted(os.listdir(dst)) == ["a_mesh.ply", "b_mesh.ply", "c_mesh.ply"]
    order = sp.find_stl(str(src))                                                 # sorted paths: b_mesh, c_mesh, sub/a_mesh
    assert [os.path.relpath(p, src) for p in order] == ["b_mesh.stl", "c_mesh.stl", os.path.join("sub", "a_mesh.stl")]
    want = sp.sample_meshes([sp.read_stl(p) for p in order], 500, seed=9)[0].cpu().numpy()
    for cloud, path in zip(want, order):
        got = metrics.read_ply(str(dst / (os.path.splitext(os.path.basename(path))[0] + ".ply")))
        assert got.dtype == np.float32 and got.tobytes() == cloud.tobytes(), path
