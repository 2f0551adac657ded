"""Surface sampling of the reference's ``sample_points.py`` (step 1 of ``eval.sh``: every generated ``.stl`` -> a 2000-point ``.ply``) on the
MI355X.

    sample_surface / sample_meshes      -> bg_mesh_sample  (csrc/mesh_sample.hip; the reference calls ``trimesh.sample.sample_surface`` in one
                                           CPU process per core): area-weighted triangle pick in fp64, trimesh's reflected barycentric
                                           placement in fp32, all meshes of a batch in one launch
    read_stl, write_ply, main           host glue (``python -m brepgen_amd.sample_points --in_dir D --out_dir O``)

Seed semantics are the project's, not numpy's global generator: a cloud depends only on (seed, draw_id, GLOBAL mesh index, the mesh) --
not on the batch or the rank it was sampled in -- like the ancestral noise of ``sampling.device_randn``.  Meshes are taken as triangle
soups ``[T, 3, 3]``; vertex merging and repair (``trimesh.load``) do not change a surface sample and are not done.  There is no CPU
path: without a GPU or the library every sampling entry raises ``BrepgenHipError``.
"""
import argparse
import os
import struct

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

N_POINTS = 2000                 # sample_points.py:65


def _device():
    _lib.load()
    if not torch.cuda.is_available():
        raise _lib.BrepgenHipError("brepgen_amd runs on the MI355X only (no GPU visible); no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _soup(mesh, index, device):
    t = torch.as_tensor(np.asarray(mesh) if not torch.is_tensor(mesh) else mesh)
    if t.dim() != 3 or tuple(t.shape[1:]) != (3, 3):
        raise ValueError(f"mesh {index}: expected triangles [T, 3, 3], got {tuple(t.shape)}")
    return t.detach().to(device=device, dtype=torch.float32)


@torch.no_grad()
def _launch(triangles, count, seed, draw_id, first_mesh, uniforms):
    """One bg_mesh_sample call, results as the kernel left them (a degenerate mesh: face -1, NaN points):
    (points [M, count, 3] fp32, face [M, count] int32, area [M] fp64)."""
    device = _device()
    count, M = int(count), len(triangles)
    if count < 1:
        raise ValueError(f"count must be >= 1, got {count}")
    soups = [_soup(mesh, i, device) for i, mesh in enumerate(triangles)]
    sizes = [int(s.shape[0]) for s in soups]
    if sum(sizes) >= 2 ** 31:
        raise ValueError(f"{sum(sizes)} triangles in one call exceed the int32 offsets; sample in smaller batches")
    tri = torch.cat(soups + [torch.zeros(1, 3, 3, device=device)]).contiguous()      # one pad triangle: never an empty allocation
    tri_off = torch.tensor(np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]), dtype=torch.int32).to(device)
    uni = None
    if uniforms is not None:
        uni = torch.as_tensor(np.asarray(uniforms) if not torch.is_tensor(uniforms) else uniforms)
        if tuple(uni.shape) != (M, count, 3):
            raise ValueError(f"uniforms: expected [{M}, {count}, 3], got {tuple(uni.shape)}")
        uni = uni.detach().to(device=device, dtype=torch.float64).contiguous()
    cdf_ws = torch.empty(tri.shape[0], device=device, dtype=torch.float64)
    points = torch.empty(M, count, 3, device=device, dtype=torch.float32)
    face = torch.empty(M, count, device=device, dtype=torch.int32)
    area = torch.empty(M, device=device, dtype=torch.float64)
    check(_lib.load().bg_mesh_sample(ptr(tri), ptr(tri_off), M, count, int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw_id) & 0xFFFFFFFF,
                                     int(first_mesh), ptr(uni), ptr(cdf_ws), ptr(points), ptr(face), ptr(area), stream()),
          "bg_mesh_sample")
    return points, face, area


def sample_meshes(triangles, count=N_POINTS, seed=0, draw_id=0, first_mesh=0, uniforms=None):
    """`count` area-weighted surface points on each mesh of `triangles` (a list of [T_i, 3, 3] arrays or tensors), one C call.

    -> (points [M, count, 3] fp32, face_index [M, count] int32 -- the triangle within its mesh --, area [M] fp64), device tensors.
    Mesh i is sampled as GLOBAL mesh `first_mesh + i`: a shard of a larger list reproduces its clouds of the whole call bit for bit.
    `uniforms` ([M, count, 3] float64 in [0, 1): triangle pick, two barycentric draws) replaces the device's Philox draw.
    Raises ValueError naming the mesh whose area is not finite and positive (no triangles, collapsed, NaN / Inf vertices)."""
    points, face, area = _launch(triangles, count, seed, draw_id, first_mesh, uniforms)
    bad = torch.nonzero(~(torch.isfinite(area) & (area > 0))).flatten().tolist()
    if bad:
        raise ValueError(f"mesh {bad[0]} has no finite positive surface area (area = {float(area[bad[0]])}); "
                         f"{len(bad)} such mesh(es) in the batch: {bad[:8]}")
    return points, face, area


def sample_surface(vertices, faces, count, seed=0, draw_id=0, mesh_index=0, uniforms=None):
    """trimesh.sample.sample_surface's pair for one indexed mesh: (points [count, 3] fp32, face_index [count] int64), device tensors.
    vertices [V, 3], faces [F, 3] (integer); `uniforms` [count, 3] as in `sample_meshes`."""
    device = _device()
    v = torch.as_tensor(np.asarray(vertices) if not torch.is_tensor(vertices) else vertices).to(device=device, dtype=torch.float32)
    f = torch.as_tensor(np.asarray(faces) if not torch.is_tensor(faces) else faces).to(device=device, dtype=torch.int64)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"expected vertices [V, 3] and faces [F, 3], got {tuple(v.shape)} and {tuple(f.shape)}")
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise ValueError(f"faces index vertices outside 0 .. {v.shape[0] - 1}")
    if uniforms is not None:
        uniforms = torch.as_tensor(np.asarray(uniforms) if not torch.is_tensor(uniforms) else uniforms)[None]
    points, face, _ = sample_meshes([v[f]], count, seed, draw_id, mesh_index, uniforms)
    return points[0], face[0].to(torch.int64)


# ---- host glue: STL in, PLY out, the folder walk of sample_points.py ---------------------------------------------------------------

def read_stl(path):
    """[T, 3, 3] float32 triangle soup of a binary STL (80-byte header, little-endian count, 50-byte records; recognised by
    size == 84 + 50 n) or an ASCII one (`vertex x y z` lines, three per facet).  Normals are ignored."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) >= 84:
        n = struct.unpack_from("<I", data, 80)[0]
        if len(data) == 84 + 50 * n:
            rec = np.frombuffer(data, dtype=np.dtype([("normal", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]), count=n, offset=84)
            return np.ascontiguousarray(rec["v"], dtype=np.float32)
    if not data.lstrip().startswith(b"solid"):
        raise ValueError(f"{path}: neither a binary STL (size 84 + 50 n) nor an ASCII one: truncated or not an STL file")
    tris, facet, closed = [], None, False
    for raw in data.decode("ascii", errors="replace").splitlines():
        tok = raw.split()
        if not tok:
            continue
        if tok[0] == "facet":
            if facet is not None:
                raise ValueError(f"{path}: facet {len(tris)} is not closed")
            facet = []
        elif tok[0] == "vertex":
            if facet is None or len(tok) != 4:
                raise ValueError(f"{path}: malformed vertex line {raw.strip()!r}")
            try:
                facet.append([float(v) for v in tok[1:]])
            except ValueError:
                raise ValueError(f"{path}: malformed vertex line {raw.strip()!r}") from None
        elif tok[0] == "endfacet":
            if facet is None or len(facet) != 3:
                raise ValueError(f"{path}: facet {len(tris)} has {0 if facet is None else len(facet)} vertices, not 3")
            tris.append(facet)
            facet = None
        elif tok[0] == "endsolid":
            closed = True
    if facet is not None or not closed:
        raise ValueError(f"{path}: truncated after {len(tris)} facets (no endsolid)")
    return np.asarray(tris, dtype=np.float32).reshape(-1, 3, 3)


def write_ply(points, path):
    """Binary little-endian PLY 1.0 with one `vertex` element of float x, y, z (what `metrics.read_ply` reads back bit for bit)."""
    pts = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"expected points [n, 3], got {pts.shape}")
    header = ["ply", "format binary_little_endian 1.0", "comment vertices", f"element vertex {len(pts)}",
              "property float x", "property float y", "property float z", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(np.ascontiguousarray(pts, dtype="<f4").tobytes())


def find_stl(folder):
    """Every name ending in `.stl` below `folder`, sorted: the position in this list is the GLOBAL mesh index, so `--seed` fixes the run."""
    return sorted(os.path.join(d, name) for d, _, names in os.walk(folder) for name in names if name.endswith(".stl"))


# command line of the reference's script: (flag, type, default, help)
_CLI = (("--in_dir", str, None, "folder walked for .stl files"),
        ("--out_dir", str, None, "folder for <name>.ply; files within are overwritten"),
        ("--n_points", int, N_POINTS, "points per mesh"),
        ("--seed", int, 0, "Philox key of the run"),
        ("--batch", int, 256, "meshes per launch (the result does not depend on it)"))


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m brepgen_amd.sample_points",
                                     description="sample_points.py on the MI355X: a point cloud (.ply) for every .stl")
    for flag, kind, default, text in _CLI:
        parser.add_argument(flag, type=kind, default=default, help=text)
    return parser


def main(argv=None):
    opt = build_parser().parse_args(argv)
    if not opt.in_dir or not opt.out_dir:
        raise SystemExit("--in_dir and --out_dir are required")
    if opt.batch < 1:
        raise SystemExit("--batch must be >= 1")
    paths = find_stl(opt.in_dir)
    os.makedirs(opt.out_dir, exist_ok=True)
    written = []
    for lo in range(0, len(paths), opt.batch):
        chunk = paths[lo:lo + opt.batch]
        try:
            points, _, _ = sample_meshes([read_stl(p) for p in chunk], opt.n_points, seed=opt.seed, first_mesh=lo)
        except ValueError as err:
            raise SystemExit(f"meshes {lo} .. {lo + len(chunk) - 1} ({chunk[0]} ...): {err}") from None
        points = points.cpu().numpy()
        for path, cloud in zip(chunk, points):
            out = os.path.join(opt.out_dir, os.path.splitext(os.path.basename(path))[0] + ".ply")
            write_ply(cloud, out)
            written.append(out)
    print(f"{len(written)} point clouds of {opt.n_points} points written to {opt.out_dir}")
    return written


if __name__ == "__main__":
    main()
