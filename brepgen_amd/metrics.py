"""Evaluation metrics of the reference's ``pc_metric.py`` (COV / MMD / JSD over sets of point clouds) on the MI355X.

Same names, arguments and return shapes as the reference, so ``pc_metric.py``'s ``main`` can import them from here:

    pairwise_chamfer / compute_cov_mmd      -> bg_chamfer_pairwise  (csrc/metrics.hip; the reference calls the `chamfer_distance`
                                               CUDA extension once per sample cloud and batch of 64 reference clouds)
    entropy_of_occupancy_grid / jsd_between_point_cloud_sets
                                            -> bg_occupancy_counts  (the reference runs an sklearn KD-tree on the CPU); entropy and
                                               JSD follow from the counts in numpy float64 with the reference's formulas
    normalize_pc, read_ply, main            host glue (``python -m brepgen_amd.metrics --fake DIR --real DIR``)

Clouds are taken as fp32 ``[n, P, 3]`` arrays (numpy or tensors on any device) and moved to the current device.  There is no CPU
path: without a GPU or the library every entry raises ``BrepgenHipError``.
"""
import argparse
import os
import random
import warnings

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

N_POINTS = 2000                 # pc_metric.py:15
MAX_RESOLUTION = 64             # bg_occupancy_counts keeps one bit per cell of a cloud's grid in LDS


def _device_clouds(pcs, what):
    """[n, P, 3] fp32 contiguous on the current device (the reference's `.cuda()`); raises without a GPU or the library."""
    _lib.load()
    if not torch.cuda.is_available():
        raise _lib.BrepgenHipError("brepgen_amd runs on the MI355X only (no GPU visible); no CPU fallback")
    t = torch.as_tensor(np.asarray(pcs) if not torch.is_tensor(pcs) else pcs)
    if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: expected [n, P, 3] point clouds with n, P >= 1, got {tuple(t.shape)}")
    return t.detach().to(device=torch.device("cuda", torch.cuda.current_device()), dtype=torch.float32).contiguous()


@torch.no_grad()
def pairwise_chamfer(sample_pcs, ref_pcs):
    """[S, R] device tensor: out[i, j] = mean_p min_q |s_ip - r_jq|^2 + mean_q min_p |s_ip - r_jq|^2 (pc_metric.py:45-80)."""
    a, b = _device_clouds(sample_pcs, "sample_pcs"), _device_clouds(ref_pcs, "ref_pcs")
    out = torch.empty(a.shape[0], b.shape[0], device=a.device, dtype=torch.float32)
    check(_lib.load().bg_chamfer_pairwise(ptr(a), a.shape[0], a.shape[1], ptr(b), b.shape[0], b.shape[1], ptr(out), stream()),
          "bg_chamfer_pairwise")
    return out


@torch.no_grad()
def compute_cov_mmd(sample_pcs, ref_pcs, batch_size=None):
    """pc_metric.py:83-95.  `batch_size` is accepted for the reference's signature; the result does not depend on it."""
    all_dist = pairwise_chamfer(sample_pcs, ref_pcs)
    matched = torch.argmin(all_dist, dim=1).unique().numel()        # reference clouds that are some sample's nearest
    mmd = torch.amin(all_dist, dim=0).mean()                        # every reference cloud's distance to its nearest sample
    cov = torch.tensor(matched / all_dist.shape[1], dtype=all_dist.dtype)      # reported through fp32, as the reference does
    return {"MMD-CD": mmd.item(), "COV-CD": cov.item()}


def grid_axis(resolution):
    """fp32 node coordinates of the reference's occupancy grid along one axis: `resolution` nodes from -1 to 1, node i at
    i * step - 1 evaluated in double and then rounded to fp32 (the reference fills an fp32 grid from double arithmetic)."""
    step = 2.0 / (resolution - 1)
    return (np.arange(resolution, dtype=np.float64) * step - 1.0).astype(np.float32)


@torch.no_grad()
def occupancy_counts(pclouds, grid_resolution):
    """(point_counts, cloud_counts): two int64 numpy arrays [resolution^3], the reference's grid_counters and
    grid_bernoulli_rvars (pc_metric.py:128-139).  Nearest node per axis, the lower index on an exact tie."""
    res = int(grid_resolution)
    if not 2 <= res <= MAX_RESOLUTION:
        raise ValueError(f"grid resolution {res} outside 2 .. {MAX_RESOLUTION}")
    pts = _device_clouds(pclouds, "pclouds")
    axis = torch.from_numpy(grid_axis(res)).to(pts.device)
    counts = torch.zeros(2, res ** 3, device=pts.device, dtype=torch.int32)
    check(_lib.load().bg_occupancy_counts(ptr(pts), pts.shape[0], pts.shape[1], ptr(axis), res, counts[0].data_ptr(),
                                          counts[1].data_ptr(), stream()), "bg_occupancy_counts")
    c = counts.cpu().numpy().astype(np.int64)
    return c[0], c[1]


def entropy_from_cloud_counts(cloud_counts, n_clouds):
    """Mean over the cells of the entropy (nats) of each cell's `touched by a cloud` Bernoulli variable (pc_metric.py:141-149)."""
    p = np.asarray(cloud_counts, dtype=np.float64) / float(n_clouds)
    p = p[p > 0]
    q = 1.0 - p
    h = -(p * np.log(p)) - np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0)), 0.0)
    return float(np.sum(h)) / len(cloud_counts)


def entropy_of_occupancy_grid(pclouds, grid_resolution, in_sphere=False):
    """pc_metric.py:110-149: (entropy, grid_counters) with grid_counters a float64 array [resolution^3]."""
    if in_sphere:
        raise ValueError("the sphere-clipped grid is not a product grid and is not supported (the reference never requests it)")
    reach = max(abs(v) for v in _min_max(pclouds))
    if reach > 1.001:                                    # the reference's tolerance on the unit cube
        warnings.warn(f"point clouds reach |coordinate| = {reach:.4g}: outside the unit cube the grid covers")
    point_counts, cloud_counts = occupancy_counts(pclouds, grid_resolution)
    return entropy_from_cloud_counts(cloud_counts, len(pclouds)), point_counts.astype(np.float64)


def _min_max(pcs):
    if torch.is_tensor(pcs):
        return float(pcs.min()), float(pcs.max())
    pcs = np.asarray(pcs)
    return float(pcs.min()), float(pcs.max())


def _entropy_bits(weights):
    """Shannon entropy in bits of a non-negative weight vector, normalised to sum 1."""
    prob = weights / weights.sum()
    prob = prob[prob > 0]
    return float(-(prob * np.log2(prob)).sum())


def jensen_shannon_divergence(P, Q):
    """Jensen-Shannon divergence in bits of two count vectors (the reference's quantity), in float64:
    H((p + q) / 2) - (H(p) + H(q)) / 2 with p, q the normalised counts."""
    counts = [np.asarray(v, dtype=np.float64) for v in (P, Q)]
    if counts[0].shape != counts[1].shape or counts[0].ndim != 1:
        raise ValueError(f"two count vectors of one length expected, got shapes {counts[0].shape} and {counts[1].shape}")
    if min(c.min() for c in counts) < 0 or min(c.sum() for c in counts) <= 0:
        raise ValueError("counts must be non-negative and not all zero")
    p, q = (c / c.sum() for c in counts)
    return _entropy_bits(0.5 * (p + q)) - 0.5 * (_entropy_bits(p) + _entropy_bits(q))


def jsd_between_point_cloud_sets(sample_pcs, ref_pcs, in_unit_sphere=False, resolution=28):
    """pc_metric.py:98-107: JSD between the occupancy-count distributions of two sets of clouds."""
    if in_unit_sphere:
        raise ValueError("the sphere-clipped grid is not a product grid and is not supported (the reference never requests it)")
    sample_counts = entropy_of_occupancy_grid(sample_pcs, resolution)[1]
    ref_counts = entropy_of_occupancy_grid(ref_pcs, resolution)[1]
    return jensen_shannon_divergence(sample_counts, ref_counts)


# ---- host glue: PLY files, normalisation, the evaluation loop of pc_metric.py:287-350 --------------------------------------------------

def normalize_pc(points):
    """pc_metric.py:219-226: centre on the mean, scale the largest |coordinate| to 1."""
    points = points - np.mean(points, axis=0)
    return points / np.max(np.abs(points))


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path):
    """[n, 3] array of the `vertex` element's x, y, z (float or double; `ascii` or `binary_little_endian`), the files
    sample_points.py:write_ply emits.  Other scalar vertex properties are skipped; list properties of the vertex element are not read."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: PLY header without end_header")
            tok = line.decode("ascii", errors="replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                if tok[1] == "list":
                    elements[-1][2].append((tok[-1], None))
                else:
                    if tok[1] not in _PLY_TYPES:
                        raise ValueError(f"{path}: unknown PLY property type {tok[1]}")
                    elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt not in ("ascii", "binary_little_endian"):
            raise ValueError(f"{path}: PLY format {fmt!r} is not supported (ascii, binary_little_endian)")
        if not elements or elements[0][0] != "vertex":
            raise ValueError(f"{path}: the first PLY element must be `vertex`")
        _, count, props = elements[0]
        names = [n for n, _ in props]
        if any(t is None for _, t in props) or not all(k in names for k in "xyz"):
            raise ValueError(f"{path}: the vertex element needs scalar x, y, z properties")
        for k in "xyz":
            if props[names.index(k)][1] not in ("f4", "f8"):
                raise ValueError(f"{path}: vertex {k} must be float or double")
        if fmt == "ascii":
            rows = np.loadtxt(f, dtype=np.float64, max_rows=count, ndmin=2) if count else np.zeros((0, len(props)))
            if rows.shape != (count, len(props)):
                raise ValueError(f"{path}: expected {count} vertex rows of {len(props)} values")
            cols = [rows[:, names.index(k)].astype(props[names.index(k)][1]) for k in "xyz"]
        else:
            dt = np.dtype([(n, "<" + t) for n, t in props])
            data = np.frombuffer(f.read(count * dt.itemsize), dtype=dt)
            if len(data) != count:
                raise ValueError(f"{path}: truncated vertex data")
            cols = [np.array(data[k]) for k in "xyz"]
    return np.stack(cols, axis=1)


def _load_cloud(path, rng):
    """One evaluation cloud from a PLY file: at most N_POINTS points (a random draw without replacement if the file holds more),
    then `normalize_pc` -- what the reference's loader hands to the metrics."""
    pts = read_ply(path)
    if len(pts) > N_POINTS:
        pts = pts[rng.sample(range(len(pts)), N_POINTS)]
    return normalize_pc(pts)


def _load_folder(folder, rng):
    """[n, P, 3]: every `.ply` below `folder`, in sorted path order (so that `--seed` fixes the whole run)."""
    paths = sorted(os.path.join(d, name) for d, _, names in os.walk(folder) for name in names if name.endswith(".ply"))
    if not paths:
        raise ValueError(f"no .ply file below {folder}")
    return np.stack([_load_cloud(path, rng) for path in paths])


# command line of the reference's evaluation script: (flag, type, default, help)
_CLI = (("--fake", str, None, "folder of generated clouds (.ply); the results go to <fake>_results.txt"),
        ("--real", str, None, "folder of test-set clouds (.ply)"),
        ("--n_test", int, 1000, "reference clouds per repetition"),
        ("--multi", int, 3, "generated clouds per repetition = multi * n_test"),
        ("--times", int, 10, "repetitions"),
        ("--batch_size", int, 64, "accepted for the reference's command line; unused"),
        ("--seed", int, None, "makes the subsampling repeatable"))
_SCORES = ("MMD-CD", "COV-CD", "JSD")


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m brepgen_amd.metrics", description="COV / MMD / JSD of pc_metric.py on the MI355X")
    for flag, kind, default, text in _CLI:
        parser.add_argument(flag, type=kind, default=default, help=text)
    return parser


def _run_once(fake, real, n_fake, n_real, rng):
    """One repetition: a random subset of each set, scored.  Returns {'MMD-CD', 'COV-CD', 'JSD'} as Python floats."""
    fake = fake[rng.sample(range(len(fake)), n_fake)]
    real = real[rng.sample(range(len(real)), n_real)]
    scores = compute_cov_mmd(fake, real)
    scores["JSD"] = float(jsd_between_point_cloud_sets(fake, real))
    return scores


def main(argv=None):
    opt = build_parser().parse_args(argv)
    if not opt.fake or not opt.real:
        raise SystemExit("--fake and --real are required")
    rng = random.Random(opt.seed)                       # seed None: seeded from the system, like the module-level generator
    print(f"n_test: {opt.n_test}, multiplier: {opt.multi}, repeat times: {opt.times}")
    real = _load_folder(opt.real, rng)
    print(f"real point clouds: {real.shape}")
    fake = _load_folder(opt.fake, rng)
    print(f"fake point clouds: {fake.shape}")
    runs = []
    with open(opt.fake + "_results.txt", "w") as report:
        for rep in range(opt.times):
            print(f"iteration {rep}...")
            runs.append(_run_once(fake, real, opt.multi * opt.n_test, opt.n_test, rng))
            for sink in (None, report):                 # one dict per line, on the terminal and in the file
                print(runs[-1], file=sink)
        mean = {"avg-" + key: float(np.mean([run[key] for run in runs])) for key in _SCORES}
        print("average result:")
        for sink in (None, report):
            print(mean, file=sink)
    return mean


if __name__ == "__main__":
    main()
