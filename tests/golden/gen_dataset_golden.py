#!/usr/bin/env python
"""Generate the training-batch fixtures ``tests/golden/dataset_*.npz`` from the REFERENCE's own ``dataset.py`` / ``utils.py``.

Runs on the CPU where the reference checkout is (the ``BREPGEN_REFERENCE`` environment variable names it), like gen_metrics_golden.py.
``utils.py`` imports packages that are not installable here; ``chamferdist`` and ``OCC.*`` (and ``mpl_toolkits`` / ``tqdm`` if absent)
are stubbed in ``sys.modules`` -- none of them is called by the code used here.  ``np.random.rand``, ``np.random.permutation`` and
``random.choice`` are wrapped to RECORD every draw of a ``__getitem__`` call; the recorded draws are stored as the key arrays of
include/brepgen_hip.h (``key[p[i]] = i`` replays permutation p).  The augment decision is forced per call by mapping the real draw u to
1 - u / 2 (> 0.5) or u / 2 (<= 0.5): the reference's code path is taken either way.

Records are synthetic: 4 CADs with F in {1, 2, 5, 6} at max_face 6 / max_edge 5 (face degrees cover 1 and 5; every edge of a CAD with
more than one face lies in two faces), values on the 1/8 lattice (multiples of 2^-6, so the archives compress; boxes and corners
without an exact 0, which the reference's 90-degree matrices turn into a ~1e-16 residue and the exact rotation into 0), plus one
record whose corner pairs tie exactly in x, and in x and y (used without augmentation only).  Files:

    dataset_records.npz   the records, and the table pad_repeat(arange(n), L) for 1 <= n <= L <= 12
    dataset_<kind>.npz    recorded draws and the reference's __getitem__ outputs for SurfPos / SurfZ / EdgePos / EdgeZ, plain and augmented
    dataset_points.npz    SurfData / EdgeData inputs, draws, outputs and ref_dev (the reference's deviation from the fp64 restatement)
    dataset_filter.npz    filter records (pairs exactly at fp32(0.05) after scaling and one ulp below, F = max_face + 1, a degree of
                          max_edge + 1, an empty adjacency list) and filter_data's verdicts

The generator asserts on its own inputs: no augmented corner pair ties in the leading coordinate within 1e-6, and the restatement
(tests/dataset_restate.py) meets the bounds of tests/test_dataset_cpu.py against the reference before anything is written.

    BREPGEN_REFERENCE=<reference checkout> python tests/golden/gen_dataset_golden.py
"""
import importlib
import os
import pickle
import random
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import dataset_restate as dr  # noqa: E402
from gen_metrics_golden import save_npz  # noqa: E402

REF = os.environ.get("BREPGEN_REFERENCE", "")
OUT = os.path.join(ROOT, "tests", "golden")
MAX_FACE, MAX_EDGE, BBOX_SCALED, THRESHOLD = 6, 5, 3, 0.05
KEYS12 = ("surf_wcs", "edge_wcs", "surf_ncs", "edge_ncs", "corner_wcs", "edgeFace_adj", "edgeCorner_adj", "faceEdge_adj",
          "surf_bbox_wcs", "edge_bbox_wcs", "corner_unique", "uid")
SIZE_LIMIT = 240 * 1000


class _Anything(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def import_reference():
    assert os.path.isdir(REF), "set BREPGEN_REFERENCE to the reference checkout"
    stubs = ["chamferdist", "OCC", "OCC.Core", "OCC.Core.gp", "OCC.Core.TColgp", "OCC.Core.GeomAPI", "OCC.Core.GeomAbs",
             "OCC.Core.BRepBuilderAPI", "OCC.Extend", "OCC.Extend.TopologyUtils", "OCC.Core.ShapeFix", "OCC.Core.ShapeAnalysis"]
    for name in ("mpl_toolkits.mplot3d.art3d", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            parts = name.split(".")
            stubs += [".".join(parts[:i + 1]) for i in range(len(parts))]
    for name in stubs:
        sys.modules[name] = _Anything(name)
    if "tqdm" in stubs:
        sys.modules["tqdm"].tqdm = lambda it, **kw: it
    sys.path.insert(0, REF)
    import dataset
    return dataset


class Recorder:
    """Wraps the three draw functions the reference's __getitem__ uses; `force` decides the augment branch of the next call."""

    def __init__(self):
        self.rand, self.choice, self.permutation = np.random.rand, random.choice, np.random.permutation
        self.force = None
        self.reset()

    def reset(self):
        self.u, self.angles, self.perms = [], [], []

    def __enter__(self):
        def rand():
            u = float(self.rand())
            if self.force is not None:
                u = 1.0 - u / 2 if self.force else u / 2
            self.u.append(u)
            return u

        def choice(seq):
            self.angles.append(self.choice(seq))
            return self.angles[-1]

        def permutation(n):
            self.perms.append(np.asarray(self.permutation(n)))
            return self.perms[-1]

        np.random.rand, random.choice, np.random.permutation = rand, choice, permutation
        return self

    def __exit__(self, *exc):
        np.random.rand, random.choice, np.random.permutation = self.rand, self.choice, self.permutation


# ---- synthetic records --------------------------------------------------------------------------------------------------------------

def lattice(rng, shape, lo=-8, hi=8):
    return (rng.integers(lo, hi + 1, size=shape) / 8.0).astype(np.float32)


def far_apart_boxes(rng, n):
    """n boxes [lo < 0 < hi] on the 1/8 lattice, every pair at least 1/8 apart in some coordinate (never "the same" at 3 x, 0.05).
    No coordinate is 0: there the reference's augmentation leaves a residue of cos(pi/2) ~ 1e-16 where the exact rotation gives 0."""
    while True:
        lo = lattice(rng, (n, 3), -8, -1)
        hi = lattice(rng, (n, 3), 1, 8)
        b = np.concatenate([lo, hi], 1)
        d = np.abs(b[:, None] - b[None]).max(-1) + np.eye(n)
        if n == 0 or d.min() >= 0.125:
            return b


def adjacency(rng, F):
    """faceEdge_adj and the edge count: every edge joins two faces (one face: a single closed edge)."""
    if F == 1:
        return [np.array([0])], 1
    pairs = [(0, 1)] * MAX_EDGE if F == 2 else [(i, (i + 1) % (F - (F == 6))) for i in range(F - (F == 6))]
    if F == 6:
        pairs.append((0, 5))                                # face 5 hangs on one edge: degree 1
    deg = np.bincount(np.array(pairs).ravel(), minlength=F)
    while F > 2 and deg.max() < MAX_EDGE:
        i, j = sorted(rng.choice(F - (F == 6), size=2, replace=False))
        if deg[i] < MAX_EDGE and deg[j] < MAX_EDGE:
            pairs.append((int(i), int(j)))
            deg[i] += 1
            deg[j] += 1
    adj = [[] for _ in range(F)]
    for e, (i, j) in enumerate(pairs):
        adj[i].append(e)
        adj[j].append(e)
    return [np.array(a) for a in adj], len(pairs)


def corner_pairs(rng, n):
    """[n, 2, 3] on the 1/8 lattice without 0; the two corners of a pair differ in every coordinate (no tie under any rotation)."""
    while True:
        c = lattice(rng, (n, 2, 3), 1, 8) * rng.choice(np.float32([-1, 1]), size=(n, 2, 3))
        if (c[:, 0] != c[:, 1]).all():
            return c


def make_record(rng, F, adj=None, n_edges=None, grids=True):
    if adj is None:
        adj, n_edges = adjacency(rng, F)
    shape = (lambda *s: lattice(rng, s)) if grids else (lambda *s: np.zeros(s, np.float32))
    rec = {k: None for k in KEYS12}
    rec.update(surf_ncs=shape(F, 32, 32, 3), edge_ncs=shape(n_edges, 32, 3), corner_wcs=corner_pairs(rng, n_edges),
               faceEdge_adj=adj, surf_bbox_wcs=far_apart_boxes(rng, F), edge_bbox_wcs=far_apart_boxes(rng, n_edges), uid="synthetic")
    return rec


def tie_record(rng):
    rec = make_record(rng, 2)
    c = rec["corner_wcs"]
    c[0] = [[0.5, 0.25, -0.125], [0.5, -0.25, 0.75]]        # tie in x: y decides, the pair swaps
    c[1] = [[-0.25, 0.125, 0.5], [-0.25, 0.125, -0.5]]      # tie in x and y: z decides, the pair swaps
    c[2] = [[0.375, -0.5, 0.25], [0.375, 0.5, -1.0]]        # tie in x: already in order
    c[3] = [[0.125, 0.125, 0.125], [0.125, 0.125, 0.125]]   # full tie
    return rec


def pack_records(records, prefix):
    out = {prefix + "count": np.int64(len(records))}
    for r, rec in enumerate(records):
        for k in ("surf_ncs", "edge_ncs", "corner_wcs", "surf_bbox_wcs", "edge_bbox_wcs"):
            out[f"{prefix}{r}_{k}"] = rec[k]
        out[f"{prefix}{r}_adj_idx"] = np.concatenate([np.asarray(a, dtype=np.int32) for a in rec["faceEdge_adj"]] + [np.zeros(0, np.int32)])
        out[f"{prefix}{r}_adj_off"] = np.cumsum([0] + [len(a) for a in rec["faceEdge_adj"]]).astype(np.int32)
    return out


def write_pickles(records, folder, tag):
    paths = []
    for r, rec in enumerate(records):
        paths.append(os.path.join(folder, f"{tag}{r}.pkl"))
        with open(paths[-1], "wb") as f:
            pickle.dump(rec, f)
    return paths


# ---- the reference's __getitem__, with its draws ----------------------------------------------------------------------------------------

def draws_of(kind, rec, recorder):
    F, perms = len(rec["surf_bbox_wcs"]), list(recorder.perms)
    d = {"u": np.float64(recorder.u[0]), "turns": np.array([a // 90 for a in recorder.angles] or [1, 1, 1], np.int32),
         "face_key1": np.zeros(MAX_FACE, np.uint32), "face_key2": np.zeros(MAX_FACE, np.uint32),
         "edge_key1": np.zeros((MAX_FACE, MAX_EDGE), np.uint32), "edge_key2": np.zeros((MAX_FACE, MAX_EDGE), np.uint32)}
    assert len(recorder.u) == 1 and len(recorder.angles) in (0, 3)
    if kind in ("EdgePos", "EdgeZ"):
        for f in range(F):
            d["edge_key1"][f] = dr.keys_of(perms.pop(0), MAX_EDGE)
            if kind == "EdgePos":
                d["edge_key2"][f] = dr.keys_of(perms.pop(0), MAX_EDGE)
    d["face_key1"] = dr.keys_of(perms.pop(0), MAX_FACE)
    if kind == "SurfPos":
        d["face_key2"] = dr.keys_of(perms.pop(0), MAX_FACE)
    assert not perms
    return d


def ldm_goldens(ds_mod, kind, records, paths, recorder):
    """name -> array: per mode ("plain": every record, aug off; "aug": records 0-3, augmentation forced) the stacked draws and outputs."""
    cls = getattr(ds_mod, kind + "Data")
    arrays = {}
    for mode, ids in (("plain", list(range(len(records)))), ("aug", [0, 1, 2, 3])):
        obj = cls.__new__(cls)
        obj.max_face, obj.max_edge, obj.bbox_scaled, obj.aug, obj.data = MAX_FACE, MAX_EDGE, BBOX_SCALED, mode == "aug", paths
        draws, outs = [], []
        for r in ids:
            recorder.reset()
            recorder.force = mode == "aug"
            item = obj[r]
            item = item if isinstance(item, tuple) else (item,)
            outs.append([t.numpy() for t in item])
            draws.append(draws_of(kind, records[r], recorder))
            assert (len(recorder.angles) == 3) == (mode == "aug")
        arrays[f"{mode}_records"] = np.array(ids, np.int32)
        for k in draws[0]:
            arrays[f"{mode}_draw_{k}"] = np.stack([d[k] for d in draws])
        for i in range(len(outs[0])):
            arrays[f"{mode}_out{i}"] = np.stack([o[i] for o in outs])
        # the restatement against the reference, by the bounds the tests use
        stacked = {k: arrays[f"{mode}_draw_{k}"] for k in draws[0]}
        mine = dr.batch(records, ids, kind, MAX_FACE, MAX_EDGE, BBOX_SCALED, mode == "aug", stacked)
        for i, (a, b) in enumerate(zip(mine, (arrays[f"{mode}_out{i}"] for i in range(len(mine))))):
            check_output(kind, mode, i, a, b)
    return arrays


GRID_OUTPUTS = {"SurfZ": (1,), "EdgePos": (1,), "EdgeZ": (0, 3), "SurfPos": ()}


def check_output(kind, mode, i, mine, ref):
    assert mine.shape == ref.shape, (kind, mode, i, mine.shape, ref.shape)
    if mode == "aug" and i in GRID_OUTPUTS[kind]:
        bound = dr.ulp32(ref) + 2.0 ** -50 * float(np.abs(ref).max())
        assert (np.abs(mine.astype(np.float64) - ref.astype(np.float64)) <= bound).all(), (kind, mode, i)
    elif ref.dtype == np.bool_:
        assert mine.dtype == np.bool_ and (mine == ref).all(), (kind, mode, i)
    else:
        assert mine.dtype == np.float32 and ref.dtype == np.float32
        assert (mine.view(np.uint32) == ref.view(np.uint32)).all(), (kind, mode, i, int((mine.view(np.uint32) != ref.view(np.uint32)).sum()))


def assert_no_augmented_corner_ties(records, arrays):
    for b, r in enumerate(arrays["aug_records"]):
        code = dr.rot_code(arrays["aug_draw_turns"][b])
        c = dr.rot3(records[r]["corner_wcs"].astype(np.float64), code)
        assert (np.abs(c[:, 0, 0] - c[:, 1, 0]) > 1e-6).all(), f"record {r}: an augmented corner pair ties in the leading coordinate"
        for k in ("corner_wcs", "surf_bbox_wcs", "edge_bbox_wcs"):
            assert (records[r][k] != 0).all(), f"record {r}: an exact 0 in {k} (the reference rotates it to ~1e-16, not to 0)"


# ---- point augmentation ---------------------------------------------------------------------------------------------------------------

def point_goldens(ds_mod, recorder, rng):
    arrays = {}
    for name, cls, shape, force in (("surf", ds_mod.SurfData, (4, 32, 32, 3), (True, False, True, True)),
                                    ("edge", ds_mod.EdgeData, (6, 32, 3), (True, True, False, True, False, True))):
        data = (rng.uniform(-1, 1, size=shape) * rng.uniform(0.2, 1.0, size=(shape[0],) + (1,) * (len(shape) - 1))).astype(np.float32)
        obj = cls.__new__(cls)
        obj.validate, obj.aug, obj.data = False, True, data
        u, turns, outs = [], [], []
        for m in range(shape[0]):
            recorder.reset()
            recorder.force = force[m]
            outs.append(obj[m].numpy())
            u.append(recorder.u[0])
            turns.append([a // 90 for a in recorder.angles] or [1, 1, 1])
        out = np.stack(outs)
        u, turns = np.array(u), np.array(turns, np.int32)
        flat = data.reshape(shape[0], -1, 3)
        r32 = dr.augment_points(flat, u, turns, True, "fp32").reshape(shape)
        r64 = dr.augment_points(flat, u, turns, True, "fp64").reshape(shape)
        ref_dev = 0.0
        for m in range(shape[0]):
            top = float(np.abs(out[m]).max())
            bound = dr.ulp32(out[m]) + 2.0 ** -48 * top
            assert (np.abs(r32[m].astype(np.float64) - out[m].astype(np.float64)) <= bound).all(), (name, m)
            ref_dev = max(ref_dev, float(np.abs(r64[m].astype(np.float64) - out[m].astype(np.float64)).max()) / top)
            if not force[m]:
                assert (out[m].view(np.uint32) == data[m].view(np.uint32)).all()
        arrays.update({f"{name}_x": data, f"{name}_u": u, f"{name}_turns": turns, f"{name}_out": out, f"{name}_ref_dev": np.float64(ref_dev)})
        print(f"points {name}: ref_dev = {ref_dev:.3e} (relative to max|ref|)")
    return arrays


# ---- admission filter -------------------------------------------------------------------------------------------------------------------

def at_threshold(below):
    """fp32 (a, b) with |fp32(a * 3) - fp32(b * 3)| == fp32(0.05) exactly in fp32 (below: one ulp under it), found by search among
    the neighbours of 0.05 / 3 (b) and the first multiples of 2^-29 (a)."""
    target = np.float32(THRESHOLD)
    if below:
        target = np.nextafter(target, np.float32(0))
    three = np.float32(BBOX_SCALED)
    for k in range(16):
        a = np.float32(k * 2.0 ** -29)
        b = np.float32(THRESHOLD / 3)
        for _ in range(64):
            b = np.nextafter(b, np.float32(0))
        for _ in range(128):
            if np.abs(np.float32(a * three) - np.float32(b * three)) == target:
                return a, b
            b = np.nextafter(b, np.float32(1))
    raise AssertionError("no fp32 pair maps onto the threshold")


def filter_records(rng):
    recs, notes = [], []

    def add(note, rec):
        recs.append(rec)
        notes.append(note)

    add("plain", make_record(rng, 5, grids=False))
    for what in ("surf_bbox_wcs", "edge_bbox_wcs"):
        for below in (False, True):
            rec = make_record(rng, 2, grids=False)                 # both faces list edges 0 .. 4
            rec[what][1] = rec[what][0]
            rec[what][0, 4], rec[what][1, 4] = at_threshold(below)
            add(f"{what} pair {'one ulp below' if below else 'exactly at'} the threshold", rec)
    add("F = max_face + 1", make_record(rng, MAX_FACE + 1, grids=False))
    adj = [np.arange(MAX_EDGE + 1), np.arange(MAX_EDGE + 1)]
    add("a degree of max_edge + 1", make_record(rng, 2, adj, MAX_EDGE + 1, grids=False))
    adj = [np.array([0, 1]), np.zeros(0, np.int64), np.array([0, 1])]
    add("an empty adjacency list", make_record(rng, 3, adj, 2, grids=False))
    rec = make_record(rng, 6, grids=False)                         # the same edge box twice, but never within one face's list
    lists = rec["faceEdge_adj"]
    e_a = int(lists[5][0])
    e_b = next(e for e in range(len(rec["edge_bbox_wcs"])) if not any(e in a and e_a in a for a in lists))
    rec["edge_bbox_wcs"][e_b] = rec["edge_bbox_wcs"][e_a]
    add("equal edge boxes in different faces", rec)
    return recs, notes


def main():
    ds_mod = import_reference()
    rng = np.random.default_rng(20)
    np.random.seed(7)
    random.seed(7)
    records = [make_record(rng, F) for F in (1, 2, 5, 6)] + [tie_record(rng)]
    degrees = sorted({len(a) for rec in records for a in rec["faceEdge_adj"]})
    assert degrees[0] == 1 and degrees[-1] == MAX_EDGE, degrees
    files = {}
    table = {f"pad_repeat_{n}_{L}": ds_mod.pad_repeat(np.arange(n), L).astype(np.int32) for L in range(1, 13) for n in range(1, L + 1)}
    for (n, L), v in (((int(k.split("_")[2]), int(k.split("_")[3])), v) for k, v in table.items()):
        assert (dr.pad_repeat_src(n, L) == v).all(), (n, L)
    files["dataset_records"] = {**pack_records(records, "r"), **table}
    with tempfile.TemporaryDirectory() as tmp, Recorder() as recorder:
        paths = write_pickles(records, tmp, "cad")
        for kind in dr.KINDS:
            arrays = ldm_goldens(ds_mod, kind, records, paths, recorder)
            if kind == "EdgeZ":
                assert_no_augmented_corner_ties(records, arrays)
            files["dataset_" + kind.lower()] = arrays
        files["dataset_points"] = point_goldens(ds_mod, recorder, rng)
        frecs, notes = filter_records(rng)
        fpaths = write_pickles(frecs, tmp, "filter")
        verdict = np.array([ds_mod.filter_data((p, MAX_FACE, MAX_EDGE, BBOX_SCALED, THRESHOLD, -1))[0] is not None for p in fpaths])
        mine = np.array([dr.keep(rec, MAX_FACE, MAX_EDGE, BBOX_SCALED, THRESHOLD) for rec in frecs])
        for note, v in zip(notes, verdict):
            print(f"filter: {'keep' if v else 'drop'}  {note}")
        assert (mine == verdict).all(), (mine, verdict)
        assert verdict.tolist() == [True, True, False, True, False, False, False, False, True], verdict
        files["dataset_filter"] = {**pack_records(frecs, "r"), "keep": verdict, "notes": np.array(notes)}
    for name, arrays in files.items():
        path = os.path.join(OUT, name + ".npz")
        save_npz(path, arrays)
        size = os.path.getsize(path)
        print(f"{name}: {size} bytes")
        assert size <= SIZE_LIMIT, (name, size)


if __name__ == "__main__":
    main()
