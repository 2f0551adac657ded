#!/usr/bin/env python
"""Generate the de-duplication fixtures ``tests/golden/dedup_*.npz`` by running the REFERENCE's own ``data_process/deduplicate_cad.py``
and ``deduplicate_surfedge.py``.

Runs on the CPU where the reference checkout is (the ``BREPGEN_REFERENCE`` environment variable names it), like
gen_dataset_golden.py.  ``convert_utils.py`` imports ``occwl.*``, which is not installable here: those modules (and ``tqdm`` if absent)
are stubbed in ``sys.modules`` -- none of them is called by the two scripts.  The scripts themselves are run with ``runpy`` and a
patched ``sys.argv``, option ``furniture``, 6 bits, on a temporary folder of synthetic 12-key records written in ``process_brep.py``'s
key order (``deduplicate_surfedge.py`` unpacks ``data.values()`` positionally).

``deduplicate_cad.py`` takes its train list from ``load_furniture_pkl``: ``os.walk`` order, ``random.shuffle``, the first 90 %.  First
occurrence depends on that order, and ``os.walk``'s is the file system's, so ``random.shuffle`` is patched for the run to SORT the list
(the identity would leave the file system's order in place): 12 records ``cads/cad_00.pkl`` .. ``cad_11.pkl`` become the train list in
that order and two fillers ``cads/zz_0.pkl`` / ``zz_1.pkl`` the val and test entries.  The visited order is stored.
``deduplicate_surfedge.py`` is run on that full train list, for surfaces and for edges.

Records (values on the 1/8 lattice, smooth patches, so the archive compresses; ``*_wcs`` and ``*_ncs`` are different arrays):

    0  three faces                          1  exact repeat of 0 (duplicate)         2  0 with its faces permuted (duplicate)
    3  faces [a, a, b]                      4  faces [a, b, b] (not a duplicate of 3)
    5, 6  share one face and two edges (deduplicate_surfedge.py keeps them once); 5 holds one edge twice
    7  one face s                           8  s with one coordinate moved by 0.3 of a 6-bit step, same side of the boundary (duplicate)
    9  s with that coordinate moved by 0.7 of a step, across the boundary (kept)
    10 six faces                            11 one face whose first 192 values are the 6-bit lattice points 2k/63 - 1 and their fp32
                                               neighbours: an fp64 or fused evaluation of real2bit changes this record's digest

Before anything is written the generator asserts that tests/dedup_restate.py reproduces the scripts' outputs.

    BREPGEN_REFERENCE=<reference checkout> python tests/golden/gen_dedup_golden.py
"""
import importlib
import os
import pickle
import random
import runpy
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import dedup_restate as dd  # noqa: E402
from gen_metrics_golden import save_npz  # noqa: E402

REF = os.environ.get("BREPGEN_REFERENCE", "")
OUT = os.path.join(ROOT, "tests", "golden")
BIT = 6
SIZE_LIMIT = 240 * 1000


class _Anything(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def stub_imports():
    stubs = ["occwl", "occwl.uvgrid", "occwl.compound", "occwl.solid", "occwl.shell", "occwl.entity_mapper"]
    try:
        importlib.import_module("tqdm")
    except ImportError:
        stubs.append("tqdm")
    for name in stubs:
        sys.modules[name] = _Anything(name)
    if "tqdm" in stubs:
        sys.modules["tqdm"].tqdm = lambda it, **kw: it


def run_script(name, argv, cwd):
    """The reference's script as __main__ with its own folder importable (convert_utils) and `cwd` as the working directory."""
    folder = os.path.join(REF, "data_process")
    old_argv, old_cwd, old_shuffle = sys.argv, os.getcwd(), random.shuffle
    sys.argv, random.shuffle = [name] + argv, lambda lst: lst.sort()
    sys.path.insert(0, folder)
    sys.modules.pop("convert_utils", None)
    os.chdir(cwd)
    try:
        runpy.run_path(os.path.join(folder, name), run_name="__main__")
    finally:
        os.chdir(old_cwd)
        sys.path.remove(folder)
        sys.argv, random.shuffle = old_argv, old_shuffle


def patch(g, shape):
    """A smooth random patch [*shape, 3] in [-1, 1] on the 1/8 lattice."""
    axes = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing="ij")
    out = np.zeros(shape + (3,))
    for c in range(3):
        v = g.uniform(-0.4, 0.4)
        for a in axes:
            v = v + g.uniform(-0.5, 0.5) * a
        if len(axes) == 2:
            v = v + g.uniform(-0.4, 0.4) * axes[0] * axes[1]
        out[..., c] = v
    return (np.round(np.clip(out, -1.0, 1.0) * 8.0) / 8.0).astype(np.float32)


def moved(face, step_fraction):
    """`face` with coordinate [5, 7, 1] at 0.5 + step_fraction of the way from 6-bit level 40 to 41."""
    out = face.copy()
    out[5, 7, 1] = np.float32(2.0 * (40.5 + step_fraction) / 63.0 - 1.0)
    return out


def build_records():
    g = np.random.default_rng(20240807)
    sw = [patch(g, (32, 32)) for _ in range(20)]      # surf_wcs pool
    sn = [patch(g, (32, 32)) for _ in range(20)]      # surf_ncs pool (same sharing structure, other values)
    ew = [patch(g, (32,)) for _ in range(24)]
    en = [patch(g, (32,)) for _ in range(24)]
    for pool in (sw, sn):
        pool[12], pool[13], pool[14] = moved(pool[12], 0.0), moved(pool[12], 0.3), moved(pool[12], 0.7)
        pool[19].reshape(-1)[:192] = dd.lattice_neighbours(BIT)
    faces = [[0, 1, 2], [0, 1, 2], [2, 0, 1], [3, 3, 4], [3, 4, 4], [5, 6], [6, 7], [12], [13], [14], [8, 9, 10, 11, 15, 16], [19]]
    edges = [[0, 1, 2], [0, 1, 2], [2, 0, 1], [3, 4], [4, 5], [6, 7, 8, 7], [7, 8, 9], [10, 11], [10, 12], [13, 14],
             [15, 16, 17, 18, 19], [20, 21]]
    records = []
    for r, (fs, es) in enumerate(zip(faces, edges)):
        rec = {k: np.zeros(0, np.float32) for k in dd.KEYS12}
        rec["surf_wcs"], rec["surf_ncs"] = np.stack([sw[f] for f in fs]), np.stack([sn[f] for f in fs])
        rec["edge_wcs"], rec["edge_ncs"] = np.stack([ew[e] for e in es]), np.stack([en[e] for e in es])
        rec["uid"] = f"cad_{r:02d}"
        records.append(rec)
    fillers = []
    for r in range(2):
        rec = dict(records[0], uid=f"zz_{r}")
        fillers.append(rec)
    # the boundary trio does what its description says, in the reference's own arithmetic
    q = [dd.real2bit_numpy(sw[i], BIT)[5, 7, 1] for i in (12, 13, 14)]
    assert q[0] == q[1] == 40 and q[2] == 41 and abs(float(sw[13][5, 7, 1]) - float(sw[14][5, 7, 1])) < 2.0 / 63.0, q
    return records, fillers


def main():
    assert os.path.isdir(os.path.join(REF, "data_process")), "set BREPGEN_REFERENCE to the reference checkout"
    stub_imports()
    records, fillers = build_records()
    with tempfile.TemporaryDirectory() as tmp:
        assert "." not in tmp, "deduplicate_surfedge.py cuts its output name at the first dot of the list's path"
        os.makedirs(os.path.join(tmp, "data", "cads"))
        for rec in records + fillers:
            assert tuple(rec) == dd.KEYS12
            with open(os.path.join(tmp, "data", "cads", rec["uid"] + ".pkl"), "wb") as f:
                pickle.dump(rec, f)
        data = os.path.join(tmp, "data")
        run_script("deduplicate_cad.py", ["--data", data, "--bit", str(BIT), "--option", "furniture"], tmp)
        with open(os.path.join(tmp, f"furniture_data_split_{BIT}bit.pkl"), "rb") as f:
            split = pickle.load(f)
        order = [f"cads/{rec['uid']}.pkl" for rec in records]             # what the sorted "shuffle" makes load_furniture_pkl return
        assert split["val"] == ["cads/zz_0.pkl"] and split["test"] == ["cads/zz_1.pkl"] and set(split["train"]) <= set(order)
        with open(os.path.join(tmp, "full.pkl"), "wb") as f:
            pickle.dump({"train": order, "val": split["val"], "test": split["test"]}, f)
        unique = {}
        for which, flag in (("surface", []), ("edge", ["--edge"])):
            run_script("deduplicate_surfedge.py", ["--data", data, "--list", os.path.join(tmp, "full.pkl"), "--bit", str(BIT),
                                                   "--option", "furniture"] + flag, tmp)
            with open(os.path.join(tmp, f"full_{which}.pkl"), "rb") as f:
                unique[which] = np.array(pickle.load(f), dtype=np.float32)

    # the restatement reproduces the scripts before anything is written
    keep = dd.dedup_cads(records, BIT)
    assert [u for u, k in zip(order, keep) if k] == split["train"], (keep, split["train"])
    assert keep.tolist() == [True, False, False, True, True, True, True, True, False, True, True, True], keep
    ref_keys = [dd.reference_key([dd.item_digest(s, BIT) for s in rec["surf_wcs"]]) for rec in records]
    assert dd.first_occurrence(ref_keys).tolist() == keep.tolist()
    for which, key in (("surface", "surf_ncs"), ("edge", "edge_ncs")):
        got = dd.unique_items(records, key, BIT)
        assert got.shape == unique[which].shape and got.tobytes() == unique[which].tobytes(), which
    n_surf, n_edge = sum(len(r["surf_ncs"]) for r in records), sum(len(r["edge_ncs"]) for r in records)
    assert len(unique["surface"]) < n_surf and len(unique["edge"]) < n_edge
    for n in (1, 6, 8, 16):
        x = dd.lattice_neighbours(n)
        assert (dd.real2bit(x, n) == dd.real2bit_numpy(x, n)).all(), n

    arrays = {"rcount": np.int64(len(records)), "order": np.array(order), "bit": np.int64(BIT)}
    for r, rec in enumerate(records):
        for k in dd.GRID_KEYS:
            arrays[f"r{r}_{k}"] = rec[k]
        arrays[f"r{r}_uid"] = np.array(rec["uid"])
    outputs = {"bit": np.int64(BIT), "cad_train": np.array(split["train"]), "cad_val": np.array(split["val"]),
               "cad_test": np.array(split["test"]), "surface_unique": unique["surface"], "edge_unique": unique["edge"]}
    for name, arr in (("records", arrays), ("outputs", outputs)):
        path = os.path.join(OUT, f"dedup_{name}.npz")
        save_npz(path, arr)
        size = os.path.getsize(path)
        assert size <= SIZE_LIMIT, (path, size)
        print(f"{path}: {size} bytes")


if __name__ == "__main__":
    main()
