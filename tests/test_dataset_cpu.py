"""CPU-side checks of the training-batch assembly (brepgen_amd/dataset.py, csrc/batch.hip): the numpy restatement
(tests/dataset_restate.py) against the reference's own outputs (tests/golden/dataset_*.npz, gen_dataset_golden.py), and the ABI
boundary.  No kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import brepgen_amd as bga
from brepgen_amd import _lib, dataset
from tests import dataset_restate as dr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_FACE, MAX_EDGE = 6, 5


def golden(name):
    return np.load(os.path.join(GOLDEN, f"dataset_{name}.npz"))


@pytest.fixture(scope="module")
def records():
    return dr.load_records(golden("records"))


@pytest.mark.parametrize("mode", ["plain", "aug"])
@pytest.mark.parametrize("kind", list(dr.KINDS))
def test_restatement_against_the_reference(records, kind, mode):
    """Masks, every not-augmented output, and the boxes and corners of augmented outputs bitwise; augmented grids within
    ulp32(ref) + 2^-50 max|ref| (dataset_restate.assert_output)."""
    g = golden(kind.lower())
    ids = g[f"{mode}_records"].tolist()
    draws = {k: g[f"{mode}_draw_{k}"] for k in ("u", "turns", "face_key1", "face_key2", "edge_key1", "edge_key2")}
    assert (draws["u"] > 0.5).all() if mode == "aug" else (draws["u"] <= 0.5).all()
    got = dr.batch(records, ids, kind, MAX_FACE, MAX_EDGE, 3, mode == "aug", draws)
    assert len(got) == sum(k.startswith(f"{mode}_out") for k in g.files)
    for i, t in enumerate(got):
        dr.assert_output(t, g[f"{mode}_out{i}"], mode == "aug" and i in dr.GRID_OUTPUTS[kind], (kind, mode, i))


def test_the_tie_record_orders_its_corners_by_the_next_coordinate(records):
    """Record 4 (plain only): corner pairs tying exactly in x, and in x and y, come out ordered by the next coordinate."""
    v = dr._corners(records[4]["corner_wcs"], 0, 3).reshape(-1, 2, 3)
    assert (v[0, 0] == np.float32([1.5, -0.75, 2.25])).all() and (v[1, 0] == np.float32([-0.75, 0.375, -1.5])).all()
    assert (v[2, 0] == np.float32([1.125, -1.5, 0.75])).all() and (v[3, 0] == v[3, 1]).all()


def test_pad_repeat_table():
    g = golden("records")
    names = [k for k in g.files if k.startswith("pad_repeat_")]
    assert len(names) == 12 * 13 // 2
    for k in names:
        n, L = (int(v) for v in k.split("_")[2:])
        src = dr.pad_repeat_src(n, L)
        assert (src == g[k]).all(), (n, L)
        counts = np.bincount(src, minlength=n)
        assert set(counts.tolist()) <= {L // n, L // n + 1} and counts.sum() == L


def test_filter_restatement_against_filter_data():
    g = golden("filter")
    recs = dr.load_records(g)
    got = [dr.keep(rec, MAX_FACE, MAX_EDGE, 3, 0.05) for rec in recs]
    assert got == g["keep"].tolist(), list(zip(g["notes"].tolist(), got))
    assert 0 < sum(got) < len(got)


@pytest.mark.parametrize("name", ["surf", "edge"])
def test_point_augmentation_restatement(name):
    """The restatement with the reference's fp32 first centre meets ulp32 + 2^-48 max|ref| against the reference; items that were not
    augmented are bitwise copies; the fp64 restatement deviates by the stored ref_dev."""
    g = golden("points")
    x, u, turns, ref = g[f"{name}_x"], g[f"{name}_u"], g[f"{name}_turns"], g[f"{name}_out"]
    M = len(x)
    assert (u > 0.5).any() and (u <= 0.5).any()
    r32 = dr.augment_points(x.reshape(M, -1, 3), u, turns, True, "fp32").reshape(x.shape)
    r64 = dr.augment_points(x.reshape(M, -1, 3), u, turns, True, "fp64").reshape(x.shape)
    for m in range(M):
        if u[m] <= 0.5:
            assert r32[m].tobytes() == x[m].tobytes() == ref[m].tobytes() == r64[m].tobytes()
            continue
        top = float(np.abs(ref[m]).max())
        d = np.abs(r32[m].astype(np.float64) - ref[m])
        assert (d <= dr.ulp32(ref[m]) + 2.0 ** -48 * top).all(), (m, float(d.max()))
        assert float(np.abs(r64[m].astype(np.float64) - ref[m]).max()) <= float(g[f"{name}_ref_dev"]) * top
    assert dr.augment_points(x.reshape(M, -1, 3), u, turns, False).tobytes() == x.tobytes()


# ---- the ABI boundary -------------------------------------------------------------------------------------------------------------

NEW_ENTRIES = ("bg_cad_filter", "bg_batch_plan", "bg_batch_gather", "bg_points_rotate_normalize")


def test_exports_and_signatures():
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name][1] and getattr(lib, name).restype is C.c_int
    assert lib.bg_abi_version() == 7 == _lib.ABI_VERSION                       # added entries: the ABI number stays
    for name in ("CADStore", "augment_points"):
        assert getattr(bga, name) is getattr(dataset, name) and name in bga.__all__
    # the C structs as the header lays them out (LP64: 9 pointers + 4 ints; 6 pointers; 7 pointers)
    assert (C.sizeof(_lib.CadStore), C.sizeof(_lib.BatchDraws), C.sizeof(_lib.BatchOut)) == (88, 48, 56)


def test_argument_errors_are_negative_and_explained():
    lib = _lib.load()
    fake = 0x10000                                    # aligned, never dereferenced: validation fails first

    def store(**kw):
        s = _lib.CadStore(*([fake] * 9), 4, 10, 20, 40)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    out = _lib.BatchOut(*([fake] * 7))
    plan = lambda st=store(), idx=fake, B=2, kind=3, S=6, E=5, face=fake, edge=fake, rot=fake, scale=fake: lib.bg_batch_plan(   # noqa: E731
        C.byref(st) if st is not None else None, idx, B, kind, S, E, 1, 1, 0, None, face, edge, rot, scale, None)
    gather = lambda st=store(), kind=3, B=2, S=6, E=5, face=fake, edge=fake, rot=fake, scale=fake, o=out: lib.bg_batch_gather(   # noqa: E731
        C.byref(st) if st is not None else None, kind, B, S, E, 3.0, face, edge, rot, scale, C.byref(o) if o is not None else None, None)

    for call in (plan, gather):
        assert call(st=None) == _lib.BG_E_ARG and b"null" in lib.bg_last_error()
        assert call(st=store(adj_idx=None)) == _lib.BG_E_ARG and b"null" in lib.bg_last_error()
        assert call(st=store(n_faces=-1)) == _lib.BG_E_SHAPE and b"negative" in lib.bg_last_error()
        assert call(st=store(edge_ncs=fake + 4)) == _lib.BG_E_ALIGN and b"aligned" in lib.bg_last_error()
        assert call(kind=4) == _lib.BG_E_ARG and b"kind" in lib.bg_last_error()
        for kw in (dict(B=-1), dict(S=0), dict(E=0), dict(S=513, E=1), dict(S=64, E=65)):
            assert call(**kw) == _lib.BG_E_SHAPE and b"max_face" in lib.bg_last_error(), kw
        assert call(face=None) == _lib.BG_E_ARG and call(rot=None) == _lib.BG_E_ARG and call(scale=None) == _lib.BG_E_ARG
        assert call(edge=None) == _lib.BG_E_ARG and b"edge_src" in lib.bg_last_error()
        assert call(B=0, face=None) == 0                                       # nothing to do
    assert plan(idx=None) == _lib.BG_E_ARG
    assert gather(o=None) == _lib.BG_E_ARG
    assert gather(o=_lib.BatchOut(fake, fake, fake, fake, None, fake, fake)) == _lib.BG_E_ARG and b"output" in lib.bg_last_error()
    assert gather(o=_lib.BatchOut(fake, fake + 8, fake, fake, fake, fake, fake)) == _lib.BG_E_ALIGN

    filt = lambda st=store(), S=6, E=5, keep=fake: lib.bg_cad_filter(C.byref(st) if st is not None else None, S, E, 3.0, 0.05, keep, None)   # noqa: E731
    assert filt(st=None) == _lib.BG_E_ARG and b"null" in lib.bg_last_error()
    assert filt(S=0) == _lib.BG_E_SHAPE and filt(E=0) == _lib.BG_E_SHAPE and lib.bg_last_error()
    assert filt(keep=None) == _lib.BG_E_ARG and b"keep" in lib.bg_last_error()
    assert filt(st=store(n_records=0), keep=None) == 0

    pts = lambda x=fake, M=3, P=32, first=0, u=None, turns=None, o=fake: lib.bg_points_rotate_normalize(x, M, P, 1, 1, 0, first, u, turns, o, None)   # noqa: E731
    assert pts(x=None) == _lib.BG_E_ARG and b"null" in lib.bg_last_error()
    assert pts(o=None) == _lib.BG_E_ARG
    for kw in (dict(P=0), dict(P=1025), dict(M=-1), dict(first=-1)):
        assert pts(**kw) == _lib.BG_E_SHAPE and lib.bg_last_error(), kw
    assert pts(turns=fake) == _lib.BG_E_ARG and b"turns" in lib.bg_last_error()
    assert pts(M=0, x=None, o=None) == 0


def test_oversize_records_raise_before_any_launch(records):
    """F > max_face, a degree > max_edge or an empty adjacency list: ValueError on the host, from the sizes the store keeps there."""
    store = dataset.CADStore.__new__(dataset.CADStore)           # the host side alone: no device is touched
    store._summarise(records, None)
    assert store.n_faces.tolist() == [1, 2, 5, 6, 2] and store.max_degree.max() == MAX_EDGE and store.min_degree.min() == 1
    assert store._indices([0, 3, 4], MAX_FACE, MAX_EDGE).tolist() == [0, 3, 4]
    with pytest.raises(ValueError, match="max_face"):
        store._indices([0, 3], MAX_FACE - 1, MAX_EDGE)
    with pytest.raises(ValueError, match="max_edge"):
        store._indices([2], MAX_FACE, MAX_EDGE - 1)
    with pytest.raises(ValueError, match="record numbers"):
        store._indices([5], MAX_FACE, MAX_EDGE)
    empty = dict(records[1], faceEdge_adj=[records[1]["faceEdge_adj"][0], np.zeros(0, np.int64)])
    store._summarise([empty], None)
    with pytest.raises(ValueError, match="0 edges"):
        store._indices([0], MAX_FACE, MAX_EDGE)
    with pytest.raises(ValueError, match="outside"):
        store._summarise([dict(records[1], faceEdge_adj=[np.array([0, 99]), np.array([1])])], None)
    with pytest.raises(ValueError, match="shape"):
        store._summarise([dict(records[1], surf_ncs=records[1]["surf_ncs"][:1])], None)


def test_no_cpu_fallback(records, monkeypatch):
    with pytest.raises(_lib.BrepgenHipError):
        bga.CADStore.from_records(records, device="cpu")
    with pytest.raises(_lib.BrepgenHipError):
        bga.augment_points(torch.zeros(2, 32, 3))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # also where the suite runs next to a GPU
    with pytest.raises(_lib.BrepgenHipError):
        bga.CADStore.from_records(records)


def test_the_product_does_not_import_the_oracle():
    src = open(dataset.__file__).read()
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", src, flags=re.M)
    modules = {v.__name__.split(".")[0] for v in vars(dataset).values() if isinstance(v, type(os))}
    assert not modules & {"oracle", "tests"}, modules
