"""CPU-side checks of the training-set de-duplication (brepgen_amd/deduplicate.py, csrc/hash_dedup.hip): the numpy + hashlib
restatement (tests/dedup_restate.py) against the reference's scripts' own outputs (tests/golden/dedup_*.npz, gen_dedup_golden.py), the
quantisation's rounding order, and the ABI boundary.  Every comparison is exact.  No kernel is launched."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest
import torch

import brepgen_amd as bga
from brepgen_amd import _lib, dataset, deduplicate
from tests import dedup_restate as dd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_ENTRIES = ("bg_points_sha256", "bg_digest_group_keys", "bg_first_occurrence")


@pytest.fixture(scope="module")
def fixtures():
    rec = np.load(os.path.join(GOLDEN, "dedup_records.npz"))
    return dd.load_records(rec), rec["order"].tolist(), np.load(os.path.join(GOLDEN, "dedup_outputs.npz"))


def test_restatement_reproduces_the_reference_scripts(fixtures):
    records, order, out = fixtures
    bit = int(out["bit"])
    assert len(records) == 12 and tuple(records[0]) == dd.KEYS12 and order == [f"cads/{r['uid']}.pkl" for r in records]
    keep = dd.dedup_cads(records, bit)
    assert [u for u, k in zip(order, keep) if k] == out["cad_train"].tolist()
    assert keep.tolist() == [True, False, False, True, True, True, True, True, False, True, True, True]
    # the 32-byte key decides as the reference's '_'-joined sorted hex string does
    ref_keys = [dd.reference_key([dd.item_digest(s, bit) for s in r["surf_wcs"]]) for r in records]
    assert dd.first_occurrence(ref_keys).tolist() == keep.tolist()
    for which, key in (("surface", "surf_ncs"), ("edge", "edge_ncs")):
        got, want = dd.unique_items(records, key, bit), out[f"{which}_unique"]
        assert got.shape == want.shape and got.dtype == want.dtype == np.float32 and got.tobytes() == want.tobytes()
        assert len(want) < sum(len(r[key]) for r in records)


def test_the_fixture_holds_the_cases_it_promises(fixtures):
    records, _, out = fixtures
    bit = int(out["bit"])
    d = [[dd.item_digest(s, bit) for s in r["surf_wcs"]] for r in records]
    assert d[1] == d[0] and d[2] != d[0] and sorted(d[2]) == sorted(d[0])                    # repeat; permuted repeat
    assert set(d[3]) == set(d[4]) and sorted(d[3]) != sorted(d[4]) and len(d[3]) == 3        # [a, a, b] against [a, b, b]
    s7, s8, s9 = (records[i]["surf_wcs"][0] for i in (7, 8, 9))
    step = 2.0 / (2 ** bit - 1)
    assert 0 < np.abs(s7 - s8).max() < step and 0 < np.abs(s8 - s9).max() < step and d[7] == d[8] != d[9]
    # record 11 carries the lattice neighbours: an fp64 evaluation of real2bit gives another message
    x = records[11]["surf_wcs"][0].astype(np.float64)
    q64 = np.clip((x + 1.0) * (2 ** bit - 1) / 2.0, 0, 2 ** bit - 1).astype(np.int64)
    assert (q64 != dd.real2bit(records[11]["surf_wcs"][0], bit)).any()
    shared = {dd.item_digest(s, bit) for s in records[5]["surf_ncs"]} & {dd.item_digest(s, bit) for s in records[6]["surf_ncs"]}
    assert len(shared) == 1


@pytest.mark.parametrize("n_bits", [1, 6, 8, 16])
def test_real2bit_restated_step_by_step_equals_numpy(n_bits):
    """On every lattice point 2 k / (2^n - 1) - 1 and its two fp32 neighbours, and on the values the clip defines."""
    x = np.concatenate([dd.lattice_neighbours(n_bits), np.float32([1, -1, -0.0, 0.0, 1.5, -1.5, np.inf, -np.inf, 3e38, -3e38, 1e-45])])
    assert x.dtype == np.float32 and len(x) == 3 * 2 ** n_bits + 11
    got, want = dd.real2bit(x, n_bits), dd.real2bit_numpy(x, n_bits)
    assert got.dtype == want.dtype == np.int64 and (got == want).all()
    assert got.min() == 0 and got.max() == 2 ** n_bits - 1


def test_item_digest_message_layout():
    """24 P bytes, little-endian int64, memory order; the padding cases of SHA-256 are hashlib's business here."""
    item = np.float32([[-1, 0, 1], [0.5, -0.5, 2]])
    q = dd.real2bit(item, 6)
    assert q.tolist() == [[0, 31, 63], [47, 15, 63]]
    msg = b"".join(int(v).to_bytes(8, "little") for v in q.reshape(-1))
    assert dd.item_digest(item, 6) == hashlib.sha256(msg).digest()
    assert dd.group_key([]) == hashlib.sha256(b"").digest()
    a, b = dd.item_digest(item, 6), dd.item_digest(item, 5)
    assert dd.group_key([a, a, b]) != dd.group_key([a, b, b]) and dd.group_key([a, b]) == dd.group_key([b, a])


# ---- the ABI boundary -------------------------------------------------------------------------------------------------------------

def test_exports_and_signatures():
    lib = _lib.load()
    u8p, vp = _lib.u8p, _lib.vp
    want = {"bg_points_sha256": [_lib.fp, C.c_longlong, C.c_int, C.c_int, u8p, vp],
            "bg_digest_group_keys": [u8p, vp, C.c_int, C.c_int, u8p, vp],
            "bg_first_occurrence": [u8p, C.c_longlong, vp, C.c_longlong, u8p, vp]}
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name][1] == want[name] and getattr(lib, name).restype is C.c_int
    assert lib.bg_abi_version() == 7 == _lib.ABI_VERSION                       # added entries: the ABI number stays
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "brepgen_hip.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
    for name in ("point_digests", "cad_keys", "first_occurrence", "dedup_cads", "unique_items"):
        assert getattr(bga, name) is getattr(deduplicate, name) and name in bga.__all__
    assert callable(dataset.CADStore.unique_surfaces) and callable(dataset.CADStore.unique_edges)
    assert "hash_dedup.hip" in __import__("brepgen_amd.build", fromlist=["SOURCES"]).SOURCES


def test_argument_errors_are_negative_and_explained():
    lib = _lib.load()
    fake = 0x10000                                    # aligned, never dereferenced: validation fails first

    sha = lambda x=fake, M=3, P=32, bits=6, d=fake: lib.bg_points_sha256(x, M, P, bits, d, None)   # noqa: E731
    assert sha(x=None) == _lib.BG_E_ARG and b"null" in lib.bg_last_error()
    assert sha(d=None) == _lib.BG_E_ARG and b"null" in lib.bg_last_error()
    for kw in (dict(P=0), dict(P=1025), dict(bits=0), dict(bits=17), dict(M=-1)):
        assert sha(**kw) == _lib.BG_E_SHAPE and b"n_bits" in lib.bg_last_error(), kw
    assert sha(d=fake + 4) == _lib.BG_E_ALIGN and b"aligned" in lib.bg_last_error()
    assert sha(M=0, x=None, d=None) == 0

    keys = lambda d=fake, off=fake, N=4, mg=6, key=fake: lib.bg_digest_group_keys(d, off, N, mg, key, None)   # noqa: E731
    assert keys(d=None) == _lib.BG_E_ARG and b"null" in lib.bg_last_error()
    assert keys(off=None) == _lib.BG_E_ARG and keys(key=None) == _lib.BG_E_ARG
    assert keys(mg=4097) == _lib.BG_E_SHAPE and b"4096" in lib.bg_last_error()
    assert keys(mg=-1) == _lib.BG_E_SHAPE and keys(N=-1) == _lib.BG_E_SHAPE
    assert keys(key=fake + 8) == _lib.BG_E_ALIGN
    assert keys(N=0, d=None, off=None, key=None) == 0

    first = lambda key=fake, N=5, table=fake, T=16, keep=fake: lib.bg_first_occurrence(key, N, table, T, keep, None)   # noqa: E731
    for kw in (dict(key=None), dict(table=None), dict(keep=None)):
        assert first(**kw) == _lib.BG_E_ARG and b"null" in lib.bg_last_error(), kw
    for kw in (dict(T=12), dict(T=8), dict(T=0), dict(T=-16), dict(N=1, T=1), dict(N=8, T=8)):      # no power of two; below 2 N
        assert first(**kw) == _lib.BG_E_SHAPE and b"power of two" in lib.bg_last_error(), kw
    assert first(N=-1) == _lib.BG_E_SHAPE and lib.bg_last_error()
    assert first(key=fake + 4) == _lib.BG_E_ALIGN
    assert first(N=0, key=None, table=None, keep=None, T=2) == 0


def test_table_size():
    for n in range(0, 70):
        T = deduplicate.table_size(n)
        assert T >= 2 and T >= 2 * n and T & (T - 1) == 0 and (T < 4 * n or n <= 1)
    assert deduplicate.table_size(1 << 20) == 1 << 21 and deduplicate.table_size((1 << 20) + 1) == 1 << 22


def test_no_cpu_fallback(fixtures, monkeypatch):
    records = fixtures[0]
    with pytest.raises(_lib.BrepgenHipError):
        bga.point_digests(torch.zeros(2, 32, 3))
    with pytest.raises(_lib.BrepgenHipError):
        bga.cad_keys(torch.zeros(2, 32, dtype=torch.uint8), [0, 1, 2])
    with pytest.raises(_lib.BrepgenHipError):
        bga.first_occurrence(torch.zeros(2, 32, dtype=torch.uint8))
    with pytest.raises(_lib.BrepgenHipError):
        bga.dedup_cads(records, device="cpu")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # also where the suite runs next to a GPU
    with pytest.raises(_lib.BrepgenHipError):
        bga.dedup_cads(records)
    with pytest.raises(_lib.BrepgenHipError):
        bga.unique_items(records, "edge_ncs")


def test_record_paths_follow_the_reference():
    assert deduplicate.record_path("D", "cads/x.pkl", "furniture") == os.path.join("D", "cads/x.pkl")
    assert deduplicate.record_path("D", "00123456.pkl", "abc") == os.path.join("D", "0012", "00123456.pkl")
    assert deduplicate.record_path("D", "00009999.pkl", "deepcad") == os.path.join("D", "0000", "00009999.pkl")


def test_the_product_does_not_import_the_oracle():
    src = open(deduplicate.__file__).read()
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", src, flags=re.M)
    assert "hashlib" not in src                                                # the digests come from the kernels


def test_hash_kernels_use_no_scratch():
    """One lane per item keeps 8 state words, the 16-word rolling schedule and the next slab (32 floats) in registers; a spill would
    put scratch traffic into every round.  Read from the compiler's resource report, as test_abi_cpu.py does for the GEMMs."""
    from tests.train_cpu import resource_usage
    names, scratch, spills, _ = resource_usage("hash_dedup.hip")
    assert len(names) == 5, names      # points (16-byte and 4-byte loads), group keys, claim, keep
    assert sum("points_sha256_kernel" in n for n in names) == 2
    assert all(v == 0 for v in scratch) and all(v == 0 for v in spills), list(zip(names, scratch, spills))
