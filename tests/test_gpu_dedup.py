"""Training-set de-duplication on the device (brepgen_amd/deduplicate.py, csrc/hash_dedup.hip) against hashlib, the numpy restatement
(tests/dedup_restate.py) and the reference's scripts' own outputs (tests/golden/dedup_*.npz).  Every comparison is exact: digests byte
for byte, masks and index lists element for element.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import brepgen_amd as bga
from brepgen_amd import deduplicate
from tests import dedup_restate as dd
from tests.guarded import guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SPECIALS = np.float32([1.0, -1.0, -0.0, 0.0, 1.5, -1.5, np.inf, -np.inf])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def values(g, shape, bit):
    """Lattice neighbours of `bit` bits, the values the clip defines and uniform noise, mixed."""
    n = int(np.prod(shape))
    pool = np.concatenate([dd.lattice_neighbours(bit), SPECIALS])
    x = np.where(g.random(n) < 0.5, pool[g.integers(0, len(pool), n)], g.uniform(-1.1, 1.1, n).astype(np.float32))
    x[:len(SPECIALS)] = SPECIALS[:n]
    return x.astype(np.float32).reshape(shape)


# ---- (i) quantise + SHA-256 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bit", [1, 6, 8, 16])
@pytest.mark.parametrize("P", [1, 2, 3, 5, 8, 32, 1024])
def test_point_digests_against_hashlib(P, bit):
    """P: one block (1, 2), a block boundary (3), residue 56 where the length needs a block of its own (5), residue 0 where the padding
    is a block of its own (8, 32, 1024); M around the 64 items of a wave."""
    g = np.random.default_rng(1000 * P + bit)
    sizes = (3, 65) if P == 1024 else (1, 63, 64, 65, 130)
    x = values(g, (max(sizes), P, 3), bit)
    want = dd.digests(x, bit)
    xd = dev(x)
    for M in sizes:
        got = host(bga.point_digests(xd[:M], bit))
        assert got.shape == (M, 32) and got.dtype == np.uint8
        bad = np.nonzero((got != want[:M]).any(axis=1))[0]
        assert bad.size == 0, (P, bit, M, bad[:8].tolist(), bytes(got[bad[0]]).hex(), bytes(want[bad[0]]).hex())


@pytest.mark.parametrize("bit", [1, 6, 8, 16])
def test_every_lattice_neighbour_quantises_as_numpy_does(bit):
    """All 3 * 2^bit lattice points and fp32 neighbours, three per item: a digest differs iff a value quantises differently."""
    x = dd.lattice_neighbours(bit).reshape(3, -1).T.copy()                   # [2^bit, 3]: (below, on, above) of lattice point k
    assert (dd.real2bit(x, bit) == dd.real2bit_numpy(x, bit)).all()
    got = host(bga.point_digests(dev(x.reshape(-1, 1, 3)), bit))
    assert (got == dd.digests(x.reshape(-1, 1, 3), bit)).all()


def test_point_digests_shapes_and_layouts():
    g = np.random.default_rng(7)
    x = values(g, (70, 32, 32, 3), 6)
    want = dd.digests(x, 6)
    xd = dev(x)
    assert (host(bga.point_digests(xd, 6)) == want).all()                     # [M, 32, 32, 3] as it sits in a record
    assert (host(bga.point_digests(xd[1:], 6)) == want[1:]).all()             # an offset view
    e = values(g, (67, 32, 3), 6)
    assert (host(bga.point_digests(dev(e))) == dd.digests(e, 6)).all()        # bit defaults to the reference's 6
    odd = values(g, (66, 7, 3), 6)
    assert (host(bga.point_digests(dev(odd)[1:], 6)) == dd.digests(odd[1:], 6)).all()      # items that are not 16-byte aligned
    assert bga.point_digests(xd[:0], 6).shape == (0, 32)
    assert bytes(host(bga.point_digests(xd[:1], 6))[0]).hex() == __import__("hashlib").sha256(
        dd.real2bit(x[0], 6).reshape(-1, 3).tobytes()).hexdigest()
    with pytest.raises(ValueError):
        bga.point_digests(dev(np.zeros((2, 1025, 3), np.float32)), 6)
    with pytest.raises(ValueError):
        bga.point_digests(xd, 17)


@pytest.mark.parametrize("M,P", [(65, 32), (3, 1024), (130, 5)])
def test_point_digests_write_exactly_their_output(M, P):
    g = np.random.default_rng(M + P)
    x = values(g, (M, P, 3), 6)
    out = guarded((M, 32), torch.uint8, "cuda")
    bga.point_digests(dev(x), 6, out=out.view)
    out.assert_untouched(f"digest M={M} P={P}")
    assert (host(out.view) == dd.digests(x, 6)).all()


# ---- (ii) the key of a group -------------------------------------------------------------------------------------------------------------

def random_digests(g, n):
    return g.integers(0, 256, (n, 32), dtype=np.uint8)


def test_cad_keys_against_the_restatement():
    g = np.random.default_rng(11)
    sizes = [0, 1, 2, 3, 70, 257, 0, 5, 64, 65]
    d = random_digests(g, sum(sizes))
    off = np.concatenate([[0], np.cumsum(sizes)])
    d[off[4] + 10] = d[off[4] + 40]                                           # the same face twice inside a group
    d[off[5]:off[5] + 100, :8] = d[off[5], :8]                                # 100 digests that agree in their first 8 bytes ...
    d[off[5] + 100:off[5] + 120, :31] = d[off[5] + 100, :31]                  # ... and 20 that differ in the last byte only
    d[off[5] + 110] = d[off[5] + 105]
    got = host(bga.cad_keys(dev(d), off))
    want = dd.group_keys(d, off)
    assert got.shape == (len(sizes), 32) and (got == want).all(), np.nonzero((got != want).any(axis=1))[0]
    assert bytes(got[0]) == __import__("hashlib").sha256(b"").digest() == bytes(got[6])
    # offsets on the device, the largest group from the host
    again = host(bga.cad_keys(dev(d), dev(off.astype(np.int32)), max_group=257))
    assert (again == want).all()
    with pytest.raises(ValueError):
        bga.cad_keys(dev(d), dev(off.astype(np.int32)))
    with pytest.raises(ValueError):
        bga.cad_keys(dev(d), [0, len(d) + 1])


def test_cad_keys_are_order_free_and_count_repeats():
    g = np.random.default_rng(12)
    a, b = random_digests(g, 2)
    base = random_digests(g, 70)
    groups = [base, base[g.permutation(70)], base[::-1], [a, a, b], [a, b, b], [b, a, a], [a, b], [b, a], [a], [a, a]]
    d = np.concatenate([np.asarray(x, dtype=np.uint8).reshape(-1, 32) for x in groups])
    off = np.concatenate([[0], np.cumsum([len(x) for x in groups])])
    k = host(bga.cad_keys(dev(d), off))
    assert (k == dd.group_keys(d, off)).all()
    assert (k[0] == k[1]).all() and (k[0] == k[2]).all()                      # permuted groups
    assert (k[3] != k[4]).any() and (k[3] == k[5]).all()                      # [a, a, b] is not [a, b, b]
    assert (k[6] == k[7]).all() and (k[8] != k[9]).any()


def test_cad_keys_write_exactly_their_output():
    g = np.random.default_rng(13)
    d = random_digests(g, 40)
    off = np.arange(0, 44, 4)
    out = guarded((10, 32), torch.uint8, "cuda")
    bga.cad_keys(dev(d), off, out=out.view)
    out.assert_untouched("keys")
    assert (host(out.view) == dd.group_keys(d, off)).all()


# ---- (iii) first occurrence --------------------------------------------------------------------------------------------------------------

def check_first(keys):
    kd = dev(keys)
    a, b = host(bga.first_occurrence(kd)), host(bga.first_occurrence(kd))
    want = dd.first_occurrence(list(keys))
    assert a.dtype == np.bool_ and a.tolist() == want.tolist(), np.nonzero(a != want)[0][:8]
    assert (a == b).all()                                                     # the probe order may vary, the mask may not
    return a


@pytest.mark.parametrize("N", [1, 2, 64, 65, 1000])
def test_first_occurrence(N):
    g = np.random.default_rng(N)
    pool = random_digests(g, max(1, N // 3))
    mixed = pool[g.integers(0, len(pool), N)]
    assert check_first(mixed).sum() == len({k.tobytes() for k in mixed})
    assert check_first(np.repeat(pool[:1], N, axis=0)).tolist() == [True] + [False] * (N - 1)       # all equal
    assert check_first(random_digests(g, N)).all()                                                # all distinct
    # distinct keys that share their first 8 bytes: one home slot, every one probes past the others (with repeats mixed in)
    same_home = random_digests(g, N)
    same_home[:, :8] = same_home[0, :8]
    check_first(same_home)
    check_first(same_home[g.integers(0, N, N)])
    # a run that wraps round the end of the table: home slots T - 2 and T - 1 (header: first 8 bytes, little-endian, masked to T - 1)
    T = deduplicate.table_size(N)
    wrap = random_digests(g, N)
    wrap[:, :8] = np.frombuffer(np.uint64(T - 2).tobytes(), np.uint8)
    wrap[1::2, 0] += 1
    wrap[:, 4:8] = g.integers(0, 256, (N, 4), dtype=np.uint8)                  # bits above the mask do not matter
    assert check_first(wrap).all()
    check_first(wrap[g.integers(0, N, N)])


def test_first_occurrence_of_nothing():
    assert bga.first_occurrence(torch.empty(0, 32, dtype=torch.uint8, device="cuda")).shape == (0,)


# ---- (iv) end to end on the reference's scripts' outputs -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixtures():
    rec = np.load(os.path.join(GOLDEN, "dedup_records.npz"))
    return dd.load_records(rec), rec["order"].tolist(), np.load(os.path.join(GOLDEN, "dedup_outputs.npz"))


@pytest.mark.parametrize("chunk", [1, 5, 1000])
def test_dedup_cads_keeps_what_the_reference_keeps(fixtures, chunk):
    records, order, out = fixtures
    keep = bga.dedup_cads(records, bit=int(out["bit"]), chunk=chunk)
    assert isinstance(keep, np.ndarray) and keep.dtype == np.bool_ and keep.shape == (len(records),)
    assert [u for u, k in zip(order, keep) if k] == out["cad_train"].tolist()


@pytest.mark.parametrize("chunk", [1, 5, 1000])
@pytest.mark.parametrize("which", ["surf_ncs", "edge_ncs"])
def test_unique_items_are_the_reference_unique_data(fixtures, which, chunk):
    records, _, out = fixtures
    want = out["surface_unique" if which == "surf_ncs" else "edge_unique"]
    got = bga.unique_items(records, which, bit=int(out["bit"]), chunk=chunk)
    assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes()


def test_records_without_faces_are_duplicates_of_the_first_such(fixtures):
    records = fixtures[0]
    empty = dict(records[0], surf_wcs=np.zeros((0, 32, 32, 3), np.float32), surf_ncs=np.zeros((0, 32, 32, 3), np.float32))
    recs = [empty, records[0], empty, records[3], empty]
    assert bga.dedup_cads(recs, chunk=2).tolist() == dd.dedup_cads(recs, 6).tolist() == [True, True, False, True, False]
    assert bga.unique_items([empty, empty], "surf_ncs").shape == (0, 32, 32, 3)
    got = bga.unique_items(recs, "surf_ncs", chunk=1)
    assert got.tobytes() == dd.unique_items(recs, "surf_ncs", 6).tobytes()


def test_store_methods(fixtures):
    records, _, out = fixtures
    full = []
    for r in records:
        F, E = len(r["surf_ncs"]), len(r["edge_ncs"])
        full.append({"surf_ncs": r["surf_ncs"], "edge_ncs": r["edge_ncs"], "corner_wcs": np.zeros((E, 2, 3), np.float32),
                     "surf_bbox_wcs": np.zeros((F, 6), np.float32), "edge_bbox_wcs": np.zeros((E, 6), np.float32),
                     "faceEdge_adj": [np.zeros(1, np.int64)] * F})
    store = bga.CADStore.from_records(full)
    for rows, key, name in ((store.unique_surfaces(), "surf_ncs", "surface_unique"), (store.unique_edges(bit=6), "edge_ncs", "edge_unique")):
        items = np.concatenate([r[key] for r in records])
        assert rows.is_cuda and rows.dtype == torch.int64
        rows = host(rows)
        assert rows.tolist() == np.nonzero(dd.first_occurrence(list(dd.digests(items, 6))))[0].tolist()      # ascending, no pad row
        assert items[rows].tobytes() == out[name].tobytes()
    assert len(store.surf_ncs) == sum(len(r["surf_ncs"]) for r in records) + 1          # the pad row is still there


def run_cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "brepgen_amd.deduplicate"] + args, cwd=cwd, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_command_line_cad(fixtures, tmp_path):
    """`cad` on a folder of the golden records, option furniture: the reference's pickle, under its default name."""
    records, order, out = fixtures
    os.makedirs(tmp_path / "data" / "cads")
    for rec in records:
        with open(tmp_path / "data" / "cads" / (rec["uid"] + ".pkl"), "wb") as f:
            pickle.dump(rec, f)
    split = {"train": order, "val": out["cad_val"].tolist(), "test": out["cad_test"].tolist()}
    with open(tmp_path / "split.pkl", "wb") as f:
        pickle.dump(split, f)
    run_cli(["cad", "--data", str(tmp_path / "data"), "--split", str(tmp_path / "split.pkl"), "--bit", "6", "--option", "furniture",
             "--chunk", "5"], str(tmp_path))
    with open(tmp_path / "furniture_data_split_6bit.pkl", "rb") as f:
        got = pickle.load(f)
    assert got == {"train": out["cad_train"].tolist(), "val": split["val"], "test": split["test"]}


@pytest.mark.parametrize("edge", [False, True])
def test_command_line_surfedge(fixtures, tmp_path, edge):
    """`surfedge` with option abc: records under DIR/<uid // 10000, four digits>/uid, the output beside the list."""
    records, _, out = fixtures
    uids = [f"{20000 * r + 7:08d}.pkl" for r in range(len(records))]
    for uid, rec in zip(uids, records):
        folder = tmp_path / "data" / f"{int(uid[:8]) // 10000:04d}"
        os.makedirs(folder, exist_ok=True)
        with open(folder / uid, "wb") as f:
            pickle.dump(rec, f)
    with open(tmp_path / "train.pkl", "wb") as f:
        pickle.dump({"train": uids, "val": [], "test": []}, f)
    run_cli(["surfedge", "--data", str(tmp_path / "data"), "--list", str(tmp_path / "train.pkl"), "--bit", "6", "--option", "abc"] +
            (["--edge"] if edge else []), str(tmp_path))
    with open(tmp_path / ("train_edge.pkl" if edge else "train_surface.pkl"), "rb") as f:
        got = pickle.load(f)
    want = out["edge_unique" if edge else "surface_unique"]
    assert isinstance(got, list) and len(got) == len(want)
    assert all(a.dtype == np.float32 and a.shape == w.shape and a.tobytes() == w.tobytes() for a, w in zip(got, want))
