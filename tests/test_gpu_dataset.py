"""Training batches on the device (brepgen_amd/dataset.py, csrc/batch.hip) against the reference's own outputs
(tests/golden/dataset_*.npz) and the numpy restatement (tests/dataset_restate.py), at the fixtures' shapes: 5 CADs with F in
{1, 2, 5, 6, 2}, max_face 6, max_edge 5.

Bounds (derived in the issue that introduced them, restated in dataset_restate.assert_output): masks, every not-augmented output and
the boxes and corners of augmented outputs are BITWISE the reference's; augmented grids differ by at most ulp32(ref) + 2^-50 max|ref|
(the reference's cos(pi/2) residues); against the restatement everything is bitwise.  Point augmentation: ulp32 + 2^-48 max|ref|
against the fp64 restatement, plus the fixture's ref_dev against the reference (whose first centring is in fp32).
"""
import os

import numpy as np
import pytest
import torch

import brepgen_amd as bga
from brepgen_amd import training
from brepgen_amd.sampling import noise_key
from tests import dataset_restate as dr
from tests.guarded import guarded, sentinel_bits

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S, E = 6, 5
KINDS = list(dr.KINDS)
DRAW_NAMES = ("u", "turns", "face_key1", "face_key2", "edge_key1", "edge_key2")


def golden(name):
    return np.load(os.path.join(GOLDEN, f"dataset_{name}.npz"))


@pytest.fixture(scope="module")
def records():
    return dr.load_records(golden("records"))


@pytest.fixture(scope="module")
def store(records):
    return bga.CADStore.from_records(records)


def host(t):
    return t.cpu().numpy()


def recorded(kind, mode):
    g = golden(kind.lower())
    draws = {k: g[f"{mode}_draw_{k}"] for k in DRAW_NAMES}
    want = [g[f"{mode}_out{i}"] for i in range(sum(k.startswith(f"{mode}_out") for k in g.files))]
    return g[f"{mode}_records"].tolist(), draws, want


# ---- (i) the four kinds from recorded draws against the reference --------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["plain", "aug"])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_from_recorded_draws_against_the_reference(store, kind, mode):
    ids, draws, want = recorded(kind, mode)
    got = store.batch(kind, ids, S, E, bbox_scaled=3, aug=mode == "aug", draws=draws)
    assert len(got) == len(want)
    for i, (t, ref) in enumerate(zip(got, want)):
        assert t.is_cuda and t.dtype == (torch.bool if ref.dtype == np.bool_ else torch.float32)
        dr.assert_output(host(t), ref, mode == "aug" and i in dr.GRID_OUTPUTS[kind], (kind, mode, i))


# ---- (ii) the same calls into guard-banded, poisoned buffers ---------------------------------------------------------------------------

OUT_SHAPES = {"surf_pos": ((S, 6), torch.float32), "surf_ncs": ((S, 32, 32, 3), torch.float32), "surf_mask": ((S,), torch.uint8),
              "edge_pos": ((S, E, 6), torch.float32), "edge_ncs": ((S, E, 32, 3), torch.float32), "edge_mask": ((S, E), torch.uint8),
              "vertex_pos": ((S, E, 6), torch.float32)}
OUT_NAMES = {"SurfPos": ("surf_pos",), "SurfZ": ("surf_pos", "surf_ncs", "surf_mask"), "EdgePos": ("edge_pos", "surf_ncs", "surf_pos", "surf_mask"),
             "EdgeZ": ("edge_ncs", "edge_pos", "edge_mask", "surf_ncs", "surf_pos", "vertex_pos")}


@pytest.mark.parametrize("mode", ["plain", "aug"])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_writes_every_element_and_nothing_else(store, kind, mode):
    ids, draws, _ = recorded(kind, mode)
    B = len(ids)
    plain = store.batch(kind, ids, S, E, aug=mode == "aug", draws=draws)
    bufs = {name: guarded((B,) + OUT_SHAPES[name][0], OUT_SHAPES[name][1], "cuda") for name in OUT_NAMES[kind]}
    got = store.batch(kind, ids, S, E, aug=mode == "aug", draws=draws, out={name: b.view for name, b in bufs.items()})
    face_src, edge_src, _, _, _ = store.plan(kind, ids, S, E, aug=mode == "aug", draws=draws)
    for name, t, ref in zip(OUT_NAMES[kind], got, plain):
        bufs[name].assert_untouched(f"{kind} {name}")
        bufs[name].assert_fully_written(f"{kind} {name}")
        assert t.shape == ref.shape and host(t).tobytes() == host(ref).tobytes(), name
        src = host(edge_src if name.startswith(("edge", "vertex")) else face_src)
        if name.endswith("mask"):
            raw = host(bufs[name].view).reshape(src.shape)
            assert set(np.unique(raw).tolist()) <= {0, 1} and (raw.astype(bool) == (src < 0)).all(), name
        else:
            bits = host(t).view(np.uint32).reshape(src.shape + (-1,))
            assert (bits[src < 0] == 0).all(), f"{name}: padding is not +0.0"
            assert int(sentinel_bits(torch.float32)[1]) not in bits[src >= 0], name


# ---- (iii) Philox mode --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_philox_batch_equals_the_restatement_and_is_batch_independent(store, records, kind):
    ids, draw_id = [3, 0, 2, 1, 2], 5
    gen = torch.Generator().manual_seed(1234)
    seed = noise_key(gen)
    got = store.batch(kind, ids, S, E, aug=True, generator=gen, draw_id=draw_id)
    draws = dr.philox_draws(ids, S, E, seed, draw_id)
    assert 0 < int((draws["u"] > 0.5).sum()) < len(ids)                         # both branches are in the batch
    want = dr.batch(records, ids, kind, S, E, 3, True, draws)
    for i, (t, ref) in enumerate(zip(got, want)):
        dr.assert_output(host(t), ref, False, (kind, i))                        # bitwise, grids included
    again = store.batch(kind, ids, S, E, aug=True, generator=torch.Generator().manual_seed(1234), draw_id=draw_id)
    other = store.batch(kind, ids, S, E, aug=True, generator=gen, draw_id=draw_id + 1)
    assert all(host(a).tobytes() == host(b).tobytes() for a, b in zip(got, again))
    assert any(host(a).tobytes() != host(b).tobytes() for a, b in zip(got, other))
    alone = store.batch(kind, [2], S, E, aug=True, generator=gen, draw_id=draw_id)
    for a, b in zip(got, alone):
        assert host(a[2]).tobytes() == host(b[0]).tobytes() == host(a[4]).tobytes()      # record 2 in [3,0,2,1,2] and in [2]


@pytest.mark.parametrize("kind", KINDS)
def test_philox_plan_holds_the_right_multisets(store, records, kind):
    ids = [0, 1, 2, 3, 4]
    face_src, edge_src, rot, scale, _ = store.plan(kind, ids, S, E, aug=True, generator=torch.Generator().manual_seed(9), draw_id=1)
    face_src, face_off, edge_off = host(face_src), host(store.face_off), host(store.edge_off)
    for b, r in enumerate(ids):
        rec = records[r]
        F, f0, e0 = len(rec["surf_bbox_wcs"]), int(face_off[r]), int(edge_off[r])
        counts = np.bincount(face_src[b][face_src[b] >= 0] - f0, minlength=F)
        if kind == "SurfPos":
            assert counts.sum() == S and set(counts.tolist()) <= {S // F, S // F + 1}
            continue
        assert (counts == 1).all() and (face_src[b, :F] >= 0).all() and (face_src[b, F:] == -1).all()
        if edge_src is None:
            continue
        rows = host(edge_src)[b]
        assert (rows[F:] == -1).all()
        for slot in range(F):
            adj = np.sort(np.asarray(rec["faceEdge_adj"][face_src[b, slot] - f0]))
            d = len(adj)
            live = rows[slot][rows[slot] >= 0] - e0
            if kind == "EdgeZ":
                assert (np.sort(live) == adj).all() and (rows[slot, :d] >= 0).all() and (rows[slot, d:] == -1).all()
            else:
                vals, cnt = np.unique(live, return_counts=True)
                assert (vals == adj).all() and cnt.sum() == E and set(cnt.tolist()) <= {E // d, E // d + 1}
    want = np.stack([[np.abs(records[r][k]).max() for k in ("surf_bbox_wcs", "edge_bbox_wcs", "corner_wcs")] for r in ids])
    assert (host(scale) == want.astype(np.float64)).all()
    assert all(c == 0 or all(1 <= (c >> s) & 3 <= 3 for s in (0, 2, 4)) for c in host(rot).tolist())


# ---- (iv) the draws' distribution -----------------------------------------------------------------------------------------------------------

def test_augment_decision_is_a_fair_coin_and_all_27_turn_triples_occur():
    """4096 one-face records, aug=True: the augmented share within 0.5 +- 0.047 (6 sigma of a fair coin, sigma = 0.0078)."""
    n = 4096
    one = {"surf_ncs": np.zeros((1, 32, 32, 3), np.float32), "edge_ncs": np.zeros((1, 32, 3), np.float32),
           "corner_wcs": np.ones((1, 2, 3), np.float32), "faceEdge_adj": [np.array([0])],
           "surf_bbox_wcs": np.ones((1, 6), np.float32), "edge_bbox_wcs": np.ones((1, 6), np.float32)}
    big = bga.CADStore.from_records([one] * n)
    _, _, rot, _, _ = big.plan("SurfPos", np.arange(n), S, E, aug=True, generator=torch.Generator().manual_seed(77))
    rot = host(rot)
    share = float((rot != 0).mean())
    assert abs(share - 0.5) <= 0.047, share
    assert len(set(rot[rot != 0].tolist())) == 27
    _, _, off, _, _ = big.plan("SurfPos", np.arange(n), S, E, aug=False, generator=torch.Generator().manual_seed(77))
    assert not host(off).any()


# ---- (v) the admission filter -----------------------------------------------------------------------------------------------------------------

def test_keep_mask_against_filter_data():
    g = golden("filter")
    fstore = bga.CADStore.from_records(dr.load_records(g))
    keep = fstore.keep_mask(S, E, bbox_scaled=3, threshold=0.05)
    assert keep.dtype == torch.bool and host(keep).tolist() == g["keep"].tolist(), list(zip(g["notes"].tolist(), host(keep).tolist()))
    buf = guarded((len(fstore),), torch.uint8, "cuda")
    from brepgen_amd import _lib
    import ctypes as C
    _lib.check(_lib.load().bg_cad_filter(C.byref(fstore._c), S, E, 3.0, 0.05, _lib.ptr(buf.view), _lib.stream()), "bg_cad_filter")
    buf.assert_untouched("keep")
    assert host(buf.view).reshape(-1).tolist() == [int(k) for k in g["keep"]]


# ---- (vi) point augmentation ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["edge", "surf"])           # P = 32, P = 1024
def test_augment_points_against_the_restatement_and_the_reference(name):
    g = golden("points")
    x, u, turns, ref = g[f"{name}_x"], g[f"{name}_u"], g[f"{name}_turns"], g[f"{name}_out"]
    M = len(x)
    buf = guarded((M, x[0].size), torch.float32, "cuda")
    got = host(bga.augment_points(torch.from_numpy(x).cuda(), aug=True, draws={"u": u, "turns": turns}, out=buf.view)).reshape(x.shape)
    buf.assert_untouched(name)
    buf.assert_fully_written(name)
    r64 = dr.augment_points(x.reshape(M, -1, 3), u, turns, True, "fp64").reshape(x.shape)
    ref_dev = float(g[f"{name}_ref_dev"])
    for m in range(M):
        if u[m] <= 0.5:
            assert got[m].tobytes() == x[m].tobytes()
            continue
        d = np.abs(got[m].astype(np.float64) - r64[m])
        bound = dr.ulp32(r64[m]) + 2.0 ** -48 * float(np.abs(r64[m]).max())
        print(f"{name} item {m}: max excess over ulp32 vs the fp64 restatement {float((d - dr.ulp32(r64[m])).max()):.3e}")
        assert (d <= bound).all(), (m, float(d.max()))
        top = float(np.abs(ref[m]).max())
        d = np.abs(got[m].astype(np.float64) - ref[m])
        assert (d <= dr.ulp32(ref[m]) + (2.0 ** -48 + ref_dev) * top).all(), (m, float(d.max()), ref_dev)
    off = host(bga.augment_points(torch.from_numpy(x).cuda(), aug=False, draws={"u": u, "turns": turns}))
    assert off.tobytes() == x.tobytes()


def test_augment_points_philox_is_reproducible_and_item_keyed():
    x = torch.from_numpy(golden("points")["edge_x"]).cuda()
    gen = torch.Generator().manual_seed(5)
    seed = noise_key(gen)
    a = bga.augment_points(x, generator=gen, draw_id=2, first_item=10)
    draws = dr.philox_point_draws(len(x), seed, 2, 10)
    b = bga.augment_points(x, draws=draws)
    tail = bga.augment_points(x[3:], generator=gen, draw_id=2, first_item=13)
    assert host(a).tobytes() == host(b).tobytes() and host(a[3:]).tobytes() == host(tail).tobytes()


# ---- (vii) into the training forward ----------------------------------------------------------------------------------------------------------------

def test_surfz_batch_feeds_ldm_loss(store, records):
    from oracle import vae as ov
    from tests import parity_cases as pc
    net, _ = pc.build_net("SurfZNet", 41, False, torch.float32)
    enc = bga.AutoencoderKLFastEncode(**pc.SURF_CFG)
    enc.load_state_dict(ov.seeded_state_dict(ov.surf_encoder_spec(), 51), strict=True)
    enc = enc.cuda().eval()
    ddpm = bga.DDPMScheduler(num_train_timesteps=1000, beta_schedule="linear", prediction_type="epsilon", beta_start=0.0001,
                             beta_end=0.02, clip_sample=False)
    ids, gen = [2, 1], torch.Generator().manual_seed(7)          # record 2 is augmented, record 1 is not
    seed = noise_key(gen)
    noise = torch.randn(2, S, 48, generator=torch.Generator().manual_seed(4)).cuda()
    t = torch.tensor([99, 499]).cuda()

    def loss(surf_pos, surf_ncs, surf_mask):
        z = training.surface_tokens(enc, surf_ncs)
        return float(training.ldm_loss(net, ddpm, z, t, noise, (surf_pos,), surf_mask)["mean"])

    on_device = loss(*store.batch("SurfZ", ids, S, E, aug=True, generator=gen))
    on_host = loss(*(torch.from_numpy(a).cuda() for a in dr.batch(records, ids, "SurfZ", S, E, 3, True, dr.philox_draws(ids, S, E, seed, 0))))
    assert np.isfinite(on_device) and on_device == on_host, (on_device, on_host)
