"""Numpy restatement of the device-side batch assembly (csrc/batch.hip, brepgen_amd/dataset.py).  TEST INFRASTRUCTURE, written from
include/brepgen_hip.h: keys -> slot maps (``plan``), the gather (``gather`` / ``batch``), the admission filter (``keep``), the point
augmentation (``augment_points``) and the Philox draws (``philox_draws`` / ``philox_point_draws``, through oracle/philox.py).

A record is a dict with the reference's keys: surf_ncs [F,32,32,3], edge_ncs [Ne,32,3], corner_wcs [Ne,2,3], faceEdge_adj (a list of F
integer arrays, edge ids local to the record), surf_bbox_wcs [F,6], edge_bbox_wcs [Ne,6]; all fp32.
"""
import numpy as np

from oracle import philox

KINDS = {"SurfPos": 0, "SurfZ": 1, "EdgePos": 2, "EdgeZ": 3}
TAG, TAG_POINTS, CAD_ELEM = 0xDA7A0000, 0xDA7B0000, 0xFFFFFFFF
f32, f64 = np.float32, np.float64


# ---- rotation: the signed coordinate permutation ------------------------------------------------------------------------------------

def _quarter(a, b, q):
    if q == 1:
        return -b, a
    if q == 2:
        return -a, -b
    if q == 3:
        return b, -a
    return a, b


def rot3(p, code):
    """p [..., 3] (any float dtype), code = qx | qy << 2 | qz << 4: x, then y, then z; a negated zero becomes +0.0."""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    y, z = _quarter(y, z, code & 3)
    z, x = _quarter(z, x, (code >> 2) & 3)
    x, y = _quarter(x, y, (code >> 4) & 3)
    return np.stack([x, y, z], -1) + p.dtype.type(0)


def rot_code(turns):
    return int(turns[0]) | (int(turns[1]) << 2) | (int(turns[2]) << 4)


# ---- plan ---------------------------------------------------------------------------------------------------------------------------

def pad_repeat_src(n, L):
    r = L // n
    sep = L - r * n
    i = np.arange(L)
    return np.where(i < sep * (r + 1), i // (r + 1), sep + (i - sep * (r + 1)) // max(r, 1))


def _argsort(keys):
    return np.argsort(np.asarray(keys, dtype=np.uint32), kind="stable")


def plan(rec, kind, S, E, draws, aug):
    """Slot maps of one CAD: face_src [S] (LOCAL face, -1 padding), edge_src [S, E] (LOCAL edge, -1; None for the face kinds), rot code.
    draws: dict u, turns [3], face_key1 / face_key2 [S], edge_key1 / edge_key2 [S, E] (missing = zeros)."""
    F = len(rec["surf_bbox_wcs"])
    zeros_s, zeros_se = np.zeros(S, np.uint32), np.zeros((S, E), np.uint32)
    fk1, fk2 = draws.get("face_key1", zeros_s), draws.get("face_key2", zeros_s)
    ek1, ek2 = draws.get("edge_key1", zeros_se), draws.get("edge_key2", zeros_se)
    code = rot_code(draws.get("turns", (1, 1, 1))) if (aug and float(draws.get("u", 0.0)) > 0.5) else 0
    order = _argsort(fk1[:F])
    face_src = np.full(S, -1, np.int64)
    if kind == "SurfPos":
        padded = order[pad_repeat_src(F, S)]
        return padded[_argsort(fk2[:S])], None, code
    face_src[:F] = order
    if kind == "SurfZ":
        return face_src, None, code
    rows = np.full((F, E), -1, np.int64)                 # by ORIGINAL face
    for f, adj in enumerate(rec["faceEdge_adj"]):
        adj = np.asarray(adj, dtype=np.int64)
        d = len(adj)
        shuffled = adj[_argsort(ek1[f, :d])]
        if kind == "EdgePos":
            rows[f] = shuffled[pad_repeat_src(d, E)][_argsort(ek2[f, :E])]
        else:
            rows[f, :d] = shuffled
    edge_src = np.full((S, E), -1, np.int64)
    edge_src[:F] = rows[order]
    return face_src, edge_src, code


# ---- gather -------------------------------------------------------------------------------------------------------------------------

def _scale(a):
    return f64(np.max(np.abs(np.asarray(a, dtype=f32)))) if np.size(a) else f64(0.0)


def _boxes(pos, code, bs):
    pos = np.asarray(pos, dtype=f32)
    if not code:
        return pos * f32(bs)
    s = _scale(pos)
    p = rot3(pos[:, :3].astype(f64), code) / s
    q = rot3(pos[:, 3:].astype(f64), code) / s
    return np.concatenate([np.minimum(p, q) * f64(f32(bs)), np.maximum(p, q) * f64(f32(bs))], -1).astype(f32)


def _corners(corner, code, bs):
    corner = np.asarray(corner, dtype=f32).reshape(-1, 2, 3)
    if not code:
        c = corner * f32(bs)
    else:
        c = rot3(corner.astype(f64), code) / _scale(corner) * f64(f32(bs))
    out = np.empty_like(c)
    for e, pair in enumerate(c):
        out[e] = pair[np.lexsort((pair[:, 2], pair[:, 1], pair[:, 0]))]
    return out.reshape(-1, 6).astype(f32)


def _grids(g, code):
    g = np.asarray(g, dtype=f32)
    return rot3(g, code) if code else g


def _take(rows, src):
    """rows [n, ...] gathered by src [...] with -1 -> +0.0."""
    out = np.zeros(src.shape + rows.shape[1:], dtype=rows.dtype)
    live = src >= 0
    out[live] = rows[src[live]]
    return out


def gather(rec, kind, face_src, edge_src, code, bbox_scaled=3):
    """The tensors of one CAD in the reference's return order (masks as bool)."""
    surf_pos = _take(_boxes(rec["surf_bbox_wcs"], code, bbox_scaled), face_src)
    if kind == "SurfPos":
        return (surf_pos,)
    surf_ncs = _take(_grids(rec["surf_ncs"], code), face_src)
    surf_mask = face_src < 0
    if kind == "SurfZ":
        return surf_pos, surf_ncs, surf_mask
    edge_pos = _take(_boxes(rec["edge_bbox_wcs"], code, bbox_scaled), edge_src)
    if kind == "EdgePos":
        return edge_pos, surf_ncs, surf_pos, surf_mask
    edge_ncs = _take(_grids(rec["edge_ncs"], code), edge_src)
    vertex_pos = _take(_corners(rec["corner_wcs"], code, bbox_scaled), edge_src)
    return edge_ncs, edge_pos, edge_src < 0, surf_ncs, surf_pos, vertex_pos


def cad_draws(draws, b):
    """Row b of stacked draws (dict of arrays with a leading batch axis) as one CAD's dict."""
    return {k: np.asarray(v)[b] for k, v in draws.items() if v is not None}


def batch(records, indices, kind, S, E, bbox_scaled=3, aug=False, draws=None):
    """What ``CADStore.batch`` returns (without class labels), stacked over the batch; draws: stacked arrays (see ``philox_draws``)."""
    outs = []
    for b, r in enumerate(indices):
        face_src, edge_src, code = plan(records[r], kind, S, E, cad_draws(draws or {}, b), aug)
        outs.append(gather(records[r], kind, face_src, edge_src, code, bbox_scaled))
    return tuple(np.stack(col) for col in zip(*outs))


# ---- Philox draws -------------------------------------------------------------------------------------------------------------------

def _key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def _u01(w):
    return ((w >> np.uint32(9)).astype(f32) + f32(0.5)) * f32(1.0 / 8388608.0)


def _turns(w):
    return 1 + ((w.astype(np.uint64) * np.uint64(3)) >> np.uint64(32)).astype(np.int32)


def philox_draws(record_numbers, S, E, seed, draw_id):
    """The device's own draws of a batch as stacked arrays: u [B], turns [B, 3], face_key1 / 2 [B, S], edge_key1 / 2 [B, S, E]."""
    recs = np.asarray(record_numbers, dtype=np.uint32)
    B = len(recs)
    c = np.zeros((B, 4), np.uint32)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = CAD_ELEM, recs, draw_id, TAG
    w = philox.philox4x32_10(c, _key(seed))
    c = np.zeros((B, S, 4), np.uint32)
    c[..., 0], c[..., 1], c[..., 2], c[..., 3] = np.arange(S)[None], recs[:, None], draw_id, TAG
    wf = philox.philox4x32_10(c, _key(seed))
    c = np.zeros((B, S, E, 4), np.uint32)
    c[..., 0], c[..., 1], c[..., 2] = np.arange(E)[None, None], recs[:, None, None], draw_id
    c[..., 3] = (TAG | (np.arange(S) + 1))[None, :, None]
    we = philox.philox4x32_10(c, _key(seed))
    return {"u": _u01(w[:, 0]).astype(f64), "turns": _turns(w[:, 1:4]), "face_key1": wf[..., 0], "face_key2": wf[..., 1],
            "edge_key1": we[..., 0], "edge_key2": we[..., 1]}


def philox_point_draws(M, seed, draw_id, first_item=0):
    g = first_item + np.arange(M, dtype=np.uint64)
    c = np.zeros((M, 4), np.uint32)
    c[:, 1], c[:, 2] = (g & np.uint64(0xFFFFFFFF)).astype(np.uint32), draw_id
    c[:, 3] = (np.uint64(TAG_POINTS) | ((g >> np.uint64(32)) & np.uint64(0xFFFF))).astype(np.uint32)
    w = philox.philox4x32_10(c, _key(seed))
    return {"u": _u01(w[:, 0]).astype(f64), "turns": _turns(w[:, 1:4])}


def keys_of(perm, size):
    """Keys that replay the recorded permutation p (out[i] = in[p[i]]): key[p[i]] = i, zero beyond."""
    key = np.zeros(size, np.uint32)
    key[np.asarray(perm, dtype=np.int64)] = np.arange(len(perm), dtype=np.uint32)
    return key


# ---- admission filter ---------------------------------------------------------------------------------------------------------------

def _any_same(boxes, scale, thr):
    b = np.asarray(boxes, dtype=f32) * f32(scale)
    d = np.abs(b[:, None, :] - b[None, :, :]).max(-1)
    return bool((d[np.triu_indices(len(b), 1)] < f32(thr)).any())


def keep(rec, max_face, max_edge, scale=3, threshold=0.05):
    if len(rec["surf_bbox_wcs"]) > max_face:
        return False
    if any(len(a) > max_edge or len(a) == 0 for a in rec["faceEdge_adj"]):
        return False
    if _any_same(rec["surf_bbox_wcs"], scale, threshold):
        return False
    edge_pos = np.asarray(rec["edge_bbox_wcs"], dtype=f32)
    return not any(_any_same(edge_pos[np.asarray(a, dtype=np.int64)], scale, threshold) for a in rec["faceEdge_adj"])


# ---- point augmentation -------------------------------------------------------------------------------------------------------------

def augment_points(x, u, turns, aug=True, first_centre="fp64"):
    """x [M, P, 3] fp32 -> fp32.  first_centre="fp32": the first mean and subtraction in fp32, as numpy does for the reference's fp32
    input (np.mean with an fp32 accumulator); "fp64": everything in fp64, as the device computes."""
    x = np.asarray(x, dtype=f32)
    out = x.copy()
    for m in range(len(x)):
        if not (aug and float(u[m]) > 0.5):
            continue
        p = x[m] if first_centre == "fp32" else x[m].astype(f64)
        for axis in range(3):
            centre = np.mean(p, axis=0)
            c = (p - centre).astype(f64)
            c = rot3(c, int(turns[m][axis]) << (2 * axis))
            p = c + centre.astype(f64)
            p = p / np.max(np.abs(p))
        out[m] = p.astype(f32)
    return out


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=f32))).astype(f64)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------

def load_records(npz, prefix="r"):
    """The records of a tests/golden/dataset_*.npz archive (gen_dataset_golden.py: pack_records) as a list of dicts."""
    out = []
    for r in range(int(npz[prefix + "count"])):
        rec = {k: npz[f"{prefix}{r}_{k}"] for k in ("surf_ncs", "edge_ncs", "corner_wcs", "surf_bbox_wcs", "edge_bbox_wcs")}
        off, idx = npz[f"{prefix}{r}_adj_off"], npz[f"{prefix}{r}_adj_idx"]
        rec["faceEdge_adj"] = [idx[off[f]:off[f + 1]] for f in range(len(off) - 1)]
        out.append(rec)
    return out


# outputs that hold point grids, by kind (positions in the reference's return order): bounded, not bitwise, when augmented
GRID_OUTPUTS = {"SurfPos": (), "SurfZ": (1,), "EdgePos": (1,), "EdgeZ": (0, 3)}


def assert_output(got, ref, grid_bound, what):
    """Bitwise equality, or -- for an augmented grid -- |d| <= ulp32(ref) + 2^-50 max|ref| (the reference's 90-degree matrices carry
    cos(pi/2), sin(pi), cos(3 pi/2) <= 1.84e-16 each: three rotations leave <= 5.5e-16 < 2^-50 of the largest coordinate where the
    exact rotation gives the coordinate itself, or 0)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if grid_bound:
        d = np.abs(got.astype(f64) - ref.astype(f64))
        bound = ulp32(ref) + 2.0 ** -50 * float(np.abs(ref).max())
        assert (d <= bound).all(), (what, float((d - bound).max()))
    elif ref.dtype == np.bool_:
        assert (got == ref).all(), what
    else:
        diff = got.view(np.uint32) != ref.view(np.uint32)
        assert not diff.any(), (what, int(diff.sum()))
