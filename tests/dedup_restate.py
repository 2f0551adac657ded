"""The contract of the reference's ``data_process/deduplicate_cad.py`` / ``deduplicate_surfedge.py`` in numpy + hashlib: what
brepgen_amd/deduplicate.py (csrc/hash_dedup.hip) has to reproduce byte for byte.  tests/golden/gen_dedup_golden.py checks this file
against the scripts themselves before it writes tests/golden/dedup_*.npz.
"""
import hashlib

import numpy as np

KEYS12 = ("surf_wcs", "edge_wcs", "surf_ncs", "edge_ncs", "corner_wcs", "edgeFace_adj", "edgeCorner_adj", "faceEdge_adj",
          "surf_bbox_wcs", "edge_bbox_wcs", "corner_unique", "uid")          # process_brep.py's record, in ITS order
GRID_KEYS = ("surf_wcs", "edge_wcs", "surf_ncs", "edge_ncs")


def real2bit(x, n_bits):
    """convert_utils.real2bit on float32 data, one fp32 rounding per step: (x + 1) * (2^n - 1) / 2, clip, truncate to int64."""
    x = np.asarray(x, dtype=np.float32)
    r = np.float32(2 ** n_bits - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x + np.float32(1.0)).astype(np.float32)
        t = (t * r).astype(np.float32)
        t = (t / np.float32(2.0)).astype(np.float32)
        t = np.minimum(np.maximum(t, np.float32(0.0)), r)
        return t.astype(np.int64)


def real2bit_numpy(data, n_bits=8, min_range=-1, max_range=1):
    """The reference's expression, typed as it stands there (Python scalars beside a float32 array)."""
    range_quantize = 2 ** n_bits - 1
    with np.errstate(invalid="ignore", over="ignore"):
        data_quantize = (data - min_range) * range_quantize / (max_range - min_range)
        data_quantize = np.clip(data_quantize, a_min=0, a_max=range_quantize)
        return data_quantize.astype(int)


def item_digest(item, n_bits):
    """sha256 of one item's quantised points: 24 P message bytes (little-endian int64, memory order)."""
    return hashlib.sha256(real2bit(item, n_bits).reshape(-1, 3).astype("<i8").tobytes()).digest()


def digests(items, n_bits):
    """uint8 [M, 32] for items [M, ..., 3] (quantised in one piece: the same values as item by item)."""
    q = real2bit(items, n_bits).astype("<i8").reshape(len(items), -1)
    return np.array([np.frombuffer(hashlib.sha256(row.tobytes()).digest(), np.uint8) for row in q], dtype=np.uint8).reshape(len(q), 32)


def group_key(ds):
    """The 32-byte key of a group of digests (bytes objects or uint8 rows): sha256 of them sorted and concatenated."""
    return hashlib.sha256(b"".join(sorted(bytes(bytearray(d)) for d in ds))).digest()


def reference_key(ds):
    """deduplicate_cad.py's own key: the sorted hex digests joined by '_'."""
    return "_".join(sorted(bytes(bytearray(d)).hex() for d in ds))


def group_keys(ds, offsets):
    return np.array([np.frombuffer(group_key(ds[offsets[n]:offsets[n + 1]]), np.uint8) for n in range(len(offsets) - 1)],
                    dtype=np.uint8).reshape(len(offsets) - 1, 32)


def first_occurrence(keys):
    """bool [N]: True where no earlier key is equal (keys: rows of bytes, or any hashable per entry)."""
    seen, keep = set(), []
    for k in keys:
        k = k.tobytes() if isinstance(k, np.ndarray) else k
        keep.append(k not in seen)
        seen.add(k)
    return np.array(keep, dtype=bool)


def dedup_cads(records, n_bits):
    """Keep mask of the records in the order given (deduplicate_cad.py's walk over the train list)."""
    return first_occurrence([group_key([item_digest(s, n_bits) for s in rec["surf_wcs"]]) for rec in records])


def unique_items(records, which, n_bits):
    """The kept surf_ncs / edge_ncs items, in order (deduplicate_surfedge.py's unique_data as one array)."""
    items = [it for rec in records for it in np.asarray(rec[which], dtype=np.float32)]
    keep = first_occurrence([item_digest(it, n_bits) for it in items])
    return np.array([it for it, k in zip(items, keep) if k], dtype=np.float32)


def lattice_neighbours(n_bits):
    """float32 [3 * 2^n]: every lattice point 2 k / (2^n - 1) - 1 with its two fp32 neighbours."""
    k = np.arange(2 ** n_bits, dtype=np.float64)
    c = (2.0 * k / (2 ** n_bits - 1) - 1.0).astype(np.float32)
    return np.concatenate([np.nextafter(c, np.float32(-2)), c, np.nextafter(c, np.float32(2))]).astype(np.float32)


def load_records(npz, prefix="r"):
    """The records of tests/golden/dedup_records.npz as 12-key dicts in the reference's key order (keys the scripts do not read hold
    empty arrays), in the order the generator stored them."""
    out = []
    for r in range(int(npz[prefix + "count"])):
        rec = {}
        for k in KEYS12:
            if k in GRID_KEYS:
                rec[k] = npz[f"{prefix}{r}_{k}"]
            elif k == "uid":
                rec[k] = str(npz[f"{prefix}{r}_uid"])
            else:
                rec[k] = np.zeros(0, np.float32)
        out.append(rec)
    return out
