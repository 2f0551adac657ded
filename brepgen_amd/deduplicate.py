"""Training-set de-duplication of the reference's ``data_process/`` on the MI355X: the step between ``process_brep.py`` and training
that turns parsed CADs into the lists the loaders start from.

    point_digests     -> bg_points_sha256       sha256(real2bit(item, bit).reshape(-1, 3).tobytes()) of every surface / edge grid
    cad_keys          -> bg_digest_group_keys   deduplicate_cad.py's key of a CAD: its faces' digests, sorted (as one 32-byte hash)
    first_occurrence  -> bg_first_occurrence    "keep an item iff its key is new", walking in order
    dedup_cads        deduplicate_cad.py        records (or pickles) -> keep mask of the train list      (*_data_split_6bit.pkl)
    unique_items      deduplicate_surfedge.py   records (or pickles) -> the kept surf_ncs / edge_ncs     (*_surface.pkl, *_edge.pkl)
    CADStore.unique_surfaces / unique_edges     the same on a store's arrays, which already sit on the device (dataset.py)

    python -m brepgen_amd.deduplicate cad --data DIR --split FILE --bit 6 --option {abc,deepcad,furniture} [--out FILE]
    python -m brepgen_amd.deduplicate surfedge --data DIR --list FILE [--edge] --bit 6 --option {abc,deepcad,furniture} [--out FILE]

Both commands write pickles in the reference's formats under its default names (``<option>_data_split_<bit>bit.pkl`` in the working
directory; ``<list without extension>_surface.pkl`` / ``_edge.pkl``).  Scope: the 90/5/5 ``random.shuffle`` split of
``load_abc_pkl`` / ``load_furniture_pkl`` and the DeepCAD json are host bookkeeping and are not rebuilt -- ``--split`` takes a pickle
with ``train`` / ``val`` / ``test`` uid lists instead.  A data set does not fit the device at once, its 32-byte digests do: records are
hashed ``chunk`` at a time, keys and first occurrence run once over everything.  There is no CPU path: without a GPU or the library
every entry raises ``BrepgenHipError``.
"""
import argparse
import math
import os
import pickle

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from ._train import require_device
from .dataset import _device

P_MAX, BIT_MAX, GROUP_MAX = 1024, 16, 4096      # csrc/hash_dedup.hip


def table_size(n):
    """Slots of bg_first_occurrence's table for n keys: the power of two >= 2 n (>= 2)."""
    return max(2, 1 << (2 * int(n) - 1).bit_length()) if n > 0 else 2


def _on_device(t, what, dtype):
    _lib.load()
    require_device(t, what)
    if t.dtype != dtype:
        raise ValueError(f"{what}: expected {dtype}, got {t.dtype}")
    return t.contiguous()


@torch.no_grad()
def point_digests(x, bit=6, out=None):
    """uint8 [M, 32] on the device: the SHA-256 of every item of x [M, ..., 3] (fp32, device; at most 1024 points per item) quantised
    to `bit` bits, as the reference's scripts hash it.  ``bytes(d[m].tolist()).hex()`` is its hexdigest.  Does not synchronise."""
    x = _on_device(x, "point_digests", torch.float32)
    if x.dim() < 2 or x.shape[-1] != 3:
        raise ValueError(f"expected fp32 points [M, ..., 3], got {tuple(x.shape)}")
    M = x.shape[0]
    P = x[0].numel() // 3 if M else 1
    if not 1 <= P <= P_MAX or not 1 <= int(bit) <= BIT_MAX:
        raise ValueError(f"{P} points per item at {bit} bits; bg_points_sha256 takes 1 .. {P_MAX} points and 1 .. {BIT_MAX} bits")
    d = torch.empty(M, 32, dtype=torch.uint8, device=x.device) if out is None else out
    check(_lib.load().bg_points_sha256(ptr(x), M, P, int(bit), ptr(d), stream()), "bg_points_sha256")
    return d


@torch.no_grad()
def cad_keys(digests, offsets, max_group=None, out=None):
    """uint8 [N, 32] on the device: key n = sha256 of the sorted digests offsets[n] .. offsets[n + 1] - 1.  `offsets` [N + 1] ascending,
    on the host (numpy, list, CPU tensor); a device tensor needs `max_group` (the largest group), since reading it back would
    synchronise.  Does not synchronise."""
    digests = _on_device(digests, "cad_keys", torch.uint8)
    if digests.dim() != 2 or digests.shape[1] != 32:
        raise ValueError(f"expected digests [M, 32], got {tuple(digests.shape)}")
    if torch.is_tensor(offsets) and offsets.is_cuda:
        if max_group is None:
            raise ValueError("cad_keys: offsets on the device need max_group (the largest group) from the host")
        off = offsets.to(torch.int32).contiguous()
    else:
        o = np.asarray(offsets.numpy() if torch.is_tensor(offsets) else offsets, dtype=np.int64).reshape(-1)
        if o.size < 1 or o[0] < 0 or (np.diff(o) < 0).any() or o[-1] > digests.shape[0]:
            raise ValueError(f"cad_keys: offsets must ascend from >= 0 to <= {digests.shape[0]} digests")
        max_group = int(np.diff(o).max()) if o.size > 1 else 0
        off = torch.from_numpy(o.astype(np.int32)).to(digests.device)
    N = off.numel() - 1
    if not 0 <= int(max_group) <= GROUP_MAX:
        raise ValueError(f"cad_keys: a group of {max_group} digests; bg_digest_group_keys takes at most {GROUP_MAX}")
    key = torch.empty(N, 32, dtype=torch.uint8, device=digests.device) if out is None else out
    check(_lib.load().bg_digest_group_keys(ptr(digests), ptr(off), N, int(max_group), ptr(key), stream()), "bg_digest_group_keys")
    return key


@torch.no_grad()
def first_occurrence(keys):
    """bool [N] on the device: True where no earlier row of keys [N, 32] (uint8, device) is the same.  Does not synchronise."""
    keys = _on_device(keys, "first_occurrence", torch.uint8)
    if keys.dim() != 2 or keys.shape[1] != 32:
        raise ValueError(f"expected keys [N, 32], got {tuple(keys.shape)}")
    N = keys.shape[0]
    T = table_size(N)
    table = torch.empty(T, dtype=torch.int32, device=keys.device)
    keep = torch.empty(N, dtype=torch.uint8, device=keys.device)
    check(_lib.load().bg_first_occurrence(ptr(keys), N, ptr(table), T, ptr(keep), stream()), "bg_first_occurrence")
    return keep.bool()


def _records(records):
    for rec in records:
        if isinstance(rec, (str, os.PathLike)):
            with open(rec, "rb") as f:
                rec = pickle.load(f)
        yield rec


def _chunks(records, key, chunk):
    """(items [m, P, 3] float32 on the host, items per record) for every `chunk` records, in order."""
    parts, counts, P = [], [], None

    def flush():
        full = [p for p in parts if len(p)]
        items = np.concatenate(full) if full else np.zeros((0, P or 1, 3), np.float32)
        return np.ascontiguousarray(items), counts

    for rec in _records(records):
        a = np.asarray(rec[key], dtype=np.float32)
        a = a.reshape(len(a), -1, 3) if a.size else np.zeros((0, P or 1, 3), np.float32)
        if a.size:
            if P not in (None, a.shape[1]):
                raise ValueError(f"{key}: items of {a.shape[1]} points after items of {P}")
            P = a.shape[1]
        parts.append(a)
        counts.append(len(a))
        if len(counts) == chunk:
            yield flush()
            parts, counts = [], []
    if counts:
        yield flush()


def _digest_chunks(records, key, bit, chunk, device, keep_items):
    """All digests [sum m, 32] on the device, the per-record counts, and (keep_items) the host chunks themselves."""
    if int(chunk) < 1:
        raise ValueError("chunk must be at least one record")
    digests, counts, held = [], [], []
    for items, c in _chunks(records, key, int(chunk)):
        counts += c
        if len(items):
            digests.append(point_digests(torch.from_numpy(items).to(device), bit))
            if keep_items:
                held.append(items)
    d = torch.cat(digests) if digests else torch.empty(0, 32, dtype=torch.uint8, device=device)
    return d, np.asarray(counts, dtype=np.int64), held


@torch.no_grad()
def dedup_cads(records, bit=6, chunk=1024, device=None):
    """deduplicate_cad.py: host bool [N], True for the records (dicts, or paths to pickles; read in the order given) whose sorted
    ``surf_wcs`` digests have not been seen before.  Faces are quantised and hashed `chunk` records at a time; keys and first occurrence
    run once over all digests.  One host synchronisation: the mask's copy back."""
    device = _device(device)
    d, counts, _ = _digest_chunks(records, "surf_wcs", bit, chunk, device, False)
    if counts.sum() >= 2 ** 31 - 1:
        raise ValueError("more faces than the int32 offsets of one call hold; split the list")
    keys = cad_keys(d, np.concatenate([[0], np.cumsum(counts)]))
    return first_occurrence(keys).cpu().numpy()


@torch.no_grad()
def unique_items(records, which="surf_ncs", bit=6, chunk=1024, device=None):
    """deduplicate_surfedge.py: the kept ``surf_ncs`` / ``edge_ncs`` items of the records as one float32 array [K, 32, 32, 3] /
    [K, 32, 3] in the reference's order (``list(result)`` is its ``unique_data``).  One digest array is kept across the chunks and one
    first-occurrence pass runs at the end; the kept rows are gathered on the host from the chunks already seen, which needs the one host
    synchronisation of this function: the keep mask's copy back."""
    if which not in ("surf_ncs", "edge_ncs"):
        raise ValueError(f"which must be 'surf_ncs' or 'edge_ncs', got {which!r}")
    device = _device(device)
    d, _, held = _digest_chunks(records, which, bit, chunk, device, True)
    tail = (32, 32, 3) if which == "surf_ncs" else (32, 3)
    if not held:
        return np.zeros((0,) + tail, np.float32)
    keep = first_occurrence(d).cpu().numpy()
    items = np.concatenate(held)[keep]
    return items.reshape((len(items),) + tail) if items.shape[1] * 3 == math.prod(tail) else items


def record_path(data, uid, option):
    """Where the reference's scripts look for record `uid`: DIR/uid (furniture) or DIR/<uid // 10000, four digits>/uid."""
    if option == "furniture":
        return os.path.join(data, uid)
    return os.path.join(data, str(math.floor(int(uid.split(".")[0]) / 10000)).zfill(4), uid)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m brepgen_amd.deduplicate", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("cad", "surfedge"):
        p = sub.add_parser(name)
        p.add_argument("--data", required=True, help="folder of the per-CAD pickles")
        p.add_argument("--bit", type=int, default=6, help="de-duplication precision")
        p.add_argument("--option", choices=["abc", "deepcad", "furniture"], default="abc")
        p.add_argument("--chunk", type=int, default=1024, help="records hashed per upload")
        p.add_argument("--out", default=None, help="output pickle (default: the reference's name)")
        if name == "cad":
            p.add_argument("--split", required=True, help="pickle with 'train' / 'val' / 'test' uid lists")
        else:
            p.add_argument("--list", required=True, help="pickle whose 'train' entry lists the uids")
            p.add_argument("--edge", action="store_true", help="edges instead of surfaces")
    args = ap.parse_args(argv)
    with open(args.split if args.cmd == "cad" else args.list, "rb") as f:
        split = pickle.load(f)
    paths = [record_path(args.data, uid, args.option) for uid in split["train"]]
    if args.cmd == "cad":
        keep = dedup_cads(paths, args.bit, args.chunk)
        result = {"train": [uid for uid, k in zip(split["train"], keep) if k], "val": split["val"], "test": split["test"]}
        out = args.out or f"{args.option}_data_split_{args.bit}bit.pkl"
        kept, total = len(result["train"]), len(paths)
    else:
        result = list(unique_items(paths, "edge_ncs" if args.edge else "surf_ncs", args.bit, args.chunk))
        out = args.out or os.path.splitext(args.list)[0] + ("_edge.pkl" if args.edge else "_surface.pkl")
        kept, total = len(result), None
    with open(out, "wb") as f:
        pickle.dump(result, f)
    print(f"{out}: kept {kept}" + (f" of {total}" if total is not None else ""))


if __name__ == "__main__":
    main()
