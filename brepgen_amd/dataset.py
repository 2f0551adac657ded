"""Training batches of the reference's ``dataset.py`` on the MI355X: from a folder of its ``.pkl`` records to the tensors
``training.surface_tokens`` / ``edge_tokens`` / ``ldm_loss`` / ``vae_loss`` take.

    CADStore.keep_mask        -> bg_cad_filter    filter_data / load_data (a ``Pool(os.cpu_count())`` over every record there)
    CADStore.batch            -> bg_batch_plan    the draws, shuffles, pad_repeat / pad_zero of SurfPosData .. EdgeZData.__getitem__
                                 bg_batch_gather  rotation augmentation, recomputed boxes, mating duplication, masks, sorted corners:
                                                  one memory-bound launch per batch (csrc/batch.hip)
    augment_points            -> bg_points_rotate_normalize   SurfData / EdgeData (utils.rotate_point_cloud)

The records are packed once into contiguous device arrays (``CADStore``); a batch is two launches and no host work beyond checking the
records' sizes, which the store keeps on the host.  Nothing here synchronises.  Two deliberate deviations from the reference
(DESIGN.md section 4): the device's draws are Philox blocks keyed by ``sampling.noise_key(generator)`` and the record's GLOBAL number,
not numpy's global stream (``draws=`` replays recorded ones: the parity mode), and on the augmented path exact zeros stay exact, so a
corner pair that ties exactly in its leading coordinate is ordered by the next one.  There is no CPU path: without a GPU or the
library every entry raises ``BrepgenHipError``.
"""
import ctypes as C
import pickle

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .sampling import noise_key

KINDS = {"SurfPos": _lib.BG_SURFPOS, "SurfZ": _lib.BG_SURFZ, "EdgePos": _lib.BG_EDGEPOS, "EdgeZ": _lib.BG_EDGEZ}
_RECORD_KEYS = ("surf_ncs", "edge_ncs", "corner_wcs", "faceEdge_adj", "surf_bbox_wcs", "edge_bbox_wcs")
# draws= members: (name, dtype, shape per CAD as a function of (S, E))
_DRAWS = (("u", np.float64, lambda S, E: ()), ("turns", np.int32, lambda S, E: (3,)),
          ("face_key1", np.int64, lambda S, E: (S,)), ("face_key2", np.int64, lambda S, E: (S,)),
          ("edge_key1", np.int64, lambda S, E: (S, E)), ("edge_key2", np.int64, lambda S, E: (S, E)))


def _device(device=None):
    _lib.load()
    if device is not None and torch.device(device).type != "cuda":
        raise _lib.BrepgenHipError(f"brepgen_amd.dataset runs on the MI355X only (device {device!r}); there is no CPU fallback")
    if not torch.cuda.is_available():
        raise _lib.BrepgenHipError("brepgen_amd runs on the MI355X only (no GPU visible); no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _check_record(rec, r):
    missing = [k for k in _RECORD_KEYS if k not in rec]
    if missing:
        raise ValueError(f"record {r}: missing {missing}")
    F, Ne = len(rec["surf_bbox_wcs"]), len(rec["edge_bbox_wcs"])
    shapes = {"surf_ncs": (F, 32, 32, 3), "surf_bbox_wcs": (F, 6), "edge_ncs": (Ne, 32, 3), "edge_bbox_wcs": (Ne, 6), "corner_wcs": (Ne, 2, 3)}
    for k, want in shapes.items():
        got = tuple(np.shape(rec[k]))
        if got != want and not (0 in want and int(np.prod(got)) == 0):
            raise ValueError(f"record {r}: {k} has shape {got}, expected {want}")
    if len(rec["faceEdge_adj"]) != F:
        raise ValueError(f"record {r}: faceEdge_adj lists {len(rec['faceEdge_adj'])} faces, surf_bbox_wcs {F}")
    for f, adj in enumerate(rec["faceEdge_adj"]):
        a = np.asarray(adj, dtype=np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() >= Ne):
            raise ValueError(f"record {r}: face {f} refers to edges outside 0 .. {Ne - 1}")


class CADStore:
    """N records packed once on the device.  Members (device tensors): surf_ncs [sum F, 32, 32, 3], surf_pos [sum F, 6], edge_ncs
    [sum E, 32, 3], edge_pos [sum E, 6], corner_wcs [sum E, 2, 3], face_off / edge_off [N + 1], adj_off [sum F + 1], adj_idx [sum A]
    (edge ids local to the CAD), cls [N] (-1 = none).  On the host: n_faces [N], max_degree / min_degree [N], classes [N]."""

    def _summarise(self, records, classes):
        """The host side of the store: sizes per record, checked (no device involved)."""
        if classes is not None and len(classes) != len(records):
            raise ValueError(f"{len(classes)} classes for {len(records)} records")
        for r, rec in enumerate(records):
            _check_record(rec, r)
        self.n_records = len(records)
        self.n_faces = np.array([len(rec["surf_bbox_wcs"]) for rec in records], dtype=np.int64)
        self.n_edges = np.array([len(rec["edge_bbox_wcs"]) for rec in records], dtype=np.int64)
        degrees = [[len(a) for a in rec["faceEdge_adj"]] for rec in records]
        self.max_degree = np.array([max(d, default=0) for d in degrees], dtype=np.int64)
        self.min_degree = np.array([min(d, default=0) for d in degrees], dtype=np.int64)
        self.classes = None if classes is None else np.asarray(classes, dtype=np.int64)
        flat_deg = np.array([d for ds in degrees for d in ds], dtype=np.int64)
        if max(int(self.n_faces.sum()), int(self.n_edges.sum()), int(flat_deg.sum())) >= 2 ** 31 - 1:
            raise ValueError("the records exceed the int32 offsets of one store; split them")
        return flat_deg

    @classmethod
    def from_records(cls, records, device=None, classes=None):
        device = _device(device)
        records = list(records)
        self = cls.__new__(cls)
        flat_deg = self._summarise(records, classes)
        n, n_edges = self.n_records, self.n_edges

        def cat(key, tail, dtype=np.float32):
            parts = [np.asarray(rec[key], dtype=dtype).reshape((-1,) + tail) for rec in records]
            parts.append(np.zeros((1,) + tail, dtype=dtype))                 # one pad row: never an empty allocation
            return torch.from_numpy(np.ascontiguousarray(np.concatenate(parts))).to(device)

        def offsets(sizes):
            return torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(device)

        self.surf_ncs, self.surf_pos = cat("surf_ncs", (32, 32, 3)), cat("surf_bbox_wcs", (6,))
        self.edge_ncs, self.edge_pos = cat("edge_ncs", (32, 3)), cat("edge_bbox_wcs", (6,))
        self.corner_wcs = cat("corner_wcs", (2, 3))
        self.face_off, self.edge_off, self.adj_off = offsets(self.n_faces), offsets(n_edges), offsets(flat_deg)
        adj = [np.asarray(a, dtype=np.int32).reshape(-1) for rec in records for a in rec["faceEdge_adj"]] + [np.zeros(1, np.int32)]
        self.adj_idx = torch.from_numpy(np.concatenate(adj)).to(device)
        self.cls = torch.from_numpy(np.full(n, -1, np.int32) if classes is None else self.classes.astype(np.int32)).to(device)
        self.device = device
        self._c = _lib.CadStore(ptr(self.surf_ncs), ptr(self.surf_pos), ptr(self.edge_ncs), ptr(self.edge_pos), ptr(self.corner_wcs),
                                ptr(self.face_off), ptr(self.edge_off), ptr(self.adj_off), ptr(self.adj_idx),
                                n, int(self.n_faces.sum()), int(n_edges.sum()), int(flat_deg.sum()))
        return self

    @classmethod
    def from_pickles(cls, paths, classes=None, device=None):
        """The reference's per-CAD pickles (process_brep.py), in the order given: the position in `paths` is the GLOBAL record number."""
        records = []
        for path in paths:
            with open(path, "rb") as f:
                records.append(pickle.load(f))
        return cls.from_records(records, device, classes)

    def __len__(self):
        return self.n_records

    @torch.no_grad()
    def keep_mask(self, max_face, max_edge, bbox_scaled=3, threshold=0.05):
        """bool [N] on the device: filter_data's verdict for every record (True = admitted)."""
        keep = torch.empty(len(self), dtype=torch.uint8, device=self.device)
        check(_lib.load().bg_cad_filter(C.byref(self._c), int(max_face), int(max_edge), float(bbox_scaled), float(threshold), ptr(keep),
                                        stream()), "bg_cad_filter")
        return keep.bool()

    def _unique_rows(self, grids, n, bit):
        from . import deduplicate
        if n == 0:
            return torch.empty(0, dtype=torch.int64, device=self.device)
        return deduplicate.first_occurrence(deduplicate.point_digests(grids[:n], bit)).nonzero().reshape(-1)

    @torch.no_grad()
    def unique_surfaces(self, bit=6):
        """int64 [K] on the device, ascending: the rows of surf_ncs that deduplicate_surfedge.py keeps (first occurrence of every
        `bit`-bit quantised grid; deduplicate.py), the store's pad row excluded.  Turning the mask into row numbers synchronises once."""
        return self._unique_rows(self.surf_ncs, self._c.n_faces, bit)

    @torch.no_grad()
    def unique_edges(self, bit=6):
        """int64 [K] on the device, ascending: the same for the rows of edge_ncs."""
        return self._unique_rows(self.edge_ncs, self._c.n_edges, bit)

    def _indices(self, indices, max_face, max_edge):
        idx = _host(indices).astype(np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise ValueError(f"record numbers must lie in 0 .. {len(self) - 1}")
        for r in idx:
            if self.n_faces[r] > max_face:
                raise ValueError(f"record {r} has {self.n_faces[r]} faces, more than max_face = {max_face} (keep_mask filters such records)")
            if self.n_faces[r] and (self.max_degree[r] > max_edge or self.min_degree[r] == 0):
                raise ValueError(f"record {r} has a face with {self.max_degree[r] if self.max_degree[r] > max_edge else 0} edges "
                                 f"(allowed: 1 .. max_edge = {max_edge}; keep_mask filters such records)")
        return idx

    def _draws(self, draws, B, S, E):
        """The caller's recorded draws as the C struct (+ the tensors that back it)."""
        unknown = set(draws) - {name for name, _, _ in _DRAWS}
        if unknown:
            raise ValueError(f"draws: unknown members {sorted(unknown)}")
        held, fields = [], {}
        for name, dtype, shape in _DRAWS:
            if draws.get(name) is None:
                continue
            a = np.ascontiguousarray(_host(draws[name]))
            if tuple(a.shape) != (B,) + shape(S, E):
                raise ValueError(f"draws[{name!r}]: expected shape {(B,) + shape(S, E)}, got {tuple(a.shape)}")
            a = a.astype(dtype)
            if name == "turns" and a.size and (a.min() < 1 or a.max() > 3):
                raise ValueError("draws['turns']: quarter turns are 1, 2 or 3")
            if dtype is np.int64:                                                # uint32 keys travel as their int32 bit pattern
                if a.size and (a.min() < 0 or a.max() >= 2 ** 32):
                    raise ValueError(f"draws[{name!r}]: keys are uint32")
                a = a.astype(np.uint32).view(np.int32)
            t = torch.from_numpy(a).to(self.device)
            held.append(t)
            fields[name] = ptr(t)
        return _lib.BatchDraws(**fields), held

    @torch.no_grad()
    def plan(self, kind, indices, max_face, max_edge, aug=False, generator=None, draw_id=0, draws=None):
        """The slot maps of a batch (bg_batch_plan): face_src [B, S] int32, edge_src [B, S, E] int32 (None for the face kinds), rot [B]
        int32, scale [B, 3] float64 -- rows of the store's arrays, -1 = zero padding."""
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
        S, E = int(max_face), int(max_edge)
        idx = self._indices(indices, S, E)
        B = len(idx)
        idx_dev = torch.from_numpy(idx.astype(np.int32)).to(self.device)
        face_src = torch.empty(B, S, dtype=torch.int32, device=self.device)
        edge_src = torch.empty(B, S, E, dtype=torch.int32, device=self.device) if KINDS[kind] >= _lib.BG_EDGEPOS else None
        rot = torch.empty(B, dtype=torch.int32, device=self.device)
        scale = torch.empty(B, 3, dtype=torch.float64, device=self.device)
        c_draws, held = (None, None) if draws is None else self._draws(draws, B, S, E)
        seed = 0 if draws is not None else noise_key(generator)
        check(_lib.load().bg_batch_plan(C.byref(self._c), ptr(idx_dev), B, KINDS[kind], S, E, int(bool(aug)), seed & 0xFFFFFFFFFFFFFFFF,
                                        int(draw_id) & 0xFFFFFFFF, None if c_draws is None else C.byref(c_draws), ptr(face_src),
                                        ptr(edge_src), ptr(rot), ptr(scale), stream()), "bg_batch_plan")
        del held                                   # stream-ordered allocator: the plan launch is already queued behind their upload
        return face_src, edge_src, rot, scale, idx

    @torch.no_grad()
    def batch(self, kind, indices, max_face, max_edge, bbox_scaled=3, aug=False, generator=None, draw_id=0, draws=None, out=None):
        """One batch of `kind` ("SurfPos", "SurfZ", "EdgePos", "EdgeZ") for the records `indices` (host integers), as the reference's
        dataset returns it after the default collate, on the device:
            SurfPos: (surf_pos [B,S,6],)                  SurfZ: (surf_pos, surf_ncs [B,S,32,32,3], surf_mask [B,S] bool)
            EdgePos: (edge_pos [B,S,E,6], surf_ncs, surf_pos, surf_mask)
            EdgeZ:   (edge_ncs [B,S,E,32,3], edge_pos, edge_mask [B,S,E] bool, surf_ncs, surf_pos, vertex_pos [B,S,E,6])
        plus class_label int64 [B, 1] = class + 1 when the store has classes.  Draws come from Philox, keyed by
        noise_key(generator) and draw_id, or from `draws` (dict: u [B], turns [B,3], face_key1 / face_key2 [B,S], edge_key1 /
        edge_key2 [B,S,E]; see include/brepgen_hip.h).  `out`: a dict of preallocated tensors to write into (tests)."""
        face_src, edge_src, rot, scale, idx = self.plan(kind, indices, max_face, max_edge, aug, generator, draw_id, draws)
        B, S, E, k = len(idx), int(max_face), int(max_edge), KINDS[kind]
        shapes = {"surf_pos": ((B, S, 6), torch.float32)}
        if k != _lib.BG_SURFPOS:
            shapes["surf_ncs"] = ((B, S, 32, 32, 3), torch.float32)
        if k in (_lib.BG_SURFZ, _lib.BG_EDGEPOS):
            shapes["surf_mask"] = ((B, S), torch.uint8)
        if k >= _lib.BG_EDGEPOS:
            shapes["edge_pos"] = ((B, S, E, 6), torch.float32)
        if k == _lib.BG_EDGEZ:
            shapes.update(edge_ncs=((B, S, E, 32, 3), torch.float32), edge_mask=((B, S, E), torch.uint8), vertex_pos=((B, S, E, 6), torch.float32))
        t = {}
        for name, (shape, dtype) in shapes.items():
            t[name] = torch.empty(shape, dtype=dtype, device=self.device) if out is None else out[name]
            if out is not None and (t[name].numel() != int(np.prod(shape)) or t[name].dtype != dtype or not t[name].is_cuda):
                raise ValueError(f"out[{name!r}]: expected {int(np.prod(shape))} elements of {dtype} on the device")
        c_out = _lib.BatchOut(**{name: ptr(v) for name, v in t.items()})
        check(_lib.load().bg_batch_gather(C.byref(self._c), k, B, S, E, float(bbox_scaled), ptr(face_src), ptr(edge_src), ptr(rot), ptr(scale),
                                          C.byref(c_out), stream()), "bg_batch_gather")
        for name in ("surf_mask", "edge_mask"):
            if name in t:
                t[name] = t[name].view(torch.bool).reshape(shapes[name][0])
        order = {"SurfPos": ("surf_pos",), "SurfZ": ("surf_pos", "surf_ncs", "surf_mask"),
                 "EdgePos": ("edge_pos", "surf_ncs", "surf_pos", "surf_mask"),
                 "EdgeZ": ("edge_ncs", "edge_pos", "edge_mask", "surf_ncs", "surf_pos", "vertex_pos")}[kind]
        result = tuple(t[name] if out is None else t[name].reshape(shapes[name][0]) for name in order)
        if self.classes is not None:
            result += (torch.from_numpy(self.classes[idx] + 1).reshape(B, 1).to(self.device),)
        return result


@torch.no_grad()
def augment_points(x, aug=True, generator=None, draw_id=0, draws=None, first_item=0, out=None):
    """SurfData / EdgeData's augmentation for a batch x [M, ..., 3] (fp32, device; e.g. [M, 32, 32, 3] or [M, 32, 3]; at most 1024
    points per item): item m is rotated about x, y, z by random quarter turns and normalised (utils.rotate_point_cloud, in fp64) iff
    aug and its uniform draw exceeds 0.5; every other item is a bitwise copy.  Draws: Philox keyed by noise_key(generator), draw_id and
    the GLOBAL item number first_item + m, or `draws` = {"u": [M], "turns": [M, 3]}."""
    _lib.load()
    if not torch.is_tensor(x) or not x.is_cuda:
        raise _lib.BrepgenHipError("augment_points runs on the MI355X only (x must be a device tensor); there is no CPU fallback")
    if x.dim() < 3 or x.shape[-1] != 3 or x.dtype != torch.float32:
        raise ValueError(f"expected fp32 points [M, ..., 3], got {tuple(x.shape)} {x.dtype}")
    x = x.contiguous()
    M = x.shape[0]
    P = x[0].numel() // 3 if M else 1
    if not 1 <= P <= 1024:
        raise ValueError(f"{P} points per item; bg_points_rotate_normalize takes 1 .. 1024")
    u = turns = None
    if draws is not None:
        u = torch.as_tensor(_host(draws["u"])).to(torch.float64).reshape(-1).contiguous().to(x.device)
        turns = torch.as_tensor(_host(draws["turns"])).to(torch.int32).reshape(-1, 3).contiguous()
        if u.shape[0] != M or turns.shape[0] != M:
            raise ValueError(f"draws: expected u [{M}] and turns [{M}, 3]")
        if turns.numel() and (int(turns.min()) < 1 or int(turns.max()) > 3):
            raise ValueError("draws['turns']: quarter turns are 1, 2 or 3")
        turns = turns.to(x.device)
    res = torch.empty_like(x) if out is None else out
    seed = 0 if draws is not None else noise_key(generator)
    check(_lib.load().bg_points_rotate_normalize(ptr(x), M, P, int(bool(aug)), seed & 0xFFFFFFFFFFFFFFFF, int(draw_id) & 0xFFFFFFFF,
                                                 int(first_item), ptr(u), ptr(turns), ptr(res), stream()), "bg_points_rotate_normalize")
    return res
