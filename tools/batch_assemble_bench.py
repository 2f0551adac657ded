#!/usr/bin/env python
"""Batch assembly (bg_batch_plan + bg_batch_gather, csrc/batch.hip) at the reference's training shape: one EdgeZ and one SurfZ batch of
`--batch` CADs x `--max_face` faces x `--max_edge` edges from a store of `--records` synthetic records, augmentation on.  Per kind: the
gather kernel's time (hipEvent pair around the launch, bg_profile_begin / bg_profile_end), the bytes it reads plus writes (counted from
the plan: a padded slot is written, not read), the resulting TB/s, the time of the whole `CADStore.batch` call, and the wall time of the
numpy restatement (tests/dataset_restate.py) of the same batch on this host -- the only "before" there is: the reference assembles its
batches in numpy inside DataLoader workers.

The yardstick is the CDNA guide's figure for whole random rows gathered into registers (5.5-5.8 TB/s at 1,152- and 2,304-byte rows, a
float4 copy at 6.29 TB/s); it is REPORTED, not asserted: the edge rows here are 384 bytes, shorter than any row of that table.

    python tools/batch_assemble_bench.py [--records 512 --batch 256 --max_face 50 --max_edge 30 --repeats 20 --out profiles/r10/batch_assemble.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GUIDE_GATHER_TBPS = [5.5, 5.8]
GUIDE_COPY_TBPS = 6.29


def synthetic_record(rng, max_face, max_edge):
    """A closed-shell-like record: F faces on a ring plus random chords, every edge in two faces, degrees in 1 .. max_edge."""
    F = int(rng.integers(max(2, max_face // 2), max_face + 1))
    pairs = [(0, 1)] if F == 2 else [(i, (i + 1) % F) for i in range(F)]
    deg = np.bincount(np.array(pairs).ravel(), minlength=F)
    for _ in range(int(rng.integers(F, 4 * F))):
        i, j = rng.choice(F, size=2, replace=False)
        if deg[i] < max_edge and deg[j] < max_edge:
            pairs.append((int(i), int(j)))
            deg[i] += 1
            deg[j] += 1
    adj = [[] for _ in range(F)]
    for e, (i, j) in enumerate(pairs):
        adj[i].append(e)
        adj[j].append(e)
    n = len(pairs)
    lo = rng.uniform(-1, 0, size=(F + n, 3))
    box = np.concatenate([lo, lo + rng.uniform(0.1, 1, size=(F + n, 3))], 1).astype(np.float32)
    return {"surf_ncs": rng.uniform(-1, 1, size=(F, 32, 32, 3)).astype(np.float32), "edge_ncs": rng.uniform(-1, 1, size=(n, 32, 3)).astype(np.float32),
            "corner_wcs": rng.uniform(-1, 1, size=(n, 2, 3)).astype(np.float32), "faceEdge_adj": [np.array(a) for a in adj],
            "surf_bbox_wcs": box[:F], "edge_bbox_wcs": box[F:]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=512)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--max_face", type=int, default=50)
    ap.add_argument("--max_edge", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the record to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_assemble_bench needs the GPU: a CPU run measures nothing")
    import brepgen_amd as bga
    from brepgen_amd import _lib
    from brepgen_amd.sampling import noise_key
    from tests import dataset_restate as dr
    rng = np.random.default_rng(10)
    S, E, B = args.max_face, args.max_edge, args.batch
    records = [synthetic_record(rng, S, E) for _ in range(args.records)]
    store = bga.CADStore.from_records(records)
    keep = store.keep_mask(S, E)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    rec = {"records": args.records, "batch": B, "max_face": S, "max_edge": E, "device": torch.cuda.get_device_name(0),
           "store_bytes": int(sum(t.numel() * t.element_size() for t in (store.surf_ncs, store.edge_ncs, store.surf_pos, store.edge_pos,
                                                                          store.corner_wcs))),
           "records_admitted_by_keep_mask": int(keep.sum()),
           "kernel_timing": "hipEvent pair around the bg_batch_gather launch (bg_profile_begin / bg_profile_end), median of the repeats, a "
                            "different random batch each repeat, two warm-up batches",
           "call_timing": "torch.cuda.Event pair around CADStore.batch (index upload, bg_batch_plan, output allocation, bg_batch_gather)",
           "guide_gather_TBps": GUIDE_GATHER_TBPS, "guide_float4_copy_TBps": GUIDE_COPY_TBPS,
           "note": "no figure for this kernel existed before it: nothing in the project preceded it; the guide's rows are 1,152 and "
                   "2,304 bytes long, the edge grids here 384 bytes"}
    for kind in ("EdgeZ", "SurfZ"):
        gen = torch.Generator().manual_seed(1)
        batches = [rng.choice(args.records, size=B, replace=False) for _ in range(args.repeats + 2)]
        for ids in batches[:2]:
            store.batch(kind, ids, S, E, aug=True, generator=gen)
        torch.cuda.synchronize()
        kernel_ms, call_ms, moved = [], [], []
        for r, ids in enumerate(batches[2:]):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with _lib.profile() as prof:
                start.record()
                out = store.batch(kind, ids, S, E, aug=True, generator=gen, draw_id=r)
                stop.record()
                torch.cuda.synchronize()
            call_ms.append(start.elapsed_time(stop))
            kernel_ms.append(sum(row["total_ms"] for row in prof.rows))
            face_src, edge_src, _, _, _ = store.plan(kind, ids, S, E, aug=True, generator=gen, draw_id=r)
            live_f = int((face_src >= 0).sum())
            n_f = B * S
            read = live_f * (12288 + 24) + n_f * 4
            written = n_f * (12288 + 24 + (1 if kind == "SurfZ" else 0))
            if kind == "EdgeZ":
                live_e, n_e = int((edge_src >= 0).sum()), B * S * E
                read += live_e * (384 + 24 + 24) + n_e * 4
                written += n_e * (384 + 24 + 24 + 1)
            moved.append(read + written)
        k, m = med(kernel_ms), med(moved)
        # the numpy restatement of the last batch, with the device's own draws
        draws = dr.philox_draws(ids, S, E, noise_key(gen), args.repeats - 1)
        t0 = time.perf_counter()
        want = dr.batch(records, ids, kind, S, E, 3, True, draws)
        numpy_s = time.perf_counter() - t0
        same = all(a.cpu().numpy().tobytes() == w.tobytes() for a, w in zip(out, want))
        rec[kind] = {"gather_kernel_ms": round(k, 4), "gather_kernel_all_repeats_ms": [round(v, 4) for v in kernel_ms],
                     "batch_call_ms": round(med(call_ms), 4), "bytes_read_plus_written": int(m),
                     "bytes_formula": "read: live rows x (grid + box [+ corners]) + 4 B per slot of the plan; written: every slot's grid, box "
                                      "[, corners] and mask byte",
                     "TBps": round(m / (k * 1e-3) / 1e12, 3), "output_bytes": int(sum(t.numel() * t.element_size() for t in out)),
                     "numpy_restatement_same_host_s": round(numpy_s, 3), "equals_numpy_restatement_bitwise": bool(same)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
