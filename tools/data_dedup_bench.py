#!/usr/bin/env python
"""Training-set de-duplication (csrc/hash_dedup.hip) at data-set size: bg_points_sha256 on 2^17 surface grids and 2^20 edge grids of
noise at 6 bits, bg_digest_group_keys + bg_first_occurrence at N = 2^20, next to the reference's own formulation -- numpy real2bit +
hashlib.sha256 per item, one Python loop (data_process/deduplicate_surfedge.py) -- timed on this host's CPU on a subset and scaled
linearly (its work is the same for every item); the record says so.

Two floors are reported beside the hashing kernel ("Training-set de-duplication"):
    memory    bytes read (12 P per item) + 32 written, over the HBM rate
    integer   lane-ops per SHA-256 block (counted in the ISA) x blocks per item x items, over the chip's 32-bit integer issue rate

    python tools/data_dedup_bench.py [--surfaces 131072 --edges 1048576 --cads 1048576 --repeats 5 --out data_dedup.json]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

from bench_common import med

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12                    # MI355X HBM3E peak (spec); a float4 copy reaches about 6.3e12
INT_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9   # 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz: one 32-bit VALU lane-op per lane and clock
LANE_OPS_PER_BLOCK = 1705                   # VALU instructions of one data block in points_sha256_kernel<true> (ISA of the -O3 build:
                                            # 558 v_alignbit, 457 v_xor, 228 v_add3, 87 shifts, 72 adds, 192 bit-selects, ..., 40 for quantising)


def blocks_per_item(P):
    return (24 * P + 9 + 63) // 64          # message + 0x80 + 8 length bytes, in 64-byte blocks


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), res


def real2bit(data, n_bits):                 # convert_utils.real2bit as it stands in the reference
    range_quantize = 2 ** n_bits - 1
    data_quantize = (data - (-1)) * range_quantize / (1 - (-1))
    return np.clip(data_quantize, a_min=0, a_max=range_quantize).astype(int)


def reference_s(items, bit):
    """Seconds the reference's loop takes for `items` on this host: real2bit on the record's array, then sha256 per item."""
    t0 = time.perf_counter()
    bits = real2bit(items, bit)
    seen = set()
    for b in bits:
        seen.add(hashlib.sha256(b.reshape(-1, 3).tobytes()).hexdigest())
    return time.perf_counter() - t0, len(seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--surfaces", type=int, default=1 << 17)
    ap.add_argument("--edges", type=int, default=1 << 20)
    ap.add_argument("--cads", type=int, default=1 << 20)
    ap.add_argument("--faces-per-cad", type=int, default=8)
    ap.add_argument("--bit", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reference-surfaces", type=int, default=512)
    ap.add_argument("--reference-edges", type=int, default=16384)
    ap.add_argument("--out", default=None, help="also write the record to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("data_dedup_bench needs the GPU: a CPU run measures nothing")
    from brepgen_amd import deduplicate as dd
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(1)
    rec = {"device": torch.cuda.get_device_name(dev), "bit": args.bit,
           "timing": "hipEvent pair around one call, one full-size warm-up, median of the repeats",
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "int_lane_ops_per_s": INT_LANE_OPS_PER_S, "lane_ops_per_block": LANE_OPS_PER_BLOCK}

    for name, M, tail, n_ref in (("surfaces", args.surfaces, (32, 32, 3), args.reference_surfaces), ("edges", args.edges, (32, 3), args.reference_edges)):
        x = torch.rand((M,) + tail, generator=g, device=dev) * 2 - 1
        P = int(np.prod(tail)) // 3
        d0 = dd.point_digests(x, args.bit)                                # code object, allocator, one full-size warm-up
        ms = []
        for _ in range(max(3, args.repeats)):
            t, d = event_ms(lambda: dd.point_digests(x, args.bit))
            ms.append(t)
            assert torch.equal(d, d0), "the digests changed between two runs"
        n_ref = min(n_ref, M)
        sub = x[:n_ref].cpu().numpy()
        ref_s, _ = reference_s(sub, args.bit)
        want = hashlib.sha256(real2bit(sub[0], args.bit).reshape(-1, 3).tobytes()).digest()
        assert bytes(d0[0].cpu().numpy()) == want, "device digest differs from the reference's"
        s = med(ms) / 1e3
        mem_floor = M * (12.0 * P + 32.0) / HBM_BYTES_PER_S
        int_floor = float(M) * blocks_per_item(P) * LANE_OPS_PER_BLOCK / INT_LANE_OPS_PER_S
        rec[name] = {"items": M, "points_per_item": P, "sha256_blocks_per_item": blocks_per_item(P),
                     "bg_points_sha256_s": round(s, 6), "all_repeats_ms": [round(v, 3) for v in ms],
                     "items_per_s": M / s, "input_bytes_per_s": M * 12.0 * P / s,
                     "memory_floor_s": round(mem_floor, 6), "integer_issue_floor_s": round(int_floor, 6),
                     "bound_by": "integer issue" if int_floor > mem_floor else "memory",
                     "fraction_of_the_larger_floor": round(max(mem_floor, int_floor) / s, 4),
                     "reference": f"numpy real2bit + hashlib.sha256 per item in one Python loop on this host's CPU, timed on {n_ref} items "
                                  f"and scaled linearly by {M}/{n_ref}",
                     "reference_items_timed": n_ref, "reference_timed_s": round(ref_s, 4), "reference_scaled_s": round(ref_s * M / n_ref, 2),
                     "speedup_over_reference": round(ref_s * M / n_ref / s, 1)}
        del x

    N, F = args.cads, args.faces_per_cad
    digests = torch.randint(0, 256, (N * F, 32), generator=g, device=dev, dtype=torch.uint8)
    half = N // 2
    digests[(N - half) * F:] = digests[:half * F]                         # the last N // 2 CADs repeat the first N // 2
    off = np.arange(N + 1, dtype=np.int64) * F
    k0 = dd.cad_keys(digests, off)
    f0 = dd.first_occurrence(k0)
    assert int(f0.sum()) == N - half and bool(f0[:N - half].all())
    off_dev = torch.from_numpy(off.astype(np.int32)).to(dev)
    key_ms, first_ms = [], []
    for _ in range(max(3, args.repeats)):
        t, k = event_ms(lambda: dd.cad_keys(digests, off_dev, max_group=F))
        key_ms.append(t)
        t, f = event_ms(lambda: dd.first_occurrence(k))
        first_ms.append(t)
        assert torch.equal(k, k0) and torch.equal(f, f0)
    rec["cads"] = {"cads": N, "faces_per_cad": F, "bg_digest_group_keys_s": round(med(key_ms) / 1e3, 6),
                   "bg_first_occurrence_s": round(med(first_ms) / 1e3, 6), "keys_all_repeats_ms": [round(v, 3) for v in key_ms],
                   "first_all_repeats_ms": [round(v, 3) for v in first_ms], "table_slots": dd.table_size(N),
                   "first_occurrence_includes": "clearing the table, both launches and the table / mask allocations"}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
