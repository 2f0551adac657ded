#!/usr/bin/env python
"""Pairwise Chamfer matrix (bg_chamfer_pairwise, csrc/metrics.hip) at the reference's operating point -- pc_metric.py's main: 3 x 1000
generated against 1000 test clouds of 2000 points -- next to torch-ROCm eager running the reference's own formulation on the same GPU in
the same process (three bmm per batch of 64 reference clouds, the expanded |x|^2 + |y|^2 - 2 x.y matrix, two min reductions: what
pc_metric.py's distChamfer does).  The yardstick is timed on `--yardstick-rows` sample clouds and scaled linearly to S (its work is the
same for every row); the record says so.

    python tools/metrics_bench.py [--S 3000 --R 1000 --P 2000 --repeats 5 --yardstick-rows 8 --out metrics_pairwise.json]
    python tools/metrics_bench.py --single          # one call and nothing else: the program for a kernel trace
"""
import argparse
import glob
import json
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_VECTOR_FLOPS = 157.3e12                # MI355X peak fp32 vector rate; one fma lane-op = 2 flop
LANE_OPS_PER_POINT_PAIR = 7                 # direct form: 3 sub + 1 mul + 2 fma + two halves of a v_min3 (row minimum, column partial)
                                            # (pinned in the ISA by tests/test_metrics_cpu.py::test_chamfer_kernel_keeps_its_instruction_mix_and_does_not_spill)


def synthetic_clouds(n, P, seed):
    """Points on random boxes, centred and scaled into the unit cube like the reference's normalize_pc."""
    g = np.random.default_rng(seed)
    half = g.uniform(0.15, 1.0, size=(n, 1, 3))
    pts = g.uniform(-1.0, 1.0, size=(n, P, 3)) * half
    face = g.integers(0, 3, size=(n, P))
    sign = np.where(g.random((n, P)) < 0.5, -1.0, 1.0)
    np.put_along_axis(pts, face[..., None], sign[..., None] * np.take_along_axis(np.broadcast_to(half, pts.shape), face[..., None], 2), 2)
    pts -= pts.mean(axis=1, keepdims=True)
    pts /= np.abs(pts).max(axis=(1, 2), keepdims=True)
    return torch.from_numpy(pts.astype(np.float32))


def eager_rows(sample_rows, ref, batch):
    """[rows, R] Chamfer values the way the reference computes them in torch: per sample cloud and batch of reference clouds."""
    out = []
    for x in sample_rows:
        row = []
        for r0 in range(0, ref.shape[0], batch):
            y = ref[r0:r0 + batch]
            xb = x.unsqueeze(0).expand(y.shape[0], -1, -1).contiguous()
            xx, yy, xy = torch.bmm(xb, xb.transpose(2, 1)), torch.bmm(y, y.transpose(2, 1)), torch.bmm(xb, y.transpose(2, 1))
            nx = torch.diagonal(xx, dim1=1, dim2=2).unsqueeze(2)
            ny = torch.diagonal(yy, dim1=1, dim2=2).unsqueeze(1)
            d = nx + ny - 2 * xy
            row.append(d.min(2).values.mean(1) + d.min(1).values.mean(1))
        out.append(torch.cat(row))
    return torch.stack(out)


def sensors(dev):
    """hwmon files of this device: package power and shader clock, in the sensor's unit / 1e6 (W, MHz)."""
    pr = torch.cuda.get_device_properties(dev)
    want = "%04x:%02x:%02x" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, getattr(pr, "pci_device_id", 0)) if hasattr(pr, "pci_bus_id") else None
    sens = {}
    for card in sorted(glob.glob("/sys/class/drm/card*")):
        if "-" in os.path.basename(card) or (want and want not in os.path.realpath(os.path.join(card, "device"))):
            continue
        for hw in glob.glob(os.path.join(card, "device", "hwmon", "hwmon*")):
            for key, names in (("W", ("power1_average", "power1_input")), ("MHz", ("freq1_input",))):
                for n in names:
                    if key not in sens and os.path.exists(os.path.join(hw, n)):
                        sens[key] = os.path.join(hw, n)

    def read(key):
        try:
            return int(open(sens[key]).read()) / 1e6
        except (KeyError, OSError, ValueError):
            return None
    return read


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=3000)
    ap.add_argument("--R", type=int, default=1000)
    ap.add_argument("--P", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--yardstick-rows", type=int, default=8)
    ap.add_argument("--ref-batch", type=int, default=64)
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--out", default=None, help="also write the record to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs the GPU: a CPU run measures nothing")
    from brepgen_amd import metrics
    dev = torch.device("cuda", torch.cuda.current_device())
    sample, ref = synthetic_clouds(args.S, args.P, 1).to(dev), synthetic_clouds(args.R, args.P, 2).to(dev)
    if args.single:
        out = metrics.pairwise_chamfer(sample, ref)
        torch.cuda.synchronize()
        print(json.dumps({"single_call": True, "S": args.S, "R": args.R, "P": args.P, "mean": float(out.mean())}))
        return

    read, samples, stop = sensors(dev), [], threading.Event()

    def poll():
        while not stop.is_set():
            samples.append((read("W"), read("MHz")))
            time.sleep(0.02)
    metrics.pairwise_chamfer(sample[:64], ref[:64])                      # code object, allocator
    _, out = event_ms(lambda: metrics.pairwise_chamfer(sample, ref))     # one full-size warm-up
    th = threading.Thread(target=poll)
    th.start()
    hip_ms = []
    for _ in range(max(5, args.repeats)):
        ms, again = event_ms(lambda: metrics.pairwise_chamfer(sample, ref))
        hip_ms.append(ms)
        assert torch.equal(out, again), "the matrix changed between two runs"
    stop.set()
    th.join()
    rows = min(args.yardstick_rows, args.S)
    with torch.no_grad():
        eager_rows(sample[:1], ref, args.ref_batch)                      # warm-up: rocBLAS picks its kernels
        torch.cuda.synchronize()
        eager_ms = []
        for _ in range(max(5, args.repeats)):
            ms, eager = event_ms(lambda: eager_rows(sample[:rows], ref, args.ref_batch))
            eager_ms.append(ms)
    med = lambda v: sorted(v)[len(v) // 2]
    hip_s, eager_s = med(hip_ms) / 1e3, med(eager_ms) / 1e3 * args.S / rows
    point_pairs = float(args.S) * args.R * args.P * args.P
    floor_s = point_pairs * LANE_OPS_PER_POINT_PAIR / (FP32_VECTOR_FLOPS / 2)
    rel = ((out[:rows] - eager).abs() / eager).max()
    tail = samples[len(samples) // 2:]
    rec = {"S": args.S, "R": args.R, "P": args.P, "device": torch.cuda.get_device_name(dev),
           "hip_pairwise_chamfer_s": round(hip_s, 5), "hip_all_repeats_ms": [round(v, 2) for v in hip_ms],
           "timing": "hipEvent pair around one bg_chamfer_pairwise call, one full-size warm-up, median of the repeats",
           "point_pairs": point_pairs, "point_pairs_per_s": point_pairs / hip_s,
           "lane_ops_per_point_pair": LANE_OPS_PER_POINT_PAIR, "fp32_vector_issue_floor_s": round(floor_s, 5),
           "fraction_of_fp32_vector_issue_floor": round(floor_s / hip_s, 4),
           "yardstick": f"torch-ROCm eager, the reference's formulation (3 bmm + expanded matrix + 2 min per batch of {args.ref_batch} reference "
                        f"clouds), timed on {rows} sample rows and scaled linearly by {args.S}/{rows}",
           "yardstick_rows_timed": rows, "yardstick_rows_ms": [round(v, 2) for v in eager_ms], "yardstick_scaled_s": round(eager_s, 3),
           "speedup_over_yardstick": round(eager_s / hip_s, 2),
           "max_relative_difference_hip_vs_yardstick_on_those_rows": float(rel),
           "power_W_second_half": med([p for p, _ in tail if p is not None]) if any(p is not None for p, _ in tail) else None,
           "shader_clock_MHz_second_half": med([f for _, f in tail if f is not None]) if any(f is not None for _, f in tail) else None}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
