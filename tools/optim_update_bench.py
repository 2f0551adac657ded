#!/usr/bin/env python
"""The update half of a trainer iteration at real size: the parameter set of a SurfZNet (the LDM trainers' setting: AdamW (0.95, 0.999),
wd 1e-6, max_norm 50) and of the surface AutoencoderKL (the VAE trainers': (0.9, 0.999), wd 1e-5, max_norm 5) with seeded gradients, as

    torch_foreach   clip_grad_norm_ + GradScaler.step + GradScaler.update with torch.optim.AdamW as torch builds it by default
    torch_fused     the same with AdamW(fused=True)
    hip_fused       brepgen_amd.optim: scaler.step(opt, max_norm) + scaler.update()       (three launches)
    hip_literal     brepgen_amd.optim: clip_grad_norm_ + scaler.step(opt) + scaler.update()  (five launches)

in one process, alternated: `--rounds` rounds, each timing `--iters` updates of every variant, every update between its own pair of
device events; before each update, outside the timed span, the variant's gradients are restored from a master copy (torch's variants
clip and unscale theirs in place, the literal HIP form clips in place), so every timed update of every variant sees the same values.
Reported per variant: the median round's ms per update, the spread of its rounds (min .. max), kernel launches per update (device
kernels torch.profiler records during one update; null where it gives none) and host synchronisations per update (the warnings
torch.cuda.set_sync_debug_mode("warn") raises during one update: one per call that makes the host wait for the device), and for the
HIP variants the bytes/s of the 32 B per parameter an update has to move (read g; read p, g, m, v; write p, m, v) next to the
6.3 TB/s a float4 copy reaches on the MI355X.

    python tools/optim_update_bench.py [--iters 40 --rounds 6 --warmup 10 --out profiles/r11/optim_update.json]
"""
import argparse
import json
import os
import sys
import warnings

import torch

from bench_common import med

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE_BYTES_PER_S = 6.3e12
BYTES_PER_PARAM = 32


def make_variant(kind, shapes, hyper, max_norm, seed):
    from brepgen_amd import optim
    g = torch.Generator(device="cuda").manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=g, device="cuda") * 0.02) for s in shapes]
    master = [torch.randn(p.shape, generator=g, device="cuda") * 64.0 for p in params]      # gradients of a loss scaled by 2^16
    for p, m in zip(params, master):
        p.grad = m.clone()
    grads = [p.grad for p in params]

    def restore():
        torch._foreach_copy_(grads, master)

    if kind.startswith("torch"):
        opt = torch.optim.AdamW(params, fused=(kind == "torch_fused") or None, **hyper)
        scaler = torch.amp.GradScaler("cuda")
        scaler.scale(torch.zeros((), device="cuda"))

        def update():
            torch.nn.utils.clip_grad_norm_(params, max_norm=max_norm)
            scaler.step(opt)
            scaler.update()
    else:
        opt = optim.AdamW(params, **hyper)
        scaler = optim.GradScaler()
        if kind == "hip_fused":
            def update():
                scaler.step(opt, max_norm=max_norm)
                scaler.update()
        else:
            def update():
                optim.clip_grad_norm_(params, max_norm)
                scaler.step(opt)
                scaler.update()
    return update, restore


def count_launches(update, restore):
    """Device kernels torch.profiler records during one update, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        restore()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            update()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        return len(kernels) or None
    except Exception as e:                                                                          # noqa: BLE001
        print(f"torch.profiler unavailable: {e!r}", file=sys.stderr)
        return None


def count_syncs(update, restore):
    """Calls of one update that make the host wait for the device, as torch's sync debug mode reports them (one warning each)."""
    restore()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            update()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum("synchroniz" in str(w.message).lower() for w in caught)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "optim_update.json"))
    args = ap.parse_args()
    import brepgen_amd as bga
    from brepgen_amd.pipeline import SURF_VAE_CFG
    workloads = {
        "SurfZNet": ([tuple(p.shape) for p in bga.SurfZNet(False).parameters()], dict(lr=5e-4, betas=(0.95, 0.999), eps=1e-8, weight_decay=1e-6), 50.0),
        "AutoencoderKL_surface": ([tuple(p.shape) for p in bga.AutoencoderKL(**SURF_VAE_CFG).parameters()],
                                  dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5), 5.0),
    }
    kinds = ("torch_foreach", "torch_fused", "hip_fused", "hip_literal")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters_per_round": args.iters, "rounds": args.rounds,
              "bytes_per_param": BYTES_PER_PARAM, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE_BYTES_PER_S, "workloads": {}}
    for name, (shapes, hyper, max_norm) in workloads.items():
        n_params = sum(int(torch.Size(s).numel()) for s in shapes)
        updates = {k: make_variant(k, shapes, hyper, max_norm, 1234) for k in kinds}
        for k in kinds:
            for _ in range(args.warmup):
                updates[k][1]()
                updates[k][0]()
        torch.cuda.synchronize()
        ms = {k: [] for k in kinds}
        for _ in range(args.rounds):
            for k in kinds:
                update, restore = updates[k]
                pairs = []
                for _ in range(args.iters):
                    restore()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    update()
                    b.record()
                    pairs.append((a, b))
                torch.cuda.synchronize()
                ms[k].append(sum(a.elapsed_time(b) for a, b in pairs) / args.iters)
        rows = {}
        for k in kinds:
            launches, syncs = count_launches(*updates[k]), count_syncs(*updates[k])
            m = med(ms[k])
            rows[k] = {"ms_per_update": round(m, 5), "rounds_min_ms": round(min(ms[k]), 5), "rounds_max_ms": round(max(ms[k]), 5),
                       "all_rounds_ms": [round(v, 5) for v in ms[k]], "launches_per_update": launches, "host_syncs_per_update": syncs}
            if k.startswith("hip"):
                bps = BYTES_PER_PARAM * n_params / (m * 1e-3)
                rows[k]["bytes_per_s"] = round(bps, 1)
                rows[k]["share_of_achievable_hbm"] = round(bps / HBM_ACHIEVABLE_BYTES_PER_S, 4)
        result["workloads"][name] = {"tensors": len(shapes), "parameters": n_params, "floor_ms_at_achievable_hbm": round(
            BYTES_PER_PARAM * n_params / HBM_ACHIEVABLE_BYTES_PER_S * 1e3, 5), "variants": rows}
        print(name, json.dumps(rows), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
