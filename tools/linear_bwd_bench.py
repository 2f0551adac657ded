#!/usr/bin/env python
"""The Linear layers' backward at the trainers' shapes: bg_linear_wgrad per forced split (the data behind the AUTO rule) and
brepgen_amd.linear.linear forward + backward next to torch's F.linear under autocast with fp32 parameters -- same GPU, same dtype,
same leaves.

    M = 512 x 30, 512 x 50, 256 x 50, 64 x 1500 tokens   x   in_proj (2304 x 768), out_proj (768 x 768), linear1 (1024 x 768),
    linear2 (768 x 1024)   x   fp16, bf16

Every M runs in a child process of its own under a time limit (a parent that never touches the device starts them one after another
and stops at the first that fails).  In a child the candidates alternate: `--rounds` rounds of `--iters` calls each, every call
between its own pair of device events on one stream; reported is the median round.
  * `wgrad_ms[S]`: bg_linear_wgrad alone (fp32 dW and db out) with split = S forced, and `auto` = what split = 0 resolves to;
  * `hip` / `torch`: forward and backward of the op under torch.autocast with fp32 weight and bias leaves and a 16-bit x leaf.  The
    torch figure includes its two weight casts, its dy.t() handling, its bias reduction and the cast of dW back to fp32 -- what the
    trainers run today; ours includes the two bg_weight_cast launches;
  * the wgrad's share of the nominal MFMA peak (2.5 PFLOP/s dense fp16 / bf16; 2 M N K FLOP) and the bytes it moves -- dy and x once,
    dW once, plus the fp32 partials written and read back when S > 1 -- against the 8 TB/s HBM stream rate DESIGN.md uses;
  * clocks and power as torch reports them after the timed window (or "not available").

    python tools/linear_bwd_bench.py [--iters 20 --rounds 5 --warmup 3 --out profiles/r14/linear_bwd_bench.json]
"""
import json
import os
import sys

from bench_common import device_state, phases, train_bench_main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOKENS = [512 * 30, 512 * 50, 256 * 50, 64 * 1500]
LAYERS = {"in_proj": (2304, 768), "out_proj": (768, 768), "linear1": (1024, 768), "linear2": (768, 1024)}
SPLITS = (1, 2, 4, 8, 16, 32)
MFMA_PEAK, HBM_RATE = 2.5e15, 8e12


def no_empty_slice(M, S, row_step=32):
    """bg_linear_wgrad's slicing rule (include/brepgen_hip.h): a forced split that leaves a slice empty is rejected"""
    steps = (M + row_step - 1) // row_step
    return (S - 1) * ((steps + S - 1) // S) * row_step < M


def child(M, iters, rounds, warmup):
    import torch
    import torch.nn.functional as F

    from brepgen_amd import _lib
    from brepgen_amd import linear as L
    lib = _lib.load()
    code = {torch.float16: _lib.BG_F16, torch.bfloat16: _lib.BG_BF16}
    stream = torch.cuda.current_stream().cuda_stream
    ev = lambda: torch.cuda.Event(enable_timing=True)                                                # noqa: E731
    rows = []
    for layer, (N, K) in LAYERS.items():
        for dtype in (torch.float16, torch.bfloat16):
            g = torch.Generator(device="cuda").manual_seed(M + N + K)
            x = torch.randn(M, K, generator=g, device="cuda").to(dtype)
            dy = torch.randn(M, N, generator=g, device="cuda").to(dtype)
            w = (torch.randn(N, K, generator=g, device="cuda") / K ** 0.5).requires_grad_(True)
            b = torch.randn(N, generator=g, device="cuda").requires_grad_(True)
            xl = x.clone().requires_grad_(True)
            dw = torch.empty(N, K, device="cuda")
            db = torch.empty(N, device="cuda")
            auto = lib.bg_linear_wgrad_split(M, N, K)
            ws = torch.empty(max(lib.bg_linear_wgrad_workspace_bytes(M, N, K, max(SPLITS)) // 4, 1), device="cuda")

            def wgrad(S, plain_walk=0):
                def call():
                    os.environ["BG_LINEAR_WGRAD_WALK"] = "plain" if plain_walk else "xcd"      # read by the library at every call
                    a, c = ev(), ev()
                    a.record()
                    _lib.check(lib.bg_linear_wgrad(dy.data_ptr(), N, x.data_ptr(), K, dw.data_ptr(), db.data_ptr(), M, N, K, code[dtype],
                                                   _lib.BG_F32, S, ws.data_ptr(), ws.numel() * 4, stream), "bg_linear_wgrad")
                    c.record()
                    return a, c
                return call

            splits = [S for S in SPLITS if no_empty_slice(M, S)]
            t_w = phases(torch, {str(S): wgrad(S) for S in splits}, iters, rounds, warmup)

            def fwd_bwd(fn):
                def call():
                    xl.grad = w.grad = b.grad = None
                    a, c, d = ev(), ev(), ev()
                    a.record()
                    with torch.autocast("cuda", dtype=dtype):
                        y = fn(xl, w, b)
                    c.record()
                    y.backward(dy)
                    d.record()
                    return a, c, d
                return call

            t_op = phases(torch, {"hip": fwd_bwd(L.linear), "torch": fwd_bwd(F.linear)}, iters, rounds, warmup, 2)
            state = device_state(torch)
            flop = 2.0 * M * N * K
            need = 2.0 * M * (N + K) + 4.0 * N * (K + 1)
            t_walk = phases(torch, {"xcd": wgrad(auto), "plain": wgrad(auto, 1)}, iters, rounds, warmup)
            os.environ.pop("BG_LINEAR_WGRAD_WALK", None)
            t_auto = t_walk["xcd"][0]
            best = min(splits, key=lambda S: t_w[str(S)][0])
            row = {"M": M, "layer": layer, "N": N, "K": K, "dtype": str(dtype)[6:],
                   "wgrad_ms": {S: round(v[0], 4) for S, v in t_w.items()}, "auto_split": auto, "wgrad_auto_ms": round(t_auto, 4),
                   "wgrad_auto_plain_walk_ms": round(t_walk["plain"][0], 4), "best_forced_split": best, "wgrad_auto_over_best": round(t_auto / t_w[str(best)][0], 3),
                   "wgrad_share_of_mfma_peak": round(flop / (t_auto * 1e-3) / MFMA_PEAK, 4),
                   "wgrad_bytes_needed": need, "wgrad_bytes_moved": need + (8.0 * auto * N * (K + 1) if auto > 1 else 0.0),
                   "device": state}
            row["wgrad_share_of_hbm_rate"] = round(row["wgrad_bytes_moved"] / (t_auto * 1e-3) / HBM_RATE, 4)
            for name in ("hip", "torch"):
                fw, bw = t_op[name]
                row[name] = {"fwd_ms": round(fw, 4), "bwd_ms": round(bw, 4), "total_ms": round(fw + bw, 4)}
            row["speedup_total"] = round(row["torch"]["total_ms"] / row["hip"]["total_ms"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    return train_bench_main(__file__, os.path.join(ROOT, "profiles", "r14", "linear_bwd_bench.json"), [(M,) for M in TOKENS], ("M",),
                            lambda M, a: child(M, a.iters, a.rounds, a.warmup),
                            lambda a: {"mfma_peak_flops": MFMA_PEAK, "hbm_stream_rate": HBM_RATE, "iters_per_round": a.iters, "rounds": a.rounds},
                            iters=20, warmup=3)


if __name__ == "__main__":
    sys.exit(main())
