#!/usr/bin/env python
"""Forward + backward of the attention core at the trainers' shapes: brepgen_amd.self_attention (csrc/attn_train.hip) next to
torch's F.scaled_dot_product_attention, same GPU, same dtype, same packed qkv leaf, same ragged key-padding mask (~70 % fill), same
dropout probability.

    (B, N) = (512, 30), (512, 50), (512, 64)   the face trainers (max_face = 50)      (64, 1500)   the edge trainers' bound (50 x 30)
    fp16 and bf16, p = 0 and p = 0.1

Every shape runs in a child process of its own under a time limit (a parent that never touches the device starts them one after
another and stops at the first that fails).  In a child the two implementations alternate: `--rounds` rounds of `--iters` calls each,
every call (forward, backward) between its own pair of device events; reported is the median round.
  * `hip` is the op as shipped (N <= 64: the one-launch short-sequence backward), `hip_general` the same with the general two-launch
    backward forced (N <= 64 only: the A/B that decides which one BG_ATTN_BWD_AUTO takes);
  * `torch` slices the packed leaf into strided q / k / v views and builds the boolean attn_mask on every call, as nn.MultiheadAttention
    does, so its backward includes the three slice-backward zero-fills and adds over [B, N, 2304]; `torch_split` starts from pre-split
    contiguous [B, 12, N, 64] leaves and a prebuilt mask: the attention kernels alone;
  * TFLOP/s of the backward against the nominal MFMA peak (2.5 PFLOP/s dense fp16 / bf16): with the TWELVE products the two kernels
    execute (S and dP three times -- the dQ kernel's delta walk, its second walk, the dK/dV kernel --, and dQ, dK, dV twice each: dS
    and P~ enter as hi + lo pairs) and with the FIVE of the algorithm; one product = 2 B 12 N^2 64;
  * bytes: what this op has to move (forward: qkv in, out out; dQ kernel: qkv and dout in, dq out; dK/dV kernel: qkv and dout in, dk
    and dv out; lse and delta are small) and, where torch picked its math backend, an estimate of that path's traffic: the same plus every pass over a [B, 12, N, N] tensor (10 without dropout, 16 with);
  * which backend torch picked (torch._fused_sdp_choice).

    python tools/attn_bwd_bench.py [--iters 20 --rounds 5 --warmup 5 --out profiles/r13/attn_bwd_bench.json]
"""
import json
import os
import sys

from bench_common import med, phases, train_bench_main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(512, 30), (512, 50), (512, 64), (64, 1500)]
MFMA_PEAK = 2.5e15
H, DH, D = 12, 64, 768


def child(B, N, iters, rounds, warmup):
    import torch
    import torch.nn.functional as F

    import brepgen_amd as bga
    from brepgen_amd import _lib, attention
    g = torch.Generator(device="cuda").manual_seed(1000 * B + N)
    lens = (torch.rand(B, generator=g, device="cuda") * 0.6 + 0.4) * N
    kpm = torch.arange(N, device="cuda")[None, :] >= lens.ceil().clamp(1, N)[:, None]
    rows = []
    for dtype in (torch.float16, torch.bfloat16):
        qkv = torch.randn(B, N, 3 * D, generator=g, device="cuda")
        qkv[..., :2 * D] *= 2.0 ** 0.5
        qkv = qkv.to(dtype).requires_grad_(True)
        dout = torch.randn(B, N, D, generator=g, device="cuda").to(dtype)
        for p in (0.0, 0.1):
            def ours():
                attention.BACKWARD_VARIANT = _lib.BG_ATTN_BWD_AUTO
                return bga.self_attention(qkv, kpm, p, True, 0.125, seed=7, draw_id=1)

            def ours_general():
                attention.BACKWARD_VARIANT = _lib.BG_ATTN_BWD_GENERAL
                return bga.self_attention(qkv, kpm, p, True, 0.125, seed=7, draw_id=1)

            am = ~kpm[:, None, None, :]
            qs, ks_, vs = (qkv.detach()[..., i * D:(i + 1) * D].reshape(B, N, H, DH).transpose(1, 2).contiguous().requires_grad_(True)
                           for i in range(3))
            dout_s = dout.reshape(B, N, H, DH).transpose(1, 2).contiguous()

            def theirs_split():
                return F.scaled_dot_product_attention(qs, ks_, vs, attn_mask=am, dropout_p=p, scale=0.125)

            def theirs():
                q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(B, N, H, DH).transpose(1, 2) for i in range(3))
                o = F.scaled_dot_product_attention(q, k, v, attn_mask=~kpm[:, None, None, :], dropout_p=p, scale=0.125)
                return o.transpose(1, 2).reshape(B, N, D)

            try:
                q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(B, N, H, DH).transpose(1, 2) for i in range(3))
                backend = int(torch._fused_sdp_choice(q, k, v, ~kpm[:, None, None, :], p, False))
                backend = {0: "math", 1: "flash", 2: "efficient", 3: "cudnn"}.get(backend, str(backend))
            except Exception as e:                                                                  # noqa: BLE001
                backend = f"unknown ({e!r})"
            fns = {"hip": ours, "torch": theirs, "torch_split": theirs_split}
            if N <= 64:
                fns["hip_general"] = ours_general
            grad_of = {name: (dout_s if name == "torch_split" else dout) for name in fns}

            def fwd_bwd(name, f):
                def call():
                    qkv.grad = qs.grad = ks_.grad = vs.grad = None
                    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                    a.record()
                    o = f()
                    b.record()
                    o.backward(grad_of[name])
                    c.record()
                    return a, b, c
                return call

            ms = phases(torch, {name: fwd_bwd(name, f) for name, f in fns.items()}, iters, rounds, warmup, 2, all_rounds=True)
            gemm = 2.0 * B * H * N * N * DH
            es = 2
            row_bytes = B * N * D * es
            ours_bytes = (3 + 1) * row_bytes + (3 + 1 + 1) * row_bytes + (3 + 1 + 2) * row_bytes           # forward; dQ kernel; dK/dV kernel
            nn_pass = B * H * N * N * es
            row = {"B": B, "N": N, "dtype": str(dtype)[6:], "dropout_p": p, "torch_backend": backend,
                   "mask_fill": round(float((~kpm).float().mean()), 3)}
            for name in fns:
                fw, bw = med(ms[name][0]), med(ms[name][1])
                row[name] = {"fwd_ms": round(fw, 4), "bwd_ms": round(bw, 4), "total_ms": round(fw + bw, 4),
                             "bwd_rounds_ms": [round(x, 4) for x in ms[name][1]]}
            bw = row["hip"]["bwd_ms"] * 1e-3
            n_exec = 8 if N <= 64 else 12              # short kernel: S, dP once, dQ / dK / dV twice each (hi + lo); general: see above
            row["hip"].update({"bwd_products_executed": n_exec, "bwd_tflops_executed": round(n_exec * gemm / bw / 1e12, 2),
                               "bwd_tflops_algorithmic_5": round(5 * gemm / bw / 1e12, 2),
                               "bwd_share_of_mfma_peak_executed": round(n_exec * gemm / bw / MFMA_PEAK, 4),
                               "bytes_needed": ours_bytes})
            if backend == "math":
                row["torch"]["bytes_estimated"] = ours_bytes + (16 if p > 0 else 10) * nn_pass
            row["speedup_total"] = round(row["torch"]["total_ms"] / row["hip"]["total_ms"], 3)
            row["speedup_total_vs_torch_split"] = round(row["torch_split"]["total_ms"] / row["hip"]["total_ms"], 3)
            attention.BACKWARD_VARIANT = _lib.BG_ATTN_BWD_AUTO
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    return train_bench_main(__file__, os.path.join(ROOT, "profiles", "r13", "attn_bwd_bench.json"), SHAPES, ("B", "N"),
                            lambda B, N, a: child(B, N, a.iters, a.rounds, a.warmup),
                            lambda a: {"mfma_peak_flops": MFMA_PEAK, "iters_per_round": a.iters, "rounds": a.rounds},
                            iters=20, warmup=5, timeout=300)


if __name__ == "__main__":
    sys.exit(main())
