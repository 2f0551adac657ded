#!/usr/bin/env python
"""The VAEs' ResnetBlock2D in training (csrc/conv_train.hip, brepgen_amd/conv.py) at the VAE trainers' batch of 512 and the surface
VAE's resnet shapes: 32 x 32 x 128, 16 x 16 x 256, 8 x 8 x 512, 4 x 4 x 512 (grid x channels, cin = cout).

Every shape runs in a child process of its own under a time limit (a parent that never touches the device starts them one after another
and stops at the first that fails).  Per shape, bf16:
  (i)   bg_conv_wgrad alone (fp32 output, auto split) against bg_linear_wgrad on a MATERIALISED im2col matrix of the same M, N, K (the
        matrix is written once, outside the timing) and against that launch a second time (the noise figure): windows of `--launches`
        launches between one pair of device events, `--rounds` windows per candidate, candidates alternating; the median window's time
        per launch, the ratio conv / linear, and 2 M N K FLOP per second as a share of the nominal 2.5 PFLOP/s bf16 MFMA peak.
  (ii)  bg_gn_act_bwd (SiLU, with dgamma / dbeta, with and without dskip): the bytes it must move -- pass 1 reads da and x, pass 2 reads
        them again (+ dskip) and writes dx: 20 (24) bytes per element, plus the fp64 partials -- per second as a share of the 6.3 TB/s
        streaming rate of the CDNA guide.
  (iii) one DeviceResnetBlock2D, forward + backward, against the torch block (nn.GroupNorm, nn.SiLU, nn.Conv2d) under the same autocast
        in torch's default and in its channels_last memory format, and against the faster of the two a second time (`torch_again`: the
        spread); alternated, every call between its own device events.

    python tools/conv_train_bench.py [--launches 20 --rounds 5 --warmup 2 --out profiles/r18/conv_train_bench.json]
"""
import os
import sys

from bench_common import phases, train_bench_main, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = 512                                            # utils.get_args_vae's default
CASES = [(32, 128), (16, 256), (8, 512), (4, 512)]     # (grid side, channels)
STREAM_RATE, MFMA_PEAK = 6.3e12, 2.5e15


def kernel_rows(torch, hw, C, launches, rounds, warmup):
    from brepgen_amd import _lib
    lib = _lib.load()
    F32, BF = _lib.BG_F32, _lib.BG_BF16
    bf, s_ = torch.bfloat16, torch.cuda.current_stream().cuda_stream
    p_ = lambda t: None if t is None else t.data_ptr()                                               # noqa: E731
    S, H, W, N, kh, kw = BATCH, hw, hw, C, 3, 3
    M, K = S * H * W, kh * kw * C
    g = torch.Generator(device="cuda").manual_seed(hw + C)
    a32 = torch.randn(M, C, generator=g, device="cuda")
    a, dy = a32.to(bf), torch.randn(M, N, generator=g, device="cuda").to(bf)
    col = torch.empty(M, K, dtype=bf, device="cuda")                     # the matrix the conv entry never writes
    _lib.check(lib.bg_im2col(p_(a32), p_(col), BF, S, H, W, C, kh, kw, 0, 1, 1, 1, H, W, None, None, None, 1, 0, None, s_), "bg_im2col")
    dw, dw2, db = torch.empty(N, K, device="cuda"), torch.empty(N, K, device="cuda"), torch.empty(N, device="cuda")
    nb_c, nb_l = lib.bg_conv_wgrad_workspace_bytes(S, H, W, N, C, kh, kw, 0), lib.bg_linear_wgrad_workspace_bytes(M, N, K, 0)
    ws_c, ws_l = torch.empty(max(nb_c, 16), dtype=torch.uint8, device="cuda"), torch.empty(max(nb_l, 16), dtype=torch.uint8, device="cuda")
    conv = lambda: lib.bg_conv_wgrad(p_(dy), N, p_(a), C, p_(dw), p_(db), S, H, W, N, C, kh, kw, BF, F32, 0, p_(ws_c), nb_c, s_)       # noqa: E731
    lin = lambda: lib.bg_linear_wgrad(p_(dy), N, p_(col), K, p_(dw2), p_(db), M, N, K, BF, F32, 0, p_(ws_l), nb_l, s_)                # noqa: E731
    # GroupNorm + SiLU backward
    x, da, dskip, dx = a32, torch.randn(M, C, generator=g, device="cuda"), torch.randn(M, C, generator=g, device="cuda"), torch.empty(M, C, device="cuda")
    gamma, beta, G = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), 32
    stats, dgm, dbt = torch.empty(S, G, 2, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    _lib.check(lib.bg_groupnorm_stats(p_(x), p_(stats), S, H * W, C, G, 1e-6, s_), "bg_groupnorm_stats")
    nb_g = lib.bg_gn_act_bwd_workspace_bytes(S, H * W, C, G)
    ws_g = torch.empty(nb_g, dtype=torch.uint8, device="cuda")
    gn = lambda sk: lib.bg_gn_act_bwd(p_(da), p_(x), p_(stats), p_(gamma), p_(beta), p_(sk), p_(dx), p_(dgm), p_(dbt), S, H * W, C, G, 1,      # noqa: E731
                                      p_(ws_g), nb_g, s_)
    fns = {"conv_wgrad": conv, "linear_wgrad_on_im2col": lin, "linear_wgrad_on_im2col_again": lin,
           "gn_act_bwd": lambda: gn(None), "gn_act_bwd_dskip": lambda: gn(dskip)}
    for name, f in fns.items():
        _lib.check(f(), name)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2), "bg_conv_wgrad and bg_linear_wgrad on the materialised matrix differ"     # same products, same order
    t = windows(torch, fns, launches, rounds, warmup)
    flop, elems = 2.0 * M * N * K, float(M) * C
    split = lib.bg_conv_wgrad_split(S, H, W, N, C, kh, kw)
    row = {"grid": hw, "C": C, "M": M, "N": N, "K": K, "split": split}
    for k in ("conv_wgrad", "linear_wgrad_on_im2col", "linear_wgrad_on_im2col_again"):
        row[k] = {"ms": round(t[k], 5), "share_of_mfma_peak": round(flop / (t[k] * 1e-3) / MFMA_PEAK, 3)}
    row["conv_over_linear"] = round(t["conv_wgrad"] / t["linear_wgrad_on_im2col"], 4)
    row["spread_linear_vs_itself"] = round(abs(t["linear_wgrad_on_im2col"] - t["linear_wgrad_on_im2col_again"]) / t["linear_wgrad_on_im2col"], 4)
    for k, per in (("gn_act_bwd", 20.0), ("gn_act_bwd_dskip", 24.0)):
        need = per * elems + 2.0 * nb_g
        row[k] = {"ms": round(t[k], 5), "bytes_needed": need, "share_of_stream_rate": round(need / (t[k] * 1e-3) / STREAM_RATE, 3)}
    return row


def block_row(torch, hw, C, rounds, warmup):
    import copy

    import torch.nn as nn

    import brepgen_amd as bga

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.norm1, self.conv1 = nn.GroupNorm(32, C, eps=1e-6), nn.Conv2d(C, C, 3, padding=1)
            self.norm2, self.conv2 = nn.GroupNorm(32, C, eps=1e-6), nn.Conv2d(C, C, 3, padding=1)
            self.nonlinearity = nn.SiLU()

        def forward(self, x):
            h = self.conv1(self.nonlinearity(self.norm1(x)))
            return x + self.conv2(self.nonlinearity(self.norm2(h)))

    torch.manual_seed(hw)
    base = Block().cuda()
    models = {"torch": copy.deepcopy(base), "torch_channels_last": copy.deepcopy(base).to(memory_format=torch.channels_last),
              "device": bga.use_device_resnets(nn.ModuleList([copy.deepcopy(base)]))[0]}
    x = torch.randn(BATCH, C, hw, hw, device="cuda")
    g = torch.randn(BATCH, C, hw, hw, device="cuda")
    inputs = {"torch": (x, g), "torch_channels_last": (x.contiguous(memory_format=torch.channels_last), g.contiguous(memory_format=torch.channels_last)),
              "device": (x.permute(0, 2, 3, 1).contiguous(), g.permute(0, 2, 3, 1).contiguous())}
    ev = lambda: torch.cuda.Event(enable_timing=True)                                              # noqa: E731

    def run(name):
        model = models[name]
        xin, gin = inputs[name]
        xin = xin.clone().requires_grad_()

        def call():
            model.zero_grad(set_to_none=True)
            xin.grad = None
            a, c, d = ev(), ev(), ev()
            a.record()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = model(xin)
            c.record()
            out.backward(gin)
            d.record()
            return a, c, d
        return call

    fns = {k: run(k) for k in models}
    first = phases(torch, fns, 2, 2, warmup, 2)                          # which torch format is faster here
    best = min(("torch", "torch_channels_last"), key=lambda k: sum(first[k]))
    models["torch_again"], inputs["torch_again"] = models[best], inputs[best]
    fns["torch_again"] = run("torch_again")
    tm = phases(torch, fns, 3, rounds, warmup, 2)
    row = {"grid": hw, "C": C, "batch": BATCH, "faster_torch_format": best}
    for k, v in tm.items():
        row[k] = {"fwd_ms": round(v[0], 3), "bwd_ms": round(v[1], 3), "total_ms": round(sum(v), 3)}
    row["spread_torch_vs_itself"] = round(abs(row[best]["total_ms"] - row["torch_again"]["total_ms"]) / row[best]["total_ms"], 4)
    row["device_over_torch"] = round(row["device"]["total_ms"] / row[best]["total_ms"], 4)
    return row


def child(what, hw, C, args):
    import torch
    if what == "kernels":
        return [{"what": what, **kernel_rows(torch, hw, C, args.launches, args.rounds, args.warmup)}]
    return [{"what": what, **block_row(torch, hw, C, args.rounds, args.warmup)}]


def main():
    cases = [(what, hw, C) for what in ("kernels", "block") for hw, C in CASES]
    return train_bench_main(__file__, os.path.join(ROOT, "profiles", "r18", "conv_train_bench.json"), cases, ("what", "grid", "C"), child,
                            lambda a: {"stream_rate_bytes_per_s": STREAM_RATE, "mfma_peak_flops": MFMA_PEAK, "batch": BATCH,
                                       "launches_per_window": a.launches, "rounds": a.rounds, "autocast": "bfloat16"}, launches=20)


if __name__ == "__main__":
    sys.exit(main())
