#!/usr/bin/env python
"""The VAEs' two resampling convolutions in training (csrc/conv_train.hip, brepgen_amd/conv.py: conv_down, conv_up) at the VAE trainers'
batch of 512 and the surface VAE's six shapes, bf16:
    conv_down (Downsample2D)  32 -> 16 x 128,  16 -> 8 x 256,  8 -> 4 x 512        (grid -> grid x channels, cin = cout)
    conv_up   (Upsample2D)     4 -> 8 x 512,   8 -> 16 x 512, 16 -> 32 x 256

Every case runs in a child process of its own under a time limit (a parent that never touches the device starts them one after another
and stops at the first that fails).  Per shape:
  (i)   `kernels`: bg_conv_wgrad_geom alone (fp32 output, auto split) against bg_conv_wgrad on a stride-1 problem of the same M, N, K
        (a of the OUTPUT grid) and against that launch a second time (the noise figure).  For conv_down also bg_conv_down_dgrad against
        the forward convolution of the same FLOPs -- bg_im2col (stride 2) + bg_gemm_bias_act_fwd as conv_down runs it, and that GEMM alone.
        Windows of `--launches` launches between one pair of device events, `--rounds` windows per candidate, candidates alternating; the
        median window's time per launch.
  (ii)  `op`: conv_down / conv_up forward + backward against stock torch (F.pad + stride-2 nn.Conv2d | F.interpolate + nn.Conv2d) under
        the same autocast in torch's default and in its channels_last memory format, and against the faster of the two a second time
        (`torch_again`: the spread); alternated, every call between its own device events.

    python tools/conv_resample_bench.py [--launches 20 --rounds 5 --warmup 2 --out profiles/r19/conv_resample_bench.json]
"""
import os
import sys

from bench_common import phases, train_bench_main, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = 512                                            # utils.get_args_vae's default
CASES = [("down", 32, 128), ("down", 16, 256), ("down", 8, 512), ("up", 4, 512), ("up", 8, 512), ("up", 16, 256)]     # (geometry, input grid side, channels)
MFMA_PEAK = 2.5e15


def kernel_rows(torch, geom, hw, C, launches, rounds, warmup):
    from brepgen_amd import _lib
    lib = _lib.load()
    F32, BF = _lib.BG_F32, _lib.BG_BF16
    bf, s_ = torch.bfloat16, torch.cuda.current_stream().cuda_stream
    p_ = lambda t: None if t is None else t.data_ptr()                                               # noqa: E731
    down = geom == "down"
    code = _lib.BG_CONV_DOWN2 if down else _lib.BG_CONV_UP2
    S, H, W, N = BATCH, hw, hw, C
    Ho = Wo = hw // 2 if down else 2 * hw
    M, K = S * Ho * Wo, 9 * C
    g = torch.Generator(device="cuda").manual_seed(hw + C)
    a32 = torch.randn(S * H * W, C, generator=g, device="cuda")
    a, dy = a32.to(bf), torch.randn(M, N, generator=g, device="cuda").to(bf)
    a_same = torch.randn(M, C, generator=g, device="cuda").to(bf)         # the stride-1 problem of the same M, N, K: a on the output grid
    dw, dw2, db = torch.empty(N, K, device="cuda"), torch.empty(N, K, device="cuda"), torch.empty(N, device="cuda")
    nb_g, nb_s = lib.bg_conv_wgrad_geom_workspace_bytes(S, H, W, N, C, 3, 3, code, 0), lib.bg_conv_wgrad_workspace_bytes(S, Ho, Wo, N, C, 3, 3, 0)
    ws_g, ws_s = torch.empty(max(nb_g, 16), dtype=torch.uint8, device="cuda"), torch.empty(max(nb_s, 16), dtype=torch.uint8, device="cuda")
    fns = {
        "wgrad_geom": lambda: lib.bg_conv_wgrad_geom(p_(dy), N, p_(a), C, p_(dw), p_(db), S, H, W, N, C, 3, 3, code, BF, F32, 0, p_(ws_g), nb_g, s_),
        "wgrad_same": lambda: lib.bg_conv_wgrad(p_(dy), N, p_(a_same), C, p_(dw2), p_(db), S, Ho, Wo, N, C, 3, 3, BF, F32, 0, p_(ws_s), nb_s, s_),
    }
    fns["wgrad_same_again"] = fns["wgrad_same"]
    if down:
        w = torch.randn(N, C, 3, 3, generator=g, device="cuda") / K ** 0.5
        w16, pack = torch.empty(N, K, dtype=bf, device="cuda"), torch.empty(9 * C * N, dtype=bf, device="cuda")
        _lib.check(lib.bg_conv_weight_pack_down(p_(w), F32, N, C, p_(w16), p_(pack), BF, s_), "bg_conv_weight_pack_down")
        dx, y, col = torch.empty(S * H * W, C, device="cuda"), torch.empty(M, N, device="cuda"), torch.empty(M, K, dtype=bf, device="cuda")
        nb_d = lib.bg_conv_down_dgrad_workspace_bytes(S, H, W, N, C)
        ws_d = torch.empty(nb_d, dtype=torch.uint8, device="cuda")
        im2col = lambda: lib.bg_im2col(p_(a32), p_(col), BF, S, H, W, C, 3, 3, 0, 2, 0, 0, Ho, Wo, None, None, None, 1, 0, None, s_)       # noqa: E731
        gemm = lambda: lib.bg_gemm_bias_act_fwd(p_(col), K, p_(w16), None, p_(y), N, M, N, N, K, BF, F32, 0, None, 0, 1, s_)             # noqa: E731
        fns["down_dgrad"] = lambda: lib.bg_conv_down_dgrad(p_(dy), N, p_(pack), p_(dx), S, H, W, N, C, BF, p_(ws_d), nb_d, s_)
        fns["fwd_im2col_gemm"] = lambda: im2col() or gemm()
        fns["fwd_gemm_alone"] = gemm
    for name, f in fns.items():
        _lib.check(f(), name)
    torch.cuda.synchronize()
    t = windows(torch, fns, launches, rounds, warmup)
    flop = 2.0 * M * N * K
    row = {"geom": geom, "grid": hw, "C": C, "M": M, "N": N, "K": K, "split": lib.bg_conv_wgrad_geom_split(S, H, W, N, C, 3, 3, code)}
    for k in fns:
        row[k] = {"ms": round(t[k], 5), "share_of_mfma_peak": round(flop / (t[k] * 1e-3) / MFMA_PEAK, 3)}
    row["geom_over_same"] = round(t["wgrad_geom"] / t["wgrad_same"], 4)
    row["spread_same_vs_itself"] = round(abs(t["wgrad_same"] - t["wgrad_same_again"]) / t["wgrad_same"], 4)
    if down:
        row["dgrad_over_fwd"] = round(t["down_dgrad"] / t["fwd_im2col_gemm"], 4)
        row["dgrad_over_fwd_gemm_alone"] = round(t["down_dgrad"] / t["fwd_gemm_alone"], 4)
    return row


def op_row(torch, geom, hw, C, rounds, warmup):
    import copy

    import torch.nn as nn
    import torch.nn.functional as F

    import brepgen_amd as bga

    down = geom == "down"

    class Sampler(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv2d(C, C, 3, stride=2) if down else nn.Conv2d(C, C, 3, padding=1)

        def forward(self, x):
            return self.conv(F.pad(x, (0, 1, 0, 1)) if down else F.interpolate(x, scale_factor=2.0, mode="nearest"))

    torch.manual_seed(hw)
    base = Sampler().cuda()
    dev = (bga.DeviceDownsample2D if down else bga.DeviceUpsample2D)(C).cuda()
    dev.load_state_dict(base.state_dict())
    models = {"torch": copy.deepcopy(base), "torch_channels_last": copy.deepcopy(base).to(memory_format=torch.channels_last), "device": dev}
    ho = hw // 2 if down else 2 * hw
    x = torch.randn(BATCH, C, hw, hw, device="cuda")
    g = torch.randn(BATCH, C, ho, ho, device="cuda")
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
    row = {"geom": geom, "grid": hw, "C": C, "batch": BATCH, "faster_torch_format": best}
    for k, v in tm.items():
        row[k] = {"fwd_ms": round(v[0], 3), "bwd_ms": round(v[1], 3), "total_ms": round(sum(v), 3)}
    row["spread_torch_vs_itself"] = round(abs(row[best]["total_ms"] - row["torch_again"]["total_ms"]) / row[best]["total_ms"], 4)
    row["device_over_torch"] = round(row["device"]["total_ms"] / row[best]["total_ms"], 4)
    return row


def child(what, geom, hw, C, args):
    import torch
    if what == "kernels":
        return [{"what": what, **kernel_rows(torch, geom, hw, C, args.launches, args.rounds, args.warmup)}]
    return [{"what": what, **op_row(torch, geom, hw, C, args.rounds, args.warmup)}]


def main():
    cases = [(what, geom, hw, C) for what in ("kernels", "op") for geom, hw, C in CASES]
    return train_bench_main(__file__, os.path.join(ROOT, "profiles", "r19", "conv_resample_bench.json"), cases, ("what", "geom", "grid", "C"), child,
                            lambda a: {"mfma_peak_flops": MFMA_PEAK, "batch": BATCH, "launches_per_window": a.launches, "rounds": a.rounds,
                                       "autocast": "bfloat16"}, launches=20)


if __name__ == "__main__":
    sys.exit(main())
