#!/usr/bin/env python
"""The encoder-layer glue (csrc/layer_train.hip, brepgen_amd/layer.py) at the trainers' shapes.

    tokens = 512 x 30, 512 x 60, 64 x 1500 (B x N)   x   bf16 branches with an fp32 or a bf16 residual stream

Every token count runs in a child process of its own under a time limit (a parent that never touches the device starts them one after
another and stops at the first that fails).  In a child:
  * per kernel (`kernels`): each entry alone through the C ABI, windows of `--launches` launches between one pair of device events,
    `--rounds` windows per candidate, candidates alternating; reported are the median window's time per launch, the bytes the
    algorithm has to move (computed here from the shapes: every operand read once, every result written once, the fp64 partials of
    bg_ln_bwd written and read back), and those bytes per second as a share of the 6.3 TB/s streaming rate of the CDNA guide;
  * per op (`ops`): forward and backward of the autograd op next to the torch op sequence that does the same work under
    torch.autocast, alternated in the same process, every call between its own device events;
  * per encoder (`encoder`): forward + backward of a 12-layer nn.TransformerEncoder(768, 12, 1024, dropout 0.1, norm_first) under bf16
    autocast in the parent commit's configuration (use_device_attention + use_device_linear, torch for the rest: `parent`), the same
    configuration a second time (`parent_again`: the spread) and use_device_layer (`layer`), alternated.

    python tools/layer_train_bench.py [--launches 300 --rounds 5 --warmup 2 --out profiles/r15/layer_train_bench.json]
"""
import os
import sys

from bench_common import phases, train_bench_main, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(512, 30), (512, 60), (64, 1500)]          # (B, N)
STREAM_RATE = 6.3e12
P, SEED = 0.1, 77


def kernel_rows(torch, B, N, sdt, launches, rounds, warmup):
    from brepgen_amd import _lib
    lib = _lib.load()
    code = {torch.float32: _lib.BG_F32, torch.bfloat16: _lib.BG_BF16}
    bf, M, s = torch.bfloat16, B * N, torch.cuda.current_stream().cuda_stream
    ss = 4 if sdt == torch.float32 else 2
    g = torch.Generator(device="cuda").manual_seed(M)
    rnd = lambda c, dt: torch.randn(M, c, generator=g, device="cuda").to(dt)                       # noqa: E731
    x, dskip, skip, dout = rnd(768, sdt), rnd(768, sdt), rnd(768, sdt), rnd(768, sdt)
    dy, branch, x1, dh = rnd(768, bf), rnd(768, bf), rnd(1024, bf), rnd(1024, bf)
    gamma, beta = torch.ones(768, device="cuda"), torch.zeros(768, device="cuda")
    y, dx, out, dbr = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(skip), torch.empty_like(branch)
    h, dx1 = torch.empty_like(x1), torch.empty_like(x1)
    stats, dg, db = torch.empty(M, 2, device="cuda"), torch.empty(768, device="cuda"), torch.empty(768, device="cuda")
    nws = lib.bg_ln_bwd_workspace_bytes(M)
    ws = torch.empty(nws // 8, dtype=torch.float64, device="cuda")
    p_ = lambda t: t.data_ptr()                                                                    # noqa: E731
    key = (P, SEED, 5)
    fns = {
        "ln_train_fwd": lambda: lib.bg_ln_train_fwd(p_(x), code[sdt], p_(gamma), p_(beta), p_(y), code[bf], p_(stats), M, 1e-5, s),
        "ln_bwd": lambda: lib.bg_ln_bwd(p_(dy), code[bf], p_(x), code[sdt], p_(stats), p_(gamma), p_(dskip), p_(dx), p_(dg), p_(db), M, p_(ws), nws, s),
        "ln_bwd_dx_only": lambda: lib.bg_ln_bwd(p_(dy), code[bf], p_(x), code[sdt], p_(stats), p_(gamma), p_(dskip), p_(dx), None, None, M, None, 0, s),
        "dropout_add_fwd": lambda: lib.bg_dropout_add_fwd(p_(branch), code[bf], p_(skip), p_(out), code[sdt], M, 768, B, *key, 1, 0, s),
        "dropout_add_fwd_p0": lambda: lib.bg_dropout_add_fwd(p_(branch), code[bf], p_(skip), p_(out), code[sdt], M, 768, B, 0.0, SEED, 5, 1, 0, s),
        "dropout_bwd": lambda: lib.bg_dropout_bwd(p_(dout), code[sdt], p_(dbr), code[bf], M, 768, B, *key, 1, 0, s),
        "relu_dropout_fwd": lambda: lib.bg_relu_dropout_fwd(p_(x1), p_(h), code[bf], M, 1024, B, *key, 2, 0, s),
        "relu_dropout_fwd_p0": lambda: lib.bg_relu_dropout_fwd(p_(x1), p_(h), code[bf], M, 1024, B, 0.0, SEED, 5, 2, 0, s),
        "relu_dropout_bwd": lambda: lib.bg_relu_dropout_bwd(p_(h), p_(dh), p_(dx1), code[bf], M, 1024, P, s),
    }
    for name, f in fns.items():
        _lib.check(f(), name)
    e768, e1024 = float(M) * 768, float(M) * 1024
    need = {
        "ln_train_fwd": e768 * (ss + 2) + 8.0 * M + 2 * 768 * 4,
        "ln_bwd": e768 * (2 + 3 * ss) + 8.0 * M + 768 * 4 + 2.0 * nws + 2 * 768 * 4,
        "ln_bwd_dx_only": e768 * (2 + 3 * ss) + 8.0 * M + 768 * 4,
        "dropout_add_fwd": e768 * (2 + 2 * ss), "dropout_add_fwd_p0": e768 * (2 + 2 * ss),
        "dropout_bwd": e768 * (ss + 2),
        "relu_dropout_fwd": e1024 * 4, "relu_dropout_fwd_p0": e1024 * 4, "relu_dropout_bwd": e1024 * 6,
    }
    t = windows(torch, fns, launches, rounds, warmup)
    return [{"kernel": k, "ms": round(t[k], 5), "bytes_needed": need[k], "tb_per_s": round(need[k] / (t[k] * 1e-3) / 1e12, 3),
             "share_of_stream_rate": round(need[k] / (t[k] * 1e-3) / STREAM_RATE, 3)} for k in fns]


def op_rows(torch, B, N, sdt, iters, rounds, warmup):
    import torch.nn.functional as F

    from brepgen_amd import layer as L
    bf, M = torch.bfloat16, B * N
    g = torch.Generator(device="cuda").manual_seed(M + 1)
    rnd = lambda c, dt: torch.randn(N, B, c, generator=g, device="cuda").to(dt)                    # noqa: E731
    xl, skl = rnd(768, sdt).requires_grad_(True), rnd(768, sdt).requires_grad_(True)
    brl, x1l = rnd(768, bf).requires_grad_(True), rnd(1024, bf).requires_grad_(True)
    dy, dskip, dout, dh = rnd(768, bf), rnd(768, sdt), rnd(768, sdt), rnd(1024, bf)
    w, b = torch.ones(768, device="cuda", requires_grad=True), torch.zeros(768, device="cuda", requires_grad=True)
    ev = lambda: torch.cuda.Event(enable_timing=True)                                              # noqa: E731

    def run(fwd, leaves, grads):
        def call():
            for t in leaves:
                t.grad = None
            a, c, d = ev(), ev(), ev()
            a.record()
            with torch.autocast("cuda", dtype=bf):
                outs = fwd()
            c.record()
            torch.autograd.backward(list(outs), list(grads))
            d.record()
            return a, c, d
        return call

    def torch_ln():
        return F.layer_norm(xl, (768,), w, b).to(bf), xl.view_as(xl)

    cases = {
        "layer_norm+skip": (lambda: L.layer_norm(xl, w, b, return_skip=True), torch_ln, (xl, w, b), (dy, dskip)),
        "dropout_add": (lambda: (L.dropout_add(brl, skl, P, True, seed=SEED, draw_id=5),),
                        lambda: (skl + F.dropout(brl, P, True),), (brl, skl), (dout,)),
        "relu_dropout": (lambda: (L.relu_dropout(x1l, P, True, seed=SEED, draw_id=5),),
                         lambda: (F.dropout(F.relu(x1l), P, True),), (x1l,), (dh,)),
    }
    rows = []
    for name, (ours, theirs, leaves, grads) in cases.items():
        t = phases(torch, {"hip": run(ours, leaves, grads), "torch": run(theirs, leaves, grads)}, iters, rounds, warmup, 2)
        row = {"op": name}
        for k in ("hip", "torch"):
            row[k] = {"fwd_ms": round(t[k][0], 4), "bwd_ms": round(t[k][1], 4), "total_ms": round(sum(t[k]), 4)}
        row["speedup_total"] = round(row["torch"]["total_ms"] / row["hip"]["total_ms"], 3)
        rows.append(row)
    return rows


def encoder_row(torch, B, N, iters, rounds, warmup):
    import copy

    import torch.nn as nn

    import brepgen_amd as bga
    torch.manual_seed(N)
    base = nn.TransformerEncoder(nn.TransformerEncoderLayer(768, 12, 1024, dropout=P, norm_first=True), 12, norm=nn.LayerNorm(768),
                                 enable_nested_tensor=False).cuda().train()
    encs = {"parent": bga.use_device_linear(bga.use_device_attention(copy.deepcopy(base), seed=SEED)),
            "parent_again": bga.use_device_linear(bga.use_device_attention(copy.deepcopy(base), seed=SEED)),
            "layer": bga.use_device_layer(copy.deepcopy(base), seed=SEED)}
    x = torch.randn(N, B, 768, device="cuda")
    gout = torch.randn(N, B, 768, device="cuda")
    mask = torch.zeros(B, N, dtype=torch.bool, device="cuda")
    mask[:, N - N // 5:] = True
    ev = lambda: torch.cuda.Event(enable_timing=True)                                              # noqa: E731

    def run(enc):
        def call():
            enc.zero_grad(set_to_none=True)
            a, c, d = ev(), ev(), ev()
            a.record()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = enc(x, src_key_padding_mask=mask)
            c.record()
            out.backward(gout.to(out.dtype))
            d.record()
            return a, c, d
        return call

    t = phases(torch, {k: run(e) for k, e in encs.items()}, iters, rounds, warmup, 2)
    row = {k: {"fwd_ms": round(v[0], 3), "bwd_ms": round(v[1], 3), "total_ms": round(sum(v), 3)} for k, v in t.items()}
    row["spread_parent_vs_itself"] = round(abs(row["parent"]["total_ms"] - row["parent_again"]["total_ms"]) / row["parent"]["total_ms"], 4)
    row["layer_over_parent"] = round(row["layer"]["total_ms"] / row["parent"]["total_ms"], 4)
    return row


def child(B, N, args):
    import torch
    out = {"B": B, "N": N, "tokens": B * N, "streams": {}}
    for sdt in (torch.float32, torch.bfloat16):
        out["streams"][str(sdt)[6:]] = {"kernels": kernel_rows(torch, B, N, sdt, args.launches, args.rounds, args.warmup),
                                        "ops": op_rows(torch, B, N, sdt, 20, args.rounds, args.warmup)}
    out["encoder"] = encoder_row(torch, B, N, 3, args.rounds, args.warmup)
    return out


def main():
    return train_bench_main(__file__, os.path.join(ROOT, "profiles", "r15", "layer_train_bench.json"), SHAPES, ("B", "N"),
                            lambda B, N, args: [child(B, N, args)],
                            lambda a: {"stream_rate_bytes_per_s": STREAM_RATE, "launches_per_window": a.launches, "rounds": a.rounds,
                                       "dropout_p": P}, launches=300)


if __name__ == "__main__":
    sys.exit(main())
