#!/usr/bin/env python
"""Two builds of libbrepgen_hip.so in ONE process (brepgen_amd/_ab_old.so = the previous commit's build, copied there by hand): the
training attention entries bg_attn_train_fwd / bg_attn_bwd of both on the same seeded operands.

  bits    out, lse and dqkv byte for byte: fp16 / bf16 x p in {0, 0.1} x masks {none, one_empty} x backward {general, short (N <= 64)}
          at (B, N) = (3, 5), (3, 33), (3, 64), (2, 130)
  speed   the trainers' shapes (tools/attn_bwd_bench.py): per round old / new / old back to back, medians of 5 rounds.  The two
          measurements of the OLD library against each other are the margin: new must not be slower than the slower of them.
          Judged are the rows that launch a kernel whose instruction stream differs from the previous commit's
          (profiles/r14/attn_tile_isa.json, written by the one-off compiler-output comparison); the others run the same code and
          are recorded only.

Every step (the bit cases, each timed shape) runs under its own alarm; nothing is retried.  Exit status 1 on a byte mismatch, 2 on a
shape outside its margin.     python tools/attn_train_ab_libs.py [--out profiles/r14/attn_tile_ab.json]"""
import argparse
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from brepgen_amd import _lib
from bench_common import old_library

ENTRIES = ("bg_attn_train_fwd", "bg_attn_bwd", "bg_attn_bwd_workspace_bytes")
DT = {torch.float16: _lib.BG_F16, torch.bfloat16: _lib.BG_BF16}
GENERAL, SHORT, AUTO = _lib.BG_ATTN_BWD_GENERAL, _lib.BG_ATTN_BWD_SHORT, _lib.BG_ATTN_BWD_AUTO
BIT_SHAPES = ((3, 5), (3, 33), (3, 64), (2, 130))
TIME_SHAPES = ((512, 30), (512, 50), (512, 64), (64, 1500))
SEED, DRAW = 0x5EED, 3


def operands(B, N, dtype, mask, seed):
    """qkv [B*N, 2304], dout [B*N, 768] (q, k scaled so that the scores 0.125 q.k spread over +-2), key_pad uint8 [B, N] or None:
    `tail` pads another length per sample, `one_empty` pads every key of the last sample as well."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * N, 2304, generator=g)
    qkv[:, :1536] *= 2.0 ** 0.5
    dout = torch.randn(B * N, 768, generator=g)
    kp = None
    if mask != "none":
        kp = torch.zeros(B, N, dtype=torch.uint8)
        for b in range(B):
            kp[b, max(1, (N * (b + 2)) // (B + 2)):] = 1
        if mask == "one_empty":
            kp[B - 1] = 1
        kp = kp.cuda()
    return qkv.to(dtype).cuda(), dout.to(dtype).cuda(), kp


class Call:
    """forward + backward of one library on fixed operands, into its own output buffers"""

    def __init__(self, lib, qkv, dout, kp, B, N, p, variant):
        self.lib, self.qkv, self.dout, self.kp, self.B, self.N, self.p, self.variant = lib, qkv, dout, kp, B, N, p, variant
        self.code = DT[qkv.dtype]
        self.out = torch.zeros(B * N, 768, dtype=qkv.dtype, device="cuda")
        self.lse = torch.zeros(B, 12, N, dtype=torch.float32, device="cuda")
        self.dqkv = torch.zeros(B * N, 2304, dtype=qkv.dtype, device="cuda")
        self.ws_bytes = lib.bg_attn_bwd_workspace_bytes(B, N, self.code)
        self.ws = torch.zeros(max(self.ws_bytes, 4) // 4, dtype=torch.float32, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream
        self.kpp = None if kp is None else kp.data_ptr()

    def fwd(self):
        rc = self.lib.bg_attn_train_fwd(self.qkv.data_ptr(), self.kpp, self.out.data_ptr(), self.lse.data_ptr(), self.B, self.N, self.code,
                                        0.125, self.p, SEED, DRAW, 0, self.st)
        assert rc == 0, rc

    def bwd(self):
        rc = self.lib.bg_attn_bwd(self.qkv.data_ptr(), self.kpp, self.lse.data_ptr(), self.dout.data_ptr(), self.dqkv.data_ptr(), self.B,
                                  self.N, self.code, 0.125, self.p, SEED, DRAW, 0, self.variant, self.ws.data_ptr(), self.ws_bytes, self.st)
        assert rc == 0, rc


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def bit_cases(old, new):
    rows = []
    for dtype in DT:
        for B, N in BIT_SHAPES:
            for mask in ("none", "one_empty"):
                for p in (0.0, 0.1):
                    for variant in (GENERAL, SHORT):
                        if variant == SHORT and N > 64:
                            continue
                        qkv, dout, kp = operands(B, N, dtype, mask, 100 * N + B)
                        co, cn = Call(old, qkv, dout, kp, B, N, p, variant), Call(new, qkv, dout, kp, B, N, p, variant)
                        for c in (co, cn):
                            c.fwd()
                            c.bwd()
                        torch.cuda.synchronize()
                        row = {"dtype": str(dtype)[6:], "B": B, "N": N, "mask": mask, "dropout_p": p,
                               "variant": "short" if variant == SHORT else "general",
                               "out": same_bytes(co.out, cn.out), "lse": same_bytes(co.lse, cn.lse), "dqkv": same_bytes(co.dqkv, cn.dqkv)}
                        rows.append(row)
                        print(json.dumps(row), flush=True)
    return rows


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                 # us per call


def launched(entry, N, f16, drop):
    """demangled names of the kernels an entry launches at this shape (csrc/attn_train.hip: bg_attn_train_fwd, bg_attn_bwd)"""
    a, b = str(f16).lower(), str(drop).lower()
    if entry == "fwd":
        return [f"void bg::at_fwd16_kernel<{a}, {b}>("]
    if entry == "bwd" and N <= 64:
        return [f"void bg::at_bwd16_short_kernel<{a}, {b}>("]
    return [f"void bg::at_bwd16_kernel<{a}, {b}, false>(", f"void bg::at_bwd16_kernel<{a}, {b}, true>("]


def time_shape(old, new, B, N, iters, rounds, window_us, isa):
    rows = []
    for dtype in DT:
        for p in (0.0, 0.1):
            qkv, dout, kp = operands(B, N, dtype, "tail", 7 * N + B)
            variants = [("bwd", AUTO)] + ([("bwd_general", GENERAL)] if N <= 64 else [])
            calls = {name: (Call(old, qkv, dout, kp, B, N, p, v), Call(new, qkv, dout, kp, B, N, p, v)) for name, v in variants}
            what = {"fwd": (calls["bwd"][0].fwd, calls["bwd"][1].fwd)}
            what.update({name: (co.bwd, cn.bwd) for name, (co, cn) in calls.items()})
            for co, cn in calls.values():                          # lse for the backward; warm-up of every kernel timed below
                for c in (co, cn):
                    for _ in range(3):
                        c.fwd()
                        c.bwd()
            torch.cuda.synchronize()
            for name, (fo, fn) in what.items():
                t = {"old_a": [], "new": [], "old_b": []}
                n = max(iters, min(400, int(window_us / timed(fo, 5)) + 1))      # a timed window lasts at least `window_us`
                for _ in range(rounds):
                    t["old_a"].append(timed(fo, n))
                    t["new"].append(timed(fn, n))
                    t["old_b"].append(timed(fo, n))
                m = {k: statistics.median(v) for k, v in t.items()}
                lo, hi = min(m["old_a"], m["old_b"]), max(m["old_a"], m["old_b"])
                changed = [k for k in launched(name, N, dtype == torch.float16, p > 0)
                           if not all(v["identical"] for full, v in isa.items() if full.startswith(k))]
                row = {"B": B, "N": N, "dtype": str(dtype)[6:], "dropout_p": p, "entry": name, "calls_per_window": n,
                       "kernels_changed": changed,
                       "old_a_us": round(m["old_a"], 2), "new_us": round(m["new"], 2), "old_b_us": round(m["old_b"], 2),
                       "new_over_old": round(m["new"] / lo, 4), "old_over_old": round(hi / lo, 4), "within_margin": m["new"] <= hi, "judged": bool(changed),
                       "rounds_us": {k: [round(x, 2) for x in v] for k, v in t.items()}}
                rows.append(row)
                print(json.dumps({k: v for k, v in row.items() if k != "rounds_us"}), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "attn_tile_ab.json"))
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window, at least")
    ap.add_argument("--window-us", type=float, default=10000.0, help="a timed window lasts at least this long (up to 400 calls)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--isa", default=os.path.join(ROOT, "profiles", "r14", "attn_tile_isa.json"), help="per-kernel compiler-output comparison")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds per step (SIGALRM ends the process)")
    args = ap.parse_args()
    with open(args.isa) as f:
        isa = json.load(f)["kernels"]
    new, old = _lib.load(), old_library(_lib._SIGNATURES, ENTRIES)
    res = {"device": torch.cuda.get_device_name(0), "min_calls_per_window": args.iters, "min_window_us": args.window_us, "rounds": args.rounds}
    signal.alarm(args.step_timeout)
    res["bits"] = bit_cases(old, new)
    res["timing"] = []
    for B, N in TIME_SHAPES:
        signal.alarm(args.step_timeout)
        res["timing"] += time_shape(old, new, B, N, args.iters, args.rounds, args.window_us, isa)
    signal.alarm(0)
    res["bits_identical"] = all(r["out"] and r["lse"] and r["dqkv"] for r in res["bits"])
    res["outside_margin"] = [{k: r[k] for k in ("B", "N", "dtype", "dropout_p", "entry")} for r in res["timing"] if r["judged"] and not r["within_margin"]]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"out": args.out, "bits_identical": res["bits_identical"], "outside_margin": len(res["outside_margin"])}))
    return 1 if not res["bits_identical"] else (2 if res["outside_margin"] else 0)


if __name__ == "__main__":
    sys.exit(main())
