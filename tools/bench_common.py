"""What the bench tools share: the median, the two alternated device-event timers, the old build of a two-library A/B, the device's state, the parent loop that runs
one time-limited child process per shape, and the command line of the training benches around it.  Imports neither torch nor the
package: the parent of a bench never touches the device."""
import argparse
import json
import os
import subprocess
import sys


def med(v):
    return sorted(v)[len(v) // 2]


def windows(torch, fns, launches, rounds, warmup):
    """{name: median ms per launch}: fns[name]() enqueues one launch; `launches` of them between one pair of device events"""
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for name, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                f()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / launches)
    return {k: med(v) for k, v in ms.items()}


def phases(torch, fns, iters, rounds, warmup, n=1, all_rounds=False):
    """{name: [median ms per phase]}: fns[name]() runs one call and returns the n + 1 events it recorded; the candidates alternate round
    by round.  all_rounds: every round's figure per phase instead of the median."""
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ms = {k: [[] for _ in range(n)] for k in fns}
    for _ in range(rounds):
        for name, f in fns.items():
            evs = [f() for _ in range(iters)]
            torch.cuda.synchronize()
            for p in range(n):
                ms[name][p].append(sum(e[p].elapsed_time(e[p + 1]) for e in evs) / iters)
    return ms if all_rounds else {k: [med(v) for v in per] for k, per in ms.items()}


def old_library(signatures, entries):
    """The two-library A/B tools' second library: brepgen_amd/_ab_old.so (the previous commit's build, copied there by hand) with the
    signatures of `entries` taken from `signatures` (the binding's table, brepgen_amd/_lib.py _SIGNATURES)."""
    import ctypes
    old = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "brepgen_amd", "_ab_old.so"))
    for name in entries:
        fn = getattr(old, name)
        fn.restype, fn.argtypes = signatures[name]
    return old


def device_state(torch):
    out = {}
    for key, fn in (("clock_mhz", "clock_rate"), ("power_draw", "power_draw"), ("temperature_c", "temperature")):
        try:
            out[key] = int(getattr(torch.cuda, fn)())
        except Exception as e:                                                                      # noqa: BLE001
            out[key] = f"not available ({type(e).__name__})"
    return out


def run_children(script, shapes, names, options, timeout, out, head):
    """The parent of a bench: `script --child <shape> <options>` once per shape, each a fresh process under `timeout` seconds, one
    after another; a child prints its rows as "ROWS <json list>".  Nothing more is started on the device after a failure.  Writes
    {**head, "rows", "failed"} to `out`; -> the exit status.  names: the keys of a shape in the failure record."""
    rows, failed = [], None
    for shape in shapes:
        cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(script), "--child", *map(str, shape), *map(str, options)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")]
        if r.returncode != 0 or not got:
            failed = {**dict(zip(names, shape)), "returncode": r.returncode, "stderr": r.stderr[-2000:]}
            print(json.dumps(failed), file=sys.stderr)
            break
        new = json.loads(got[0][5:])
        rows += new
        for row in new:
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({**head, "rows": rows, "failed": failed}, f, indent=1)
    print(json.dumps({"out": out, "rows": len(rows), "failed": failed is not None}))
    return 1 if failed else 0


def train_bench_main(script, out, shapes, names, child, head, launches=None, iters=None, warmup=2, timeout=240):
    """The command line of a training bench: --launches (per timed window) or --iters (per round), whichever default is given,
    --rounds, --warmup, --timeout (seconds per child), --out, and the hidden `--child <shape>` hand-off.  As a child: child(*shape,
    args) -> the shape's rows (a shape's numbers arrive as ints), printed as the ROWS line.  Otherwise `run_children` over `shapes`
    with head(args) as the head of the JSON file.  -> the exit status."""
    window = "iters" if launches is None else "launches"
    ap = argparse.ArgumentParser()
    ap.add_argument("--" + window, type=int, default=iters if launches is None else launches,
                    help=None if launches is None else "launches per timed window (per kernel)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--timeout", type=int, default=timeout, help="seconds per case (child process)")
    ap.add_argument("--out", default=out)
    ap.add_argument("--child", nargs=len(names), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        shape = [int(v) if v.lstrip("-").isdigit() else v for v in args.child]
        print("ROWS " + json.dumps(child(*shape, args)))
        return 0
    options = ("--" + window, getattr(args, window), "--rounds", args.rounds, "--warmup", args.warmup)
    return run_children(script, shapes, names, options, args.timeout, args.out, head(args))
