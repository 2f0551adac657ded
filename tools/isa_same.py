"""Are the device kernels of two builds the same kernels?  A CPU tool for pull requests that move host code only.

    python -m brepgen_amd.build --force --save-temps        (in the old tree and in the new tree)
    python tools/isa_same.py OLD/brepgen_amd/_build NEW/brepgen_amd/_build [--out FILE.json]

Of every `*-hip-amdgcn-amd-amdhsa-gfx950.s` the `.file` / `.ident` / comment lines, the `__hip_cuid_*` hash and the function ordinal in
`.LBB<n>_` / `.Lfunc_end<n>` labels are dropped; the text is split at symbol labels, and the symbols with their instruction text and
the entries of `amdhsa.kernels` (registers, kernarg offsets) are compared as SETS per translation unit, so another emission order of
the kernels within a unit is no difference.  Nothing is asked about WHICH instructions occur: text is only tested for equality.
Prints one line per unit that differs and a JSON summary; the exit status and `main`'s return value are the number of differences.
"""
import argparse
import json
import os
import re
import sys

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")                    # a symbol label (local .L labels start with a dot and stay in the text)


def _clean(line):
    line = line.split(";", 1)[0].rstrip()                         # comments (no string operand of these files holds a ';')
    line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", line)
    return re.sub(r"\.(LBB|Lfunc_(?:begin|end))\d+", r".\1", line)


def unit(path):
    """(symbols, kernels): {symbol: its text} and the set of `amdhsa.kernels` entries of one assembly file"""
    lines = []
    with open(path) as fh:
        for raw in fh:
            line = _clean(raw)
            if line.strip() and not line.lstrip().startswith((".file", ".ident")):
                lines.append(line)
    meta = lines.index("amdhsa.kernels:") if "amdhsa.kernels:" in lines else len(lines)
    symbols, name = {}, ""
    for line in lines[:meta]:
        m = LABEL.match(line)
        if m:
            name = m.group(1)
        symbols.setdefault(name, []).append(line)
    kernels, entry = set(), []
    for line in lines[meta + 1:]:
        if not line.startswith("  "):                             # the next top-level key of the metadata ends the list
            break
        if line.startswith("  - ") and entry:
            kernels.add("\n".join(entry))
            entry = []
        entry.append(line)
    if entry:
        kernels.add("\n".join(entry))
    return {k: "\n".join(v) for k, v in symbols.items()}, kernels


def compare(old_dir, new_dir):
    """{"units", "symbols", "kernels", "differences", "differing": {unit: [what differs]}} of two _build directories"""
    old = {f[:-len(SUFFIX)] for f in os.listdir(old_dir) if f.endswith(SUFFIX)}
    new = {f[:-len(SUFFIX)] for f in os.listdir(new_dir) if f.endswith(SUFFIX)}
    out = {"units": len(old | new), "symbols": 0, "kernels": 0, "differences": 0, "differing": {}}
    for u in sorted(old | new):
        if u not in old or u not in new:
            diffs = ["unit only in the " + ("new" if u in new else "old") + " build"]
        else:
            (so, ko), (sn, kn) = unit(os.path.join(old_dir, u + SUFFIX)), unit(os.path.join(new_dir, u + SUFFIX))
            out["symbols"] += len(sn)
            out["kernels"] += len(kn)
            diffs = [f"symbol {s}: " + ("text differs" if s in so and s in sn else "only in the " + ("new" if s in sn else "old") + " build")
                     for s in sorted(set(so) | set(sn)) if so.get(s) != sn.get(s)]
            if ko != kn:
                diffs.append(f"amdhsa.kernels: {len(ko ^ kn)} entries differ")
        if diffs:
            out["differing"][u] = diffs
            out["differences"] += len(diffs)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_build")
    ap.add_argument("new_build")
    ap.add_argument("--out", help="also write the summary to this JSON file")
    args = ap.parse_args(argv)
    res = compare(args.old_build, args.new_build)
    for u, diffs in res["differing"].items():
        for d in diffs:
            print(f"{u}: {d}")
    print(json.dumps({k: res[k] for k in ("units", "symbols", "kernels", "differences")}))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    return res["differences"]


if __name__ == "__main__":
    sys.exit(min(main(), 255))
