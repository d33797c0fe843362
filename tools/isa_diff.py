#!/usr/bin/env python3
"""tools/isa_diff.py <parent.s> <branch.s> [--json out.json [--brief]]: do two gfx950 device listings hold
the same kernels? (hipcc --offload-arch=gfx950 -O3 -std=c++20 -fPIC -x hip -I include
--cuda-device-only -S unit.hip). With two directories: every <name>.s found in both.

Per kernel symbol it compares the metadata (.vgpr_count, .sgpr_count, .vgpr_spill_count,
.sgpr_spill_count, .private_segment_fixed_size, .group_segment_fixed_size = static LDS), the
instruction count and the per-opcode histogram. Listing text is not compared: register numbers
and the place of a few moves differ between any two compiles of refactored source, and the
__hip_cuid_* lines between any two compiles at all. Every opcode counts alike; only differences
are reported. Exit status 1 if any kernel differs. ISA study only."""
import collections
import json
import os
import re
import sys

META = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size")


def parse(path):
    """{kernel symbol: {"meta": {...}, "insts": n, "ops": Counter}}"""
    lines = open(path).read().split("\n")
    meta = {}
    cur = {}
    for ln in lines:  # the amdhsa.kernels note: one "- .agpr_count:" block per kernel
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)\s*$", ln)
        if not m:
            continue
        if ln.lstrip().startswith("- .agpr_count"):
            cur = {}
        cur[m.group(1)] = m.group(2)
        if m.group(1) == "name":
            meta[m.group(2)] = cur
    out = {}
    body = None
    for ln in lines:
        m = re.match(r"(\w+):", ln)
        if m and m.group(1) in meta:
            body = collections.Counter()
            out[m.group(1)] = {"meta": {k: int(meta[m.group(1)][k]) for k in META}, "ops": body}
            continue
        if body is None:
            continue
        if ln.startswith(".Lfunc_end"):
            body = None
            continue
        m = re.match(r"\t([a-z]\w*)", ln)  # an instruction: tab, opcode (directives start with '.')
        if m:
            body[m.group(1)] += 1
    for k in out.values():
        k["insts"] = sum(k["ops"].values())
    return out


def diff(a_path, b_path):
    a, b = parse(a_path), parse(b_path)
    res = {"kernels": len(a), "equal": 0, "differences": []}
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            res["differences"].append({"kernel": name, "only_in": "parent" if name in a else "branch"})
            continue
        d = {}
        for k in META:
            if a[name]["meta"][k] != b[name]["meta"][k]:
                d[k] = [a[name]["meta"][k], b[name]["meta"][k]]
        if a[name]["insts"] != b[name]["insts"]:
            d["insts"] = [a[name]["insts"], b[name]["insts"]]
        ops = {o: [a[name]["ops"][o], b[name]["ops"][o]] for o in sorted(set(a[name]["ops"]) | set(b[name]["ops"]))
               if a[name]["ops"][o] != b[name]["ops"][o]}
        if ops:
            d["ops"] = ops
        if d:
            res["differences"].append({"kernel": name, **d})
        else:
            res["equal"] += 1
    res["insts"] = sum(k["insts"] for k in b.values())
    return res


def main():
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    if out:
        args.remove(out)
    pa, pb = args
    if os.path.isdir(pa):
        names = sorted(n for n in os.listdir(pa) if n.endswith(".s") and os.path.exists(os.path.join(pb, n)))
        res = {n[:-2]: diff(os.path.join(pa, n), os.path.join(pb, n)) for n in names}
    else:
        res = {os.path.basename(pb)[:-2]: diff(pa, pb)}
    txt = json.dumps(res, indent=1)
    if "--brief" in sys.argv:  # a file to commit: no opcode histograms, one line per differing kernel
        units = []
        for unit, r in res.items():
            head = json.dumps({k: v for k, v in r.items() if k != "differences"})[:-1]
            diffs = ",\n".join("   " + json.dumps({k: v for k, v in d.items() if k != "ops"}) for d in r["differences"])
            units.append(f' {json.dumps(unit)}: {head}, "differences": [' + ("\n" + diffs + "\n  " if diffs else "") + "]}")
        txt = "{\n" + ",\n".join(units) + "\n}"
    if out:
        open(out, "w").write(txt + "\n")
    for unit, r in res.items():
        print(f"{unit}: {r['equal']}/{r['kernels']} kernels equal, {r['insts']} instructions")
        for d in r["differences"]:
            print("  DIFFERS", json.dumps(d))
    return 1 if any(r["differences"] or not r["kernels"] for r in res.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
