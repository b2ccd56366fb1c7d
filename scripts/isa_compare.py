#!/usr/bin/env python3
"""Compare the kernels of two sets of gfx950 assembly files (hipcc ... --cuda-device-only -S), kernel by kernel.

    python scripts/isa_compare.py --old OLD.s [OLD2.s ...] --new NEW.s [NEW2.s ...]

For a refactor that must not change the generated code: per kernel the resource numbers of the code object's
metadata (VGPRs, SGPRs, scratch bytes, LDS bytes), the instruction count and whether the opcode histogram
(mnemonic -> count) is the same.  Kernels are matched by mangled name; one whose parameter list changed (and with it
the mangled name) is matched by its demangled name without the parameters.  Verdict per kernel:
  identical      same instructions in the same order, registers and labels included
  renamed only   same resource numbers, instruction count and opcode histogram; register numbers or block order differ
  DIFFERENT      anything else (the differing numbers / opcodes are listed)
Exit status 1 if any kernel is DIFFERENT or has no partner.
"""
import argparse
import collections
import re
import subprocess
import sys

FIELDS = [".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size"]


def parse(path):
    """{mangled kernel name: {"res": {field: int}, "ins": [instruction lines]}}"""
    text = open(path).read().split("\n")
    bodies, cur = {}, None
    for line in text:
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1)
            bodies[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None:
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        bodies[cur].append(re.sub(r"\.L(BB|func_end|tmp)\d+", r".L\1", re.sub(r"\s+", " ", s)))   # (labels carry the function's number in its file)
    kernels, name, res = {}, None, {}
    for line in text:
        s = line.strip()
        if s.startswith("- .agpr_count:") or s.startswith("- .args:"):
            if name:
                kernels[name] = {"res": res, "ins": bodies.get(name, [])}
            name, res = None, {}
        m = re.match(r"^(?:- )?(\.\w+):\s*(\S+)$", s)
        if not m:
            continue
        if m.group(1) == ".name":
            name = m.group(2)
        elif m.group(1) in FIELDS:
            res[m.group(1)] = int(m.group(2))
    if name:
        kernels[name] = {"res": res, "ins": bodies.get(name, [])}
    return {k: v for k, v in kernels.items() if len(v["res"]) == len(FIELDS)}


def demangle(names):
    out = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def short(dem):
    """psamd::k_pairs<1, 8>(...) -> k_pairs<1, 8>"""
    s = re.sub(r"^void ", "", dem)
    depth = 0
    for i, ch in enumerate(s):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            s = s[:i]
            break
    return s.replace("psamd::", "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    old, new = {}, {}
    for p in a.old:
        old.update(parse(p))
    for p in a.new:
        new.update(parse(p))
    dem = demangle(sorted(set(old) | set(new)))
    new_by_short = {short(dem[k]): k for k in new}
    bad = 0
    print("%-34s %-27s %-27s %s" % ("kernel", "old vgpr sgpr scratch lds ins", "new vgpr sgpr scratch lds ins", "verdict"))
    for k in sorted(old, key=lambda k: short(dem[k])):
        sk = short(dem[k])
        partner = k if k in new else new_by_short.get(sk)
        if partner is None:
            print("%-34s no partner in the new files" % sk)
            bad += 1
            continue
        o, n = old[k], new[partner]
        ro = [o["res"][f] for f in FIELDS] + [len(o["ins"])]
        rn = [n["res"][f] for f in FIELDS] + [len(n["ins"])]
        ho = collections.Counter(i.split(" ")[0] for i in o["ins"])
        hn = collections.Counter(i.split(" ")[0] for i in n["ins"])
        if o["ins"] == n["ins"] and ro == rn:
            verdict = "identical"
        elif ro == rn and ho == hn:
            verdict = "renamed only"
        else:
            diff = ["%s %+d" % (m, hn[m] - ho[m]) for m in sorted(set(ho) | set(hn)) if ho[m] != hn[m]]
            verdict = "DIFFERENT" + (" (name changed)" if partner != k else "") + ": " + ", ".join(diff[:12]) + (" ..." if len(diff) > 12 else "")
            bad += 1
        print("%-34s %-27s %-27s %s" % (sk, " ".join(map(str, ro)), " ".join(map(str, rn)), verdict))
    for k in sorted(set(short(dem[k]) for k in new) - set(short(dem[k]) for k in old)):
        print("%-34s only in the new files" % k)
        bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
