#!/usr/bin/env python3
"""Kernel resource usage from a compile log, one build or two side by side.

Compile render.hip with -Rpass-analysis=kernel-resource-usage added to the Makefile's
HIPFLAGS (compile only: no GPU is needed) and keep the compiler's output:

    make -C ba_pathtracing_fur_amd/csrc HIPFLAGS='... -Rpass-analysis=kernel-resource-usage' 2> tree.log
    python3 tools/kernel_resources.py tree.log [parent.log] [--match k_extend,k_path]

With one log: a row per kernel instance (VGPRs, SGPRs, scratch bytes per lane, waves per
SIMD, LDS bytes).  With two: the rows of the first beside the second's, `changed` where
a figure differs and `new` where the second has no such instance.  An instance whose
last template argument is `false` is also looked up without it, so that a kernel that
gained a defaulted parameter is compared with its former self.  The exit status is 1 if
a matched kernel gained scratch or lost occupancy against the second log.
"""
import argparse
import re
import subprocess
import sys

FIELDS = (("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds"))


def parse(path):
    """{demangled kernel name without its parameter list: figures}"""
    rows, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+%s: (\d+)" % re.escape(label), line)
            if m:
                cur[key] = int(m.group(1))
    names = list(rows)
    out = subprocess.run(["c++filt"], input="\n".join(names), text=True, capture_output=True).stdout.split("\n")
    short = lambda s: re.sub(r"^void ", "", s.split("(")[0])
    return {short(d): rows[n] for n, d in zip(names, out)}


def former(name):
    """The instance's name before its last template argument, a `false`, existed."""
    m = re.match(r"(.*)<(.*)>$", name)
    if not m or not re.search(r"(^|, )false$", m.group(2)):
        return None
    args = re.sub(r"(^|, )false$", "", m.group(2))
    return "%s<%s>" % (m.group(1), args) if args else m.group(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log")
    ap.add_argument("other", nargs="?")
    ap.add_argument("--match", default="k_generate,k_extend,k_shade,k_path,k_aov_trace")
    a = ap.parse_args()
    want = a.match.split(",")
    new, old = parse(a.log), parse(a.other) if a.other else None
    names = sorted(n for n in new if n.split("<")[0] in want)
    fig = lambda d: "vgpr %3d sgpr %3d scratch %3d occ %d lds %5d" % tuple(d.get(k, -1) for _, k in FIELDS)
    bad = 0
    for n in names:
        r = new[n]
        line = fig(r)
        if old is not None:
            o = old.get(n)
            if o is None and former(n) is not None:
                o = old.get(former(n))
            if o is None:
                line += "  | " + " " * len(fig(r)) + "  new    "
            else:
                line += "  | " + fig(o) + ("  changed" if o != r else "  same   ")
                if r.get("scratch", 0) > o.get("scratch", 0) or r.get("occ", 0) < o.get("occ", 0):
                    bad += 1
                    line += " WORSE"
        print(line + "  " + n)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
