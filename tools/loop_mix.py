"""Static instruction mix of the traversal kernels' loops, from a gfx950 assembly listing.

usage: hipcc <the Makefile's HIPFLAGS> -S --offload-device-only render.hip -o render.s
       python tools/loop_mix.py render.s [name substring ...] > table.md

For every kernel whose mangled name contains one of the substrings (default: the
uninstrumented k_extend / k_shadow instances) prints one markdown row: VGPRs, SGPRs,
scratch bytes per lane, and the instructions by kind between the first backward-branch
target and the last backward branch of the kernel (its persistent loop: refill, flush
and the traversal iteration).  Static counts: what the loop holds, not what a wave
executes; the executed counts per wave iteration come from tools/mix_per_bounce.py.
"""
import re
import sys

src = sys.argv[1]
want = sys.argv[2:] or ["k_extendILb0", "k_shadowILb0"]
text = open(src).read()
lines = text.split("\n")

funcs, cur = {}, None
for ln in lines:
    m = re.match(r"^(_Z\w+):", ln)
    if m and cur is None:
        cur = m.group(1)
        funcs[cur] = []
    elif cur is not None:
        if ln.startswith(".Lfunc_end"):
            cur = None
        else:
            funcs[cur].append(ln)
meta = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
        for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}


def count(body):
    c = dict(salu=0, branch=0, valu=0, vmem=0, lds=0, smem=0, wait=0)
    for ln in body:
        ln = ln.strip()
        if not ln or ln[0] in ".;" or ln.endswith(":"):
            continue
        op = ln.split()[0]
        if op.startswith(("s_waitcnt", "s_nop")):
            c["wait"] += 1
        elif op.startswith(("s_load", "s_buffer_load")):
            c["smem"] += 1
        elif op.startswith(("s_cbranch", "s_branch")):
            c["branch"] += 1
            c["salu"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
            c["vmem"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
    return c


print("| kernel | VGPRs | SGPRs | scratch | SALU (of which branches) | VALU | VMEM | LDS | SMEM |")
print("|---|---|---|---|---|---|---|---|---|")
for name, body in funcs.items():
    if not any(w in name for w in want):
        continue
    labels = {m.group(1): k for k, ln in enumerate(body) for m in [re.match(r"^(\.LBB\w+):", ln)] if m}
    lo = hi = None
    for k, ln in enumerate(body):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\w+)", ln)
        if m and labels.get(m.group(1), k) < k:
            lo = labels[m.group(1)] if lo is None else min(lo, labels[m.group(1)])
            hi = k
    c = count(body[lo:hi + 1]) if lo is not None else count(body)
    md = meta.get(name, {})
    short = re.sub(r"^_Z\d+(k_\w+?)I(.*?)EEv.*", lambda m: m.group(1) + "<" + ",".join((m.group(2) + "E").replace("Lb0E", "0").replace("Lb1E", "1")) + ">", name)
    print(f"| {short} | {md.get('next_free_vgpr')} | {md.get('next_free_sgpr')} | {md.get('private_segment_fixed_size')} | "
          f"{c['salu']} ({c['branch']}) | {c['valu']} | {c['vmem']} | {c['lds']} | {c['smem']} |")
