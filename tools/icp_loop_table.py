#!/usr/bin/env python3
"""Static instruction table of a kernel's loops, from its ISA: the control-flow graph's loops (strongly connected
components, nested ones indented) with their instruction counts, the lane moves among them and the pieces of the compiler's
float64 square root (v_rsq_f64, v_ldexp_f64, v_cmp_class_f64).  With a loop's header label as third argument: the lane reads
in that loop that reload a spilled scalar (a v_readlane_b32 from a VGPR that some v_writelane_b32 of the kernel writes) apart
from those of reductions and broadcasts, and which of them sit in nested loops.  profiles/icp_one_wave_trims.txt is this
table for the later iterations of k_icp<double> (the loop with six unrolled queries).

usage: hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Iinclude -S --cuda-device-only -o icp.s <package>/csrc/icp_kernels.hip
       icp_loop_table.py icp.s _ZN4slam5k_icpIdEEvNS_7IcpArgsE [.LBB3_602]"""
import re, sys
sys.setrecursionlimit(100000)
text = open(sys.argv[1]).read().split("\n")
sym = sys.argv[2]
start = next(i for i, l in enumerate(text) if l.startswith(sym + ":"))
end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
body = text[start:end]
def isinst(l):
    return bool(re.match(r"^\t[a-z]", l)) and not l.startswith("\t.")
# basic blocks
blocks = []   # (label or None, [instructions])
cur = {"labels": [], "ins": []}
blocks.append(cur)
for l in body:
    m = re.match(r"^(\.LBB\d+_\d+):", l)
    if m:
        if cur["ins"] or cur["labels"]:
            cur = {"labels": [], "ins": []}; blocks.append(cur)
        cur["labels"].append(m.group(1)); continue
    if isinst(l):
        cur["ins"].append(l.strip())
        op = l.split()[0]
        if op.startswith("s_branch") or op.startswith("s_cbranch") or op == "s_endpgm" or op.startswith("s_setpc"):
            cur = {"labels": [], "ins": []}; blocks.append(cur)
lab2b = {}
for i, b in enumerate(blocks):
    for lb in b["labels"]: lab2b[lb] = i
succ = [[] for _ in blocks]
for i, b in enumerate(blocks):
    last = b["ins"][-1] if b["ins"] else ""
    op = last.split()[0] if last else ""
    if op.startswith("s_branch") or op.startswith("s_cbranch"):
        t = last.split()[1]
        if t in lab2b: succ[i].append(lab2b[t])
    if not (op.startswith("s_branch") or op == "s_endpgm") and i + 1 < len(blocks):
        succ[i].append(i + 1)
# Tarjan, iterative
def sccs(nodes, succ):
    index = {}; low = {}; onst = set(); st = []; out = []; idx = [0]
    nodes = set(nodes)
    for root in sorted(nodes):
        if root in index: continue
        work = [(root, 0)]
        while work:
            v, pi = work.pop()
            if pi == 0:
                index[v] = low[v] = idx[0]; idx[0] += 1; st.append(v); onst.add(v)
            rec = False
            ss = [w for w in succ[v] if w in nodes]
            for k in range(pi, len(ss)):
                w = ss[k]
                if w not in index:
                    work.append((v, k + 1)); work.append((w, 0)); rec = True; break
                elif w in onst:
                    low[v] = min(low[v], index[w])
            if rec: continue
            if low[v] == index[v]:
                comp = []
                while True:
                    w = st.pop(); onst.discard(w); comp.append(w)
                    if w == v: break
                out.append(comp)
            if work:
                p = work[-1][0]
                low[p] = min(low[p], low[v])
    return out
def stats(bs):
    ins = [x.split()[0] for b in bs for x in blocks[b]["ins"]]
    c = lambda f: sum(1 for x in ins if f(x))
    return dict(total=len(ins), valu=c(lambda x: x.startswith("v_")), readlane=c(lambda x: x.startswith("v_readlane")), writelane=c(lambda x: x.startswith("v_writelane")),
                rsq64=c(lambda x: x.startswith("v_rsq_f64")), ldexp64=c(lambda x: x.startswith("v_ldexp_f64")), cmpclass64=c(lambda x: x.startswith("v_cmp_class_f64")),
                s_load=c(lambda x: x.startswith("s_load")), blocks=len(bs))
print("kernel", stats(range(len(blocks))))
def show(nodes, depth, mindepth_print=2):
    for comp in sccs(nodes, succ):
        if len(comp) == 1 and comp[0] not in succ[comp[0]]: continue
        s = stats(comp)
        if s["total"] >= 150:
            print("  " * depth + "loop at block %d (%s)" % (min(comp), ",".join(blocks[min(comp)]["labels"])), s)
            if depth < mindepth_print:
                # nested: remove header (min index block by layout is not nec. header; remove the block with preds outside)
                preds_out = [v for v in comp if any(v in succ[u] for u in range(len(blocks)) if u not in set(comp))]
                inner = set(comp) - set(preds_out[:1] or [min(comp)])
                show(inner, depth + 1)
show(range(len(blocks)), 0)

# ---- spill analysis of the chosen loop (argv[3] = header label)
if len(sys.argv) > 3:
    hdr = lab2b[sys.argv[3]]
    comp = next(c for c in sccs(range(len(blocks)), succ) if hdr in c)
    spillv = set()
    for b in blocks:
        for x in b["ins"]:
            if x.startswith("v_writelane"):
                spillv.add(x.split()[1].rstrip(","))
    print("spill VGPRs (targets of v_writelane anywhere in the kernel):", sorted(spillv))
    inner = set()
    for c in sccs(set(comp) - {hdr}, succ):
        if len(c) > 1 or c[0] in succ[c[0]]:
            inner |= set(c)
    n_sp = n_other = n_sp_inner = 0
    for b in sorted(comp):
        for x in blocks[b]["ins"]:
            if x.startswith("v_readlane"):
                src = x.split()[2].rstrip(",")
                if src in spillv:
                    n_sp += 1
                    n_sp_inner += b in inner
                    print("  spill reload block", b, "inner" if b in inner else "straight", x)
                else:
                    n_other += 1
    tot = sum(len(blocks[b]["ins"]) for b in comp); tot_inner = sum(len(blocks[b]["ins"]) for b in inner)
    print("loop total", tot, "in nested loops", tot_inner, "straight-line", tot - tot_inner)
    print("spill reloads", n_sp, "(in nested loops %d)" % n_sp_inner, "other readlane", n_other)
