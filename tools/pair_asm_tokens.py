#!/usr/bin/env python
"""tools/pair_asm_tokens.py conv_pair.s: k_espcn_pair (hipcc -S --cuda-device-only with the flags of _build.py) reduced to tokens -- rN ds_read, wN s_waitcnt lgkmcnt(N), MN v_mfma, s ds_write / ds_add, | a branch -- for every basic block with at least eight MFMAs
(profiles/pair_pipeline_asm.txt)."""
import re, sys
src = open(sys.argv[1]).read().split("\n")
inside = False; blocks = []; cur = None
for ln in src:
    s = ln.strip()
    if re.match(r"_ZN3srk\S*k_espcn_pairE\S*:", s): inside = True; cur = ["entry", []]; blocks.append(cur); continue
    if not inside: continue
    if s.startswith(".Lfunc_end") : break
    m = re.match(r"(\.LBB\d+_\d+):", s)
    if m: cur = [m.group(1), []]; blocks.append(cur); continue
    if s.startswith("ds_read"): cur[1].append("r")
    elif s.startswith("v_mfma"): cur[1].append("M")
    elif s.startswith("s_waitcnt"):
        m = re.search(r"lgkmcnt\((\d+)\)", s)
        if m: cur[1].append("w%s" % m.group(1))
    elif s.startswith("ds_write") or s.startswith("ds_add"): cur[1].append("s")
    elif s.startswith("s_cbranch") or s.startswith("s_branch"): cur[1].append("|")
def rle(t):
    out = []; i = 0
    while i < len(t):
        j = i
        while j < len(t) and t[j] == t[i]: j += 1
        out.append(t[i] + (str(j - i) if j - i > 1 and t[i] in "rMs" else "") if t[i] in "rMs" else " ".join([t[i]] * (j - i)))
        i = j
    return " ".join(out)
tot = 0
for name, t in blocks:
    nm = t.count("M"); tot += nm
    if nm >= 8: print("%s  [%d MFMA, %d ds_read, %d lgkmcnt(0)]\n  %s\n" % (name, nm, t.count("r"), t.count("w0"), rle(t)))
print("v_mfma total", tot)
