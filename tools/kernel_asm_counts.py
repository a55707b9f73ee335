#!/usr/bin/env python3
"""Static counts of one kernel in a device assembly file (tools/kasm.sh METRIC PART OUT.s): instructions, VALU, SALU, lane
reads / writes (v_readlane / v_writelane: what a scalar spill costs on the vector pipe), VGPRs, SGPR spills and code bytes from the
compiler's own summary -- for the whole kernel and for the span of its expansion loop.

    tools/kernel_asm_counts.py OUT.s 'hnsw_search_kernelILi0ELi1ELi0ELi1ELb1E' [more symbol substrings ...]

The expansion loop is found from the layout: the kernel's largest backward branch spans the loop over a workgroup's queries, the
largest one strictly inside it the loop over a query's expansions.  The span is counted in layout order, so blocks the compiler
moved behind the loop (the unlikely paths) are not in it, and blocks of an inner loop are counted once.
"""
import re
import sys

NOT_ALU = ("s_load", "s_buffer_load", "s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_endpgm", "s_barrier", "s_swappc", "s_setpc",
           "s_getpc", "s_sleep", "s_setprio", "s_sendmsg", "s_memtime", "s_memrealtime", "s_code_end", "s_trap", "s_inst_prefetch")


def kernel_lines(text, sym):
    lines = text.split("\n")
    start = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and sym in l]
    if len(start) != 1:
        raise SystemExit("%d labels match %r" % (len(start), sym))
    i0 = start[0]
    i1 = next(i for i in range(i0, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    tail = lines[i1:i1 + 80]
    return lines[i0 + 1:i1], tail


def counts(body):
    c = dict(instructions=0, valu=0, salu=0, v_readlane=0, v_writelane=0, vmem=0, lds=0)
    for l in body:
        op = l.strip().split(" ")[0].split("\t")[0]
        if not op or op.startswith((";", ".")) or op.endswith(":"):
            continue
        c["instructions"] += 1
        if op.startswith("v_readlane") or op.startswith("v_readfirstlane"):
            c["v_readlane"] += 1
        if op.startswith("v_writelane"):
            c["v_writelane"] += 1
        if op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("s_") and not op.startswith(NOT_ALU):
            c["salu"] += 1
        elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
            c["vmem"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
    return c


def loop_span(body):
    """(first, last) line of the second-level loop: see the module text"""
    label_at = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\w+):", l)
        if m:
            label_at[m.group(1)] = i
    back = []
    for i, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\w+)", l)
        if m and m.group(1) in label_at and label_at[m.group(1)] <= i:
            back.append((label_at[m.group(1)], i))
    if not back:
        return None
    outer = max(back, key=lambda b: b[1] - b[0])
    inner = [b for b in back if b != outer and outer[0] <= b[0] and b[1] <= outer[1]]
    return max(inner, key=lambda b: b[1] - b[0]) if inner else None


def summary(tail):
    out = {}
    for l in tail:
        for key, name in (("codeLenInByte", "code_bytes"), ("NumVgprs", "vgprs"), ("NumSgprs", "sgprs"), ("SGPRSpill", "sgpr_spills"),
                          ("VGPRSpill", "vgpr_spills"), ("ScratchSize", "scratch_bytes"), ("Occupancy", "occupancy")):
            m = re.match(r"^;\s*%s\s*[=:]\s*(\d+)" % key, l.strip())
            if m and name not in out:
                out[name] = int(m.group(1))
    return out


def sgpr_spills(text, sym):
    """.sgpr_spill_count of the kernel's metadata entry (its keys are sorted: the count stands in front of .symbol)"""
    lines = text.split("\n")
    for i, l in enumerate(lines):
        if l.strip().startswith(".symbol:") and sym in l:
            for j in range(i, max(i - 12, 0), -1):
                m = re.match(r"\s*\.sgpr_spill_count:\s*(\d+)", lines[j])
                if m:
                    return int(m.group(1))
    return None


def main():
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    text = open(sys.argv[1]).read()
    for sym in sys.argv[2:]:
        body, tail = kernel_lines(text, sym)
        print(sym)
        print("  whole kernel   ", counts(body), dict(summary(tail), sgpr_spills=sgpr_spills(text, sym)))
        span = loop_span(body)
        if span:
            print("  expansion loop ", counts(body[span[0]:span[1] + 1]), "(%d lines of layout)" % (span[1] - span[0] + 1))


if __name__ == "__main__":
    main()
