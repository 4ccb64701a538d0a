"""Instruction counts per labelled block of one kernel in a compiler listing.

    hipcc ... --cuda-device-only -S -o k.s csrc/rt_kernels.hip
    python tools/isa_classes.py k.s rt_trace_tinyILi0ELi1ELi37ELb0E
    python tools/isa_classes.py k.s SYMBOL --path entry,LBB5_2,LBB5_7   # one path's sum
    python tools/isa_classes.py k.s --list                              # the kernels of the file

SYMBOL is the kernel's (mangled) label or a unique part of it.  Every
instruction is put into a class by the prefix of its mnemonic:

    valu    vector ALU                     v_*
    salu    scalar ALU                     s_* not listed below
    branch  s_branch, s_cbranch_*, s_setpc / s_swappc / s_call
    smem    scalar memory                  s_load_*, s_buffer_load_*, s_memtime ...
    vmem    vector memory and LDS          global_*, flat_*, buffer_*, scratch_*, ds_*
    wait    s_nop, s_waitcnt*, s_sleep
    other   s_endpgm, s_barrier, messages ...

and counted in the block it stands in (a block runs from one `.LBBn_m:`
label to the next; the code before the first label is `entry`).  The
listing is static: what a wave executes is the sum over the blocks on its
path (--path), which the reader takes from the branches at the blocks' ends.
Lane spills of scalars (v_writelane / v_readlane) are counted beside the
classes, as they are vector instructions doing the scalar side's work.
"""
from __future__ import annotations

import argparse
import re
import sys

CLASSES = ("valu", "salu", "branch", "smem", "vmem", "wait", "other")
BRANCH = ("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_call")
SMEM = ("s_load", "s_buffer_load", "s_scratch_load", "s_memtime", "s_memrealtime", "s_dcache_inv", "s_atc_probe")
WAIT = ("s_nop", "s_waitcnt", "s_sleep")
OTHER = ("s_endpgm", "s_barrier", "s_sendmsg", "s_trap", "s_icache_inv", "s_setprio", "s_sethalt", "s_code_end",
         "s_wakeup", "s_ttrace", "s_incperflevel", "s_decperflevel")
VMEM = ("global_", "flat_", "buffer_", "scratch_", "ds_", "tbuffer_", "image_")

LABEL = re.compile(r"^(\.?[A-Za-z_$][\w$.]*):")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")


def classify(mn: str) -> str | None:
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith(VMEM):
        return "vmem"
    if not mn.startswith("s_"):
        return None  # a directive's operand or something that is no instruction
    for cls, pre in (("branch", BRANCH), ("smem", SMEM), ("wait", WAIT), ("other", OTHER)):
        if mn.startswith(pre):
            return cls
    return "salu"


def kernels(lines):
    """(label, first line, end line) of every function of the listing."""
    out, cur = [], None
    for i, ln in enumerate(lines):
        m = LABEL.match(ln)
        if m and not m.group(1).startswith(".") and cur is None and i and ".type" in "".join(lines[max(0, i - 4):i]):
            cur = (m.group(1), i + 1)
        elif cur and ln.startswith(".Lfunc_end"):
            out.append((cur[0], cur[1], i))
            cur = None
    return out


def count(lines):
    """[(block, {class: n, 'lane_spill': n})] in listing order."""
    blocks = [("entry", dict.fromkeys(CLASSES + ("lane_spill",), 0))]
    for ln in lines:
        text = ln.split(";", 1)[0]
        m = LABEL.match(text)
        if m:
            if m.group(1).startswith(".LBB"):
                blocks.append((m.group(1)[1:], dict.fromkeys(CLASSES + ("lane_spill",), 0)))
            continue
        m = INSN.match(text)
        if not m:
            continue
        cls = classify(m.group(1))
        if cls is None:
            continue
        blocks[-1][1][cls] += 1
        if m.group(1).startswith(("v_writelane", "v_readlane")):
            blocks[-1][1]["lane_spill"] += 1
    return blocks


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("symbol", nargs="?")
    ap.add_argument("--list", action="store_true", help="print the listing's function labels")
    ap.add_argument("--path", help="comma-separated block names: print only their sum")
    ap.add_argument("--total", action="store_true", help="print only the kernel's total")
    a = ap.parse_args()
    with open(a.listing) as f:
        lines = f.read().splitlines()
    ks = kernels(lines)
    if a.list or not a.symbol:
        for name, b, e in ks:
            print(name)
        return 0
    hit = [k for k in ks if k[0] == a.symbol] or [k for k in ks if a.symbol in k[0]]
    if len(hit) != 1:
        print(f"{a.symbol}: {len(hit)} kernels match" + "".join("\n  " + k[0] for k in hit[:20]), file=sys.stderr)
        return 2
    name, b, e = hit[0]
    blocks = count(lines[b:e])
    cols = CLASSES + ("lane_spill",)
    head = f"{'block':<14}" + "".join(f"{c:>11}" for c in cols) + f"{'all':>8}"

    def row(label, d):
        return f"{label:<14}" + "".join(f"{d[c]:>11}" for c in cols) + f"{sum(d[c] for c in CLASSES):>8}"

    total = {c: sum(d[c] for _, d in blocks) for c in cols}
    print(f"# {name}: {len(blocks)} blocks")
    print(head)
    if a.path:
        want = [p.strip().lstrip(".") for p in a.path.split(",") if p.strip()]
        by = dict(blocks)
        missing = [p for p in want if p not in by]
        if missing:
            print("no such block: " + ", ".join(missing), file=sys.stderr)
            return 2
        print(row("path", {c: sum(by[p][c] for p in want) for c in cols}))
        return 0
    if not a.total:
        for label, d in blocks:
            print(row(label, d))
    print(row("total", total))
    return 0


if __name__ == "__main__":
    sys.exit(main())
