#!/usr/bin/env python3
"""Instruction-class counts per basic block of one kernel in a device assembly file.

An accounting aid for instruction-count work on the forward's steady tile:

    hipcc <the Makefile's flags> --cuda-device-only -S csrc/attention_fwd_v2.hip -o fwd_v2.s
    python tools/isa_count.py fwd_v2.s 'mfa_fwd2_share_kernel<mfa::F16, 128, 64, true, true, true, true>'

The kernel is named by a substring (or regular expression) of its mangled or demangled symbol.
Blocks start at labels (.LBBn_m:) and at the compiler's `; %bb.n:` comments: a block reached
only by fall-through has no label, and splitting at labels alone merges it into its
predecessor.  By default only blocks inside a loop (between a backward branch and its target)
that hold at least --min-insts instructions and --min-mfma MFMAs are printed; --all prints
every block.

Per block: MFMA, VALU, SALU, LDS, vector memory, scalar memory, waits (s_waitcnt, with the
lgkmcnt-only ones counted apart), s_nop (and the wait states they add up to), branches and
barriers; then the VALU and SALU mnemonics with their counts.
"""
from __future__ import annotations

import argparse
import collections
import re
import shutil
import subprocess
import sys

LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BBCOM = re.compile(r"^; %bb\.(\d+):")
INSTR = re.compile(r"^\s+([a-z][a-z0-9_]+)\b(.*)$")
SYM = re.compile(r"^([A-Za-z_][\w$.]*):\s*(?:;.*)?$")
SUFFIX = re.compile(r"_(e32|e64|dpp|sdwa|e64_dpp)$")


def demangle(names: list[str]) -> dict[str, str]:
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    try:
        out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True,
                             check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}
    return {n: (out[i] if i < len(out) and out[i] else n) for i, n in enumerate(names)}


def kernel_symbols(lines: list[str]) -> list[tuple[str, int]]:
    """(symbol, line index) of every function defined in the file."""
    types = set()
    for ln in lines:
        m = re.match(r"^\s+\.type\s+([^,\s]+),@function", ln)
        if m:
            types.add(m.group(1))
    found = []
    for i, ln in enumerate(lines):
        m = SYM.match(ln)
        if m and m.group(1) in types:
            found.append((m.group(1), i))
    return found


def classify(mn: str) -> str:
    if mn.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if mn.startswith("ds_"):
        return "lds"
    if mn == "s_waitcnt" or mn.startswith("s_waitcnt_"):
        return "wait"
    if mn == "s_nop":
        return "nop"
    if mn == "s_barrier":
        return "barrier"
    if mn.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")):
        return "branch"
    if mn.startswith(("s_load", "s_buffer_load", "s_scratch_load")):
        return "smem"
    if mn.startswith(("buffer_", "global_", "flat_", "scratch_", "tbuffer_")):
        return "vmem"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith("v_"):
        return "valu"
    return "other"


class Block:
    def __init__(self, name: str, line: int):
        self.name, self.line = name, line
        self.n = collections.Counter()
        self.valu = collections.Counter()
        self.salu = collections.Counter()
        self.nop_states = 0
        self.lgkm_waits = 0
        self.in_loop = False

    def add(self, mn: str, rest: str) -> None:
        cls = classify(mn)
        self.n[cls] += 1
        if cls == "valu":
            self.valu[SUFFIX.sub("", mn)] += 1
        elif cls == "salu":
            self.salu[mn] += 1
        elif cls == "nop":
            m = re.search(r"(\d+)", rest)
            self.nop_states += (int(m.group(1)) if m else 0) + 1
        elif cls == "wait" and "lgkmcnt" in rest and "vmcnt" not in rest:
            self.lgkm_waits += 1


def parse_kernel(lines: list[str], start: int):
    """Blocks of the function whose symbol is at line `start`, and its resource comments."""
    blocks = [Block("entry", start + 1)]
    label_block: dict[str, int] = {}
    branches: list[tuple[int, str]] = []  # (block index, target label)
    info: dict[str, str] = {}
    i = start + 1
    while i < len(lines):
        ln = lines[i]
        if ln.startswith(".Lfunc_end"):
            break
        m = LABEL.match(ln)
        if m:
            blocks.append(Block(m.group(1), i + 1))
            label_block[m.group(1)] = len(blocks) - 1
        else:
            m = BBCOM.match(ln)
            if m:
                if blocks[-1].n:  # a label directly followed by its %bb comment is one block
                    blocks.append(Block("%bb." + m.group(1), i + 1))
                elif blocks[-1].name == "entry":
                    blocks[-1].name = "%bb." + m.group(1)
            else:
                m = INSTR.match(ln)
                if m and not ln.lstrip().startswith((".", ";")):
                    blocks[-1].add(m.group(1), m.group(2))
                    if m.group(1).startswith(("s_cbranch", "s_branch")):
                        t = re.search(r"(\.LBB\d+_\d+)", m.group(2))
                        if t:
                            branches.append((len(blocks) - 1, t.group(1)))
        i += 1
    for src, tgt in branches:
        dst = label_block.get(tgt)
        if dst is not None and dst <= src:
            for b in blocks[dst:src + 1]:
                b.in_loop = True
    # Resource comments follow the function's end up to the next function.
    while i < len(lines) and not lines[i].lstrip().startswith(".globl"):
        m = re.match(r"^; (NumVgprs|NumAgprs|TotalNumVgprs|NumSgprs|ScratchSize|Occupancy|"
                     r"LDSByteSize|codeLenInByte): (\S+)", lines[i])
        if m:
            info[m.group(1)] = m.group(2)
        i += 1
    return blocks, info


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm", help="device assembly (hipcc --cuda-device-only -S)")
    ap.add_argument("kernel", help="substring or regular expression of the kernel's symbol")
    ap.add_argument("--all", action="store_true", help="every block, not only loop blocks")
    ap.add_argument("--min-mfma", type=int, default=0,
                    help="least MFMAs for a loop block to be printed (default 0)")
    ap.add_argument("--min-insts", type=int, default=16,
                    help="least instructions for a loop block to be printed (default 16)")
    ap.add_argument("--no-mnemonics", action="store_true", help="totals only")
    a = ap.parse_args()
    with open(a.asm, errors="replace") as f:
        lines = f.read().split("\n")
    syms = kernel_symbols(lines)
    pretty = demangle([s for s, _ in syms])
    try:
        pat = re.compile(a.kernel)
    except re.error:
        pat = None
    hits = [(s, i) for s, i in syms
            if a.kernel in s or a.kernel in pretty[s] or (pat and (pat.search(s) or pat.search(pretty[s])))]
    if not hits:
        print(f"isa_count: no function matches {a.kernel!r}; the file defines:", file=sys.stderr)
        for s, _ in syms:
            print("  " + pretty[s], file=sys.stderr)
        return 1
    for sym, at in hits:
        blocks, info = parse_kernel(lines, at)
        print(f"== {pretty[sym]}")
        print("   " + "  ".join(f"{k} {v}" for k, v in info.items()))
        for b in blocks:
            if not a.all and not (b.in_loop and b.n["mfma"] >= a.min_mfma and
                                  sum(b.n.values()) >= a.min_insts):
                continue
            n = b.n
            print(f"  {b.name:<12} line {b.line:<7} {'loop' if b.in_loop else '    '} "
                  f"mfma {n['mfma']:>3} valu {n['valu']:>3} salu {n['salu']:>3} lds {n['lds']:>3} "
                  f"vmem {n['vmem']:>2} smem {n['smem']:>2} wait {n['wait']:>2} "
                  f"(lgkm-only {b.lgkm_waits}) nop {n['nop']} ({b.nop_states} states) "
                  f"branch {n['branch']} barrier {n['barrier']}")
            if not a.no_mnemonics:
                for title, c in (("valu", b.valu), ("salu", b.salu)):
                    if c:
                        print(f"      {title}: " + ", ".join(f"{k} {v}" for k, v in c.most_common()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
