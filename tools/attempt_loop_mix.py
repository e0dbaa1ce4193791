#!/usr/bin/env python3
"""Issue-slot mix of the RK45 attempt loops in a `make asm` listing (csrc/stg_step_rk45.s or the combined spintorque_hip.s).

For each kernel named below the loops (backward branches) of at least MIN_LEN instructions are listed with the classes a lone
wavefront pays one issue slot each for: VALU fp64, other VALU, SALU, LDS, waits (s_waitcnt / s_nop), barrier, branches, memory.
The attempt loop of an integrating wavefront is the loop with the most fp64 VALU instructions; the producer's loop is the one
that writes LDS.  With --ops the opcode histogram of every listed loop is printed as well.

usage: python tools/attempt_loop_mix.py <file.s> [--ops] [--min-len N] [kernel-substring ...]"""
import collections
import re
import sys

# RK45, AXIS_Z, one device class, float actions, full-N launch (IDS = false): the bench rows
KERNELS = {
    "paired thermal (headline: PC, 1 + 1 wavefronts)": "stg_step_kernelILi2ELb1ELi0ELb1ELb0EfLb1ELi1ELb0EE",
    "inline thermal (4 wavefronts per workgroup)": "stg_step_kernelILi2ELb1ELi0ELb1ELb0EfLb0ELi4ELb0EE",
    "T = 0 K (4 wavefronts per workgroup)": "stg_step_kernelILi2ELb0ELi0ELb1ELb0EfLb0ELi4ELb0EE",
    "refill, thermal": "stg_step_refill_kernelILb1ELb0ELb1EfLi4ELb0EE",
    "refill, T = 0 K": "stg_step_refill_kernelILb0ELb0ELb1EfLi4ELb0EE",
}
ORDER = ["VALU fp64", "VALU other", "SALU", "LDS", "wait", "barrier", "branch", "memory"]


def classify(op):
    if op.startswith("v_"):
        return "VALU fp64" if "f64" in op or op == "v_mov_b64" else "VALU other"
    if op in ("s_waitcnt", "s_nop") or op.startswith("s_waitcnt"):
        return "wait"
    if op == "s_barrier":
        return "barrier"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    return "memory"


def kernel_insts(lines, key):
    start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and key in l.split(":")[0]), None)
    if start is None:
        return None, None
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    labels, insts = {}, []
    for l in lines[start + 1:end]:
        t = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        if not t or t.startswith(";") or t.startswith(".") or t.endswith(":"):
            continue
        # (an inline-asm block arrives as one line per instruction already; strip trailing comments)
        insts.append(t.split(";")[0].strip())
    return labels, insts


def loops_of(labels, insts, min_len):
    out = []
    for idx, t in enumerate(insts):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", t)
        if m:
            tgt = labels.get(m.group(1))
            if tgt is not None and tgt <= idx and idx - tgt + 1 >= min_len:
                out.append((tgt, idx))
    # innermost only: drop a loop that contains another listed loop
    return [(a, b) for a, b in out if not any((a <= c and d <= b) and (a, b) != (c, d) for c, d in out)]


def main():
    args = sys.argv[1:]
    show_ops = "--ops" in args
    if show_ops:
        args.remove("--ops")
    min_len = 150
    if "--min-len" in args:
        j = args.index("--min-len")
        min_len = int(args[j + 1])
        del args[j:j + 2]
    path, keys = args[0], args[1:]
    lines = open(path).read().split("\n")
    sel = {k: k for k in keys} if keys else KERNELS
    for title, key in sel.items():
        labels, insts = kernel_insts(lines, key)
        if insts is None:
            print(f"== {title}: kernel {key} not in the listing")
            continue
        print(f"== {title}  [{key}]  {len(insts)} instructions")
        for a, b in loops_of(labels, insts, min_len):
            seq = insts[a:b + 1]
            g = collections.Counter(classify(t.split()[0]) for t in seq)
            kind = "producer" if any(t.startswith("ds_write") for t in seq) and g["VALU fp64"] < 100 else "integrating"
            print(f"  loop [{a},{b}] ({kind}) slots={len(seq)}: " + ", ".join(f"{k}={g[k]}" for k in ORDER if g[k]))
            if show_ops:
                ops = collections.Counter(t.split()[0] for t in seq)
                for cls in ORDER:
                    row = sorted(((o, c) for o, c in ops.items() if classify(o) == cls), key=lambda x: -x[1])
                    if row:
                        print(f"      {cls:10s} " + ", ".join(f"{o}={c}" for o, c in row))


if __name__ == "__main__":
    main()
