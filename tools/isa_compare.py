#!/usr/bin/env python3
"""Loop-by-loop comparison of the step kernels of two hipcc -S listings (e.g. before / after a change to stg_kernels.hpp).
Every kernel of `before` whose name holds `key` is matched with the kernel of `after` that has the same name, or -- for a kernel that
gained a trailing `bool` template parameter -- the same name with that parameter false; their loops (backward branches spanning at least
min_len instructions, as tools/isa_loops.py finds them) are listed with their lengths and instruction counts.
usage: python tools/isa_compare.py <before.s> <after.s> [key=stg_step] [min_len=100]"""
import collections
import re
import sys


def functions(path, key):
    out, name, body = {}, None, []
    for l in open(path):
        if name is None:
            head = l.split(";")[0].strip()
            if l.startswith("_Z") and head.endswith(":") and key in head:
                name, body = head[:-1], []
            continue
        if l.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        body.append(l.strip())
    return out


def loops(body, min_len):
    labels, insts = {}, []
    for t in body:
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        if not t or t.startswith(";") or t.startswith(".") or t.endswith(":"):
            continue
        insts.append(t.split(";")[0].strip())
    res = []
    for idx, t in enumerate(insts):
        m = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)", t)
        if m:
            tgt = labels.get(m.group(1) or m.group(2))
            if tgt is not None and tgt <= idx and idx - tgt >= min_len:
                seq = insts[tgt:idx + 1]
                res.append((len(seq), collections.Counter(s.split()[0] for s in seq)))
    return len(insts), res


def main():
    before, after = sys.argv[1], sys.argv[2]
    key = sys.argv[3] if len(sys.argv) > 3 else "stg_step"
    min_len = int(sys.argv[4]) if len(sys.argv) > 4 else 100
    fb, fa = functions(before, key), functions(after, key)
    same = diff = missing = 0
    for name in sorted(fb):
        alt = re.sub(r"EEv(\w*)$", r"ELb0EEv\1", name)         # the same kernel with a trailing `false` template argument
        other = fa.get(name) or fa.get(alt)
        if other is None:
            print(f"MISSING {name}")
            missing += 1
            continue
        nb, lb = loops(fb[name], min_len)
        na, la = loops(other, min_len)
        ok = [x[0] for x in lb] == [x[0] for x in la] and all(x[1] == y[1] for x, y in zip(lb, la))
        same += ok
        diff += not ok
        print(f"{'same' if ok else 'DIFF'} {name}: total {nb} -> {na}; loops " + (" ".join(str(x[0]) for x in lb) or "-") +
              ((" -> " + (" ".join(str(x[0]) for x in la) or "-")) if not ok else ""))
    print(f"{len(fb)} kernels of `before`: {same} with identical loops, {diff} different, {missing} missing")
    return 1 if (diff or missing) else 0


if __name__ == "__main__":
    sys.exit(main())
