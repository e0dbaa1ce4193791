#!/usr/bin/env python3
"""Are the kernels of two hipcc -S listings the same machine code?  Every function (`_Z...:` up to its .Lfunc_end) of `before` is
compared as text with the function of the same name in `after`: comments stripped, basic-block labels .LBB<f>_<n> renumbered to
.LBB_<n> (the function index moves when a translation unit gains or loses a function).  Functions only `after` has are listed.
--rename OLD=NEW (repeatable) replaces the substring OLD by NEW in the names and bodies of `before`, so that a body can be held against
the differently named one that took its place: a kernel that became an instantiation of a merged template.  Names are mangled, so the
length prefix belongs to the substring: --rename 22stg_step_shaped_kernel=21stg_step_pulse_kernel.
usage: python tools/isa_identical.py [--rename OLD=NEW ...] <before.s> <after.s> [name-substring ...]
(exit status 1 if a body differs or is missing)"""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for l in open(path):
        if name is None:
            head = l.split(";")[0].strip()
            if l.startswith("_Z") and head.endswith(":"):
                name, body = head[:-1], []
            continue
        if l.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        t = l.split(";")[0].strip()
        if t:
            body.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t))
    return out


def main():
    renames = []
    while len(sys.argv) > 2 and sys.argv[1] == "--rename":
        renames.append(sys.argv[2].split("=", 1))
        del sys.argv[1:3]

    def renamed(t):
        for old, new in renames:
            t = t.replace(old, new)
        return t

    before, after, keys = functions(sys.argv[1]), functions(sys.argv[2]), sys.argv[3:]
    before = {renamed(k): [renamed(t) for t in v] for k, v in before.items()}
    pick = lambda d: {k: v for k, v in d.items() if not keys or any(s in k for s in keys)}      # noqa: E731
    before, after = pick(before), pick(after)
    same = diff = missing = lines = 0
    for name in sorted(before):
        if name not in after:
            print(f"MISSING   {name}")
            missing += 1
        elif before[name] != after[name]:
            print(f"DIFFERENT {name}: {len(before[name])} -> {len(after[name])} lines")
            diff += 1
        else:
            same += 1
            lines += len(before[name])
    new = sorted(set(after) - set(before))
    print(f"{sys.argv[1]} -> {sys.argv[2]}: before {len(before)} functions, after {len(after)}; identical {same} ({lines} lines compared), "
          f"different {diff}, only-before {missing}, only-after {len(new)}")
    for name in new:
        print(f"  only after: {name}")
    return 1 if (diff or missing) else 0


if __name__ == "__main__":
    sys.exit(main())
