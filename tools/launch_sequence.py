#!/usr/bin/env python
"""The ordered launch sequence of a `rocprofv3 --kernel-trace --output-format csv` run: one line per kernel, `name | grid x y z | workgroup x y z | LDS bytes`, in start
order, ALL kernels (grid_* in work-items, as rocprofv3 reports them).  Two builds of the library launch the same work when these files compare equal (experiments/r13.md).
usage: launch_sequence.py <directory or csv> [--compress]      (--compress: consecutive identical launches as one line xN, a repeated block once with its count)"""
import csv, glob, os, re, sys

path = sys.argv[1]
files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
assert len(files) == 1, f"expected one kernel trace under {path}, found {files}"
rows = [{k.lower(): v for k, v in r.items()} for r in csv.DictReader(open(files[0]))]
rows.sort(key=lambda r: (int(r["start_timestamp"]), int(r["dispatch_id"])))
short = lambda n: re.sub(r"\(.*", "", n.replace("(anonymous namespace)::", "")).replace("void bevgen::", "").replace("bevgen::", "")
cols = ["grid_size_x", "grid_size_y", "grid_size_z", "workgroup_size_x", "workgroup_size_y", "workgroup_size_z", "lds_block_size"]
lines = [" | ".join([short(r["kernel_name"])] + [r[c] for c in cols]) for r in rows]


def compress(ls, indent=""):
    out, i = [], 0
    while i < len(ls):
        best = (0, 1, 1)   # (launches covered, period, repetitions)
        for p in range(1, min(400, (len(ls) - i) // 2) + 1):
            n = 1
            while ls[i + n * p:i + (n + 1) * p] == ls[i:i + p]: n += 1
            if n > 1 and n * p > best[0]: best = (n * p, p, n)
        if best[1] == 1 and best[0]:
            out.append(f"{indent}{ls[i]}   x{best[2]}")
        elif best[0]:
            out += [f"{indent}# the next block ({best[1]} launches), {best[2]} times in a row:"] + compress(ls[i:i + best[1]], indent + "  ") + [f"{indent}# (end of block)"]
        else:
            out.append(indent + ls[i])
        i += max(best[0], 1)
    return out


print("\n".join(compress(lines) if "--compress" in sys.argv else lines))
