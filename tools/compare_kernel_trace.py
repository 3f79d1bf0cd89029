#!/usr/bin/env python3
"""Do two runs of one program launch the same dense kernels?   usage: tools/compare_kernel_trace.py OLD.csv NEW.csv

From two `rocprofv3 --kernel-trace --output-format csv` traces it keeps the dispatches of the dense products (kernel names
with `k_gemm_`, and `k_colsum_final` behind the nt products with column sums), in dispatch order, and compares the two
sequences of (kernel, grid size, workgroup size, LDS block size) line by line.  Prints the first difference and the launch
count per kernel; exits 1 on any difference.

What it is for: a change to the host side of csrc/dense.hip that must not move any shape to another kernel, occupancy class
(the LDS reservation decides how many workgroups share a CU) or grid -- trace tests/test_gpu_dense_exact.py before and after.
A trace cut down to the kept rows (any subset of the columns used here) compares the same."""
import collections
import csv
import sys

SIZES = ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z", "LDS_Block_Size")


def dispatches(path):
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "k_gemm_" in r["Kernel_Name"] or "k_colsum_final" in r["Kernel_Name"]]
    missing = [c for c in SIZES if rows and c not in rows[0]]
    if missing:
        sys.exit(f"{path}: no column {', '.join(missing)} (not a rocprofv3 kernel trace?)")
    if rows and "Dispatch_Id" in rows[0]:
        rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"],) + tuple(int(r[c]) for c in SIZES) for r in rows]


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__.split("\n\n")[0])
    old, new = dispatches(sys.argv[1]), dispatches(sys.argv[2])
    first = next((i for i, (a, b) in enumerate(zip(old, new)) if a != b), None)
    if first is None and len(old) != len(new):
        first = min(len(old), len(new))
    counts_old, counts_new = (collections.Counter(d[0] for d in ds) for ds in (old, new))
    print(f"{'old':>7s} {'new':>7s}  kernel")
    for name in sorted(set(counts_old) | set(counts_new)):
        flag = "" if counts_old[name] == counts_new[name] else "   <-- differs"
        print(f"{counts_old[name]:7d} {counts_new[name]:7d}  {name}{flag}")
    print(f"{len(old)} dispatches of {len(counts_old)} kernels in {sys.argv[1]}, {len(new)} of {len(counts_new)} in {sys.argv[2]}")
    if first is None:
        print("identical: every dispatch has the same kernel, grid, workgroup size and LDS block size")
        return 0
    print(f"FIRST DIFFERENCE at dispatch {first}:")
    for tag, ds in (("old", old), ("new", new)):
        if first < len(ds):
            name, *sz = ds[first]
            print(f"  {tag}: grid {sz[0]} x {sz[1]} x {sz[2]}, workgroup {sz[3]} x {sz[4]} x {sz[5]}, LDS {sz[6]}  {name}")
        else:
            print(f"  {tag}: (the trace ends)")
    return 1


if __name__ == "__main__":
    sys.exit(main())
