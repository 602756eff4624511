"""Compare two rocprofv3 kernel traces: same kernel names in the same order, same grid, workgroup size and LDS size per dispatch."""
import csv
import glob
import sys


def load(d):
    files = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))
    assert len(files) == 1, (d, files)
    with open(files[0]) as fh:
        rows = list(csv.DictReader(fh))
    cols = [c for c in rows[0] if any(s in c for s in ("Grid", "Workgroup", "LDS"))]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return cols, [(r["Kernel_Name"],) + tuple(r[c] for c in cols) for r in rows]


ca, a = load(sys.argv[1])
cb, b = load(sys.argv[2])
print("columns compared: Kernel_Name,", ", ".join(ca))
print(f"dispatches: {len(a)} / {len(b)}")
assert ca == cb
ours = [r for r in a if r[0].startswith(("k_", "void k_"))]
print(f"of them the library's own kernels (first trace): {len(ours)}; distinct names: {len(set(r[0] for r in ours))}")
bad = 0
for i, (x, y) in enumerate(zip(a, b)):
    if x != y:
        bad += 1
        if bad <= 40:
            print(f"DIFF dispatch {i}:\n  - {x}\n  + {y}")
if len(a) != len(b):
    bad += abs(len(a) - len(b))
print("EMPTY DIFF: the two traces list the same kernels in the same order with the same grid, workgroup and LDS sizes" if bad == 0
      else f"{bad} dispatches differ")
for name in sorted(set(r[0] for r in ours)):
    shapes = sorted(set(r[1:] for r in ours if r[0] == name))
    print(f"  {name}: {len([r for r in ours if r[0] == name])} dispatches, {len(shapes)} distinct (grid, workgroup, LDS)")
sys.exit(1 if bad else 0)
