"""Launches per step, mean duration and ms per step of every (kernel, workgroups) pair of a rocprofv3 --kernel-trace CSV: the same
kernel at two batch sizes shows as two rows (the tables of profiles/dedup_*_launches_by_grid.txt).
    python tools/ktrace_by_grid.py <kernel_trace.csv[.gz]> <steps incl. warm-up> [name regex]"""
import collections, csv, gzip, io, re, sys
path, steps = sys.argv[1], int(sys.argv[2])
flt = sys.argv[3] if len(sys.argv) > 3 else ""
f = io.TextIOWrapper(gzip.open(path)) if path.endswith(".gz") else open(path)
acc = collections.defaultdict(lambda: [0, 0.0])
for r in csv.DictReader(f):
    name = r["Kernel_Name"]
    if flt and not re.search(flt, name):
        continue
    short = re.sub(r"\(.*$", "", re.sub(r"^void ", "", name))[:70]
    wg = 1
    for d in "XYZ":
        wg *= max(int(r.get(f"Grid_Size_{d}") or 1) // max(int(r.get(f"Workgroup_Size_{d}") or 1), 1), 1)
    a = acc[(short, wg)]
    a[0] += 1
    a[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
for (k, wg), (n, us) in sorted(acc.items()):
    print(f"{k:70s} wg {wg:7d}  launches/step {n / steps:6.1f}  mean {us / n:8.1f} us  ms/step {us / steps / 1000:7.3f}")
