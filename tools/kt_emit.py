"""per-launch medians of k_scatter_emit by grid size (x = 512-sample chunks: the field's call, proposal level 0, proposal level 1)
from a rocprofv3 kernel_trace.csv; k_scatter_accumulate alongside, unchanged kernels for the spread.
usage: kt_emit.py <csv>   (the first 20 launches of a (kernel, grid) pair are warm-up and left out)"""
import collections, csv, re, sys
agg = collections.defaultdict(list)
for r in sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"])):
    k = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").replace("fnr::", "")
    if not re.match(r"k_scatter_", k):
        continue
    g = r.get("Grid_Size") or r.get("Grid_Size_X") or ""
    agg[(k[:48], g)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for (k, g), v in sorted(agg.items()):
    v = sorted(v[20:] if len(v) > 40 else v)
    print(f"{k:48s} grid {g:>9s} n {len(v):4d} median {v[len(v) // 2]:7.1f} us  min {v[0]:7.1f}  p90 {v[len(v) * 9 // 10]:7.1f}")
