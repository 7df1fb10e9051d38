"""per-launch medians of k_prop_bwd per proposal level from a rocprofv3 kernel_trace.csv: the launches come in pairs (level 0, then
level 1, of one update step), so level = position inside the pair; k_prop_reduce2 alongside, an unchanged kernel for the spread.
usage: kt_prop_bwd.py <csv>   (the first 20 launches of k_prop_bwd are warm-up and left out)"""
import collections, csv, re, sys
agg = collections.defaultdict(list)
n = 0
for r in sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"])):
    k = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").replace("fnr::", "")
    us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    g = r.get("Grid_Size") or r.get("Grid_Size_X") or ""
    if re.match(r"k_prop_bwd", k):
        agg[(f"{k[:32]} level {n % 2}", g)].append(us)
        n += 1
    elif re.match(r"k_prop_reduce", k):
        agg[(k[:40], g)].append(us)
for (k, g), v in sorted(agg.items()):
    v = sorted(v[10:] if len(v) > 20 else v)      # 20 launches = 10 per level
    print(f"{k:48s} grid {g:>9s} n {len(v):4d} median {v[len(v) // 2]:7.1f} us  min {v[0]:7.1f}  p90 {v[len(v) * 9 // 10]:7.1f}")
