"""per-launch medians of the per-ray kernels from a rocprofv3 kernel_trace.csv; k_weights_pdf split by its position in the step
(launches alternate: first proposal level, second proposal level).   usage: kt_per_ray.py <csv>   (the first 20 launches of a kernel are warm-up and left out)"""
import collections, csv, re, sys
rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
agg = collections.defaultdict(list)
for r in rows:
    k = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").replace("fnr::", "")
    if not re.match(r"k_train_losses|k_weights_pdf|k_composite_fwd_bwd|k_composite_bwd|k_weights_bwd|k_distortion_bwd|k_composite_fwd\b", k):
        continue
    agg[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
def med(v):
    v = sorted(v); return v[len(v) // 2]
for k, v in sorted(agg.items()):
    v = v[20:] if len(v) > 40 else v   # warm-up launches
    if k.startswith("k_weights_pdf") and "<" not in k:
        for i, tag in ((0, "even launches"), (1, "odd launches")):
            s = v[i::2]; print(f"{k:40s} {tag:14s} n {len(s):4d} median {med(s):6.1f} us min {min(s):6.1f}")
    else:
        print(f"{k:40s} {'':14s} n {len(v):4d} median {med(v):6.1f} us min {min(v):6.1f}")
