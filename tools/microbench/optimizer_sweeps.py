"""The optimiser sweeps in isolation, for same-box A/B runs of two builds of the library (FNR_LIB_PATH, tools/build_variant.sh):
fnr_adam_step and fnr_radam_step over 2^24 floats, fnr_adam_step_spans over the default fruit_nerf arena's parameter groups as
FusedAdam.step issues it (one span per group, own learning rate and step count), fnr_adam_step_spans_dev over the same spans.
Per leg 10 untimed calls, then 50 calls timed one by one with HIP events; prints one JSON line: median / min / max in us.

    FNR_LIB_PATH=... python tools/microbench/optimizer_sweeps.py [label]

profiles/optimizer_sweeps.md has the numbers this was written for."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from fruitnerf_amd import _kernels as K, _lib as L   # noqa: E402
from fruitnerf_amd.fruit_nerf import FruitModel, FruitNerfModelConfig   # noqa: E402
from fruitnerf_amd.data.semantics import apple_metadata   # noqa: E402

WARMUP, TIMED = 10, 50
B1, B2, EPS = 0.9, 0.999, 1e-15
dev = torch.device("cuda:0")


def state(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=g) * s).to(dev) for s in (0.1, 1e-3, 1e-3)] + [(torch.rand(n, generator=g) * 1e-6).to(dev)]


def leg(call):
    for _ in range(WARMUP):
        call()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(TIMED)]
    for a, b in pairs:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in pairs]
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def main():
    result = {"label": sys.argv[1] if len(sys.argv) > 1 else "", "lib": L.LIB_PATH}
    p, g, m, v = state(1 << 24, 0)
    result["adam_step 2^24"] = leg(lambda: K.adam_step(p, g, m, v, 1e-2, B1, B2, EPS, 10, 1.0, True))
    result["radam_step 2^24"] = leg(lambda: K.radam_step(p, g, m, v, 1e-2, B1, B2, EPS, 10, 1.0, True))
    del p, g, m, v
    model = FruitModel(FruitNerfModelConfig(), apple_metadata(), num_train_data=10, device=dev)
    model.train()
    arena = model.arena()
    n = arena.params.numel()
    p, g, m, v = state(n, 1)
    # the groups after warm-up: the proposal networks have taken fewer steps than the field, the rates differ
    spans = [(a, b - a, 1e-2 / (i + 1), 10 - 3 * i) for i, (a, b) in enumerate(arena.group_ranges.values())]
    result["arena floats"], result["spans"] = n, [s[:2] for s in spans]
    result["adam_step_spans arena"] = leg(lambda: K.adam_step_spans(p, g, m, v, spans, "adam", B1, B2, EPS, 1.0, True))
    steps = torch.tensor([s[3] for s in spans], dtype=torch.int64, device=dev)
    scalars = torch.zeros(L.FNR_ADAM_DEV_SCALAR_FLOATS, device=dev)
    dev_spans = [s[:3] for s in spans]
    result["adam_step_spans_dev arena"] = leg(lambda: K.adam_step_spans_dev(p, g, m, v, dev_spans, steps, "adam", B1, B2, EPS, scalars))
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
