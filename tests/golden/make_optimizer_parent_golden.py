"""What the optimiser sweeps (fnr_adam_step, fnr_radam_step, fnr_adam_step_spans, fnr_adam_step_spans_dev) compute, as bit
patterns: for every case below a SHA-256 of the raw bytes of the parameters, exp_avg, exp_avg_sq and the gradient after the
call (and of the device step counters for the _dev entry point) — one digest per array and case, taken over the case's calls
in their order — recorded on the commit BEFORE a change of the sweeps that is meant to keep every result bit:

    python -m tests.golden.make_optimizer_parent_golden      # writes tests/golden/optimizer_parent_digests.json

tests/test_gpu_optimizer_same_bits.py computes the same cases on the checked-out tree and compares, exactly.  The results
are deterministic by construction: every element is read and written by one thread, from its own four values and the
span's scalars; nothing is summed across threads, so neither the grid nor the CU count enters.

Inputs: _update_inputs of tests/test_gpu_hash_scatter.py (imported; CPU generator, fixed seeds, random moments)."""
import functools
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "optimizer_parent_digests.json")
LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8
# float4 counts of the whole-buffer entry points: one thread, one partial wave, one short of / one past a workgroup, and the
# first size at which the grid-stride loop (at most 8192 workgroups of 256) takes a second trip
N4 = (1, 3, 255, 257, 8192 * 256 + 5)
STEPS = {"adam": (1, 1000), "radam": (1, 5, 6)}     # RAdam with beta2 = 0.999: 5 is the last unrectified step, 6 the first rectified
OPTIONS = tuple(itertools.product((0, 1), (0.0, 1e-2), (1.0, 0.5)))      # zero_grad x weight_decay x grad_scale
ARENA = 1 << 16
# (offset, count, lr, step), offsets and counts multiples of 4
SPAN_SETS = {
    "1 span": [(64, 4100, 1e-2, 6)],
    "8 spans with gaps": [(0, 4, 6e-4, 1), (8, 1020, 1e-2, 5), (1032, 1024, 3e-3, 6), (4096, 1028, 1e-3, 1000), (8192, 12, 2e-2, 2),
                          (8300, 20000, 5e-4, 7), (30000, 4, 1e-2, 3), (40000, 25536, 1e-4, 6)],
    "a span of count 0 in the middle": [(128, 2052, 1e-2, 5), (4096, 0, 1e-3, 9), (8192, 1000, 3e-3, 6)],
    "2 spans adjacent": [(256, 1028, 1e-2, 1), (1284, 2048, 5e-3, 6)],
}
SPAN_OPTIONS = ((1, 0.0, 1.0), (0, 1e-2, 0.5))          # zero_grad, weight_decay, grad_scale
DEV_OPTIONS = tuple(itertools.product((None, 0.0, 1.0), (None, 1024.0), (0, 1)))   # found_inf x grad_scale x zero_grad
ARRAYS = ("parameters", "exp_avg", "exp_avg_sq", "gradient")


class Digests:
    """One SHA-256 per array name over the raw bytes of that array after every call of a case, in the order of the calls."""

    def __init__(self, names):
        self.h = {name: hashlib.sha256() for name in names}

    def add(self, tensors):
        for h, t in zip(self.h.values(), tensors):
            h.update(t.detach().contiguous().cpu().numpy().tobytes())

    def hex(self):
        return {name: h.hexdigest() for name, h in self.h.items()}


def rectified(beta2: float, step: int) -> bool:
    """torch.optim.RAdam's rho_t > 5, from the float32 beta2 in double as the library derives it."""
    b2 = float(np.float32(beta2))
    b2t = b2 ** step
    rho_inf = 2.0 / (1.0 - b2) - 1.0
    return rho_inf - 2.0 * step * b2t / (1.0 - b2t) > 5.0


@functools.lru_cache(maxsize=2)
def _inputs(n: int):
    from tests.test_gpu_hash_scatter import _update_inputs
    return _update_inputs(n, 900 + n % 97, "random")


def step_case(algorithm, step, n4):
    """fnr_adam_step / fnr_radam_step over 4 n4 floats, every combination of OPTIONS."""
    def run(dev):
        from fruitnerf_amd import _kernels as K
        fn = K.adam_step if algorithm == "adam" else K.radam_step
        out = Digests(ARRAYS)
        for zero_grad, wd, gs in OPTIONS:
            d = [t.to(dev) for t in _inputs(4 * n4)]
            fn(d[0], d[1], d[2], d[3], LR, B1, B2, EPS, step, gs, bool(zero_grad), wd)
            torch.cuda.synchronize()
            assert bool(d[1].any()) != bool(zero_grad)
            out.add(d)
        return out.hex()
    return run


def spans_case(algorithm, name):
    """fnr_adam_step_spans over SPAN_SETS[name] of one arena, both SPAN_OPTIONS."""
    def run(dev):
        from fruitnerf_amd import _kernels as K
        out = Digests(ARRAYS)
        for zero_grad, wd, gs in SPAN_OPTIONS:
            d = [t.to(dev) for t in _inputs(ARENA)]
            K.adam_step_spans(d[0], d[1], d[2], d[3], SPAN_SETS[name], algorithm, B1, B2, EPS, grad_scale=gs,
                              zero_grad=bool(zero_grad), weight_decay=wd)
            torch.cuda.synchronize()
            out.add(d)
        return out.hex()
    return run


def spans_dev_case(algorithm, name):
    """fnr_adam_step_spans_dev over SPAN_SETS[name], two consecutive calls for every combination of DEV_OPTIONS; the counters
    start one below the spans' steps, so that the first call takes the steps of the host-scalar case.  A skipped step
    (found_inf = 1) is checked here as well as digested: parameters, moments and counters as they were, the gradient zero
    inside the spans with zero_grad and as it was without."""
    def run(dev):
        from fruitnerf_amd import _kernels as K, _lib as L
        spans = SPAN_SETS[name]
        inside = torch.zeros(ARENA, dtype=torch.bool)
        for a, cnt, _, _ in spans:
            inside[a:a + cnt] = True
        out = Digests(ARRAYS + ("steps",))
        for found_inf, scale, zero_grad in DEV_OPTIONS:
            host = list(_inputs(ARENA))
            if scale is not None:
                host[1] = host[1] * scale
            d = [t.to(dev) for t in host]
            steps0 = torch.tensor([s - 1 for _, _, _, s in spans], dtype=torch.int64)
            steps = steps0.to(dev)
            scalars = torch.zeros(L.FNR_ADAM_DEV_SCALAR_FLOATS, device=dev)
            gs = None if scale is None else torch.tensor([scale], device=dev)
            fi = None if found_inf is None else torch.tensor([found_inf], device=dev)
            for call in (1, 2):
                K.adam_step_spans_dev(d[0], d[1], d[2], d[3], [s[:3] for s in spans], steps, algorithm, B1, B2, EPS, scalars,
                                      grad_scale=gs, found_inf=fi, zero_grad=bool(zero_grad), weight_decay=1e-2)
                torch.cuda.synchronize()
                if found_inf:
                    assert all(torch.equal(d[q].cpu(), host[q]) for q in (0, 2, 3)) and torch.equal(steps.cpu(), steps0)
                    g = d[1].cpu()
                    assert torch.equal(g[~inside], host[1][~inside])
                    assert not bool(g[inside].any()) if zero_grad else torch.equal(g, host[1])
                else:
                    assert torch.equal(steps.cpu(), steps0 + call)
                out.add(d + [steps])
        return out.hex()
    return run


def _cases():
    c = {}
    for algorithm, steps in STEPS.items():
        for step in steps:
            for n4 in N4:
                c[f"{algorithm}_step step {step} n4 {n4}"] = step_case(algorithm, step, n4)
    for algorithm in STEPS:
        for name in SPAN_SETS:
            c[f"adam_step_spans {algorithm} {name}"] = spans_case(algorithm, name)
            c[f"adam_step_spans_dev {algorithm} {name}"] = spans_dev_case(algorithm, name)
    return c


CASES = _cases()


def compute(case: str, dev) -> dict:
    """One case on `dev` -> {array name: sha256}."""
    return CASES[case](dev)


def main(argv) -> int:
    out = argv[1] if len(argv) > 1 else FIXTURE
    dev = torch.device("cuda:0")
    result = {}
    for case in CASES:
        result[case] = compute(case, dev)
        print(f"[optimizer golden] {case}: " + ", ".join(f"{k} {v[:10]}" for k, v in result[case].items()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write('{"cases": {\n' + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in result.items()) + "\n}}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
