"""What the field MLP's backward (fnr_field_mlp_bwd, _rays, _adam, _semgrad: field_mlp_bwd.hip and the branch kernels it runs)
computes, as bit patterns: for every case below a SHA-256 of the raw bytes of each result — d_feats, d_position where a
Jacobian is given, the gradient arena (every weight, bias and embedding gradient), and for the calls that take the
optimiser's step the parameters and both moments — recorded on the commit BEFORE a change that is meant to keep every bit:

    python -m tests.golden.make_field_mlp_bwd_parent_golden      # writes tests/golden/field_mlp_bwd_parent_digests.json

tests/test_gpu_field_mlp_bwd_same_bits.py computes the same cases on the checked-out tree and compares, exactly.

Inputs: the networks, batches and upstream gradients of tests/field_reference.py and the device side of
tests/test_gpu_field_kernels.py (imported: seeded CPU generators).  No float64 reference is needed for a digest, so no
sample is excluded: make_upstream's values as they are.  Parameters, gradients and moments live in four flat arenas of one
layout, the way the optimiser holds them (the fused step addresses a parameter through its gradient's address).

A case is (shape, arithmetic, size) and runs ten calls: five call forms — plain, _rays, _adam with the Jacobian, _semgrad
bare, _semgrad with the Jacobian and the optimiser's step — each with the forward pass's saved workspace (h, ray bias,
fragment images) and with a bare h (ray bias and images recomputed by the backward).
Sizes (R, S), the smallest at which the launch path can differ: (1, 16) one tile, one workgroup; (5, 16) an odd tile count,
the two-tile wave group is ragged; (6, 24) tiles straddle rays: gsum_extra and its memset; "cap": N just above 512 x CUs
(field_reference.grid_stride_shape, the size rule of test_grid_stride_second_pass), some waves take a second pass.  The file
records the CU count; the "cap" cases hold on that CU count only.

Why the bits are reproducible: every sum has a fixed order and a single writer, except the float atomics into gsum_extra
(tiles that straddle rays, S % 16 != 0).  In the bf16 modes a straddling tile adds ONE value per ray and slot, and for
S >= 16 a ray has at most two such tiles: at most two adds onto zero, which commute.  The fp32 colour kernel adds per
SAMPLE instead (k_field_mlp_bwd_color: one atomicAdd per valid lane of a straddling tile), so a slot's value is
order-free only while ONE wave instruction feeds it: with S = 24 every ray has exactly one straddling tile (S % 16 = 8: its
first or its last eight samples), and the lanes of one instruction are combined in the hardware's own, fixed order — the
self-check below sees that, as tests/test_gpu_field_kernels.py::test_structure_in_every_arithmetic has at S = 40.  That is
why the "cap" case keeps grid_stride_shape's N rule but takes S = 24 and not its S = 41, where a ray can have two
straddling tiles from two waves.
Excluded: S < 16, the per-sample query path, puts the adds of many tiles into one slot and is not bit-reproducible; it
stays covered by the float64 tests of tests/test_gpu_field_kernels.py ((37, 1), (21, 8) and test_nothing_is_written_past_n).

Self-check: every case is computed twice here, and a digest that differs between the two runs is not written."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "field_mlp_bwd_parent_digests.json")
MODES = ("fp32", "bf16x3", "bf16")
SIZES = ((1, 16), (5, 16), (6, 24), "cap")
CAP_S = 24
# (name, jacobian, optimiser's step, semgrad) -> fnr_field_mlp_bwd | _rays | _adam | _semgrad | _semgrad
FORMS = (("plain", False, False, False), ("rays", True, False, False), ("adam + jacobian", True, True, False),
         ("semgrad", False, False, True), ("semgrad + jacobian + adam", True, True, True))
ADAM = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, step=3)


def _fk():
    from tests import test_gpu_field_kernels as fk
    return fk


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().view(-1).view(torch.int32).numpy().tobytes()).hexdigest()


def cus() -> int:
    from fruitnerf_amd import _lib as Lb
    return int(Lb.device_check()["cus"])


def size(rs):
    """(R, S) of a case; "cap": the smallest odd R with R x 24 at or above grid_stride_shape's N (R odd: N % 16 = 8, so N is
    no multiple of any kernel's pass and the last tile is ragged)."""
    if rs != "cap":
        return rs
    from tests import field_reference as fr
    R41, S41, passes = fr.grid_stride_shape(cus())
    R = (R41 * S41 + CAP_S - 1) // CAP_S
    R += 1 - R % 2
    assert all(R * CAP_S > p and (R * CAP_S) % p != 0 for p in passes.values())
    return R, CAP_S


class Arenas:
    """The device side of test_gpu_field_kernels.Device with its parameters and gradients re-homed in flat arenas of one
    layout (64-float aligned spans), next to seeded moments; `reset` puts every arena back to its first state."""

    def __init__(self, dev, net, batch, mode):
        D = self.D = _fk().Device(dev, net, batch, mode)
        keys = [(k, i) for k in D.names for i in range(2)] + [("embedding", None)]
        tensor = lambda t, key: t[key[0]] if key[1] is None else t[key[0]][key[1]]   # noqa: E731
        self.spans, off = {}, 0
        for key in keys:
            t = tensor(D.par, key)
            self.spans[key] = (off, t.numel(), tuple(t.shape))
            off += (t.numel() + 63) // 64 * 64
        g = torch.Generator().manual_seed(4711)
        first = torch.zeros(off)
        for key, (a, n, _) in self.spans.items():
            first[a:a + n] = tensor(D.par, key).cpu().reshape(-1)
        self.first = {"parameters": first.to(dev), "exp_avg": (1e-3 * torch.randn(off, generator=g)).to(dev),
                      "exp_avg_sq": (1e-6 * (0.1 + torch.rand(off, generator=g))).to(dev), "gradients": torch.zeros(off, device=dev)}
        self.flat = {k: v.clone() for k, v in self.first.items()}

        def views(flat):
            out = {k: tuple(flat[a:a + n].view(sh) for a, n, sh in (self.spans[(k, 0)], self.spans[(k, 1)])) for k in D.names}
            a, n, sh = self.spans[("embedding", None)]
            out["embedding"] = flat[a:a + n].view(sh)
            return out
        D.par, D.grad = views(self.flat["parameters"]), views(self.flat["gradients"])
        D.c_net, D.c_grad = D._struct(D.par), D._struct(D.grad)

    def reset(self):
        for k, v in self.flat.items():
            v.copy_(self.first[k])

    def weight_adam(self):
        from fruitnerf_amd import _lib as Lb
        h, f = ADAM, self.flat
        adam = Lb.table_adam(0, h["lr"], h["beta1"], h["beta2"], h["eps"], h["step"], 1.0, 0.0, Lb.ptr(f["parameters"]),
                             Lb.ptr(f["exp_avg"]), Lb.ptr(f["exp_avg_sq"]), None)
        return adam, f["gradients"]


def _case(shape, mode, rs):
    def run(dev):
        from fruitnerf_amd import _kernels as K
        from tests import field_reference as fr
        fk = _fk()
        R, S = size(rs)
        net, batch = fr.make_net(shape), fr.make_batch(R, S)
        up = {k: v.to(dev).contiguous() for k, v in fr.make_upstream(batch).items()}
        A = Arenas(dev, net, batch, mode)
        D = A.D
        _, saved = D.forward()
        jac = fk._jacobian(batch, dev)
        out = {}
        for form, with_jac, fused, semgrad in FORMS:
            for ws_name, h_saved in (("saved forward workspace", saved), ("bare h", saved[0])):
                A.reset()
                got = K.field_mlp_bwd(D.c_net, D.c_grad, D.rays, S, D.feats, h_saved, D.sel, up["dd"], up["dr"], up["dl"],
                                      jacobian=jac if with_jac else None, weight_adam=A.weight_adam() if fused else None,
                                      semgrad=semgrad)
                torch.cuda.synchronize()
                res = {"d_feats": got[0] if with_jac else got, "gradients": A.flat["gradients"]}
                if with_jac:
                    res["d_position"] = got[1]
                if fused:
                    res.update({k: A.flat[k] for k in ("parameters", "exp_avg", "exp_avg_sq")})
                out.update({f"{form}, {ws_name}: {k}": digest(v) for k, v in res.items()})
        return out
    return run


def _cases():
    from tests import field_reference as fr
    c, cap_bound = {}, set()
    for shape in fr.SHAPES:
        for mode in MODES:
            for rs in SIZES:
                name = f"{shape} {mode} " + ("cap" if rs == "cap" else "R=%d S=%d" % rs)
                c[name] = _case(shape, mode, rs)
                if rs == "cap":
                    cap_bound.add(name)
    return c, cap_bound


CASES, CAP_BOUND = _cases()


def compute(case: str, dev) -> dict:
    """One case on `dev` -> {call form, workspace: array name -> sha256}."""
    return CASES[case](dev)


def main(argv) -> int:
    out = argv[1] if len(argv) > 1 else FIXTURE
    dev = torch.device("cuda:0")
    result = {"cus": cus(), "cases": {}}
    for case in CASES:
        first, second = compute(case, dev), compute(case, dev)
        differ = [k for k in first if first[k] != second[k]]
        if differ:
            print(f"[field mlp bwd golden] {case}: not reproducible, nothing written: {differ}", flush=True)
            return 1
        result["cases"][case] = first
        print(f"[field mlp bwd golden] {case}: {len(first)} digests, " + " ".join(v[:6] for v in list(first.values())[:8]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write('{"cus": %d, "cases": {\n' % result["cus"] +
                ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in result["cases"].items()) + "\n}}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
