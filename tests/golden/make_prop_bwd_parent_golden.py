"""What the proposal networks' backward (prop_bwd.hip: k_prop_bwd -> k_prop_reduce / k_prop_reduce2 -> the binned scatter)
computes, as bit patterns: for every case below a SHA-256 of the raw bytes of each result array (d_position and the gradients
of w0, b0, w1, b1 and the table; parameters and both moments for the calls that take the optimiser's step), recorded on the
commit BEFORE a change of the kernel body that is meant to keep every result bit:

    python -m tests.golden.make_prop_bwd_parent_golden      # writes tests/golden/prop_bwd_parent_digests.json

tests/test_gpu_prop_bwd_same_bits.py computes the same cases on the checked-out tree and compares, exactly.  The results are
deterministic by construction: a sample's d_feats and d_position depend on that sample alone, a wave's MFMA accumulators take
its samples in a fixed order, the four waves and then the workgroups' partial vectors are summed in a fixed order by one
writer, and the scatter sums in 64-bit fixed point.  The workgroup count is min(ceil(N / 256), 3 x CUs): the file records
the CU count, and the cases whose N is made from it (or exceeds it) hold on that CU count only.

Inputs: the networks, geometries and upstream gradients of tests/test_gpu_proposal_kernels.py (imported, CPU generators with
fixed seeds).  No float64 reference is needed for a digest, so _d_density gets a forward record without kink or near-lattice
samples: the same seeded values, none of them zeroed."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "prop_bwd_parent_digests.json")
LEVELS = (1, 2, 5, 7, 8)
SIZES = (1, 255, 256, 257, 1000, "cap")          # "cap": cap x 256 - 56, one pass per workgroup, the last one ragged
GRADS = ("table", "w0", "b0", "w1", "b1")
ADAM = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, step=3)


def _pk():
    from tests import test_gpu_proposal_kernels as pk
    return pk


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().view(-1).view(torch.int32).numpy().tobytes()).hexdigest()


def cus() -> int:
    from fruitnerf_amd import _lib as Lb
    return int(Lb.device_check()["cus"])


def _dd(geom, seed):
    """_d_density of the imported helpers on a record without kink / near-lattice samples (module docstring)."""
    n = geom["x"].shape[0]
    none = torch.zeros(n, dtype=torch.bool)
    return _pk()._d_density(dict(sel=_pk()._selector(geom["x"]), kink=none, near=none, n_near=0), seed)


def _size(n):
    cap = 3 * cus()
    return {"cap": cap * 256 - 56, "2cap": 2 * cap * 256 + 300}.get(n, n)


def single_case(L, N, posgrad):
    """fnr_prop_density_bwd into zero gradients: rays at N = 1000 (contracted positions, S = 25), points elsewhere."""
    def run(dev):
        pk = _pk()
        n = _size(N)
        net = pk._net(L)
        geom = pk._geometry("rays" if n == 1000 else "points", L, n, seed=3)
        got, _ = pk._kernel_backward(dev, net, geom, _dd(geom, 5 + L), want_position_grad=posgrad)
        return {k: v for k, v in got.items() if v is not None}
    return run


class _Arena:
    """Gradients, parameters and both moments of some networks as four flat device tensors with one layout, the way the
    optimiser's arenas hold them (fnr_prop_density_bwd_adam addresses the weights' parameters through the gradient arena)."""

    def __init__(self, nets, dev, seed):
        pk = _pk()
        self.spans, off = [], 0
        for net in nets:
            span = {}
            for k in GRADS:
                span[k] = (off, net[k].numel(), tuple(net[k].shape))
                off += (net[k].numel() + 63) // 64 * 64
            self.spans.append(span)
        g = torch.Generator().manual_seed(seed)
        params = torch.zeros(off)
        for net, span in zip(nets, self.spans):
            for k, (a, n, _) in span.items():
                params[a:a + n] = net[k].reshape(-1)
        self.params = params.to(dev)
        self.exp_avg = (1e-3 * torch.randn(off, generator=g)).to(dev)
        self.exp_avg_sq = (1e-6 * (0.1 + torch.rand(off, generator=g))).to(dev)
        self.grads = torch.zeros(off, device=dev)
        self.structs = [(pk._struct(net, dev, self.views(self.params, i)), pk._struct(net, dev, self.views(self.grads, i)))
                        for i, net in enumerate(nets)]

    def views(self, flat, i):
        return {k: flat[a:a + n].view(shape) for k, (a, n, shape) in self.spans[i].items()}

    def descriptors(self):
        from fruitnerf_amd import _lib as Lb
        h = ADAM

        def adam(p, m, v):
            return Lb.table_adam(0, h["lr"], h["beta1"], h["beta2"], h["eps"], h["step"], 1.0, 0.0, Lb.ptr(p), Lb.ptr(m), Lb.ptr(v), None)
        tables = []
        for span in self.spans:
            a, n, _ = span["table"]
            tables.append(adam(self.params[a:a + n], self.exp_avg[a:a + n], self.exp_avg_sq[a:a + n]))
        return tables, adam(self.params, self.exp_avg, self.exp_avg_sq)

    def results(self):
        return {"parameters": self.params, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "gradient arena": self.grads}


def adam_case(L, kind, N):
    """fnr_prop_density_bwd_adam -> d_position and the arenas after the step."""
    def run(dev):
        from fruitnerf_amd import _kernels as K
        pk = _pk()
        net = pk._net(L)
        geom = pk._geometry(kind, L, N, seed=4)
        dd = _dd(geom, 11 + L)
        arena = _Arena([net], dev, 100 + L)
        tables, weights = arena.descriptors()
        D = pk._device_side(net, geom, dev)
        (pn, gn), = arena.structs
        _, feats = K.prop_density_fwd(pn, D["warp"], D["rays"], D["euclid"], geom["S"], save_feats=True)
        d_pos = K.prop_density_bwd(pn, gn, D["warp"], D["rays"], D["euclid"], geom["S"], feats, dd.to(dev).contiguous(),
                                   want_position_grad=True, adam=(tables[0], weights, arena.grads))
        torch.cuda.synchronize()
        return dict(arena.results(), d_position=d_pos)
    return run


def pair_case(split, fused):
    """fnr_prop_density_bwd_pair / _pair_split on an L = 5 and an L = 7 level that share 40 rays (S = 25 and 17) -> both
    d_position and the gradients (or, with the optimiser's step, the arenas)."""
    def run(dev):
        from fruitnerf_amd import _kernels as K
        pk = _pk()
        nets = [pk._net(5), pk._net(7)]
        geoms = [pk._rays(40, 25, seed=6), pk._rays(40, 17, seed=6)]
        dds = [_dd(g, 31 + i).to(dev).contiguous() for i, g in enumerate(geoms)]
        arena = _Arena(nets, dev, 57)
        Ds = [pk._device_side(n, g, dev) for n, g in zip(nets, geoms)]
        pns, gns = [s[0] for s in arena.structs], [s[1] for s in arena.structs]
        feats = [K.prop_density_fwd(pn, D["warp"], D["rays"], D["euclid"], g["S"], save_feats=True)[1]
                 for pn, D, g in zip(pns, Ds, geoms)]
        adam = None
        if fused:
            tables, weights = arena.descriptors()
            adam = (tables, weights, arena.grads)
        d_pos = K.prop_density_bwd_pair(pns, gns, [D["warp"] for D in Ds], Ds[0]["rays"], [D["euclid"] for D in Ds],
                                        [g["S"] for g in geoms], feats, dds, want_position_grad=True, adam=adam,
                                        position_ready=K.Event() if split else None)
        torch.cuda.synchronize()
        out = {"d_position[0]": d_pos[0], "d_position[1]": d_pos[1]}
        if fused:
            out.update(arena.results())
        else:
            for q in range(2):
                out.update({f"grad of {k}[{q}]": v for k, v in arena.views(arena.grads, q).items()})
        return out
    return run


def _cases():
    c, cap_bound = {}, set()
    for L in LEVELS:
        for posgrad in (True, False):
            for N in SIZES + (("2cap",) if L == 5 else ()):     # "2cap": 2 cap 256 + 300, two and three passes, ragged tail late
                name = f"L={L} N={N} position gradient {'on' if posgrad else 'off'}"
                c[name] = single_case(L, N, posgrad)
                if isinstance(N, str):
                    cap_bound.add(name)
    c["adam L=5 rays N=1000"] = adam_case(5, "rays", 1000)
    c["adam L=7 points N=257"] = adam_case(7, "points", 257)
    for split in (False, True):
        for fused in (False, True):
            c[f"pair{'_split' if split else ''} L=5,7{' adam' if fused else ''}"] = pair_case(split, fused)
    return c, cap_bound


CASES, CAP_BOUND = _cases()


def compute(case: str, dev) -> dict:
    """One case on `dev` -> {array name: sha256}."""
    from fruitnerf_amd import _lib as Lb
    Lb.scatter_overflows(reset=True)
    out = {k: digest(v) for k, v in CASES[case](dev).items()}
    assert Lb.scatter_overflows(reset=True) == 0, f"{case}: a queue overflowed — the table's result is not bit-defined"
    return out


def main(argv) -> int:
    out = argv[1] if len(argv) > 1 else FIXTURE
    dev = torch.device("cuda:0")
    result = {"cus": cus(), "cases": {}}
    for case in CASES:
        result["cases"][case] = compute(case, dev)
        print(f"[prop bwd golden] {case}: " + ", ".join(f"{k} {v[:10]}" for k, v in result["cases"][case].items()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write('{"cus": %d, "cases": {\n' % result["cus"] +
                ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in result["cases"].items()) + "\n}}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
