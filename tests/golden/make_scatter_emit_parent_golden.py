"""What the binned hash-grid scatter (hash_scatter.hip: k_scatter_emit -> k_scatter_accumulate) computes, as bit patterns: for
every case below a SHA-256 of each result array (gradient tables; parameters and both moments for the fused calls; the
proposal pair's gradients and d_position) with two integer sums, recorded on the commit BEFORE a change that is meant to keep
every result bit:

    python -m tests.golden.make_scatter_emit_parent_golden      # writes tests/golden/scatter_emit_parent.json

tests/test_gpu_scatter_emit_same_bits.py computes the same cases on the checked-out tree and compares, exactly.  The results
are deterministic by construction (the accumulate kernel sums in 64-bit fixed point, every table row has one writer, record
order inside a queue does not matter), so a digest is a fair yardstick; overflowing queues (float atomics in arbitrary order)
are not, and are left to the bounded tests of tests/test_gpu_hash_scatter.py.

Inputs: the grids, geometries and feature gradients of tests/test_gpu_hash_scatter.py (imported, CPU generators with fixed
seeds), the proposal pair on a FruitModel whose proposal parameters are overwritten from a CPU generator."""
import contextlib
import functools
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "scatter_emit_parent.json")
PAIR_RAYS = 64


def digest(t: torch.Tensor) -> dict:
    """SHA-256 of the array's 32-bit words, how many of them are non-zero, and their sum mod 2^64."""
    words = t.detach().contiguous().cpu().view(-1).view(torch.int32).numpy().view("uint32")
    return {"sha256": hashlib.sha256(words.tobytes()).hexdigest(), "words": int(words.size),
            "nonzero": int((words != 0).sum()), "sum": int(words.astype("uint64").sum(dtype="uint64"))}


@contextlib.contextmanager
def emit_lpb(value):
    """FNR_EMIT_LPB (levels per emit workgroup; the library reads it at every call) for the length of a case."""
    saved = os.environ.get("FNR_EMIT_LPB")
    if value is not None:
        os.environ["FNR_EMIT_LPB"] = str(value)
    try:
        yield
    finally:
        if saved is None:
            os.environ.pop("FNR_EMIT_LPB", None)
        else:
            os.environ["FNR_EMIT_LPB"] = saved


def _hs():
    from tests import test_gpu_hash_scatter as hs
    return hs


def scatter_case(grid_name, kind, N, lpb=None, per_level=False):
    """fnr_hash_encode_bwd into a zero table -> {"table"}."""
    def run(dev):
        hs = _hs()
        grid = hs._grid(grid_name)
        geom = hs._runs() if kind == "runs" else hs._geom(kind, N, seed=len(grid_name))
        df = hs._d_feats(len(grid[1]), geom, grid[1], 3 + N)
        calls = [(l, 1) for l in range(len(grid[1]))] if per_level else None
        with emit_lpb(lpb):
            return {"table": hs._scatter(dev, grid, geom, df, calls=calls)}
    return run


def fused_case(N, case_index=1):
    """fnr_hash_encode_bwd_adam on small16 from a random state -> parameters, both moments, the gradient table (left zero).
    N = 0: the same buffers with no rays (every row still takes its step)."""
    def run(dev):
        hs = _hs()
        grid = hs._grid("small16")
        geom = hs._geom("points", N if N else 1000, seed=7)
        df = hs._d_feats(16, geom, grid[1], 41 + N)
        n = (len(grid[1]) << grid[0]) * 2
        g = torch.Generator().manual_seed(1000 + N)
        state = dict(p=(0.1 * torch.randn(n, generator=g)).to(dev), m=(1e-3 * torch.randn(n, generator=g)).to(dev),
                     v=(1e-6 * (0.1 + torch.rand(n, generator=g))).to(dev))
        out = hs._fused(dev, grid, geom, df, hs.ADAM_CASES[case_index], state, N=(0 if N == 0 else None))
        return {"parameters": out["p"], "exp_avg": out["m"], "exp_avg_sq": out["v"], "gradient table": out["g"]}
    return run


@functools.lru_cache(maxsize=None)
def _pair_model(dev):
    from fruitnerf_amd.data.semantics import apple_metadata
    from fruitnerf_amd.fruit_nerf import FruitModel, FruitNerfModelConfig
    from fruitnerf_amd.training import FusedAdam
    torch.manual_seed(0)
    model = FruitModel(FruitNerfModelConfig(), apple_metadata(), num_train_data=16, device=dev)
    model.train()
    arena = model.arena()
    arena.reattach_grads()
    opt = FusedAdam(model)
    a, b = arena.group_ranges["proposal_networks"]
    with torch.no_grad():     # trained-like tables and weights, the same on every machine
        arena.params[a:b].copy_(((torch.rand(b - a, generator=torch.Generator().manual_seed(77)) * 2 - 1) * 0.5).to(dev))
    return model, arena, opt


def pair_case(S):
    """fnr_prop_density_bwd_pair_split (gradients, no optimiser) of the two `fruit_nerf` proposal networks on PAIR_RAYS rays
    with S = (samples of level 0, of level 1) -> the networks' gradient span (tables and weights) and both d_position."""
    def run(dev):
        from fruitnerf_amd import _kernels as K
        from tests import util
        model, arena, _ = _pair_model(dev)
        nets = list(model.proposal_networks)
        R = PAIR_RAYS
        a, b = arena.group_ranges["proposal_networks"]
        g = torch.Generator().manual_seed(7 + S[0])
        o, d, _, cam = util.random_rays(R, 16, seed=3)
        rays = K.RaysArg(o.to(dev), d.to(dev), torch.full((R, 1), 0.05, device=dev), torch.full((R, 1), 1000.0, device=dev),
                         cam.to(dev))
        spacing, euclid0 = K.sample_spaced(rays, 1, S[0], torch.rand(R, generator=g).to(dev))
        dens0, feats0 = K.prop_density_fwd(nets[0].prop_struct(), nets[0].warp_struct(), rays, euclid0, S[0], save_feats=True)
        _, _, _, euclid1 = K.weights_pdf(rays, 1, S[0], S[1], dens0, spacing, euclid0, 1.0, torch.rand(R, generator=g).to(dev))
        _, feats1 = K.prop_density_fwd(nets[1].prop_struct(), nets[1].warp_struct(), rays, euclid1, S[1], save_feats=True)
        dd = [(1e-2 * torch.randn(R, s, generator=g)).to(dev) for s in S]
        arena.grads[a:b].zero_()
        d_pos = K.prop_density_bwd_pair([n.prop_struct() for n in nets], [n.prop_struct(grads=True) for n in nets],
                                        [n.warp_struct() for n in nets], rays, [euclid0, euclid1], list(S), [feats0, feats1], dd,
                                        want_position_grad=True, adam=None, position_ready=K.Event())
        torch.cuda.synchronize()
        return {"gradients": arena.grads[a:b].clone(), "d_position[0]": d_pos[0], "d_position[1]": d_pos[1]}
    return run


def _cases():
    c = {}
    for N in (1, 511, 512, 513, 1000, 2100):
        c[f"small16 points N={N}"] = scatter_case("small16", "points", N)
    for N in (1, 511, 1000, 2100):          # rays come in multiples of 48: 511, 512 and 513 are the same 528 samples
        c[f"small16 rays N={N}"] = scatter_case("small16", "rays", N)
    for lpb in (1, 2, 16):
        c[f"small16 points N=1000 FNR_EMIT_LPB={lpb}"] = scatter_case("small16", "points", 1000, lpb=lpb)
    # (the runs geometry on small16 is left out: its blocks of samples in one coarse cell overflow a 1024-record queue at the
    #  middle levels, where they share a bin but no longer a cell — not bit-defined; tests/test_gpu_hash_scatter.py bounds it)
    c["rows8k runs"] = scatter_case("rows8k", "runs", 1200)
    c["edge2 points N=1000, one call per level"] = scatter_case("edge2", "points", 1000, per_level=True)
    c["edge2 rays N=1000, one call per level"] = scatter_case("edge2", "rays", 1000, per_level=True)
    for name in ("rows8k", "bins64", "bins256", "tiny6", "tiny10"):
        c[f"{name} points N=1000"] = scatter_case(name, "points", 1000)
    c["fused radam N=0"] = fused_case(0, case_index=3)
    c["fused adam N=513"] = fused_case(513)
    c["fused adam N=2100"] = fused_case(2100)
    c["proposal pair split S=(32,16)"] = pair_case((32, 16))
    c["proposal pair split S=(16,32)"] = pair_case((16, 32))
    return c


CASES = _cases()


def compute(case: str, dev) -> dict:
    """One case on `dev` -> {array name: digest}."""
    from fruitnerf_amd import _lib as L
    L.scatter_overflows(reset=True)
    out = {k: digest(v) for k, v in CASES[case](dev).items()}
    assert L.scatter_overflows(reset=True) == 0, f"{case}: a queue overflowed — the result is not bit-defined"
    return out


def main(argv) -> int:
    out = argv[1] if len(argv) > 1 else FIXTURE
    dev = torch.device("cuda:0")
    result = {}
    for case in CASES:
        try:
            result[case] = compute(case, dev)
        except AssertionError as e:     # no digest for this case: take it out of CASES and say so in the test's docstring
            print(f"[scatter emit golden] NOT RECORDED: {e}", flush=True)
            continue
        print(f"[scatter emit golden] {case}: " + ", ".join(f"{k} {v['sha256'][:12]} ({v['nonzero']} non-zero words)"
                                                           for k, v in result[case].items()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in result.items())
                + "\n}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
