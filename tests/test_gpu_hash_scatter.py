"""The field hash table's backward — fnr_hash_encode_bwd and fnr_hash_encode_bwd_adam (hash_scatter.hip: k_scatter_emit,
k_scatter_accumulate) with the optimiser sweeps behind them (fnr_adam_step, fnr_radam_step) — against a float64 reference
written in plain torch, per table row and feature and per parameter / moment entry, never against a batch maximum or a
column sum.  The hash-grid reference is the one of tests/test_gpu_proposal_kernels.py (_encode: corners from ceil / floor
of x * scaling in the oracle's order, HashEncoding.hash_fn's hash, weights from scaled - floor), imported unchanged.

Reference.  Samples x (float32, upcast; unselected samples — a coordinate outside (0, 1) — encoded at position 0, as the
kernel and the oracle do: row hash(0,0,0) = 0 of every level with weight 1, their d_feats non-zero), d_feats [L,N,2]
(float32, upcast): table_grad[l T + idx[l,n,k], j] += W[l,n,k] d_feats[l,n,j] by index_add_ in float64.

Geometries.  POINTS: warp mode 1, unit box, S = 1, zero directions, origins = x, so x reaches the kernel bit for bit; the
28 edge samples of _points are in (N >= 255); no sample is left out (where fl32(x s) rounds onto an integer the float64
product misses the records are continuous, the u sc term below covers it, and the kernel's non-zero records go to a subset
of the reference's rows).  RAYS: warp mode 0, _rays(R, 48) with R = ceil(N / 48); samples within 4 ulp of a lattice plane
get d_feats = 0, at most 3 % of N (asserted).  RUNS (points): blocks of 2, 15, 16, 17, 33, 64, 65, 513 consecutive samples
jittered inside one cell of the coarsest level, laid across a 16-lane row, a wave and a 512-sample workgroup boundary, the
last one ending on the last valid sample of a ragged workgroup; at the fine levels the same samples sit in cells of their own.

Grids (built with K.make_grid, no model): small16 2^14 x hash_scalings(16, 16, 2048) (32 bins of 512 rows: the whole call
emits per corner, its coarse level groups by corner pairs), big16 2^14 x hash_scalings(16, 16, 4096) (scaling 4095), edge2
2^14 x [511, 512] called once per level (last scaling on the pair path, first off it), rows8k 2^18 x [16, 300, 2048, 4095]
(8192-row bins), bins64 2^19 x [64, 2048], bins256 2^21 x [16, 4095] (SC_MAX_BINS), tiny 2^6 and 2^10 x [16, 37] (2- and
32-row bins).  N = 1, 511, 512, 513, 1000, 2100 on small16, 1000 elsewhere.

Error model, u = 2^-24 (the proposal tests' table bound without an upstream-error term: d_feats is an input):
  bound(row, j) = C_TAB sum_records (u W_k |df_j| + |df_j| sum_a W'_a,k u sc_a) + cnt_row 2^(nb + e_l - 56),   C_TAB = 8
  the first term: the weight's and the product's roundings and the pre-summed runs; the second: fl32(x s) carries
  |d sc| <= u sc, the weight is multilinear in the offsets; the third: the scatter's 64-bit block fixed point — a record is
  rounded to 2^-S, S = 62 - nb - e, n < 2^nb the bin's records (<= 8 N), vmax < 2^e the LEVEL's largest emitted value: e_l
  of the reference's largest record + 1 + 6 for pre-summed runs.
  accumulate test: + u |prefill + ref| outside the constant (the final rounding of prefill + sum).
  overflow test: rows of a level some queue of which overflowed are summed in part by float atomics in arbitrary order:
  cnt_row u sum|records| (recursive summation) in place of the fixed-point term.
The constant is not tuned against the kernel: the same reference evaluated in float32 on the CPU over this module's own
inputs stays <= 1/4 of the bound, which leaves the kernel 4x for its other order of summation.

The optimiser update (test 9), per entry, hyper-parameters as the float32 values the kernels get, g' = g grad_scale + wd p:
  E_g = u |g grad_scale| (+ u (|wd p| + |g'|) with weight decay)
  E_m = (1 - b1) E_g + u (2 (1 - b1) |g' - m| + |m'|)                                       m' = m + (g' - m)(1 - b1)
  E_v = u |v b2| + (1 - b2) (2 |g'| E_g + 2 u g'^2) + u |v'|                                v' = v b2 + (1 - b2) g'^2
  E_r = E_v / (2 sqrt(v')) + u sqrt(v')                                                     sqrtf
  Adam   den = sqrt(v') / sqrt(bc2) + eps:  E_den = (E_r + 2 u sqrt(v')) / sqrt(bc2) + u den
         upd = (lr / bc1) m' / den:          E_p = (lr / bc1) (E_m / den + |m'| E_den / den^2) + 4 u |upd| + u |p'|
  RAdam  mhat = m' / bc1, rectified (rho_t > 5) ad = sqrt(bc2) / (sqrt(v') + eps), upd = lr mhat rect ad:
         E_p = lr rect (ad (E_m / bc1 + 2 u |mhat|) + |mhat| ad (2 u + (E_r + u (sqrt(v') + eps)) / (sqrt(v') + eps)))
               + 4 u |upd| + u |p'|;      not rectified (upd = lr mhat): E_p = lr (E_m / bc1 + 2 u |mhat|) + u |upd| + u |p'|
  bounds C_P E_p, C_M E_m, C_V E_v.  E is a first-order bound that single roundings attain (an entry without a gradient:
  m' = 0.9 m is one product and one sum): the float32 CPU evaluation of the same update reaches 1.00 E_p, 0.95 E_m, 0.98 E_v,
  so C_P = C_M = C_V = 4 puts it at 1/4.  The kernels take the same operations in the same order; division and sqrtf may
  round differently.
  fnr_adam_step / fnr_radam_step take multiples of 4 entries (one float4 per thread): n = 1, 3, 255, 1025 float4s.

Worst |err| / bound over every test of this file, [CPU float32, MI355X] (every assertion is worst <= 1):
  table gradient, points / rays, every grid     [0.20, 0.20]
  runs geometry                                 [0.12, 0.12]
  dynamic range 2^+-20                          [0.20, 0.20]
  overflow, per row                             [0.046, 0.046]
  accumulate into a prefilled table             [0.97, 0.97]     got - prefill where the prefill dwarfs the row's gradient:
                                                the final rounding alone (u |prefill + ref|, outside the constant), which
                                                round-to-nearest attains on both sides — as in the proposal tests (0.78)
  update: parameters / exp_avg / exp_avg_sq     [0.25, 0.25] / [0.24, 0.23] / [0.25, 0.25]
"""
import math

import pytest
import torch

from tests.test_gpu_proposal_kernels import (F8, N_EDGE, U, UNIT_BOX, C_TAB, _encode, _near_lattice, _points, _rays,
                                             _selector)

pytestmark = pytest.mark.gpu

B1, B2, EPS, LR = 0.9, 0.999, 1e-15, 1e-2
C_P, C_M, C_V = 4.0, 4.0, 4.0
FLOAT32 = "float32"           # `dev` of the CPU yardstick: the float32 evaluation of the reference in place of the kernel
WORST = {}                    # quantity -> worst ratio seen (printed by the tests, collected by the yardstick run)


def _K():
    from fruitnerf_amd import _kernels as K
    return K


def _Lb():
    from fruitnerf_amd import _lib as Lb
    return Lb


def _note(what, name, ratio):
    v = float(ratio)
    WORST[what] = max(WORST.get(what, 0.0), v)
    print(f"[hash scatter] {what} {name}: worst |err| / bound = {v:.3g}")
    return v


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# grids, geometries, feature gradients (float32, CPU)
# ---------------------------------------------------------------------------------------------------------------------

def _hash_scalings(n, lo, hi):
    """fruitnerf_amd._kernels.hash_scalings (nerfstudio's float32 floor(min_res growth^level)); imported lazily."""
    return _K().hash_scalings(n, lo, hi)


def _grid(name):
    """-> (log2_T, scalings)"""
    return {"small16": lambda: (14, _hash_scalings(16, 16, 2048)), "big16": lambda: (14, _hash_scalings(16, 16, 4096)),
            "edge2": lambda: (14, [511, 512]), "rows8k": lambda: (18, [16, 300, 2048, 4095]),
            "bins64": lambda: (19, [64, 2048]), "bins256": lambda: (21, [16, 4095]),
            "tiny6": lambda: (6, [16, 37]), "tiny10": lambda: (10, [16, 37])}[name]()


GRIDS = ["small16", "big16", "edge2", "rows8k", "bins64", "bins256", "tiny6", "tiny10"]
SMALL16_N = (1, 511, 512, 513, 1000, 2100)


def _plan(log2_T, N):
    """hash_scatter.hip's scatter_plan as documented: -> (log2 of the rows per bin, bins per level, queue capacity)."""
    log2_rows = max(0, min(13, log2_T - 5))
    bins = 1 << (log2_T - log2_rows)
    cap = max(1024, -(-3 * -(-8 * N // bins) // 1024) * 1024)
    return log2_rows, bins, cap


def _geom(kind, N, seed=0):
    if kind == "points":
        return _points(8, N, seed)                       # L = 8 of the proposal scalings: lattice planes of 16 and of 512
    return _rays(-(-N // 48), 48, seed=seed)


def _from_x(x):
    N = x.shape[0]
    return dict(mode=1, R=N, S=1, o=x.contiguous(), d=torch.zeros(N, 3), t=torch.tensor([[0.5, 1.5]]).repeat(N, 1),
                x=x.contiguous(), exempt_exact=True, n_edge=0)


RUNS = ((15, 2), (24, 15), (46, 16), (63, 17), (100, 33), (160, 64), (480, 65), (600, 513), (1200 - 33, 33))
RUNS_N = 1200                                            # two workgroups of 512 and a ragged one of 176


def _runs():
    """Random points with RUNS = (first sample, length) blocks jittered inside one cell of the coarsest level (16) each."""
    g = torch.Generator().manual_seed(4242)
    x = torch.rand(RUNS_N, 3, generator=g) * 0.98 + 0.01
    for i, (a, n) in enumerate(RUNS):
        cell = torch.tensor([1 + i, 14 - i, 3 + (5 * i) % 11], dtype=torch.float32)
        x[a:a + n] = (cell + 0.05 + 0.9 * torch.rand(n, 3, generator=g)) / 16.0
    return _from_x(x)


def _two_points(N):
    """Two fixed points alternating: no two neighbouring samples share a cell, every record of a level lands on 16 rows."""
    pts = torch.tensor([[0.2113, 0.3371, 0.4242], [0.7031, 0.6127, 0.8393]])
    return _from_x(pts[torch.arange(N) % 2])


def _d_feats(L, geom, scal, seed, dynamic_range=False):
    """[L,N,2]: 1e-3 randn, a few samples exactly 0 and a few 1e3 times the rest (dynamic_range: magnitudes log-uniform over
    2^+-20 inside each level, random signs); rays: 0 at the samples next to a lattice plane (<= 3 % of N, asserted)."""
    N = geom["x"].shape[0]
    g = torch.Generator().manual_seed(seed)
    if dynamic_range:
        df = torch.exp2(torch.rand(L, N, 2, generator=g) * 40.0 - 20.0) * (torch.randint(0, 2, (L, N, 2), generator=g) * 2 - 1)
    else:
        df = 1e-3 * torch.randn(L, N, 2, generator=g)
        if N >= 64:
            df[:, torch.randint(0, N, (max(2, N // 200),), generator=g)] = 0.0
            df[:, torch.randint(0, N, (max(2, N // 200),), generator=g)] *= 1e3
    if geom["mode"] == 0:
        near = _near_lattice(geom, scal)
        assert int(near.sum()) <= 0.03 * N, f"{int(near.sum())} of {N} samples sit next to a lattice plane"
        df[:, near] = 0.0
    return df.contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# the reference (float64) with its bound, and its float32 evaluation (the yardstick)
# ---------------------------------------------------------------------------------------------------------------------

def _records(geom, scal, log2_T, df, lb, cnt, dtype):
    """-> flat row index [cnt N 8], records [cnt,N,8,2] and the encode pieces, of levels [lb, lb + cnt), in `dtype`."""
    x32 = geom["x"]
    xm = (x32 * _selector(x32)[:, None]).to(dtype)
    T = 1 << log2_T
    e = _encode(torch.zeros(1, 2, dtype=dtype).expand(cnt * T, 2), xm, scal[lb:lb + cnt], log2_T)
    return (e["idx"] + lb * T).reshape(-1), e["W"][..., None] * df[lb:lb + cnt].to(dtype)[:, :, None, :], e


def _reference(grid, geom, df, lb=0, cnt=None):
    """float64: grad [L T, 2]; tb = the bound's sum over records (without C_TAB), floor = its fixed-point term, recursive =
    cnt_row u sum|records| (overflow test), per_bin [cnt, bins] = non-zero records per bin."""
    log2_T, scal = grid
    L, T, N = len(scal), 1 << log2_T, geom["x"].shape[0]
    cnt = L - lb if cnt is None else cnt
    idx, rec, e = _records(geom, scal, log2_T, df, lb, cnt, F8)
    wa, sc = e["wa"], e["sc"]
    absrec = rec.abs()
    Wp_sc = sum((wa[(a + 1) % 3] * wa[(a + 2) % 3]) * sc[..., a, None] for a in range(3))                 # [cnt,N,8]
    err = U * (absrec + Wp_sc[..., None] * df[lb:lb + cnt].double().abs()[:, :, None, :])
    add = lambda v: torch.zeros(L * T, 2, dtype=F8).index_add_(0, idx, v.reshape(-1, 2))   # noqa: E731
    n_row = add((absrec > 0).double())
    nb = (8 * N).bit_length()
    e_l = torch.frexp(absrec.amax((1, 2, 3)).clamp_min(1e-300))[1]                                        # [cnt]
    quantum = torch.zeros(L * T, 1, dtype=F8)
    quantum[lb * T:(lb + cnt) * T, 0] = torch.ldexp(torch.ones(cnt, dtype=F8), e_l + nb - 56).repeat_interleave(T)
    log2_rows, bins, _ = _plan(log2_T, N)
    live = (absrec > 0).any(-1).reshape(-1)
    per_bin = torch.bincount(((idx - lb * T) >> log2_rows)[live], minlength=cnt * bins).view(cnt, bins)
    return dict(grad=add(rec), tb=add(err), floor=n_row * quantum, recursive=n_row * U * add(absrec), per_bin=per_bin)


MUTATION = None   # CPU stand-ins of kernel bugs (tests/test_hash_scatter_cpu.py): the float32 evaluation then has to leave a bound


def _scatter_float32(grid, geom, df, lb, cnt, prefill):
    log2_T, scal = grid
    idx, rec, _ = _records(geom, scal, log2_T, df, lb, cnt, torch.float32)
    if MUTATION == "swapped corner weights":
        rec = rec[:, :, [0, 3, 2, 1, 4, 5, 6, 7]]
    elif MUTATION == "dropped last record":
        rec = rec.clone()
        rec.view(-1, 2)[rec.view(-1, 2).abs().sum(1).nonzero()[-1]] = 0.0
    elif MUTATION == "fixed point 2^24 too coarse":                       # S = 62 - nb - e - 24 with nb = 9 (n < 512 per bin)
        q = torch.ldexp(torch.ones(cnt, dtype=F8), torch.frexp(rec.abs().amax((1, 2, 3)).clamp_min(1e-30))[1] + 9 + 24 - 62)
        rec = (torch.round(rec.double() / q[:, None, None, None]) * q[:, None, None, None]).float()
    out = torch.zeros(len(scal) << log2_T, 2).index_add_(0, idx, rec.reshape(-1, 2))
    return out if prefill is None else prefill + out                                   # one final rounding, as the kernel's


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------

def _device_geometry(dev, geom, N=None):
    """-> (rays, warp, euclid); N = 0: the same (non-null) buffers with no rays."""
    K = _K()
    rays = K.RaysArg(geom["o"].to(dev), geom["d"].to(dev), None, None)
    if N == 0:
        rays.n = 0
        rays.c.n_rays = 0
    return rays, K.make_warp(geom["mode"], UNIT_BOX), geom["t"].to(dev).contiguous()


def _scatter_dev(dev, grid, geom, df, table, lb=0, cnt=None):
    """fnr_hash_encode_bwd of levels [lb, lb + cnt) into the device tensor `table` [L T, 2]."""
    K = _K()
    log2_T, scal = grid
    rays, warp, euclid = _device_geometry(dev, geom)
    K.hash_encode_bwd(K.make_grid(table, len(scal), log2_T, scal), warp, rays, euclid, geom["S"], df.to(dev).contiguous(), lb, cnt)


def _scatter(dev, grid, geom, df, lb=0, cnt=None, prefill=None, calls=None):
    """-> the gradient table [L T, 2] (CPU float32) after the calls [(lb, cnt), ...] (default: one call)."""
    log2_T, scal = grid
    calls = [(lb, len(scal) - lb if cnt is None else cnt)] if calls is None else calls
    if dev == FLOAT32:
        out = prefill
        for a, c in calls:
            out = _scatter_float32(grid, geom, df, a, c, out)
        return out
    table = (torch.zeros(len(scal) << log2_T, 2) if prefill is None else prefill).to(dev).contiguous()
    for a, c in calls:
        _scatter_dev(dev, grid, geom, df, table, a, c)
    torch.cuda.synchronize()
    return table.cpu()


def _prefill(grid, seed=99):
    log2_T, scal = grid
    return (0.05 * torch.randn(len(scal) << log2_T, 2, generator=torch.Generator().manual_seed(seed))).contiguous()


def _check(what, name, got, ref, prefill=None, recursive_levels=None, T=None):
    """Per row and feature: |got - ref| <= C_TAB tb + the fixed-point term (rows of `recursive_levels`: the recursive-
    summation term) (+ u |prefill + ref|); entries without a reference record: exactly the prefill (zero).  -> worst ratio"""
    floor = ref["floor"]
    if recursive_levels is not None:
        floor = floor.clone()
        for l in recursive_levels:
            floor[l * T:(l + 1) * T] = ref["recursive"][l * T:(l + 1) * T]
    bound = C_TAB * ref["tb"] + floor
    g = got.double()
    base = torch.zeros_like(got) if prefill is None else prefill
    if prefill is not None:
        bound = bound + U * (prefill.double() + ref["grad"]).abs()
        g = g - prefill.double()
    untouched = ref["tb"] == 0
    assert torch.equal(got[untouched], base[untouched]), f"{name}: entries without a record changed"
    assert float(ref["grad"].abs().max()) > 0, f"{name}: the reference gradient is all zero"
    return _note(what, name, ((g - ref["grad"]).abs() / (bound + 1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------------
# 1 - 6: the gradient per row
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["points", "rays"])
@pytest.mark.parametrize("name", GRIDS)
def test_gradient_per_row_and_feature(dev, name, kind):
    """(1) fnr_hash_encode_bwd on every grid: the gradient per table row and feature within the bound, exact zeros on rows
    without a reference record; edge2 by one call per level.  [0.20, 0.20]"""
    grid = _grid(name)
    L = len(grid[1])
    worst, seen = 0.0, set()
    for N in (SMALL16_N if name == "small16" else (1000,)):
        geom = _geom(kind, N, seed=len(name))
        if geom["x"].shape[0] in seen:                    # rays come in multiples of 48: 511, 512, 513 -> 528 once
            continue
        seen.add(geom["x"].shape[0])
        df = _d_feats(L, geom, grid[1], 3 + N)
        calls = [(l, 1) for l in range(L)] if name == "edge2" else None
        got = _scatter(dev, grid, geom, df, calls=calls)
        worst = max(worst, _check("table", f"{name}[{kind},N={geom['x'].shape[0]}]", got, _reference(grid, geom, df)))
        assert kind == "rays" or N < 255 or geom["n_edge"] == N_EDGE
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["small16", "rows8k"])
def test_runs_of_samples_in_one_cell(dev, name):
    """(2) Runs of 2 .. 513 consecutive samples in one coarse cell across the 16-lane, wave and workgroup boundaries, the last
    one ending on the last valid sample: the DPP pre-sums and their tails.  [0.12, 0.12]"""
    grid = _grid(name)
    geom = _runs()
    x16 = torch.floor(geom["x"] * 16.0)
    for a, n in RUNS:
        assert bool((x16[a:a + n] == x16[a]).all()) and (a == 0 or not torch.equal(x16[a - 1], x16[a])), (a, n)
    assert RUNS[-1][0] + RUNS[-1][1] == RUNS_N and RUNS_N % 512 != 0
    fine = torch.floor(geom["x"][600:1113].double() * grid[1][-1])
    assert torch.unique(fine, dim=0).shape[0] > 500                       # cells of their own at the finest level
    df = _d_feats(len(grid[1]), geom, grid[1], 11)
    got = _scatter(dev, grid, geom, df)
    assert _check("runs", name, got, _reference(grid, geom, df)) <= 1.0


GROUPS = [(0, 16), (0, 4), (4, 4), (8, 4), (12, 4), (15, 1), (3, 5)]


@pytest.mark.parametrize("lpb", ["1", "2", "3", "5"])
def test_level_groups_and_levels_per_workgroup(dev, monkeypatch, lpb):
    """(3) small16 by level groups, FNR_EMIT_LPB levels per emit workgroup: the group's levels bit-identical to the whole call
    (made with the library's own choice), every other level's rows untouched down to the bits of a random prefill."""
    grid = _grid("small16")
    T = 1 << grid[0]
    geom = _geom("points", 1000, seed=2)
    df = _d_feats(16, geom, grid[1], 19)
    pre = _prefill(grid)
    whole = _scatter(dev, grid, geom, df, prefill=pre)
    assert not torch.equal(whole, pre)
    monkeypatch.setenv("FNR_EMIT_LPB", lpb)
    for lb, cnt in GROUPS:
        got = _scatter(dev, grid, geom, df, lb, cnt, prefill=pre)
        inside = torch.zeros(16 * T, dtype=torch.bool)
        inside[lb * T:(lb + cnt) * T] = True
        assert torch.equal(got[inside], whole[inside]), f"levels [{lb},+{cnt}) at lpb {lpb} differ from the whole call"
        assert torch.equal(got[~inside], pre[~inside]), f"levels outside [{lb},+{cnt}) at lpb {lpb} were written"


@pytest.mark.parametrize("name", ["small16", "rows8k"])
def test_gradient_is_added_to_a_prefilled_table(dev, name):
    """(4) `+=` into the gradient table: prefill 0.05 randn, got - prefill against the reference, + u |prefill + ref| for
    the final rounding outside the constant.  [0.97, 0.97]"""
    grid = _grid(name)
    pre = _prefill(grid)
    worst = 0.0
    for kind in ("points", "rays"):
        geom = _geom(kind, 1000, seed=4)
        df = _d_feats(len(grid[1]), geom, grid[1], 23)
        got = _scatter(dev, grid, geom, df, prefill=pre)
        worst = max(worst, _check("accumulate", f"{name}[{kind}]", got, _reference(grid, geom, df), prefill=pre))
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["small16", "rows8k"])
def test_dynamic_range_inside_a_level(dev, name):
    """(5) |d_feats| log-uniform over 2^+-20 inside each level: every row within the bound, rows that hold only small values
    included — and the fixed-point term is what bounds some of them (the case is not vacuous).  [0.20, 0.20]"""
    grid = _grid(name)
    geom = _geom("points", 1000, seed=5)
    df = _d_feats(len(grid[1]), geom, grid[1], 29, dynamic_range=True)
    ref = _reference(grid, geom, df)
    dominated = (ref["floor"] > C_TAB * ref["tb"]) & (ref["tb"] > 0)
    assert int(dominated.sum()) >= 100, "the fixed-point term dominates the bound on too few rows"
    got = _scatter(dev, grid, geom, df)
    assert _check("dynamic range", name, got, ref) <= 1.0


OVERFLOW_N = 4096


def _overflow_case():
    grid = _grid("small16")
    geom = _two_points(OVERFLOW_N)
    df = _d_feats(16, geom, grid[1], 31)
    ref = _reference(grid, geom, df)
    _, bins, cap = _plan(grid[0], OVERFLOW_N)
    assert (bins, cap) == (32, 3072)
    excess = (ref["per_bin"] - cap).clamp_min(0).sum(1)
    assert bool((excess > 0).all()), f"levels without an overflowing bin: {excess.tolist()}"
    return grid, geom, df, ref


def _random_case_that_fits(seed):
    grid = _grid("small16")
    geom = _geom("points", OVERFLOW_N, seed=seed)
    df = _d_feats(16, geom, grid[1], 37)
    ref = _reference(grid, geom, df)
    assert int(ref["per_bin"].max()) <= _plan(grid[0], OVERFLOW_N)[2]
    return grid, geom, df, ref


def test_overflowing_queues_per_row_and_the_workspace_after_them(dev):
    """(6) Two points x 2048 samples each: some bin of every level exceeds the plan's capacity (from the reference's own
    histogram: capacity 3072, 8032 .. 14176 records beyond it per level; the random input's fullest bin holds 1536), the
    library reports the fallback, every row is within the recursive-summation bound.  Then random points
    through the SAME workspace (same sizes: workspace_clean = 1): no overflow, the gradient bit-identical to a call on a
    fresh workspace, and the fused call — which only reads the gradient table where a queue overflowed — leaves a
    prefilled gradient table alone and steps as on a fresh workspace: flag, level maximum and done counter were put back.
    [0.046, 0.046]"""
    grid, geom, df, ref = _overflow_case()
    T = 1 << grid[0]
    if dev == FLOAT32:
        got = _scatter(dev, grid, geom, df)
        assert _check("overflow", "small16", got, ref, recursive_levels=range(16), T=T) <= 1.0
        return
    K, Lb = _K(), _Lb()
    K._forget_scatter_workspaces(dev)
    Lb.scatter_overflows(reset=True)
    got = _scatter(dev, grid, geom, df)
    n_over = Lb.scatter_overflows(reset=True)
    print(f"[hash scatter] overflow: {n_over} records through the atomic fallback")
    assert n_over > 0
    assert _check("overflow", "small16", got, ref, recursive_levels=range(16), T=T) <= 1.0
    # the same workspace, told clean
    grid, geom2, df2, ref2 = _random_case_that_fits(6)
    fresh_before = K.fresh_workspaces()
    after = _scatter(dev, grid, geom2, df2)
    assert K.fresh_workspaces() == fresh_before, "the second call did not reuse the workspace"
    assert Lb.scatter_overflows(reset=True) == 0
    state = _fused_state(dev, grid, seed=3)
    garbage = _prefill(grid, seed=5).to(dev)
    fused_after = _fused(dev, grid, geom2, df2, ADAM_CASES[0], state, grad_table=garbage.clone())
    assert K.fresh_workspaces() == fresh_before
    K._forget_scatter_workspaces(dev)
    fresh = _scatter(dev, grid, geom2, df2)
    assert K.fresh_workspaces() == fresh_before + 1
    assert torch.equal(after, fresh), "a call after an overflowing one differs from the same call on a fresh workspace"
    assert _check("table", "small16[after overflow]", after, ref2) <= 1.0
    K._forget_scatter_workspaces(dev)
    fused_fresh = _fused(dev, grid, geom2, df2, ADAM_CASES[0], state, grad_table=garbage.clone())
    for k in ("p", "m", "v"):
        assert torch.equal(fused_after[k], fused_fresh[k]), f"fused step after an overflowing call: {k} differs"
    assert torch.equal(fused_after["g"], garbage) and torch.equal(fused_fresh["g"], garbage), "the gradient table was written"
    assert Lb.scatter_overflows(reset=True) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 7 - 9: the fused optimiser step
# ---------------------------------------------------------------------------------------------------------------------

# (algorithm, step, grad_scale, weight_decay, starting moments): Adam at steps 1 and 7, RAdam either side of rho_t = 5
ADAM_CASES = [("adam", 1, 1.0, 0.0, "random"), ("adam", 7, 0.5, 0.0, "random"), ("radam", 5, 1.0, 1e-2, "random"),
              ("radam", 6, 0.5, 0.0, "random"), ("adam", 1, 1.0, 1e-2, "zero"), ("radam", 6, 1.0, 0.0, "zero")]


def _rho(step):
    b2 = _f32(B2)
    rho_inf = 2.0 / (1.0 - b2) - 1.0
    return rho_inf - 2.0 * step * b2 ** step / (1.0 - b2 ** step)


def _fused_state(dev, grid, seed, moments="random"):
    """Parameters 0.1 randn, exp_avg 1e-3 randn, exp_avg_sq 1e-6 (0.1 + rand) (or zero moments), on the device."""
    n = (len(grid[1]) << grid[0]) * 2
    g = torch.Generator(device=dev).manual_seed(seed)
    p = 0.1 * torch.randn(n, device=dev, generator=g)
    m = 1e-3 * torch.randn(n, device=dev, generator=g)
    v = 1e-6 * (0.1 + torch.rand(n, device=dev, generator=g))
    return dict(p=p, m=m if moments == "random" else torch.zeros_like(m), v=v if moments == "random" else torch.zeros_like(v))


def _placed(t, offset):
    """A copy of t that starts `offset` floats into a fresh (256-byte aligned) buffer."""
    buf = torch.empty(t.numel() + offset + 4, dtype=t.dtype, device=t.device)
    out = buf[offset:offset + t.numel()]
    out.copy_(t)
    return out


def _fused(dev, grid, geom, df, case, state, touched=None, offset=0, N=None, grad_table=None):
    """fnr_hash_encode_bwd_adam from a copy of `state` -> dict p, m, v, g (device tensors; g = the gradient table after)."""
    K, Lb = _K(), _Lb()
    log2_T, scal = grid
    alg, step, gs, wd, _ = case
    s = {k: _placed(state[k], offset) for k in ("p", "m", "v")}
    assert all(t.data_ptr() % 16 == 4 * offset for t in s.values())
    g = torch.zeros(len(scal) << log2_T, 2, device=dev) if grad_table is None else grad_table
    rays, warp, euclid = _device_geometry(dev, geom, N)
    args = Lb.table_adam(0 if alg == "adam" else 1, LR, B1, B2, EPS, step, gs, wd, Lb.ptr(s["p"]), Lb.ptr(s["m"]), Lb.ptr(s["v"]),
                         Lb.ptr(touched))
    K.hash_encode_bwd_adam(K.make_grid(g, len(scal), log2_T, scal), warp, rays, euclid, geom["S"], df.to(dev).contiguous(), args)
    torch.cuda.synchronize()
    return dict(s, g=g)


def _unfused(dev, grid, geom, df, case, state, N=None):
    """fnr_hash_encode_bwd, then fnr_adam_step / fnr_radam_step (zero_grad) over the table's span."""
    K = _K()
    log2_T, scal = grid
    alg, step, gs, wd, _ = case
    s = {k: state[k].clone() for k in ("p", "m", "v")}
    g = torch.zeros(len(scal) << log2_T, 2, device=dev)
    if N != 0:
        _scatter_dev(dev, grid, geom, df, g)
    grad = g.clone()
    (K.adam_step if alg == "adam" else K.radam_step)(s["p"], g.view(-1), s["m"], s["v"], LR, B1, B2, EPS, step, gs, True, wd)
    torch.cuda.synchronize()
    return dict(s, g=g, grad=grad)


def _same_state(name, a, b):
    for k in ("p", "m", "v"):
        assert torch.equal(a[k], b[k]), f"{name}: {k} differs in {int((a[k] != b[k]).sum())} entries"
    assert not bool(a["g"].any()) and not bool(b["g"].any()), f"{name}: the gradient table is not left zero"


@pytest.mark.parametrize("name", GRIDS)
def test_fused_step_is_the_scatter_then_the_step(dev, name):
    """(7) fnr_hash_encode_bwd_adam against fnr_hash_encode_bwd + fnr_adam_step / fnr_radam_step: parameters and both moments
    bit-identical, the gradient table left zero — Adam at steps 1 and 7, RAdam at 5 and 6 (either side of rho_t = 5),
    grad_scale 0.5, weight decay, random and zero starting moments; slices 8 bytes off a 16-byte boundary (row-by-row
    sweep); N = 0 (moment decay only)."""
    assert _rho(5) <= 5.0 < _rho(6)
    grid = _grid(name)
    geom = _geom("points", 1000, seed=7)
    df = _d_feats(len(grid[1]), geom, grid[1], 41)
    for i, case in enumerate(ADAM_CASES):
        state = _fused_state(dev, grid, seed=10 + i, moments=case[4])
        want = _unfused(dev, grid, geom, df, case, state)
        assert not torch.equal(want["p"], state["p"]) and bool(want["grad"].any())
        _same_state(f"{name} {case}", _fused(dev, grid, geom, df, case, state), want)
        if i in (1, 2):
            _same_state(f"{name} {case} off 16-byte alignment", _fused(dev, grid, geom, df, case, state, offset=2), want)
    for case in (ADAM_CASES[1], ADAM_CASES[3]):
        state = _fused_state(dev, grid, seed=20)
        want = _unfused(dev, grid, geom, df, case, state, N=0)
        assert not torch.equal(want["m"], state["m"])
        _same_state(f"{name} {case} N = 0", _fused(dev, grid, geom, df, case, state, N=0), want)


@pytest.mark.parametrize("case", [ADAM_CASES[0], ADAM_CASES[3]])
def test_fused_step_on_overflowing_queues(dev, case):
    """(7) the overflowing input of (6): the rows that receive records (summed in part by float atomics, in arbitrary order)
    within 2e-3 relative of the unfused path, every other entry bit-identical, the gradient table left zero."""
    grid, geom, df, ref = _overflow_case()
    Lb = _Lb()
    state = _fused_state(dev, grid, seed=30)
    want = _unfused(dev, grid, geom, df, case, state)
    Lb.scatter_overflows(reset=True)
    got = _fused(dev, grid, geom, df, case, state)
    assert Lb.scatter_overflows(reset=True) > 0
    hot = (ref["tb"] != 0).reshape(-1).to(dev)
    assert 0 < int(hot.sum()) <= 16 * 16 * 2
    for k in ("p", "m", "v"):
        assert torch.equal(got[k][~hot], want[k][~hot]), f"{k}: entries without a record differ"
        assert torch.allclose(got[k][hot], want[k][hot], rtol=2e-3, atol=1e-6), f"{k}: rows summed by atomics"
    assert not bool(got["g"].any())


def _bits(bitmap):
    return ((bitmap.view(-1, 1) >> torch.arange(32, device=bitmap.device, dtype=torch.int32)) & 1).reshape(-1).bool()


@pytest.mark.parametrize("offset", [0, 2])
def test_sparse_touch_bitmap_small(dev, offset):
    """(8) Three fused steps on small16 with different samples from zero moments, with the bitmap and with touched = NULL:
    state bit-identical, a bit set exactly where the dense run's pair of rows has a non-zero moment (offset 2: slices 8
    bytes off a 16-byte boundary, the row-by-row sweep keeps the bitmap too)."""
    grid = _grid("small16")
    n_pairs = 16 << (grid[0] - 1)
    runs = {}
    for sparse in (True, False):
        state = _fused_state(dev, grid, seed=40, moments="zero")
        bitmap = torch.zeros(n_pairs // 32, dtype=torch.int32, device=dev) if sparse else None
        for step in (1, 2, 3):
            geom = _geom("points", 1000, seed=50 + step)
            df = _d_feats(16, geom, grid[1], 60 + step)
            out = _fused(dev, grid, geom, df, ("adam", step, 1.0, 0.0, "zero"), state, touched=bitmap, offset=offset)
            state = {k: out[k].clone() for k in ("p", "m", "v")}
        runs[sparse] = (state, bitmap)
    (sp, bitmap), (dense, _) = runs[True], runs[False]
    for k in ("p", "m", "v"):
        assert torch.equal(sp[k], dense[k]), f"{k} differs between the sparse-touch and the dense sweeps"
    moved = (dense["m"].view(-1, 4) != 0).any(1) | (dense["v"].view(-1, 4) != 0).any(1)
    assert 1000 < int(moved.sum()) < n_pairs
    assert torch.equal(_bits(bitmap), moved), "the bitmap and the dense run's moments disagree"


@pytest.mark.parametrize("name", ["tiny6", "tiny10"])
def test_bitmap_changes_nothing_below_64_rows_per_bin(dev, name):
    """(8) 2- and 32-row bins (less than one bitmap word): passing a bitmap changes neither the state nor the bitmap."""
    grid = _grid(name)
    geom = _geom("points", 1000, seed=8)
    df = _d_feats(2, geom, grid[1], 43)
    state = _fused_state(dev, grid, seed=41, moments="zero")
    bitmap = torch.zeros(max(1, (2 << (grid[0] - 1)) // 32), dtype=torch.int32, device=dev)
    with_bitmap = _fused(dev, grid, geom, df, ADAM_CASES[0], state, touched=bitmap)
    without = _fused(dev, grid, geom, df, ADAM_CASES[0], state)
    for k in ("p", "m", "v"):
        assert torch.equal(with_bitmap[k], without[k]) and not torch.equal(without[k], state[k]), k
    assert not bool(bitmap.any())


def _hyper(case):
    alg, step, gs, wd, _ = case
    b1, b2 = _f32(B1), _f32(B2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    rho_inf = 2.0 / (1.0 - b2) - 1.0
    rho_t = rho_inf - 2.0 * step * b2 ** step / bc2
    rect = math.sqrt((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) if rho_t > 5.0 else -1.0
    return dict(radam=alg == "radam", lr=_f32(LR), b1=b1, b2=b2, eps=_f32(EPS), gs=_f32(gs), wd=_f32(wd), bc1=bc1,
                bc2s=math.sqrt(bc2), rect=rect)


def _update_reference(case, p, g, m, v):
    """torch.optim.Adam / RAdam (L2 weight decay) in float64 on float32 inputs -> (p', m', v') and (E_p, E_m, E_v)."""
    h = _hyper(case)
    p, g, m, v = (t.double() for t in (p, g, m, v))
    gg = g * h["gs"] + h["wd"] * p
    E_g = U * (g * h["gs"]).abs() + (U * ((h["wd"] * p).abs() + gg.abs()) if h["wd"] != 0 else 0.0)
    m1 = torch.lerp(m, gg, 1.0 - h["b1"])
    E_m = (1 - h["b1"]) * E_g + U * (2 * (1 - h["b1"]) * (gg - m).abs() + m1.abs())
    v1 = v * h["b2"] + (1.0 - h["b2"]) * gg * gg
    E_v = U * (v * h["b2"]).abs() + (1 - h["b2"]) * (2 * gg.abs() * E_g + 2 * U * gg * gg) + U * v1.abs()
    r = v1.sqrt()
    E_r = E_v / (2 * r).clamp_min(1e-300) + U * r
    if not h["radam"]:
        den = r / h["bc2s"] + h["eps"]
        upd = (h["lr"] / h["bc1"]) * (m1 / den)
        E_den = (E_r + 2 * U * r) / h["bc2s"] + U * den
        E_u = (h["lr"] / h["bc1"]) * (E_m / den + m1.abs() * E_den / den ** 2) + 4 * U * upd.abs()
    else:
        mhat = m1 / h["bc1"]
        E_mhat = E_m / h["bc1"] + 2 * U * mhat.abs()
        if h["rect"] >= 0:
            ad = h["bc2s"] / (r + h["eps"])
            upd = h["lr"] * mhat * h["rect"] * ad
            E_ad = ad * (2 * U + (E_r + U * (r + h["eps"])) / (r + h["eps"]))
            E_u = h["lr"] * h["rect"] * (ad * E_mhat + mhat.abs() * E_ad) + 4 * U * upd.abs()
        else:
            upd = h["lr"] * mhat
            E_u = h["lr"] * E_mhat + U * upd.abs()
    p1 = p - upd
    return (p1, m1, v1), (E_u + U * p1.abs(), E_m, E_v)


def _update_float32(case, p, g, m, v):
    """table_adam_update's (adam.hpp) operations in their order, float32 on the CPU (the yardstick of C_P, C_M, C_V)."""
    h = _hyper(case)
    f = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
    gr = g * f(h["gs"])
    if h["wd"] != 0:
        gr = gr + f(h["wd"]) * p
    m1 = m + (gr - m) * (f(1.0) - f(h["b1"]))
    v1 = v * f(h["b2"]) + (f(1.0) - f(h["b2"])) * gr * gr
    if not h["radam"]:
        p1 = p - (f(h["lr"]) / f(h["bc1"])) * (m1 / (v1.sqrt() / f(h["bc2s"]) + f(h["eps"])))
    elif h["rect"] >= 0:
        p1 = p - f(h["lr"]) * (m1 / f(h["bc1"]) * f(h["rect"]) * (f(h["bc2s"]) / (v1.sqrt() + f(h["eps"]))))
    else:
        p1 = p - f(h["lr"]) * (m1 / f(h["bc1"]))
    return p1, m1, v1


def _check_update(name, case, before, g, after):
    """before / after: (p, m, v) CPU float32; g the float32 gradient the step consumed.  -> worst ratios (p, m, v)"""
    ref, err = _update_reference(case, before[0], g, before[1], before[2])
    out = []
    for what, c, got, r, e in zip(("update.parameters", "update.exp_avg", "update.exp_avg_sq"), (C_P, C_M, C_V), after, ref, err):
        out.append(_note(what, name, ((got.double() - r).abs() / (c * e + 1e-300)).max()))
    return out


def _update_inputs(n, seed, moments):
    g = torch.Generator().manual_seed(seed)
    p = 0.1 * torch.randn(n, generator=g)
    grad = 1e-3 * torch.randn(n, generator=g)
    grad[torch.randint(0, n, (max(1, n // 50),), generator=g)] *= 1e3
    m = 1e-3 * torch.randn(n, generator=g)
    v = 1e-6 * (0.1 + torch.rand(n, generator=g))
    return p, grad, (m if moments == "random" else torch.zeros(n)), (v if moments == "random" else torch.zeros(n))


@pytest.mark.parametrize("case", ADAM_CASES)
def test_optimiser_sweeps_per_entry(dev, case):
    """(9) fnr_adam_step / fnr_radam_step at 1, 3, 255 and 1025 float4s (the entry points take multiples of 4 entries): parameters,
    exp_avg and exp_avg_sq per entry against torch's formulas in float64; the gradient is zeroed.
    [parameters 0.25, 0.25; exp_avg 0.24, 0.23; exp_avg_sq 0.25, 0.25]"""
    worst = []
    for n4 in (1, 3, 255, 1025):
        p, g, m, v = _update_inputs(4 * n4, 70 + n4, case[4])
        if dev == FLOAT32:
            after = _update_float32(case, p, g, m, v)
        else:
            K = _K()
            d = [t.to(dev) for t in (p, g, m, v)]
            (K.adam_step if case[0] == "adam" else K.radam_step)(d[0], d[1], d[2], d[3], LR, B1, B2, EPS, case[1], case[2], True, case[3])
            torch.cuda.synchronize()
            assert not bool(d[1].any())
            after = tuple(t.cpu() for t in (d[0], d[2], d[3]))
        worst += _check_update(f"{case[:4]} n = {n4} float4", case, (p, m, v), g, after)
    assert max(worst) <= 1.0


@pytest.mark.parametrize("case", ADAM_CASES[:4])
def test_fused_sweep_per_entry(dev, case):
    """(9) The fused sweep on small16 (aligned: two rows per thread; 8 bytes off: row by row) from random parameters, non-zero
    exp_avg and positive exp_avg_sq: per entry against torch's formulas in float64 applied to the kernel's own float32
    gradient (fnr_hash_encode_bwd's, itself checked per row above)."""
    grid = _grid("small16")
    geom = _geom("points", 1000, seed=9)
    df = _d_feats(16, geom, grid[1], 47)
    if dev == FLOAT32:
        p, _, m, v = _update_inputs(32 << grid[0], 80, "random")
        g = _scatter(dev, grid, geom, df).view(-1)
        assert max(_check_update(f"fused {case[:4]}", case, (p, m, v), g, _update_float32(case, p, g, m, v))) <= 1.0
        return
    state = _fused_state(dev, grid, seed=80)
    g = _scatter(dev, grid, geom, df).view(-1)
    before = tuple(state[k].cpu() for k in ("p", "m", "v"))
    for offset in (0, 2):
        out = _fused(dev, grid, geom, df, case, state, offset=offset)
        after = tuple(out[k].cpu() for k in ("p", "m", "v"))
        assert max(_check_update(f"fused {case[:4]} offset {offset}", case, before, g, after)) <= 1.0


def test_a_table_too_large_for_the_bin_histogram_is_refused(dev):
    """(10) log2_hashmap_size = 22 (512 bins of 8192 rows > SC_MAX_BINS): both entry points return the error, nothing is
    launched — the table, the state and the library's record counter stay as they were."""
    K, Lb = _K(), _Lb()
    grid = (22, [16])
    geom = _geom("points", 1000, seed=10)
    df = _d_feats(1, geom, grid[1], 53)
    pre = _prefill(grid)
    table = pre.to(dev)
    torch.cuda.synchronize()
    records = Lb.scatter_records()
    with pytest.raises(RuntimeError, match="too large for the bin histogram"):
        _scatter_dev(dev, grid, geom, df, table)
    state = _fused_state(dev, grid, seed=90)
    with pytest.raises(RuntimeError, match="too large for the bin histogram"):
        _fused(dev, grid, geom, df, ADAM_CASES[0], state, grad_table=table)
    torch.cuda.synchronize()
    assert Lb.scatter_records() == records and torch.equal(table.cpu(), pre)
