"""Shared by tests/test_gpu_export_compact.py and tests/test_export_reference_cpu.py: the export compaction
(fnr_export_compact, csrc/export.hip; the reference project's exporter_utils.py:111-153) as plain NumPy, and the inputs.

The operation.  Float32 density[N], rgb[N,3], logit[N]; positions either explicit [N,3] or a lattice (xs, ys, zs, ray_begin):
sample n lies on ray ray_begin + n // n_z at depth k = n % n_z, ray r has ix = r // n_y, iy = r % n_y, position
(xs[ix], ys[iy], zs[k]) (int64 arithmetic).  Flags:
  den = density >= 70, sem = logit >= 3            exact float32 comparisons (IEEE: NaN compares false)
  cm  = sigmoid(logit) > fp32(0.9)                  evaluated in float64
Sets (include/fruitnerf_hip.h): 0 = den & cm, 1 = den & sem, 2 = den.  Per set the ORDERED list of selected sample indices;
points and rgb are copies of the selected rows, colour channel 3 is the float64 sigmoid(logit) (sets 0, 1) or
sigmoid(density) (set 2: density >= 70, so 1.0 to float32 and beyond).

The colormap flag is the only comparison that the device does not evaluate exactly (1 / (1 + expf(-x)) in float32, a few
ulp), so `margin` gives, per sample, (sigmoid64(logit) - fp32(0.9)) / 2^-24 — 2^-24 is the float32 spacing at 0.9 — and every
builder keeps |margin| >= MIN_MARGIN_ULP = 16 (about 1.1e-5 in logit: d sigmoid / d logit = 0.09 at the cut): draws that land
nearer are moved outward to 45 ulp.  With that no sample is excluded from any comparison.

Since logit >= 3 implies sigmoid(logit) > 0.9, set 1 is always a subset of set 0: the "sets differ" pattern puts the samples
that are in set 0 ONLY and the samples that are in set 1 at sparse, mutually disjoint places.
"""
import math

import numpy as np

U = 2.0 ** -24
CUT_DENSITY = np.float32(70.0)
CUT_LOGIT = np.float32(3.0)
CUT_SIGMOID = np.float32(0.9)
MIN_MARGIN_ULP = 16.0
# the float64 logit whose sigmoid is fp32(0.9), and how far a draw that lands too near is moved away from it
LOGIT_AT_CUT = math.log(float(CUT_SIGMOID) / (1.0 - float(CUT_SIGMOID)))
PUSH_LOGIT = 3e-5                     # 3e-5 * 0.09 / 2^-24 = 45 ulp
NEAR_LOGIT = 2.2e-5                   # draws within this of the cut (33 ulp) are moved
SENTINEL = -7777.25                   # no input and no output of any case holds it
EXP_TILE, EXP_PER_THREAD, SCAN_CHUNK = 1024, 4, 1024       # csrc/export.hip

SIZES = (1, 3, 1023, 1024, 1025, 4 * 1024 + 1, 1024 * 1024 + 1, 2 * 1024 * 1024 + 3 * 1024 + 5)
PATTERNS = ("none", "all", "sparse", "alternating_tiles", "lane63_last", "last_only", "sets_differ")
PATTERN_SIZES = (4 * 1024 + 1, 1024 * 1024 + 1)
RUNNING_SIZES = (1500, 0, 3 * 1024 + 7, 700)
RUNNING_START = (5, 0, 17)
CAPACITY_N = 4 * 1024 + 1
RANDOM_SEED = 7                       # with it the calls of 1 and of 3 samples select something
LATTICE = (7, 5, 37)
LATTICE_RANGES = ((0, 35), (0, 13), (3, 19), (3, 32), (11, 24), (11, 6))    # (ray_begin, n_rays); 7 * 5 = 35 rays


def sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def sigmoid32_cpu(x):
    """The device's formula, 1 / (1 + expf(-x)), every operation in float32 on the CPU: the yardstick for channel 3."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))).astype(np.float32)


def margin_ulp(logit):
    """(sigmoid64(logit) - fp32(0.9)) / ulp(0.9); NaN for a NaN logit."""
    return (sigmoid64(logit) - float(CUT_SIGMOID)) / U


def lattice_indices(n_y, n_z, ray_begin, n_rays):
    n = np.arange(int(n_rays) * int(n_z), dtype=np.int64)
    r = int(ray_begin) + n // int(n_z)
    return r // int(n_y), r % int(n_y), n % int(n_z)


def lattice_positions(xs, ys, zs, ray_begin, n_rays):
    ix, iy, k = lattice_indices(len(ys), len(zs), ray_begin, n_rays)
    return np.stack([xs[ix], ys[iy], zs[k]], axis=1).astype(np.float32)


def reference(density, rgb, logit, positions=None, lattice=None):
    """-> {"flags": bool [3, N], "margin": float64 [N], "sets": [{"idx", "points", "rgb", "alpha"}] * 3}"""
    density, logit = np.asarray(density), np.asarray(logit)
    assert density.dtype == np.float32 and logit.dtype == np.float32 and rgb.dtype == np.float32
    if positions is None:
        xs, ys, zs, ray_begin = lattice
        assert density.size % len(zs) == 0
        positions = lattice_positions(xs, ys, zs, ray_begin, density.size // len(zs))
    assert positions.dtype == np.float32 and positions.shape == (density.size, 3)
    with np.errstate(invalid="ignore"):
        den = density >= CUT_DENSITY
        sem = logit >= CUT_LOGIT
        s64 = sigmoid64(logit)
        cm = s64 > float(CUT_SIGMOID)
    flags = np.stack([den & cm, den & sem, den])
    sets = []
    for s in range(3):
        idx = np.flatnonzero(flags[s])
        alpha = sigmoid64(density[idx]) if s == 2 else s64[idx]
        sets.append({"idx": idx, "points": positions[idx], "rgb": rgb[idx], "alpha": alpha})
    return {"flags": flags, "margin": (s64 - float(CUT_SIGMOID)) / U, "sets": sets}


# ---- inputs ---------------------------------------------------------------------------------------------------------


def keep_off_the_cuts(logit):
    """Float32 logits moved outward where they land within NEAR_LOGIT of the colormap cut or within 1.5e-3 of logit == 3."""
    x = np.asarray(logit, dtype=np.float64).copy()
    d = x - LOGIT_AT_CUT
    near = np.abs(d) < NEAR_LOGIT
    x[near] = LOGIT_AT_CUT + np.where(d[near] >= 0, PUSH_LOGIT, -PUSH_LOGIT)
    d = x - 3.0
    near = np.abs(d) < 1.5e-3
    x[near] = 3.0 + np.where(d[near] >= 0, 2e-3, -2e-3)
    return x.astype(np.float32)


def selection_mask(N, pattern, rng):
    n = np.arange(N, dtype=np.int64)
    if pattern == "none":
        return np.zeros(N, dtype=bool)
    if pattern in ("all", "sets_differ"):
        return np.ones(N, dtype=bool)
    if pattern == "sparse":
        return rng.random(N) < 1e-3
    if pattern == "alternating_tiles":
        return (n // EXP_TILE) % 2 == 0
    if pattern == "lane63_last":          # thread t of a tile holds samples 4 t .. 4 t + 3; lane 63 of a wave: t % 64 == 63
        return n % (64 * EXP_PER_THREAD) == 64 * EXP_PER_THREAD - 1
    if pattern == "last_only":
        return n == N - 1
    if pattern == "random":
        return rng.random(N) < 0.3
    raise ValueError(pattern)


def make_inputs(N, pattern="random", seed=0):
    """-> density [N], rgb [N,3], logit [N], positions [N,3] (float32).
    `random`: density passes at 30 % of the samples, the logits are N(2.2, 1.5) independently of it (about half pass the
    colormap cut, about 30 % logit >= 3), so the three sets differ.  `sets_differ`: density passes everywhere, 1 % of the
    samples are in set 0 only, another 1 % in sets 0 and 1.  Every other pattern: a selected sample passes all three cuts, an
    unselected one fails the density cut alone (its logit is still N(2.2, 1.5): a kernel that forgot `density &&` shows)."""
    rng = np.random.default_rng([seed, N, PATTERNS.index(pattern) if pattern in PATTERNS else len(PATTERNS)])
    sel = selection_mask(N, pattern, rng)
    density = np.where(sel, rng.uniform(71.0, 200.0, N), rng.uniform(0.0, 69.0, N)).astype(np.float32)
    logit = rng.normal(2.2, 1.5, N)
    if pattern == "sets_differ":
        logit = rng.uniform(-6.0, 2.1, N)
        kind = rng.random(N)
        only_cm, both = kind < 0.01, (kind >= 0.5) & (kind < 0.51)
        logit[only_cm] = rng.uniform(2.25, 2.95, int(only_cm.sum()))
        logit[both] = rng.uniform(3.1, 8.0, int(both.sum()))
    elif pattern != "random":
        logit[sel] = rng.uniform(3.1, 8.0, int(sel.sum()))
    rgb = rng.random((N, 3), dtype=np.float32)
    positions = rng.uniform(-2.0, 2.0, (N, 3)).astype(np.float32)
    return density, rgb, keep_off_the_cuts(logit), positions


def edge_lists():
    f = np.float32
    inf = f(np.inf)
    density = np.array([np.nextafter(f(70), f(0)), f(70), np.nextafter(f(70), inf), f(np.nan), inf, -inf, f(0), f(-1)],
                       dtype=np.float32)
    ln9 = math.log(9.0)
    logit = np.array([np.nextafter(f(3), f(0)), f(3), np.nextafter(f(3), inf), ln9 - 2e-5, ln9 + 2e-5, ln9 - 1e-3, ln9 + 1e-3,
                      np.nan, np.inf, -np.inf, 100.0, -100.0], dtype=np.float32)
    return density, logit


def make_edge_inputs(seed=0):
    """The full cross product of the two edge lists (8 densities x 12 logits = 96 samples)."""
    d, l = edge_lists()
    density, logit = np.repeat(d, l.size), np.tile(l, d.size)
    rng = np.random.default_rng([seed, 96])
    return (density, rng.random((density.size, 3), dtype=np.float32), logit,
            rng.uniform(-2.0, 2.0, (density.size, 3)).astype(np.float32))


def make_lattice(n_x, n_y, n_z, seed=0):
    rng = np.random.default_rng([seed, n_x, n_y, n_z])
    return tuple(np.sort(rng.uniform(-1.0, 1.0, n)).astype(np.float32) for n in (n_x, n_y, n_z))


def lattice_cases():
    """(name, (n_x, n_y, n_z), ray_begin, n_rays)"""
    out = [(f"7x5x37[{b}+{n}]", LATTICE, b, n) for b, n in LATTICE_RANGES]
    out.append(("7x5x1[3+32]", (7, 5, 1), 3, 32))
    out.append(("1000x600x8[599000+1000]", (1000, 600, 8), 599000, 1000))
    return out


def all_cases():
    """Every (name, density, rgb, logit) that the GPU test feeds to the kernel, one at a time (the large ones are not kept)."""
    for N in SIZES:
        d, c, l, _ = make_inputs(N, "random", seed=RANDOM_SEED)
        yield f"random[{N}]", d, c, l
    for N in PATTERN_SIZES:
        for p in PATTERNS:
            d, c, l, _ = make_inputs(N, p, seed=2)
            yield f"{p}[{N}]", d, c, l
    d, c, l, _ = make_edge_inputs()
    yield "edges", d, c, l
    for i, N in enumerate(RUNNING_SIZES):
        d, c, l, _ = make_inputs(N, "random", seed=10 + i)
        yield f"running[{i}]", d, c, l
    d, c, l, _ = make_inputs(CAPACITY_N, "random", seed=3)
    yield "capacity", d, c, l
    for name, (n_x, n_y, n_z), _, n_rays in lattice_cases():
        d, c, l, _ = make_inputs(n_rays * n_z, "random", seed=4)
        yield f"lattice {name}", d, c, l


def alpha_ratio(got32, want64):
    """Worst |got - want| / (u * want) over the entries (0 where there are none)."""
    if want64.size == 0:
        return 0.0
    return float(np.max(np.abs(got32.astype(np.float64) - want64) / (U * want64)))


_yardstick = None


def alpha_yardstick():
    """Worst error of the float32 CPU evaluation of 1 / (1 + exp(-x)), in units of u * sigmoid64(x), over every logit whose
    sigmoid the GPU test compares (the samples of sets 0 and 1 of every case).  The kernel is granted 4 x this."""
    global _yardstick
    if _yardstick is None:
        worst = 0.0
        for _, density, _, logit in all_cases():
            with np.errstate(invalid="ignore"):
                used = (density >= CUT_DENSITY) & (sigmoid64(logit) > float(CUT_SIGMOID))
            worst = max(worst, alpha_ratio(sigmoid32_cpu(logit[used]), sigmoid64(logit[used])))
        _yardstick = worst
    return _yardstick
