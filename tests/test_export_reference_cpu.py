"""tests/export_reference.py checked without a GPU: the reference against the literal statement of the reference project's
selection (exporter_utils.py:111-153, torch float32 masks and gathers), the inputs' distance from the three cuts, the
selection rate of every pattern, the lattice index arithmetic against a triple loop, and the float32 CPU yardstick of
colour channel 3.

Measured: the float32 CPU evaluation of 1 / (1 + exp(-x)) errs by at most 1.640 u sigmoid(x) over the compared logits (u = 2^-24,
sigmoid >= 0.9, e = exp(-x) <= 1 / 9): the rounding of 1 + e (half an ulp of [1, 2) = u, relative to 1 + e: at most u) plus
the rounding of the quotient (half an ulp of [0.5, 1) = u / 2, relative to s: at most 0.56 u) plus expf's own error scaled
by e / (1 + e) <= 0.1.  The bound asserted here, 2.5, is that sum with expf granted several ulp."""
import math

import numpy as np
import pytest
import torch

from tests import export_reference as er


def _literal_selection(density, rgb, logit, positions):
    """exporter_utils.py:105-153 with rgb_flag, as written (the [N,3] repeats, mask.sum(dim=1).to(bool), torch.hstack);
    semantics_colormap is fruit_nerf.py:263-265: heaviside(sigmoid(semantics) - 0.9, 0)."""
    den_t, log_t = torch.from_numpy(density), torch.from_numpy(logit)
    points_3d, rgb_t = torch.from_numpy(positions).reshape(-1, 3), torch.from_numpy(rgb).reshape(-1, 3)
    colormap = torch.heaviside(torch.sigmoid(log_t) - 0.9, torch.tensor([0.0]))
    semantic = log_t.reshape(-1, 1).repeat(1, 3)
    semantics_colormap = colormap.reshape(-1, 1).repeat(1, 3)
    dens = den_t.reshape(-1, 1).repeat(1, 3)
    mask_sem = semantic >= 3
    mask_den = dens >= 70
    mask_sem_colormap = semantics_colormap >= 0.999
    out = []
    m = mask_sem_colormap.sum(dim=1).to(bool) & mask_den.sum(dim=1).to(bool)
    out.append((m, points_3d[m], torch.hstack([rgb_t[m], torch.sigmoid(semantic[m][:, 0]).unsqueeze(-1)])))
    m = mask_sem.sum(dim=1).to(bool) & mask_den.sum(dim=1).to(bool)
    out.append((m, points_3d[m], torch.hstack([rgb_t[m], torch.sigmoid(semantic[m][:, 0]).unsqueeze(-1)])))
    m = mask_den.sum(dim=1).to(bool)
    out.append((m, points_3d[m], torch.hstack([rgb_t[m], torch.sigmoid(dens[m][:, 0]).unsqueeze(-1)])))
    return out


def _check_against_literal(density, rgb, logit, positions):
    ref = er.reference(density, rgb, logit, positions)
    lit = _literal_selection(density, rgb, logit, positions)
    for s in range(3):
        mask, pts, col = lit[s]
        assert np.array_equal(ref["flags"][s], mask.numpy()), s
        assert np.array_equal(ref["sets"][s]["idx"], np.flatnonzero(mask.numpy())), s
        assert torch.equal(torch.from_numpy(ref["sets"][s]["points"]), pts), s
        assert torch.equal(torch.from_numpy(ref["sets"][s]["rgb"]), col[:, :3]), s
        # torch's float32 sigmoid against the float64 one: a few float32 roundings
        assert er.alpha_ratio(col[:, 3].numpy(), ref["sets"][s]["alpha"]) <= 4.0, s
    return ref


@pytest.mark.parametrize("N", [n for n in er.SIZES if n <= er.PATTERN_SIZES[1]])
def test_reference_is_the_reference_projects_selection_on_random_inputs(N):
    _check_against_literal(*er.make_inputs(N, "random", seed=er.RANDOM_SEED))


@pytest.mark.parametrize("pattern", er.PATTERNS)
def test_reference_is_the_reference_projects_selection_on_every_pattern(pattern):
    _check_against_literal(*er.make_inputs(er.PATTERN_SIZES[0], pattern, seed=2))


def test_reference_on_the_threshold_edges_follows_ieee():
    density, rgb, logit, positions = er.make_edge_inputs()
    d_list, l_list = er.edge_lists()
    assert density.size == d_list.size * l_list.size == 8 * 12
    ref = _check_against_literal(density, rgb, logit, positions)
    # expected flags spelled out: densities [70-, 70, 70+, nan, +inf, -inf, 0, -1], logits [3-, 3, 3+, ln9 -+ 2e-5, ln9 -+ 1e-3,
    # nan, +inf, -inf, 100, -100]
    den = np.array([0, 1, 1, 0, 1, 0, 0, 0], dtype=bool)
    sem = np.array([0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 1, 0], dtype=bool)
    cm = np.array([1, 1, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0], dtype=bool)
    want = np.stack([np.outer(den, cm).ravel(), np.outer(den, sem).ravel(), np.repeat(den, l_list.size)])
    assert np.array_equal(ref["flags"], want)
    # NaN selects nothing; logit = +inf is in both semantic sets with channel 3 == 1
    assert not ref["flags"][:, np.isnan(density)].any() and not ref["flags"][:2, np.isnan(logit)].any()
    for s in (0, 1):
        at_inf = np.isposinf(logit[ref["sets"][s]["idx"]])
        assert at_inf.sum() == den.sum() and np.all(ref["sets"][s]["alpha"][at_inf] == 1.0)
    assert np.all(ref["sets"][2]["alpha"] == 1.0)
    # the deliberate near values still keep the 16 ulp
    finite = np.isfinite(logit)
    assert np.min(np.abs(ref["margin"][finite])) >= er.MIN_MARGIN_ULP


def test_every_input_keeps_its_distance_from_the_cuts():
    """|sigmoid64(logit) - fp32(0.9)| >= 16 ulp(0.9) for every logit of every case the GPU test runs; density == 70 and
    logit == 3 are approached by the edge case alone."""
    seen = 0
    for name, density, _, logit in er.all_cases():
        m = er.margin_ulp(logit)
        finite = ~np.isnan(m)
        assert finite.all() or name == "edges", name
        if m.size:
            assert np.min(np.abs(m[finite])) >= er.MIN_MARGIN_ULP, (name, float(np.min(np.abs(m[finite]))))
        if name != "edges":
            assert np.all(np.abs(density.astype(np.float64) - 70.0) >= 1.0), name
            assert np.all(np.abs(logit.astype(np.float64) - 3.0) >= 1e-3), name
        assert density.dtype == logit.dtype == np.float32
        seen += 1
    assert seen == len(er.SIZES) + 2 * len(er.PATTERNS) + 1 + len(er.RUNNING_SIZES) + 1 + len(er.lattice_cases())
    # the push itself: draws at and next to the cut end up 45 ulp away, on their own side
    x = np.float32(er.LOGIT_AT_CUT) + np.float32(1e-6) * np.arange(-30, 31, dtype=np.float32)
    moved = er.keep_off_the_cuts(x)
    assert np.min(np.abs(er.margin_ulp(moved))) >= 2 * er.MIN_MARGIN_ULP
    d = x.astype(np.float64) - er.LOGIT_AT_CUT
    assert np.array_equal(np.sign(er.margin_ulp(moved)), np.where(d >= 0, 1.0, -1.0))


@pytest.mark.parametrize("N", er.PATTERN_SIZES)
def test_each_pattern_selects_what_its_name_says(N):
    tiles = -(-N // er.EXP_TILE)
    counts = {}
    for p in er.PATTERNS + ("random",):
        density, rgb, logit, positions = er.make_inputs(N, p, seed=2 if p != "random" else er.RANDOM_SEED)
        ref = er.reference(density, rgb, logit, positions)
        counts[p] = c = [int(f.sum()) for f in ref["flags"]]
        if p not in ("random", "sets_differ"):
            assert c[0] == c[1] == c[2], p           # a selected sample is in all three sets
    assert counts["none"] == [0, 0, 0] and counts["all"] == [N, N, N] and counts["last_only"] == [1, 1, 1]
    assert counts["lane63_last"][2] == N // 256
    full, rest = divmod(N, er.EXP_TILE)
    assert counts["alternating_tiles"][2] == ((full + 1) // 2) * er.EXP_TILE + (rest if full % 2 == 0 else 0)
    assert tiles > 1 and counts["alternating_tiles"][2] not in (0, N)

    def binomial(count, p):                           # 5 standard deviations of a binomial draw
        return abs(count - N * p) <= 5.0 * math.sqrt(N * p * (1 - p))
    assert counts["sparse"][2] >= 1 and binomial(counts["sparse"][2], 1e-3)
    assert binomial(counts["random"][2], 0.3)
    assert 0.25 * counts["random"][2] < counts["random"][1] < counts["random"][0] < 0.7 * counts["random"][2]
    c0, c1, c2 = counts["sets_differ"]
    assert c2 == N and binomial(c1, 0.01) and binomial(c0 - c1, 0.01)


def test_the_patterns_place_their_samples_where_the_kernel_is_cut():
    N = er.PATTERN_SIZES[0]
    sel = er.reference(*er.make_inputs(N, "lane63_last", seed=2))["flags"][2]
    n = np.flatnonzero(sel)
    thread = (n % er.EXP_TILE) // er.EXP_PER_THREAD
    assert np.all(n % er.EXP_PER_THREAD == er.EXP_PER_THREAD - 1) and np.all(thread % 64 == 63)
    sel = er.reference(*er.make_inputs(N, "alternating_tiles", seed=2))["flags"][2]
    per_tile = [int(sel[t * er.EXP_TILE:(t + 1) * er.EXP_TILE].sum()) for t in range(-(-N // er.EXP_TILE))]
    assert per_tile == [1024, 0, 1024, 0, 1]
    sel = er.reference(*er.make_inputs(N, "last_only", seed=2))["flags"]
    assert np.array_equal(np.flatnonzero(sel[0]), [N - 1])
    # the smallest calls select something
    for n_small in (1, 3):
        assert er.reference(*er.make_inputs(n_small, "random", seed=er.RANDOM_SEED))["flags"].any(), n_small
    # sizes: the scan's chunk of 1024 tiles is passed once and twice, the last chunk ragged
    chunks = [-(-(-(-n // er.EXP_TILE)) // er.SCAN_CHUNK) for n in er.SIZES]
    assert chunks == [1, 1, 1, 1, 1, 1, 2, 3]
    assert (-(-er.SIZES[-2] // er.EXP_TILE)) % er.SCAN_CHUNK == 1 and (-(-er.SIZES[-1] // er.EXP_TILE)) % er.SCAN_CHUNK == 4


def test_lattice_index_arithmetic_against_a_triple_loop():
    n_x, n_y, n_z = er.LATTICE
    xs, ys, zs = er.make_lattice(n_x, n_y, n_z)
    brute = np.array([(xs[i], ys[j], zs[k]) for i in range(n_x) for j in range(n_y) for k in range(n_z)], dtype=np.float32)
    assert brute.shape == (n_x * n_y * n_z, 3)
    for ray_begin, n_rays in er.LATTICE_RANGES + ((0, 0), (34, 1)):
        got = er.lattice_positions(xs, ys, zs, ray_begin, n_rays)
        assert np.array_equal(got, brute[ray_begin * n_z:(ray_begin + n_rays) * n_z]), (ray_begin, n_rays)
    assert any((b + n) % n_y for b, n in er.LATTICE_RANGES) and any(b % n_y for b, _ in er.LATTICE_RANGES)
    assert any(b + n == n_x * n_y for b, n in er.LATTICE_RANGES)
    # the large lattice: ray 599 000 is (ix, iy) = (998, 200)
    ix, iy, k = er.lattice_indices(600, 8, 599000, 1000)
    assert (ix[0], iy[0], k[0]) == (998, 200, 0) and (ix[-1], iy[-1], k[-1]) == (999, 599, 7)
    # reference(): lattice and materialised positions give the same lists
    density, rgb, logit, _ = er.make_inputs(19 * n_z, "random", seed=4)
    a = er.reference(density, rgb, logit, lattice=(xs, ys, zs, 3))
    b = er.reference(density, rgb, logit, positions=er.lattice_positions(xs, ys, zs, 3, 19))
    for s in range(3):
        assert np.array_equal(a["sets"][s]["idx"], b["sets"][s]["idx"])
        assert np.array_equal(a["sets"][s]["points"], b["sets"][s]["points"])


def test_channel_3_yardstick():
    """The float32 CPU evaluation of the device's formula against float64 over the compared logits; set 2 is exactly 1."""
    ratio = er.alpha_yardstick()
    print(f"[export channel 3] float32 CPU worst |err| / (u s) = {ratio:.3f}; the kernel is granted {4 * ratio:.3f}")
    assert 0.5 <= ratio <= 2.5
    for d in (70.0, 71.0, 200.0, np.inf):
        assert er.sigmoid64(np.float32(d)) == 1.0 or 1.0 - er.sigmoid64(np.float32(d)) < 2.0 ** -53
        assert np.float32(er.sigmoid64(np.float32(d))) == np.float32(1.0) and er.sigmoid32_cpu(np.float32(d)) == np.float32(1.0)
