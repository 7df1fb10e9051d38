"""tests/spaced_sampler_reference.py without a device: the float64 reference is nerfstudio's sampler (oracle/ns_torch.py run in
float64) up to the float32 linspace the kernels read, it reproduces the reference's own bins (tests/golden/reference_pins.npz),
a float32 restatement of the kernel's arithmetic stays within half of every bound over the inputs of
tests/test_gpu_spaced_sampler.py, and the prologue's numbers sit on the stated Philox words and share none with the random
background or the per-edge jitter."""
import os

import numpy as np
import pytest
import torch

from oracle import ns_torch as ns
from tests import edge_jitter_reference as ej
from tests import spaced_sampler_reference as sr
from tests.composite_background_reference import random_background, step_randoms

F8, U = sr.F8, sr.U
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEEDS = ((1, 1), (0x1234567890ABCDEF, 0x1_0000_0003))


def _ns_sampler(kind, S, training):
    smp = (ns.SpacedSampler(spacing_fn=lambda x: x, spacing_fn_inv=lambda x: x, num_samples=S) if kind == 0
           else ns.UniformLinDispPiecewiseSampler(num_samples=S))
    smp.train(training)
    return smp


def _ns_bins64(kind, S, nears, fars, t_rand):
    """ns.SpacedSampler / ns.UniformLinDispPiecewiseSampler in float64 -> (spacing [R,S+1], euclid [R,S+1])."""
    R = nears.shape[0]
    rb = ns.RayBundle(torch.zeros(R, 3, dtype=F8), torch.ones(R, 3, dtype=F8), torch.ones(R, 1, dtype=F8),
                      nears=nears.double(), fars=fars.double())
    t = None if t_rand is None else t_rand.double().reshape(R, -1)
    rs = _ns_sampler(kind, S, t_rand is not None)(rb, t_rand=t)
    spacing = torch.cat([rs.spacing_starts[..., 0], rs.spacing_ends[:, -1:, 0]], -1)
    euclid = torch.cat([rs.frustums.starts[..., 0], rs.frustums.ends[:, -1:, 0]], -1)
    return spacing, euclid


@pytest.mark.parametrize("kind", sr.KINDS)
def test_reference_is_the_nerfstudio_sampler_in_float64(kind):
    """Every form and shape of the GPU cases.  The one difference allowed is the float32 linspace: <= 2^-24 in a spacing bin
    (a jittered bin is a convex combination of linspace values), and that times the slope of the transform,
    |de/db| = inv'(s) (s_far - s_near), inv' = 1 (kind 0), 2 below s = 1/2 and 2 e^2 above (kind 1), in a euclidean bin."""
    worst_s = worst_e = 0.0
    for R, S in sr.SHAPES:
        for form in sr.FORMS:
            seed = sr.case_seed(kind, R, S, form)
            nears, fars = sr.planes(R, seed)
            t = sr.jitter(R, S, form, seed + 1)
            sp, eu = sr.spaced_bins64(kind, S, nears, fars, t)
            ref_sp, ref_eu = _ns_bins64(kind, S, nears, fars, t)
            assert sp.shape == eu.shape == (R, S + 1) and sp.dtype == eu.dtype == F8
            d_s = (sp - ref_sp).abs()
            assert bool((d_s <= U).all()), (R, S, form, float(d_s.max()))
            span = (sr.spacing_fn(kind, fars.double()) - sr.spacing_fn(kind, nears.double())).abs()
            big = torch.maximum(eu, ref_eu)
            slope = span * (1.0 if kind == 0 else torch.maximum(torch.full_like(big, 2.0), 2 * big * big))
            tol = 1.001 * slope * U + 1e-13 * (1 + big)
            d_e = (eu - ref_eu).abs()
            assert bool((d_e <= tol).all()), (R, S, form, float((d_e / tol).max()))
            worst_s, worst_e = max(worst_s, float(d_s.max()) / U), max(worst_e, float((d_e / tol).max()))
    print(f"[spaced sampler cpu] kind {kind}: float32 against float64 linspace, worst spacing {worst_s:.3g} u, euclid "
          f"{worst_e:.3g} of its propagation")


def test_forms_of_one_jitter_agree():
    """[R], [R,1] and a per-edge table with constant rows are the same bins."""
    nears, fars = sr.planes(9, 5)
    t = sr.jitter(9, 6, "ray", 6)
    a = sr.spaced_bins64(1, 6, nears, fars, t)
    b = sr.spaced_bins64(1, 6, nears, fars, t[:, None])
    c = sr.spaced_bins64(1, 6, nears, fars, t[:, None].expand(9, 7).contiguous())
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("mode", ["eval", "train_single", "train"])
def test_reference_reproduces_the_pinned_sampler(mode):
    """The smp:: records of tests/golden/reference_pins.npz (the reference's UniformSamplerWithNoise, float32): euclidean bins
    within 2e-6 max(far), the tolerance tests/test_gpu_reference_pins.py holds the kernel to on the same records; spacing
    bins within the 4u of a float32 evaluation, and equal in eval mode."""
    g = np.load(os.path.join(GOLD, "reference_pins.npz"))
    nears, fars = torch.from_numpy(g["smp::nears"]), torch.from_numpy(g["smp::fars"])
    t = None if mode == "eval" else torch.from_numpy(g[f"smp::{mode}::t_rand"])
    sp, eu = sr.spaced_bins64(0, 6, nears, fars, t)
    tol = 2e-6 * float(fars.max())
    for got, lo, hi in ((eu, "bin_starts", "bin_ends"), (sp, "spacing_starts", "spacing_ends")):
        starts = torch.from_numpy(g[f"smp::{mode}::{lo}"])[..., 0].double().expand(5, 6)
        ends = torch.from_numpy(g[f"smp::{mode}::{hi}"])[..., 0].double().expand(5, 6)
        if got is sp and mode == "eval":
            assert torch.equal(got[:, :-1], starts) and torch.equal(got[:, 1:], ends)
        bar = tol if got is eu else 4 * U
        err = max(float((got[:, :-1] - starts).abs().max()), float((got[:, 1:] - ends).abs().max()))
        print(f"[spaced sampler cpu] pins {mode} {lo[:-7]}: max |float64 - pinned| {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (mode, lo)
    probe = torch.linspace(0, 1, 4)[None, :].expand(5, -1)
    want = torch.from_numpy(g[f"smp::{mode}::spacing_to_euclidean(probe)"]).double()
    assert float((sr.euclid_of64(0, probe, nears, fars) - want).abs().max()) <= tol


def test_planes_and_jitter_are_what_the_gpu_tests_assume():
    nears, fars = sr.planes(sr.N_RAYS, 3)
    assert nears.dtype == fars.dtype == torch.float32 and nears.shape == fars.shape == (sr.N_RAYS, 1)
    for i, (n, f) in enumerate(sr.REGIMES):
        assert float(nears[i]) == float(np.float32(n)) and float(fars[i]) == float(np.float32(f))
    assert float(nears[5]) < 1.0 < float(fars[5]) and float(nears[4]) == float(fars[4])
    rnd = sr.random_rows(sr.N_RAYS)
    assert bool((fars[rnd] >= nears[rnd]).all()) and bool((nears[rnd] >= 0).all()) and bool((nears[rnd] < 2).all())
    assert bool((nears[rnd] < 1).any()) and bool((nears[rnd] > 1).any()) and bool((fars[rnd] < 1).any())
    assert sr.planes(1, 0)[0].shape == (1, 1)
    for form, shape in (("ray", (70,)), ("ray1", (70, 1)), ("edge", (70, 49))):
        t = sr.jitter(70, 48, form, 1)
        assert tuple(t.shape) == shape and t.dtype == torch.float32
        rows = t.reshape(70, -1)
        assert bool((rows[0] == 0.0).all()) and bool((rows[1] == np.float32(sr.T_MAX)).all())
        assert bool((rows >= 0).all()) and bool((rows < 1).all())
    assert sr.jitter(70, 48, "eval", 1) is None and float(sr.jitter(1, 1, "edge", 1).abs().max()) == 0.0


def test_float32_restatement_stays_within_half_of_every_bound():
    """The kernel's operations in the kernel's order in float32 torch on the CPU (no fused multiply-add) over every case of
    tests/test_gpu_spaced_sampler.py: spacing against spaced_bins64, euclidean bins against euclid_of64 of the float32 spacing
    bins (and of sorted random spacing bins under the planes of the resampling cases).  At most 1/2 of each bound; the
    edges of the jitter range hold in float32 (t = 0 gives `lower`, t = 1 - 2^-24 stays <= `upper`).
    Resolved bins (float64 width above the two edges' bounds) do not decrease.
    [measured: spacing 0.25, euclid kind 0 0.0644, kind 1 0.344, under resampling 0.245]"""
    worst = {"spacing": 0.0, "euclid kind 0": 0.0, "euclid kind 1": 0.0, "euclid under resampling": 0.0}
    for kind in sr.KINDS:
        for R, S in sr.SHAPES:
            lower, upper = sr.midpoints32(S)
            for form in sr.FORMS:
                seed = sr.case_seed(kind, R, S, form)
                nears, fars = sr.planes(R, seed)
                t = sr.jitter(R, S, form, seed + 1)
                sp32, eu32 = sr.spaced_bins32(kind, S, nears, fars, t)
                sp64, eu64 = sr.spaced_bins64(kind, S, nears, fars, t)
                e_ref = sr.euclid_of64(kind, sp32, nears, fars)
                b_s, b_e = sr.bounds(kind, sp64, e_ref)
                assert torch.isfinite(sp32).all() and torch.isfinite(eu32).all()
                if t is None:
                    assert torch.equal(sp32.double(), sp64)
                else:
                    assert torch.equal(sp32[0], lower)
                    assert R == 1 or bool((sp32[1] <= upper).all())
                _, b64 = sr.bounds(kind, sp64, eu64)
                assert bool((eu32[:, 1:] >= eu32[:, :-1])[sr.resolved(eu64, b64)].all()), "a resolved bin decreases"
                assert bool((sp32[:, 1:] >= sp32[:, :-1])[sr.resolved(sp64, b_s)].all()), "a resolved spacing bin decreases"
                worst["spacing"] = max(worst["spacing"], float(sr.ratio(sp32.double() - sp64, b_s).max()))
                k = f"euclid kind {kind}"
                worst[k] = max(worst[k], float(sr.ratio(eu32.double() - e_ref, b_e).max()))
        for S_new in sr.PDF_S_NEW:
            R = 15
            nears, fars = sr.planes(R, 500 + S_new + kind)
            g = torch.Generator().manual_seed(S_new)
            sp = torch.sort(torch.rand(R, S_new + 1, generator=g), 1).values
            sp[:, 0], sp[:, -1] = 0.0, 1.0
            e_ref = sr.euclid_of64(kind, sp, nears, fars)
            _, b_e = sr.bounds(kind, sp.double(), e_ref)
            r = float(sr.ratio(sr.euclid_of32(kind, sp, nears, fars).double() - e_ref, b_e).max())
            worst["euclid under resampling"] = max(worst["euclid under resampling"], r)
    for k, v in worst.items():
        print(f"[spaced sampler cpu] float32 restatement, {k}: worst |err| / bound = {v:.3g}")
        assert v <= 0.5, k


def test_resolved_bins_exclude_the_degenerate_rows():
    """The monotonicity mask leaves out every bin of the near = far and straddling rows and keeps nearly all others."""
    for kind in sr.KINDS:
        nears, fars = sr.planes(sr.N_RAYS, 11)
        sp, eu = sr.spaced_bins64(kind, 48, nears, fars, sr.jitter(sr.N_RAYS, 48, "ray", 12))
        _, b_e = sr.bounds(kind, sp, eu)
        ok = sr.resolved(eu, b_e)
        for r in sr.DEGENERATE_ROWS:
            assert not bool(ok[r].any()), r
        assert float(ok.double().mean()) > 0.9


@pytest.mark.parametrize("seed,offset", SEEDS)
def test_prologue_randoms_are_the_stated_words(seed, offset):
    R = 257
    u, jit = sr.prologue_randoms(seed, offset, R, 5)
    g0, g1 = step_randoms(seed, offset, R, 0), step_randoms(seed, offset, R, 1)
    assert u.shape == (R, 3) and jit.shape == (5, R) and u.dtype == jit.dtype == np.float32
    for i in range(3):
        assert np.array_equal(u[:, i], g0[:, i])
    assert np.array_equal(jit[0], g0[:, 3])
    for i in range(4):
        assert np.array_equal(jit[1 + i], g1[:, i])
    assert np.array_equal(sr.prologue_randoms(seed, offset, R, 3)[1], jit[:3])
    assert np.array_equal(sr.prologue_randoms(seed, offset, 100, 5)[0], u[:100])        # a ray's numbers are its own
    # every half of the 64-bit seed and offset reaches the numbers
    for s2, o2 in ((seed ^ (1 << 32), offset), (seed ^ 1, offset), (seed, offset ^ (1 << 32)), (seed, offset + 1)):
        u2, jit2 = sr.prologue_randoms(s2, o2, R, 5)
        assert (u2 != u).mean() > 0.99 and (jit2 != jit).mean() > 0.99, (hex(s2), hex(o2))


@pytest.mark.parametrize("seed,offset", SEEDS)
def test_prologue_shares_no_word_with_the_background_or_the_edge_jitter(seed, offset):
    """Per ray, the eight numbers of groups 0 and 1 against the background triple (group 2) and the 49 level-0 edge jitters
    (group 3, quads 0 - 12): the 24 bits a number keeps of its word never coincide (by chance: 3e-5 per ray)."""
    R, n_edges = 257, 49
    u, jit = sr.prologue_randoms(seed, offset, R, 5)
    mine = np.concatenate([u, jit.T], axis=1)                                            # [R, 8]
    others = np.concatenate([random_background(seed, offset, R).numpy(), ej.edge_jitter(seed, offset, 0, R, n_edges)], axis=1)
    assert mine.shape == (R, 8) and others.shape == (R, 3 + n_edges)
    assert not bool((mine[:, :, None] == others[:, None, :]).any())
    assert not bool((mine[:, :, None] == mine[:, None, :])[:, ~np.eye(8, dtype=bool)].any())
