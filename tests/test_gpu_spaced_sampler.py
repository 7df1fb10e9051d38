"""The code that starts a step — fnr_sample_spaced (k_sample_spaced; sampler_math.hpp), the level-0 role and the random numbers
of fnr_train_prologue (pixel_sampler.hip; step_randoms.hpp) and the per-ray planes of fnr_weights_pdf / fnr_weights_pdf_edges —
against the float64 reference of tests/spaced_sampler_reference.py (plain torch, written from the nerfstudio definition and
pinned on oracle/ns_torch.py in float64 by tests/test_spaced_sampler_cpu.py), per bin edge, never against a tensor maximum.

Inputs are made on the CPU and seeded.  Every ray has planes of its own (reference.planes): the training default (0.05, 1000),
the evaluation default (0, 1000), near on the kink of the lin-disp map (1, 4), both planes below it (0.3, 0.9), near = far,
planes an ulp to either side of the kink, the export lattice's (0, sqrt 3), and random planes with near in [0, 2) and bins from
1e-9 to 1000 wide.  The jitter has a row of 0.0 and a row of 1 - 2^-24, the ends of what the generators return.

Bounds (derived in the reference's docstring, none fitted): spacing bins 4 u absolute, u = 2^-24, and EQUAL to the float32
linspace in eval; euclidean bins 2e-6 |e| (kind 0), 2e-6 |e| + 2^-21 e^2 (kind 1), the bound of
tests/test_gpu_ray_kernels.py::test_weights_pdf_every_stage, checked as a stage against the float64 transform of the kernel's
OWN float32 spacing bins.  Both maps are continuous with equal slopes on either side of their kinks (x = 1, s = 1/2), so a
float32 value on the other side of a kink from its float64 twin stays inside the bound: no element is excluded.
Monotonicity e_{j+1} >= e_j is asserted only on bins whose float64 width exceeds the sum of their two edges' bounds, and never
on the near = far and straddling rays: float32 arithmetic (torch's own included) yields bins there that decrease by an ulp.

Worst |err| / bound over every test of this file, [CPU emulation (the float32 restatement of
tests/test_spaced_sampler_cpu.py), MI355X]:
  quantity                  [CPU, MI355X]
  spacing                   [0.25, 0.25]
  euclid kind 0             [0.0644, 0.0644]
  euclid kind 1             [0.344, 0.344]
  euclid under resampling   [0.245, 0.298]
No pair is more than a factor 4 apart: the kernel performs the restatement's operations in the restatement's order, and the
first three rows agree to the digits shown.  The resampling row differs because the CPU figure is measured on sorted random
spacing bins (the inverse-CDF stage is not restated), the MI355X figure on the bins the kernel resampled.
Teeth (the same reference with every ray given its neighbour's planes must violate the euclidean bound on >= 90 % of the
random-plane rays): fnr_sample_spaced 63 of 63 rays (100 %) in each of the 48 cases with R = 70; the PDF resampling 8 of 8 rays
(100 %) in each of its 54 calls.
The prologue's u [R,3] and jitter rows are bit-equal to the stated Philox4x32-10 words (groups 0 and 1 of
step_randoms.hpp) at every case; its level-0 bins are bit-equal to fnr_sample_spaced on the row it returned.
No defect was found in sampler.hip, sampler_math.hpp, pixel_sampler.hip or step_randoms.hpp.  The tests do fail on a wrong
kernel: with `fars[r - 1]` read in k_sample_spaced and weights_pdf_ray and the seed's high word dropped from word group 1,
60 of the 83 cases failed (every case with per-ray planes or with the 64-bit seed).
"""
import numpy as np
import pytest
import torch

from tests import edge_jitter_reference as ej
from tests import spaced_sampler_reference as sr

pytestmark = pytest.mark.gpu

F8, U = sr.F8, sr.U
SEEDS = ((1, 1), (0x1234567890ABCDEF, 0x1_0000_0003))


def _K():
    from fruitnerf_amd import _kernels as K
    return K


def _worst(name, ratio):
    v = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[spaced sampler] {name}: worst |err| / bound = {v:.3g}")
    return v


def _rays(dev, nears, fars, seed=0):
    R = nears.shape[0]
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    return _K().RaysArg(torch.zeros(R, 3, device=dev), d.to(dev), nears.to(dev), fars.to(dev))


def _teeth(name, kind, spacing, euclid, nears, fars, bar=0.9):
    """The reference under every ray's NEIGHBOUR's planes: the share of random-plane rays with an element outside its bound."""
    rolled = sr.euclid_of64(kind, spacing, nears.roll(1, 0), fars.roll(1, 0))
    _, b = sr.bounds(kind, spacing.double(), rolled)
    caught = (sr.ratio(euclid.double() - rolled, b) > 1.0).any(1)[sr.random_rows(nears.shape[0])]
    share = float(caught.double().mean())
    print(f"[spaced sampler] {name}: planes rolled by one ray are caught on {int(caught.sum())} of {caught.numel()} "
          f"random-plane rays ({100 * share:.0f} %)")
    assert share >= bar, name
    return share


def _check_bins(name, kind, S, nears, fars, t, spacing, euclid):
    """spacing [R,S+1], euclid [R,S+1] (float32, CPU) of a spaced sampler against the float64 reference: per element."""
    R = nears.shape[0]
    assert spacing.shape == euclid.shape == (R, S + 1)
    assert bool(torch.isfinite(spacing).all()) and bool(torch.isfinite(euclid).all()), name
    sp64, eu64 = sr.spaced_bins64(kind, S, nears, fars, t)
    e_ref = sr.euclid_of64(kind, spacing, nears, fars)            # the stage: the kernel's own spacing bins
    b_s, b_e = sr.bounds(kind, sp64, e_ref)
    if t is None:
        assert torch.equal(spacing, sr.base_bins(S)[None, :].expand(R, S + 1)), f"{name}: eval bins are not the linspace"
    else:
        lower, upper = sr.midpoints32(S)
        rows = t.reshape(R, -1)
        assert bool((rows[0] == 0.0).all()) and torch.equal(spacing[0], lower), f"{name}: jitter 0 is not `lower`"
        if R > 1:
            assert bool((rows[1] == np.float32(sr.T_MAX)).all()) and bool((spacing[1] <= upper).all()), \
                f"{name}: jitter 1 - 2^-24 passes `upper`"
    w_s = _worst(f"{name} spacing", sr.ratio(spacing.double() - sp64, b_s))
    w_e = _worst(f"{name} euclid kind {kind}", sr.ratio(euclid.double() - e_ref, b_e))
    assert w_s <= 1.0 and w_e <= 1.0, name
    # monotone where float64 resolves the bin
    _, b64 = sr.bounds(kind, sp64, eu64)
    for values, ref, bound in ((euclid, eu64, b64), (spacing, sp64, b_s)):
        ok = sr.resolved(ref, bound)
        for r in sr.DEGENERATE_ROWS:
            if r < R and values is euclid:
                assert not bool(ok[r].any()), "a bin of a near = far ray counts as resolved"
        assert bool((values[:, 1:] >= values[:, :-1])[ok].all()), f"{name}: a resolved bin decreases"


# ---- a. fnr_sample_spaced --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sr.FORMS)
@pytest.mark.parametrize("R,S", sr.SHAPES)
@pytest.mark.parametrize("kind", sr.KINDS)
def test_sample_spaced_against_float64(dev, kind, R, S, form):
    """k_sample_spaced, one thread per bin edge: S = 255 makes a ray one workgroup of 256 threads, S = 1 one partial workgroup,
    S = 513 rays that straddle workgroups and a partial last one; eval, one jitter per ray as [R] and [R,1], one per edge."""
    K = _K()
    seed = sr.case_seed(kind, R, S, form)
    nears, fars = sr.planes(R, seed)
    t = sr.jitter(R, S, form, seed + 1)
    spacing, euclid = K.sample_spaced(_rays(dev, nears, fars), kind, S, None if t is None else t.to(dev))
    spacing, euclid = spacing.cpu(), euclid.cpu()
    name = f"sample_spaced[kind {kind}, R {R}, S {S}, {form}]"
    _check_bins(name, kind, S, nears, fars, t, spacing, euclid)
    if R > sr.N_REGIMES:
        _teeth(name, kind, spacing, euclid, nears, fars)


# ---- b. the samplers built on it -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["eval", "ray1", "edge"])
def test_uniform_sampler_with_noise_carries_per_ray_planes(dev, form):
    """UniformSamplerWithNoise on a RayBundle with per-ray planes: bin_starts / bin_ends are exactly fnr_sample_spaced's
    euclidean bins (kind 0), spacing_starts / spacing_ends its spacing bins, and both hold the float64 bounds."""
    from fruitnerf_amd.components.ray_samplers import UniformSamplerWithNoise
    from fruitnerf_amd.rays import RayBundle
    K = _K()
    R, S = sr.N_RAYS, 6
    seed = sr.case_seed(0, R, S, form) + 17
    nears, fars = sr.planes(R, seed)
    t = sr.jitter(R, S, form, seed + 1)
    rays = _rays(dev, nears, fars)
    rb = RayBundle(rays.origins, rays.directions, None, None, nears.to(dev), fars.to(dev))
    smp = UniformSamplerWithNoise(num_samples=S, single_jitter=(form == "ray1"))
    smp.train(form != "eval")
    rs = smp.generate_ray_samples(rb, t_rand=None if t is None else t.to(dev))
    spacing, euclid = K.sample_spaced(rays, 0, S, None if t is None else t.to(dev))
    assert torch.equal(rs.frustums.starts[..., 0], euclid[:, :-1]) and torch.equal(rs.frustums.ends[..., 0], euclid[:, 1:])
    assert torch.equal(rs.spacing_starts[..., 0], spacing[:, :-1]) and torch.equal(rs.spacing_ends[..., 0], spacing[:, 1:])
    got_sp = torch.cat([rs.spacing_starts[..., 0], rs.spacing_ends[:, -1:, 0]], -1).cpu()
    got_eu = torch.cat([rs.frustums.starts[..., 0], rs.frustums.ends[:, -1:, 0]], -1).cpu()
    _check_bins(f"UniformSamplerWithNoise[{form}]", 0, S, nears, fars, t, got_sp, got_eu)


@pytest.fixture(scope="module")
def model(dev):
    from tests import util
    cfg = util.small_config(log2=13, prop_log2=11)
    return util.make_hip_like(util.make_oracle(cfg, seed=3), dev)


@pytest.mark.parametrize("form", ["eval", "ray1", "edge"])
def test_model_initial_sampler_carries_per_ray_planes(dev, model, form):
    """Level 0 of the model's proposal sampling (lin-disp piecewise) on a RayBundle that brings its own planes: exactly
    fnr_sample_spaced(kind 1) on those planes, and within the float64 bounds."""
    from fruitnerf_amd.rays import RayBundle
    from tests import util
    K = _K()
    hm = model
    R, S = sr.N_RAYS, hm.proposal_sampler.num_proposal_samples_per_ray[0]
    seed = sr.case_seed(1, R, S, form) + 29
    nears, fars = sr.planes(R, seed)
    t = sr.jitter(R, S, form, seed + 1)
    o, d, pa, cam = util.random_rays(R, 7, seed=2)
    rb = RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev), nears.to(dev), fars.to(dev))
    hm.train(form != "eval")
    hm.proposal_sampler.single_jitter = form != "edge"
    try:
        with torch.no_grad():
            _, ctx = hm._render(hm._collide(rb), jitter=None if t is None else [t.to(dev), None, None])
    finally:
        hm.proposal_sampler.single_jitter = bool(hm.config.use_single_jitter)
    level0 = ctx.levels[0]
    assert level0["S"] == S
    rays = K.RaysArg(rb.origins, rb.directions, rb.nears, rb.fars)
    spacing, euclid = K.sample_spaced(rays, 1, S, None if t is None else t.to(dev))
    assert torch.equal(level0["spacing"], spacing) and torch.equal(level0["euclid"], euclid)
    _check_bins(f"model level 0[{form}]", 1, S, nears, fars, t, level0["spacing"].cpu(), level0["euclid"].cpu())


# ---- c. per-ray planes in the PDF resampling -------------------------------------------------------------------------------
@pytest.mark.parametrize("S_prev", sr.PDF_S_PREV)
def test_weights_pdf_reads_every_ray_s_own_planes(dev, S_prev):
    """fnr_weights_pdf (rand [R] and eval) and fnr_weights_pdf_edges (rand [R, S_new + 1]) with planes of the rays' own, on
    the densities and previous bins of test_weights_pdf_every_stage, anneal 1: euclid_new within the euclidean bound of the
    float64 transform of the kernel's OWN spacing_new under ray r's planes — and outside it under ray r - 1's."""
    from tests.test_gpu_ray_kernels import _batch
    K = _K()
    edges, dens, _, _ = _batch(S_prev, seed=3)
    R = edges.shape[0]
    g = torch.Generator().manual_seed(S_prev)
    worst, shares = [], []
    for kind in sr.KINDS:
        sp = torch.sort(torch.rand(R, S_prev + 1, generator=g), 1).values
        sp[:, 0], sp[:, -1] = 0.0, 1.0
        for S_new in sr.PDF_S_NEW:
            nears, fars = sr.planes(R, 7919 * S_prev + 31 * S_new + kind)
            rays = _rays(dev, nears, fars)
            args = (dens.to(dev), sp.contiguous().to(dev), edges.to(dev), 1.0)
            forms = (("per ray", dict(rand=torch.rand(R, generator=g))), ("eval", dict(rand=None)),
                     ("per edge", dict(rand=torch.rand(R, S_new + 1, generator=g), per_edge=True)))
            for form, kw in forms:
                rand = kw.pop("rand")
                _, _, sp_new, eu_new = K.weights_pdf(rays, kind, S_prev, S_new, *args, None if rand is None else rand.to(dev),
                                                     **kw)
                sp_new, eu_new = sp_new.cpu(), eu_new.cpu()
                assert bool(torch.isfinite(sp_new).all()) and bool(torch.isfinite(eu_new).all())
                assert float(sp_new.min()) >= 0.0 and float(sp_new.max()) <= 1.0
                e_ref = sr.euclid_of64(kind, sp_new, nears, fars)
                _, b_e = sr.bounds(kind, sp_new.double(), e_ref)
                name = f"weights_pdf[S_prev {S_prev}, S_new {S_new}, kind {kind}, {form}]"
                worst.append(_worst(f"{name} euclid under resampling", sr.ratio(eu_new.double() - e_ref, b_e)))
                shares.append(_teeth(name, kind, sp_new, eu_new, nears, fars))
    assert max(worst) <= 1.0
    print(f"[spaced sampler] weights_pdf[S_prev {S_prev}] teeth: least share caught {100 * min(shares):.0f} %")


# ---- d. the prologue's numbers ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cameras(dev):
    """3 cameras of 16 x 16 random pixels."""
    from fruitnerf_amd.data import synthetic_apple as sa
    K = _K()
    rng = np.random.default_rng(0)
    images = torch.from_numpy(rng.integers(0, 256, (3, 16, 16, 3)).astype(np.uint8)).to(dev)
    masks = torch.from_numpy(rng.integers(0, 2, (3, 16, 16)).astype(np.uint8)).to(dev)
    c2w = sa.make_cameras(3, seed=0).to(dev)
    g = torch.Generator().manual_seed(3)
    pose = torch.cat([torch.randn(3, 3, generator=g) * 0.02, torch.randn(3, 3, generator=g) * 0.03], 1)
    return {"iset": K.ImageSetArg(images, masks, c2w, 20.0, 20.0, 8.0, 8.0), "pose": pose.to(dev)}


@pytest.mark.parametrize("seed,offset", SEEDS)
@pytest.mark.parametrize("R", [1, 257, 1030])
def test_prologue_numbers_are_the_stated_philox_words(dev, cameras, R, seed, offset):
    """u [R,3] = words 0-2 of group 0, jitter rows = word 3 of group 0 then words 0-3 of group 1, bit for bit, for 3 and 5
    rows, with and without a pose, one partial / two / five workgroups of rays, a seed and an offset with high words; the
    per-edge form writes the same u; offset + 1 gives other numbers, the reference's again.  (With a pose the launch needs at
    least as many rays as cameras: R = 1 then draws from one camera.)"""
    K = _K()
    for with_pose in (False, True):
        n_train = min(3, R) if with_pose else 3
        ids = torch.arange(n_train, device=dev)
        pose = cameras["pose"][:n_train].contiguous() if with_pose else None
        for n_jitter in (3, 5):
            kw = dict(pose_adjustment=pose, near=0.05, far=1000.0, S0=3)
            first = None
            for off in (offset, offset + 1):
                out = K.train_prologue(cameras["iset"], ids, R, seed, off, n_jitter=n_jitter, **kw)
                u, jit = sr.prologue_randoms(seed, off, R, n_jitter)
                got_u, got_j = out["u"].cpu().numpy(), out["jitter"].cpu().numpy()
                assert got_j.shape == (n_jitter, R)
                assert np.array_equal(got_u, u), ("u", with_pose, n_jitter, hex(off))
                assert np.array_equal(got_j, jit), ("jitter", with_pose, n_jitter, hex(off))
                edges = K.train_prologue(cameras["iset"], ids, R, seed, off, per_edge=True, **kw)
                assert edges["jitter"] is None and torch.equal(edges["u"], out["u"]), "the per-edge form draws another u"
                if first is None:
                    first = (got_u, got_j)
            assert not np.array_equal(first[0], got_u) and not np.array_equal(first[1], got_j), "offset + 1 draws the same numbers"


# ---- e. the prologue's level 0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S0", [1, 255])
@pytest.mark.parametrize("near,far", [(0.0, 1000.0), (0.05, 1000.0), (2.0, 6.0)])
@pytest.mark.parametrize("kind", sr.KINDS)
def test_prologue_level0_away_from_the_training_default(dev, cameras, kind, near, far, S0):
    """The level-0 role of k_train_prologue at both spacing kinds, the evaluation planes, the training planes and planes
    beyond the kink: within the float64 bounds on the jitter the launch itself returned (row 0; per edge:
    fnr_edge_jitter(level 0)), and bit-equal to fnr_sample_spaced on it."""
    K = _K()
    R = sr.N_RAYS
    seed, offset = SEEDS[1]
    ids = torch.arange(3, device=dev)
    nears, fars = torch.full((R, 1), near), torch.full((R, 1), far)
    for per_edge in (False, True):
        out = K.train_prologue(cameras["iset"], ids, R, seed, offset, None, near, far, S0, spacing_kind=kind, per_edge=per_edge)
        if per_edge:
            t = K.edge_jitter(seed, offset, 0, R, S0 + 1, dev)
            assert np.array_equal(t.cpu().numpy(), ej.edge_jitter(seed, offset, 0, R, S0 + 1))
        else:
            t = out["jitter"][0].contiguous()
            assert np.array_equal(t.cpu().numpy(), sr.prologue_randoms(seed, offset, R, 1)[1][0])
        rays = K.RaysArg(out["origins"], out["directions"], nears.to(dev), fars.to(dev), out["cam"])
        spacing, euclid = K.sample_spaced(rays, kind, S0, t)
        assert torch.equal(out["spacing"], spacing) and torch.equal(out["euclid"], euclid), (kind, near, far, S0, per_edge)
        name = f"prologue level 0[kind {kind}, ({near:g}, {far:g}), S0 {S0}, {'per edge' if per_edge else 'per ray'}]"
        sp, eu, tc = out["spacing"].cpu(), out["euclid"].cpu(), t.cpu()
        sp64, _ = sr.spaced_bins64(kind, S0, nears, fars, tc)
        e_ref = sr.euclid_of64(kind, sp, nears, fars)
        b_s, b_e = sr.bounds(kind, sp64, e_ref)
        assert bool(torch.isfinite(sp).all()) and bool(torch.isfinite(eu).all())
        assert _worst(f"{name} spacing", sr.ratio(sp.double() - sp64, b_s)) <= 1.0
        assert _worst(f"{name} euclid kind {kind}", sr.ratio(eu.double() - e_ref, b_e)) <= 1.0
