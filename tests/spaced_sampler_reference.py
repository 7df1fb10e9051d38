"""Float64 reference of the spaced sampler (fnr_sample_spaced, the level-0 role of fnr_train_prologue and the transform
stage of fnr_weights_pdf) and the stated Philox words of the prologue's numbers, in plain torch and numpy.  Shared by
tests/test_spaced_sampler_cpu.py (which pins it on oracle/ns_torch.py and on tests/golden/reference_pins.npz and measures a
float32 restatement against the bounds) and tests/test_gpu_spaced_sampler.py (which holds the kernels to it).

Definition (nerfstudio SpacedSampler.generate_ray_samples, UniformLinDispPiecewiseSampler), with x_0 .. x_S the float32
torch.linspace(0, 1, S + 1) the kernels read (K.host_linspace) and near, far the float32 planes of the ray, all upcast:
  centre_j = (x_j + x_{j+1}) / 2,  lower = (x_0, centre_0 .. centre_{S-1}),  upper = (centre_0 .. centre_{S-1}, x_S)
  b_j = lower_j + (upper_j - lower_j) t            (training; t one number per ray or one per bin edge; eval: b_j = x_j)
  e_j = inv(b_j fn(far) + (1 - b_j) fn(near))
  kind 0 (uniform):            fn(x) = inv(x) = x
  kind 1 (lin-disp piecewise): fn(x) = x / 2 for x < 1, 1 - 1 / (2x) otherwise;  inv(s) = 2s for s < 1/2, 1 / (2 - 2s) otherwise

Bounds, per element, u = 2^-24:
  spacing bins  4u absolute.  Every value is in [0, 1]: each of the two midpoints is one rounded sum of magnitude <= 2 halved
                exactly (<= u / 2 each), upper - lower inherits both and rounds once more (<= 3u / 2 in all, its own rounding
                below u / 2 since the width is <= 1/2), the product with t < 1 rounds once (<= u / 2) and the final sum once
                (<= u / 2): <= 3u.  Eval bins are the linspace values themselves: they must compare EQUAL.
  euclidean     the bound tests/test_gpu_ray_kernels.py::test_weights_pdf_every_stage states for the same transform, checked
                as a stage — against the float64 transform of the float32 spacing bins under test:
                kind 0: 2e-6 |e| (e = b far + (1 - b) near, two non-negative float32 products and their sum, relatively
                accurate to a few u); kind 1: 2e-6 |e| + 2^-21 e^2 (s = b s_far + (1 - b) s_near carries |ds| <= 2^-22 and
                e = 1 / (2 - 2s) turns ds into 2 e^2 ds).
  Kinks: fn is continuous at x = 1 with slope 1/2 on both sides, inv at s = 1/2 with slope 2 on both sides (2s and
  1 / (2 - 2s) agree to first order there).  A float32 value that lands on the other side of a kink from its float64 twin is
  therefore evaluated by a branch that differs from the twin's by O(d^2) for a distance d ~ u from the kink: it stays inside
  the bound, and no element is excluded on that account.

Monotonicity: float32 arithmetic (torch's own included) yields euclidean bins that decrease by an ulp where near ~ far; the
tests assert e_{j+1} >= e_j only where the float64 bin width exceeds the two edges' bounds (`resolved`).
"""
import numpy as np
import torch

from tests.composite_background_reference import step_randoms

F8 = torch.float64
U = 2.0 ** -24
T_MAX = 1.0 - U                      # the largest number the generators return: (2^24 - 1) 2^-24
FORMS = ("eval", "ray", "ray1", "edge")
# (near, far) of the regime rows of planes(): the training and the evaluation default, near on the kink of the lin-disp map,
# both planes below it, near = far, planes an ulp to either side of the kink, the export lattice's (0, sqrt 3)
REGIMES = ((0.0, 1000.0), (0.05, 1000.0), (1.0, 4.0), (0.3, 0.9), (2.0, 2.0), (0.999999, 1.000001), (0.0, 3.0 ** 0.5))
N_REGIMES = len(REGIMES)
DEGENERATE_ROWS = (4, 5)             # near = far and the straddling row: never asserted monotone

# The cases of tests/test_gpu_spaced_sampler.py, which tests/test_spaced_sampler_cpu.py runs through the float32 restatement.
# One thread per bin edge, 256 threads per workgroup: with S = 255 a ray is exactly one workgroup, with S = 1 and R = 70 the
# launch is one partial workgroup, with S = 513 rays straddle workgroups and the last one is partial.
KINDS = (0, 1)
SAMPLES = (1, 6, 48, 255, 256, 513)
N_RAYS = 70
SHAPES = tuple((N_RAYS, S) for S in SAMPLES) + ((1, 1),)
PDF_S_PREV = (48, 96, 321)
PDF_S_NEW = (1, 48, 96)


def case_seed(kind: int, R: int, S: int, form: str) -> int:
    return 1000003 * kind + 7919 * S + 31 * R + FORMS.index(form)


# ---- the maps ------------------------------------------------------------------------------------------------------
def spacing_fn(kind: int, x: torch.Tensor) -> torch.Tensor:
    return x if kind == 0 else torch.where(x < 1, x / 2, 1 - 1 / (2 * x))


def spacing_fn_inv(kind: int, s: torch.Tensor) -> torch.Tensor:
    return s if kind == 0 else torch.where(s < 0.5, 2 * s, 1 / (2 - 2 * s))


def base_bins(S: int) -> torch.Tensor:
    """The float32 linspace the kernels read (fruitnerf_amd._kernels.host_linspace evaluates the same call on the CPU)."""
    return torch.linspace(0.0, 1.0, S + 1, dtype=torch.float32)


def _midpoints(x: torch.Tensor):
    centre = (x[1:] + x[:-1]) / 2.0
    return torch.cat([x[:1], centre]), torch.cat([centre, x[-1:]])       # lower, upper


def _per_row(t_rand, R: int, S: int, dtype) -> torch.Tensor:
    """t_rand [R] / [R,1] -> [R,1]; [R,S+1] stays (for S = 0 edges per row the two cannot be told apart and agree)."""
    t = torch.as_tensor(t_rand).to(dtype)
    if t.dim() == 1:
        assert t.shape[0] == R, (tuple(t.shape), R)
        return t[:, None]
    assert tuple(t.shape) in ((R, 1), (R, S + 1)), (tuple(t.shape), R, S)
    return t


def euclid_of64(kind: int, spacing: torch.Tensor, nears: torch.Tensor, fars: torch.Tensor) -> torch.Tensor:
    """The float64 spacing -> euclidean transform of GIVEN spacing bins [R, S+1] under the float32 planes [R] / [R,1]."""
    b = spacing.to(F8)
    s_near = spacing_fn(kind, nears.to(F8).reshape(-1, 1))
    s_far = spacing_fn(kind, fars.to(F8).reshape(-1, 1))
    return spacing_fn_inv(kind, b * s_far + (1 - b) * s_near)


def spaced_bins64(kind: int, S: int, nears: torch.Tensor, fars: torch.Tensor, t_rand=None):
    """-> (spacing [R,S+1], euclid [R,S+1]) float64.  t_rand: None (eval), [R] / [R,1] (one per ray) or [R,S+1] (one per edge)."""
    R = nears.reshape(-1).shape[0]
    x = base_bins(S).to(F8)
    if t_rand is None:
        b = x[None, :].expand(R, S + 1)
    else:
        lower, upper = _midpoints(x)
        b = lower[None, :] + (upper - lower)[None, :] * _per_row(t_rand, R, S, F8)
    b = b.contiguous()
    return b, euclid_of64(kind, b, nears, fars)


# ---- the float32 restatement: the kernel's operations in the kernel's order, each rounded once (no fused multiply-add) ----
def midpoints32(S: int):
    """lower, upper [S+1] float32 as spaced_bin_edge forms them: fdiv(fadd(x_{j+1}, x_j), 2)."""
    return _midpoints(base_bins(S))


def spaced_bins32(kind: int, S: int, nears: torch.Tensor, fars: torch.Tensor, t_rand=None):
    """k_sample_spaced in float32 torch on the CPU -> (spacing, euclid) float32."""
    R = nears.reshape(-1).shape[0]
    x = base_bins(S)
    if t_rand is None:
        b = x[None, :].expand(R, S + 1).contiguous()
    else:
        lower, upper = midpoints32(S)
        width = (upper - lower)[None, :]
        b = lower[None, :] + width * _per_row(t_rand, R, S, torch.float32)
    return b, euclid_of32(kind, b, nears, fars)


def euclid_of32(kind: int, spacing: torch.Tensor, nears: torch.Tensor, fars: torch.Tensor) -> torch.Tensor:
    """spacing_to_euclid in float32: inv(fadd(fmul(b, s_far), fmul(fsub(1, b), s_near)))."""
    b = spacing.float()
    s_near = spacing_fn(kind, nears.float().reshape(-1, 1))
    s_far = spacing_fn(kind, fars.float().reshape(-1, 1))
    p_far = b * s_far
    p_near = (1.0 - b) * s_near
    return spacing_fn_inv(kind, p_far + p_near)


# ---- inputs --------------------------------------------------------------------------------------------------------
def planes(R: int, seed: int):
    """float32 nears, fars [R,1]: the regime rows first (as many as fit), then near in [0, 2), far = near + r^3 1000 with r
    uniform — planes on either side of the lin-disp kink, bins from 1e-9 to 1000 wide, no two rays alike."""
    g = torch.Generator().manual_seed(seed)
    near = torch.rand(R, generator=g, dtype=F8) * 2.0
    far = near + torch.rand(R, generator=g, dtype=F8) ** 3 * 1000.0
    for i, (n, f) in enumerate(REGIMES[:R]):
        near[i], far[i] = n, f
    nears, fars = near.float()[:, None].contiguous(), far.float()[:, None].contiguous()
    pairs = set(zip(nears.reshape(-1).tolist(), fars.reshape(-1).tolist()))
    assert len(pairs) == R, "two rays share their planes"
    return nears, fars


def jitter(R: int, S: int, form: str, seed: int):
    """t_rand of one form (FORMS): None, [R], [R,1] or [R,S+1] float32 in [0, 1) on the generators' 2^-24 grid; row 0 is all
    0.0 and row 1 (where there is one) all 1 - 2^-24, the ends of what the generators return."""
    if form == "eval":
        return None
    g = torch.Generator().manual_seed(seed)
    cols = S + 1 if form == "edge" else 1
    t = torch.randint(0, 2 ** 24, (R, cols), generator=g).to(torch.float32) * np.float32(U)
    t[0] = 0.0
    if R > 1:
        t[1] = T_MAX
    return t.reshape(-1).contiguous() if form == "ray" else t.contiguous()


def random_rows(R: int) -> slice:
    """The rows of planes(R, .) that carry random planes."""
    return slice(min(N_REGIMES, R), R)


# ---- bounds --------------------------------------------------------------------------------------------------------
def bounds(kind: int, spacing64: torch.Tensor, euclid64: torch.Tensor):
    """-> (spacing bound, euclidean bound), per element, as derived in the module docstring."""
    e = euclid64.to(F8).abs()
    b_e = 2e-6 * e
    if kind == 1:
        b_e = b_e + 2.0 ** -21 * e * e
    return torch.full_like(spacing64.to(F8), 4 * U), b_e


def ratio(err: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """|err| / bound per element, 0 where both are 0 (e = 0 at near = 0 is exact) and inf where only the bound is."""
    err = err.abs().to(F8)
    return torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                             torch.zeros_like(err)))


def resolved(values64: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """[R,S] bool: the bins whose float64 width exceeds the sum of their two edges' bounds — where float32 bins must not
    decrease."""
    return (values64[:, 1:] - values64[:, :-1]) > (bound[:, 1:] + bound[:, :-1])


# ---- the prologue's numbers ----------------------------------------------------------------------------------------
def prologue_randoms(seed: int, offset: int, n_rays: int, n_jitter: int):
    """What fnr_train_prologue writes for rays 0 .. n_rays - 1 of step (seed, offset), as step_randoms.hpp states it:
    u [R,3] = words 0-2 of word group 0 (image, y, x of the pixel); jitter [n_jitter, R] (n_jitter <= 5) = word 3 of group 0,
    then words 0-3 of group 1 (the samplers' single jitters, level by level).  float32 numpy arrays."""
    assert 0 <= n_jitter <= 5
    g0 = step_randoms(seed, offset, n_rays, 0)
    g1 = step_randoms(seed, offset, n_rays, 1)
    rows = np.concatenate([g0[:, 3:4], g1], axis=1).T            # [5, R]
    return np.ascontiguousarray(g0[:, :3]), np.ascontiguousarray(rows[:n_jitter])
