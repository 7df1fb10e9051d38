"""The main field's hash-grid encode and its input gradient — fnr_hash_encode_fwd / fnr_hash_encode_lattice (hashgrid.hip:
k_hash_encode<RaySource>, <LatticeSource>: features, selector, the saved input Jacobian) and fnr_hash_encode_input_grad
(position_grad.hip: k_hash_input_grad), then both through their consumers (k_position_from_jacobian, k_position_reduce)
— against a float64 reference written in plain torch, per level, axis, sample and feature, never against a batch maximum.

Reference.  The unit-cube position x of every sample is taken as the float32 value the kernel forms (the oracle's float32
operations in the oracle's order) and upcast; unselected samples (a coordinate outside (0, 1)) are encoded at position 0.
Features: float64 _encode of tests/test_gpu_proposal_kernels.py (corners from ceil / floor of x * scaling,
HashEncoding.hash_fn's hash, weights from scaled - floor), imported unchanged, and — wherever nerfstudio's class can
express the grid (every hash_scalings grid) — ns.HashEncoding in float32, bit for bit.  Jacobian: float64 autograd of
_encode(...)["feat"][l, :, f].sum() w.r.t. x, one backward per (l, f) (samples are independent) -> J[l, :, n, f];
expected jac[l, a, n, f] = selector J, partial[l, n, a] = selector sum_f d_feats[l, n, f] J[l, a, n, f].  The consumers
(d): float64 autograd through Frustums.get_positions -> contraction or AABB normalisation -> selector
(tests/test_gpu_ray_kernels.py: _ray_grad_ref, _contrib_scale) applied to the float64 unit-cube gradient sum_l,f d_feats J.

Geometries.  POINTS: warp mode 1, unit box, S = 1, zero directions, origins = x, so x reaches the kernel bit for bit; the
28 edge samples of _points are in (N >= 255: lattice points of the coarsest level and of 1 / 512 on one, two and three
axes, one ulp either side of a plane, the faces, one ulp inside the faces).  RAYS: warp mode 0, _rays(R, S) with R S = N
exactly and bins out to t = 1000.  RUNS: _runs() of the scatter tests (runs of samples in one coarse cell across lane-row,
wave and workgroup boundaries).  AABB rays: warp mode 1 with the non-unit box of test_gpu_ray_kernels.AABB, about half of
the samples outside it.  LATTICE: LatticeArg 5 x 7 x 33 with unevenly spaced coordinates that reach beyond the box, ray
ranges (0, 35), (3, 29) (crosses ix boundaries with ray_begin != 0) and (34, 1), both warp modes — features and selector
only: the lattice entry point saves no Jacobian.

Grids (K.make_grid, no model; tables uniform in +-0.8): the GRIDS of tests/test_gpu_hash_scatter.py (small16 = 2^14 x
hash_scalings(16, 16, 2048), big16, edge2, rows8k, bins64, bins256, tiny6, tiny10), hs1 / hs5 / hs8 / hs12 = 2^14 x
hash_scalings(L, 16, 2048) (L % 8 != 0: the plain branch of decode_block; L = 8: one level per XCD) and default19 = 2^19 x
hash_scalings(16, 16, 2048).  N = 1, 2, 255, 511, 512, 513, 1000, 2100 on small16 (a 512-sample workgroup: two samples per
thread, the second slot clamped to N - 1 while the first is live; odd N: a lane pair whose odd lane is past the end),
N = 1000 everywhere else.

What a float64 reference and a float32 kernel may legitimately disagree on: the grid cell where fl32(x s) rounds ONTO an
integer.  Features are continuous there (they stay in, the u sc term covers them), the Jacobian is not.  Samples that
_near_lattice flags (|x s - rint(x s)| <= 4 ulp32 at some level and axis; points: only where the float32 product is
inexact, so the lattice-point and one-ulp edge samples stay in) leave checks (b) and get d_feats = 0 in (c), (d).  At
most 3 % of N for rays, under 1 % of the random points (the edge samples one ulp inside x = 1 are next to the last plane
of every level whose scaling is no power of two, by design) — asserted, and asserted for the reference alone in
tests/test_hash_encode_cpu.py.  The share is a property of the inputs alone: a window of 8 ulp32 around every plane is
about 2^-20.5 sum_l,a x_a s_l of the cube, 0.75 % for 16 levels up to 2048 and 1.1 % up to 4096, so the 1 % of the points
is tight there; POINT_SEED / RAY_SEED are seeds at which every case of this file is under its cap (big16: 9 of 1000).
The runs are the scatter file's fixed geometry and count as points: 12 of 1200 on small16, which is not under 1 %, so they
run on hs8 (every scaling a power of two, no sample leaves; decode_block's XCD branch) and hs12 (5 of 1200; plain branch).

Error model, u = 2^-24, first order (sc_a = |x_a s_l|, W_k the 8 corner weights, W'_a,k / W''_ab,k the weight with the
factor of axis a / of axes a and b left out, v_kf the corner rows):
  features  C_FEAT E_f,  E_f = u (9 sum_k W_k |v_k| + sum_a sc_a sum_k W'_a,k |v_k|)         (the proposal file's, C_FEAT = 8)
  Jacobian  C_JAC B,     B[l,a,n,f] = s_l (u sum_k W'_a,k |v_kf| + sum_{b != a} u sc_b sum_k W''_ab,k |v_kf|)
            the proposal file's d_position bound with |df| = 1, E_df = 0, one level and one feature: the first term is the
            roundings of blend_input_grad (a corner difference, two nested blends with 1 - o, the product with s), the
            second fl32(x s) carrying |d sc| <= u sc into the two other axes' offsets.
  partial   C_PART sum_f |d_feats[l,n,f]| B[l,a,n,f]          (k_hash_input_grad forms d_k = df . v_k first: one fma more)
  consumers (d), per ray and component: 1e-5 sum_n |J_warp^T g|_n (that file's bound for the reduction, the maximum over
            the components as there) + sum_n |J_warp^T| C_PART sum_l,f |d_feats| B (times t_mid for the directions)
  (e) contract_jacobian with random Jacobians of 8, 12, 16 levels: geometry and bound (1e-5 sum |contributions|) of
            test_position_grad_reduce_every_entry_point.
Exact: the selector everywhere; features of unselected samples = row 0 of the level; Jacobian and partial rows of
unselected samples = 0; Jacobian and partial on an axis whose float32 offset is 0 = 0 (ceil = floor there, the corner
pairs coincide and their differences vanish); partial[..., 3] = 0; rows of samples with d_feats = 0.
(The zeros of unselected samples do not depend on the `sel ?` in front of the scaling: warp_position has already moved
such a sample to x = 0, where all eight corners are row 0 and every corner difference is 0.  A build without the
`sel ?` in both producers passes this file; a build with one corner difference of blend_input_grad negated, or with two
axes of the Jacobian store swapped, fails (b), (c) and (d) on every grid.)

C_JAC = 6 and C_PART = 10 are not tuned against the kernel: the kernel's operations in the kernel's order (grid_cell,
blend_input_grad, s * g; library built with -ffp-contract=off) evaluated in float32 on the CPU over this module's own
inputs stay <= 1/4 of every bound (tests/test_hash_encode_cpu.py asserts it), which leaves the kernel 4x for another
order of summation.  Worst |err| / bound over every test of this file, [CPU float32, MI355X] (every assertion is <= 1):
  features                                       [0.115, 0.115]
  Jacobian                                       [0.236, 0.236]
  partial                                        [0.229, 0.229]
  consumers, from the Jacobian / from partial    [0.014, 0.014] / [0.014, 0.014]
  contract_jacobian 8 / 12 / 16 levels           [0.067, 0.062] / [0.059, 0.059] / [0.031, 0.041]
"""
import pytest
import torch

from oracle import ns_torch as ns
from tests import test_gpu_ray_kernels as rk
from tests.test_gpu_hash_scatter import GRIDS, RUNS, RUNS_N, _grid, _hash_scalings, _runs
from tests.test_gpu_proposal_kernels import (C_FEAT, F8, N_EDGE, SIDES, U, UNIT_BOX, _encode, _encode_scales, _near_lattice,
                                             _points, _rays, _selector)

pytestmark = pytest.mark.gpu

C_JAC, C_PART = 6.0, 10.0
FLOAT32 = "float32"           # `dev` of the CPU yardstick: the float32 evaluation of the kernel's operations in its place
WORST = {}                    # quantity -> worst ratio seen (printed by the tests, collected by the yardstick run)
NEAR = {}                     # geometry -> largest share of samples left out (collected by the yardstick run)
MUTATION = None               # CPU stand-ins of kernel bugs (tests/test_hash_encode_cpu.py): the float32 evaluation then has to fail
assert SIDES[0].tolist() == [1, 1, 1] and SIDES[6].tolist() == [0, 0, 0]      # corner 0 = ccc (weights o), 6 = fff (1 - o)

HS = {"hs1": 1, "hs5": 5, "hs8": 8, "hs12": 12}
ALL_GRIDS = GRIDS + list(HS) + ["default19"]
SMALL16_N = (1, 2, 255, 511, 512, 513, 1000, 2100)
RAY_SHAPES = {1: (1, 1), 2: (1, 2), 255: (15, 17), 511: (7, 73), 512: (16, 32), 513: (27, 19), 1000: (40, 25), 2100: (50, 42)}
LATTICE_RANGES = ((0, 35), (3, 29), (34, 1))
POINT_SEED, RAY_SEED = 9, 5     # of the inputs; the shares of samples next to a lattice plane they give are asserted


def _K():
    from fruitnerf_amd import _kernels as K
    return K


def _note(what, name, ratio):
    v = float(ratio.max()) if ratio.numel() else 0.0
    WORST[what] = max(WORST.get(what, 0.0), v)
    print(f"[hash encode] {what} {name}: worst |err| / bound = {v:.3g}")
    return v


# ---------------------------------------------------------------------------------------------------------------------
# grids and geometries (float32, CPU)
# ---------------------------------------------------------------------------------------------------------------------

_TABLES = {}


def _case_grid(name):
    """-> dict(name, log2_T, scal, table [L T, 2] uniform in +-0.8, hs = the HashEncoding arguments that express it | None)."""
    if name not in _TABLES:
        if len(_TABLES) > 3:
            _TABLES.clear()
        if name in HS:
            log2_T, scal, hs = 14, _hash_scalings(HS[name], 16, 2048), (HS[name], 16, 2048)
        elif name == "default19":
            log2_T, scal, hs = 19, _hash_scalings(16, 16, 2048), (16, 16, 2048)
        else:
            log2_T, scal = _grid(name)
            hs = {"small16": (16, 16, 2048), "big16": (16, 16, 4096)}.get(name)
        g = torch.Generator().manual_seed(1000 * len(scal) + log2_T + 7 * len(name))
        table = ((torch.rand(len(scal) << log2_T, 2, generator=g) * 2 - 1) * 0.8).contiguous()
        _TABLES[name] = dict(name=name, log2_T=log2_T, scal=[int(s) for s in scal], table=table, hs=hs)
    return _TABLES[name]


def _ray_case(N, seed=0):
    return dict(_rays(*RAY_SHAPES[N], seed=seed), aabb=UNIT_BOX)


def _point_case(N, seed=0):
    return dict(_points(8, N, seed), aabb=UNIT_BOX)            # L = 8 of the proposal scalings: lattice planes of 16 and of 512


def _aabb_case(R, S, seed=0):
    """Random rays across the non-unit box of the ray-kernel tests, warp mode 1 (_ray_geometry's mode 1 at any R)."""
    g = torch.Generator().manual_seed(11 * R + S + 1009 * seed)
    o = torch.randn(R, 3, generator=g) * 0.5
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    t = torch.sort(torch.rand(R, S + 1, generator=g) * 4.0, 1).values
    pos = o[:, None, :] + d[:, None, :] * (t[:, :-1, None] + t[:, 1:, None]) / 2         # Frustums.get_positions, float32
    x = ns.get_normalized_positions(pos, rk.AABB).reshape(-1, 3)
    return dict(mode=1, R=R, S=S, o=o.contiguous(), d=d.contiguous(), t=t.contiguous(), x=x.contiguous(), exempt_exact=False,
                n_edge=0, aabb=rk.AABB)


def _geometry_case(o, d, t, mode):
    """A geometry of test_gpu_ray_kernels._ray_geometry as a case of this file."""
    pos = o[:, None, :] + d[:, None, :] * (t[:, :-1, None] + t[:, 1:, None]) / 2
    x = rk._unit_cube(pos, mode).reshape(-1, 3)
    return dict(mode=mode, R=o.shape[0], S=t.shape[1] - 1, o=o, d=d, t=t, x=x.contiguous(), exempt_exact=False, n_edge=0,
                aabb=rk.AABB)


LATTICE_XS = torch.tensor([-1.7, -0.55, 0.1, 0.8125, 1.6])
LATTICE_YS = torch.tensor([-1.2, -0.9, -0.3, 0.0, 0.26, 0.875, 1.1])
LATTICE_ZS = (torch.cumsum(0.02 + 0.19 * torch.rand(33, generator=torch.Generator().manual_seed(33)), 0) - 0.9).contiguous()


def _lattice_case(mode, ray_begin, n_rays):
    """Samples [ray_begin, +n_rays) x 33 of the 5 x 7 x 33 lattice: ray r = ix * 7 + iy, sample k -> (xs[ix], ys[iy], zs[k])."""
    n_z = LATTICE_ZS.numel()
    r = torch.arange(ray_begin, ray_begin + n_rays).repeat_interleave(n_z)
    k = torch.arange(n_z).repeat(n_rays)
    pos = torch.stack([LATTICE_XS[r // LATTICE_YS.numel()], LATTICE_YS[r % LATTICE_YS.numel()], LATTICE_ZS[k]], 1)
    return dict(mode=mode, lattice=(ray_begin, n_rays), x=rk._unit_cube(pos, mode).contiguous(), exempt_exact=False, n_edge=0,
                aabb=rk.AABB)


def _near(case, grid, what):
    """The samples next to a lattice plane, with their cap: under 1 % of the random points, 3 % of N for the ray geometries."""
    near = _near_lattice(case, grid["scal"])
    N = case["x"].shape[0]
    n = int(near[case["n_edge"]:].sum())
    NEAR[what] = max(NEAR.get(what, 0.0), n / N)
    if what == "points":
        assert n < 0.01 * N or n == 0, f"{n} of {N} points sit next to a lattice plane"
    else:
        assert n <= 0.03 * N, f"{n} of {N} samples ({what}) sit next to a lattice plane"
    return near


def _d_feats(L, N, near, seed):
    """[L,N,2]: 1e-2 randn, a few samples exactly 0 and a few 1e3 times the rest; 0 at the samples next to a lattice plane."""
    g = torch.Generator().manual_seed(seed)
    df = 1e-2 * torch.randn(L, N, 2, generator=g)
    zero = torch.zeros(N, dtype=torch.bool)
    if N >= 64:
        zero[torch.randint(0, N, (max(2, N // 200),), generator=g)] = True
        df[:, torch.randint(0, N, (max(2, N // 200),), generator=g)] *= 1e3
    df[:, zero | near] = 0.0
    return df.contiguous(), zero


# ---------------------------------------------------------------------------------------------------------------------
# the reference (float64) with its bounds
# ---------------------------------------------------------------------------------------------------------------------

def _reference(grid, x32, jacobian=True):
    """float64, level by level: feat [L,N,2], E_f [L,N,2], J [L,3,N,2] (without the selector), B [L,3,N,2] (the Jacobian's
    bound without its constant), sel [N], off0 [L,N,3] = the float32 offset is 0."""
    L, T, N = len(grid["scal"]), 1 << grid["log2_T"], x32.shape[0]
    sel = _selector(x32)
    xm32 = x32 * sel[:, None]
    out = dict(sel=sel, feat=torch.empty(L, N, 2, dtype=F8), E_f=torch.empty(L, N, 2, dtype=F8),
               J=torch.zeros(L, 3, N, 2, dtype=F8), B=torch.zeros(L, 3, N, 2, dtype=F8))
    sc32 = xm32[None] * torch.tensor(grid["scal"], dtype=torch.float32)[:, None, None]
    out["off0"] = (sc32 - torch.floor(sc32)) == 0
    for l, s in enumerate(grid["scal"]):
        x = xm32.double().requires_grad_(jacobian)
        e = _encode(grid["table"][l * T:(l + 1) * T].double(), x, [s], grid["log2_T"])
        out["feat"][l] = e["feat"][0].detach()
        out["E_f"][l] = _encode_scales(e).view(N, 1, 2)[:, 0]
        if not jacobian:
            continue
        for f in range(2):
            out["J"][l, :, :, f] = torch.autograd.grad(e["feat"][0, :, f].sum(), x, retain_graph=f == 0)[0].T
        wa, av, sc = [w.detach()[0] for w in e["wa"]], e["v"].detach()[0].abs(), e["sc"][0]       # [N,8], [N,8,2], [N,3]
        for a in range(3):
            o1, o2 = (a + 1) % 3, (a + 2) % 3
            first = ((wa[o1] * wa[o2])[..., None] * av).sum(1)
            second = sum(sc[:, b, None] * (wa[3 - a - b][..., None] * av).sum(1) for b in (o1, o2))
            out["B"][l, a] = float(s) * U * (first + second)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the kernels, and the float32 evaluation of their operations (the yardstick)
# ---------------------------------------------------------------------------------------------------------------------

def _pieces32(grid, x32):
    """grid_cell and the gathers in float32 -> selector [N], corner rows v [L,N,8,2], offsets o [L,N,3]."""
    sel = _selector(x32)
    e = _encode(grid["table"], x32 * sel[:, None], grid["scal"], grid["log2_T"])
    return sel, e["v"], torch.stack([e["wa"][a][..., 0] for a in range(3)], -1)


def _interp32(v, o):
    """common.hpp grid_interp (HashEncoding.forward's blend): v [L,N,8,2], o [L,N,3] -> [L,N,2]"""
    ox, oy, oz = (o[..., a, None] for a in range(3))
    lerp = lambda p, q, w: p * w + q * (1 - w)   # noqa: E731
    f03, f12 = lerp(v[:, :, 0], v[:, :, 3], ox), lerp(v[:, :, 1], v[:, :, 2], ox)
    f56, f47 = lerp(v[:, :, 5], v[:, :, 6], ox), lerp(v[:, :, 4], v[:, :, 7], ox)
    return lerp(lerp(f03, f12, oy), lerp(f47, f56, oy), oz)


def _blend_input_grad32(d, o):
    """hash_sources.hpp blend_input_grad: d [L,N,8,F], o [L,N,3] -> [L,N,3,F]"""
    ox, oy, oz = (o[..., a, None] for a in range(3))
    mx, my, mz = 1.0 - ox, 1.0 - oy, 1.0 - oz
    d = [d[:, :, k] for k in range(8)]
    sign = -1.0 if MUTATION == "corner sign" else 1.0
    g0 = oz * (oy * (d[0] - d[3]) + my * (d[1] - d[2])) + mz * (oy * (d[4] - d[7]) + my * sign * (d[5] - d[6]))
    g1 = oz * (ox * (d[0] - d[1]) + mx * (d[3] - d[2])) + mz * (ox * (d[4] - d[5]) + mx * (d[7] - d[6]))
    g2 = oy * (ox * (d[0] - d[4]) + mx * (d[3] - d[7])) + my * (ox * (d[1] - d[5]) + mx * (d[2] - d[6]))
    return torch.stack([g1, g0, g2] if MUTATION == "swapped axes" else [g0, g1, g2], 2)


def _scale32(grid, sel):
    return torch.tensor(grid["scal"], dtype=torch.float32)[:, None] * sel                            # sel ? scaling : 0


def _device_table(dev, grid):
    return None if dev == FLOAT32 else grid["table"].to(dev).contiguous()


def _device_args(dev, grid, case, table):
    K = _K()
    rays = K.RaysArg(case["o"].to(dev), case["d"].to(dev), None, None)
    return (K.make_grid(table, len(grid["scal"]), grid["log2_T"], grid["scal"]), K.make_warp(case["mode"], case["aabb"]), rays,
            case["t"].to(dev).contiguous(), case["S"])


def _encode_any(dev, grid, case, table, want_jacobian=True):
    """-> feats [L,N,2], selector [N] (uint8), jac [L,3,N,2] | None — CPU tensors."""
    if dev == FLOAT32:
        sel, v, o = _pieces32(grid, case["x"])
        jac = None
        if want_jacobian and "lattice" not in case:
            jac = (_scale32(grid, sel)[:, None, :, None] * _blend_input_grad32(v, o).permute(0, 2, 1, 3)).contiguous()
        return _interp32(v, o), sel.to(torch.uint8), jac
    K = _K()
    if "lattice" in case:
        lat = K.LatticeArg(LATTICE_XS.to(dev), LATTICE_YS.to(dev), LATTICE_ZS.to(dev))
        g = K.make_grid(table, len(grid["scal"]), grid["log2_T"], grid["scal"])
        out = K.hash_encode_lattice(g, K.make_warp(case["mode"], case["aabb"]), lat, *case["lattice"]) + (None,)
    else:
        out = K.hash_encode_fwd(*_device_args(dev, grid, case, table), want_jacobian=want_jacobian)
        out = out if want_jacobian else out + (None,)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in out)


def _input_grad_any(dev, grid, case, table, df):
    """fnr_hash_encode_input_grad -> partial [L,N,4] (CPU)."""
    if dev == FLOAT32:
        sel, v, o = _pieces32(grid, case["x"])
        d = df[:, :, None, 0] * v[..., 0] + df[:, :, None, 1] * v[..., 1]                 # fmaf(gf.x, v.x, gf.y * v.y)
        g = _scale32(grid, sel)[..., None] * _blend_input_grad32(d[..., None], o)[..., 0]
        return torch.cat([g, torch.zeros_like(g[..., :1])], -1).contiguous()
    out = _K().hash_encode_input_grad(*_device_args(dev, grid, case, table), df.to(dev).contiguous())
    torch.cuda.synchronize()
    return out.cpu()


def _ray_sums32(case, g_unit):
    """The consumers' chain in float32 on the CPU: autograd of sum g . x(p) w.r.t. origins and directions."""
    o = case["o"].clone().requires_grad_(True)
    d = case["d"].clone().requires_grad_(True)
    t, S = case["t"], case["S"]
    p = o[:, None, :] + d[:, None, :] * (t[:, :-1, None] + t[:, 1:, None]) / 2
    (rk._unit_cube(p, case["mode"]) * g_unit.view(-1, S, 3)).sum().backward()
    return o.grad, d.grad


def _from_jacobian_any(dev, case, jac, df):
    if dev == FLOAT32:
        g = torch.zeros(jac.shape[2], 3)
        for l in range(jac.shape[0]):                                                # contract_jacobian: level by level
            g = g + (df[l, :, None, 0] * jac[l, :, :, 0].T + df[l, :, None, 1] * jac[l, :, :, 1].T)
        return _ray_sums32(case, g)
    K = _K()
    R = case["R"]
    d_o, d_d = torch.zeros(R, 3, device=dev), torch.zeros(R, 3, device=dev)
    K.position_grad_from_jacobian(K.make_warp(case["mode"], case["aabb"]), K.RaysArg(case["o"].to(dev), case["d"].to(dev), None, None),
                                  case["t"].to(dev).contiguous(), case["S"], jac.to(dev).contiguous(), df.to(dev).contiguous(), d_o, d_d)
    torch.cuda.synchronize()
    return d_o.cpu(), d_d.cpu()


def _reduce_any(dev, case, partial):
    if dev == FLOAT32:
        g = torch.zeros(partial.shape[1], 3)
        for l in range(partial.shape[0]):
            g = g + partial[l, :, :3]
        return _ray_sums32(case, g)
    K = _K()
    R = case["R"]
    d_o, d_d = torch.zeros(R, 3, device=dev), torch.zeros(R, 3, device=dev)
    K.position_grad_reduce(K.make_warp(case["mode"], case["aabb"]), K.RaysArg(case["o"].to(dev), case["d"].to(dev), None, None),
                           case["t"].to(dev).contiguous(), case["S"], partial.to(dev).contiguous(), d_o, d_d)
    torch.cuda.synchronize()
    return d_o.cpu(), d_d.cpu()


# ---------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------

def _check_features(name, grid, case, ref, feats, selector):
    """(a) selector exact, row 0 at unselected samples, float64 within C_FEAT E_f, ns.HashEncoding bit for bit."""
    L, T = len(grid["scal"]), 1 << grid["log2_T"]
    sel = ref["sel"]
    assert selector.dtype == torch.uint8 and torch.equal(selector.bool(), sel), f"{name}: selector"
    assert bool((selector <= 1).all())
    row0 = grid["table"][torch.arange(L) * T]                                                       # hash(0,0,0) = 0
    assert torch.equal(feats[:, ~sel], row0[:, None, :].expand(-1, int((~sel).sum()), -1)), f"{name}: features of unselected samples"
    if grid["hs"] is not None:
        enc = ns.HashEncoding(num_levels=grid["hs"][0], min_res=grid["hs"][1], max_res=grid["hs"][2], log2_hashmap_size=grid["log2_T"])
        assert [int(s) for s in enc.scalings.tolist()] == grid["scal"]
        with torch.no_grad():
            enc.hash_table.copy_(grid["table"])
            want = enc(case["x"] * sel[:, None]).view(-1, L, 2).permute(1, 0, 2)
        assert torch.equal(feats, want), f"{name}: features differ from HashEncoding's in {int((feats != want).sum())} entries"
    return _note("features", name, (feats.double() - ref["feat"]).abs() / (C_FEAT * ref["E_f"] + 1e-300))


def _check_jacobian(name, ref, near, jac):
    """(b) per level, axis, sample and feature."""
    sel, keep = ref["sel"], ref["sel"] & ~near
    L = jac.shape[0]
    assert jac.shape == ref["J"].shape
    assert not bool(jac[:, :, ~sel].any()), f"{name}: Jacobian of unselected samples"
    off0 = (ref["off0"] & sel[None, :, None]).permute(0, 2, 1)                                       # [L,3,N]
    assert not bool(jac[off0].any()), f"{name}: Jacobian on an axis whose offset is 0"
    assert not keep.any() or float(ref["J"][:, :, keep].abs().max()) > 0
    ratio = (jac.double() - ref["J"] * sel[None, None, :, None]).abs() / (C_JAC * ref["B"] + 1e-300)
    return _note("jacobian", name, ratio[:, :, keep]), int(off0.sum())


def _check_partial(name, ref, df, zero, near, partial):
    """(c) per level, sample and axis."""
    sel = ref["sel"]
    assert partial.shape == (df.shape[0], df.shape[1], 4)
    assert not bool(partial[..., 3].any()), f"{name}: partial[..., 3]"
    assert not bool(partial[:, ~sel | zero | near].any()), f"{name}: partial of unselected or zero-d_feats samples"
    assert not bool(partial[..., :3][(ref["off0"] & sel[None, :, None])].any()), f"{name}: partial on an axis whose offset is 0"
    want = torch.einsum("lnf,lanf->lna", df.double(), ref["J"]) * sel[None, :, None]
    bound = C_PART * torch.einsum("lnf,lanf->lna", df.double().abs(), ref["B"])
    assert float(want.abs().max()) > 0 or not bool((sel & ~zero & ~near).any())
    return _note("partial", name, (partial[..., :3].double() - want).abs() / (bound + 1e-300))


def _check_all(dev, grid, case, name, what, table, seed):
    """(a), (b), (c) of one geometry on one grid -> worst ratio, the (level, sample, axis) entries of offset 0, the reference."""
    L, N = len(grid["scal"]), case["x"].shape[0]
    ref = _reference(grid, case["x"])
    near = _near(case, grid, what)
    feats, selector, jac = _encode_any(dev, grid, case, table)
    worst = [_check_features(name, grid, case, ref, feats, selector)]
    w, n_off0 = _check_jacobian(name, ref, near, jac)
    df, zero = _d_feats(L, N, near, seed)
    worst += [w, _check_partial(name, ref, df, zero, near, _input_grad_any(dev, grid, case, table, df))]
    return max(worst), n_off0, ref


# ---------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["points", "rays"])
@pytest.mark.parametrize("name", ALL_GRIDS)
def test_features_jacobian_and_input_grad_per_sample(dev, name, kind):
    """(a), (b), (c) on every grid: N = 1 .. 2100 on small16, 1000 elsewhere; points carry the 28 edge samples, whose
    lattice points must give exact zeros on the axes that sit on a plane."""
    grid = _case_grid(name)
    table = _device_table(dev, grid)
    worst = 0.0
    for N in (SMALL16_N if name == "small16" else (1000,)):
        case = _point_case(N, seed=POINT_SEED) if kind == "points" else _ray_case(N, seed=RAY_SEED)
        assert case["x"].shape[0] == N
        w, n_off0, ref = _check_all(dev, grid, case, f"{name}[{kind},N={N}]", kind, table, 3 + N)
        worst = max(worst, w)
        if kind == "points" and N >= 255:
            assert case["n_edge"] == N_EDGE and n_off0 >= 10 and int((~ref["sel"]).sum()) >= 6
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["hs8", "hs12"])
def test_runs_of_samples_in_one_cell(dev, name):
    """(a), (b), (c) on runs of 2 .. 513 consecutive samples in one coarse cell across the 16-lane, wave and workgroup
    boundaries, the last one ending on the last valid sample of a ragged workgroup: what the lane-pair gathers see when
    neighbouring lanes ask for the same rows."""
    grid = _case_grid(name)
    case = dict(_runs(), aabb=UNIT_BOX)
    x16 = torch.floor(case["x"] * 16.0)
    assert all(bool((x16[a:a + n] == x16[a]).all()) for a, n in RUNS) and RUNS[-1][0] + RUNS[-1][1] == RUNS_N == case["x"].shape[0]
    assert _check_all(dev, grid, case, f"{name}[runs]", "points", _device_table(dev, grid), 11)[0] <= 1.0


@pytest.mark.parametrize("name", ["small16", "hs5", "tiny6"])
def test_rays_through_a_non_unit_box(dev, name):
    """(a), (b), (c) in warp mode 1 with the box [-1.5, 1.5] x [-1, 1] x [-0.5, 2.5]: the division by the box lengths, and
    between a quarter and three quarters of the samples outside the box."""
    grid = _case_grid(name)
    case = _aabb_case(40, 25, seed=1)
    w, _, ref = _check_all(dev, grid, case, f"{name}[aabb rays]", "aabb rays", _device_table(dev, grid), 13)
    assert 0.25 <= float(ref["sel"].double().mean()) <= 0.75
    assert w <= 1.0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["small16", "hs5", "hs8", "tiny6"])
def test_lattice_source(dev, name, mode):
    """(a) through fnr_hash_encode_lattice: a 5 x 7 x 33 lattice with uneven coordinates beyond the box, ray ranges (0, 35),
    (3, 29) and (34, 1); each range equals its slice of the whole lattice bit for bit."""
    grid = _case_grid(name)
    table = _device_table(dev, grid)
    assert float(LATTICE_XS.abs().max()) > 1.5 and float(LATTICE_YS.abs().max()) > 1.0
    assert float(LATTICE_ZS.min()) < -0.5 < 2.5 < float(LATTICE_ZS.max())
    assert bool((LATTICE_ZS[1:] > LATTICE_ZS[:-1]).all()) and float(LATTICE_ZS.diff().max()) > 3 * float(LATTICE_ZS.diff().min())
    worst, whole = 0.0, None
    for begin, n_rays in LATTICE_RANGES:
        case = _lattice_case(mode, begin, n_rays)
        ref = _reference(grid, case["x"], jacobian=False)
        feats, selector, none = _encode_any(dev, grid, case, table)
        assert none is None and feats.shape == (len(grid["scal"]), n_rays * 33, 2)
        worst = max(worst, _check_features(f"{name}[lattice {mode},{begin}+{n_rays}]", grid, case, ref, feats, selector))
        if whole is None:
            whole = (feats, selector)
            assert mode == 0 or 0.2 <= float(ref["sel"].double().mean()) <= 0.8
        part = slice(begin * 33, (begin + n_rays) * 33)
        assert torch.equal(feats, whole[0][:, part]) and torch.equal(selector, whole[1][part])
    assert worst <= 1.0


@pytest.mark.parametrize("S", [48, 129])
@pytest.mark.parametrize("mode", [0, 1])
def test_both_producers_through_their_consumers(dev, mode, S):
    """(d) 19 rays x S samples, 16 levels: the device's own Jacobian through position_grad_from_jacobian and its own partial
    through position_grad_reduce, each against float64 autograd end to end, per ray and component."""
    grid = _case_grid("small16")
    table = _device_table(dev, grid)
    o, d, t = rk._ray_geometry(S, torch.Generator().manual_seed(100 * mode + S), mode)
    case = _geometry_case(o, d, t, mode)
    R, N = case["R"], case["x"].shape[0]
    ref = _reference(grid, case["x"])
    near = _near(case, grid, "rays" if mode == 0 else "aabb rays")
    df, _ = _d_feats(16, N, near, 17 + S)
    sel = ref["sel"]
    g_unit = (torch.einsum("lnf,lanf->na", df.double(), ref["J"]) * sel[:, None]).view(R, S, 3)
    ref_o, ref_d, sel64 = rk._ray_grad_ref(o, d, t, g_unit, mode)
    assert torch.equal(sel64.reshape(-1), sel) and float(ref_o.abs().max()) > 0
    mag_o, mag_d = rk._contrib_scale(o, d, t, g_unit, mode)
    # the per-sample bound of (c), summed over the levels, through |J_warp^T| (and times t_mid)
    E = (C_PART * torch.einsum("lnf,lanf->na", df.double().abs(), ref["B"]) * sel[:, None])
    t64 = t.double()
    tm = ((t64[:, :-1] + t64[:, 1:]) / 2)[..., None]
    p = (o.double()[:, None, :] + d.double()[:, None, :] * tm).reshape(-1, 3).requires_grad_(True)
    x = rk._unit_cube(p, mode)
    Ep = sum(torch.autograd.grad(x[:, a].sum(), p, retain_graph=True)[0].abs() * E[:, a, None] for a in range(3)).view(R, S, 3)
    bound_o, bound_d = 1e-5 * mag_o + Ep.sum(1), 1e-5 * mag_d + (Ep * tm).sum(1)
    feats, selector, jac = _encode_any(dev, grid, case, table)
    partial = _input_grad_any(dev, grid, case, table, df)
    worst = 0.0
    for what, (d_o, d_d) in (("via jacobian", _from_jacobian_any(dev, case, jac, df)), ("via partial", _reduce_any(dev, case, partial))):
        worst = max(worst, _note(what, f"[{mode},{S}].d_origins", (d_o.double() - ref_o).abs() / (bound_o + 1e-300)),
                    _note(what, f"[{mode},{S}].d_directions", (d_d.double() - ref_d).abs() / (bound_d + 1e-300)))
    assert worst <= 1.0


@pytest.mark.parametrize("levels", [8, 12, 16])
@pytest.mark.parametrize("mode", [0, 1])
def test_contract_jacobian_at_every_loop_shape(dev, mode, levels):
    """(e) position_grad_from_jacobian with random Jacobians of 8 (one unrolled pass), 12 (a pass and a tail of 4) and 16
    levels (two passes): geometry and bound of test_position_grad_reduce_every_entry_point (S = 1, 48, 129, 512; 1e-5 of
    the sum of the per-sample |contributions|)."""
    g = torch.Generator().manual_seed(10 * levels + mode)
    worst = 0.0
    for S in (1, 48, 129, 512):
        o, d, t = rk._ray_geometry(S, g, mode)
        case = _geometry_case(o, d, t, mode)
        R, sel = case["R"], _selector(case["x"])
        jac = torch.randn(levels, 3, R * S, 2, generator=g)
        df = torch.randn(levels, R * S, 2, generator=g)
        jac[:, :, ~sel] = 0.0
        gj = torch.einsum("lanf,lnf->na", jac.double(), df.double()).view(R, S, 3)
        ref_o, ref_d, _ = rk._ray_grad_ref(o, d, t, gj, mode)
        mag_o, mag_d = rk._contrib_scale(o, d, t, gj, mode)
        d_o, d_d = _from_jacobian_any(dev, case, jac.contiguous(), df.contiguous())
        name = f"[{mode},{levels} levels,S={S}]"
        worst = max(worst, _note("contract", name + ".d_origins", (d_o.double() - ref_o).abs() / (1e-5 * mag_o + 1e-300)),
                    _note("contract", name + ".d_directions", (d_d.double() - ref_d).abs() / (1e-5 * mag_d + 1e-300)))
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["small16", "hs5"])
def test_repeatability_and_want_jacobian(dev, name):
    """(f) Two calls give the same bits for features, selector, Jacobian and partial; a call without the Jacobian gives the
    same features and selector."""
    grid = _case_grid(name)
    table = _device_table(dev, grid)
    for case in (_ray_case(2100, seed=8), _point_case(513, seed=8)):
        df, _ = _d_feats(len(grid["scal"]), case["x"].shape[0], torch.zeros(case["x"].shape[0], dtype=torch.bool), 19)
        first = _encode_any(dev, grid, case, table) + (_input_grad_any(dev, grid, case, table, df),)
        second = _encode_any(dev, grid, case, table) + (_input_grad_any(dev, grid, case, table, df),)
        for what, a, b in zip(("features", "selector", "jacobian", "partial"), first, second):
            assert torch.equal(a, b) and not bool(torch.isnan(a.float()).any()), f"{name}: {what} differs between two calls"
        feats, selector, none = _encode_any(dev, grid, case, table, want_jacobian=False)
        assert none is None and torch.equal(feats, first[0]) and torch.equal(selector, first[1])
