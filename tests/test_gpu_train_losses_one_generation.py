"""fnr_train_losses after its kernel was specialised per samples-per-lane (two, four, eight) and the distortion metric moved
into the interlevel wave of the smallest proposal level: against the separate launches (fnr_losses_fwd, fnr_interlevel_fwd per
level, fnr_distortion, fnr_weights_bwd) bit for bit where the arithmetic is the same — every gradient — and against the float64
references of tests/test_gpu_ray_kernels.py, with that file's bars, for the five scalars (their sums are fixed point in the one
launch, float in the separate ones).

Shapes: R = 5 and 259 (no multiple of the 4 rays of a workgroup; 259 needs a second 256-ray rgb / semantic workgroup); S_f = 7
and 48; proposal levels (96, 256) — the two- / four-wide boundary and the shapes of a training step —, (64, 65) — one / two
samples per lane —, (1,) — a single level whose LDS region (3 + 4 floats) cannot hold the distortion scratch (2 S_f): the metric
keeps workgroups of its own — and (512, 2): the eight-wide form, the distortion hosted by the two-sample level."""
import ctypes as C
import math

import pytest
import torch

from oracle import ns_torch as ns
from tests import test_gpu_ray_kernels as rk

pytestmark = pytest.mark.gpu

F8 = torch.float64
SEM_W = rk.SEM_W
LEVELS = [(96, 256), (64, 65), (1,), (512, 2)]


def _call(dev, inp, prop, want_distortion, fuse, give_dwp, accum):
    """fnr_train_losses itself (fruitnerf_amd._kernels.train_losses never passes d_weights_p together with d_density_p).
    -> losses [5], d_rgb, d_sem, [d_wp per level or None], [d_density per level or None]"""
    from fruitnerf_amd import _lib as L
    lib = L.load()
    rgb, image, sem, mask, c, w = inp
    R, S_f, n = rgb.shape[0], w.shape[1], len(prop)
    losses = torch.empty(5, device=dev)
    d_rgb, d_sem = torch.empty(R, 3, device=dev), torch.empty(R, device=dev)
    d_wp = [torch.full((R, p[0]), float("nan"), device=dev) for p in prop] if give_dwp else None
    d_dn = [torch.full((R, p[0]), float("nan"), device=dev) for p in prop] if fuse else None

    def vps(ts):
        return None if ts is None else (C.c_void_p * max(n, 1))(*[L.ptr(t) for t in ts])
    sp = (C.c_int * max(n, 1))(*[p[0] for p in prop])
    rc = lib.fnr_train_losses(R, L.ptr(rgb), L.ptr(image), L.ptr(sem), L.ptr(mask), float(SEM_W), L.ptr(d_rgb), L.ptr(d_sem),
                              S_f, L.ptr(c), L.ptr(w), n, sp, vps([p[1] for p in prop]), vps([p[2] for p in prop]), vps(d_wp),
                              vps([p[3] for p in prop]) if fuse else None, vps([p[4] for p in prop]) if fuse else None,
                              vps(d_dn), 1.0, 1 if want_distortion else 0, L.ptr(accum), L.ptr(losses), L.stream_ptr(dev))
    L.check(rc, "train_losses")
    return losses, d_rgb, d_sem, d_wp, d_dn


def _inputs(R, S_f, levels, dev):
    """The batches of test_gpu_ray_kernels.test_train_losses_against_float64 (weights on a 2^-12 grid, proposal densities whose
    get_weights gives the grid weights) -> device inputs, device levels, CPU copies."""
    g = torch.Generator().manual_seed(1000 * R + 10 * S_f + len(levels) + levels[0])
    rgb, image, sem, mask = rk._loss_inputs(max(R, 14), g)
    rgb, image, sem, mask = (t[:R].contiguous() for t in (rgb, image, sem, mask))
    c, w = rk._dyadic_hist(R, S_f, g)
    prop = []
    for S_p in levels:
        cp, wp = rk._dyadic_hist(R, S_p, g)
        wp = wp / 2 ** math.ceil(math.log2(max(float(wp.sum(1).max()), 1e-9) + 1e-9))
        ep = torch.cumsum(torch.rand(R, S_p + 1, generator=g) * 0.05 + 0.01, 1)
        delta = (ep[:, 1:] - ep[:, :-1]).double()
        T = 1 - torch.cat([torch.zeros(R, 1, dtype=F8), torch.cumsum(wp.double(), 1)[:, :-1]], 1)
        dn = (-torch.log1p(-wp.double() / T) / delta).float()
        prop.append((S_p, cp.contiguous(), wp.contiguous(), ep.contiguous(), dn.contiguous()))
    cpu = (rgb, image, sem, mask, c, w)
    return tuple(t.to(dev) for t in cpu), [(p[0],) + tuple(t.to(dev) for t in p[1:]) for p in prop], cpu, prop


@pytest.fixture(scope="module")
def reference(dev):
    """(R, S_f, levels) -> inputs and everything they are compared with, computed once."""
    cache = {}

    def get(R, S_f, levels):
        key = (R, S_f, levels)
        if key in cache:
            return cache[key]
        from fruitnerf_amd import _kernels as K, _lib as L
        inp, prop, cpu, prop_cpu = _inputs(R, S_f, levels, dev)
        rgb, image, sem, mask, c, w = inp
        _, ref_drgb, ref_dsem = K.losses_fwd(rgb, image, sem, mask, SEM_W)
        slots = torch.zeros(L.FNR_LOSS_SLOTS, device=dev)
        ref_dwp = [K.interlevel_fwd(S_f, c, w, p[0], p[1], p[2], 1.0, slots) for p in prop]
        one = torch.ones(1, device=dev)
        ref_ddn = [K.weights_bwd(p[0], p[3], p[4], p[2], g, one) for p, g in zip(prop, ref_dwp)]
        # float64: the five scalars
        ref = rk._losses_ref(*cpu[:4])
        il = sum(ns.lossfun_outer(cpu[4].double(), cpu[5].double(), p[1].double(), p[2].double()).mean() for p in prop_cpu)
        dist = ns.lossfun_distortion(cpu[4].double(), cpu[5].double()).mean()
        want = torch.stack([ref[0], ref[1], ref[2], torch.as_tensor(il, dtype=F8), dist])
        n_waves = 4 * ((R + 255) // 256)
        fix = torch.tensor([n_waves * 2.0 ** -35 / (3 * R), n_waves * 2.0 ** -35 / R * SEM_W, 0.0,
                            R * len(levels) * 2.0 ** -35, R * 2.0 ** -35], dtype=F8)      # fixed-point slots: 2^-34 each
        fix[2] = 10 / math.log(10) * fix[0] / want[0]
        cache[key] = dict(inp=inp, prop=prop, d_rgb=ref_drgb, d_sem=ref_dsem, d_wp=ref_dwp, d_dn=ref_ddn, want=want, fix=fix)
        return cache[key]
    return get


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("S_f", [7, 48])
@pytest.mark.parametrize("R", [5, 259])
def test_one_launch_is_the_separate_launches(dev, reference, R, S_f, levels):
    """Every gradient bit-identical to the separate launches' (d_rgb, d_sem, d_wp; fused: d_density == fnr_weights_bwd of the
    separate d_wp, with d_wp written as well where a buffer is given); the five scalars against float64 at 2e-6 relative plus
    the fixed-point term; distortion on and off; each combination twice on the accumulator the call before left behind."""
    from fruitnerf_amd import _lib as L
    ref = reference(R, S_f, levels)
    accum = torch.zeros(L.FNR_TRAIN_LOSSES_ACCUM_FLOATS, device=dev)
    for want_distortion in (False, True):
        for fuse, give_dwp in ((False, True), (True, False), (True, True)):
            first = None
            for _ in range(2):
                losses, d_rgb, d_sem, d_wp, d_dn = _call(dev, ref["inp"], ref["prop"], want_distortion, fuse, give_dwp, accum)
                tag = f"R={R} S_f={S_f} levels={levels} distortion={want_distortion} fuse={fuse} d_wp={give_dwp}"
                assert torch.equal(d_rgb, ref["d_rgb"]) and torch.equal(d_sem, ref["d_sem"]), tag
                if give_dwp:
                    for a, b in zip(d_wp, ref["d_wp"]):
                        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), tag
                if fuse:
                    for a, b in zip(d_dn, ref["d_dn"]):
                        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), tag
                want = ref["want"].clone()
                if not want_distortion:
                    want[4] = 0.0
                got = losses.cpu().double()
                ratio = (got - want).abs() / (2e-6 * want.abs() + ref["fix"])
                assert rk._worst(f"train_losses one launch [{tag}]", ratio) <= 1.0, (got.tolist(), want.tolist())
                if not want_distortion:
                    assert float(got[4]) == 0.0
                assert float(accum.abs().max()) == 0.0, tag          # self-cleaned
                if first is None:
                    first = losses.clone()
                assert torch.equal(first.view(torch.int32), losses.view(torch.int32)), tag


@pytest.mark.parametrize("levels", [(96, 256), (1,)])
def test_a_non_finite_contribution_still_gives_nan_scalars(dev, reference, levels):
    """A NaN weight in one ray of the final level reaches the interlevel sum and the distortion sum, whichever wave forms them
    (hosted by the 96-sample level's waves; workgroups of its own beside the one-sample level): the scalars are NaN, the
    accumulator comes back clean and the next call is finite again."""
    from fruitnerf_amd import _lib as L
    ref = reference(5, 48, levels)
    rgb, image, sem, mask, c, w = ref["inp"]
    w_bad = w.clone()
    w_bad[3, 11] = float("nan")
    accum = torch.zeros(L.FNR_TRAIN_LOSSES_ACCUM_FLOATS, device=dev)
    losses, *_ = _call(dev, (rgb, image, sem, mask, c, w_bad), ref["prop"], True, True, False, accum)
    assert bool(torch.isnan(losses).all()), losses.tolist()
    assert float(accum.abs().max()) == 0.0
    losses, *_ = _call(dev, ref["inp"], ref["prop"], True, True, False, accum)
    assert bool(torch.isfinite(losses).all()), losses.tolist()
