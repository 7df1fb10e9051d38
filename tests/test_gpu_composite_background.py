"""background_color = "white" | "black" | "random" and use_gradient_scaling (Nerfacto's switches, fruit_nerf.py:164, 280-281,
322-323) in the compositing kernels, on the GPU.

Kernel level: the four `_opt` compositing calls against float64 autograd of comp + b (1 - acc) written in
tests/composite_background_reference.py (pinned on oracle/ns_torch.py by tests/test_composite_background_cpu.py), per ray and
per element, on the regime batch of tests/test_gpu_ray_kernels.py and at that file's bounds: 2e-6 relative + A_k for forward
quantities, 1e-5 per ray for d_rgb / d_logit, 1e-4 of the two-term scale for d_density.  With scaling on, reference and
bound are multiplied by the float64 s_k and 4 * 2^-24 |ref| is added for the three roundings of the float32 s_k (add, square,
the final product).  The launches are each other bit for bit where the header says so.
Generator: bit-equal to a numpy Philox4x32-10.  Model level: fused step = autograd step (gradients to the bit, reported scalars to 1e-6), steps record and replay, the default
configuration makes the calls and gives the outputs it did."""
import copy
import functools

import pytest
import torch

from tests import composite_background_reference as ref
from tests import util
from tests.test_gpu_ray_kernels import SEM_W, U, _batch, _rays, _samples64, _two_term_scale, _weight_arith

pytestmark = pytest.mark.gpu

# E = 1, 2, 3, 8 with full and partial last lanes on the R = 15 regime batch (R % 4 == 3); R = 1 at S = 48
CASES = [(1, 15), (2, 15), (48, 15), (64, 15), (65, 15), (129, 15), (512, 15), (48, 1)]
RANDOM_ROWS = slice(9, 15)      # rows 0-8 of the batch are the regimes


def _K():
    from fruitnerf_amd import _kernels as K
    return K


@functools.lru_cache(maxsize=None)
def _case(S, R):
    """The batch of tests/test_gpu_ray_kernels.py at S (R = 1: one of its random rays) + a per-ray background, per-ray
    gradients, an image 0.25 off the composite and a mask — CPU tensors, shared by every test, never modified."""
    edges, dens, rgb, logit = _batch(S)
    if R == 1:
        edges, dens, rgb, logit = (t[9:10].contiguous() for t in (edges, dens, rgb, logit))
    g = torch.Generator().manual_seed(1000 * S + R)
    bg = torch.rand(R, 3, generator=g)
    g_rgb = torch.randn(R, 3, generator=g)
    g_sem = torch.randn(R, generator=g)
    mask = (torch.arange(R) % 2).float()
    if R > 2:
        mask[1], mask[2] = 0.0, 1.0                                  # logits +-40 on the wrong side: |grad| ~ 1
    return edges, dens, rgb, logit, bg, g_rgb, g_sem, mask


def _backgrounds(bg):
    return {"white": torch.ones(3), "black": torch.zeros(3), "given": bg}


def _worst(name, ratio):
    v = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[composite background] {name}: worst |err| / bound = {v:.3g}")
    return v


# ---------------------------------------------------------------------------------------------------------------------
# preconditions, on the float64 reference alone
# ---------------------------------------------------------------------------------------------------------------------

def _density_bound(edges, dens, rgb, logit, b64, r, semgrad, gw_err=None):
    """1e-4 of the two-term scale (+ its floors) for d_density under the background colour b64 [R,3] (explicit, or the last
    sample's) — tests/test_gpu_ray_kernels._two_term_scale with |gw_k| = |g_rgb| . |c_k - b| (+ |g_sem| |logit_k|)."""
    gw_abs = (r["g_rgb"].abs()[:, None, :] * (rgb.double() - b64[:, None, :]).abs()).sum(-1)
    if semgrad:
        gw_abs = gw_abs + r["g_sem"].abs()[:, None] * logit.double().abs()
    return _two_term_scale(edges, dens, r["w"], gw_abs, gw_err)[0]


def test_preconditions_on_the_reference():
    """White against last_sample moves d_density by more than 100x its bound on more than 10 % of the elements of the random
    rays; every batch with S >= 48 has samples with s_k < 1 and samples with s_k = 1 (rows 6-8: integer edges, m_0 = 0.5);
    the empty ray composites to exactly the background.  No device involved."""
    for S, R in CASES:
        edges, dens, rgb, logit, bg, g_rgb, g_sem, mask = _case(S, R)
        white = ref.backward(edges, dens, rgb, logit, torch.ones(3), g_rgb=g_rgb, g_sem=g_sem)
        if R > 1:
            last = ref.backward(edges, dens, rgb, logit, None, g_rgb=g_rgb, g_sem=g_sem)
            bound = _density_bound(edges, dens, rgb, logit, torch.ones(R, 3, dtype=torch.float64), white, False)
            moved = ((white["d_density"] - last["d_density"]).abs() > 100 * bound)[RANDOM_ROWS]
            if S >= 2:      # (S = 1: the only sample IS the last one and c_0 - c_last = 0 is the whole gradient)
                assert float(moved.double().mean()) > 0.10, f"S={S}: {float(moved.double().mean()):.3f}"
            for name, b in _backgrounds(bg).items():
                out = ref.composite(white["w"], rgb.double(), b, True)
                assert torch.equal(out[0], b.double().expand(R, 3)[0]), f"S={S} {name}: empty ray"
        s64, s32 = ref.distance_scale64(edges), ref.distance_scale32(edges)
        if S >= 48 and R > 1:
            assert bool((s64 < 1).any()) and bool((s64 == 1).any()), f"S={S}"
            assert float(s64[6, 0]) == 0.25 and float(s32[6, 0]) == 0.25
        assert float((s32.double() - s64).abs().max()) <= 3 * U


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("S,R", CASES)
def test_composite_forward_with_explicit_background_per_ray(dev, S, R, training):
    """fnr_composite_fwd_opt for white, black and a per-ray buffer: rgb per ray at the forward bound of
    test_composite_forward_per_ray with |b| in the last sample's place; every other output is fnr_composite_fwd's, bit for
    bit; the empty ray is exactly the background; eval clamps (the batch's colours leave [0, 1]) and does not touch b."""
    K = _K()
    edges, dens, rgb, logit, bg, *_ = _case(S, R)
    rgb = rgb.clone()
    if not training and R > 1:
        rgb[3, S // 2 + 1:, 1] = float("nan")                           # behind the spike: nan_to_num in eval only
    rays = _rays(R, dev)
    ev, dv, cv, lv = edges.to(dev), dens.to(dev), rgb.to(dev), logit.to(dev)
    plain = K.composite_fwd(rays, S, ev, dv, cv, lv, training)
    w64 = _samples64(edges).get_weights(dens.double()[..., None])[..., 0]       # the oracle's weights
    acc64 = w64.sum(1)
    A = _weight_arith(edges, dens)
    ca = torch.nan_to_num(rgb.double()).abs()
    worst, clamped = [], False
    for name, b in _backgrounds(bg).items():
        got = K.composite_fwd_opt(rays, S, ev, dv, cv, lv, training, K.CompositeOptions(b.to(dev)))
        for i in (0, 2, 3, 4, 5):
            assert torch.equal(got[i], plain[i]), f"{name}: output {i} differs from composite_fwd"
        out = got[1].cpu().double()
        b64 = b.double().expand(R, 3)
        c64 = ref.composite(w64, rgb.double(), b, training)
        raw = ref.composite(w64, torch.nan_to_num(rgb.double()), b, True)
        s_rgb = 2e-6 * ((w64[..., None] * ca).sum(1) + b64.abs() * (1 + acc64[:, None])) + \
            (A[..., None] * (ca + b64.abs()[:, None, :])).sum(1)
        worst.append(((out - c64).abs() / (s_rgb + 1e-300)).max())
        if R > 1:
            assert torch.equal(got[1][0].cpu(), b.expand(R, 3)[0]), f"{name}: the empty ray is not exactly the background"
        if not training:
            assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0, name
            clamped = clamped or bool(((raw < 0) | (raw > 1)).any())
    assert training or clamped or S < 48 or R == 1, "no composite left [0, 1]: the clamp was not exercised"
    assert _worst(f"composite_fwd_opt[S={S} R={R} {'train' if training else 'eval'}].rgb", torch.stack(worst)) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------

def _check_grads(name, worst, case, b, got, r, inputs, semgrad, scaling):
    """tests/test_gpu_ray_kernels._check_composite_grads for a background b (None: the last sample), the semantic term
    (tests/test_gpu_semantic_gradients._density_ratio) and gradient scaling.  inputs: "given" | "rounded" | "own"."""
    edges, dens, rgb, logit = case[:4]
    R, S = dens.shape
    d_s, d_c, d_l = (t.cpu().double().view(R, S, *t.shape[1:]) for t in got)
    w64, g_sem, g_rgb_abs, sem64 = r["w"], r["g_sem"], r["g_rgb"].abs(), r["sem"]
    if inputs == "own":
        A = _weight_arith(edges, dens)
        la = logit.double().abs()
        sem_err = 2e-6 * (w64 * la).sum(1) + (A * la).sum(1)
    else:
        A = U * w64
        sem_err = U * sem64.abs() if inputs == "rounded" else torch.zeros_like(sem64)
    sig = torch.sigmoid(sem64)
    d_gs = SEM_W / R * sig * (1 - sig) * sem_err
    b64 = rgb.double()[:, -1, :] if b is None else b.double().expand(R, 3)
    gw_err = d_gs[:, None] * logit.double().abs() if (semgrad and inputs != "given") else None
    bounds = {"d_density": _density_bound(edges, dens, rgb, logit, b64, r, semgrad, gw_err)}
    cmax = r["d_rgb"].abs().flatten(1).max(1).values[:, None, None]
    bg_err = torch.zeros_like(r["d_rgb"])
    if b is None:   # the background share 1 - sum_k w_k on sample S-1: a float32 difference
        bg_err[:, -1, :] = g_rgb_abs * ((S + 63) // 64 + 6) * U + g_rgb_abs * A.sum(1, keepdim=True)
    bounds["d_rgb"] = 1e-5 * cmax + bg_err + g_rgb_abs[:, None, :] * A[..., None]
    lmax = r["d_logit"].abs().max(1, keepdim=True).values
    bounds["d_logit"] = 1e-5 * lmax + SEM_W * 2.0 ** -22 / R * w64 + g_sem.abs()[:, None] * A + d_gs[:, None] * (w64 + A)
    s64 = ref.distance_scale64(edges)
    for key, g in (("d_density", d_s), ("d_rgb", d_c), ("d_logit", d_l)):
        want, bound = r[key], bounds[key]
        if scaling:
            sk = s64[..., None] if key == "d_rgb" else s64
            want = want * sk
            bound = bound * sk + 4 * U * want.abs()
        worst.setdefault(f"{name}.{key}", []).append(((g - want).abs() / (bound + 1e-300)).max())


@pytest.mark.parametrize("S,R", CASES)
def test_composite_backward_with_options_per_element(dev, S, R):
    """fnr_composite_bwd_opt (given per-ray gradients), fnr_composite_bwd_targets_opt and fnr_composite_fwd_bwd_targets_opt
    for an explicit background — per ray (row stride 3) and one triple (white, row stride 0) — with scaling off and on and
    the semantic weights detached and attached, and for the last sample with scaling: d_density, d_rgb and d_logit per
    element against float64 autograd.  With scaling on every output is float32(s_k) x the unscaled output, bit for bit.
    [measured on an MI355X, worst err / bound over all cases: d_density 0.21 (fused, white, S = 512), d_rgb 0.19,
    d_logit 0.085]"""
    K = _K()
    case = _case(S, R)
    edges, dens, rgb, logit, bg, g_rgb, g_sem, mask = case
    rays = _rays(R, dev)
    ev, dv, cv, lv = edges.to(dev), dens.to(dev), rgb.to(dev), logit.to(dev)
    s32 = ref.distance_scale32(edges).to(dev).reshape(-1)
    worst = {}
    for bname, b in (("given", bg), ("white", torch.ones(3)), ("last_sample", None)):
        for semgrad in (False, True):
            r_g = ref.backward(edges, dens, rgb, logit, b, g_rgb=g_rgb, g_sem=g_sem, semantic_gradients=semgrad)
            image = (r_g["out"] + 0.25).float()
            r_t = ref.backward(edges, dens, rgb, logit, b, image=image, mask=mask, semantic_gradients=semgrad,
                               sem_weight=SEM_W)
            wk = r_g["w"].float().to(dev)
            c32, sem32 = r_t["out"].float().to(dev), r_t["sem"].float().to(dev)
            unscaled = None
            for scaling in (False, True):
                if b is None and not scaling:
                    continue        # the entry points without options: tests/test_gpu_ray_kernels.py
                opts = K.CompositeOptions(None if b is None else b.to(dev), scaling, semgrad)
                tag = f"{bname}{'+scale' if scaling else ''}{'+sem' if semgrad else ''}"
                got = {"bwd": K.composite_bwd_opt(rays, S, ev, dv, cv, lv, wk, g_rgb.to(dev), g_sem.to(dev), opts),
                       "targets": K.composite_bwd_targets_opt(rays, S, ev, dv, cv, lv, wk, c32, image.to(dev), sem32,
                                                              mask.to(dev), SEM_W, opts),
                       "fused": K.composite_fwd_bwd_targets_opt(rays, S, ev, dv, cv, lv, image.to(dev), mask.to(dev), SEM_W,
                                                                opts)[1]}
                _check_grads(f"bwd[{tag}]", worst, case, b, got["bwd"], r_g, "given", semgrad, scaling)
                _check_grads(f"targets[{tag}]", worst, case, b, got["targets"], r_t, "rounded", semgrad, scaling)
                _check_grads(f"fused[{tag}]", worst, case, b, got["fused"], r_t, "own", semgrad, scaling)
                if not scaling:
                    unscaled = got
                elif unscaled is not None:
                    for k in got:
                        for i, nm in enumerate(("d_density", "d_rgb", "d_logit")):
                            want = unscaled[k][i] * (s32[:, None] if i == 1 else s32)
                            assert torch.equal(got[k][i], want), f"{k}[{tag}].{nm} is not float32(s_k) x the unscaled output"
            if b is None:       # last sample + scaling against s_k x the entry points without options
                if semgrad:
                    plain = K.composite_bwd_semgrad(rays, S, ev, dv, cv, lv, wk, g_rgb.to(dev), g_sem.to(dev))
                else:
                    plain = K.composite_bwd(rays, S, ev, dv, cv, wk, g_rgb.to(dev), g_sem.to(dev))
                for i, nm in enumerate(("d_density", "d_rgb", "d_logit")):
                    want = plain[i] * (s32[:, None] if i == 1 else s32)
                    assert torch.equal(got["bwd"][i], want), f"bwd[last_sample+scale].{nm}"
    print(f"[composite background] S={S} R={R}: {len(worst)} quantities")
    top = sorted(((float(torch.stack(v).max()), k) for k, v in worst.items()), reverse=True)[:3]
    print(f"[composite background] S={S} R={R} worst three: {top}")
    for k, v in worst.items():
        assert float(torch.stack(v).max()) <= 1.0, (k, float(torch.stack(v).max()))


@pytest.mark.parametrize("S,R", CASES)
def test_options_launches_are_each_other(dev, S, R):
    """fnr_composite_bwd_targets_opt == fnr_train_losses -> fnr_composite_bwd_opt; fnr_composite_fwd_bwd_targets_opt ==
    fnr_composite_fwd_opt -> fnr_composite_bwd_targets_opt; with {last sample, no scaling} the four `_opt` entry points are
    the entry points without options — all bit for bit, semantic weights detached and attached."""
    from fruitnerf_amd import _lib as L
    K = _K()
    edges, dens, rgb, logit, bg, g_rgb, g_sem, mask = _case(S, R)
    rays = _rays(R, dev)
    ev, dv, cv, lv = edges.to(dev), dens.to(dev), rgb.to(dev), logit.to(dev)
    g0 = torch.Generator().manual_seed(S)
    image = torch.rand(R, 3, generator=g0).to(dev)
    mk = mask[:, None].to(dev)
    sp_f = torch.sort(torch.rand(R, S + 1, generator=g0), dim=-1).values.to(dev)
    accum = torch.zeros(L.FNR_TRAIN_LOSSES_ACCUM_FLOATS, device=dev)
    sem_w = 2.0
    names = ("weights", "rgb", "accumulation", "depth", "semantics", "labels")
    for b in (bg.to(dev), torch.ones(3, device=dev), None):
        for scaling in (False, True):
            for semgrad in (False, True):
                opts = K.CompositeOptions(b, scaling, semgrad)
                tag = f"bg={'last' if b is None else tuple(b.shape)} scale={scaling} sem={semgrad}"
                fwd = K.composite_fwd_opt(rays, S, ev, dv, cv, lv, True, opts)
                weights, out_rgb, _, _, out_sem, _ = fwd
                _, gr, gs, _ = K.train_losses(out_rgb, image, out_sem, mk, sem_w, S, sp_f, weights.view(R, S), [], 1.0, False,
                                              accum)
                given = K.composite_bwd_opt(rays, S, ev, dv, cv, lv, weights, gr, gs, opts)
                targets = K.composite_bwd_targets_opt(rays, S, ev, dv, cv, lv, weights, out_rgb, image, out_sem, mk, sem_w,
                                                      opts)
                fwd2, fused = K.composite_fwd_bwd_targets_opt(rays, S, ev, dv, cv, lv, image, mk, sem_w, opts)
                for nm, a, c in zip(names, fwd2, fwd):
                    assert torch.equal(a, c), f"{tag} fused forward {nm}"
                for nm, g, t, f in zip(("d_density", "d_rgb", "d_logit"), given, targets, fused):
                    assert torch.equal(t, g), f"{tag} targets {nm}: {int((t != g).sum())} of {g.numel()} differ"
                    assert torch.equal(f, g), f"{tag} fused {nm}: {int((f != g).sum())} of {g.numel()} differ"
                if opts.plain:
                    old_fwd = K.composite_fwd(rays, S, ev, dv, cv, lv, True)
                    if semgrad:
                        old = K.composite_bwd_semgrad(rays, S, ev, dv, cv, lv, weights, gr, gs)
                        old_t = K.composite_bwd_targets_semgrad(rays, S, ev, dv, cv, lv, weights, out_rgb, image, out_sem, mk,
                                                                sem_w)
                    else:
                        old = K.composite_bwd(rays, S, ev, dv, cv, weights, gr, gs)
                        old_t = K.composite_bwd_targets(rays, S, ev, dv, cv, weights, out_rgb, image, out_sem, mk, sem_w)
                    old_f2, old_f = K.composite_fwd_bwd_targets(rays, S, ev, dv, cv, lv, image, mk, sem_w, semgrad=semgrad)
                    for nm, a, c, d in zip(names, fwd, old_fwd, old_f2):
                        assert torch.equal(a, c) and torch.equal(a, d), f"{tag} plain forward {nm}"
                    for nm, g, a, c, d in zip(("d_density", "d_rgb", "d_logit"), given, old, old_t, old_f):
                        assert float(g.abs().max()) > 0 or S == 1, nm
                        assert torch.equal(g, a) and torch.equal(g, c) and torch.equal(g, d), f"{tag} plain {nm}"


# ---------------------------------------------------------------------------------------------------------------------
# the random background
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 257, 1000])
def test_random_background_is_philox(dev, R):
    """fnr_random_background against the numpy Philox4x32-10 of the reference module (counter (ray, group 2, offset), key
    seed, (x >> 8) 2^-24), bit for bit; in [0, 1); another offset, other numbers; a 64-bit seed and offset."""
    K = _K()
    for seed, offset in ((1, 1), (0x1234567890ABCDEF, 0x1_0000_0003)):
        got = K.random_background(seed, offset, R, dev).cpu()
        want = ref.random_background(seed, offset, R)
        assert got.shape == (R, 3) and torch.equal(got, want)
        assert float(got.min()) >= 0.0 and float(got.max()) < 1.0
        other = K.random_background(seed, offset + 1, R, dev).cpu()
        assert not torch.equal(other, got) and torch.equal(other, ref.random_background(seed, offset + 1, R))
    if R == 1000:
        assert 0.45 < float(got.mean()) < 0.55


def _image_set(dev, n_train=5, HW=24):
    from fruitnerf_amd.data import synthetic_apple as sa
    scene = sa.make_scene(seed=0, device=dev)
    c2w = sa.make_cameras(n_train, seed=0, device=dev)
    focal = 1111.0 * HW / 800
    return sa, sa.render_dataset(scene, c2w, H=HW, W=HW, fx=focal, fy=focal), n_train


def test_prologue_numbers_do_not_depend_on_the_generator(dev):
    """fnr_train_prologue for one (seed, offset) with and without fnr_random_background enqueued behind it: every output
    bit-identical; the batcher hands the background on as presampled["background"], drawn with the prologue's seed and
    offset, only when asked."""
    K = _K()
    sa, data, n_train = _image_set(dev)
    ids = torch.arange(n_train, device=dev)
    R, seed, offset = 257, 5, 9
    s = K.ImageSetArg(data["images"], data["masks"], data["c2w"], data["fx"], data["fy"], data["cx"], data["cy"])
    a = K.train_prologue(s, ids, R, seed, offset, None, 0.05, 1000.0, 32)
    b = K.train_prologue(s, ids, R, seed, offset, None, 0.05, 1000.0, 32)
    bgd = K.random_background(seed, offset, R, dev)
    torch.cuda.synchronize()
    for k, v in a.items():
        if torch.is_tensor(v):
            assert torch.equal(v, b[k]), k
    assert torch.equal(bgd.cpu(), ref.random_background(seed, offset, R))
    # words 0-2 of group 0 are the pixel draw: the background is none of the prologue's numbers
    assert not torch.equal(bgd, a["u"])
    level0 = {"S": 32, "near": 0.05, "far": 1000.0, "n_jitter": 3}
    outs = {}
    for want in (False, True):
        batcher = sa.PixelBatcher(data, ids, seed=seed)
        o, d, cam, batch = batcher.sample(R, level0=dict(level0, random_background=want))
        outs[want] = (o, d, cam, batch["image"], batch["fruit_mask"], batcher.last_presample["spacing"])
        assert ("background" in batcher.last_presample) is want
        if want:
            assert torch.equal(batcher.last_presample["background"].cpu(), ref.random_background(seed, 1, R))
    for x, y in zip(outs[False], outs[True]):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------

def _with(cfg, color, scaling, semgrad=False):
    cfg = copy.deepcopy(cfg)
    cfg.background_color, cfg.use_gradient_scaling, cfg.pass_semantic_gradients = color, scaling, semgrad
    return cfg


def _hip_model(om, dev, color, scaling, semgrad=False, test_mode=None):
    """The HIP model of an oracle model, made half transparent first: tests/util.randomize_ gives opaque rays (measured on the
    oracle: 1 - accumulation <= 1.8e-7, a background would not show); with the density logit's bias 6 lower the 160 rays of
    the step tests have 1 - accumulation between 0.2 and 0.77, median 0.59."""
    om = copy.deepcopy(om)
    with torch.no_grad():
        om.field.mlp_base_mlp.layers[1].bias[0].sub_(6.0)
    hm = util.make_hip_like(om, dev, test_mode=test_mode)
    hm.config.background_color, hm.config.use_gradient_scaling = color, scaling
    hm.config.pass_semantic_gradients = hm.field.pass_semantic_gradients = semgrad
    return hm


FUSED_CONFIGS = [("white", True, False), ("black", False, True), ("random", True, True), ("last_sample", True, False)]


@functools.lru_cache(maxsize=None)
def _fused_and_autograd(dev, color, scaling, semgrad):
    """One training step on the same rays, jitters and — for "random" — background through loss.backward() (the `_RenderFn`
    node: fnr_composite_bwd_opt), through fused_forward_backward, and through loss.backward() of the default configuration.
    -> [(loss dict, metrics dict, gradient arena)] x 3 and the arena's group slices."""
    from fruitnerf_amd.rays import RayBundle
    from fruitnerf_amd.training import fused_forward_backward
    from tests.test_gpu_training_parity import _batch as _image_batch
    cfg = util.small_config(log2=15, prop_log2=13)
    om = util.make_oracle(cfg, seed=9)
    R = 160
    o, d, pa, cam = util.random_rays(R, 7, seed=4)
    jit = [torch.rand(R, 1).to(dev) for _ in range(3)]
    hb = {k: v.to(dev) for k, v in _image_batch(R, 8).items()}
    background = ref.random_background(3, 1, R).to(dev)
    results = []
    for fused in (False, True, None):          # None: the autograd step of the default configuration
        hm = _hip_model(om, dev, *(("last_sample", False, semgrad) if fused is None else (color, scaling, semgrad)))
        hm.train()
        hm.set_anneal(0)
        rb = RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev), presampled={"background": background})
        if fused:
            ld, md = fused_forward_backward(hm, rb, hb, jitter=jit)
        else:
            out = hm(rb, jitter=jit)
            md = hm.get_metrics_dict(out, hb)
            ld = hm.get_loss_dict(out, hb)
            sum(ld.values()).backward()
        torch.cuda.synchronize()
        results.append(({k: float(v.detach()) for k, v in ld.items()}, {k: float(v) for k, v in md.items()},
                        hm.arena().grads.clone()))
        slices = {g: hm.arena().group_slice(g) for g in ("proposal_networks", "fields")}
    return results, slices


@pytest.mark.parametrize("color,scaling,semgrad", FUSED_CONFIGS)
def test_fused_step_gradients_are_the_autograd_step_s(dev, color, scaling, semgrad):
    """Every gradient of the arena — the field's, which the compositing backward with its options feeds, and the proposal
    networks' — is bit for bit the same after fused_forward_backward and after loss.backward(); and the options are wired:
    the field's gradients differ from the default configuration's by more than 1 % of their maximum.
    [measured on an MI355X: 0 of 164232 + 1065656 entries differ in each of the four configurations]"""
    ((_, _, g_a), (_, _, g_f), (_, _, g_off)), slices = _fused_and_autograd(dev, color, scaling, semgrad)
    for name, sl in slices.items():
        a, f = g_a[sl], g_f[sl]
        print(f"[composite background fused {color} scale={scaling} sem={semgrad}] {name}: max |autograd - fused| = "
              f"{(a - f).abs().max().item():.3e} of {a.abs().max().item():.3e}, {int((a != f).sum())} of {a.numel()} differ")
    for name, sl in slices.items():
        assert float(g_a[sl].abs().max()) > 0, name
        assert torch.equal(g_a[sl], g_f[sl]), f"{name}: {int((g_a[sl] != g_f[sl]).sum())} gradient entries differ"
    sl = slices["fields"]
    assert (g_a[sl] - g_off[sl]).abs().max().item() > 1e-2 * g_a[sl].abs().max().item()


@pytest.mark.parametrize("color,scaling,semgrad", FUSED_CONFIGS)
def test_fused_step_losses_and_metrics_match_the_autograd_step_s(dev, color, scaling, semgrad):
    """The loss and metric VALUES of the two paths at the 1e-6 relative of tests/test_gpu_training_parity.py::
    test_fused_step_matches_the_autograd_step: they are the same per-ray terms summed by different launches (loss.backward():
    fnr_losses_fwd, fnr_interlevel_fwd, fnr_distortion, float sums; the fused step: fnr_train_losses, fixed-point sums —
    tests/test_gpu_training_parity.py holds those launches to each other at 1e-6 too), with and without the options.
    [measured on an MI355X: interlevel_loss up to 1.8e-7, rgb_loss up to 9.2e-8 relative, the others equal]"""
    ((ld_a, md_a, _), (ld_f, md_f, _), _), _ = _fused_and_autograd(dev, color, scaling, semgrad)
    pairs = {k: (ld_a[k], ld_f[k]) for k in ld_a}
    pairs.update({k: (md_a[k], md_f[k]) for k in md_a})
    for k, (a, f) in pairs.items():
        print(f"[composite background fused {color} scale={scaling} sem={semgrad}] {k}: autograd {a!r} fused {f!r} "
              f"rel {abs(a - f) / max(abs(a), 1e-30):.2e}")
    assert set(pairs) == {"rgb_loss", "semantics_loss", "interlevel_loss", "psnr", "distortion"}
    for k, (a, f) in pairs.items():
        assert abs(a - f) <= 1e-6 * max(abs(a), 1e-6), k


NEW_RECORDABLE = {"fnr_composite_fwd_opt", "fnr_composite_bwd_targets_opt", "fnr_composite_fwd_bwd_targets_opt"}


@pytest.mark.parametrize("color,scaling", [("white", True), ("random", False)])
def test_training_steps_record_replay_and_reproduce(dev, color, scaling):
    """The training loop under white + scaling and under random: steps record (fnr_program_end succeeds) and the programs
    hold the `_opt` entry points — and, for random, the generator — by name and none of the compositing calls without
    options; replayed training is the interpreted training bit for bit over 18 steps; the same run twice gives identical
    parameter bits.  For random the background of a step is the generator's for the batcher's seed and that step's offset."""
    from fruitnerf_amd import _lib as L
    from tests.test_gpu_sequencer import _interpreted, _loop

    def run(steps=18):
        loop, hm, opt, batcher, cam = _loop(dev, n_rays=160)
        hm.config.background_color, hm.config.use_gradient_scaling = color, scaling
        losses = []
        for i in range(steps):
            ld, md = loop.step(want_metrics=(i % 3 != 0))
            losses.append(torch.stack(list(ld.values())).clone())
        torch.cuda.synchronize()
        lib = L.load()
        names = set()
        for prog in loop._programs.values():
            names |= {lib.fnr_program_op_name(prog.handle, i).decode() for i in range(lib.fnr_program_size(prog.handle))}
        background = (batcher.last_presample or {}).get("background")
        if color == "random":
            assert torch.equal(background.cpu(), ref.random_background(batcher.gen.initial_seed(), batcher._offset, 160))
        else:
            assert background is None
        return hm.arena().params.clone(), opt.exp_avg.clone(), torch.stack(losses), dict(loop.stats), names
    p1, m1, l1, stats, names = run()
    p2, m2, l2, _, _ = run()
    p_i, m_i, l_i, stats_i, _ = _interpreted(run)
    print(f"[composite background sequencer {color}] stats", stats, sorted(n for n in names if "composite" in n or "random" in n))
    assert stats["record_failed"] == 0 and stats["recorded"] >= 2 and stats["replayed"] >= 4, stats
    assert stats_i["replayed"] == 0
    assert names & NEW_RECORDABLE
    assert "fnr_composite_bwd_targets_opt" in names or "fnr_composite_fwd_bwd_targets_opt" in names
    assert ("fnr_random_background" in names) is (color == "random")
    assert not names & {"fnr_composite_bwd_targets", "fnr_composite_fwd_bwd_targets", "fnr_composite_bwd_targets_semgrad",
                        "fnr_composite_fwd_bwd_targets_semgrad"}
    assert "fnr_composite_fwd" not in names
    assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(l1, l2), "two runs differ"
    assert torch.equal(p1, p_i) and torch.equal(m1, m_i) and torch.equal(l1, l_i), "replayed and interpreted steps differ"


# What a default-configuration step of the loop of tests/test_gpu_sequencer._loop (camera optimiser, two streams, look-ahead)
# asks of the C ABI, by entry-point name, interpreted — recorded on the commit before background colours and gradient scaling
# existed.  A: a step that trains the proposal networks; B: one that does not (the compositing launch runs its own backward).
_AHEAD = ["fnr_train_prologue", "fnr_prop_density_fwd", "fnr_weights_pdf", "fnr_prop_density_fwd", "fnr_weights_pdf"]
_FORWARD = ["fnr_hash_encode_fwd", "fnr_field_mlp_fwd"]
PARENT_CALLS = {
    "A": _FORWARD + ["fnr_composite_fwd", "fnr_stream_wait_stream", "fnr_train_losses", "fnr_prop_density_bwd_pair_split",
                     "fnr_composite_bwd_targets", "fnr_field_mlp_bwd_adam", "fnr_stream_wait_event",
                     "fnr_position_grad_reduce_multi", "fnr_camera_pose_grad_adam", "fnr_event_record",
                     "fnr_hash_encode_bwd_adam", "fnr_stream_wait_event"] + _AHEAD + ["fnr_stream_wait_stream"],
    "B": _FORWARD + ["fnr_composite_fwd_bwd_targets", "fnr_stream_wait_stream", "fnr_train_losses", "fnr_field_mlp_bwd_adam",
                     "fnr_event_record", "fnr_hash_encode_bwd_adam", "fnr_stream_wait_event",
                     "fnr_position_grad_reduce_multi", "fnr_camera_pose_grad_adam"] + _AHEAD + ["fnr_stream_wait_stream"],
}
PARENT_CALLS["first"] = _AHEAD + PARENT_CALLS["A"]      # step 0 samples its own rays: nothing was sampled ahead for it


def _default_step_calls(dev, steps):
    """-> per step: (trained the proposal networks?, metrics?, [entry points called])."""
    from fruitnerf_amd import _lib as L
    from tests.test_gpu_sequencer import _interpreted, _loop
    from fruitnerf_amd.training import _PROGRAM_QUERIES

    def run():
        loop, hm, opt, batcher, cam = _loop(dev, n_rays=160)
        assert hm.config.background_color == "last_sample" and not hm.config.use_gradient_scaling
        out = []
        for i in range(steps):
            log = L.begin_call_log()
            try:
                loop.step(want_metrics=(i % 3 != 0))
            finally:
                names = L.end_call_log(log)
            out.append((bool(hm._last_render_updated), i % 3 != 0, [n for n in names if n not in _PROGRAM_QUERIES]))
        torch.cuda.synchronize()
        return out
    return _interpreted(run)


def test_default_configuration_makes_the_calls_it_made(dev):
    """A model with the default configuration makes exactly the entry-point calls, by name and in order, that it made on the
    parent commit (PARENT_CALLS: from a run of that commit) — none of the `_opt` calls, no generator."""
    steps = _default_step_calls(dev, 14)
    kinds = set()
    for i, (updated, metrics, names) in enumerate(steps):
        kind = ("first" if i == 0 else "A" if updated else "B")
        kinds.add(kind)
        assert names == PARENT_CALLS[kind], f"step {i} ({kind}): {names}"
        assert not any(n.endswith("_opt") or n == "fnr_random_background" for n in names)
    assert kinds == {"first", "A", "B"}


# The same for a model driven the way a Nerfstudio Trainer drives it — model(ray_bundle), get_metrics_dict, get_loss_dict,
# loss.backward() — in training mode, and the first three in eval mode; from a run of the same parent commit.
_SAMPLING = ["fnr_sample_spaced", "fnr_prop_density_fwd", "fnr_weights_pdf", "fnr_prop_density_fwd", "fnr_weights_pdf"]
PARENT_AUTOGRAD_CALLS = {
    "train": _SAMPLING + ["fnr_hash_encode_fwd", "fnr_field_mlp_fwd", "fnr_composite_fwd", "fnr_losses_fwd", "fnr_distortion",
                          "fnr_interlevel_fwd", "fnr_interlevel_fwd", "fnr_weights_bwd", "fnr_prop_density_bwd",
                          "fnr_weights_bwd", "fnr_prop_density_bwd", "fnr_composite_bwd", "fnr_field_mlp_bwd",
                          "fnr_hash_encode_bwd"],
    "eval": _SAMPLING + ["fnr_hash_encode_fwd", "fnr_embedding_mean", "fnr_field_mlp_fwd", "fnr_composite_fwd",
                         "fnr_losses_fwd", "fnr_distortion"],
}


def test_default_configuration_makes_the_autograd_path_s_calls(dev):
    """model(...) -> get_metrics_dict -> get_loss_dict -> loss.backward() of a default-configuration model: the entry points
    of the parent commit, by name and in order, on the first step and on the second, in training and in eval mode."""
    from fruitnerf_amd import _lib as L
    from fruitnerf_amd.rays import RayBundle
    from fruitnerf_amd.training import _PROGRAM_QUERIES
    from tests.test_gpu_training_parity import _batch as _image_batch
    hm = util.make_hip_like(util.make_oracle(util.small_config(log2=15, prop_log2=13), seed=9), dev)
    assert hm.config.background_color == "last_sample" and not hm.config.use_gradient_scaling
    R = 160
    o, d, pa, cam = util.random_rays(R, 7, seed=4)
    hb = {k: v.to(dev) for k, v in _image_batch(R, 8).items()}
    hm.arena()
    for mode in ("train", "train", "eval"):
        hm.train(mode == "train")
        hm.set_anneal(0)
        log = L.begin_call_log()
        try:
            out = hm(RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev)))
            hm.get_metrics_dict(out, hb)
            ld = hm.get_loss_dict(out, hb)
            if mode == "train":
                sum(ld.values()).backward()
            torch.cuda.synchronize()
        finally:
            names = [n for n in L.end_call_log(log) if n not in _PROGRAM_QUERIES]
        assert names == PARENT_AUTOGRAD_CALLS[mode], f"{mode}: {names}"


def test_forward_outputs_depend_on_the_background_alone(dev):
    """Train, eval, inference and export mode of FruitModel, the three configurations against each other (that the default
    configuration's outputs are what they were is held by the suites named below, against the oracle and stored vectors).  Gradient scaling is backward-only: every output tensor is
    bit-identical with it on and off.  A white background changes "rgb" alone (export mode composites nothing).
    (tests/test_gpu_forward_parity.py and tests/test_golden.py hold the default configuration's outputs to the oracle.)"""
    from fruitnerf_amd.data.fruit_datamanager import ExportDataManager
    from fruitnerf_amd.rays import RayBundle
    cfg = util.small_config(log2=14)
    R = 96
    o, d, pa, cam = util.random_rays(R, 7, seed=6)
    jit = [torch.rand(R, 1).to(dev) for _ in range(3)]
    aabb = ((-1.0, -0.6, -1.0), (1.0, 0.6, 1.0))

    def outputs(color, scaling):
        res = {}
        mk = lambda mode=None: _hip_model(util.make_oracle(cfg, seed=2, test_mode=mode), dev, color, scaling,  # noqa: E731
                                          test_mode=mode)
        hm = mk()
        rb = lambda: RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev))  # noqa: E731
        hm.train()
        hm.set_anneal(0)
        res["train"] = hm(rb(), jitter=jit)
        hm.eval()
        res["eval"] = hm(rb())
        hi = mk("inference")
        hi.eval()
        res["inference"] = hi(rb())
        he = mk("export")
        he.eval()
        he.setup_inference(True, 16, deterministic=True)
        dm = ExportDataManager(dev, eval_num_rays_per_batch=97)
        dm.setup_inference(aabb=aabb, num_points=16)
        res["export"] = he(dm.next_sample_volume(0)[0])
        torch.cuda.synchronize()
        return res
    default, scaled, white = outputs("last_sample", False), outputs("last_sample", True), outputs("white", False)
    for mode in default:
        compared = 0
        for k, v in default[mode].items():
            if not torch.is_tensor(v):
                continue
            assert torch.equal(v.detach(), scaled[mode][k].detach()), f"{mode}: {k} depends on gradient scaling"
            if k == "rgb" and mode != "export":
                assert not torch.equal(v.detach(), white[mode][k].detach()), f"{mode}: white background not wired"
            else:
                assert torch.equal(v.detach(), white[mode][k].detach()), f"{mode}: {k} depends on the background"
            compared += 1
        assert compared >= 3, mode
