"""use_single_jitter=False on the device: one stratified jitter per bin edge, drawn inside the kernels that consume it.

  1. fnr_edge_jitter against the numpy restatement of the counter layout (tests/edge_jitter_reference.py), bit for bit.
  2. fnr_train_prologue_edges: level 0 is fnr_sample_spaced(per bin) on fnr_edge_jitter(level 0), everything else is
     fnr_train_prologue_mode's on the same seed and offset, bit for bit.
  3. fnr_weights_pdf_edges: drawing in the kernel = the pointer form fed fnr_edge_jitter; the pointer form fed constant rows =
     fnr_weights_pdf(rand [R]); the evaluation form = fnr_weights_pdf's.
  4. fnr_weights_pdf_edges per stage against float64 ns.PDFSampler(single_jitter=False), at the bounds of
     tests/test_gpu_ray_kernels.py::test_weights_pdf_every_stage.
  5. The model against the oracle with the switch off (losses, metrics, every parameter gradient), and the eval pass.
  6. The training loop: records, replays, reproduces, also when the attribute flips between steps; fused = autograd
     gradients; the default loop's programs name the entry points they always named."""
import copy

import numpy as np
import pytest
import torch

from oracle import ns_torch as ns
from tests import edge_jitter_reference as ej
from tests import util
from tests.test_gpu_ray_kernels import (U, _batch, _check_median, _inverse_cdf_slope, _rays, _samples64, _spacing_fns,
                                        _weight_arith, _worst)

pytestmark = pytest.mark.gpu

F8 = torch.float64
SEED, OFFSET = (0xC0FFEE12 << 32) | 0x89ABCDEF, (7 << 32) + 5      # a seed with its high word set, an offset above 2^32
S_NEW = (1, 48, 96, 512)                                          # nb = 2, 49, 97, 513: partial quads, the tail beyond 128


def _K():
    from fruitnerf_amd import _kernels as K
    return K


# ---- 1. the generator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,n_edges,level", [(1, 2, 0), (257, 49, 2), (300, 513, 4)])
def test_edge_jitter_is_the_stated_philox_words(dev, R, n_edges, level):
    K = _K()
    got = K.edge_jitter(SEED, OFFSET, level, R, n_edges, dev).cpu().numpy()
    assert np.array_equal(got, ej.edge_jitter(SEED, OFFSET, level, R, n_edges))


# ---- 2. the prologue -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    from tests.test_gpu_composite_background import _image_set
    K = _K()
    sa, data, n_train = _image_set(dev)
    iset = K.ImageSetArg(data["images"], data["masks"], data["c2w"], data["fx"], data["fy"], data["cx"], data["cy"])
    g = torch.Generator().manual_seed(11)
    f = float(data["fx"])
    intr = torch.tensor([[f, f, 12.0, 12.0]]).repeat(n_train, 1) * (1 + 0.05 * torch.rand(n_train, 4, generator=g))
    dist = torch.randn(n_train, 6, generator=g) * torch.tensor([0.05, 0.02, 0.005, 0.001, 0.003, 0.003])
    pose = torch.cat([torch.randn(n_train, 3, generator=g) * 0.02, torch.randn(n_train, 3, generator=g) * 0.03], 1)
    pose[0, 3:] = 0.0
    return {"iset": iset, "ids": torch.arange(n_train, device=dev), "n_train": n_train,
            "cams": K.CameraTableArg(intr.to(dev), dist.to(dev)), "pose": pose.to(dev)}


@pytest.mark.parametrize("cams,pose_mode", [(False, None), (True, None), (False, "SO3xR3"), (True, "SE3"), (False, "SE3")])
def test_prologue_edges_is_the_separate_launches(dev, scene, cams, pose_mode):
    """[every comparison exact on an MI355X]"""
    from fruitnerf_amd import _lib as L
    K = _K()
    table = scene["cams"] if cams else None
    pose = scene["pose"] if pose_mode is not None else None
    mode = L.POSE_MODES[pose_mode] if pose_mode is not None else L.FNR_POSE_SO3XR3
    near, far = 0.05, 1000.0
    for S0 in (1, 3, 256):
        for R in (5, 300):
            kw = dict(pose_adjustment=pose, near=near, far=far, S0=S0, cams=table, pose_mode=mode)
            got = K.train_prologue(scene["iset"], scene["ids"], R, SEED, OFFSET, per_edge=True, **kw)
            ref = K.train_prologue(scene["iset"], scene["ids"], R, SEED, OFFSET, **kw)
            assert got["jitter"] is None
            for k in ("u", "origins", "directions", "cam", "image", "mask"):
                assert torch.equal(got[k], ref[k]), (k, S0, R)
            if pose is not None:
                assert torch.equal(got["c2w_adjusted"], ref["c2w_adjusted"])
                assert torch.equal(got["c2w_adjusted"], K.camera_adjust(scene["iset"], scene["ids"], pose, pose_mode=mode))
            jit0 = K.edge_jitter(SEED, OFFSET, 0, R, S0 + 1, dev)
            assert np.array_equal(jit0.cpu().numpy(), ej.edge_jitter(SEED, OFFSET, 0, R, S0 + 1))
            rays = K.RaysArg(got["origins"], got["directions"], torch.full((R, 1), near, device=dev),
                             torch.full((R, 1), far, device=dev), got["cam"])
            spacing, euclid = K.sample_spaced(rays, 1, S0, jit0)
            assert torch.equal(got["spacing"], spacing) and torch.equal(got["euclid"], euclid), (S0, R)
            assert not torch.equal(got["spacing"], ref["spacing"])           # (one number per ray gives other bins)
            for bins in (got["spacing"], got["euclid"]):
                assert bool((bins[:, 1:] >= bins[:, :-1]).all()), "a row of bins decreases"


# ---- 3. the PDF stage, bit ties --------------------------------------------------------------------------------------------
def _pdf_inputs(S_prev, dev, seed=3):
    edges, dens, _, _ = _batch(S_prev, seed=seed)
    R = edges.shape[0]
    g = torch.Generator().manual_seed(1000 + S_prev)
    sp = torch.sort(torch.rand(R, S_prev + 1, generator=g), 1).values
    sp[:, 0], sp[:, -1] = 0.0, 1.0
    return R, edges, dens, sp.contiguous(), g


@pytest.mark.parametrize("S_prev", [64, 96, 256, 321])       # one per kernel width (1, 2, 4, 8 samples per lane)
def test_pdf_edges_bit_ties(dev, S_prev):
    """(a) draw = the pointer form on fnr_edge_jitter(level); (b) constant rows = fnr_weights_pdf(rand [R]); (c) the evaluation
    form = fnr_weights_pdf's.  Weights, median depth and both bin arrays, bit for bit.  [exact on an MI355X]"""
    K = _K()
    R, edges, dens, sp, g = _pdf_inputs(S_prev, dev)
    rays = _rays(R, dev, 0.05, 1000.0)
    args = (dens.to(dev), sp.to(dev), edges.to(dev))
    names = ("weights", "median depth", "spacing", "euclid")
    for S_new in S_NEW:
        nb = S_new + 1
        for kind, anneal in ((1, 0.37), (0, 1.0)):
            for level in (1, 2):
                table = K.edge_jitter(SEED, OFFSET, level, R, nb, dev)
                drawn = K.weights_pdf(rays, kind, S_prev, S_new, *args, anneal, None, per_edge=True, draw=(SEED, OFFSET, level))
                fed = K.weights_pdf(rays, kind, S_prev, S_new, *args, anneal, table, per_edge=True)
                for n, a, b in zip(names, drawn, fed):
                    assert torch.equal(a, b), ("draw", n, S_new, kind, level)
            other = K.weights_pdf(rays, kind, S_prev, S_new, *args, anneal, None, per_edge=True, draw=(SEED, OFFSET + 1, 1))
            assert not torch.equal(other[2], fed[2]), "another offset draws the same numbers"
            rand = torch.rand(R, generator=g).to(dev)
            per_ray = K.weights_pdf(rays, kind, S_prev, S_new, *args, anneal, rand)
            rows = K.weights_pdf(rays, kind, S_prev, S_new, *args, anneal, rand[:, None].expand(R, nb).contiguous(), per_edge=True)
            for n, a, b in zip(names, rows, per_ray):
                assert torch.equal(a, b), ("constant rows", n, S_new, kind)
            ev = K.weights_pdf(rays, kind, S_prev, S_new, *args, anneal, None)
            ev_e = K.weights_pdf(rays, kind, S_prev, S_new, *args, anneal, None, per_edge=True)
            for n, a, b in zip(names, ev_e, ev):
                assert torch.equal(a, b), ("eval", n, S_new, kind)


# ---- 4. the PDF stage, float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_prev", [1, 48, 96, 256, 321, 512])
def test_pdf_edges_every_stage(dev, S_prev):
    """tests/test_gpu_ray_kernels.py::test_weights_pdf_every_stage with one jitter per new bin edge: rand [R, S_new + 1] is fed
    to the kernel (fnr_weights_pdf_edges) and, in float64, to ns.PDFSampler(single_jitter=False).  Same batch (`_batch`), both
    spacing kinds, anneal 0 / 0.37 / 1, S_new 1 / 48 / 96 / 512, and the same three bounds: the per-edge u is u_base[j] +
    rand[r, j] / nb, the two float32 operations of the single-jitter u, so the derivations there carry over unchanged.
    [measured on an MI355X: w 0.15, spacing 0.28, euclid 0.34]"""
    K = _K()
    worst = {}
    near, far = 0.05, 1000.0
    edges, dens, _, _ = _batch(S_prev, seed=3)
    R = edges.shape[0]
    w64 = _samples64(edges).get_weights(dens.double()[..., None])[..., 0]
    A = _weight_arith(edges, dens)
    E = (S_prev + 63) // 64
    g = torch.Generator().manual_seed(S_prev)
    for kind in (0, 1):
        fn, inv = _spacing_fns(kind)
        lo, hi = (float(fn(torch.tensor(v, dtype=torch.float32).double())) for v in (near, far))
        sp = torch.sort(torch.rand(R, S_prev + 1, generator=g), 1).values
        sp[:, 0], sp[:, -1] = 0.0, 1.0
        spacing_prev = sp.contiguous()

        def to_euclid(x):
            return inv(x * hi + (1 - x) * lo)
        rs_prev = ns.RaySamples(frustums=None, spacing_starts=spacing_prev.double()[:, :-1, None],
                                spacing_ends=spacing_prev.double()[:, 1:, None], spacing_to_euclidean_fn=to_euclid)
        rb = ns.RayBundle(torch.zeros(R, 3, dtype=F8), torch.zeros(R, 3, dtype=F8), torch.ones(R, 1, dtype=F8))
        for anneal in (0.0, 0.37, 1.0):
            for S_new in S_NEW:
                rand = torch.rand(R, S_new + 1, generator=g)
                w, depth, sp_new, eu_new = K.weights_pdf(_rays(R, dev, near, far), kind, S_prev, S_new, dens.to(dev),
                                                         spacing_prev.to(dev), edges.to(dev), anneal, rand.to(dev),
                                                         per_edge=True)
                w, depth, sp_new, eu_new = (t.cpu() for t in (w, depth, sp_new, eu_new))
                wmax = w64.max(1, keepdim=True).values
                worst.setdefault("w", []).append(((w.double() - w64).abs() / (2e-6 * wmax + A + 1e-300)).max())
                _check_median(f"weights_pdf_edges S_prev={S_prev}", depth, edges, w64)
                smp = ns.PDFSampler(num_samples=S_new, include_original=False, single_jitter=False)
                smp.train(True)
                wa = torch.pow(w.double(), anneal)      # the resampling stage on the kernel's own weights
                out = smp(rb, rs_prev, wa[..., None], rand=rand.double())
                ref_sp = torch.cat([out.spacing_starts[..., 0], out.spacing_ends[..., -1:, 0]], -1)
                b = 2e-6 + _inverse_cdf_slope(spacing_prev, wa, ref_sp) * (E + 8) * U
                worst.setdefault("spacing", []).append(((sp_new.double() - ref_sp).abs() / b).max())
                e_ref = to_euclid(sp_new.double())
                b = 2e-6 * e_ref.abs() + (2.0 ** -21 * e_ref ** 2 if kind == 1 else 0.0)
                worst.setdefault("euclid", []).append(((eu_new.double() - e_ref).abs() / b).max())
                assert torch.isfinite(sp_new).all()
    for k, v in worst.items():
        assert _worst(f"weights_pdf_edges[{S_prev}].{k}", torch.stack(v)) <= 1.0, k


# ---- 5. the model against the oracle ---------------------------------------------------------------------------------------
def _edge_jitters(R, counts=(256, 96, 48), seed=77):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(R, S + 1, generator=g) for S in counts]


@pytest.mark.parametrize("step", [0, 12])
def test_losses_and_all_gradients_with_per_edge_jitter(dev, step):
    """tests/test_gpu_training_parity.py::test_losses_and_all_gradients (its fruit_nerf bars) with use_single_jitter=False and
    jitter [R,257], [R,97], [R,49] given to both sides; then the eval pass, which draws nothing: bit-equal to the same model
    with the attribute on; and a `jitter=` list of the other form is a ValueError."""
    from fruitnerf_amd.rays import RayBundle
    from tests.test_gpu_training_parity import _batch as _image_batch, _grad_report, _oracle_step
    cfg = util.small_config(log2=15, prop_log2=13)
    cfg.use_single_jitter = False
    cfg.proposal_weights_anneal_max_num_iters, cfg.max_res = 1000, 2048
    om = util.make_oracle(cfg, seed=5)
    hm = util.make_hip_like(om, dev)
    assert hm.proposal_sampler.single_jitter is False
    om.train()
    hm.train()
    for m in (om, hm):
        m.proposal_sampler._step = step
        m.proposal_sampler._steps_since_update = 0
    R = 160
    o, d, pa, cam = util.random_rays(R, 7, seed=21)
    jit = _edge_jitters(R)
    batch = _image_batch(R, 3)
    out, ld_ref, md_ref = _oracle_step(om, o, d, pa, cam, jit, batch, step)

    def bundle():
        return RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev))
    hm.set_anneal(step)
    hout = hm(bundle(), jitter=[j.to(dev) for j in jit])
    hb = {k: v.to(dev) for k, v in batch.items()}
    md = hm.get_metrics_dict(hout, hb)
    ld = hm.get_loss_dict(hout, hb)
    sum(ld.values()).backward()
    torch.cuda.synchronize()
    for k in ld_ref:
        a, b = float(ld[k]), float(ld_ref[k])
        print(f"[per-edge jitter loss step={step}] {k}: hip {a:.8e} oracle {b:.8e}")
        assert abs(a - b) <= 2e-5 * max(abs(b), 1e-3), k
    for k in md_ref:
        a, b = float(md[k]), float(md_ref[k])
        print(f"[per-edge jitter metric step={step}] {k}: hip {a:.6e} oracle {b:.6e}")
        assert abs(a - b) <= 1e-4 * max(abs(b), 1e-3), k
    worst = _grad_report(om, hm, f" per-edge step={step}")
    assert worst <= 2e-3, f"worst relative gradient error {worst}"
    # a list of the other form is refused, whichever way the attribute stands
    with pytest.raises(ValueError, match=r"\(160, 257\)"):
        hm(bundle(), jitter=[torch.rand(R, 1, device=dev) for _ in range(3)])
    hm.proposal_sampler.single_jitter = True
    with pytest.raises(ValueError, match=r"\(160, 1\)"):
        hm(bundle(), jitter=[j.to(dev) for j in jit])
    # eval: nothing is drawn, the switch changes nothing
    hm.eval()
    with torch.no_grad():
        on = hm(bundle())
        hm.proposal_sampler.single_jitter = False
        off = hm(bundle())
    torch.cuda.synchronize()
    keys = ("rgb", "accumulation", "depth", "semantics", "prop_depth_0", "prop_depth_1")
    for k in keys:
        assert torch.equal(on[k], off[k]), k


# ---- 6. the training loop --------------------------------------------------------------------------------------------------
SAMPLING_ENTRY_POINTS = {"fnr_train_prologue", "fnr_train_prologue_cams", "fnr_train_prologue_mode", "fnr_train_prologue_edges",
                         "fnr_weights_pdf", "fnr_weights_pdf_edges", "fnr_edge_jitter"}


def _run_loop(dev, single_jitter, steps=18):
    from fruitnerf_amd import _lib as L
    from tests.test_gpu_sequencer import _loop
    K = _K()
    loop, hm, opt, batcher, cam = _loop(dev, n_rays=160)
    hm.proposal_sampler.single_jitter = single_jitter
    losses = []
    for i in range(steps):
        ld, md = loop.step(want_metrics=(i % 3 != 0))
        losses.append(torch.stack(list(ld.values())).clone())
    torch.cuda.synchronize()
    lib = L.load()
    names = set()
    for prog in loop._programs.values():
        names |= {lib.fnr_program_op_name(prog.handle, i).decode() for i in range(lib.fnr_program_size(prog.handle))}
    pre = batcher.last_presample
    if not single_jitter:
        # what was drawn ahead for the next step: level 0 is the spaced sampler on the generator's numbers for this offset
        assert pre["per_edge"] is True and "jitter" not in pre
        assert pre["seed"] == batcher.gen.initial_seed() and pre["offset"] == batcher._offset
        rb = loop._next[1]
        S0 = hm.proposal_sampler.num_proposal_samples_per_ray[0]
        jit0 = K.edge_jitter(pre["seed"], batcher._offset, 0, 160, S0 + 1, dev)
        rays = K.RaysArg(rb.origins, rb.directions, torch.full((160, 1), float(hm.config.near_plane), device=dev),
                         torch.full((160, 1), float(hm.config.far_plane), device=dev), rb.camera_indices)
        spacing, euclid = K.sample_spaced(rays, 1, S0, jit0)
        assert torch.equal(pre["spacing"], spacing) and torch.equal(pre["euclid"], euclid)
    else:
        assert not pre.get("per_edge") and len(pre["jitter"]) == 3
    return hm.arena().params.clone(), opt.exp_avg.clone(), torch.stack(losses), dict(loop.stats), names


def test_training_steps_record_replay_and_reproduce_with_per_edge_jitter(dev):
    """tests/test_gpu_composite_background.py::test_training_steps_record_replay_and_reproduce with the sampler's attribute
    off: 18 steps record and replay, the programs hold the per-edge prologue and PDF entry points and none of the per-ray ones,
    replayed = interpreted and run = run bit for bit; with the attribute on, the loop's programs name the entry points they
    always named."""
    from tests.test_gpu_sequencer import _interpreted
    p1, m1, l1, stats, names = _run_loop(dev, False)
    p2, m2, l2, _, _ = _run_loop(dev, False)
    p_i, m_i, l_i, stats_i, _ = _interpreted(lambda: _run_loop(dev, False))
    print("[per-edge jitter sequencer] stats", stats, sorted(names & SAMPLING_ENTRY_POINTS))
    assert stats["record_failed"] == 0 and stats["recorded"] >= 2 and stats["replayed"] >= 4, stats
    assert stats_i["replayed"] == 0
    assert names & SAMPLING_ENTRY_POINTS == {"fnr_train_prologue_edges", "fnr_weights_pdf_edges"}
    assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(l1, l2), "two runs differ"
    assert torch.equal(p1, p_i) and torch.equal(m1, m_i) and torch.equal(l1, l_i), "replayed and interpreted steps differ"
    p_on, _, l_on, stats_on, names_on = _run_loop(dev, True)
    assert stats_on["record_failed"] == 0 and stats_on["replayed"] >= 4, stats_on
    assert names_on & SAMPLING_ENTRY_POINTS == {"fnr_train_prologue", "fnr_weights_pdf"}
    assert not torch.equal(p_on, p1) and not torch.equal(l_on, l1)           # (the switch is wired: other samples)


def test_flipping_the_attribute_between_steps_replays_no_program_of_the_other_form(dev):
    """30 steps with the attribute off, on (steps 14 - 21) and off again: when it flips, the rays sampled ahead are the other
    form's, and the programs recorded before the first flip exist again after the second.  Replayed = interpreted bit for bit."""
    from tests.test_gpu_sequencer import _interpreted, _loop

    def run():
        loop, hm, opt, batcher, cam = _loop(dev, n_rays=160)
        losses = []
        for i in range(30):
            hm.proposal_sampler.single_jitter = 14 <= i < 22
            ld, md = loop.step(want_metrics=(i % 3 != 0))
            losses.append(torch.stack(list(ld.values())).clone())
        torch.cuda.synchronize()
        return hm.arena().params.clone(), opt.exp_avg.clone(), torch.stack(losses), dict(loop.stats)
    p, m, l, stats = run()
    p_i, m_i, l_i, stats_i = _interpreted(run)
    print("[per-edge jitter flip] stats", stats)
    assert stats["record_failed"] == 0 and stats["replayed"] >= 6 and stats_i["replayed"] == 0, stats
    assert torch.equal(p, p_i) and torch.equal(m, m_i) and torch.equal(l, l_i), "replayed and interpreted steps differ"


def test_fused_step_gradients_are_the_autograd_step_s_with_per_edge_jitter(dev):
    """tests/test_gpu_composite_background.py::test_fused_step_gradients_are_the_autograd_step_s with per-edge jitter tensors:
    every gradient of the arena is bit for bit the same after fused_forward_backward and after loss.backward()."""
    from fruitnerf_amd.rays import RayBundle
    from fruitnerf_amd.training import fused_forward_backward
    from tests.test_gpu_training_parity import _batch as _image_batch
    cfg = util.small_config(log2=15, prop_log2=13)
    cfg.use_single_jitter = False
    om = util.make_oracle(cfg, seed=9)
    R = 160
    o, d, pa, cam = util.random_rays(R, 7, seed=4)
    jit = [j.to(dev) for j in _edge_jitters(R)]
    hb = {k: v.to(dev) for k, v in _image_batch(R, 8).items()}
    grads = []
    for fused in (False, True):
        hm = util.make_hip_like(copy.deepcopy(om), dev)
        hm.train()
        hm.set_anneal(0)
        rb = RayBundle(o.to(dev), d.to(dev), pa.to(dev), cam.to(dev))
        if fused:
            fused_forward_backward(hm, rb, hb, jitter=jit)
        else:
            out = hm(rb, jitter=jit)
            sum(hm.get_loss_dict(out, hb).values()).backward()
        torch.cuda.synchronize()
        grads.append(hm.arena().grads.clone())
        slices = {g: hm.arena().group_slice(g) for g in ("proposal_networks", "fields")}
    for name, sl in slices.items():
        a, f = grads[0][sl], grads[1][sl]
        print(f"[per-edge jitter fused] {name}: {int((a != f).sum())} of {a.numel()} gradient entries differ")
        assert float(a.abs().max()) > 0, name
        assert torch.equal(a, f), name
