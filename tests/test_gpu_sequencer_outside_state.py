"""The native step sequencer against state that changes from OUTSIDE between two steps.  A recorded program holds the
arguments of every entry point by value — the optimiser's moment and bitmap addresses, its hyper-parameters, the camera
optimiser's pose table and moments, the batcher's image set.  Whatever of that changes must select another program (or send
the step to the interpreter); a replay into the old values trains wrongly without an error.  Every scenario here runs the
same loop natively and interpreted, changes one thing after N_BEFORE steps, and requires every state to be bit-identical
after N_AFTER more — while steps were being replayed before the change and are being replayed again after it."""
import gc

import pytest
import torch

from tests.test_gpu_sequencer import _host_state, _interpreted, _loop

pytestmark = pytest.mark.gpu

N_BEFORE = N_AFTER = 24
N_TRAIN = 40            # cameras of _loop's dataset
_SHARED = {}


def _main_table_span(hm):
    table = hm.field.mlp_base_grid.hash_table
    return [(off, off + n) for _, p, off, n in hm.arena().entries if p is table][0]


def _second_dataset(dev):
    """Another scene through the cameras and shapes of _loop's dataset; rendered once, never written to."""
    if "data" not in _SHARED:
        from fruitnerf_amd.data import synthetic_apple as sa
        HW, focal = 96, 1111.0 * 96 / 800
        _SHARED["data"] = sa.render_dataset(sa.make_scene(seed=1, device=dev), sa.make_cameras(N_TRAIN, seed=0, device=dev),
                                            H=HW, W=HW, fx=focal, fy=focal)
    return _SHARED["data"]


# ---- the changes: each gets the loop (whose .optimizer / .camera / .batcher are the CURRENT objects), the model, the device
def _load_moments_in_place(loop, hm, dev):
    opt = loop.optimizer
    a, b = _main_table_span(hm)
    if opt._touched:       # (the dense-sweep run of this scenario keeps no bitmap)
        bm = opt._touched[a][1]
        clear = 1.0 - float(((bm.to(torch.int64)[:, None] >> torch.arange(32, device=dev)) & 1).float().mean())
        print(f"[outside state] row pairs of the main table with a clear bit before the load: {clear:.3f}")
        assert clear >= 0.10, "precondition: the loaded moments must reach rows the stale bitmap would skip"
    M, V = opt.exp_avg + 1e-8, opt.exp_avg_sq + 1e-16
    assert bool((M[a:b].view(-1, 4) != 0).any(dim=1).all()) and bool((V[a:b].view(-1, 4) != 0).any(dim=1).all())
    opt.exp_avg.copy_(M)
    opt.exp_avg_sq.copy_(V)
    opt.rebuild_touched()


def _zero_moments_in_place(loop, hm, dev):
    opt = loop.optimizer
    opt.exp_avg.zero_()
    opt.exp_avg_sq.zero_()
    opt.rebuild_touched()


def _reassign_moments(loop, hm, dev):
    opt = loop.optimizer
    opt.exp_avg = opt.exp_avg.clone()
    opt.exp_avg_sq = opt.exp_avg_sq.clone()
    opt.rebuild_touched()


def _set_optimizer(name, value):
    def change(loop, hm, dev):
        assert getattr(loop.optimizer, name) != value
        setattr(loop.optimizer, name, value)
    return change


def _replace_optimizer(loop, hm, dev):
    import fruitnerf_amd.training as T
    loop.optimizer = None          # nothing here holds the old one: its id() is free to be reused
    gc.collect()
    loop.optimizer = T.FusedAdam(hm)


def _replace_camera_optimizer(loop, hm, dev):
    from fruitnerf_amd.cameras.camera_optimizers import CameraAdam, CameraOptimizerConfig
    new_opt = CameraOptimizerConfig(mode="SO3xR3").setup(N_TRAIN, dev)
    loop.camera = (new_opt, CameraAdam(new_opt), loop.batcher)


def _camera_adam_betas(loop, hm, dev):
    loop.camera[1].betas = (0.8, 0.99)


def _camera_adam_reassign_moments(loop, hm, dev):
    adam = loop.camera[1]
    adam.exp_avg = adam.exp_avg.clone()
    adam.exp_avg_sq = adam.exp_avg_sq.clone()


def _replace_batcher(loop, hm, dev):
    from fruitnerf_amd.data import synthetic_apple as sa
    _SHARED.setdefault("old batchers", []).append(loop.batcher)    # (its images stay allocated: no address is handed out twice)
    loop.batcher = sa.PixelBatcher(_second_dataset(dev), torch.arange(N_TRAIN, device=dev), seed=2)
    loop.camera = (loop.camera[0], loop.camera[1], loop.batcher)
    loop.drop_lookahead()


def _unfused_step_in_between(loop, hm, dev):
    a, b = _main_table_span(hm)
    loop.optimizer.step_span(a, b, 1e-2)       # zero gradient behind the fused step's zero_grad: the moments decay, the
    # parameters move along them — and the span's bitmap is dropped (the exchange fallback and scaler_step go this way)


SCENARIOS = {
    "moments_loaded_in_place_then_rebuild_touched": _load_moments_in_place,
    "moments_zeroed_in_place_then_rebuild_touched": _zero_moments_in_place,
    "moments_reassigned": _reassign_moments,
    "optimizer_betas_changed": _set_optimizer("betas", (0.8, 0.99)),
    "optimizer_eps_changed": _set_optimizer("eps", 1e-8),
    "optimizer_weight_decay_switched_on": _set_optimizer("weight_decay", 1e-4),
    "optimizer_skip_groups_without_grad_flipped": _set_optimizer("skip_groups_without_grad", False),
    "optimizer_replaced": _replace_optimizer,
    "camera_optimizer_replaced": _replace_camera_optimizer,
    "camera_adam_betas_changed": _camera_adam_betas,
    "camera_adam_moments_reassigned": _camera_adam_reassign_moments,
    "batcher_replaced": _replace_batcher,
    "out_of_band_unfused_step": _unfused_step_in_between,
}


def _run(dev, scenario):
    """N_BEFORE steps, the change, N_AFTER steps -> ([(name, tensor)], host counters, stats at the change, stats at the end)."""
    loop, hm, _, _, _ = _loop(dev)        # (no local keeps the optimiser, the camera optimiser or the batcher)
    assert loop.optimizer.eps == 1e-15 and loop.optimizer.weight_decay == 0.0 and loop.optimizer.skip_groups_without_grad
    losses = []

    def steps(n):
        for _ in range(n):
            loss_dict, _ = loop.step()
            losses.append(torch.stack(list(loss_dict.values())).clone())
    steps(N_BEFORE)
    at_change = dict(loop.stats)
    with torch.no_grad():
        SCENARIOS[scenario](loop, hm, dev)
    steps(N_AFTER)
    torch.cuda.synchronize()
    opt, (cam_opt, cam_adam, batcher) = loop.optimizer, loop.camera
    assert batcher is loop.batcher
    tensors = [("parameters", hm.arena().params.clone()), ("exp_avg", opt.exp_avg.clone()),
               ("exp_avg_sq", opt.exp_avg_sq.clone()), ("pose_adjustment", cam_opt.pose_adjustment.data.clone()),
               ("camera exp_avg", cam_adam.exp_avg.clone()), ("camera exp_avg_sq", cam_adam.exp_avg_sq.clone()),
               ("losses", torch.stack(losses))]
    return tensors, _host_state(loop, hm, opt, batcher, (cam_opt, cam_adam)), at_change, dict(loop.stats)


def _same(scenario, what, got, ref):
    for (name, x), (_, y) in zip(got[0], ref[0]):
        if not torch.equal(x, y):
            n = int((x != y).sum()) if x.shape == y.shape else -1
            first = ""
            if name == "losses" and x.shape == y.shape:
                first = f"; first step that differs: {int((x != y).any(dim=1).nonzero()[0])}"
            pytest.fail(f"{scenario}: {name} differ between {what} ({n} of {x.numel()} entries{first})")
    assert got[1] == ref[1], f"{scenario}: host counters differ between {what}: {got[1]} != {ref[1]}"


@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_replays_after_an_outside_change_are_the_interpreted_steps(dev, scenario):
    """Bit-identity with the interpreter (the reference; no tolerance) across one change from outside, with at least 8 steps
    replayed before the change and at least 8 more after it, and no recording that failed."""
    import fruitnerf_amd.training as T
    assert T.NATIVE_SEQUENCER and T.SPARSE_TOUCH_SKIPPING, "the defaults are under test"
    native = _run(dev, scenario)
    ref = _interpreted(lambda: _run(dev, scenario))
    before, after = native[2], native[3]
    print(f"[outside state] {scenario}: replayed {before['replayed']} of {N_BEFORE} steps before the change, "
          f"{after['replayed'] - before['replayed']} of {N_AFTER} after it; stats at the end {after}")
    assert ref[3]["replayed"] == 0 and ref[3]["recorded"] == 0
    _same(scenario, "replayed and interpreted steps", native, ref)
    if scenario == "moments_loaded_in_place_then_rebuild_touched":
        # the dense sweep is the definition of Adam: the same scenario with every table row swept on every step
        saved, T.SPARSE_TOUCH_SKIPPING = T.SPARSE_TOUCH_SKIPPING, False
        try:
            dense = _interpreted(lambda: _run(dev, scenario))
        finally:
            T.SPARSE_TOUCH_SKIPPING = saved
        _same(scenario, "the interpreted steps and the interpreted dense sweep", ref, dense)
        _same(scenario, "the replayed steps and the interpreted dense sweep", native, dense)
    if scenario == "camera_optimizer_replaced":
        assert bool((native[0][3][1] != 0).any()), "the new camera optimiser was never trained"
    assert before["replayed"] >= 8, f"{scenario}: programs were not in use at the change: {before}"
    assert after["replayed"] - before["replayed"] >= 8, f"{scenario}: steps are no longer replayed after the change: {after}"
    assert after["record_failed"] == 0, f"{scenario}: {after}"
