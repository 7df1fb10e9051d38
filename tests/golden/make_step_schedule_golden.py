"""The launch schedule of a training step, as the C ABI sees it: for every configuration below, the `fnr_*` entry points
Python calls — by name, in order, and for each stream argument whether it is the launch stream, the model's second
stream or another one.  training.py decides all of that (what is launched, in which order, on which stream), so a change
there that is meant to keep the schedule is held to the lists this module wrote on the commit BEFORE the change:

    python -m tests.golden.make_step_schedule_golden            # writes tests/golden/step_schedule_parent.json

tests/test_gpu_step_schedule.py records the same cases on the checked-out tree and compares, exactly.  The recorder stands
in for the loaded library the way _lib._CallLog does; it lives here, no product file knows about it.  Which arguments of
an entry point are streams is read from include/fruitnerf_hip.h (`void* stream`, and fnr_stream_wait_stream's two).

An entry is "fnr_name" or "fnr_name@launch" / "@side" / "@other" ("@side,launch": one word per stream argument, in
argument order).  A case is stored as its distinct step shapes and the index of every step's shape."""
import contextlib
import faulthandler
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "step_schedule_parent.json")
HEADER = os.path.join(ROOT, "include", "fruitnerf_hip.h")
STEPS = 14           # step 0, the every-step updates before step 10, update and non-update steps after
N_RAYS = 160
CASE_SECONDS = 120   # a case takes a few seconds; one that hangs ends the process instead of the machine's patience


def stream_arguments() -> dict:
    """entry point -> positions of its stream arguments, from the C header's prototypes."""
    from fruitnerf_amd import _lib as L
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    found, where = set(), {}
    for m in re.finditer(r"\b(fnr_\w+)\s*\(([^()]*)\)\s*;", text):
        name, params = m.group(1), [p.strip() for p in m.group(2).split(",")]
        if name in L.SIGNATURES and len(params) == len(L.SIGNATURES[name][1]):
            found.add(name)
            idx = tuple(i for i, p in enumerate(params) if re.search(r"void\s*\*\s*(stream|waiting|signalling)$", p))
            if idx:
                where[name] = idx
    missing = [n for n, (_, args) in L.SIGNATURES.items() if args and n not in found]
    if missing:
        raise RuntimeError(f"no prototype read from {HEADER} for {missing[:5]}")
    return where


class ScheduleLog:
    """Stands in for the loaded library: notes every entry point outside training._PROGRAM_QUERIES with its streams."""

    def __init__(self, lib, where: dict, launch: int, side):
        self._lib, self._where, self._launch, self._side, self.calls = lib, where, int(launch or 0), side, []

    def _which(self, arg) -> str:
        raw = int(getattr(arg, "value", arg) or 0)
        if raw == self._launch:
            return "launch"
        side = self._side()
        return "side" if side is not None and raw == int(side.cuda_stream or 0) else "other"

    def __getattr__(self, name):
        from fruitnerf_amd.training import _PROGRAM_QUERIES
        fn = getattr(self._lib, name)
        if not name.startswith("fnr_") or name in _PROGRAM_QUERIES:
            return fn
        where, calls, which = self._where.get(name, ()), self.calls, self._which

        def logged(*a):
            calls.append(name + "@" + ",".join(which(a[i]) for i in where) if where else name)
            return fn(*a)
        return logged


class Recorder:
    """with rec.step(model): ...   -> one list of entries per block, in rec.steps."""

    def __init__(self, dev):
        self.dev, self.steps, self._where = dev, [], stream_arguments()

    @contextlib.contextmanager
    def step(self, model):
        from fruitnerf_amd import _lib as L
        lib = L.load()
        log = ScheduleLog(lib, self._where, torch.cuda.current_stream(self.dev).cuda_stream,
                          lambda: model.__dict__.get("_side_stream"))
        L._lib = log
        try:
            yield
        finally:
            L._lib = lib
            self.steps.append(log.calls)


@contextlib.contextmanager
def switches(**values):
    """Module attributes of fruitnerf_amd.training for the length of a case."""
    import fruitnerf_amd.training as T
    saved = {k: getattr(T, k) for k in values}
    for k, v in values.items():
        setattr(T, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(T, k, v)


# ---- the cases ------------------------------------------------------------------------------------------------


def loop_case(camera=True, tweak=None, **module_switches):
    """The loop of tests/test_gpu_sequencer._loop on N_RAYS rays, STEPS interpreted steps."""
    def run(dev, rec):
        from tests.test_gpu_sequencer import _loop
        with switches(NATIVE_SEQUENCER=False, **module_switches):
            loop, hm, opt, batcher, cam = _loop(dev, n_rays=N_RAYS, camera=camera)
            if tweak is not None:
                tweak(hm, opt)
            for _ in range(STEPS):
                with rec.step(hm):
                    loop.step()
            torch.cuda.synchronize()
    return run


def _semgrad(hm, opt):
    hm.config.pass_semantic_gradients = hm.field.pass_semantic_gradients = True


def _white_scaled(hm, opt):
    hm.config.background_color, hm.config.use_gradient_scaling = "white", True


def _distortion(hm, opt):
    hm.config.use_distortion_loss = True


def _per_edge(hm, opt):
    hm.proposal_sampler.single_jitter = False


def _torch_1_13_stepping(hm, opt):
    opt.skip_groups_without_grad = False


def _small_model(dev, seed, tweak=None, num_images=7):
    from tests import util
    hm = util.make_hip_like(util.make_oracle(util.small_config(log2=15, prop_log2=13), num_images=num_images, seed=seed), dev)
    if tweak is not None:
        tweak(hm, None)
    hm.arena()
    return hm


def _rays_and_batch(dev, seed):
    from fruitnerf_amd.rays import RayBundle
    from tests import util
    o, d, pa, cam = util.random_rays(N_RAYS, 7, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    batch = {"image": torch.rand(N_RAYS, 3, generator=g).to(dev),
             "fruit_mask": (torch.rand(N_RAYS, 1, generator=g) > 0.5).float().to(dev)}
    return (lambda grad=False: RayBundle(o.to(dev).requires_grad_(grad), d.to(dev).requires_grad_(grad), pa.to(dev),
                                         cam.to(dev))), batch


def eval_ray_grads_case(dev, rec):
    """fused_forward_backward(ray_grads={}) on a model in eval mode — no saved Jacobian, the gather path — on one stream,
    with the second stream (free and serialised), and with the table's optimiser step fused into the scatter."""
    import fruitnerf_amd.training as T
    hm = _small_model(dev, 9)
    hm.eval()
    rays, batch = _rays_and_batch(dev, 4)
    opt = T.FusedAdam(hm)
    for kw in ({}, {}, {"overlap_proposal_backward": True}, {"overlap_proposal_backward": True, "serialize_streams": True},
               {"table_adam": True}, {"table_adam": True, "overlap_proposal_backward": True}):
        kw = dict(kw)
        if kw.pop("table_adam", False):
            kw["table_adam"] = opt.table_adam_args(hm.field.mlp_base_grid.hash_table, "fields")[0]
        with rec.step(hm):
            T.fused_forward_backward(hm, rays(), batch, ray_grads={}, **kw)
    torch.cuda.synchronize()


def autograd_case(tweak=None, ray_grads=True):
    """model(...) -> get_metrics_dict -> get_loss_dict -> loss.backward(), twice, the rays requiring grad."""
    def run(dev, rec):
        hm = _small_model(dev, 9, tweak)
        hm.train()
        rays, batch = _rays_and_batch(dev, 4)
        for _ in range(2):
            hm.set_anneal(0)
            with rec.step(hm):
                out = hm(rays(grad=ray_grads))
                md = hm.get_metrics_dict(out, batch)
                sum(hm.get_loss_dict(out, batch, md).values()).backward()
        torch.cuda.synchronize()
    return run


def field_case(dev, rec):
    """FruitField.forward(...).backward() and get_density / get_outputs: _FieldFn."""
    from fruitnerf_amd.fruit_field import FieldHeadNames
    hm = _small_model(dev, 41)
    hm.train()
    rays, _ = _rays_and_batch(dev, 5)
    S = 24
    euclid = torch.sort(torch.rand(N_RAYS, S + 1, generator=torch.Generator().manual_seed(3)) * 1.6 + 0.2, dim=-1).values
    hs = rays().get_ray_samples(euclid[:, :-1, None].to(dev), euclid[:, 1:, None].to(dev))
    for two_calls in (False, True):
        with rec.step(hm):
            if two_calls:
                dens, emb = hm.field.get_density(hs)
                out = hm.field.get_outputs(hs, density_embedding=emb)
            else:
                out = hm.field(hs)
                dens = out[FieldHeadNames.DENSITY]
            (dens.sum() + out[FieldHeadNames.RGB].sum() + out[FieldHeadNames.SEMANTICS].sum()).backward()
    torch.cuda.synchronize()


@contextlib.contextmanager
def one_rank_group(dev, port):
    """The one-rank RCCL group of tests/test_gpu_distributed.py."""
    import torch.distributed as dist
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        yield
    finally:
        if created:
            dist.destroy_process_group()


def exchange_case(sharded: bool, level_groups: int):
    """TrainingSteps over a one-rank process group with the gradient exchange forced on (EXCHANGE_MIN_WORLD = 1)."""
    def run(dev, rec):
        import fruitnerf_amd.training as T
        from fruitnerf_amd.cameras.camera_optimizers import CameraAdam, CameraOptimizerConfig
        from fruitnerf_amd.data import synthetic_apple as sa
        n_cam, HW, focal = 8, 64, 90.0
        data = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in
                sa.render_dataset(sa.make_scene(seed=0), sa.make_cameras(n_cam, seed=0), H=HW, W=HW, fx=focal, fy=focal).items()}
        with one_rank_group(dev, 29647 + 2 * int(sharded) + level_groups), switches(NATIVE_SEQUENCER=False, EXCHANGE_MIN_WORLD=1, SHARDED_FIELD_OPTIMIZER=sharded,
                                           EXCHANGE_LEVEL_GROUPS=level_groups):
            hm = _small_model(dev, 21, num_images=n_cam)
            hm.train()
            cam = CameraOptimizerConfig(mode="SO3xR3").setup(n_cam, dev)
            batcher = sa.PixelBatcher(data, torch.arange(n_cam, device=dev), seed=3)
            loop = T.TrainingSteps(hm, T.FusedAdam(hm), batcher, N_RAYS, camera=(cam, CameraAdam(cam)), world_size=1)
            for _ in range(STEPS):
                with rec.step(hm):
                    loop.step()
            hm.field.flush_deferred_update()
            torch.cuda.synchronize()
    return run


CASES = {
    "default": loop_case(),
    "no_camera": loop_case(camera=False),
    "overlap_proposal_backward_off": loop_case(OVERLAP_PROPOSAL_BACKWARD=False),
    "overlap_proposal_backward_off_no_camera": loop_case(camera=False, OVERLAP_PROPOSAL_BACKWARD=False),
    "serialize_streams": loop_case(SERIALIZE_STREAMS=True),
    "losses_on_side_off": loop_case(LOSSES_ON_SIDE=False),
    "fuse_composite_backward_off": loop_case(FUSE_COMPOSITE_BACKWARD=False),
    "pair_proposal_levels_off": loop_case(PAIR_PROPOSAL_LEVELS=False),
    "fuse_table_optimizer_off": loop_case(FUSE_TABLE_OPTIMIZER=False),
    "fuse_weight_optimizer_off": loop_case(FUSE_WEIGHT_OPTIMIZER=False),
    "sample_ahead_off": loop_case(SAMPLE_AHEAD=False),
    "skip_groups_without_grad_off": loop_case(tweak=_torch_1_13_stepping),
    "pass_semantic_gradients": loop_case(tweak=_semgrad),
    "white_background_gradient_scaling": loop_case(tweak=_white_scaled),
    "distortion_loss": loop_case(tweak=_distortion),
    "distortion_loss_losses_on_side_off": loop_case(tweak=_distortion, LOSSES_ON_SIDE=False),
    "per_edge_jitter": loop_case(tweak=_per_edge),
    "eval_ray_grads": eval_ray_grads_case,
    "autograd": autograd_case(),
    "autograd_no_ray_grads": autograd_case(ray_grads=False),
    "autograd_distortion_loss": autograd_case(_distortion),
    "autograd_pass_semantic_gradients": autograd_case(_semgrad),
    "autograd_white_background_gradient_scaling": autograd_case(_white_scaled),
    "field_forward_backward": field_case,
    "exchange_all_reduce": exchange_case(False, 1),
    "exchange_all_reduce_two_level_groups": exchange_case(False, 2),
    "exchange_sharded": exchange_case(True, 1),
    "exchange_sharded_two_level_groups": exchange_case(True, 2),
}


def record(case: str, dev) -> dict:
    """One case on `dev`, under its own time limit -> {"shapes": [[entry, ...], ...], "steps": [shape index per step]}."""
    rec = Recorder(dev)
    faulthandler.dump_traceback_later(CASE_SECONDS, exit=True)
    try:
        torch.manual_seed(0)
        CASES[case](dev, rec)
    finally:
        faulthandler.cancel_dump_traceback_later()
    shapes, steps = [], []
    for calls in rec.steps:
        if calls not in shapes:
            shapes.append(calls)
        steps.append(shapes.index(calls))
    return {"shapes": shapes, "steps": steps}


def expand(stored: dict) -> list:
    return [stored["shapes"][i] for i in stored["steps"]]


def main(argv) -> int:
    out = argv[1] if len(argv) > 1 else FIXTURE
    dev = torch.device("cuda:0")
    result = {}
    for case in CASES:
        result[case] = record(case, dev)
        print(f"[step schedule] {case}: {len(result[case]['steps'])} steps, {len(result[case]['shapes'])} shapes, "
              f"{sum(len(s) for s in expand(result[case]))} calls", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in result.items())
                + "\n}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
