#!/usr/bin/env python3
"""Train rays/s of the loop an unmodified Nerfstudio Trainer runs over the plugin surface, by optimiser.

The loop of bench.py's `plugin_api_window` (callbacks, model(ray_bundle), get_metrics_dict, get_loss_dict, backward()
through the autograd Functions, optimiser, schedulers; fresh model, 10 untimed + 100 timed steps, camera optimiser off) in
three variants, one process, one JSON line:

  torch_optim            Optimizers over torch.optim.Adam / RAdam per group + an enabled GradScaler: what `ns-train` ran
                         while the method configs named Nerfstudio's AdamOptimizerConfig / RAdamOptimizerConfig
                         (zero_grad_all -> scale(loss).backward() -> optimizer_scaler_step_all -> update -> schedulers)
  fused_adam             training.FusedAdam.step(skip=skipped_groups(model)) called directly, no scaler: this repo's own
                         plugin-API loop (bench.py's figure of the same name)
  method_config_default  the same Trainer calls as torch_optim over Optimizers(optimizer_configs(method)): the fused
                         optimiser configs the entry points now carry (engine.optimizers.ArenaAdam)

usage: plugin_api_rate.py [--method fruit_nerf] [--steps 100] [--warmup 10] [--variants a,b,c]
"""
import argparse
import functools
import json
import os
import sys
import time
from dataclasses import dataclass
from typing import Optional

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

VARIANTS = ("torch_optim", "fused_adam", "method_config_default")


@dataclass
class TorchOptimizerConfig:
    """Nerfstudio's AdamOptimizerConfig / RAdamOptimizerConfig, as far as Optimizers reads it."""
    algorithm: str
    lr: float
    eps: float
    max_norm: Optional[float] = None
    weight_decay: float = 0

    def setup(self, params):
        cls = torch.optim.Adam if self.algorithm == "adam" else torch.optim.RAdam
        return cls(params, lr=self.lr, eps=self.eps, weight_decay=self.weight_decay)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", default="fruit_nerf")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--image-size", type=int, default=800)
    ap.add_argument("--mlp-precision", default="bf16x3")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    args = ap.parse_args()
    import bench
    from fruitnerf_amd import fruit_nerf_config as FC
    from fruitnerf_amd.data import synthetic_apple as sa
    from fruitnerf_amd.engine.callbacks import TrainingCallbackAttributes, TrainingCallbackLocation as Loc
    from fruitnerf_amd.engine.optimizers import Optimizers
    from fruitnerf_amd.hostinfo import usable_cpus
    from fruitnerf_amd.rays import RayBundle
    from fruitnerf_amd.training import skipped_groups
    torch.set_num_threads(usable_cpus())
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    focal = 1111.0 * args.image_size / 800.0
    scene = sa.make_scene(seed=0, device=dev)
    c2w = sa.make_cameras(bench.N_CAMERAS, seed=0, device=dev)
    data = sa.render_dataset(scene, c2w, H=args.image_size, W=args.image_size, fx=focal, fy=focal)
    i_train, _ = bench.split_indices(bench.N_CAMERAS, bench.TRAIN_SPLIT)
    train_ids = torch.as_tensor(i_train, device=dev)
    rays_per_batch = bench.METHODS[args.method]["rays"]

    def window(kind: str) -> dict:
        run = bench.MethodRun(args.method, args.mlp_precision, "off", dev, 0, 1, data, train_ids, len(i_train))
        model = run.model
        cbs = model.get_training_callbacks(TrainingCallbackAttributes(optimizers=None, grad_scaler=None, pipeline=None))
        opts = scaler = None
        if kind == "fused_adam":
            fused = run.opt
        else:
            configs = FC.optimizer_configs(args.method)
            if kind == "torch_optim":
                model.arena()          # (torch.optim captures the parameters; they are re-homed before or after alike)
                for g, o in FC.METHODS[args.method]["optimizers"].items():
                    configs[g]["optimizer"] = TorchOptimizerConfig(o["algorithm"], o["lr"], o["eps"])
            opts = Optimizers(configs, model.get_param_groups())
            scaler = torch.amp.GradScaler("cuda", enabled=True)
        t0 = 0.0
        for step in range(args.warmup + args.steps):
            if step == args.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            for cb in cbs:
                cb.run_callback_at_location(step, location=Loc.BEFORE_TRAIN_ITERATION)
            o, d, cam, batch = run.batcher.sample(run.rays)
            if opts is not None:
                opts.zero_grad_all()
            outputs = model(RayBundle(o, d, None, cam))
            metrics_dict = model.get_metrics_dict(outputs, batch)
            loss_dict = model.get_loss_dict(outputs, batch, metrics_dict)
            loss = functools.reduce(torch.add, loss_dict.values())
            if opts is None:
                loss.backward()
                fused.step(skip=skipped_groups(model))
            else:
                scaler.scale(loss).backward()
                opts.optimizer_scaler_step_all(scaler)
                scaler.update()
                opts.scheduler_step_all(step)
            for cb in cbs:
                cb.run_callback_at_location(step, location=Loc.AFTER_TRAIN_ITERATION)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        out = {"rays_per_s": round(args.steps * rays_per_batch / seconds, 1),
               "ms_per_step": round(1e3 * seconds / args.steps, 4),
               "final_loss": {k: round(float(v), 6) for k, v in loss_dict.items()}}
        if opts is not None:
            out["optimizer_steps"] = {g: sorted({int(s["step"]) for s in o.state_dict()["state"].values()})
                                      for g, o in opts.optimizers.items()}
            out["loss_scale"] = scaler.get_scale()
        else:
            out["optimizer_steps"] = {g: [n] for g, n in fused.group_steps.items()}
        del run, model, opts
        torch.cuda.empty_cache()
        return out

    result = {"tool": "plugin_api_rate", "method": args.method, "mlp_precision": args.mlp_precision,
              "rays_per_batch": rays_per_batch, "untimed_steps": args.warmup, "timed_steps": args.steps,
              "device": torch.cuda.get_device_name(dev), "torch": torch.__version__}
    for kind in args.variants.split(","):
        if kind not in VARIANTS:
            raise SystemExit(f"unknown variant {kind!r} (one of {', '.join(VARIANTS)})")
        result[kind] = window(kind)
    if all(k in result for k in VARIANTS):
        r = {k: result[k]["rays_per_s"] for k in VARIANTS}
        result["method_config_default_over_torch_optim"] = round(r["method_config_default"] / r["torch_optim"], 4)
        result["method_config_default_over_fused_adam"] = round(r["method_config_default"] / r["fused_adam"], 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
