"""Training step time of the default loop (TrainingSteps: 4096 rays, camera optimiser, two streams, step programs) with
use_distortion_loss off and on, on the same build: alternated windows of `steps` steps per setting, host clock around
work that ends in a device synchronise.   usage: distortion_step_time.py [fruit_nerf | fruit_nerf_big] [steps] [windows]"""
import sys
import time

import torch

sys.path.insert(0, __import__('os').getcwd())   # run from the root of the build under test
import fruitnerf_amd.training as T   # noqa: E402
from fruitnerf_amd.cameras.camera_optimizers import CameraAdam, CameraOptimizerConfig   # noqa: E402
from fruitnerf_amd.data import synthetic_apple as sa   # noqa: E402
from fruitnerf_amd.data.semantics import apple_metadata   # noqa: E402
from fruitnerf_amd.fruit_nerf import FruitModel, FruitNerfModelConfig   # noqa: E402

method = sys.argv[1] if len(sys.argv) > 1 else "fruit_nerf"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 300
windows = int(sys.argv[3]) if len(sys.argv) > 3 else 4
big = method == "fruit_nerf_big"
dev = torch.device("cuda:0")
HW, n_train = 200, 40
focal = 1111.0 * HW / 800
scene = sa.make_scene(seed=0, device=dev)
c2w = sa.make_cameras(n_train, seed=0, device=dev)
data = sa.render_dataset(scene, c2w, H=HW, W=HW, fx=focal, fy=focal)
n_rays = 8192 if big else 4096


def make(on):
    batcher = sa.PixelBatcher(data, torch.arange(n_train, device=dev), seed=1)
    torch.manual_seed(0)
    cfg = FruitNerfModelConfig(use_distortion_loss=on)
    if big:
        cfg.log2_hashmap_size, cfg.max_res = 21, 4096
        cfg.geo_feat_dim, cfg.num_layers_semantic, cfg.hidden_dim_semantics = 30, 3, 128
        cfg.num_nerf_samples_per_ray, cfg.num_proposal_samples_per_ray = 128, (512, 256)
    hm = FruitModel(cfg, apple_metadata(), num_train_data=n_train, device=dev)
    hm.train()
    alg = "radam" if big else "adam"
    opt = T.FusedAdam(hm, algorithm=alg)
    cam_opt = CameraOptimizerConfig(mode="SO3xR3").setup(n_train, dev)
    return T.TrainingSteps(hm, opt, batcher, n_rays, camera=(cam_opt, CameraAdam(cam_opt, algorithm=alg)))


loops = {on: make(on) for on in (False, True)}
for loop in loops.values():              # warm-up: every step shape recorded
    for i in range(100):
        loop.step(want_metrics=False)
torch.cuda.synchronize()
ms = {False: [], True: []}
for w in range(windows):
    for on, loop in loops.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            loop.step(want_metrics=False)
        torch.cuda.synchronize()
        ms[on].append((time.perf_counter() - t0) / steps * 1e3)
for on, v in ms.items():
    print(f"{method} {n_rays} rays use_distortion_loss={on}: " + " ".join(f"{x:.4f}" for x in v) +
          f" ms/step (windows of {steps}); median {sorted(v)[len(v) // 2]:.4f}; replayed {loops[on].stats['replayed']}")
