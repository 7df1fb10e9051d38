"""k_distortion_bwd next to k_weights_bwd (the launch class it was estimated from) at the final-level shapes of `fruit_nerf`
(4096 rays x 48 samples) and `fruit_nerf_big` (8192 x 128), alternated rounds of 50 launches each; meant to run under a
rocprofv3 kernel trace, summarised by tools/kt_per_ray.py.  Without the profiler it prints HIP-event times per launch
(launch gaps included)."""
import sys

import torch

sys.path.insert(0, __import__('os').getcwd())   # run from the root of the build under test
from fruitnerf_amd import _kernels as K   # noqa: E402

dev = torch.device('cuda:0')
g = torch.Generator().manual_seed(0)
for R, S in ((4096, 48), (8192, 128)):
    edges = torch.cumsum(torch.rand(R, S + 1, generator=g) * 0.05 + 0.01, 1)
    spacing = ((edges - edges[:, :1]) / (edges[:, -1:] - edges[:, :1])).to(dev)
    edges = edges.to(dev)
    density = (torch.rand(R, S, generator=g) * (3.0 / (S * 0.035))).to(dev)
    rays = K.RaysArg(torch.zeros(R, 3, device=dev), torch.tensor([[0.0, 0.0, 1.0]], device=dev).repeat(R, 1),
                     torch.full((R, 1), 0.05, device=dev), torch.full((R, 1), 1000.0, device=dev))
    weights = K.composite_fwd(rays, S, edges, density.view(-1), torch.rand(R * S, 3, device=dev),
                              torch.randn(R * S, device=dev), True)[0]
    d_w = torch.randn(R, S, device=dev)
    d_density = torch.zeros(R * S, device=dev)
    calls = {"weights_bwd": lambda: K.weights_bwd(S, edges, density, weights, d_w, None),
             "distortion_bwd": lambda: K.distortion_bwd(S, spacing, edges, density.view(-1), weights, 0.002, d_density)}
    ms = {k: [] for k in calls}
    for rnd in range(6):
        for name, call in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(50):
                call()
            t1.record()
            torch.cuda.synchronize()
            if rnd:                      # round 0 warms up
                ms[name].append(t0.elapsed_time(t1) / 50 * 1e3)
    for name, v in ms.items():
        print(f"{R} x {S} {name}: {sorted(v)[len(v) // 2]:.1f} us per launch (median of {len(v)} rounds of 50, HIP events; "
              f"min {min(v):.1f} max {max(v):.1f})")
