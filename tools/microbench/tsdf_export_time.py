"""Time of the TSDF mesh export's two device stages at an export-sized problem (profiles/tsdf_export.md): fusion of
`n_cameras` analytic depth images of a sphere into a `res`^3 volume (fnr_tsdf_integrate, `batch` cameras per launch) next to
a torch restatement of the same update on the same device (one camera at a time over all nodes, as Nerfstudio's TSDF does),
and marching tetrahedra on the result (fnr_tsdf_mesh_count + the host read of the counts + fnr_tsdf_mesh_emit).  The two
fusions are compared before anything is timed.  Host clock around work that ends in a device synchronise; medians.
    python tools/microbench/tsdf_export_time.py [res] [n_cameras] [H] [W] [batch] [reps]"""
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from fruitnerf_amd import _lib as L   # noqa: E402
from fruitnerf_amd.export.tsdf import TSDF   # noqa: E402

RADIUS, WALL = 0.55, 6.0


def look_at(eye):
    back = torch.nn.functional.normalize(eye, dim=0)
    right = torch.nn.functional.normalize(torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0], dtype=eye.dtype), back), dim=0)
    return torch.cat([torch.stack([right, torch.linalg.cross(back, right), back], dim=1), eye[:, None]], dim=1)


def scene(n, H, W, dev):
    """n cameras on a tilted ring of radius 2.5 around a sphere of radius RADIUS at the origin; ray-distance depth images
    (a far wall behind the sphere) and smooth colour images."""
    ang = torch.arange(n, dtype=torch.float64) * (2 * math.pi / n)
    eyes = torch.stack([2.5 * torch.cos(ang), 2.5 * torch.sin(ang), 0.8 * torch.sin(3 * ang)], dim=1)
    c2w = torch.stack([look_at(e) for e in eyes]).float().to(dev)
    f = 0.9 * W
    intr = torch.tensor([[f, f, W / 2 + 0.3, H / 2 - 0.2]], dtype=torch.float32).repeat(n, 1).to(dev)
    rows, cols = torch.meshgrid(torch.arange(H, device=dev) + 0.5, torch.arange(W, device=dev) + 0.5, indexing="ij")
    depth = torch.empty(n, H, W, device=dev)
    for c in range(n):
        d = torch.stack([(cols - intr[c, 2]) / intr[c, 0], -(rows - intr[c, 3]) / intr[c, 1], -torch.ones_like(cols)], -1)
        d = torch.nn.functional.normalize(d, dim=-1) @ c2w[c, :, :3].T
        b = d @ c2w[c, :, 3]
        disc = b * b - (c2w[c, :, 3] @ c2w[c, :, 3] - RADIUS ** 2)
        depth[c] = torch.where(disc > 0, -b - torch.sqrt(disc.clamp_min(0)), torch.full_like(b, WALL))
    rgb = 0.5 + 0.5 * torch.sin(torch.stack([rows / 7, cols / 11, (rows + cols) / 13], -1))[None] * torch.ones(n, 1, 1, 1, device=dev)
    return c2w, intr, depth, rgb.contiguous()


def torch_fuse(vol, P, truncation, c2w, intr, depth, rgb, max_weight=1.0):
    """The contract of include/fruitnerf_hip.h (ray-distance depth) in float32 torch ops, one camera at a time."""
    values, weights, colors = vol
    H, W = depth.shape[1:]
    for c in range(c2w.shape[0]):
        d, R = P - c2w[c, :, 3], c2w[c, :, :3]
        q = d[:, 0:1] * R[0] + d[:, 1:2] * R[1] + d[:, 2:3] * R[2]          # R^T d without a GEMM: plain float32 products
        z = -q[:, 2]
        col = torch.round(intr[c, 0] * q[:, 0] / z + intr[c, 2] - 0.5)
        row = torch.round(intr[c, 1] * -q[:, 1] / z + intr[c, 3] - 0.5)
        inside = (z > 0) & (col >= 0) & (col < W) & (row >= 0) & (row < H)
        pix = torch.where(inside, row * W + col, torch.zeros_like(col)).long()
        sampled = torch.where(inside, depth[c].reshape(-1)[pix], torch.zeros_like(z))
        dist = sampled - q.norm(dim=1)
        valid = inside & (sampled > 0) & (dist > -truncation)
        s = (dist / truncation).clamp(-1.0, 1.0)
        values = torch.where(valid, (values * weights + s) / (weights + 1), values)
        colors = torch.where(valid[:, None], (colors * weights[:, None] + rgb[c].reshape(-1, 3)[pix]) / (weights[:, None] + 1),
                             colors)
        weights = torch.where(valid, (weights + 1).clamp_max(max_weight), weights)
    return values, weights, colors


def timed(fn, reps, dev):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), out


def main():
    a = [int(v) for v in sys.argv[1:]]
    res, n, H, W, batch, reps = (a + [128, 20, 270, 480, 10, 7][len(a):])[:6]
    dev = torch.device("cuda:0")
    print("device:", L.device_check())
    c2w, intr, depth, rgb = scene(n, H, W, dev)
    aabb = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])

    def hip_fuse():
        tsdf = TSDF.from_aabb(aabb, res, dev)
        for b in range(0, n, batch):
            tsdf.integrate(c2w[b:b + batch], intr[b:b + batch], depth[b:b + batch], rgb[b:b + batch])
        return tsdf

    idx = torch.stack(torch.meshgrid(*[torch.arange(res, device=dev, dtype=torch.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    vs = ((aabb[1] - aabb[0]) / res).to(dev)
    P = aabb[0].to(dev) + idx * vs
    truncation = 5.0 * float(vs[0])

    def ref_fuse():
        N = res ** 3
        return torch_fuse((torch.full((N,), -1.0, device=dev), torch.zeros(N, device=dev), torch.zeros(N, 3, device=dev)),
                          P, truncation, c2w, intr, depth, rgb)

    tsdf, ref = hip_fuse(), ref_fuse()
    # the two float32 programs may round a projection that sits on a pixel tie to different pixels: those nodes read
    # another depth sample and are counted apart
    diff = (tsdf.values.reshape(-1) - ref[0]).abs()
    other = (diff > 1e-5) | (tsdf.weights.reshape(-1) != ref[1])
    print(f"kernel vs torch restatement: {int(other.sum())} of {other.numel()} nodes differ by more than 1e-5 or in weight "
          f"(largest {float(diff.max()):.3g}), max |value difference| on the rest {float(diff[~other].max()):.3g}; "
          f"observed nodes {int((ref[1] > 0).sum())}")
    def hip_again():                 # into the volume that exists: the same work per node and camera, no allocation
        for b in range(0, n, batch):
            tsdf.integrate(c2w[b:b + batch], intr[b:b + batch], depth[b:b + batch], rgb[b:b + batch])

    for _ in range(2):
        hip_again(), ref_fuse()
    med_h, min_h, _ = timed(hip_again, reps, dev)
    med_t, min_t, _ = timed(ref_fuse, max(3, reps // 2), dev)
    pairs = res ** 3 * n
    print(f"fusion {res}^3 nodes x {n} cameras of {H}x{W}, {batch} per launch: "
          f"fnr_tsdf_integrate median {med_h:.3f} ms (min {min_h:.3f}) = {pairs / med_h / 1e6:.1f} G node-cameras/s; "
          f"torch restatement median {med_t:.1f} ms (min {min_t:.1f}); ratio {med_t / med_h:.0f}x")
    tsdf.get_mesh()
    med_m, min_m, mesh = timed(tsdf.get_mesh, reps, dev)
    print(f"extraction on the result: {mesh[0].shape[0]} vertices, {mesh[1].shape[0]} faces; count + host read + emit "
          f"median {med_m:.3f} ms (min {min_m:.3f})")


if __name__ == "__main__":
    main()
