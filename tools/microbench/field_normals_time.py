"""Time of fnr_field_normals alone at the training shape (N = 4096 rays x 48 samples): HIP events around single launches,
warm-up first, the median of `reps` launches; prints the time and the fraction of the HBM floor (profiles/field_normals.md).
    python tools/microbench/field_normals_time.py [n_samples] [reps] [library]"""
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from fruitnerf_amd import _kernels as K   # noqa: E402
from fruitnerf_amd import _lib as L   # noqa: E402


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096 * 48
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    if len(sys.argv) > 3:
        L.LIB_PATH = os.path.abspath(sys.argv[3])      # another build of the library (A/B of kernel variants)
    dev = torch.device("cuda:0")
    print("device:", L.device_check())
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.rand(*s, device=dev, generator=g) * 2 - 1   # noqa: E731
    w0, b0, w1 = r(64, 32) * 0.4, r(64) * 0.3, r(16, 64) * 0.3
    feats, jac = r(16, N, 2) * 0.8, r(16, 3, N, 2) * 64
    sel = (torch.rand(N, device=dev, generator=g) > 0.12).to(torch.uint8)
    net = L.fnr_field_net()
    net.grid = K.make_grid(torch.zeros(64, device=dev), 16, 4, [16] * 16)
    net.geo_feat_dim, net.hidden_dim = 15, 64
    net.base_w0, net.base_b0, net.base_w1 = L.ptr(w0), L.ptr(b0), L.ptr(w1)
    normals = torch.empty(N, 3, device=dev)
    lib = L.load()

    def launch():
        L.check(lib.fnr_field_normals(C.byref(net), N, L.ptr(feats), L.ptr(jac), L.ptr(sel), L.ptr(normals), None,
                                      L.stream_ptr(dev)), "field_normals")

    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    # one pair of events around a window of back-to-back launches: no per-launch event bubble (the buffers, 103 MB, do not fit
    # the 4 MB L2s; the 256 MB Infinity Cache holds them, as it would behind an encode that has just written them)
    window = 200
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(window):
        launch()
    b.record()
    b.synchronize()
    print(f"back to back: {a.elapsed_time(b) / window * 1e3:.1f} us per launch over {window} launches")
    med = statistics.median(ms)
    nbytes = N * (384 + 128 + 1 + 12)
    floor_us = nbytes / 8e12 * 1e6
    print(f"fnr_field_normals N={N}: median {med * 1e3:.1f} us over {reps} launches (min {min(ms) * 1e3:.1f}, max {max(ms) * 1e3:.1f}); "
          f"{nbytes / 1e6:.1f} MB -> {nbytes / (med * 1e-3) / 1e12:.2f} TB/s, floor at 8 TB/s {floor_us:.1f} us = "
          f"{floor_us / (med * 1e3):.2f} of the time")


if __name__ == "__main__":
    main()
