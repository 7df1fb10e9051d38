"""Thin tensor-level wrappers over the C ABI (one Python function per entry point).

All tensors must live on a HIP device; every call is enqueued on PyTorch's current stream for that
device.  No arithmetic happens here.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L


def _f32c(t: Tensor) -> Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


class StepArena:
    """A caller-owned slab for the per-step buffers of a training loop (training.TrainingSteps): bump allocation, reset
    every other step.  While one is active (`use_arena`) the wrappers below take their output / scratch buffers from it
    instead of torch's caching allocator, so a step's buffers sit at the SAME addresses whenever the same sequence of
    calls runs from the same reset point — what a recorded step program (fnr_program_*) replays against.  Requests
    that do not fit fall back to torch.empty and are counted (`overflow_bytes`): the owner grows the slab between steps."""

    ALIGN = 256

    def __init__(self, device, capacity: int):
        self.device = torch.device(device)
        self.capacity = int(capacity)
        self.buf = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
        self._typed = {torch.uint8: self.buf}
        self.offset = 0
        self.overflow_bytes = 0
        self.high_water = 0

    def reset(self) -> None:
        self.offset = 0

    def alloc(self, shape, dtype) -> Tensor:
        n = 1
        for d in shape:
            n *= int(d)
        nbytes = n * _ITEMSIZE[dtype]
        start = self.offset
        end = start + nbytes
        if end > self.capacity:
            self.overflow_bytes += nbytes
            return torch.empty(*shape, dtype=dtype, device=self.device)
        self.offset = (end + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        if self.offset > self.high_water:
            self.high_water = self.offset
        typed = self._typed.get(dtype)
        if typed is None:
            typed = self._typed[dtype] = self.buf.view(dtype)
        isz = _ITEMSIZE[dtype]
        t = typed[start // isz:end // isz]           # (start is a multiple of ALIGN, hence of the item size)
        return t.view(*shape) if len(shape) != 1 else t


_ITEMSIZE = {torch.float32: 4, torch.uint8: 1, torch.int32: 4, torch.int64: 8, torch.float64: 8}
_ARENA: Optional[StepArena] = None


def use_arena(arena: Optional[StepArena]) -> Optional[StepArena]:
    """Make `arena` (or none) the source of the wrappers' per-call buffers -> the previous one."""
    global _ARENA
    prev, _ARENA = _ARENA, arena
    return prev


def _empty(*shape, dtype=torch.float32, device=None) -> Tensor:
    a = _ARENA
    if a is not None and a.device == device:
        return a.alloc(shape, dtype)
    return torch.empty(*shape, dtype=dtype, device=device)


class RaysArg:
    """fnr_rays view of RayBundle tensors (keeps the converted tensors alive)."""

    def __init__(self, origins: Tensor, directions: Tensor, nears: Optional[Tensor], fars: Optional[Tensor],
                 camera_indices: Optional[Tensor] = None):
        L.require_gpu_tensor(origins, "ray origins")
        self.device = origins.device
        self.origins = _f32c(origins.reshape(-1, 3))
        self.directions = _f32c(directions.reshape(-1, 3))
        self.n = self.origins.shape[0]
        self.nears = None if nears is None else _f32c(nears.reshape(-1))
        self.fars = None if fars is None else _f32c(fars.reshape(-1))
        self.cam = None
        if camera_indices is not None:
            self.cam = camera_indices.reshape(-1).to(torch.int32).contiguous()
        self.c = L.fnr_rays(self.n, L.ptr(self.origins), L.ptr(self.directions), L.ptr(self.nears), L.ptr(self.fars),
                            L.ptr(self.cam))

    @property
    def ref(self):
        return C.byref(self.c)


_warp_cache = {}


def make_warp(mode: int, aabb: Tensor) -> L.fnr_warp:
    # reading the aabb back is a device->host copy (a full stream sync): do it once per buffer version
    key = (mode, aabb.data_ptr(), aabb._version, str(aabb.device))
    cached = _warp_cache.get(key)
    if cached is not None:
        return cached
    w = _make_warp_uncached(mode, aabb)
    if len(_warp_cache) > 64:
        _warp_cache.clear()
    _warp_cache[key] = w
    return w


def _make_warp_uncached(mode: int, aabb: Tensor) -> L.fnr_warp:
    w = L.fnr_warp()
    w.mode = mode
    a = aabb.detach().to("cpu", torch.float32).reshape(-1).tolist()
    for i in range(6):
        w.aabb[i] = a[i]
    return w


def make_grid(table: Tensor, n_levels: int, log2_hashmap_size: int, scalings: Sequence[int]) -> L.fnr_grid:
    g = L.fnr_grid()
    g.n_levels = n_levels
    g.log2_hashmap_size = log2_hashmap_size
    for i, s in enumerate(scalings):
        g.scalings[i] = int(s)
    g.table = L.ptr(table)
    return g


def hash_scalings(num_levels: int, min_res: int, max_res: int) -> list:
    """floor(min_res * growth**levels) in float32, exactly as nerfstudio HashEncoding.__init__
    (reference call sites fruit_field.py:124-131, fruit_nerf.py:111-127)."""
    levels = torch.arange(num_levels)
    growth = np.exp((np.log(max_res) - np.log(min_res)) / (num_levels - 1)) if num_levels > 1 else 1
    return [int(v) for v in torch.floor(min_res * growth ** levels).tolist()]


_host_linspace_cache = {}


def host_linspace(start: float, end: float, steps: int, device) -> Tensor:
    """torch.linspace evaluated on the CPU (ATen's rounding), cached on the device."""
    key = (float(start), float(end), int(steps), str(device))
    t = _host_linspace_cache.get(key)
    if t is None:
        t = torch.linspace(start, end, steps, dtype=torch.float32).to(device)
        _host_linspace_cache[key] = t
    return t


# ---- stream dependencies (recordable by step programs: fnr_program_*) ---------------------------------


def _raw(stream) -> Optional[int]:
    """hipStream_t of a torch.cuda.Stream (or a raw handle / None = the default stream)."""
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else stream


class Event:
    """A hipEvent_t (timing disabled) owned by the caller: what crosses between the launch stream and the second stream
    of a training step.  Unlike torch.cuda.Event its record / wait go through the C ABI, so a step program records them."""

    def __init__(self):
        h = C.c_void_p()
        L.check(L.load().fnr_event_create(C.byref(h)), "event_create")
        self.handle = h.value

    def record(self, stream) -> None:
        L.check(L.load().fnr_event_record(self.handle, _raw(stream)), "event_record")

    def __del__(self):
        try:
            if self.handle and L._lib is not None:
                L.load().fnr_event_destroy(self.handle)
        except Exception:   # interpreter shutdown
            pass


def stream_wait_event(stream, event: Event) -> None:
    L.check(L.load().fnr_stream_wait_event(_raw(stream), event.handle), "stream_wait_event")


def stream_wait_stream(waiting, signalling) -> None:
    """Work enqueued on `waiting` from now on runs after everything `signalling` holds now (the host does not block)."""
    L.check(L.load().fnr_stream_wait_stream(_raw(waiting), _raw(signalling)), "stream_wait_stream")


# ---- samplers ---------------------------------------------------------------------------------------


def sample_spaced(rays: RaysArg, spacing_kind: int, S: int, t_rand: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """t_rand: None (bin edges = linspace), [R] / [R,1] (one jitter per ray) or [R, S+1] (one per bin edge)."""
    lib = L.load()
    dev = rays.device
    base = host_linspace(0.0, 1.0, S + 1, dev)
    spacing = _empty(rays.n, S + 1, device=dev)
    euclid = _empty(rays.n, S + 1, device=dev)
    tr = None if t_rand is None else _f32c(t_rand.reshape(-1))
    per_bin = 0
    if tr is not None and tr.numel() != rays.n:
        if tr.numel() != rays.n * (S + 1):
            raise ValueError(f"t_rand has {tr.numel()} entries; expected {rays.n} (per ray) or {rays.n * (S + 1)} (per bin)")
        per_bin = 1
    L.check(lib.fnr_sample_spaced(rays.ref, spacing_kind, S, L.ptr(base), L.ptr(tr), per_bin, L.ptr(spacing),
                                  L.ptr(euclid), L.stream_ptr(dev)), "sample_spaced")
    return spacing, euclid


def edge_jitter(seed: int, offset: int, level: int, n_rays: int, n_edges: int, device, out: Optional[Tensor] = None) -> Tensor:
    """use_single_jitter=False: [n_rays, n_edges] of U[0,1), the per-edge jitter of sampling `level` (0 = spaced sampler, 1.. =
    PDF samplers) from the training prologue's generator (fnr_edge_jitter) — what fnr_train_prologue_edges and
    fnr_weights_pdf_edges(draw) derive in their kernels on the same seed and offset."""
    lib = L.load()
    if out is None:
        out = _empty(n_rays, n_edges, device=device)
    L.check(lib.fnr_edge_jitter(int(seed) & ((1 << 64) - 1), int(offset) & ((1 << 64) - 1), int(level), n_rays, n_edges,
                                L.ptr(out), L.stream_ptr(out.device)), "edge_jitter")
    return out


def weights_pdf(rays: RaysArg, spacing_kind: int, S_prev: int, S_new: int, density: Tensor, spacing_prev: Tensor,
                euclid_prev: Tensor, anneal: float, rand: Optional[Tensor], want_depth: bool = True,
                per_edge: bool = False, draw: Optional[Tuple[int, int, int]] = None):
    """rand: None (eval: centred u) or one number per ray, [R] / [R,1]; with per_edge (single_jitter=False,
    fnr_weights_pdf_edges) one per new bin edge, [R, S_new+1], or None with draw = (seed, offset, level): the kernel draws
    K.edge_jitter(seed, offset, level) itself."""
    lib = L.load()
    dev = rays.device
    weights = _empty(rays.n, S_prev, device=dev)
    depth = _empty(rays.n, device=dev) if want_depth else None
    spacing_new = euclid_new = u_base = None
    if S_new > 0:
        nb = S_new + 1
        u_base = host_linspace(0.0, 1.0 - (1.0 / nb), nb, dev)
        spacing_new = _empty(rays.n, nb, device=dev)
        euclid_new = _empty(rays.n, nb, device=dev)
    rd = None if rand is None else _f32c(rand.reshape(-1))
    if per_edge:
        if rd is not None and rd.numel() != rays.n * (S_new + 1):
            raise ValueError(f"rand has {rd.numel()} entries; expected {rays.n * (S_new + 1)} (per bin edge)")
        seed, offset, level = draw if draw is not None else (0, 0, 0)
        L.check(lib.fnr_weights_pdf_edges(rays.ref, spacing_kind, S_prev, S_new, L.ptr(density), L.ptr(spacing_prev),
                                          L.ptr(euclid_prev), float(anneal), L.ptr(u_base), L.ptr(rd), L.ptr(weights),
                                          L.ptr(depth), L.ptr(spacing_new), L.ptr(euclid_new),
                                          int(seed) & ((1 << 64) - 1), int(offset) & ((1 << 64) - 1), int(level),
                                          1 if draw is not None else 0, L.stream_ptr(dev)), "weights_pdf_edges")
        return weights, depth, spacing_new, euclid_new
    L.check(lib.fnr_weights_pdf(rays.ref, spacing_kind, S_prev, S_new, L.ptr(density), L.ptr(spacing_prev),
                                L.ptr(euclid_prev), float(anneal), L.ptr(u_base), L.ptr(rd), L.ptr(weights),
                                L.ptr(depth), L.ptr(spacing_new), L.ptr(euclid_new), L.stream_ptr(dev)),
            "weights_pdf")
    return weights, depth, spacing_new, euclid_new


# ---- networks ----------------------------------------------------------------------------------------


def prop_density_fwd(net: L.fnr_prop_net, warp: L.fnr_warp, rays: RaysArg, euclid: Tensor, S: int,
                     save_feats: bool = False):
    lib = L.load()
    dev = rays.device
    density = _empty(rays.n, S, device=dev)
    feats = _empty(net.grid.n_levels, rays.n * S, 2, device=dev) if save_feats else None
    L.check(lib.fnr_prop_density_fwd(C.byref(net), C.byref(warp), rays.ref, L.ptr(euclid), S, L.ptr(density),
                                     L.ptr(feats), L.stream_ptr(dev)), "prop_density_fwd")
    return density, feats


def hash_encode_fwd(grid: L.fnr_grid, warp: L.fnr_warp, rays: RaysArg, euclid: Tensor, S: int,
                    want_jacobian: bool = False):
    """-> feats [L,N,2], selector [N] (+ the input Jacobian [L,3,N,2] for position_grad_from_jacobian)."""
    lib = L.load()
    dev = rays.device
    N = rays.n * S
    feats = _empty(grid.n_levels, N, 2, device=dev)
    selector = _empty(N, dtype=torch.uint8, device=dev)
    jac = _empty(grid.n_levels, 3, N, 2, device=dev) if want_jacobian else None
    L.check(lib.fnr_hash_encode_fwd(C.byref(grid), C.byref(warp), rays.ref, L.ptr(euclid), S, L.ptr(feats),
                                    L.ptr(selector), L.ptr(jac), L.stream_ptr(dev)), "hash_encode_fwd")
    return (feats, selector, jac) if want_jacobian else (feats, selector)


class LatticeArg:
    def __init__(self, xs: Tensor, ys: Tensor, zs: Tensor):
        self.xs, self.ys, self.zs = _f32c(xs), _f32c(ys), _f32c(zs)
        self.device = self.xs.device
        self.c = L.fnr_lattice(self.xs.numel(), self.ys.numel(), self.zs.numel(), L.ptr(self.xs), L.ptr(self.ys),
                               L.ptr(self.zs))

    @property
    def ref(self):
        return C.byref(self.c)


def hash_encode_lattice(grid: L.fnr_grid, warp: L.fnr_warp, lat: LatticeArg, ray_begin: int, n_rays: int):
    lib = L.load()
    dev = lat.device
    N = n_rays * lat.c.n_z
    feats = _empty(grid.n_levels, N, 2, device=dev)
    selector = _empty(N, dtype=torch.uint8, device=dev)
    L.check(lib.fnr_hash_encode_lattice(C.byref(grid), C.byref(warp), lat.ref, ray_begin, n_rays, L.ptr(feats),
                                        L.ptr(selector), L.stream_ptr(dev)), "hash_encode_lattice")
    return feats, selector


_MLP_FWD_WS = {}


def _mlp_fwd_workspace(dev, n_rays: int) -> Tensor:
    """Per-device scratch for the packed fragment image + per-ray colour bias (reused and grown on demand:
    calls are ordered on the device's stream)."""
    key = (dev.type, dev.index)
    need = L.load().fnr_field_mlp_fwd_workspace_bytes(n_rays)
    ws = _MLP_FWD_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _MLP_FWD_WS[key] = ws
    return ws


def field_mlp_fwd(net: L.fnr_field_net, rays: RaysArg, S: int, feats: Tensor, selector: Optional[Tensor],
                  mean_embedding: Optional[Tensor], want_geo: bool = False, want_h: bool = False):
    lib = L.load()
    dev = rays.device
    N = rays.n * S
    density = _empty(N, device=dev)
    rgb = _empty(N, 3, device=dev)
    logit = _empty(N, device=dev)
    geo = _empty(N, net.geo_feat_dim, device=dev) if want_geo else None
    # base-MLP output [N, 16 | 32]: saved for field_mlp_bwd; the fruit_nerf_big shape always needs it (its two
    # launches hand h over through it); + the per-ray part of mlp_head's first layer [R,64]
    h_dim = lib.fnr_field_h_dim(C.byref(net))
    if h_dim < 0:
        raise RuntimeError("fruitnerf_hip field_mlp_fwd: " + L.last_error())
    h = _empty(N, h_dim, device=dev) if (want_h or h_dim > 16) else None
    ray_bias = _empty(rays.n, 64, device=dev) if want_h else None
    # training: a private workspace, so that its packed fragment image can be handed to field_mlp_bwd
    ws = (_empty(lib.fnr_field_mlp_fwd_workspace_bytes(0), dtype=torch.uint8, device=dev) if want_h
          else _mlp_fwd_workspace(dev, rays.n))
    L.check(lib.fnr_field_mlp_fwd(C.byref(net), rays.ref, S, L.ptr(feats), L.ptr(selector), L.ptr(mean_embedding),
                                  L.ptr(density), L.ptr(rgb), L.ptr(logit), L.ptr(geo), L.ptr(h), L.ptr(ray_bias),
                                  L.ptr(ws), ws.numel(), L.stream_ptr(dev)),
            "field_mlp_fwd")
    if want_h:
        # the workspace holds the fragment images of THIS call's weights in THIS call's arithmetic (fnr_field_net.mlp_mode)
        return density, rgb, logit, geo, (h, ray_bias, ws, int(net.mlp_mode))
    return density, rgb, logit, geo


def field_normals(net: L.fnr_field_net, feats: Tensor, jacobian: Tensor, selector: Tensor, want_gradient: bool = False):
    """feats [L,N,2], jacobian [L,3,N,2], selector [N] of hash_encode_fwd(want_jacobian=True) -> normals [N,3]
    (+ the unnormalised gradient [N,3])."""
    lib = L.load()
    dev = feats.device
    N = selector.numel()
    assert feats.shape == (net.grid.n_levels, N, 2) and jacobian.shape == (net.grid.n_levels, 3, N, 2) \
        and feats.dtype == jacobian.dtype == torch.float32 and selector.dtype == torch.uint8
    normals = _empty(N, 3, device=dev)
    gradient = _empty(N, 3, device=dev) if want_gradient else None
    L.check(lib.fnr_field_normals(C.byref(net), N, L.ptr(feats), L.ptr(jacobian), L.ptr(selector), L.ptr(normals),
                                  L.ptr(gradient), L.stream_ptr(dev)), "field_normals")
    return (normals, gradient) if want_gradient else normals


def render_normals(weights: Tensor, normals: Tensor, S: int, shade: bool) -> Tensor:
    """weights [R,S], normals [R*S,3] -> the rendered normal per ray [R,3] (shade: mapped to [0,1])."""
    lib = L.load()
    dev = weights.device
    w, nr = _f32c(weights.reshape(-1, S)), _f32c(normals.reshape(-1, 3))
    R = w.shape[0]
    assert nr.shape[0] == R * S
    out = _empty(R, 3, device=dev)
    if R:
        L.check(lib.fnr_render_normals(R, S, L.ptr(w), L.ptr(nr), int(bool(shade)), L.ptr(out), L.stream_ptr(dev)),
                "render_normals")
    return out


def embedding_mean(embedding: Tensor) -> Tensor:
    lib = L.load()
    out = _empty(embedding.shape[1], device=embedding.device)
    L.check(lib.fnr_embedding_mean(L.ptr(embedding), embedding.shape[0], embedding.shape[1], L.ptr(out),
                                   L.stream_ptr(embedding.device)), "embedding_mean")
    return out


def composite_fwd(rays: RaysArg, S: int, euclid: Tensor, density: Tensor, rgb: Tensor, logit: Tensor, training: bool):
    lib = L.load()
    dev = rays.device
    weights = _empty(rays.n, S, device=dev)
    out_rgb = _empty(rays.n, 3, device=dev)
    acc = _empty(rays.n, device=dev)
    depth = _empty(rays.n, device=dev)
    sem = _empty(rays.n, device=dev)
    label = _empty(rays.n, dtype=torch.int64, device=dev)
    L.check(lib.fnr_composite_fwd(rays.ref, S, L.ptr(euclid), L.ptr(density), L.ptr(rgb), L.ptr(logit),
                                  1 if training else 0, L.ptr(weights), L.ptr(out_rgb), L.ptr(acc), L.ptr(depth),
                                  L.ptr(sem), L.ptr(label), L.stream_ptr(dev)), "composite_fwd")
    return weights, out_rgb, acc, depth, sem, label


def _composite_fwd_bwd_call(name: str, rays: RaysArg, S: int, *args):
    """fnr_<name>(rays, S, *args, <six forward outputs>, <three gradients>, stream) with the outputs allocated here (tensors
    among `args` by address, as in _composite_bwd_call).  -> (weights, out_rgb, acc, depth, sem, label), (d_density, d_rgb,
    d_logit)."""
    dev = rays.device
    N = rays.n * S
    outs = (_empty(rays.n, S, device=dev), _empty(rays.n, 3, device=dev), _empty(rays.n, device=dev),
            _empty(rays.n, device=dev), _empty(rays.n, device=dev), _empty(rays.n, dtype=torch.int64, device=dev))
    grads = (_empty(N, device=dev), _empty(N, 3, device=dev), _empty(N, device=dev))
    argv = [L.ptr(a) if isinstance(a, Tensor) else a for a in args]
    L.check(getattr(L.load(), "fnr_" + name)(rays.ref, S, *argv, *map(L.ptr, outs + grads), L.stream_ptr(dev)), name)
    return outs, grads


def composite_fwd_bwd_targets(rays: RaysArg, S: int, euclid: Tensor, density: Tensor, rgb: Tensor, logit: Tensor, image: Tensor,
                              mask: Tensor, sem_weight: float, semgrad: bool = False):
    """composite_fwd (training) and composite_bwd_targets as one launch (fnr_composite_fwd_bwd_targets): the same outputs and
    gradients, bit for bit.  -> (weights, out_rgb, acc, depth, sem, label), (d_density, d_rgb, d_logit).
    semgrad (pass_semantic_gradients): fnr_composite_fwd_bwd_targets_semgrad — d_density carries the semantic term too."""
    return _composite_fwd_bwd_call("composite_fwd_bwd_targets_semgrad" if semgrad else "composite_fwd_bwd_targets", rays, S,
                                   euclid, density, rgb, logit, _f32c(image), _f32c(mask.reshape(-1)), float(sem_weight))


class CompositeOptions:
    """fnr_composite_options for the `_opt` compositing calls.  background: None = the last sample's colour; a [3] tensor =
    one triple for every ray ("white" / "black"); an [R,3] tensor = one per ray ("random").  The tensor is kept alive here."""

    def __init__(self, background: Optional[Tensor] = None, gradient_scaling: bool = False, semgrad: bool = False):
        self.background = None if background is None else _f32c(background)
        if self.background is not None and (self.background.dim() not in (1, 2) or self.background.shape[-1] != 3):
            raise ValueError("CompositeOptions: background is a [3] or an [R,3] tensor")
        self.gradient_scaling, self.semgrad = bool(gradient_scaling), bool(semgrad)

    @property
    def plain(self) -> bool:
        """Neither option set: what the entry points without `_opt` compute."""
        return self.background is None and not self.gradient_scaling

    def ref(self, n_rays: int):
        bg = self.background
        if bg is not None and bg.dim() == 2 and bg.shape[0] != n_rays:
            raise ValueError(f"CompositeOptions: background of {bg.shape[0]} rows for {n_rays} rays")
        o = L.fnr_composite_options(L.FNR_BACKGROUND_LAST_SAMPLE if bg is None else L.FNR_BACKGROUND_EXPLICIT,
                                    3 if (bg is not None and bg.dim() == 2) else 0, L.ptr(bg),
                                    1 if self.gradient_scaling else 0, 1 if self.semgrad else 0)
        return C.byref(o)


def random_background(seed: int, offset: int, n_rays: int, device, out: Optional[Tensor] = None) -> Tensor:
    """background_color="random": [n_rays,3] of U[0,1) from the training prologue's generator (fnr_random_background: same
    seed and offset as the step's rays, a word group of its own)."""
    lib = L.load()
    if out is None:
        out = _empty(n_rays, 3, device=device)
    L.check(lib.fnr_random_background(int(seed) & ((1 << 64) - 1), int(offset) & ((1 << 64) - 1), n_rays, L.ptr(out),
                                      L.stream_ptr(out.device)), "random_background")
    return out


def composite_fwd_opt(rays: RaysArg, S: int, euclid: Tensor, density: Tensor, rgb: Tensor, logit: Tensor, training: bool,
                      opts: CompositeOptions):
    """composite_fwd with an explicit background (fnr_composite_fwd_opt)."""
    lib = L.load()
    dev = rays.device
    weights = _empty(rays.n, S, device=dev)
    out_rgb = _empty(rays.n, 3, device=dev)
    acc = _empty(rays.n, device=dev)
    depth = _empty(rays.n, device=dev)
    sem = _empty(rays.n, device=dev)
    label = _empty(rays.n, dtype=torch.int64, device=dev)
    L.check(lib.fnr_composite_fwd_opt(rays.ref, S, L.ptr(euclid), L.ptr(density), L.ptr(rgb), L.ptr(logit),
                                      1 if training else 0, opts.ref(rays.n), L.ptr(weights), L.ptr(out_rgb), L.ptr(acc),
                                      L.ptr(depth), L.ptr(sem), L.ptr(label), L.stream_ptr(dev)), "composite_fwd_opt")
    return weights, out_rgb, acc, depth, sem, label


def composite_fwd_bwd_targets_opt(rays: RaysArg, S: int, euclid: Tensor, density: Tensor, rgb: Tensor, logit: Tensor,
                                  image: Tensor, mask: Tensor, sem_weight: float, opts: CompositeOptions):
    """composite_fwd_bwd_targets under the options (fnr_composite_fwd_bwd_targets_opt): bit-identical to composite_fwd_opt +
    composite_bwd_targets_opt.  -> (weights, out_rgb, acc, depth, sem, label), (d_density, d_rgb, d_logit)."""
    return _composite_fwd_bwd_call("composite_fwd_bwd_targets_opt", rays, S, euclid, density, rgb, logit, _f32c(image),
                                   _f32c(mask.reshape(-1)), float(sem_weight), opts.ref(rays.n))


# ---- export -------------------------------------------------------------------------------------------


def export_compact(lat: Optional[LatticeArg], ray_begin: int, n_rays: int, positions: Optional[Tensor],
                   density: Tensor, rgb: Tensor, logit: Tensor, points: Sequence[Tensor], colors: Sequence[Tensor],
                   counts: Tensor) -> None:
    """Appends this batch's selected samples to the three point/colour streams (order-preserving); `counts`
    (uint64 x3, stored as int64 on the device) holds the running totals.  Positions: lattice or explicit."""
    lib = L.load()
    dev = density.device
    N = density.numel()
    if N == 0:
        return      # an empty batch appends nothing (its tensors have no storage: the C entry point would see NULLs)
    ws = _empty(lib.fnr_export_workspace_bytes(N), dtype=torch.uint8, device=dev)
    cap = points[0].shape[0]
    assert all(p.shape[0] == cap for p in points) and all(c.shape[0] == cap for c in colors)
    parr = (C.c_void_p * 3)(*[L.ptr(p) for p in points])
    carr = (C.c_void_p * 3)(*[L.ptr(c) for c in colors])
    pos = None if positions is None else _f32c(positions.reshape(-1, 3))
    L.check(lib.fnr_export_compact(None if lat is None else lat.ref, ray_begin, n_rays, L.ptr(pos), N,
                                   L.ptr(density), L.ptr(rgb), L.ptr(logit), parr, carr, cap, L.ptr(counts),
                                   L.ptr(ws), L.stream_ptr(dev)), "export_compact")


def depth_points(origins: Tensor, directions: Tensor, depth: Tensor, rgb: Tensor, box_min, box_max, points: Tensor,
                 colors: Tensor, count: Tensor, normals: Optional[Tensor] = None,
                 normals_out: Optional[Tensor] = None) -> None:
    """Appends origin + direction * depth (fp32, torch's bits) and rgb of the rays whose point lies strictly inside the
    box (box_min / box_max: 3 floats each, or both None) to points / colors [capacity,3] in ray order; `count` (uint64,
    stored as int64 [1] on the device) is the running total.  normals [R,3] + normals_out [capacity,3] (together): the
    per-ray attribute of fnr_depth_points_normals travels with its point."""
    lib = L.load()
    dev = depth.device
    R = depth.numel()
    if R == 0:
        return
    o, d, t, c = _f32c(origins.reshape(-1, 3)), _f32c(directions.reshape(-1, 3)), _f32c(depth.reshape(-1)), \
        _f32c(rgb.reshape(-1, 3))
    assert o.shape[0] == d.shape[0] == c.shape[0] == R and points.shape == colors.shape and points.is_contiguous() \
        and colors.is_contiguous() and points.dtype == colors.dtype == torch.float32
    ws = _empty(lib.fnr_export_workspace_bytes(R), dtype=torch.uint8, device=dev)
    lo = None if box_min is None else (C.c_float * 3)(*[float(v) for v in box_min])
    hi = None if box_max is None else (C.c_float * 3)(*[float(v) for v in box_max])
    if normals is None:
        assert normals_out is None
        L.check(lib.fnr_depth_points(L.ptr(o), L.ptr(d), L.ptr(t), L.ptr(c), R, lo, hi, L.ptr(points), L.ptr(colors),
                                     points.shape[0], L.ptr(count), L.ptr(ws), L.stream_ptr(dev)), "depth_points")
        return
    nr = _f32c(normals.reshape(-1, 3))
    assert nr.shape[0] == R and normals_out is not None and normals_out.shape == points.shape \
        and normals_out.is_contiguous() and normals_out.dtype == torch.float32
    L.check(lib.fnr_depth_points_normals(L.ptr(o), L.ptr(d), L.ptr(t), L.ptr(c), L.ptr(nr), R, lo, hi, L.ptr(points),
                                         L.ptr(colors), L.ptr(normals_out), points.shape[0], L.ptr(count), L.ptr(ws),
                                         L.stream_ptr(dev)), "depth_points_normals")


class TsdfVolumeArg:
    """fnr_tsdf_volume view of a TSDF volume's tensors: values / weights [nx,ny,nz], colors [nx,ny,nz,3], float32 and
    contiguous on the HIP device (kept alive here); lo / hi: 3 floats each."""

    def __init__(self, values: Tensor, weights: Tensor, colors: Tensor, lo, hi, truncation_margin: float,
                 max_weight: float):
        L.require_gpu_tensor(values, "TSDF values")
        if values.dim() != 3 or weights.shape != values.shape or colors.shape != values.shape + (3,):
            raise ValueError(f"TSDF arrays: values {tuple(values.shape)}, weights {tuple(weights.shape)}, colors "
                             f"{tuple(colors.shape)}; expected [nx,ny,nz], [nx,ny,nz], [nx,ny,nz,3]")
        for t in (values, weights, colors):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != values.device:
                raise ValueError("TSDF arrays must be contiguous float32 tensors on one device")
        self.tensors = (values, weights, colors)
        self.device = values.device
        self.n_nodes = values.numel()
        c = L.fnr_tsdf_volume()
        c.dims[:] = list(values.shape)
        c.lo[:] = [float(v) for v in lo]
        c.hi[:] = [float(v) for v in hi]
        c.truncation_margin, c.max_weight = float(truncation_margin), float(max_weight)
        c.values, c.weights, c.colors = values.data_ptr(), weights.data_ptr(), colors.data_ptr()
        self.c = c
        self.ref = C.byref(c)


def tsdf_integrate(vol: TsdfVolumeArg, c2w: Tensor, intrinsics: Tensor, depth: Tensor, rgb: Tensor,
                   mask: Optional[Tensor] = None, depth_kind: int = L.FNR_TSDF_DEPTH_RAY) -> None:
    """Fuses cameras c2w [n,3,4] / intrinsics [n,4] (fx, fy, cx, cy) with depth [n,H,W], rgb [n,H,W,3] and the optional
    mask [n,H,W] (bool / uint8, 0 = ignore the pixel) into the volume, in the order given (fnr_tsdf_integrate)."""
    n = c2w.shape[0]
    if c2w.shape != (n, 3, 4) or intrinsics.shape != (n, 4) or depth.dim() != 3 or depth.shape[0] != n \
            or rgb.shape != depth.shape + (3,) or (mask is not None and mask.shape != depth.shape):
        raise ValueError(f"tsdf_integrate: c2w {tuple(c2w.shape)}, intrinsics {tuple(intrinsics.shape)}, depth "
                         f"{tuple(depth.shape)}, rgb {tuple(rgb.shape)}"
                         + ("" if mask is None else f", mask {tuple(mask.shape)}"))
    if n == 0:
        return
    dev = vol.device
    c2w, intrinsics, depth, rgb = [_f32c(t).to(dev) for t in (c2w, intrinsics, depth, rgb)]
    m = None if mask is None else (mask != 0).to(device=dev, dtype=torch.uint8).contiguous()
    L.check(L.load().fnr_tsdf_integrate(vol.ref, n, L.ptr(c2w), L.ptr(intrinsics), depth.shape[1], depth.shape[2],
                                        L.ptr(depth), L.ptr(rgb), L.ptr(m), int(depth_kind), L.stream_ptr(dev)),
            "tsdf_integrate")


def tsdf_mesh(vol: TsdfVolumeArg):
    """Marching tetrahedra over the volume (fnr_tsdf_mesh_count, one host read of the two counts, fnr_tsdf_mesh_emit).
    -> vertices [V,3], faces [F,3] int32, normals [V,3], colors [V,3] on the device; their order is fixed by the volume."""
    lib = L.load()
    dev = vol.device
    nbytes = L.tsdf_mesh_workspace_bytes(vol.n_nodes)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    L.check(lib.fnr_tsdf_mesh_count(vol.ref, L.ptr(counts), L.ptr(ws), ws.numel() * 8, L.stream_ptr(dev)),
            "tsdf_mesh_count")
    n_vertices, n_faces = counts.tolist()
    vertices, normals, colors = (torch.empty(n_vertices, 3, device=dev) for _ in range(3))
    faces = torch.empty(n_faces, 3, dtype=torch.int32, device=dev)
    L.check(lib.fnr_tsdf_mesh_emit(vol.ref, L.ptr(ws), ws.numel() * 8, n_vertices, n_faces, L.ptr(vertices),
                                   L.ptr(normals), L.ptr(colors), L.ptr(faces), L.stream_ptr(dev)), "tsdf_mesh_emit")
    return vertices, faces, normals, colors


def _mesh_faces(faces: Tensor, who: str) -> Tensor:
    L.require_gpu_tensor(faces, f"{who} faces")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{who}: faces are int32 [F,3], got {faces.dtype} {tuple(faces.shape)}")
    return faces.contiguous()


def _workspace(nbytes: int, dev) -> Tensor:
    """nbytes of device memory, 16-byte aligned (the allocator's granule is larger)."""
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)


def mesh_components(faces: Tensor, n_vertices: int):
    """Connected components over shared edges (fnr_mesh_components; the contract is in include/fruitnerf_hip.h).
    faces int32 [F,3] with indices in [0, n_vertices) -> (face_component int32 [F], n_components, workspace); the
    workspace holds the edge table mesh_component_stats needs.  F == 0 launches nothing."""
    faces = _mesh_faces(faces, "mesh_components")
    dev, F = faces.device, faces.shape[0]
    labels = torch.empty(F, dtype=torch.int32, device=dev)
    if F == 0:
        return labels, 0, None
    lib = L.load()
    ws = _workspace(lib.fnr_mesh_workspace_bytes(F), dev)
    counts = torch.zeros(1, dtype=torch.int64, device=dev)
    L.check(lib.fnr_mesh_components(int(n_vertices), F, L.ptr(faces), L.ptr(labels), L.ptr(counts), L.ptr(ws),
                                    ws.numel() * 8, L.stream_ptr(dev)), "mesh_components")
    return labels, int(counts.item()), ws


def mesh_component_stats(vertices: Tensor, faces: Tensor, face_component: Tensor, n_components: int, workspace) -> dict:
    """Per-component statistics (fnr_mesh_component_stats) -> dict of device tensors: n_faces, boundary_edges,
    nonmanifold_edges int32 [C]; lo, hi float32 [C,3]; area, volume float64 [C]; moment float64 [C,3].  `workspace`
    is the one mesh_components returned for these faces."""
    faces = _mesh_faces(faces, "mesh_component_stats")
    L.require_gpu_tensor(vertices, "mesh_component_stats vertices")
    dev, F, C_ = faces.device, faces.shape[0], int(n_components)
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32 or vertices.device != dev \
            or face_component.shape != (F,) or face_component.dtype != torch.int32 or face_component.device != dev:
        raise ValueError("mesh_component_stats: vertices are float32 [V,3] and face_component int32 [F], on the faces' device")
    vertices, face_component = vertices.contiguous(), face_component.contiguous()
    out = {"n_faces": torch.zeros(C_, dtype=torch.int32, device=dev),
           "boundary_edges": torch.zeros(C_, dtype=torch.int32, device=dev),
           "nonmanifold_edges": torch.zeros(C_, dtype=torch.int32, device=dev),
           "lo": torch.empty(C_, 3, device=dev), "hi": torch.empty(C_, 3, device=dev),
           "area": torch.empty(C_, dtype=torch.float64, device=dev),
           "volume": torch.empty(C_, dtype=torch.float64, device=dev),
           "moment": torch.empty(C_, 3, dtype=torch.float64, device=dev)}
    if F == 0:
        if C_ != 0:
            raise ValueError("mesh_component_stats: a mesh without faces has no components")
        return out
    if workspace is None:
        raise ValueError("mesh_component_stats: needs the workspace mesh_components returned")
    arg = L.fnr_mesh_stats(*[out[k].data_ptr() for k in ("n_faces", "boundary_edges", "nonmanifold_edges", "lo", "hi",
                                                        "area", "volume", "moment")])
    L.check(L.load().fnr_mesh_component_stats(vertices.shape[0], F, L.ptr(vertices), L.ptr(faces), L.ptr(face_component),
                                              C_, L.ptr(workspace), workspace.numel() * 8, C.byref(arg),
                                              L.stream_ptr(dev)), "mesh_component_stats")
    return out


def mesh_select(faces: Tensor, n_vertices: int, face_keep: Tensor):
    """Order-preserving selection (fnr_mesh_select_count, one host read of the two counts, fnr_mesh_select_emit).
    face_keep [F] bool / uint8 -> (new_faces int32 [F',3], vertex_ids int32 [V'] ascending, face_ids int32 [F']
    ascending)."""
    faces = _mesh_faces(faces, "mesh_select")
    dev, F, V = faces.device, faces.shape[0], int(n_vertices)
    if face_keep.shape != (F,):
        raise ValueError(f"mesh_select: face_keep is [F] = [{F}], got {tuple(face_keep.shape)}")
    L.require_gpu_tensor(face_keep, "mesh_select face_keep")
    empty = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)          # noqa: E731
    if F == 0:
        return empty(0, 3), empty(0), empty(0)
    keep = (face_keep != 0).to(device=dev, dtype=torch.uint8).contiguous()
    lib = L.load()
    ws = _workspace(lib.fnr_mesh_select_workspace_bytes(V, F), dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    L.check(lib.fnr_mesh_select_count(V, F, L.ptr(faces), L.ptr(keep), L.ptr(counts), L.ptr(ws), ws.numel() * 8,
                                      L.stream_ptr(dev)), "mesh_select_count")
    n_new_vertices, n_new_faces = counts.tolist()
    new_faces, vertex_ids, face_ids = empty(n_new_faces, 3), empty(n_new_vertices), empty(n_new_faces)
    L.check(lib.fnr_mesh_select_emit(V, F, L.ptr(faces), L.ptr(ws), ws.numel() * 8, n_new_vertices, n_new_faces,
                                     L.ptr(new_faces), L.ptr(vertex_ids), L.ptr(face_ids), L.stream_ptr(dev)),
            "mesh_select_emit")
    return new_faces, vertex_ids, face_ids


MESH_ROWS_NEIGHBOURS, MESH_ROWS_FACES = 0, 1                   # FNR_MESH_ROWS_* of include/fruitnerf_hip.h
MESH_WEIGHTS = {"uniform": 0, "inverse_distance": 1}           # FNR_MESH_WEIGHTS_*


def _mesh_vertices(vertices: Tensor, dev, who: str) -> Tensor:
    L.require_gpu_tensor(vertices, f"{who} vertices")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32 or vertices.device != dev:
        raise ValueError(f"{who}: vertices are float32 [V,3] on the mesh's device, got {vertices.dtype} "
                         f"{tuple(vertices.shape)}")
    return vertices.contiguous()


def _mesh_rows(offsets: Tensor, entries: Tensor, n_rows: int, who: str):
    L.require_gpu_tensor(offsets, f"{who} offsets")
    if offsets.shape != (n_rows + 1,) or offsets.dtype != torch.int32 or entries.dim() != 1 \
            or entries.dtype != torch.int32 or entries.device != offsets.device:
        raise ValueError(f"{who}: rows are offsets int32 [{n_rows + 1}] and entries int32 [E] on one device")
    return offsets.contiguous(), entries.contiguous()


def mesh_vertex_rows(faces: Tensor, n_vertices: int, kind: int):
    """Per-vertex rows (fnr_mesh_vertex_rows_count, one host read of the count, fnr_mesh_vertex_rows_emit).  kind
    MESH_ROWS_NEIGHBOURS: row a = every b != a sharing a face with a; MESH_ROWS_FACES: row a = every face listing a; each
    once, ascending.  -> (offsets int32 [V + 1], entries int32 [E])."""
    faces = _mesh_faces(faces, "mesh_vertex_rows")
    dev, F, V = faces.device, faces.shape[0], int(n_vertices)
    if kind not in (MESH_ROWS_NEIGHBOURS, MESH_ROWS_FACES):
        raise ValueError(f"mesh_vertex_rows: kind {kind} is neither MESH_ROWS_NEIGHBOURS nor MESH_ROWS_FACES")
    if F == 0:
        return torch.zeros(V + 1, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    lib = L.load()
    ws = _workspace(lib.fnr_mesh_vertex_rows_workspace_bytes(V, F, kind), dev)
    counts = torch.zeros(1, dtype=torch.int64, device=dev)
    L.check(lib.fnr_mesh_vertex_rows_count(V, F, L.ptr(faces), kind, L.ptr(counts), L.ptr(ws), ws.numel() * 8,
                                           L.stream_ptr(dev)), "mesh_vertex_rows_count")
    E = int(counts.item())
    offsets = torch.empty(V + 1, dtype=torch.int32, device=dev)
    entries = torch.empty(E, dtype=torch.int32, device=dev)
    L.check(lib.fnr_mesh_vertex_rows_emit(V, F, kind, L.ptr(ws), ws.numel() * 8, E, L.ptr(offsets), L.ptr(entries),
                                          L.stream_ptr(dev)), "mesh_vertex_rows_emit")
    return offsets, entries


def mesh_smooth(vertices: Tensor, offsets: Tensor, neighbours: Tensor, factors, weights: str = "inverse_distance") -> Tensor:
    """fnr_mesh_smooth: one step per factor, p' = p + factor * (weighted mean of the row - p), in float64 across the
    steps.  -> float32 [V,3]."""
    vertices = _mesh_vertices(vertices, vertices.device, "mesh_smooth")
    if weights not in MESH_WEIGHTS:
        raise ValueError(f"mesh_smooth: weights is one of {sorted(MESH_WEIGHTS)}, got {weights!r}")
    dev, V = vertices.device, vertices.shape[0]
    offsets, neighbours = _mesh_rows(offsets, neighbours, V, "mesh_smooth")
    out = torch.empty_like(vertices)
    if V == 0:
        return out
    factors = [float(f) for f in factors]
    lib = L.load()
    ws = _workspace(lib.fnr_mesh_smooth_workspace_bytes(V), dev)
    L.check(lib.fnr_mesh_smooth(V, L.ptr(vertices), neighbours.shape[0], L.ptr(offsets), L.ptr(neighbours), len(factors),
                                (C.c_double * max(len(factors), 1))(*factors), MESH_WEIGHTS[weights], L.ptr(out), L.ptr(ws),
                                ws.numel() * 8, L.stream_ptr(dev)), "mesh_smooth")
    return out


def mesh_vertex_normals(vertices: Tensor, faces: Tensor, offsets: Tensor, face_rows: Tensor) -> Tensor:
    """fnr_mesh_vertex_normals: area-weighted vertex normals over the MESH_ROWS_FACES rows -> float32 [V,3]."""
    faces = _mesh_faces(faces, "mesh_vertex_normals")
    vertices = _mesh_vertices(vertices, faces.device, "mesh_vertex_normals")
    dev, V = faces.device, vertices.shape[0]
    offsets, face_rows = _mesh_rows(offsets, face_rows, V, "mesh_vertex_normals")
    normals = torch.empty_like(vertices)
    if V == 0:
        return normals
    ws = _workspace(64, dev)
    L.check(L.load().fnr_mesh_vertex_normals(V, faces.shape[0], L.ptr(vertices), L.ptr(faces), face_rows.shape[0],
                                             L.ptr(offsets), L.ptr(face_rows), L.ptr(normals), L.ptr(ws), 64,
                                             L.stream_ptr(dev)), "mesh_vertex_normals")
    return normals


def mesh_cluster(vertices: Tensor, faces: Tensor, voxel_size: float, origin) -> dict:
    """Vertex clustering (fnr_mesh_cluster_count, one host read of the two counts, fnr_mesh_cluster_emit).  origin: three
    host numbers.  -> dict of device tensors: vertex_cluster int32 [V]; offsets int32 [V' + 1] and members int32 [V]
    (the cluster rows); new_faces int32 [F',3] and face_ids int32 [F']."""
    faces = _mesh_faces(faces, "mesh_cluster")
    vertices = _mesh_vertices(vertices, faces.device, "mesh_cluster")
    dev, V, F = faces.device, vertices.shape[0], faces.shape[0]
    empty = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)          # noqa: E731
    lib = L.load()
    ws = _workspace(lib.fnr_mesh_cluster_workspace_bytes(V, F), dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    vertex_cluster = empty(V)
    o = (C.c_double * 3)(*[float(x) for x in origin])
    L.check(lib.fnr_mesh_cluster_count(V, F, L.ptr(vertices), L.ptr(faces), float(voxel_size), o, L.ptr(vertex_cluster),
                                       L.ptr(counts), L.ptr(ws), ws.numel() * 8, L.stream_ptr(dev)), "mesh_cluster_count")
    n_clusters, n_new_faces = counts.tolist() if V + F > 0 else (0, 0)
    out = {"vertex_cluster": vertex_cluster, "offsets": torch.zeros(n_clusters + 1, dtype=torch.int32, device=dev),
           "members": empty(V), "new_faces": empty(n_new_faces, 3), "face_ids": empty(n_new_faces)}
    if V > 0:
        L.check(lib.fnr_mesh_cluster_emit(V, F, L.ptr(faces), L.ptr(ws), ws.numel() * 8, n_clusters, n_new_faces,
                                          L.ptr(out["offsets"]), L.ptr(out["members"]), L.ptr(out["new_faces"]),
                                          L.ptr(out["face_ids"]), L.stream_ptr(dev)), "mesh_cluster_emit")
    return out


def mesh_rows_mean(offsets: Tensor, members: Tensor, values: Tensor) -> Tensor:
    """fnr_mesh_rows_mean: float64 mean of values [N,3] over every row's members, rounded -> float32 [rows,3]."""
    L.require_gpu_tensor(values, "mesh_rows_mean values")
    if values.dim() != 2 or values.shape[1] != 3 or values.dtype != torch.float32 or offsets.dim() != 1 or offsets.shape[0] < 1:
        raise ValueError("mesh_rows_mean: values are float32 [N,3] and offsets int32 [rows + 1]")
    R = offsets.shape[0] - 1
    offsets, members = _mesh_rows(offsets, members, R, "mesh_rows_mean")
    if values.device != offsets.device:
        raise ValueError("mesh_rows_mean: values and rows are on one device")
    dev, values = values.device, values.contiguous()
    out = torch.empty(R, 3, device=dev)
    if R == 0:
        return out
    ws = _workspace(64, dev)
    L.check(L.load().fnr_mesh_rows_mean(R, members.shape[0], L.ptr(offsets), L.ptr(members), values.shape[0], L.ptr(values),
                                        L.ptr(out), L.ptr(ws), 64, L.stream_ptr(dev)), "mesh_rows_mean")
    return out


# ---- training ---------------------------------------------------------------------------------------


def losses_fwd(rgb: Tensor, image: Tensor, semantics: Tensor, fruit_mask: Tensor, semantic_loss_weight: float):
    lib = L.load()
    dev = rgb.device
    R = rgb.shape[0]
    losses = _empty(3, device=dev)  # rgb_loss, semantics_loss, psnr
    d_rgb = _empty(R, 3, device=dev)
    d_sem = _empty(R, device=dev)
    L.check(lib.fnr_losses_fwd(R, L.ptr(_f32c(rgb)), L.ptr(_f32c(image.reshape(R, 3))),
                               L.ptr(_f32c(semantics.reshape(R))), L.ptr(_f32c(fruit_mask.reshape(R))),
                               float(semantic_loss_weight), L.ptr(losses), L.ptr(d_rgb), L.ptr(d_sem),
                               L.stream_ptr(dev)), "losses_fwd")
    return losses, d_rgb, d_sem


def interlevel_fwd(S_f: int, spacing_f: Tensor, weights_f: Tensor, S_p: int, spacing_p: Tensor, weights_p: Tensor,
                   mult: float, loss_acc: Tensor) -> Tensor:
    lib = L.load()
    dev = spacing_f.device
    R = spacing_f.shape[0]
    d_wp = _empty(R, S_p, device=dev)
    L.check(lib.fnr_interlevel_fwd(R, S_f, L.ptr(spacing_f), L.ptr(weights_f), S_p, L.ptr(spacing_p), L.ptr(weights_p),
                                   float(mult), L.ptr(loss_acc), L.ptr(d_wp), L.stream_ptr(dev)), "interlevel_fwd")
    return d_wp


def distortion(S: int, spacing: Tensor, weights: Tensor, out: Optional[Tensor] = None) -> Optional[Tensor]:
    """out: zeroed [FNR_LOSS_SLOTS] accumulator supplied by the caller (who sums it later); None -> returns the sum."""
    lib = L.load()
    dev = spacing.device
    slots = torch.zeros(L.FNR_LOSS_SLOTS, device=dev) if out is None else out
    L.check(lib.fnr_distortion(spacing.shape[0], S, L.ptr(spacing), L.ptr(weights), L.ptr(slots), L.stream_ptr(dev)),
            "distortion")
    return slots.sum() if out is None else None


def distortion_bwd(S: int, spacing: Tensor, euclid: Tensor, density: Tensor, weights: Tensor, mult: float,
                   d_density: Tensor, upstream: Optional[Tensor] = None, gradient_scaling: bool = False,
                   want_d_weights: bool = False) -> Optional[Tensor]:
    """Backward of the distortion loss of the final level (fnr_distortion_bwd), IN PLACE on d_density [N]: the term's
    d(loss)/d(density), scaled by clamp(midpoint^2, 0, 1) with gradient_scaling, is added to what the compositing backward
    left there.  upstream: device scalar (None: 1).  -> d(loss)/d(weights) [R,S] if wanted, else None."""
    lib = L.load()
    dev = spacing.device
    R = spacing.shape[0]
    assert d_density.numel() == R * S and d_density.dtype == torch.float32, "d_density is float32 [N]"
    d_w = _empty(R, S, device=dev) if want_d_weights else None
    if R == 0:
        return d_w
    L.check(lib.fnr_distortion_bwd(R, S, L.ptr(spacing), L.ptr(euclid), L.ptr(density), L.ptr(weights), float(mult),
                                   L.ptr(None if upstream is None else _f32c(upstream.reshape(1))),
                                   1 if gradient_scaling else 0, L.ptr(d_w), L.ptr(d_density), L.stream_ptr(dev)),
            "distortion_bwd")
    return d_w


def train_losses(rgb: Tensor, image: Tensor, semantics: Tensor, fruit_mask: Tensor, semantic_loss_weight: float,
                 S_f: int, spacing_f: Tensor, weights_f: Tensor, levels, interlevel_mult: float, want_distortion: bool,
                 accum: Tensor, fuse_weights_bwd: bool = False, want_ray_grads: bool = True):
    """losses_fwd + interlevel_fwd per proposal level + distortion + the slot sums in one launch.
    levels: [(S_p, spacing_p, weights_p), ...]; accum: float buffer of FNR_TRAIN_LOSSES_ACCUM_FLOATS, zeroed before its
    first use (every completed call leaves it zeroed; it is re-zeroed here when the call fails).
    -> losses [5] (rgb_loss, semantics_loss, psnr, interlevel_loss, distortion), d_rgb [R,3], d_semantics [R],
       [d_weights_p per level].
    fuse_weights_bwd: levels are (S_p, spacing_p, weights_p, euclid_p, density_p) and the last list holds each level's
    d(loss)/d(density) [R,S_p] (= weights_bwd of the level, unit upstream) instead of d_weights_p.
    want_ray_grads False: d_rgb / d_semantics are neither allocated nor written (-> None, None): the caller's composite
    backward forms them itself (composite_bwd_targets)."""
    lib = L.load()
    dev = rgb.device
    R = rgb.shape[0]
    rgb, image = _f32c(rgb), _f32c(image.reshape(R, 3))
    semantics, fruit_mask = _f32c(semantics.reshape(R)), _f32c(fruit_mask.reshape(R))
    # (never from the step arena: callers keep a step's loss scalars beyond the step after next — a replayed step
    #  program writes them to the buffer fnr_step_scalars.losses names)
    losses = torch.empty(5, device=dev)
    d_rgb = _empty(R, 3, device=dev) if want_ray_grads else None
    d_sem = _empty(R, device=dev) if want_ray_grads else None
    n = len(levels)
    outs = [_empty(R, lv[0], device=dev) for lv in levels]
    sp = (C.c_int * max(n, 1))(*[int(lv[0]) for lv in levels])
    vps = lambda ts: (C.c_void_p * max(n, 1))(*[L.ptr(t) for t in ts])   # noqa: E731
    if fuse_weights_bwd:
        d_wp, eu, dn, d_dn = None, vps([lv[3] for lv in levels]), vps([lv[4] for lv in levels]), vps(outs)
    else:
        d_wp, eu, dn, d_dn = vps(outs), None, None, None
    rc = lib.fnr_train_losses(R, L.ptr(rgb), L.ptr(image), L.ptr(semantics), L.ptr(fruit_mask),
                              float(semantic_loss_weight), L.ptr(d_rgb), L.ptr(d_sem), S_f, L.ptr(spacing_f),
                              L.ptr(weights_f), n, sp, vps([lv[1] for lv in levels]), vps([lv[2] for lv in levels]),
                              d_wp, eu, dn, d_dn, float(interlevel_mult), 1 if want_distortion else 0, L.ptr(accum),
                              L.ptr(losses), L.stream_ptr(dev))
    if rc != 0:
        accum.zero_()     # a failed call may leave slots / completion counters dirty for every later step
    L.check(rc, "train_losses")
    return losses, d_rgb, d_sem, outs


def _composite_bwd_call(name: str, rays: RaysArg, S: int, *args):
    """fnr_<name>(rays, S, *args, d_density, d_rgb, d_logit, stream) -> the three gradients, allocated here.  Tensors among
    `args` go by address; they are held until the call is enqueued and converted after the outputs are allocated, so a
    contiguous copy made for the call cannot give its memory to an output."""
    dev = rays.device
    N = rays.n * S
    grads = (_empty(N, device=dev), _empty(N, 3, device=dev), _empty(N, device=dev))
    argv = [L.ptr(a) if isinstance(a, Tensor) else a for a in args]
    L.check(getattr(L.load(), "fnr_" + name)(rays.ref, S, *argv, *map(L.ptr, grads), L.stream_ptr(dev)), name)
    return grads


def composite_bwd(rays: RaysArg, S: int, euclid: Tensor, density: Tensor, rgb: Tensor, weights: Tensor, g_rgb: Tensor,
                  g_sem: Tensor):
    return _composite_bwd_call("composite_bwd", rays, S, euclid, density, rgb, weights, _f32c(g_rgb),
                               _f32c(g_sem.reshape(-1)))


def composite_bwd_targets(rays: RaysArg, S: int, euclid: Tensor, density: Tensor, rgb: Tensor, weights: Tensor,
                          out_rgb: Tensor, image: Tensor, out_sem: Tensor, mask: Tensor, sem_weight: float):
    """composite_bwd with the per-ray loss gradients formed inside the kernel from the composited outputs and the batch
    (fnr_composite_bwd_targets): no dependence on the losses launch, same bits."""
    return _composite_bwd_call("composite_bwd_targets", rays, S, euclid, density, rgb, weights, _f32c(out_rgb), _f32c(image),
                               _f32c(out_sem.reshape(-1)), _f32c(mask.reshape(-1)), float(sem_weight))


def composite_bwd_semgrad(rays: RaysArg, S: int, euclid: Tensor, density: Tensor, rgb: Tensor, logit: Tensor,
                          weights: Tensor, g_rgb: Tensor, g_sem: Tensor):
    """composite_bwd under pass_semantic_gradients (fnr_composite_bwd_semgrad): the semantic renderer's weights are not
    detached, d_density also carries g_sem * logit_k (logit [N]: the per-sample logits); d_rgb / d_logit as composite_bwd."""
    return _composite_bwd_call("composite_bwd_semgrad", rays, S, euclid, density, rgb, logit, weights, _f32c(g_rgb),
                               _f32c(g_sem.reshape(-1)))


def composite_bwd_targets_semgrad(rays: RaysArg, S: int, euclid: Tensor, density: Tensor, rgb: Tensor, logit: Tensor,
                                  weights: Tensor, out_rgb: Tensor, image: Tensor, out_sem: Tensor, mask: Tensor,
                                  sem_weight: float):
    """composite_bwd_targets under pass_semantic_gradients (fnr_composite_bwd_targets_semgrad)."""
    return _composite_bwd_call("composite_bwd_targets_semgrad", rays, S, euclid, density, rgb, logit, weights, _f32c(out_rgb),
                               _f32c(image), _f32c(out_sem.reshape(-1)), _f32c(mask.reshape(-1)), float(sem_weight))


def composite_bwd_opt(rays: RaysArg, S: int, euclid: Tensor, density: Tensor, rgb: Tensor, logit: Tensor, weights: Tensor,
                      g_rgb: Tensor, g_sem: Tensor, opts: "CompositeOptions"):
    """composite_bwd / composite_bwd_semgrad under the options (fnr_composite_bwd_opt): explicit background, gradients
    scaled by the clamped squared distance of their sample."""
    return _composite_bwd_call("composite_bwd_opt", rays, S, euclid, density, rgb, logit, weights, _f32c(g_rgb),
                               _f32c(g_sem.reshape(-1)), opts.ref(rays.n))


def composite_bwd_targets_opt(rays: RaysArg, S: int, euclid: Tensor, density: Tensor, rgb: Tensor, logit: Tensor,
                              weights: Tensor, out_rgb: Tensor, image: Tensor, out_sem: Tensor, mask: Tensor,
                              sem_weight: float, opts: "CompositeOptions"):
    """composite_bwd_targets(_semgrad) under the options (fnr_composite_bwd_targets_opt)."""
    return _composite_bwd_call("composite_bwd_targets_opt", rays, S, euclid, density, rgb, logit, weights, _f32c(out_rgb),
                               _f32c(image), _f32c(out_sem.reshape(-1)), _f32c(mask.reshape(-1)), float(sem_weight),
                               opts.ref(rays.n))


def weights_bwd(S: int, euclid: Tensor, density: Tensor, weights: Tensor, d_weights: Tensor,
                upstream: Optional[Tensor]) -> Tensor:
    lib = L.load()
    dev = euclid.device
    R = euclid.shape[0]
    d_density = _empty(R, S, device=dev)
    L.check(lib.fnr_weights_bwd(R, S, L.ptr(euclid), L.ptr(density), L.ptr(weights), L.ptr(d_weights),
                                L.ptr(upstream), L.ptr(d_density), L.stream_ptr(dev)), "weights_bwd")
    return d_density


def field_mlp_bwd(net: L.fnr_field_net, grads: L.fnr_field_net, rays: RaysArg, S: int, feats: Tensor, h_saved,
                  selector: Tensor, d_density: Tensor, d_rgb: Tensor, d_logit: Tensor, jacobian: Optional[Tensor] = None,
                  weight_adam=None, semgrad: bool = False):
    """h_saved: what field_mlp_fwd(want_h=True) returned — (h [N,16], ray_bias [R,64], packed weights); a bare h tensor
    is accepted too (the per-ray bias and the fragment image are then recomputed).
    jacobian (hash_encode_fwd(want_jacobian=True)): -> (d_feats, d_position [N,4]): the hash grid's input gradient per
    sample rides along (fnr_field_mlp_bwd_rays); position_grad_reduce(..., d_position.view(1, N, 4), ...) finishes it.
    weight_adam = (fnr_table_adam, gradient arena): the optimiser step of the MLP weights + embedding is taken by the
    kernels that finish their gradients (fnr_field_mlp_bwd_adam, FusedAdam.weight_adam_args).
    semgrad (pass_semantic_gradients): the geometry feature that feeds mlp_semantics is not detached — any of the three
    forms above through fnr_field_mlp_bwd_semgrad."""
    lib = L.load()
    fwd_mode = h_saved[3] if isinstance(h_saved, tuple) and len(h_saved) > 3 else None
    h_saved, ray_bias, packed = (tuple(h_saved) + (None, None))[:3] if isinstance(h_saved, tuple) else (h_saved, None, None)
    if fwd_mode is not None and fwd_mode != int(net.mlp_mode):
        packed = None   # the forward ran in another arithmetic: its workspace lacks this mode's fragment images — repack
    dev = rays.device
    N = rays.n * S
    d_feats = _empty(*feats.shape, device=dev)
    nbytes = lib.fnr_field_mlp_bwd_workspace_bytes(rays.n, S)
    ws = _empty(nbytes, dtype=torch.uint8, device=dev)
    d_pos = _empty(N, 4, device=dev) if jacobian is not None else None
    adam, grad_arena = weight_adam if weight_adam is not None else (None, None)
    # every export takes the same arguments, in this order; `position` and `optimiser` only where its form has them
    common = (C.byref(net), C.byref(grads), rays.ref, S, L.ptr(feats), L.ptr(h_saved), L.ptr(ray_bias), L.ptr(packed),
              L.ptr(selector), L.ptr(d_density), L.ptr(d_rgb), L.ptr(d_logit), L.ptr(d_feats))
    position = (L.ptr(jacobian), L.ptr(d_pos))
    optimiser = (None if adam is None else C.byref(adam), L.ptr(grad_arena))
    workspace = (L.ptr(ws), nbytes, L.stream_ptr(dev))
    if semgrad:
        name, args = "field_mlp_bwd_semgrad", common + position + optimiser + workspace
    elif weight_adam is not None:
        name, args = "field_mlp_bwd_adam", common + position + optimiser + workspace
    elif jacobian is not None:
        name, args = "field_mlp_bwd_rays", common + position + workspace
    else:
        name, args = "field_mlp_bwd", common + workspace
    L.check(getattr(lib, "fnr_" + name)(*args), name)
    return (d_feats, d_pos) if jacobian is not None else d_feats


class _WorkspaceCache:
    """Persistent scatter workspaces, keyed by (device, stream, size, entry point): LRU, at most `per_tag` buffers per
    (device, entry point).  A training loop uses one key per entry point for its whole life; a process that builds many
    models in sequence (each with its own second stream out of torch's pool of 32) would otherwise keep up to 32 x the
    multi-GB queues alive.  Evicting is always safe: the buffer is only dropped from the cache (a caller that comes back
    for it allocates a new one and says workspace_clean = 0)."""

    def __init__(self, per_tag: int = 2):
        self.per_tag = per_tag
        self.entries = {}          # key -> buffer; dict order = recency (oldest first)
        self.fresh = 0             # buffers made so far (a call that got a fresh one was told workspace_clean = 0)

    def get(self, key, make):
        """-> (buffer, clean): clean = 1 when the buffer has been used by these kernels before (counters left zeroed)."""
        buf = self.entries.pop(key, None)
        if buf is not None:
            self.entries[key] = buf
            return buf, 1
        same = [k for k in self.entries if (k[0], k[1], k[4]) == (key[0], key[1], key[4])]
        for k in same[:max(0, len(same) - self.per_tag + 1)]:
            del self.entries[k]
        buf = self.entries[key] = make()
        self.fresh += 1
        return buf, 0

    # dict-like views for diagnostics
    def items(self):
        return self.entries.items()

    def __len__(self):
        return len(self.entries)

    def clear(self):
        self.entries.clear()


_SCATTER_WS = _WorkspaceCache()


# FNR_SCATTER_MEMSET=1 (hunt switch): never tell the library that the counters were left clean — every
# scatter call then zeroes its counter block with a hipMemsetAsync ahead of the emit kernel instead of relying on the
# previous call's accumulate kernel having put them back to zero (~3 us per call).
SCATTER_MEMSET_EVERY_CALL = os.environ.get("FNR_SCATTER_MEMSET") == "1"


def _scatter_workspace(dev, nbytes: int, tag: str):
    """Persistent scatter workspace per (device, stream, size, entry point) -> (buffer, clean flag).  The kernels leave
    the queue counters zeroed, so after its first use the buffer needs no memset launch (workspace_clean = 1)."""
    key = (dev.type, dev.index, L.stream_ptr(dev), nbytes, tag)
    buf, clean = _SCATTER_WS.get(key, lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
    return buf, (0 if SCATTER_MEMSET_EVERY_CALL else clean)


def fresh_workspaces() -> int:
    """How many scatter workspaces have been created so far: a step during which this moved ran a scatter with
    workspace_clean = 0 (its memset launch is not part of the steady-state sequence a step program should hold)."""
    return _SCATTER_WS.fresh


def _forget_scatter_workspaces(dev) -> None:
    """A scatter entry point failed: its launches may have been enqueued in part (emit without accumulate), which leaves
    queue counters that the next call — told workspace_clean = 1 — would add to.  Drop every cached workspace of the
    device; the next calls allocate new ones and zero their counters."""
    for k in [k for k, _ in _SCATTER_WS.items() if (k[0], k[1]) == (dev.type, dev.index)]:
        del _SCATTER_WS.entries[k]


def _scatter_check(rc: int, what: str, dev) -> None:
    if rc != 0:
        _forget_scatter_workspaces(dev)
    L.check(rc, what)


def hash_encode_bwd(grid_grad: L.fnr_grid, warp: L.fnr_warp, rays: RaysArg, euclid: Tensor, S: int,
                    d_feats: Tensor, level_begin: int = 0, level_count: Optional[int] = None) -> None:
    """Scatter the feature gradients of levels [level_begin, level_begin + level_count) (default: all) into the
    gradient table."""
    lib = L.load()
    if level_count is None:
        level_count = grid_grad.n_levels - level_begin
    nbytes = lib.fnr_hash_scatter_workspace_bytes(rays.n * S, level_count, grid_grad.log2_hashmap_size)
    ws, clean = _scatter_workspace(rays.device, nbytes, "field")
    _scatter_check(lib.fnr_hash_encode_bwd(C.byref(grid_grad), C.byref(warp), rays.ref, L.ptr(euclid), S, L.ptr(d_feats),
                                           level_begin, level_count, L.ptr(ws), nbytes, clean, L.stream_ptr(rays.device)),
                   "hash_encode_bwd", rays.device)


def hash_encode_bwd_adam(grid_grad: L.fnr_grid, warp: L.fnr_warp, rays: RaysArg, euclid: Tensor, S: int,
                         d_feats: Tensor, adam: L.fnr_table_adam) -> None:
    """hash_encode_bwd over all levels with the table's optimiser step fused into the accumulate kernel (the gradient
    table is not written; `adam` points at the table's parameter / moment slices)."""
    lib = L.load()
    nbytes = lib.fnr_hash_scatter_workspace_bytes(rays.n * S, grid_grad.n_levels, grid_grad.log2_hashmap_size)
    ws, clean = _scatter_workspace(rays.device, nbytes, "field")
    _scatter_check(lib.fnr_hash_encode_bwd_adam(C.byref(grid_grad), C.byref(warp), rays.ref, L.ptr(euclid), S, L.ptr(d_feats),
                                                L.ptr(ws), nbytes, clean, C.byref(adam), L.stream_ptr(rays.device)),
                   "hash_encode_bwd_adam", rays.device)


def _prop_bwd_buffers(net: L.fnr_prop_net, rays: RaysArg, S: int, want_position_grad: bool, tag: str):
    """One proposal level's backward -> (workspace, its size, clean flag, d_position [N,4] | None)."""
    nbytes = L.load().fnr_prop_density_bwd_workspace_bytes(rays.n * S, net.grid.n_levels, net.grid.log2_hashmap_size)
    ws, clean = _scatter_workspace(rays.device, nbytes, tag)
    return ws, nbytes, clean, (_empty(rays.n * S, 4, device=rays.device) if want_position_grad else None)


def prop_density_bwd(net: L.fnr_prop_net, grads: L.fnr_prop_net, warp: L.fnr_warp, rays: RaysArg, euclid: Tensor,
                     S: int, feats: Tensor, d_density: Tensor, want_position_grad: bool = False,
                     adam=None) -> Optional[Tensor]:
    """want_position_grad: also return d(loss)/d(unit-cube position) [N,4] for position_grad_reduce(n_levels=1).
    adam = (table fnr_table_adam, weight fnr_table_adam, gradient arena): the network's optimiser step is taken by the
    kernels that finish its gradients (fnr_prop_density_bwd_adam)."""
    lib = L.load()
    ws, nbytes, clean, d_pos = _prop_bwd_buffers(net, rays, S, want_position_grad, "prop")
    head = (C.byref(net), C.byref(grads), C.byref(warp), rays.ref, L.ptr(euclid), S, L.ptr(feats), L.ptr(d_density), L.ptr(d_pos))
    tail = (L.ptr(ws), nbytes, clean, L.stream_ptr(rays.device))
    if adam is not None:
        t_adam, w_adam, grad_arena = adam
        _scatter_check(lib.fnr_prop_density_bwd_adam(*head, C.byref(t_adam), C.byref(w_adam), L.ptr(grad_arena), *tail),
                       "prop_density_bwd_adam", rays.device)
    else:
        _scatter_check(lib.fnr_prop_density_bwd(*head, *tail), "prop_density_bwd", rays.device)
    return d_pos


def prop_density_bwd_pair(nets, grads, warps, rays: RaysArg, euclids, S, feats, d_density, want_position_grad: bool = False,
                          adam=None, position_ready=None):
    """fnr_prop_density_bwd_pair: both proposal levels of a step (lists of two), their accumulate launches as one.
    adam = ([table fnr_table_adam x 2], weight fnr_table_adam, gradient arena) or None.  -> [d_position | None] x 2.
    position_ready (Event): fnr_prop_density_bwd_pair_split — both MLP backwards first, the event recorded on
    the current stream once the d_position tensors are final, then the scatter."""
    lib = L.load()
    dev = rays.device
    ws, nbytes, clean, d_pos = zip(*[_prop_bwd_buffers(nets[q], rays, S[q], want_position_grad, f"prop{q}") for q in range(2)])
    PN, PW, PT = C.POINTER(L.fnr_prop_net), C.POINTER(L.fnr_warp), C.POINTER(L.fnr_table_adam)
    vp = lambda ts: (C.c_void_p * 2)(*[L.ptr(t) for t in ts])   # noqa: E731
    t_adams = w_adam = grad_arena = None
    if adam is not None:
        t_list, w_adam_s, grad_arena = adam
        t_adams = (PT * 2)(*[C.pointer(t) for t in t_list])
        w_adam = C.byref(w_adam_s)
    args = ((PN * 2)(*[C.pointer(n) for n in nets]), (PN * 2)(*[C.pointer(g) for g in grads]),
            (PW * 2)(*[C.pointer(w) for w in warps]), rays.ref, vp(euclids), (C.c_int * 2)(*[int(x) for x in S]), vp(feats),
            vp(d_density), vp(d_pos), t_adams, w_adam, L.ptr(grad_arena), vp(ws), (C.c_size_t * 2)(*nbytes),
            (C.c_int * 2)(*clean), L.stream_ptr(dev))
    if position_ready is not None:
        _scatter_check(lib.fnr_prop_density_bwd_pair_split(*args, C.c_void_p(position_ready.handle)),
                       "prop_density_bwd_pair_split", dev)
    else:
        _scatter_check(lib.fnr_prop_density_bwd_pair(*args), "prop_density_bwd_pair", dev)
    return list(d_pos)


def hash_encode_input_grad(grid: L.fnr_grid, warp: L.fnr_warp, rays: RaysArg, euclid: Tensor, S: int,
                           d_feats: Tensor) -> Tensor:
    """Per-level gradient w.r.t. the unit-cube sample positions: [L][N][4]."""
    lib = L.load()
    partial = _empty(grid.n_levels, rays.n * S, 4, device=rays.device)
    L.check(lib.fnr_hash_encode_input_grad(C.byref(grid), C.byref(warp), rays.ref, L.ptr(euclid), S, L.ptr(d_feats),
                                           L.ptr(partial), L.stream_ptr(rays.device)), "hash_encode_input_grad")
    return partial


def position_grad_from_jacobian(warp: L.fnr_warp, rays: RaysArg, euclid: Tensor, S: int, jacobian: Tensor,
                                d_feats: Tensor, d_origins: Tensor, d_directions: Tensor) -> None:
    """d_origins / d_directions [R,3] += ray gradient of d_feats [L,N,2] through the saved Jacobian [L,3,N,2]."""
    lib = L.load()
    L.check(lib.fnr_position_grad_from_jacobian(C.byref(warp), rays.ref, L.ptr(euclid), S, jacobian.shape[0],
                                                L.ptr(jacobian), L.ptr(d_feats), L.ptr(d_origins), L.ptr(d_directions),
                                                L.stream_ptr(rays.device)), "position_grad_from_jacobian")


def position_grad_reduce_multi(sources, rays: RaysArg, d_origins: Tensor, d_directions: Tensor,
                              accumulate: bool = False) -> None:
    """One launch for several ray-gradient sources [(warp, euclid [R,S+1], S, partial [n_levels,N,4] | [N,4]), ...]:
    d_origins / d_directions [R,3] = (or +=) the sum of their ray gradients, in source order."""
    lib = L.load()
    if len(sources) > L.FNR_MAX_POSITION_SOURCES:
        # more sources than one launch takes (> 3 proposal iterations + the field): in chunks, the later ones accumulating
        m = L.FNR_MAX_POSITION_SOURCES
        for a in range(0, len(sources), m):
            position_grad_reduce_multi(sources[a:a + m], rays, d_origins, d_directions, accumulate=accumulate or a > 0)
        return
    n = len(sources)
    warps = (C.POINTER(L.fnr_warp) * n)(*[C.pointer(w) for w, _, _, _ in sources])
    euclid = (C.c_void_p * n)(*[L.ptr(e) for _, e, _, _ in sources])
    S = (C.c_int * n)(*[int(s_) for _, _, s_, _ in sources])
    levels = (C.c_int * n)(*[(p.shape[0] if p.dim() == 3 else 1) for _, _, _, p in sources])
    partials = (C.c_void_p * n)(*[L.ptr(p) for _, _, _, p in sources])
    L.check(lib.fnr_position_grad_reduce_multi(n, warps, rays.ref, euclid, S, levels, partials, 1 if accumulate else 0,
                                               L.ptr(d_origins), L.ptr(d_directions), L.stream_ptr(rays.device)),
            "position_grad_reduce_multi")


def position_grad_reduce(warp: L.fnr_warp, rays: RaysArg, euclid: Tensor, S: int, partial: Tensor, d_origins: Tensor,
                         d_directions: Tensor) -> None:
    """d_origins / d_directions [R,3] += the ray gradient carried by `partial` ([n_levels][N][4] or [N][4])."""
    lib = L.load()
    n_levels = partial.shape[0] if partial.dim() == 3 else 1
    L.check(lib.fnr_position_grad_reduce(C.byref(warp), rays.ref, L.ptr(euclid), S, n_levels, L.ptr(partial),
                                         L.ptr(d_origins), L.ptr(d_directions), L.stream_ptr(rays.device)),
            "position_grad_reduce")


def adam_step(params: Tensor, grads: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, lr: float, beta1: float,
              beta2: float, eps: float, step: int, grad_scale: float = 1.0, zero_grad: bool = True,
              weight_decay: float = 0.0) -> None:
    lib = L.load()
    L.check(lib.fnr_adam_step(L.ptr(params), L.ptr(grads), L.ptr(exp_avg), L.ptr(exp_avg_sq), params.numel(),
                              float(lr), float(beta1), float(beta2), float(eps), int(step), float(grad_scale),
                              float(weight_decay), 1 if zero_grad else 0, L.stream_ptr(params.device)), "adam_step")


def radam_step(params: Tensor, grads: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, lr: float, beta1: float,
               beta2: float, eps: float, step: int, grad_scale: float = 1.0, zero_grad: bool = True,
               weight_decay: float = 0.0) -> None:
    """torch.optim.RAdam (the optimiser of the fruit_nerf_big / fruit_nerf_huge configs) over a flat buffer."""
    lib = L.load()
    L.check(lib.fnr_radam_step(L.ptr(params), L.ptr(grads), L.ptr(exp_avg), L.ptr(exp_avg_sq), params.numel(),
                               float(lr), float(beta1), float(beta2), float(eps), int(step), float(grad_scale),
                               float(weight_decay), 1 if zero_grad else 0, L.stream_ptr(params.device)), "radam_step")


def adam_step_spans(params: Tensor, grads: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, spans, algorithm: str,
                    beta1: float, beta2: float, eps: float, grad_scale: float = 1.0, zero_grad: bool = True,
                    weight_decay: float = 0.0) -> None:
    """One launch over several spans of one arena: spans = [(offset, count, lr, step), ...] (<= FNR_MAX_ADAM_SPANS),
    each updated exactly as adam_step / radam_step would with its own learning rate and step count."""
    lib = L.load()
    arr = (L.fnr_adam_span * len(spans))(*[L.fnr_adam_span(int(a), int(n), int(step), float(lr), 0)
                                           for a, n, lr, step in spans])
    L.check(lib.fnr_adam_step_spans(L.ptr(params), L.ptr(grads), L.ptr(exp_avg), L.ptr(exp_avg_sq), len(spans), arr,
                                    0 if algorithm == "adam" else 1, float(beta1), float(beta2), float(eps),
                                    float(grad_scale), float(weight_decay), 1 if zero_grad else 0,
                                    L.stream_ptr(params.device)), "adam_step_spans")


def adam_step_spans_dev(params: Tensor, grads: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, spans, steps: Tensor,
                        algorithm: str, beta1: float, beta2: float, eps: float, scalars: Tensor,
                        grad_scale: Optional[Tensor] = None, found_inf: Optional[Tensor] = None, zero_grad: bool = True,
                        weight_decay: float = 0.0) -> None:
    """adam_step_spans without a host round trip (fnr_adam_step_spans_dev): spans = [(offset, count, lr), ...], steps =
    int64 device tensor [len(spans)] of the steps each span has taken (advanced here unless the step is skipped),
    grad_scale / found_inf = the one-element float device tensors a torch.amp.GradScaler hands an optimiser (or None),
    scalars = FNR_ADAM_DEV_SCALAR_FLOATS floats of device scratch.  Nothing here reads a device value on the host."""
    lib = L.load()
    L.require_gpu_tensor(params, "adam_step_spans_dev: params")
    for name, t in (("grads", grads), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq), ("steps", steps),
                    ("scalars", scalars), ("grad_scale", grad_scale), ("found_inf", found_inf)):
        if t is not None and t.device != params.device:
            raise RuntimeError(f"adam_step_spans_dev: {name} is on {t.device}, the parameters on {params.device}")
    if steps.dtype != torch.int64 or steps.numel() < len(spans):
        raise RuntimeError("adam_step_spans_dev: steps must hold one int64 per span")
    if scalars.dtype != torch.float32 or scalars.numel() < L.FNR_ADAM_DEV_SCALAR_FLOATS:
        raise RuntimeError(f"adam_step_spans_dev: scalars must hold {L.FNR_ADAM_DEV_SCALAR_FLOATS} floats")
    for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != 1):
            raise RuntimeError(f"adam_step_spans_dev: {name} must be a one-element float32 tensor")
    end = max((int(a) + int(n) for a, n, _ in spans), default=0)
    if end > min(params.numel(), grads.numel(), exp_avg.numel(), exp_avg_sq.numel()):
        raise RuntimeError("adam_step_spans_dev: a span ends beyond its buffers")
    arr = (L.fnr_adam_span * len(spans))(*[L.fnr_adam_span(int(a), int(n), 0, float(lr), 0) for a, n, lr in spans])
    L.check(lib.fnr_adam_step_spans_dev(L.ptr(params), L.ptr(grads), L.ptr(exp_avg), L.ptr(exp_avg_sq), len(spans), arr,
                                        L.ptr(steps), 0 if algorithm == "adam" else 1, float(beta1), float(beta2),
                                        float(eps), L.ptr(grad_scale), L.ptr(found_inf), float(weight_decay),
                                        1 if zero_grad else 0, L.ptr(scalars), L.stream_ptr(params.device)),
            "adam_step_spans_dev")


# ---- point-cloud front-end of the counting stage ------------------------------------------------------


def _cloud_args(xyz: Tensor):
    if xyz.dtype != torch.float64 or xyz.dim() != 2 or xyz.shape[1] != 3 or not xyz.is_cuda:
        raise ValueError("point clouds are [n,3] float64 device tensors (Open3D / PLY precision)")
    xyz = xyz.contiguous()
    n = xyz.shape[0]
    ws = torch.empty(L.load().fnr_cloud_workspace_bytes(n), dtype=torch.uint8, device=xyz.device)
    return xyz, n, ws


def _bounds(xyz: Tensor):
    """Host copies of the cloud's axis-aligned bounds (Open3D GetMinBound / GetMaxBound); one 48-byte D2H sync."""
    lo_hi = torch.empty(6, dtype=torch.float64, device=xyz.device)
    ws = torch.empty(64, dtype=torch.uint8, device=xyz.device)
    L.check(L.load().fnr_cloud_bounds(L.ptr(xyz), xyz.shape[0], L.ptr(lo_hi), L.ptr(ws), ws.numel(),
                                      L.stream_ptr(xyz.device)), "cloud_bounds")
    v = lo_hi.cpu().tolist()
    return (C.c_double * 3)(*v[:3]), (C.c_double * 3)(*v[3:])


def cloud_radius_count(xyz: Tensor, radius: float, inclusive: bool) -> Tensor:
    """-> int32 [n]: neighbours within radius (strict < unless inclusive), the point itself included."""
    xyz, n, ws = _cloud_args(xyz)
    counts = torch.empty(n, dtype=torch.int32, device=xyz.device)
    if n == 0:
        return counts
    lo, hi = _bounds(xyz)
    L.check(L.load().fnr_cloud_radius_count(L.ptr(xyz), n, lo, hi, float(radius), 1 if inclusive else 0, L.ptr(counts),
                                            L.ptr(ws), ws.numel(), L.stream_ptr(xyz.device)), "cloud_radius_count")
    return counts


def cloud_dbscan(xyz: Tensor, eps: float, min_samples: int):
    """-> (labels int32 [n], n_clusters int32 [1] device)."""
    xyz, n, ws = _cloud_args(xyz)
    labels = torch.empty(n, dtype=torch.int32, device=xyz.device)
    n_clusters = torch.zeros(1, dtype=torch.int32, device=xyz.device)
    if n == 0:
        return labels, n_clusters
    lo, hi = _bounds(xyz)
    L.check(L.load().fnr_cloud_dbscan(L.ptr(xyz), n, lo, hi, float(eps), int(min_samples), L.ptr(labels),
                                      L.ptr(n_clusters), L.ptr(ws), ws.numel(), L.stream_ptr(xyz.device)),
            "cloud_dbscan")
    return labels, n_clusters


def cloud_voxel_down_sample(xyz: Tensor, rgb: Optional[Tensor], voxel_size: float):
    """-> (xyz_out [m,3], rgb_out [m,3] | None), one point per occupied voxel in ascending (iz, iy, ix) order."""
    xyz, n, ws = _cloud_args(xyz)
    if rgb is not None:
        if rgb.shape != xyz.shape or rgb.dtype != torch.float64:
            raise ValueError("colours are [n,3] float64 like the points")
        rgb = rgb.contiguous()
    if n == 0:
        return xyz.clone(), (None if rgb is None else rgb.clone())
    xyz_out = torch.empty_like(xyz)
    rgb_out = None if rgb is None else torch.empty_like(rgb)
    n_out = torch.zeros(1, dtype=torch.int32, device=xyz.device)
    lo, hi = _bounds(xyz)
    L.check(L.load().fnr_cloud_voxel_down_sample(L.ptr(xyz), L.ptr(rgb), n, lo, hi, float(voxel_size), L.ptr(xyz_out),
                                                 L.ptr(rgb_out), L.ptr(n_out), L.ptr(ws), ws.numel(),
                                                 L.stream_ptr(xyz.device)), "cloud_voxel_down_sample")
    m = int(n_out.item())
    return xyz_out[:m], (None if rgb_out is None else rgb_out[:m])


def _knn_args(xyz: Tensor, k: int):
    xyz, n, _ = _cloud_args(xyz)
    ws = torch.empty(L.load().fnr_cloud_knn_workspace_bytes(n, int(k)), dtype=torch.uint8, device=xyz.device)
    return xyz, n, ws


def cloud_knn(xyz: Tensor, k: int):
    """-> (dist2 float64 [n,k], index int32 [n,k]): the k points nearest to every point (itself included), ascending by
    (squared distance, input index); with n < k the tail of a row is +inf / -1."""
    xyz, n, ws = _knn_args(xyz, k)
    dist2 = torch.empty(n, int(k), dtype=torch.float64, device=xyz.device)
    index = torch.empty(n, int(k), dtype=torch.int32, device=xyz.device)
    lo, hi = _bounds(xyz) if n else ((C.c_double * 3)(), (C.c_double * 3)())
    L.check(L.load().fnr_cloud_knn(L.ptr(xyz), n, lo, hi, int(k), L.ptr(dist2), L.ptr(index), L.ptr(ws), ws.numel(),
                                   L.stream_ptr(xyz.device)), "cloud_knn")
    return dist2, index


def cloud_statistical_outlier(xyz: Tensor, nb_neighbors: int, std_ratio: float):
    """Open3D RemoveStatisticalOutliers -> (avg_distance float64 [n], keep bool [n], stats float64 [3] = mean, std,
    threshold; all on the device)."""
    xyz, n, ws = _knn_args(xyz, nb_neighbors)
    avg = torch.empty(n, dtype=torch.float64, device=xyz.device)
    keep = torch.empty(n, dtype=torch.uint8, device=xyz.device)
    stats = torch.zeros(3, dtype=torch.float64, device=xyz.device)
    lo, hi = _bounds(xyz) if n else ((C.c_double * 3)(), (C.c_double * 3)())
    L.check(L.load().fnr_cloud_statistical_outlier(L.ptr(xyz), n, lo, hi, int(nb_neighbors), float(std_ratio),
                                                   L.ptr(avg), L.ptr(keep), L.ptr(stats), L.ptr(ws), ws.numel(),
                                                   L.stream_ptr(xyz.device)), "cloud_statistical_outlier")
    return avg, keep.bool(), stats


def cloud_estimate_normals(xyz: Tensor, knn: int) -> Tensor:
    """Open3D EstimateNormals(KDTreeSearchParamKNN(knn)) -> float64 [n,3] unit normals (sign not oriented)."""
    xyz, n, ws = _knn_args(xyz, knn)
    normals = torch.empty(n, 3, dtype=torch.float64, device=xyz.device)
    lo, hi = _bounds(xyz) if n else ((C.c_double * 3)(), (C.c_double * 3)())
    L.check(L.load().fnr_cloud_estimate_normals(L.ptr(xyz), n, lo, hi, int(knn), L.ptr(normals), L.ptr(ws), ws.numel(),
                                                L.stream_ptr(xyz.device)), "cloud_estimate_normals")
    return normals


def _fit_points(t: Tensor, name: str) -> Tensor:
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 3 or not t.is_cuda:
        raise ValueError(f"{name}: point sets are [n,3] float64 device tensors")
    return t.contiguous()


def _host_ints(values, ctype):
    values = [int(v) for v in values]
    return (ctype * max(len(values), 1))(*values), values


def cloud_icp(tgt_xyz: Tensor, tgt_offsets, src_xyz: Tensor, src_offsets, src_id, init: Tensor,
              max_correspondence_distance: float, with_scaling: bool = True, max_iteration: int = 30,
              relative_fitness: float = 1e-6, relative_rmse: float = 1e-6):
    """shapes.registration_icp for B problems in one launch: problem b registers source segment src_id[b] of src_xyz
    (segments src_offsets[s] .. src_offsets[s+1]) onto target segment b of tgt_xyz (tgt_offsets, B + 1 entries); the
    offsets and ids are host sequences, init is [B,4,4] float64 on the device.
    -> (transformation [B,4,4], fitness [B], inlier_rmse [B], iterations int32 [B], correspondences int32 [sum of the
    problems' source sizes], corr_offsets: list of B + 1 ints); all tensors on the device."""
    tgt_xyz, src_xyz = _fit_points(tgt_xyz, "cloud_icp target"), _fit_points(src_xyz, "cloud_icp source")
    dev = tgt_xyz.device
    t_off, t_list = _host_ints(tgt_offsets, C.c_int64)
    s_off, s_list = _host_ints(src_offsets, C.c_int64)
    ids, id_list = _host_ints(src_id, C.c_int32)
    B, S = len(t_list) - 1, len(s_list) - 1
    if B < 0 or S < 0 or len(id_list) != B:
        raise ValueError("cloud_icp: tgt_offsets has B + 1 entries, src_id B, src_offsets at least one")
    if init.dtype != torch.float64 or init.numel() != 16 * B or init.device != dev:
        raise ValueError("cloud_icp: init is [B,4,4] float64 on the points' device")
    init = init.contiguous()
    corr_offsets = [0]
    for s in id_list:
        if not 0 <= s < S:
            raise ValueError(f"cloud_icp: src_id {s} outside 0 .. {S - 1}")
        corr_offsets.append(corr_offsets[-1] + max(s_list[s + 1] - s_list[s], 0))
    T = torch.empty(B, 4, 4, dtype=torch.float64, device=dev)
    fitness = torch.empty(B, dtype=torch.float64, device=dev)
    rmse = torch.empty(B, dtype=torch.float64, device=dev)
    iterations = torch.empty(B, dtype=torch.int32, device=dev)
    corr = torch.empty(corr_offsets[-1], dtype=torch.int32, device=dev)
    lib = L.load()
    ws = torch.empty(max(lib.fnr_cloud_icp_workspace_bytes(B), 1), dtype=torch.uint8, device=dev)
    L.check(lib.fnr_cloud_icp(L.ptr(tgt_xyz), tgt_xyz.shape[0], t_off, B, L.ptr(src_xyz), src_xyz.shape[0], s_off, S, ids,
                              L.ptr(init), float(max_correspondence_distance), 1 if with_scaling else 0,
                              int(max_iteration), float(relative_fitness), float(relative_rmse), L.ptr(T),
                              L.ptr(fitness), L.ptr(rmse), L.ptr(iterations), L.ptr(corr), L.ptr(ws), ws.numel(),
                              L.stream_ptr(dev)), "cloud_icp")
    return T, fitness, rmse, iterations, corr, corr_offsets


def cloud_hausdorff(a_xyz: Tensor, a_offsets, a_id, src_xyz: Tensor, src_offsets, src_id,
                    translations: Optional[Tensor] = None, trans_offsets=None, transforms: Optional[Tensor] = None):
    """shapes.hausdorff_distance(A_b, B_b) for B problems in one launch.  A_b: segment a_id[b] of a_xyz.  B_b: source
    segment src_id[b] placed at translations[trans_offsets[b] : trans_offsets[b+1]] ([n,3] device rows, stacked like
    np.vstack), or — for a problem without translations — moved by transforms[b] ([B,4,4] device).  Offsets and ids are
    host sequences.  -> (distances float64 [B,3] = A->B, B->A, their maximum; witnesses int32 [B,2] = the point of A and
    the point of the placed B that realise the two directed distances), on the device."""
    a_xyz, src_xyz = _fit_points(a_xyz, "cloud_hausdorff A"), _fit_points(src_xyz, "cloud_hausdorff source")
    dev = a_xyz.device
    a_off, a_list = _host_ints(a_offsets, C.c_int64)
    s_off, s_list = _host_ints(src_offsets, C.c_int64)
    aid, aid_list = _host_ints(a_id, C.c_int32)
    sid, sid_list = _host_ints(src_id, C.c_int32)
    B = len(aid_list)
    if len(sid_list) != B or not a_list or not s_list:
        raise ValueError("cloud_hausdorff: a_id and src_id have one entry per problem")
    t_off, n_trans, queries = None, 0, 0
    if trans_offsets is not None:
        t_off, t_list = _host_ints(trans_offsets, C.c_int64)
        if len(t_list) != B + 1:
            raise ValueError("cloud_hausdorff: trans_offsets has B + 1 entries")
        n_trans = t_list[-1]
    if n_trans:
        translations = _fit_points(translations, "cloud_hausdorff translations")
        if translations.shape[0] != n_trans:
            raise ValueError("cloud_hausdorff: trans_offsets do not end at the number of translations")
    if transforms is not None:
        if transforms.dtype != torch.float64 or transforms.numel() != 16 * B or transforms.device != dev:
            raise ValueError("cloud_hausdorff: transforms is [B,4,4] float64 on the points' device")
        transforms = transforms.contiguous()
    for b in range(B):
        if not (0 <= aid_list[b] < len(a_list) - 1 and 0 <= sid_list[b] < len(s_list) - 1):
            raise ValueError(f"cloud_hausdorff: problem {b} names a segment that does not exist")
        k = (t_list[b + 1] - t_list[b]) if trans_offsets is not None else 0
        queries += max(a_list[aid_list[b] + 1] - a_list[aid_list[b]], 0)
        queries += max(k, 1) * max(s_list[sid_list[b] + 1] - s_list[sid_list[b]], 0)
    dist = torch.empty(B, 3, dtype=torch.float64, device=dev)
    wit = torch.empty(B, 2, dtype=torch.int32, device=dev)
    lib = L.load()
    ws = torch.empty(max(lib.fnr_cloud_hausdorff_workspace_bytes(B, queries), 1), dtype=torch.uint8, device=dev)
    L.check(lib.fnr_cloud_hausdorff(L.ptr(a_xyz), a_xyz.shape[0], a_off, len(a_list) - 1, L.ptr(src_xyz),
                                    src_xyz.shape[0], s_off, len(s_list) - 1, B, aid, sid,
                                    L.ptr(translations) if n_trans else None, n_trans, t_off, L.ptr(transforms),
                                    L.ptr(dist), L.ptr(wit), L.ptr(ws), ws.numel(), L.stream_ptr(dev)),
            "cloud_hausdorff")
    return dist, wit


# ---- eval-image metrics ------------------------------------------------------------------------------


_GAUSS11 = None


def ssim_window() -> "C.Array":
    """The 11 float32 weights of torchmetrics' default SSIM window (gaussian, sigma 1.5), evaluated with torch on the
    host exactly as torchmetrics.functional.image.helper._gaussian does (arange((1 - k) / 2, (1 + k) / 2), exp, / sum)."""
    global _GAUSS11
    if _GAUSS11 is None:
        dist = torch.arange((1 - 11) / 2, (1 + 11) / 2, 1, dtype=torch.float32)
        g = torch.exp(-torch.pow(dist / 1.5, 2) / 2)
        _GAUSS11 = (C.c_float * 11)(*(g / g.sum()).tolist())
    return _GAUSS11


def image_metrics(rgb: Tensor, image: Tensor, semantics: Optional[Tensor] = None, mask: Optional[Tensor] = None) -> Tensor:
    """fnr_image_metrics on [H,W,3] images (+ [H,W] logits / mask) -> 8 doubles on the device (see the header)."""
    lib = L.load()
    L.require_gpu_tensor(rgb, "rgb")
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    rgb, image = _f32c(rgb), _f32c(image)
    sem = None if semantics is None else _f32c(semantics.reshape(H, W))
    msk = None if mask is None else _f32c(mask.reshape(H, W))
    out = torch.empty(8, dtype=torch.float64, device=rgb.device)
    nbytes = lib.fnr_image_metrics_workspace_bytes(H, W)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=rgb.device)
    L.check(lib.fnr_image_metrics(H, W, L.ptr(rgb), L.ptr(image), L.ptr(sem), L.ptr(msk), ssim_window(), L.ptr(out),
                                  L.ptr(ws), ws.numel(), L.stream_ptr(rgb.device)), "image_metrics")
    return out


# ---- caller side -------------------------------------------------------------------------------------


class ImageSetArg:
    """fnr_image_set over the on-device image batch (uint8 images [M,H,W,3], uint8 masks [M,H,W], c2w [M,3,4])."""

    def __init__(self, images: Tensor, masks: Tensor, c2w: Tensor, fx: float, fy: float, cx: float, cy: float):
        L.require_gpu_tensor(images, "images")
        assert images.dtype == torch.uint8 and masks.dtype == torch.uint8
        self.images, self.masks, self.c2w = images.contiguous(), masks.contiguous(), _f32c(c2w)
        M, H, W, _ = images.shape
        self.c = L.fnr_image_set(M, H, W, L.ptr(self.images), L.ptr(self.masks), L.ptr(self.c2w), float(fx), float(fy),
                                 float(cx), float(cy))


class CameraTableArg:
    """fnr_camera_table: per-image intrinsics [M,4] (fx, fy, cx, cy) and optional OpenCV distortion [M,6] (k1, k2, k3, k4,
    p1, p2 — nerfstudio's distortion_params order), rows indexed by dataset image like c2w.  Selects the _cams entry
    points wherever an image set is passed (the set's own fx..cy are then ignored)."""

    def __init__(self, intrinsics: Tensor, distortion: Optional[Tensor] = None):
        L.require_gpu_tensor(intrinsics, "intrinsics")
        assert intrinsics.dim() == 2 and intrinsics.shape[1] == 4, "intrinsics is [M,4] (fx, fy, cx, cy)"
        self.intrinsics = _f32c(intrinsics)
        self.distortion = None
        if distortion is not None:
            assert distortion.shape == (intrinsics.shape[0], 6), "distortion is [M,6] (k1, k2, k3, k4, p1, p2)"
            self.distortion = _f32c(distortion.to(intrinsics.device))
        self.c = L.fnr_camera_table(self.intrinsics.data_ptr(),
                                    None if self.distortion is None else self.distortion.data_ptr())

    def pointers(self) -> tuple:
        return (self.intrinsics.data_ptr(), None if self.distortion is None else self.distortion.data_ptr())

    def ref(self, image_set: "ImageSetArg"):
        """byref() of the struct for a call next to `image_set`: the kernels index the rows by dataset image."""
        if self.intrinsics.shape[0] != image_set.c.n_images:
            raise ValueError(f"camera table of {self.intrinsics.shape[0]} rows for an image set of {image_set.c.n_images}")
        return C.byref(self.c)


def _camera_entry(op: str, image_set: ImageSetArg, cams: Optional[CameraTableArg], pose_mode: int, per_edge: bool = False):
    """The entry point of `op` for a configuration -> (call, options): `call(*args)` runs it and raises on failure,
    `options` are the arguments the chosen form takes for the table and the mode (after the image set, where there is one).
    fnr_<op>_edges iff per_edge; else fnr_<op>_mode iff the mode is not SO3xR3; else fnr_<op>_cams iff a table is given; else
    fnr_<op>.  The _mode and _edges forms take a nullable table."""
    table = None if cams is None else cams.ref(image_set)
    if per_edge:
        name, options = op + "_edges", (table, pose_mode)
    elif pose_mode != L.FNR_POSE_SO3XR3:
        name, options = op + "_mode", (table, pose_mode)
    elif cams is None:
        name, options = op, ()
    else:
        name, options = op + "_cams", (table,)
    fn = getattr(L.load(), "fnr_" + name)
    return (lambda *args: L.check(fn(*args), name)), options


def _ray_outputs(R: int, dev) -> dict:
    """The per-ray outputs of pixel sampling: origins, directions, camera index, target colour, fruit mask."""
    return {"origins": _empty(R, 3, device=dev), "directions": _empty(R, 3, device=dev),
            "cam": _empty(R, dtype=torch.int32, device=dev), "image": _empty(R, 3, device=dev), "mask": _empty(R, device=dev)}


def camera_adjust(image_set: ImageSetArg, train_ids: Tensor, pose_adjustment: Tensor,
                  pose_mode: int = L.FNR_POSE_SO3XR3) -> Tensor:
    """c2w' [n_train,3,4] = multiply(c2w[train_ids], exp_map(pose_adjustment)), the exponential map of pose_mode
    (L.FNR_POSE_SO3XR3 | L.FNR_POSE_SE3; anything but SO3xR3 goes through the fnr_*_mode entry points)."""
    call, options = _camera_entry("camera_adjust", image_set, None, pose_mode)
    ids = train_ids.to(torch.int64).contiguous()
    out = torch.empty(ids.numel(), 3, 4, device=pose_adjustment.device)
    call(L.ptr(image_set.c2w), L.ptr(ids), ids.numel(), L.ptr(_f32c(pose_adjustment)), *options[1:], L.ptr(out),
         L.stream_ptr(out.device))       # (no table here: of the options only the mode)
    return out


def camera_pose_grad(image_set: ImageSetArg, train_ids: Tensor, u: Tensor, cam: Tensor, pose_adjustment: Tensor,
                     c2w_adjusted: Tensor, d_origins: Tensor, d_directions: Tensor, pose_grad: Tensor,
                     cams: Optional[CameraTableArg] = None, pose_mode: int = L.FNR_POSE_SO3XR3) -> None:
    """pose_grad [n_train,6] += d(loss)/d(pose_adjustment) from the ray gradients of the rays drawn with `u`
    (cams: through that camera table, fnr_camera_pose_grad_cams; pose_mode: the exponential map the cameras were
    adjusted with)."""
    call, options = _camera_entry("camera_pose_grad", image_set, cams, pose_mode)
    ids = train_ids.to(torch.int64).contiguous()
    call(C.byref(image_set.c), *options, L.ptr(ids), ids.numel(), u.shape[0], L.ptr(_f32c(u)), L.ptr(cam),
         L.ptr(_f32c(pose_adjustment)), L.ptr(c2w_adjusted), L.ptr(d_origins), L.ptr(d_directions), L.ptr(pose_grad),
         L.stream_ptr(u.device))


def camera_pose_grad_adam(image_set: ImageSetArg, train_ids: Tensor, u: Tensor, cam: Tensor, c2w_adjusted: Tensor,
                          d_origins: Tensor, d_directions: Tensor, pose_grad: Tensor, adam: L.fnr_table_adam,
                          cams: Optional[CameraTableArg] = None, pose_mode: int = L.FNR_POSE_SO3XR3) -> None:
    """camera_pose_grad + the pose table's Adam / RAdam step (adam.params = pose_adjustment) in one launch; pose_grad
    is consumed and left zero."""
    call, options = _camera_entry("camera_pose_grad_adam", image_set, cams, pose_mode)
    ids = train_ids.to(torch.int64).contiguous()
    call(C.byref(image_set.c), *options, L.ptr(ids), ids.numel(), u.shape[0], L.ptr(_f32c(u)), L.ptr(cam), L.ptr(c2w_adjusted),
         L.ptr(d_origins), L.ptr(d_directions), L.ptr(pose_grad), C.byref(adam), L.stream_ptr(u.device))


def train_prologue(image_set: ImageSetArg, train_ids: Tensor, n_rays: int, seed: int, offset: int,
                   pose_adjustment: Optional[Tensor], near: float, far: float, S0: int, n_jitter: int = 3,
                   spacing_kind: int = 1, cams: Optional[CameraTableArg] = None,
                   pose_mode: int = L.FNR_POSE_SO3XR3, per_edge: bool = False) -> dict:
    """fnr_train_prologue: random numbers + camera adjust + pixel sampling + level-0 spaced sampling in one launch
    (cams: rays through that camera table, fnr_train_prologue_cams; pose_mode: the exponential map of pose_adjustment;
    per_edge: one jitter per level-0 bin edge drawn in the kernel, fnr_train_prologue_edges — no "jitter" rows)."""
    call, options = _camera_entry("train_prologue", image_set, cams, pose_mode, per_edge)
    dev = image_set.images.device
    R = int(n_rays)
    ids = train_ids.to(torch.int64).contiguous()
    n_train = ids.numel()
    out = {
        "u": _empty(R, 3, device=dev), "jitter": None if per_edge else _empty(n_jitter, R, device=dev),
        **_ray_outputs(R, dev), "spacing": _empty(R, S0 + 1, device=dev), "euclid": _empty(R, S0 + 1, device=dev),
        "c2w_adjusted": _empty(n_train, 3, 4, device=dev) if pose_adjustment is not None else None,
        "S0": S0, "near": float(near), "far": float(far), "spacing_kind": spacing_kind,
    }
    base = host_linspace(0.0, 1.0, S0 + 1, dev)
    jitter = () if per_edge else (L.ptr(out["jitter"]), n_jitter)      # the per-edge form has neither argument
    call(C.byref(image_set.c), *options, L.ptr(ids), n_train, R, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
         L.ptr(_f32c(pose_adjustment)) if pose_adjustment is not None else None, L.ptr(out["c2w_adjusted"]), L.ptr(out["u"]),
         *jitter, L.ptr(out["origins"]), L.ptr(out["directions"]), L.ptr(out["cam"]), L.ptr(out["image"]), L.ptr(out["mask"]),
         float(near), float(far), spacing_kind, S0, L.ptr(base), L.ptr(out["spacing"]), L.ptr(out["euclid"]), L.stream_ptr(dev))
    return out


def sample_pixels(image_set: ImageSetArg, train_ids: Tensor, u: Tensor, c2w_adjusted: Optional[Tensor] = None,
                  cams: Optional[CameraTableArg] = None):
    call, options = _camera_entry("sample_pixels", image_set, cams, L.FNR_POSE_SO3XR3)
    dev = u.device
    R = u.shape[0]
    ids = train_ids.to(torch.int64).contiguous()
    out = _ray_outputs(R, dev)
    call(C.byref(image_set.c), *options, L.ptr(ids), ids.numel(), R, L.ptr(_f32c(u)), L.ptr(c2w_adjusted), *map(L.ptr, out.values()),
         L.stream_ptr(dev))
    return tuple(out.values())


def camera_rays(c2w: Tensor, intrinsics_row: Tensor, distortion_row: Optional[Tensor], H: int, W: int, y0: int = 0,
                y1: Optional[int] = None):
    """fnr_camera_rays: origins / directions [(y1 - y0) * W, 3] of the pixel rows [y0, y1) of ONE camera (c2w [3,4],
    its intrinsics row [4] and distortion row [6] or None), row-major."""
    lib = L.load()
    L.require_gpu_tensor(c2w, "c2w")
    dev = c2w.device
    y1 = int(H) if y1 is None else int(y1)
    n = max(y1 - int(y0), 0) * int(W)
    origins = _empty(n, 3, device=dev)
    directions = _empty(n, 3, device=dev)
    dist = None if distortion_row is None else _f32c(distortion_row.to(dev))
    L.check(lib.fnr_camera_rays(L.ptr(_f32c(c2w)), L.ptr(_f32c(intrinsics_row.to(dev))), L.ptr(dist), int(H), int(W),
                                int(y0), y1, L.ptr(origins), L.ptr(directions), L.stream_ptr(dev)), "camera_rays")
    return origins, directions
