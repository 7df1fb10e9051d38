"""What the camera / pixel-sampling kernels (pixel_sampler.hip, camera_opt.hip: fnr_sample_pixels*, fnr_train_prologue*,
fnr_camera_adjust*, fnr_camera_pose_grad*, fnr_camera_pose_grad_adam*, fnr_camera_rays) compute, as bit patterns: for every
case below a SHA-256 of the raw bytes of each output array, recorded on the commit BEFORE a change that is meant to keep
every bit:

    python -m tests.golden.make_camera_family_parent_golden      # writes tests/golden/camera_family_parent_digests.json

tests/test_gpu_camera_family_same_bits.py computes the same cases on the checked-out tree and compares, exactly.

Inputs: 6 images of 5 x 7 (H x W) on make_cameras(6), train_ids = [4, 0, 3]; a pinhole for the set and a table of six distinct
rows drawn the way tests/test_gpu_camera_models.py draws its own, scaled to the image; poses from that file's _poses
(SO3xR3: one row below the angle clamp) and from test_camera_se3_cpu.pose_rows (SE3: angular norms 0, 0.012, 1.0 — the zero
row and both branches of the coefficients).  u: row 0 is exactly 1.0, row 1 the largest float below 1, row 2 exactly 0, the
rest uniform.  The pose gradient runs on a u whose first column never picks slot 1: a camera that owns no ray.

A case is (table, pose, rays) and runs every operation that configuration reaches, through the K.* wrappers:
  table: none | intrinsics only | intrinsics + distortion;   pose: none | SO3xR3 | SE3
  rays:  1;  255 (a ragged workgroup);  257 (a second workgroup; the level-0 role starts at workgroup 2);  4097 (one past
         CPG_ROUND: a pose-gradient workgroup takes a second compaction round);  0 (below)
  sample_pixels without c2w_adjusted and, with a pose, with the adjusted cameras (camera_adjust, digested too);
  train_prologue, where it accepts the ray count (no pose, or at least as many rays as cameras): S0 in {1, 5, 48} x (jitter
    per ray | per edge); n_jitter in {1, 3, 5}, the spacing kind in {0, 1} and the offset in {7, 2^32 + 5} rotate with S0 and
    the case, and the case "level 0" runs their whole product once (the level-0 role reads neither table nor pose);
  with a pose: camera_pose_grad onto a non-zero pose_grad; camera_pose_grad_adam for adam and radam (parameters, both
    moments, the zeroed pose_grad).
rays = 0 cannot go through the wrappers (an empty tensor has no address, and the entry points refuse NULL): those cases call
the entry point the wrapper would have chosen on buffers that hold a sentinel, and digest the buffers — nothing is written,
except that the fused gradient + optimiser form still takes its step.  The same holds for the empty row block of
fnr_camera_rays (cases "camera rays": all rows, rows [1, 4), rows [2, 2)).

Why the bits are reproducible: no kernel of the family uses atomics, the pose gradient compacts in ray order and sums in a
fixed tree, and no grid depends on the CU count.  Self-check: every case is computed twice here, and a digest that differs
between the two runs is not written."""
import ctypes as C
import functools
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "camera_family_parent_digests.json")
N_IMG, H, W = 6, 5, 7
TRAIN_IDS = [4, 0, 3]
PIN = (7.75, 7.25, 3.3, 2.4)             # the image set's own pinhole (fx, fy, cx, cy)
TABLES = ("no table", "table", "distorted table")
POSES = ("no pose", "SO3xR3", "SE3")
RAYS = (1, 255, 257, 4097, 0)
S0S, N_JITTERS, KINDS, OFFSETS = (1, 5, 48), (1, 3, 5), (0, 1), (7, 2 ** 32 + 5)
NEAR, FAR, SEED = 0.05, 1000.0, 1234
R_MAX = max(RAYS)
SENTINEL = -7.0


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def scene(dev):
    """The inputs of the module docstring on `dev`, drawn once from numpy.random.default_rng(0) and torch seed 11."""
    from fruitnerf_amd import _kernels as K
    from fruitnerf_amd.data import synthetic_apple as sa
    from tests.test_camera_se3_cpu import pose_rows
    from tests.test_gpu_camera_models import _poses
    rng = np.random.default_rng(0)
    n = N_IMG
    fx = rng.uniform(4.9, 12.25, n)     # (test_gpu_camera_models' 28 .. 70 for W = 40, scaled to W = 7: the same field of view)
    Kf = np.stack([fx, fx * rng.uniform(0.95, 1.05, n), W / 2.0 + rng.uniform(-0.5, 0.5, n), H / 2.0 + rng.uniform(-0.5, 0.5, n)],
                  -1).astype(np.float32)
    Df = np.stack([rng.uniform(-0.25, 0.15, n), rng.uniform(-0.05, 0.08, n), rng.uniform(-0.01, 0.01, n),
                   rng.uniform(-0.002, 0.002, n), rng.uniform(-5e-3, 5e-3, n), rng.uniform(-5e-3, 5e-3, n)], -1).astype(np.float32)
    u = rng.uniform(0, 1, (R_MAX, 3)).astype(np.float32)
    u[0], u[1], u[2] = 1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 0.0
    u_gap = u.copy()                    # slot 1 of 3 owns no ray
    middle = (u_gap[:, 0] * 3.0).astype(np.int64) == 1
    u_gap[middle, 0] *= 0.25
    images = rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    masks = rng.integers(0, 2, (n, H, W)).astype(np.uint8)
    g = torch.Generator().manual_seed(11)
    t = {"K": torch.from_numpy(Kf), "D": torch.from_numpy(Df), "u": torch.from_numpy(u), "u_gap": torch.from_numpy(u_gap),
         "images": torch.from_numpy(images), "masks": torch.from_numpy(masks), "c2w": sa.make_cameras(n, seed=0).float(),
         "Go": torch.randn(R_MAX, 3, generator=g), "Gd": torch.randn(R_MAX, 3, generator=g),
         "grad0": 0.1 * torch.randn(len(TRAIN_IDS), 6, generator=g), "m0": 1e-3 * torch.randn(len(TRAIN_IDS), 6, generator=g),
         "v0": 1e-6 * (0.1 + torch.rand(len(TRAIN_IDS), 6, generator=g)),
         "SO3xR3": _poses(len(TRAIN_IDS)), "SE3": pose_rows(8)[[0, 3, 6]].float()}
    t = {k: v.to(dev).contiguous() for k, v in t.items()}
    assert len({tuple(r) for r in Kf.tolist()}) == n and len({tuple(r) for r in Df.tolist()}) == n
    t["iset"] = K.ImageSetArg(t["images"], t["masks"], t["c2w"], *PIN)
    t["ids"] = torch.tensor(TRAIN_IDS, device=dev)
    t["tables"] = dict(zip(TABLES, (None, K.CameraTableArg(t["K"]), K.CameraTableArg(t["K"], t["D"]))))
    return t


def _mode(pose_name):
    from fruitnerf_amd import _lib as L
    return L.POSE_MODES.get(pose_name, L.FNR_POSE_SO3XR3)


def _camera_adam(t, pose_name, algorithm, dev):
    """A CameraOptimizer on the case's poses with its CameraAdam six steps in, seeded moments and gradient."""
    from fruitnerf_amd.cameras.camera_optimizers import CameraAdam, CameraOptimizerConfig
    cam = CameraOptimizerConfig(mode=pose_name).setup(len(TRAIN_IDS), dev)
    adam = CameraAdam(cam, algorithm=algorithm)
    with torch.no_grad():
        cam.pose_adjustment.copy_(t[pose_name])
    cam.pose_adjustment.grad.copy_(t["grad0"])
    adam.exp_avg.copy_(t["m0"])
    adam.exp_avg_sq.copy_(t["v0"])
    adam.step_count = 6
    return cam, adam


def _adam_digests(cam, adam):
    return {"parameters": digest(cam.pose_adjustment.data), "exp_avg": digest(adam.exp_avg), "exp_avg_sq": digest(adam.exp_avg_sq),
            "pose_grad": digest(cam.pose_adjustment.grad)}


def _prologue_digests(out):
    return {k: digest(v) for k, v in out.items() if torch.is_tensor(v)}


def _prologue_forms(shift):
    """Six calls: S0 x (per ray | per edge); n_jitter, spacing kind and offset rotate with S0 and `shift` (the case's number)."""
    for i, S0 in enumerate(S0S):
        for per_edge in (False, True):
            j = i + shift + int(per_edge)
            yield S0, per_edge, N_JITTERS[(i + shift) % 3], KINDS[j % 2], OFFSETS[(j // 2) % 2]


def _case(table, pose_name, R, shift):
    def run(dev):
        from fruitnerf_amd import _kernels as K
        if R == 0:
            return _no_rays(table, pose_name, dev)
        t = scene(dev)
        iset, ids, cams = t["iset"], t["ids"], t["tables"][table]
        pose, mode = t.get(pose_name), _mode(pose_name)
        u, u_gap, Go, Gd = t["u"][:R], t["u_gap"][:R], t["Go"][:R], t["Gd"][:R]
        names = ("origins", "directions", "cam", "image", "mask")
        out = {f"sample_pixels: {k}": digest(v) for k, v in zip(names, K.sample_pixels(iset, ids, u, None, cams=cams))}
        if pose is not None:
            adj = K.camera_adjust(iset, ids, pose, pose_mode=mode)
            out["camera_adjust"] = digest(adj)
            out.update({f"sample_pixels, adjusted: {k}": digest(v)
                        for k, v in zip(names, K.sample_pixels(iset, ids, u, adj, cams=cams))})
        if pose is None or R >= len(TRAIN_IDS):
            for S0, per_edge, n_jitter, kind, offset in _prologue_forms(shift):
                got = K.train_prologue(iset, ids, R, SEED, offset, pose, NEAR, FAR, S0, n_jitter=n_jitter, spacing_kind=kind,
                                       cams=cams, pose_mode=mode, per_edge=per_edge)
                form = f"prologue S0={S0} " + ("per edge" if per_edge else f"n_jitter={n_jitter}") + f" kind={kind} offset={offset}"
                out.update({f"{form}: {k}": v for k, v in _prologue_digests(got).items()})
        if pose is not None:
            cam_idx = K.sample_pixels(iset, ids, u_gap, adj, cams=cams)[2]
            assert R < 3 or sorted(torch.unique(cam_idx).tolist()) == [0, 2]
            grad = t["grad0"].clone()
            K.camera_pose_grad(iset, ids, u_gap, cam_idx, pose, adj, Go, Gd, grad, cams=cams, pose_mode=mode)
            out["pose_grad"] = digest(grad)
            for algorithm in ("adam", "radam"):
                cam, adam = _camera_adam(t, pose_name, algorithm, dev)
                K.camera_pose_grad_adam(iset, ids, u_gap, cam_idx, adj, Go, Gd, cam.pose_adjustment.grad, adam.fused_step_args(),
                                        cams=cams, pose_mode=mode)
                out.update({f"pose_grad_{algorithm}: {k}": v for k, v in _adam_digests(cam, adam).items()})
        torch.cuda.synchronize()
        return out
    return run


def _entry(lib, op, iset, cams, mode, per_edge=False):
    """(function, leading arguments) by the wrappers' rule: _edges if per_edge, _mode unless SO3xR3, _cams with a table."""
    from fruitnerf_amd import _lib as L
    ref = None if cams is None else cams.ref(iset)
    if per_edge:
        return getattr(lib, op + "_edges"), (C.byref(iset.c), ref, mode)
    if mode != L.FNR_POSE_SO3XR3:
        return getattr(lib, op + "_mode"), (C.byref(iset.c), ref, mode)
    if cams is None:
        return getattr(lib, op), (C.byref(iset.c),)
    return getattr(lib, op + "_cams"), (C.byref(iset.c), ref)


def _no_rays(table, pose_name, dev):
    """n_rays = 0 on sentinel-filled buffers of four rays: nothing is written; the fused Adam form still takes its step."""
    from fruitnerf_amd import _kernels as K
    from fruitnerf_amd import _lib as L
    lib = L.load()
    t = scene(dev)
    iset, ids, cams = t["iset"], t["ids"], t["tables"][table]
    pose, mode, n, stream = t.get(pose_name), _mode(pose_name), len(TRAIN_IDS), L.stream_ptr(dev)
    u = t["u"][:4].contiguous()

    def buffers(S0):
        b = {k: torch.full(shape, SENTINEL, device=dev) for k, shape in
             (("u", (4, 3)), ("jitter", (3, 4)), ("origins", (4, 3)), ("directions", (4, 3)), ("image", (4, 3)), ("mask", (4,)),
              ("spacing", (4, S0 + 1)), ("euclid", (4, S0 + 1)), ("c2w_adjusted", (n, 3, 4)))}
        b["cam"] = torch.full((4,), int(SENTINEL), dtype=torch.int32, device=dev)
        return b
    out = {}
    b = buffers(1)
    sample = (lib.fnr_sample_pixels, (C.byref(iset.c),)) if cams is None else \
        (lib.fnr_sample_pixels_cams, (C.byref(iset.c), cams.ref(iset)))
    L.check(sample[0](*sample[1], L.ptr(ids), n, 0, L.ptr(u), None, L.ptr(b["origins"]), L.ptr(b["directions"]), L.ptr(b["cam"]),
                      L.ptr(b["image"]), L.ptr(b["mask"]), stream), "sample_pixels")
    out.update({f"sample_pixels: {k}": digest(b[k]) for k in ("origins", "directions", "cam", "image", "mask")})
    if pose is None:      # (with a pose the prologue refuses fewer rays than cameras)
        S0 = 5
        base = K.host_linspace(0.0, 1.0, S0 + 1, dev)
        for per_edge in (False, True):
            b = buffers(S0)
            fn, lead = _entry(lib, "fnr_train_prologue", iset, cams, mode, per_edge)
            jitter = () if per_edge else (L.ptr(b["jitter"]), 3)
            L.check(fn(*lead, L.ptr(ids), n, 0, SEED, OFFSETS[0], None, None, L.ptr(b["u"]), *jitter, L.ptr(b["origins"]),
                       L.ptr(b["directions"]), L.ptr(b["cam"]), L.ptr(b["image"]), L.ptr(b["mask"]), NEAR, FAR, 1, S0, L.ptr(base),
                       L.ptr(b["spacing"]), L.ptr(b["euclid"]), stream), "train_prologue")
            out.update({f"prologue per_edge={per_edge}: {k}": digest(v) for k, v in b.items()})
    else:
        adj = K.camera_adjust(iset, ids, pose, pose_mode=mode)
        cam_idx = torch.zeros(4, dtype=torch.int32, device=dev)
        grad = t["grad0"].clone()
        fn, lead = _entry(lib, "fnr_camera_pose_grad", iset, cams, mode)
        L.check(fn(*lead, L.ptr(ids), n, 0, L.ptr(u), L.ptr(cam_idx), L.ptr(pose), L.ptr(adj), L.ptr(t["Go"]), L.ptr(t["Gd"]),
                   L.ptr(grad), stream), "camera_pose_grad")
        assert torch.equal(grad, t["grad0"])
        out["pose_grad"] = digest(grad)
        for algorithm in ("adam", "radam"):
            cam, adam = _camera_adam(t, pose_name, algorithm, dev)
            args = adam.fused_step_args()
            fn, lead = _entry(lib, "fnr_camera_pose_grad_adam", iset, cams, mode)
            L.check(fn(*lead, L.ptr(ids), n, 0, L.ptr(u), L.ptr(cam_idx), L.ptr(adj), L.ptr(t["Go"]), L.ptr(t["Gd"]),
                       L.ptr(cam.pose_adjustment.grad), C.byref(args), stream), "camera_pose_grad_adam")
            assert not torch.equal(cam.pose_adjustment.data, t[pose_name]) and float(cam.pose_adjustment.grad.abs().max()) == 0.0
            out.update({f"pose_grad_{algorithm}: {k}": v for k, v in _adam_digests(cam, adam).items()})
    torch.cuda.synchronize()
    return out


def _level0(dev):
    """The whole product S0 x spacing kind x offset x (n_jitter 1 | 3 | 5 | per edge) once, at 257 rays without table or pose."""
    from fruitnerf_amd import _kernels as K
    t = scene(dev)
    out = {}
    for S0, kind, offset, form in itertools.product(S0S, KINDS, OFFSETS, N_JITTERS + ("per edge",)):
        per_edge = form == "per edge"
        got = K.train_prologue(t["iset"], t["ids"], 257, SEED, offset, None, NEAR, FAR, S0, n_jitter=3 if per_edge else form,
                               spacing_kind=kind, per_edge=per_edge)
        name = f"S0={S0} kind={kind} offset={offset} " + ("per edge" if per_edge else f"n_jitter={form}")
        out.update({f"{name}: {k}": digest(got[k]) for k in ("u", "jitter", "spacing", "euclid") if got[k] is not None})
    torch.cuda.synchronize()
    return out


def _camera_rays(dev):
    from fruitnerf_amd import _kernels as K
    from fruitnerf_amd import _lib as L
    t = scene(dev)
    out = {}
    for name, D in (("pinhole", None), ("distorted", t["D"][2])):
        for y0, y1 in ((0, H), (1, 4)):
            o, d = K.camera_rays(t["c2w"][2], t["K"][2], D, H, W, y0, y1)
            out.update({f"{name} rows [{y0}, {y1}): origins": digest(o), f"{name} rows [{y0}, {y1}): directions": digest(d)})
        o, d = torch.full((4, 3), SENTINEL, device=dev), torch.full((4, 3), SENTINEL, device=dev)
        L.check(L.load().fnr_camera_rays(L.ptr(t["c2w"][2].contiguous()), L.ptr(t["K"][2].contiguous()),
                                         None if D is None else L.ptr(D.contiguous()), H, W, 2, 2, L.ptr(o), L.ptr(d),
                                         L.stream_ptr(dev)), "camera_rays")
        out.update({f"{name} rows [2, 2): origins": digest(o), f"{name} rows [2, 2): directions": digest(d)})
    torch.cuda.synchronize()
    return out


def _cases():
    c = {}
    for shift, (table, pose, R) in enumerate(itertools.product(TABLES, POSES, RAYS)):
        c[f"{table}, {pose}, {R} rays"] = _case(table, pose, R, shift)
    c["level 0"] = _level0
    c["camera rays"] = _camera_rays
    return c


CASES = _cases()


def compute(case: str, dev) -> dict:
    """One case on `dev` -> {operation: array name -> sha256}."""
    return CASES[case](dev)


def main(argv) -> int:
    out = argv[1] if len(argv) > 1 else FIXTURE
    dev = torch.device("cuda:0")
    cases = {}
    for case in CASES:
        first, second = compute(case, dev), compute(case, dev)
        differ = [k for k in first if first[k] != second[k]]
        if differ or sorted(first) != sorted(second):
            print(f"[camera family golden] {case}: not reproducible, nothing written: {differ}", flush=True)
            return 1
        cases[case] = first
        print(f"[camera family golden] {case}: {len(first)} digests, " + " ".join(v[:6] for v in list(first.values())[:8]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write('{"cases": {\n' + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in cases.items()) +
                "\n}}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
