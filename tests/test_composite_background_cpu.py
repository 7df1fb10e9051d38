"""CPU: background_color and use_gradient_scaling (Nerfacto's switches, fruit_nerf.py:164, 280-281, 322-323) as far as they
go without a device — the model takes them, the `_opt` compositing entry points and the random-background generator are
declared and check their arguments on the host, the options struct has the header's layout, and the float64 references the
GPU tests hold the kernels to (tests/composite_background_reference.py) are pinned: the compositing reference on
oracle/ns_torch.py for the one background the oracle has, the Philox reference on the Random123 known-answer vectors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import ns_torch as ns
from tests import composite_background_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fnr_composite_fwd_opt", "fnr_composite_bwd_opt", "fnr_composite_bwd_targets_opt",
       "fnr_composite_fwd_bwd_targets_opt", "fnr_random_background")


@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("color", ["last_sample", "white", "black", "random"])
def test_model_constructs_with_every_background_and_gradient_scaling(color, scaling):
    from fruitnerf_amd.data.semantics import apple_metadata
    from fruitnerf_amd.fruit_nerf import FruitModel, FruitNerfModelConfig
    cfg = FruitNerfModelConfig(background_color=color, use_gradient_scaling=scaling, log2_hashmap_size=4)
    model = FruitModel(cfg, apple_metadata(), num_train_data=1, device="cpu")
    assert model.config.background_color == color and model.config.use_gradient_scaling is scaling
    model.train()
    spec = model.level0_spec()
    assert spec["random_background"] is (color == "random")


def test_unknown_background_is_a_value_error():
    from fruitnerf_amd.data.semantics import apple_metadata
    from fruitnerf_amd.fruit_nerf import FruitModel, FruitNerfModelConfig
    with pytest.raises(ValueError, match="purple"):
        FruitModel(FruitNerfModelConfig(background_color="purple", log2_hashmap_size=4), apple_metadata(), num_train_data=1,
                   device="cpu")


def test_new_entry_points_are_exported_with_signatures_and_abi_13():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    assert lib.fnr_abi_version() == L.ABI_VERSION == 13
    for name in NEW:
        assert name in L.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    # the options forms take their parents' arguments + the options (+ the per-sample logits where the parent has none)
    assert len(lib.fnr_composite_fwd_opt.argtypes) == len(lib.fnr_composite_fwd.argtypes) + 1
    assert len(lib.fnr_composite_bwd_opt.argtypes) == len(lib.fnr_composite_bwd_semgrad.argtypes) + 1
    assert len(lib.fnr_composite_bwd_targets_opt.argtypes) == len(lib.fnr_composite_bwd_targets_semgrad.argtypes) + 1
    assert len(lib.fnr_composite_fwd_bwd_targets_opt.argtypes) == len(lib.fnr_composite_fwd_bwd_targets.argtypes) + 1


_C_TYPES = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
            "int": C.c_int}


def test_options_struct_has_the_layout_of_the_header():
    """fnr_composite_options of _lib.py against the struct include/fruitnerf_hip.h declares, field by field: the header's
    members are turned into a ctypes structure of their own (C layout rules) and sizes, names and offsets compared."""
    from fruitnerf_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fruitnerf_hip.h")).read()
    body = re.search(r"typedef struct fnr_composite_options \{(.*?)\} fnr_composite_options;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)", decl)
        assert m, decl
        fields.append((m.group(3), C.c_void_p if m.group(2) else _C_TYPES[m.group(1)]))

    class Header(C.Structure):
        _fields_ = fields
    assert [n for n, _ in fields] == [f[0] for f in L.fnr_composite_options._fields_]
    assert C.sizeof(L.fnr_composite_options) == C.sizeof(Header) == 24
    for name, _ in fields:
        assert getattr(L.fnr_composite_options, name).offset == getattr(Header, name).offset, name
    for name in ("FNR_BACKGROUND_LAST_SAMPLE", "FNR_BACKGROUND_EXPLICIT"):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == getattr(L, name)


def test_options_entry_points_reject_invalid_arguments_without_a_gpu():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    rays = L.fnr_rays(0, None, None, None, None, None)
    one = C.c_void_p(64)      # a non-null pointer that is never dereferenced: every call below fails its host checks
    white = L.fnr_composite_options(L.FNR_BACKGROUND_EXPLICIT, 0, 64, 0, 0)
    for bad in (L.fnr_composite_options(2, 0, 64, 0, 0),                                   # unknown background
                L.fnr_composite_options(L.FNR_BACKGROUND_EXPLICIT, 0, None, 0, 0),         # explicit without a buffer
                L.fnr_composite_options(L.FNR_BACKGROUND_EXPLICIT, 4, 64, 0, 0)):          # row stride neither 0 nor 3
        rc = lib.fnr_composite_fwd_opt(C.byref(rays), 16, one, one, one, one, 1, C.byref(bad), one, one, one, one, one, None,
                                       None)
        assert rc == -1 and b"composite_fwd_opt" in lib.fnr_last_error() and b"background" in lib.fnr_last_error()
        rc = lib.fnr_composite_bwd_opt(C.byref(rays), 16, one, one, one, one, one, one, one, C.byref(bad), one, one, one, None)
        assert rc == -1 and b"composite_bwd_opt" in lib.fnr_last_error()
    rc = lib.fnr_composite_fwd_opt(C.byref(rays), 16, one, one, one, one, 1, None, one, one, one, one, one, None, None)
    assert rc == -1 and b"options" in lib.fnr_last_error()
    rc = lib.fnr_composite_fwd_opt(C.byref(rays), 513, one, one, one, one, 1, C.byref(white), one, one, one, one, one, None,
                                   None)
    assert rc == -1 and b"out of range" in lib.fnr_last_error()
    sem = L.fnr_composite_options(L.FNR_BACKGROUND_EXPLICIT, 3, 64, 1, 1)
    rc = lib.fnr_composite_bwd_targets_opt(C.byref(rays), 16, one, one, one, None, one, one, one, one, one, 1.0, C.byref(sem),
                                           one, one, one, None)
    assert rc == -1 and b"composite_bwd_targets_opt: null" in lib.fnr_last_error()       # semantic gradients without logits
    rc = lib.fnr_composite_fwd_bwd_targets_opt(C.byref(rays), 16, one, one, one, one, one, None, 1.0, C.byref(white), one, one,
                                               one, one, one, None, one, one, one, None)
    assert rc == -1 and b"composite_fwd_bwd_targets_opt: null" in lib.fnr_last_error()   # mask missing
    assert lib.fnr_random_background(1, 1, 16, None, None) == -1 and b"random_background" in lib.fnr_last_error()
    assert lib.fnr_random_background(1, 1, 0, one, None) == 0                            # no rays: nothing is launched


def test_given_gradients_form_poisons_a_recording_and_the_generator_records():
    """fnr_composite_bwd_opt is no more recordable than fnr_composite_bwd; fnr_random_background is (on zero rays: no launch)."""
    from fruitnerf_amd import _lib as L
    lib = L.load()
    prog = C.c_void_p()
    assert lib.fnr_program_create(C.byref(prog)) == 0
    try:
        rays = L.fnr_rays(0, None, None, None, None, None)
        assert lib.fnr_program_begin(prog) == 0
        lib.fnr_composite_bwd_opt(C.byref(rays), 16, None, None, None, None, None, None, None, None, None, None, None, None)
        assert lib.fnr_program_end(prog) != 0 and b"fnr_composite_bwd_opt" in lib.fnr_last_error()
        assert lib.fnr_program_begin(prog) == 0
        assert lib.fnr_random_background(3, 5, 0, C.c_void_p(64), None) == 0
        assert lib.fnr_program_end(prog) == 0 and lib.fnr_program_size(prog) == 1
        assert lib.fnr_program_op_name(prog, 0) == b"fnr_random_background"
        sc = L.fnr_step_scalars()
        sc.prologue_offset = 9
        assert lib.fnr_program_replay(prog, C.byref(sc)) == 0
    finally:
        lib.fnr_program_destroy(prog)


def _rays(R, S, seed):
    g = torch.Generator().manual_seed(seed)
    edges = torch.cumsum(torch.rand(R, S + 1, generator=g) * 0.05 + 0.01, 1)
    dens = torch.rand(R, S, generator=g) * (3.0 / (S * 0.035))
    dens[0] = 0.0
    rgb = torch.rand(R, S, 3, generator=g) * 1.4 - 0.2
    logit = torch.randn(R, S, generator=g) * 4.0
    return edges, dens, rgb, logit


@pytest.mark.parametrize("S", [1, 2, 48, 65])
@pytest.mark.parametrize("attached", [False, True])
def test_float64_reference_with_the_last_sample_is_the_oracle(S, attached):
    """The reference of the GPU tests with b = c_{S-1} (attached) against oracle/ns_torch.py — get_weights,
    render_rgb_last_sample, render_semantics and their autograd gradients, semantic weights detached or not — to 1e-12 of
    each quantity's maximum; the eval composite (nan_to_num + clamp) too."""
    R = 7
    edges, dens, rgb, logit = _rays(R, S, 100 + S)
    g = torch.Generator().manual_seed(S)
    g_rgb, g_sem = torch.randn(R, 3, generator=g), torch.randn(R, generator=g)
    got = ref.backward(edges, dens, rgb, logit, None, g_rgb=g_rgb, g_sem=g_sem, semantic_gradients=attached)
    e = edges.double()
    rs = ns.RaySamples(frustums=ns.Frustums(None, None, e[:, :-1, None], e[:, 1:, None], None),
                       deltas=(e[:, 1:] - e[:, :-1])[..., None])
    s = dens.double().requires_grad_(True)
    c = rgb.double().requires_grad_(True)
    lg = logit.double().requires_grad_(True)
    w = rs.get_weights(s[..., None])
    out = ns.render_rgb_last_sample(c, w, True)
    sem = ns.render_semantics(lg[..., None], w if attached else w.detach())[:, 0]
    ((out * g_rgb.double()).sum() + (sem * g_sem.double()).sum()).backward()
    for name, a, b in (("w", got["w"], w.detach()[..., 0]), ("out", got["out"], out.detach()), ("sem", got["sem"], sem.detach()),
                       ("d_density", got["d_density"], s.grad), ("d_rgb", got["d_rgb"], c.grad),
                       ("d_logit", got["d_logit"], lg.grad)):
        assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300), name
    bad = rgb.clone()
    bad[1, S // 2, 1] = float("nan")
    ev = ref.composite(got["w"], bad.double(), None, False)
    ev_ns = ns.render_rgb_last_sample(bad.double(), w.detach(), False)
    assert float((ev - ev_ns).abs().max()) <= 1e-12 and float(ev.min()) >= 0.0 and float(ev.max()) <= 1.0


def test_explicit_background_and_scaling_in_the_reference():
    """What the reference adds to the oracle, on its own terms: an explicit background gets the share 1 - acc and no gradient
    reaches sample S-1 through it; the empty ray composites to exactly the background; scaling multiplies the three
    gradients by clamp(m^2, 0, 1) and leaves the forward alone."""
    R, S = 6, 48
    edges, dens, rgb, logit = _rays(R, S, 3)
    g = torch.Generator().manual_seed(1)
    g_rgb, g_sem = torch.randn(R, 3, generator=g), torch.randn(R, generator=g)
    bg = torch.rand(R, 3, generator=g)
    last = ref.backward(edges, dens, rgb, logit, None, g_rgb=g_rgb, g_sem=g_sem)
    expl = ref.backward(edges, dens, rgb, logit, bg, g_rgb=g_rgb, g_sem=g_sem)
    w = expl["w"]
    acc = w.sum(1)
    assert torch.equal(expl["out"][0], bg[0].double())                        # the empty ray
    assert torch.allclose(expl["out"], (w[..., None] * rgb.double()).sum(1) + bg.double() * (1 - acc[:, None]), rtol=0, atol=1e-15)
    assert torch.allclose(expl["d_rgb"], g_rgb.double()[:, None, :] * w[..., None], rtol=0, atol=1e-15)
    share = last["d_rgb"][:, -1] - expl["d_rgb"][:, -1]
    assert torch.allclose(share, g_rgb.double() * (1 - acc[:, None]), rtol=0, atol=1e-15)
    scaled = ref.backward(edges, dens, rgb, logit, bg, g_rgb=g_rgb, g_sem=g_sem, gradient_scaling=True)
    s = ref.distance_scale64(edges)
    assert float(s.min()) < 1.0 and float(s.max()) == 1.0
    assert torch.equal(scaled["out"], expl["out"])
    for k, sk in (("d_density", s), ("d_rgb", s[..., None]), ("d_logit", s)):
        assert torch.equal(scaled[k], expl[k] * sk), k
    assert float((ref.distance_scale32(edges).double() - s).abs().max()) <= 4 * 2.0 ** -24


def test_numpy_philox_reproduces_the_random123_known_answers():
    """Random123's kat_vectors for philox4x32-10: zero counter and key, all ones, and the digits of pi."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        got = ref.philox4x32_10(np.array([counter], dtype=np.uint32), key)[0]
        assert tuple(int(x) for x in got) == want, (counter, [hex(int(x)) for x in got])
    # the step's layout: ray and offset in the counter, the word group in the top byte of its second word
    a = ref.step_randoms(seed=7, offset=3, n_rays=5, group=2)
    words = ref.philox4x32_10(np.array([[4, 2 << 24, 3, 0]], dtype=np.uint32), (7, 0))[0]
    assert a.dtype == np.float32 and a.shape == (5, 4)
    assert [float(x) for x in a[4]] == [float(np.float32(int(x) >> 8) * np.float32(2.0 ** -24)) for x in words]
    assert float(a.min()) >= 0.0 and float(a.max()) < 1.0
