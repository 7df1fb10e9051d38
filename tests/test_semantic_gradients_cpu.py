"""CPU: pass_semantic_gradients=True (fruit_nerf.py:56) as far as it goes without a device — the `_semgrad` entry points
exist, are declared, check their arguments on the host before any launch, leave the ABI version alone, and the field
builds with the switch on."""
import ctypes as C
import inspect

import pytest

SEMGRAD = ("fnr_composite_bwd_semgrad", "fnr_composite_bwd_targets_semgrad", "fnr_composite_fwd_bwd_targets_semgrad",
           "fnr_field_mlp_bwd_semgrad")


def test_semgrad_entry_points_are_declared_and_abi_is_unchanged():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    assert lib.fnr_abi_version() == 13
    src = inspect.getsource(L)
    for name in SEMGRAD:
        assert f'"{name}"' in src, f"{name} is not declared in _lib.py"
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    # the semgrad forms take their parents' arguments (+ the per-sample logits where the parent does not read them)
    assert len(lib.fnr_composite_bwd_semgrad.argtypes) == len(lib.fnr_composite_bwd.argtypes) + 1
    assert len(lib.fnr_composite_bwd_targets_semgrad.argtypes) == len(lib.fnr_composite_bwd_targets.argtypes) + 1
    assert len(lib.fnr_composite_fwd_bwd_targets_semgrad.argtypes) == len(lib.fnr_composite_fwd_bwd_targets.argtypes)
    assert len(lib.fnr_field_mlp_bwd_semgrad.argtypes) == len(lib.fnr_field_mlp_bwd_adam.argtypes)


def test_semgrad_entry_points_reject_invalid_arguments_without_a_gpu():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    rays = L.fnr_rays(0, None, None, None, None, None)
    one = C.c_void_p(64)      # a non-null pointer that is never dereferenced: every call below fails its host checks
    rc = lib.fnr_composite_bwd_semgrad(C.byref(rays), 16, one, one, one, None, one, one, one, one, one, one, None)
    assert rc == -1 and b"composite_bwd_semgrad: null" in lib.fnr_last_error()      # logit missing
    rc = lib.fnr_composite_bwd_semgrad(C.byref(rays), 513, one, one, one, one, one, one, one, one, one, one, None)
    assert rc == -1 and b"out of range" in lib.fnr_last_error()
    rc = lib.fnr_composite_bwd_targets_semgrad(None, 16, one, one, one, one, one, one, one, one, one, 1.0, one, one, one, None)
    assert rc == -1 and b"composite_bwd_targets_semgrad: null" in lib.fnr_last_error()
    rc = lib.fnr_composite_bwd_targets_semgrad(C.byref(rays), 0, one, one, one, one, one, one, one, one, one, 1.0, one, one,
                                               one, None)
    assert rc == -1 and b"out of range" in lib.fnr_last_error()
    rc = lib.fnr_composite_fwd_bwd_targets_semgrad(C.byref(rays), 16, one, one, one, one, one, None, 1.0, one, one, one, one,
                                                   one, None, one, one, one, None)
    assert rc == -1 and b"composite_fwd_bwd_targets_semgrad: null" in lib.fnr_last_error()    # mask missing
    net = L.fnr_field_net()
    adam = L.table_adam(0, 1e-2, 0.9, 0.999, 1e-8, 1, 1.0, 0.0, 1, 1, 1, None)
    args = [C.byref(net), C.byref(net), C.byref(rays), 4, one, one, None, None, None, one, one, one, one]
    # jacobian without d_position
    rc = lib.fnr_field_mlp_bwd_semgrad(*args, one, None, None, None, one, 1 << 20, None)
    assert rc == -1 and b"jacobian and d_position" in lib.fnr_last_error()
    # weight_adam without grad_arena
    rc = lib.fnr_field_mlp_bwd_semgrad(*args, None, None, C.byref(adam), None, one, 1 << 20, None)
    assert rc == -1 and b"weight_adam and grad_arena" in lib.fnr_last_error()
    # null gradients
    args[9] = None
    rc = lib.fnr_field_mlp_bwd_semgrad(*args, None, None, None, None, one, 1 << 20, None)
    assert rc == -1 and b"null" in lib.fnr_last_error()
    # a field that is not one of the built shapes
    args[9] = one
    net.grid.n_levels = 8
    rc = lib.fnr_field_mlp_bwd_semgrad(*args, None, None, None, None, one, 1 << 20, None)
    assert rc in (-1, -2)


def test_semgrad_without_fused_optimiser_poisons_a_recording():
    """Recordable only when the optimiser is fused (like fnr_field_mlp_bwd_adam); fnr_composite_bwd_semgrad never is."""
    from fruitnerf_amd import _lib as L
    lib = L.load()
    prog = C.c_void_p()
    assert lib.fnr_program_create(C.byref(prog)) == 0
    try:
        rays = L.fnr_rays(0, None, None, None, None, None)
        assert lib.fnr_program_begin(prog) == 0
        lib.fnr_composite_bwd_semgrad(C.byref(rays), 16, None, None, None, None, None, None, None, None, None, None, None)
        assert lib.fnr_program_end(prog) != 0 and b"fnr_composite_bwd_semgrad" in lib.fnr_last_error()
        assert lib.fnr_program_begin(prog) == 0
        lib.fnr_field_mlp_bwd_semgrad(None, None, None, 4, None, None, None, None, None, None, None, None, None, None, None,
                                      None, None, None, 0, None)
        assert lib.fnr_program_end(prog) != 0 and b"fnr_field_mlp_bwd_semgrad" in lib.fnr_last_error()
    finally:
        lib.fnr_program_destroy(prog)


def test_field_builds_with_the_switch_on():
    """FruitNerfModelConfig(pass_semantic_gradients=True) builds its FruitField without a device; FruitModel as a whole
    takes the switch on the HIP device and keeps the refusal tests/test_host_logic.py pins when constructed off it."""
    import torch
    from fruitnerf_amd.data.semantics import apple_metadata
    from fruitnerf_amd.fruit_field import FruitField
    from fruitnerf_amd.fruit_nerf import FruitModel, FruitNerfModelConfig
    cfg = FruitNerfModelConfig(log2_hashmap_size=4, pass_semantic_gradients=True)
    aabb = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
    for on in (False, True):
        fld = FruitField(aabb, num_images=1, num_levels=cfg.num_levels, max_res=cfg.max_res,
                         log2_hashmap_size=cfg.log2_hashmap_size, geo_feat_dim=cfg.geo_feat_dim, use_semantics=True,
                         num_semantic_classes=1, pass_semantic_gradients=cfg.pass_semantic_gradients and on)
        assert fld.pass_semantic_gradients is on
    assert "pass_semantic_gradients" in inspect.signature(FruitField.__init__).parameters
    with pytest.raises(NotImplementedError, match="HIP device"):
        FruitModel(cfg, apple_metadata(), num_train_data=1, device="cpu")


def test_per_wave_semantic_input_gradient_kernels_do_not_spill(tmp_path):
    """The kernels pass_semantic_gradients adds to the per-wave backward (namespace fnr::pw_dx: the input gradient of
    mlp_semantics, bf16 | bf16x3) meet what tests/test_isa_invariants.py::test_per_wave_backward_kernels_do_not_spill asks of
    every kernel in fnr::pw — no scratch, no spilled register, at most 256 vector registers — and the kernels of fnr::pw are
    the fourteen they were."""
    import os
    import re
    import shutil
    from tests.test_isa_invariants import HIPCC, _compile
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    text = "\n".join(_compile("field_mlp_bwd_pw.hip", tmp_path / "field_mlp_bwd_pw.s"))
    meta = re.findall(r"\.name:\s*(\S+)\s*\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s*(\d+)(?:.*\n)*?\s*\.vgpr_count:\s*(\d+)"
                      r"(?:.*\n)*?\s*\.vgpr_spill_count:\s*(\d+)", text)
    kernels = {name: (int(scratch), int(vgpr), int(spill)) for name, scratch, vgpr, spill in meta}
    assert sum(name.startswith("_ZN3fnr2pw") for name in kernels) == 14
    dx = {name: v for name, v in kernels.items() if name.startswith("_ZN3fnr5pw_dx")}
    assert len(dx) == 2 and all("k_field_mlp_sem_dx_pw" in name for name in dx), sorted(dx)
    for name, (scratch, vgpr, spill) in dx.items():
        assert scratch == 0 and spill == 0 and vgpr <= 256, (name, scratch, vgpr, spill)
