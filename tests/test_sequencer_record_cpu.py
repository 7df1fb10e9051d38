"""seq::record (fruitnerf_amd/csrc/sequencer.hpp), the one recording hook of every recordable entry point, without a device.

Through the loaded library: every call here returns before its first HIP call — on zero rays where the entry point returns
early on them, on a failing argument check otherwise (a recording hook runs ahead of the checks, so such a call is recorded all
the same) — and the fake non-null pointers are never dereferenced.  What a replay does to lr / step / offsets / anneal / losses on
the device is tests/test_gpu_sequencer*.py's; the holders themselves are driven by tests/host/seq_record_host.cpp, built and
run here."""
import ctypes as C
import os
import subprocess

import pytest

from fruitnerf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FAKE = C.c_void_p(64)      # a device pointer that is checked for NULL and never read
HOST_STRUCTS = (L.fnr_rays, L.fnr_grid, L.fnr_warp, L.fnr_prop_net, L.fnr_field_net, L.fnr_composite_options,
                L.fnr_table_adam, L.fnr_image_set, L.fnr_camera_table)
EXPLICIT_BACKGROUND = dict(background=L.FNR_BACKGROUND_EXPLICIT, background_stride=0, background_rgb=FAKE.value)


@pytest.fixture
def program():
    lib = L.load()
    h = C.c_void_p()
    assert lib.fnr_program_create(C.byref(h)) == 0 and h.value
    yield lib, h
    assert lib.fnr_program_abort(h) == 0 and lib.fnr_program_destroy(h) == 0


def default_args(name, given=None):
    """One argument per parameter of `name`: `given[i]` where there is one, else a zeroed host struct (zero rays) for a pointer to
    one, NULL for every other pointer and 0 for a number.  Returns (args, structs): the structs keep the pointees alive."""
    given = given or {}
    args, structs = [], []
    for i, t in enumerate(L.SIGNATURES[name][1]):
        if i in given:
            value = given[i]
            if isinstance(value, C.Structure):
                structs.append(value)
                value = C.byref(value)
        elif any(t is C.POINTER(s) for s in HOST_STRUCTS):
            structs.append(t._type_())
            value = C.byref(structs[-1])
        elif t is C.c_float:
            value = 0.0
        elif t in (C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t):
            value = 0
        else:
            value = None
        args.append(value)
    return args, structs


def names(lib, h):
    return [lib.fnr_program_op_name(h, i).decode() for i in range(lib.fnr_program_size(h))]


def test_host_struct_is_kept_by_value(program):
    lib, h = program
    rays = L.fnr_rays()                                                # zero rays
    opt = L.fnr_composite_options(**EXPLICIT_BACKGROUND)
    args = [C.byref(rays), 16, FAKE, FAKE, FAKE, FAKE, 1, C.byref(opt), FAKE, FAKE, FAKE, FAKE, FAKE, None, None]
    assert lib.fnr_program_begin(h) == 0
    assert lib.fnr_composite_fwd_opt(*args) == 0
    assert lib.fnr_program_end(h) == 0 and names(lib, h) == ["fnr_composite_fwd_opt"]
    opt.background = 7
    assert lib.fnr_program_replay(h, None) == 0                        # the recorded options
    assert lib.fnr_composite_fwd_opt(*args) == -1 and b"background 7" in lib.fnr_last_error()   # the caller's


def test_adam_struct_is_patched_from_the_replays_scalars(program):
    lib, h = program
    grid = L.fnr_grid(n_levels=1)
    adam = L.table_adam(0, 1e-2, 0.9, 0.999, 1e-8, 0, 1.0, 0.1, FAKE.value, FAKE.value, FAKE.value, FAKE.value, slot=1)
    args, keep = default_args("fnr_hash_encode_bwd_adam", {0: grid, 3: FAKE, 4: 16, 5: FAKE, 9: adam})
    assert lib.fnr_program_begin(h) == 0
    assert lib.fnr_hash_encode_bwd_adam(*args) == -1 and b"step must be >= 1" in lib.fnr_last_error()
    assert lib.fnr_program_end(h) == 0 and names(lib, h) == ["fnr_hash_encode_bwd_adam"]
    sc = L.fnr_step_scalars()
    sc.adam[0].lr, sc.adam[0].step = 1e-3, 5
    # step 5 passes the check the recorded step 0 fails: the replay stops at the NEXT one
    assert lib.fnr_program_replay(h, C.byref(sc)) == -1 and b"sparse-touch skipping needs weight_decay = 0" in lib.fnr_last_error()
    assert lib.fnr_program_replay(h, None) == -1 and b"step must be >= 1" in lib.fnr_last_error()
    sc.adam[0].step = 0                                                # 0 = keep the recorded lr / step
    assert lib.fnr_program_replay(h, C.byref(sc)) == -1 and b"step must be >= 1" in lib.fnr_last_error()


@pytest.mark.parametrize("name", ["fnr_composite_fwd", "fnr_hash_encode_fwd", "fnr_prop_density_fwd"])
def test_null_host_struct_records_nothing(program, name):
    lib, h = program
    rays_at = [i for i, t in enumerate(L.SIGNATURES[name][1]) if t is C.POINTER(L.fnr_rays)]
    args, keep = default_args(name, {rays_at[0]: None})
    assert lib.fnr_program_begin(h) == 0
    assert getattr(lib, name)(*args) == -1                             # (its own check names the NULL)
    assert lib.fnr_program_size(h) == 0
    assert lib.fnr_program_end(h) == 0 and lib.fnr_program_size(h) == 0


# (entry point, arguments that are not the defaults, the name it is recorded under, its status, its message)
EXPLICIT = L.fnr_composite_options(**EXPLICIT_BACKGROUND)
RECORDED = [
    ("fnr_train_prologue", {}, None, -1, b"train_prologue: null argument"),
    ("fnr_train_prologue_cams", {}, None, -1, b"train_prologue_cams: null camera table"),
    ("fnr_train_prologue_mode", {}, None, -1, b"train_prologue_cams: null camera table"),
    ("fnr_train_prologue_edges", {}, None, -1, b"train_prologue_cams: null camera table"),
    ("fnr_random_background", {}, None, -1, b"random_background: null argument"),
    ("fnr_edge_jitter", {}, None, -1, b"edge_jitter: null argument"),
    ("fnr_prop_density_fwd", {}, None, -1, b"prop_density_fwd: null argument"),
    ("fnr_weights_pdf", {}, None, -1, b"weights_pdf: null argument"),
    ("fnr_weights_pdf_edges", {}, None, -1, b"weights_pdf: null argument"),
    ("fnr_hash_encode_fwd", {}, None, -1, b"hash_encode_fwd: null rays/bins"),
    ("fnr_field_mlp_fwd", {}, None, -1, b"field_mlp_fwd: null argument"),
    ("fnr_composite_fwd", {}, None, -1, b"composite_fwd: null argument"),
    ("fnr_composite_fwd_opt", {}, "fnr_composite_fwd", -1, b"composite_fwd: null argument"),     # the last sample: delegated
    ("fnr_composite_fwd_opt", {7: EXPLICIT}, None, -1, b"composite_fwd_opt: null argument"),
    ("fnr_train_losses", {}, None, -1, b"train_losses: null argument"),
    ("fnr_distortion_bwd", {}, None, -1, b"distortion_bwd: null argument"),
    ("fnr_composite_bwd_targets", {1: 16}, None, -1, b"composite_bwd_targets: null argument"),
    ("fnr_composite_fwd_bwd_targets", {1: 16}, None, -1, b"composite_fwd_bwd_targets: null argument"),
    ("fnr_composite_bwd_targets_semgrad", {1: 16}, None, -1, b"composite_bwd_targets_semgrad: null argument"),
    ("fnr_composite_fwd_bwd_targets_semgrad", {1: 16}, None, -1, b"composite_fwd_bwd_targets_semgrad: null argument"),
    ("fnr_composite_bwd_targets_opt", {1: 16, 12: EXPLICIT}, None, -1, b"composite_bwd_targets_opt: null argument"),
    ("fnr_composite_fwd_bwd_targets_opt", {1: 16, 9: EXPLICIT}, None, -1, b"composite_fwd_bwd_targets_opt: null argument"),
    ("fnr_composite_fwd_bwd_targets_opt", {1: 16}, "fnr_composite_fwd_bwd_targets", -1,
     b"composite_fwd_bwd_targets: null argument"),
    ("fnr_field_mlp_bwd_adam", {}, None, -1, b"field_mlp_bwd_adam: weight_adam / grad_arena missing"),
    ("fnr_field_mlp_bwd_semgrad", {}, None, -1, b"field_mlp_bwd_semgrad: weight_adam and grad_arena go together"),
    ("fnr_hash_encode_bwd_adam", {}, None, -1, b"hash_encode_bwd_adam: null argument"),
    ("fnr_prop_density_bwd_pair", {}, None, -1, b"prop_density_bwd_pair: null argument"),
    ("fnr_prop_density_bwd_pair_split", {}, None, -1, b"prop_density_bwd_pair_split: null argument"),
    ("fnr_position_grad_reduce_multi", {0: 1}, None, -1, b"position_grad_reduce_multi: bad argument"),
    ("fnr_camera_pose_grad_adam", {}, None, -1, b"camera_pose_grad_adam: null argument"),
    ("fnr_camera_pose_grad_adam_cams", {}, None, -1, b"camera_pose_grad_adam_cams: null camera table"),
    ("fnr_camera_pose_grad_adam_mode", {}, None, -1, b"camera_pose_grad_adam_cams: null camera table"),
    ("fnr_stream_wait_stream", {}, None, 0, None),                     # (a stream waiting for itself enqueues nothing)
]


def test_recorded_names_and_order(program):
    """One call of every recordable entry point that can be driven without a device (fnr_event_record and fnr_stream_wait_event
    check their event and go straight to the runtime), in the order of a training step: the program lists the same names."""
    lib, h = program
    assert lib.fnr_program_begin(h) == 0
    for name, given, _, status, message in RECORDED:
        args, keep = default_args(name, given)
        assert getattr(lib, name)(*args) == status, (name, lib.fnr_last_error())
        assert message is None or message in lib.fnr_last_error(), (name, lib.fnr_last_error())
    assert lib.fnr_program_end(h) == 0
    assert names(lib, h) == [recorded or name for name, _, recorded, _, _ in RECORDED]
    # the replay stops at the first call's own failure, as the call did
    assert lib.fnr_program_replay(h, None) == -1 and b"train_prologue: null argument" in lib.fnr_last_error()


def test_recorder_holders_on_the_host(tmp_path):
    """tests/host/seq_record_host.cpp: by-value copies outlive the caller's scope, the tags and the PrologueArgs / EdgeDraw /
    fnr_table_adam patches with and without scalars, NULL host arrays, a moved program.  No sanitizer flags here."""
    assert os.path.exists(HIPCC), "hipcc builds the library these tests load"
    csrc = os.path.join(ROOT, "fruitnerf_amd", "csrc")
    exe = tmp_path / "seq_record_host"
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", csrc,
                    os.path.join(ROOT, "tests", "host", "seq_record_host.cpp"), os.path.join(csrc, "sequencer.hip"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "seq_record_host: 0 failed" in run.stdout
