"""The camera / pixel-sampling kernels compute what they computed on the parent commit, bit for bit: every case of
tests/golden/make_camera_family_parent_golden.py (the generator, with the cases' inputs: a 6-image set of 5 x 7 pixels,
train_ids [4, 0, 3], a camera table of distinct rows, the seeded poses of tests/test_gpu_camera_models.py and
tests/test_camera_se3_cpu.py, imported) is run on the checked-out tree and the SHA-256 of the raw bytes of every output array
is compared with what the generator recorded on the parent commit (tests/golden/camera_family_parent_digests.json: digests,
no arrays).

What changed under these digests: the pixel pick, the camera-frame direction, the world ray and the target gather are one
function each in camera_math.hpp, and the host side of the 14 entry points is one argument block, one validator and one
kernel selection.  What must not change is any bit of any output.

Cases: (no table | intrinsics | intrinsics + distortion) x (no pose | SO3xR3 | SE3) x (1 | 255 | 257 | 4097 | 0 rays), each
running sample_pixels, camera_adjust, train_prologue (S0 in {1, 5, 48}, per ray and per edge), camera_pose_grad and both
algorithms of camera_pose_grad_adam as far as the configuration reaches them; "level 0": the product of the prologue's
run-time options; "camera rays": all rows, an inner block and an empty block.  Why these sizes and how 0 rays are run: the
generator's docstring.  No grid depends on the CU count, so no case is tied to the recording device."""
import json

import pytest

from tests.golden import make_camera_family_parent_golden as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(G.FIXTURE) as f:
        return json.load(f)


def test_every_case_has_a_recorded_digest(golden):
    assert sorted(golden["cases"]) == sorted(G.CASES)
    assert len(G.CASES) == len(G.TABLES) * len(G.POSES) * len(G.RAYS) + 2
    assert all(len(v) > 0 and all(len(d) == 64 for d in v.values()) for v in golden["cases"].values())


@pytest.mark.parametrize("case", list(G.CASES))
def test_same_bits_as_the_parent_commit(dev, golden, case):
    got = G.compute(case, dev)
    want = golden["cases"][case]
    assert sorted(got) == sorted(want)
    differ = [name for name in want if got[name] != want[name]]
    for name in want:
        print(f"[camera family same bits] {case}: {name} {got[name][:12]} vs {want[name][:12]}")
    assert not differ, f"{case}: {differ} differ from the parent commit's"
