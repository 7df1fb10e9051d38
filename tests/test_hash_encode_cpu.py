"""tests/test_gpu_hash_encode.py without a GPU: where its constants and the CPU column of its docstring come from.

The GPU file's tests take the float32 CPU evaluation of the kernels' operations in the kernels' order (grid_cell, the
gathers, grid_interp, blend_input_grad, s * g; the consumers' chain by float32 autograd) in place of the kernels when
handed `FLOAT32` for a device.  Over the GPU file's own inputs that evaluation stays within 1/4 of every bound — the
factor 4 the kernels get for another order of summation — and its features equal ns.HashEncoding's bit for bit.  Run
through the tests, the inputs' own conditions are checked here too: the share of samples next to a lattice plane (at
most 3 % of the ray samples, under 1 % of the random points), the edge samples, the placement of the runs, the lattice's
coordinates.  And the bounds bite: three stand-ins of kernel bugs in the float32 evaluation (one corner difference of
blend_input_grad with the wrong sign, the selector dropped in front of the scaling, two axes of the Jacobian swapped)
leave them.  `pytest -s` prints the worst |err| / bound per quantity."""
import pytest

from tests import test_gpu_hash_encode as he

QUARTER = 0.25


def _worst(test, *args):
    he.WORST.clear()
    test(he.FLOAT32, *args)
    return dict(he.WORST)


def _quarter(w, *keys):
    assert set(w) == set(keys), w
    assert all(0.0 < v <= QUARTER for v in w.values()), w


@pytest.mark.parametrize("kind", ["points", "rays"])
@pytest.mark.parametrize("name", he.ALL_GRIDS)
def test_float32_evaluation_is_within_a_quarter_of_the_bounds(name, kind):
    he.NEAR.clear()
    _quarter(_worst(he.test_features_jacobian_and_input_grad_per_sample, name, kind), "features", "jacobian", "partial")
    assert he.NEAR[kind] < (0.01 if kind == "points" else 0.03 + 1e-12), he.NEAR


@pytest.mark.parametrize("name", ["hs8", "hs12"])
def test_float32_runs(name):
    he.NEAR.clear()
    _quarter(_worst(he.test_runs_of_samples_in_one_cell, name), "features", "jacobian", "partial")
    assert he.NEAR["points"] < 0.01


@pytest.mark.parametrize("name", ["small16", "hs5", "tiny6"])
def test_float32_rays_through_a_non_unit_box(name):
    he.NEAR.clear()
    _quarter(_worst(he.test_rays_through_a_non_unit_box, name), "features", "jacobian", "partial")
    assert he.NEAR["aabb rays"] <= 0.03


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["small16", "hs5", "hs8", "tiny6"])
def test_float32_lattice(name, mode):
    _quarter(_worst(he.test_lattice_source, name, mode), "features")


@pytest.mark.parametrize("S", [48, 129])
@pytest.mark.parametrize("mode", [0, 1])
def test_float32_consumers(mode, S):
    he.NEAR.clear()
    _quarter(_worst(he.test_both_producers_through_their_consumers, mode, S), "via jacobian", "via partial")
    assert max(he.NEAR.values()) <= 0.03


@pytest.mark.parametrize("levels", [8, 12, 16])
@pytest.mark.parametrize("mode", [0, 1])
def test_float32_contraction(mode, levels):
    _quarter(_worst(he.test_contract_jacobian_at_every_loop_shape, mode, levels), "contract")


def test_float32_repeatability():
    he.test_repeatability_and_want_jacobian(he.FLOAT32, "hs5")


@pytest.mark.parametrize("mutation", ["corner sign", "swapped axes"])
@pytest.mark.parametrize("test,args", [("test_features_jacobian_and_input_grad_per_sample", ("edge2", "points")),
                                       ("test_rays_through_a_non_unit_box", ("hs5",))])
def test_a_wrong_float32_evaluation_leaves_the_bound(monkeypatch, mutation, test, args):
    monkeypatch.setattr(he, "MUTATION", mutation)
    with pytest.raises(AssertionError):
        getattr(he, test)(he.FLOAT32, *args)
