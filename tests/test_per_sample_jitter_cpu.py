"""use_single_jitter=False without a device: the new entry points exist and refuse bad arguments on the host, the sampler and
the model construct with the switch off, the numpy restatement of the per-edge numbers (tests/edge_jitter_reference.py) has
the properties the counter layout promises, and an explicit `jitter=` list of the wrong shape is a ValueError."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import edge_jitter_reference as ej
from tests.composite_background_reference import step_randoms

NEW = ("fnr_edge_jitter", "fnr_train_prologue_edges", "fnr_weights_pdf_edges")
SEED, OFFSET = (0xC0FFEE12 << 32) | 0x89ABCDEF, (7 << 32) + 5


def test_library_exports_the_new_entry_points_at_abi_13():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert lib.fnr_abi_version() == L.ABI_VERSION == 13
    assert L.FNR_EDGE_JITTER_MAX_LEVELS == 5


def test_edge_jitter_refuses_bad_arguments_without_a_device():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    out = C.c_void_p(64)       # never dereferenced: every call below fails its argument checks
    assert lib.fnr_edge_jitter(1, 1, 0, 4, 4, None, None) == -1 and b"edge_jitter" in lib.fnr_last_error()
    assert lib.fnr_edge_jitter(1, 1, 0, -1, 4, out, None) == -1 and b"edge_jitter" in lib.fnr_last_error()
    for level in (-1, L.FNR_EDGE_JITTER_MAX_LEVELS):
        assert lib.fnr_edge_jitter(1, 1, level, 4, 4, out, None) == -1 and b"level" in lib.fnr_last_error()
    for n_edges in (0, L.FNR_EDGE_JITTER_MAX_EDGES + 1):
        assert lib.fnr_edge_jitter(1, 1, 0, 4, n_edges, out, None) == -1 and b"n_edges" in lib.fnr_last_error()


def test_train_prologue_edges_refuses_bad_arguments_without_a_device():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    p = C.c_void_p(64)
    good_set = L.fnr_image_set()
    good_set.n_images, good_set.H, good_set.W = 2, 4, 4
    good_set.images, good_set.masks, good_set.c2w = 64, 64, 64

    def call(set_=good_set, pose_mode=0, u=p, S0=8, base=p, pose=None, adj=None, n_rays=16):
        return lib.fnr_train_prologue_edges(C.byref(set_) if set_ is not None else None, None, pose_mode, p, 2, n_rays, 1, 1,
                                            pose, adj, u, p, p, p, p, p, 0.05, 1000.0, 1, S0, base, p, p, None)
    assert call(set_=None) == -1 and b"null" in lib.fnr_last_error()
    assert call(u=None) == -1 and b"null" in lib.fnr_last_error()
    assert call(base=None) == -1 and b"null" in lib.fnr_last_error()
    assert call(set_=L.fnr_image_set()) == -1 and b"bad image set" in lib.fnr_last_error()
    assert call(pose_mode=2) == -1 and b"pose_mode" in lib.fnr_last_error()
    for S0 in (0, -3, L.FNR_EDGE_JITTER_MAX_EDGES):
        assert call(S0=S0) == -1 and b"S0" in lib.fnr_last_error()
    assert call(pose=p) == -1 and b"go together" in lib.fnr_last_error()
    assert call(pose=p, adj=p, n_rays=1) == -1 and b"fewer rays" in lib.fnr_last_error()


def test_weights_pdf_edges_refuses_bad_arguments_without_a_device():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    p = C.c_void_p(64)
    rays = L.fnr_rays(4, None, None, None, None, None)

    def call(rays_=rays, S_prev=16, S_new=8, density=p, spacing_prev=p, rand=None, level=1, draw=0, kind=1, u_base=p):
        return lib.fnr_weights_pdf_edges(C.byref(rays_) if rays_ is not None else None, kind, S_prev, S_new, density,
                                         spacing_prev, p, 1.0, u_base, rand, p, None, p, p, 1, 1, level, draw, None)
    assert call(rays_=None) == -1 and b"null" in lib.fnr_last_error()
    assert call(density=None) == -1 and b"null" in lib.fnr_last_error()
    for S_prev in (0, 513):
        assert call(S_prev=S_prev) == -1 and b"S_prev" in lib.fnr_last_error()
    assert call(spacing_prev=None) == -1 and b"resampling" in lib.fnr_last_error()
    assert call(u_base=None) == -1 and b"resampling" in lib.fnr_last_error()
    assert call(kind=2) == -1 and b"spacing_kind" in lib.fnr_last_error()
    for level in (0, -1, L.FNR_EDGE_JITTER_MAX_LEVELS):
        assert call(level=level, draw=1) == -1 and b"level" in lib.fnr_last_error()
    assert call(rand=p, draw=1) == -1 and b"draw" in lib.fnr_last_error()


def test_sampler_and_model_construct_with_the_switch_off():
    """(Both fail on the commit before the switch was built: NotImplementedError.)"""
    from fruitnerf_amd.data.semantics import apple_metadata
    from fruitnerf_amd.fruit_nerf import FruitModel, FruitNerfModelConfig, ProposalNetworkSampler
    assert ProposalNetworkSampler().single_jitter is False          # nerfstudio's default for the class
    assert ProposalNetworkSampler(single_jitter=False).single_jitter is False
    assert ProposalNetworkSampler(single_jitter=True).single_jitter is True
    hm = FruitModel(FruitNerfModelConfig(log2_hashmap_size=4, use_single_jitter=False), apple_metadata(), num_train_data=1,
                    device="cpu")
    assert hm.proposal_sampler.single_jitter is False
    hm.train()
    assert hm.level0_spec()["per_edge"] is True
    hm.proposal_sampler.single_jitter = True                          # a pass reads the attribute, not the config
    assert hm.level0_spec()["per_edge"] is False
    on = FruitModel(FruitNerfModelConfig(log2_hashmap_size=4), apple_metadata(), num_train_data=1, device="cpu")
    assert on.proposal_sampler.single_jitter is True


def test_reference_numbers_are_uniform_words_of_their_own():
    R, E = 37, 261
    per_level = [ej.edge_jitter(SEED, OFFSET, lvl, R, E) for lvl in range(ej.EDGE_JITTER_MAX_LEVELS)]
    for x in per_level:
        assert x.dtype == np.float32 and x.shape == (R, E)
        assert (x >= 0).all() and (x < 1).all()
        assert 0.45 < float(x.mean()) < 0.55
    words = [ej.edge_jitter_words(SEED, OFFSET, lvl, R, E) for lvl in range(ej.EDGE_JITTER_MAX_LEVELS)]
    # distinct across levels, across edges (the quad boundary j = 3 -> 4 included) and across rays
    assert len(np.unique(np.stack(words))) == np.stack(words).size
    w0 = words[0]
    assert (w0[:, 3] != w0[:, 4]).all() and (w0[:, 0] != w0[:, 4]).all() and (w0[:, :-1] != w0[:, 1:]).all()
    # ... and from every word of groups 0-2 (the prologue's and the random background's) of the same ray
    for group in range(3):
        taken = step_randoms(SEED, OFFSET, R, group)                  # [R, 4] float32 of (word >> 8)
        for lvl in range(ej.EDGE_JITTER_MAX_LEVELS):
            for k in range(4):
                assert not (per_level[lvl] == taken[:, k:k + 1]).any(), (group, lvl, k)
    # another offset, another seed: other numbers; a later first ray: the same rows
    assert not np.array_equal(ej.edge_jitter(SEED, OFFSET + 1, 0, R, E), per_level[0])
    assert not np.array_equal(ej.edge_jitter(SEED ^ (1 << 40), OFFSET, 0, R, E), per_level[0])
    assert np.array_equal(ej.edge_jitter(SEED, OFFSET, 2, 7, E, first_ray=30), per_level[2][30:])
    # rays beyond 2^32 reach the counter's second word without touching the group's or the quad's bits
    far = ej.edge_jitter_words(SEED, OFFSET, 1, 2, 8, first_ray=(1 << 32) + 5)
    assert not np.array_equal(far, ej.edge_jitter_words(SEED, OFFSET, 1, 2, 8, first_ray=5))


def test_jitter_shape_errors_name_the_expected_shape():
    from fruitnerf_amd.fruit_nerf import ProposalNetworkSampler
    R = 6
    off = ProposalNetworkSampler(num_proposal_samples_per_ray=(256, 96), num_nerf_samples_per_ray=48, single_jitter=False)
    on = ProposalNetworkSampler(num_proposal_samples_per_ray=(256, 96), num_nerf_samples_per_ray=48, single_jitter=True)
    assert off.level_samples() == (256, 96, 48)
    good_off = [torch.rand(R, 257), torch.rand(R, 97), torch.rand(R, 49)]
    good_on = [torch.rand(R, 1), torch.rand(R), None]
    off.check_jitter(good_off, R)
    on.check_jitter(good_on, R)
    with pytest.raises(ValueError, match=r"\(6, 97\)"):
        off.check_jitter([good_off[0], torch.rand(R, 1), good_off[2]], R)
    with pytest.raises(ValueError, match=r"\(6, 257\)"):
        off.check_jitter([torch.rand(R), good_off[1], good_off[2]], R)
    with pytest.raises(ValueError, match=r"\(6, 49\)"):
        off.check_jitter([good_off[0], good_off[1], torch.rand(R, 48)], R)
    with pytest.raises(ValueError, match=r"\(6,\) or \(6, 1\)"):
        on.check_jitter(good_off, R)
    with pytest.raises(ValueError, match="3 sampling levels"):
        off.check_jitter(good_off[:2], R)
