"""CPU: the batched template fits of the second counting stage (fnr_cloud_icp / fnr_cloud_hausdorff, csrc/cloud_fit.hip)
are declared, exported and check their arguments on the host; the Ward tree built once cuts like ward_labels; the host
path of split_large_cluster decides as it did (tests/golden/reference_split.npz)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fnr_cloud_icp_workspace_bytes", "fnr_cloud_icp", "fnr_cloud_hausdorff_workspace_bytes", "fnr_cloud_hausdorff")


def test_new_symbols_are_exported_and_declared_and_the_abi_stays_13():
    from fruitnerf_amd import _kernels as K
    from fruitnerf_amd import _lib as L
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "fruitnerf_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert lib.fnr_abi_version() == L.ABI_VERSION == 13
    assert "#define FNR_ABI_VERSION 13" in hdr
    assert callable(K.cloud_icp) and callable(K.cloud_hausdorff)
    # the declarations cite the reference lines they replace
    block = hdr[hdr.index("fnr_cloud_icp_workspace_bytes") - 1200:hdr.index("fnr_cloud_hausdorff(")]
    assert ":262-279" in block and ":277, :315" in block
    assert lib.fnr_cloud_icp_workspace_bytes(0) == 0 and lib.fnr_cloud_icp_workspace_bytes(3) >= 3 * 32
    assert lib.fnr_cloud_hausdorff_workspace_bytes(2, 1000) >= 2 * 48 + (1000 // 256 + 4) * 16


def _i64(*v):
    return (C.c_int64 * len(v))(*v)


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


PTR = 256     # stands for a device pointer: every call below is rejected before anything could read it


def _icp(lib, **kw):
    a = dict(tgt=PTR, n_tgt=10, tgt_off=_i64(0, 4, 10), B=2, src=PTR, n_src=5, src_off=_i64(0, 5), S=1, src_id=_i32(0, 0),
             init=PTR, dist=0.01, scaling=1, iters=30, T=PTR, fit=PTR, rmse=PTR, it=PTR, corr=PTR, ws=PTR, ws_bytes=0)
    a.update(kw)
    return lib.fnr_cloud_icp(a["tgt"], a["n_tgt"], a["tgt_off"], a["B"], a["src"], a["n_src"], a["src_off"], a["S"],
                             a["src_id"], a["init"], a["dist"], a["scaling"], a["iters"], 1e-6, 1e-6, a["T"], a["fit"],
                             a["rmse"], a["it"], a["corr"], a["ws"], a["ws_bytes"], None)


def _hd(lib, **kw):
    a = dict(A=PTR, n_a=10, a_off=_i64(0, 4, 10), Sa=2, src=PTR, n_src=5, src_off=_i64(0, 5), S=1, B=2, a_id=_i32(0, 1),
             src_id=_i32(0, 0), trans=PTR, n_trans=3, trans_off=_i64(0, 0, 3), T=PTR, dist=PTR, wit=PTR, ws=PTR,
             ws_bytes=0)
    a.update(kw)
    return lib.fnr_cloud_hausdorff(a["A"], a["n_a"], a["a_off"], a["Sa"], a["src"], a["n_src"], a["src_off"], a["S"],
                                   a["B"], a["a_id"], a["src_id"], a["trans"], a["n_trans"], a["trans_off"], a["T"],
                                   a["dist"], a["wit"], a["ws"], a["ws_bytes"], None)


ICP_BAD = {
    "null target": (dict(tgt=None), b"null"),
    "null source": (dict(src=None), b"null"),
    "null tgt_offsets": (dict(tgt_off=None), b"null"),
    "null src_offsets": (dict(src_off=None), b"null"),
    "null src_id": (dict(src_id=None), b"null"),
    "null init": (dict(init=None), b"null"),
    "null transformation": (dict(T=None), b"null"),
    "null correspondences": (dict(corr=None), b"null"),
    "null workspace": (dict(ws=None), b"workspace"),
    "short workspace": (dict(), b"workspace"),
    "negative problems": (dict(B=-1), b"n_problems"),
    "negative points": (dict(n_tgt=-1), b"negative"),
    "negative sources": (dict(S=-1), b"negative"),
    "negative iterations": (dict(iters=-1), b"max_iteration"),
    "non-monotone tgt_offsets": (dict(tgt_off=_i64(0, 12, 10)), b"monotone"),
    "non-monotone src_offsets": (dict(src_off=_i64(0, 3, 2, 5), S=3), b"monotone"),
    "offsets past the points": (dict(tgt_off=_i64(0, 4, 11)), b"end at"),
    "offsets not from 0": (dict(tgt_off=_i64(1, 4, 10)), b"must be 0"),
    "src_id too large": (dict(src_id=_i32(0, 1)), b"src_id"),
    "src_id negative": (dict(src_id=_i32(-1, 0)), b"src_id"),
    "zero distance": (dict(dist=0.0), b"positive"),
    "negative distance": (dict(dist=-0.01), b"positive"),
    "NaN distance": (dict(dist=float("nan")), b"positive"),
}

HD_BAD = {
    "null A": (dict(A=None), b"null"),
    "null source": (dict(src=None), b"null"),
    "null a_offsets": (dict(a_off=None), b"null"),
    "null src_offsets": (dict(src_off=None), b"null"),
    "null a_id": (dict(a_id=None), b"null"),
    "null src_id": (dict(src_id=None), b"null"),
    "null translations": (dict(trans=None), b"null"),
    "null distances": (dict(dist=None), b"null"),
    "null witnesses": (dict(wit=None), b"null"),
    "no placement": (dict(T=None), b"neither"),
    "null workspace": (dict(ws=None), b"workspace"),
    "short workspace": (dict(), b"workspace"),
    "negative problems": (dict(B=-1), b"n_problems"),
    "negative points": (dict(n_a=-1), b"negative"),
    "negative translations": (dict(n_trans=-1), b"negative"),
    "non-monotone a_offsets": (dict(a_off=_i64(0, 12, 10)), b"monotone"),
    "non-monotone trans_offsets": (dict(trans_off=_i64(0, 4, 3)), b"monotone"),
    "offsets past the points": (dict(src_off=_i64(0, 6)), b"end at"),
    "a_id too large": (dict(a_id=_i32(0, 2)), b"a_id"),
    "src_id too large": (dict(src_id=_i32(1, 0)), b"src_id"),
    "src_id negative": (dict(src_id=_i32(0, -1)), b"src_id"),
}


@pytest.mark.parametrize("case", sorted(ICP_BAD))
def test_cloud_icp_rejects_bad_arguments_without_a_device(case):
    from fruitnerf_amd import _lib as L
    lib = L.load()
    kw, word = ICP_BAD[case]
    assert _icp(lib, **kw) == -1
    assert word in lib.fnr_last_error(), lib.fnr_last_error()


@pytest.mark.parametrize("case", sorted(HD_BAD))
def test_cloud_hausdorff_rejects_bad_arguments_without_a_device(case):
    from fruitnerf_amd import _lib as L
    lib = L.load()
    kw, word = HD_BAD[case]
    assert _hd(lib, **kw) == -1
    assert word in lib.fnr_last_error(), lib.fnr_last_error()


def test_an_empty_batch_is_accepted_and_launches_nothing():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    assert _icp(lib, B=0, tgt_off=_i64(0), n_tgt=0, src_id=None, tgt=None, ws=None) == 0
    assert _hd(lib, B=0, a_id=None, src_id=None, trans_off=None, ws=None) == 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ward_cut_of_one_tree_equals_ward_labels(seed):
    from fruitnerf_amd.clustering import shapes
    rng = np.random.default_rng(seed)
    n = [257, 400, 1000][seed]
    # a surface of two or three touching shells, like a split cluster's
    centres = np.array([[0.0, 0.0, 0.0], [0.11, 0.0, 0.0], [0.05, 0.1, 0.02]])[:2 + seed % 2]
    d = rng.normal(size=(n, 3))
    P = centres[rng.integers(0, len(centres), n)] + 0.08 * d / np.linalg.norm(d, axis=1, keepdims=True)
    tree = shapes.ward_tree(P)
    for k in range(2, 7):
        assert np.array_equal(shapes.ward_cut(tree, k), shapes.ward_labels(P, k)), k
    few = P[:3]
    assert np.array_equal(shapes.ward_cut(shapes.ward_tree(few), 6), shapes.ward_labels(few, 6))


def test_the_switch_defaults_to_the_host_and_rejects_other_values():
    from fruitnerf_amd.clustering import Clustering, FruitClustering
    assert FruitClustering().second_stage == "host" and Clustering(template_path=None).second_stage == "host"
    assert Clustering(template_path=None, second_stage="device").second_stage == "device"
    with pytest.raises(ValueError, match="second_stage"):
        FruitClustering(second_stage="gpu")
    fc = FruitClustering()
    with pytest.raises(ValueError, match="second_stage"):
        fc.count("/nonexistent.ply", second_stage="gpu")
    assert fc.count("/nonexistent.ply", second_stage="device") == 0 and fc.second_stage == "device"
    assert fc.fit_fruits_batch([]) == []                        # no split cluster: nothing is launched, no device needed


def test_host_path_decisions_on_the_reference_split_are_unchanged():
    """The default path (second_stage="host") on tests/golden/reference_split.npz: the decisions, the six hypothesis
    distances of every split cluster and the count the reference's own split_large_cluster gave."""
    from fruitnerf_amd.clustering import FruitClustering, shapes
    from tests.golden.make_reference_split_golden import make_scene
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_split.npz"))
    X, labels = make_scene()
    fc = FruitClustering(cluster_merge_distance=0.04)
    assert fc.second_stage == "host"
    fc.set_template(shapes.sphere_template(float(g["template_radius"]), int(g["template_points"])))
    Xs, ls = fc.merge_small_clusters(X, None, labels)
    count = fc.split_large_cluster(Xs, None, ls, seed=int(g["seed"]))
    got = np.array([d["distances"] for d in fc.cluster_decisions if "distances" in d])
    want = g["hypothesis_distances"]
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-9
    assert [int(np.argmin(r)) + 1 for r in want] == [d["fruits"] for d in fc.cluster_decisions if "distances" in d]
    assert count == int(g["count"]) and fc.prune_counter == 2
    assert len(fc.cluster_centers) == len(fc.valid_clusters) == count
