"""CPU: the mesh-connectivity reference (tests/mesh_components_reference.py) against an independent pure-Python flood fill
on the hand-made meshes, and what the new layer promises without a GPU: host-side refusals of the fnr_mesh_* entry points,
the ctypes struct's size, export_tsdf_mesh's new keywords, and TriangleMesh's refusal of host tensors."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_components_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flood_fill(faces):
    """Components by a sweep from face 0 upwards; neighbours found by comparing undirected edges pair by pair."""
    faces = [tuple(int(i) for i in f) for f in faces]

    def edges(f):
        return {frozenset((f[s], f[(s + 1) % 3])) for s in range(3) if f[s] != f[(s + 1) % 3]}

    sets = [edges(f) for f in faces]
    labels = [-1] * len(faces)
    n = 0
    for seed in range(len(faces)):
        if labels[seed] >= 0:
            continue
        labels[seed] = n
        stack = [seed]
        while stack:
            f = stack.pop()
            for g in range(len(faces)):
                if labels[g] < 0 and sets[f] & sets[g]:
                    labels[g] = n
                    stack.append(g)
        n += 1
    return labels, n


def _edge_counts(faces, labels, n):
    """boundary and non-manifold edges per component, with a dict of incidence counts"""
    count, owner = {}, {}
    for f, face in enumerate(faces):
        for s in range(3):
            a, b = int(face[s]), int(face[(s + 1) % 3])
            if a != b:
                key = (min(a, b), max(a, b))
                count[key] = count.get(key, 0) + 1
                owner.setdefault(key, labels[f])
    boundary, nonmanifold = [0] * n, [0] * n
    for key, k in count.items():
        if k == 1:
            boundary[owner[key]] += 1
        elif k >= 3:
            nonmanifold[owner[key]] += 1
    return boundary, nonmanifold


@pytest.mark.parametrize("name", sorted(mr.hand_made()))
def test_reference_matches_a_flood_fill(name):
    vertices, faces, expected = mr.hand_made()[name]
    labels, n = mr.components(faces)
    fill, n_fill = _flood_fill(faces)
    assert n == n_fill == expected and labels.tolist() == fill
    stats = mr.stats(vertices, faces, labels, n)
    boundary, nonmanifold = _edge_counts(faces, fill, n)
    assert stats["n_faces"].tolist() == [fill.count(c) for c in range(n)]
    assert stats["boundary_edges"].tolist() == boundary and stats["nonmanifold_edges"].tolist() == nonmanifold
    for c in range(n):
        used = np.unique(faces[np.array(fill) == c])
        assert np.array_equal(stats["lo"][c], vertices[used].min(0)) and np.array_equal(stats["hi"][c], vertices[used].max(0))
    assert bool((np.abs(stats["area"]) <= stats["abs_area"]).all()) and bool((np.abs(stats["volume"]) <= stats["abs_volume"]).all())


def test_reference_on_the_named_cases():
    meshes = mr.hand_made()
    vertices, faces, _ = meshes["tets_sharing_a_vertex"]
    labels, n = mr.components(faces)
    stats = mr.stats(vertices, faces, labels, n)
    assert n == 2 and stats["boundary_edges"].tolist() == [0, 0] and stats["nonmanifold_edges"].tolist() == [0, 0]
    assert stats["volume"][0] == pytest.approx(1.0 / 6.0, rel=1e-12) and stats["volume"][1] == pytest.approx(0.7 ** 3 / 6.0, rel=1e-6)
    vertices, faces, _ = meshes["three_on_one_edge"]
    labels, n = mr.components(faces)
    assert mr.stats(vertices, faces, labels, n)["nonmanifold_edges"].tolist() == [1]
    n_vertices, faces, expected = mr.top_index_faces()
    labels, n = mr.components(faces)
    assert n == expected == _flood_fill(faces)[1] and labels.tolist() == _flood_fill(faces)[0]
    # a strip: closed forms
    for total, cuts in ((4101, (1200, 2900)), (20003, (17000,))):
        vertices, faces, pieces = mr.strip(total, cuts, seed=3)
        labels, n = mr.components(faces)
        stats = mr.stats(vertices, faces, labels, n)
        assert faces.shape[0] == total - len(cuts) and sorted(stats["n_faces"].tolist()) == pieces
        assert np.array_equal(stats["boundary_edges"], stats["n_faces"] + 2) and not stats["nonmanifold_edges"].any()
    vertices, faces, expected = mr.triangles_and_fan()
    labels, n = mr.components(faces)
    stats = mr.stats(vertices, faces, labels, n)
    assert n == expected == 3002 and sorted(stats["n_faces"].tolist())[-2:] == [1, 64]
    assert stats["boundary_edges"][stats["n_faces"] == 64].tolist() == [66]


def test_reference_selection():
    vertices, faces, _ = mr.hand_made()["unreferenced_vertices"]
    new_faces, vertex_ids, face_ids = mr.select(faces, vertices.shape[0], [1, 0, 1])
    assert vertex_ids.tolist() == [2, 3, 5, 8, 9, 10] and face_ids.tolist() == [0, 2]
    assert new_faces.tolist() == [[0, 1, 2], [4, 5, 3]]
    assert np.array_equal(vertex_ids[new_faces], faces[face_ids])
    assert mr.vertex_mask_faces(faces, np.arange(12) != 7).tolist() == [True, False, True]
    assert mr.small_component_faces(faces, 2).tolist() == [True, True, False]
    assert mr.largest_component_faces(faces, 1).tolist() == [True, True, False]
    # ties go to the smaller component index
    assert mr.largest_component_faces(np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]]), 2).tolist() == [True, True, False]


def test_spheres_fixture_is_what_the_device_test_asserts():
    from tests import tsdf_reference as tr
    values = mr.spheres_volume()
    assert values.shape == mr.SPHERES_DIMS and values.dtype == np.float32 and not bool((values == 0).any())
    mesh = tr.extract(values, np.zeros(values.shape + (3,)), mr.SPHERES_LO, mr.SPHERES_HI)
    assert (mesh["vertices"].shape[0], mesh["faces"].shape[0]) == mr.SPHERES_COUNTS
    labels, n = mr.components(mesh["faces"])
    stats = mr.stats(mesh["vertices"], mesh["faces"], labels, n)
    assert n == 4 and tuple(stats["n_faces"].tolist()) == mr.SPHERES_COMPONENT_FACES
    assert not stats["boundary_edges"].any() and not stats["nonmanifold_edges"].any() and bool((stats["volume"] > 0).all())
    for c in range(n):                                    # Euler characteristic 2: V - E + F with E = 3 F / 2
        used = np.unique(mesh["faces"][labels == c]).size
        assert used - 3 * int(stats["n_faces"][c]) // 2 + int(stats["n_faces"][c]) == 2
    assert int(mr.small_component_faces(mesh["faces"], 25).sum()) == 2376


# ---- the library, without a GPU -----------------------------------------------------------------------------------------
def test_mesh_entry_points_refuse_bad_arguments_without_a_gpu():
    from fruitnerf_amd import _lib as L
    lib = L.load()
    assert lib.fnr_mesh_workspace_bytes(-1) == 0 and lib.fnr_mesh_workspace_bytes(0) >= 64
    small, large = lib.fnr_mesh_workspace_bytes(100), lib.fnr_mesh_workspace_bytes(100000)
    assert 0 < small < large
    assert lib.fnr_mesh_select_workspace_bytes(-1, 1) == 0 and lib.fnr_mesh_select_workspace_bytes(10, 10) >= 64 + 80
    buf = (C.c_uint64 * ((large + 64) // 8))()
    base = C.addressof(buf)
    ws = base + (-base) % 16
    p = ws + 1024                                         # any non-null pointer: nothing is dereferenced before a refusal

    def refused(rc, word):
        assert rc == -1 and word in lib.fnr_last_error(), lib.fnr_last_error()

    refused(lib.fnr_mesh_components(-1, 10, p, p, p, ws, small, None), b"< 0")
    refused(lib.fnr_mesh_components(10, -1, p, p, p, ws, small, None), b"< 0")
    refused(lib.fnr_mesh_components(1 << 31, 10, p, p, p, ws, small, None), b"2^31")
    refused(lib.fnr_mesh_components(10, 100, None, p, p, ws, small, None), b"null")
    refused(lib.fnr_mesh_components(10, 100, p, None, p, ws, small, None), b"null")
    refused(lib.fnr_mesh_components(10, 100, p, p, None, ws, small, None), b"null counts")
    refused(lib.fnr_mesh_components(10, 100, p, p, p, None, small, None), b"null workspace")
    refused(lib.fnr_mesh_components(10, 100, p, p, p, ws, small - 1, None), b"workspace")
    refused(lib.fnr_mesh_components(10, 100, p, p, p, ws + 8, small, None), b"aligned")

    out = L.fnr_mesh_stats(p, p, p, p, p, p, p, p)
    ok = lambda **kw: dict(dict(V=10, F=100, v=p, f=p, c=p, C=3, ws=ws, n=small, out=C.byref(out)), **kw)    # noqa: E731

    def stats(a):
        return lib.fnr_mesh_component_stats(a["V"], a["F"], a["v"], a["f"], a["c"], a["C"], a["ws"], a["n"], a["out"], None)

    refused(stats(ok(V=-1)), b"< 0")
    refused(stats(ok(C=-1)), b"n_components")
    refused(stats(ok(C=101)), b"n_components")           # more components than faces
    refused(stats(ok(C=0)), b"n_components")             # faces without a component
    refused(stats(ok(F=0, C=2)), b"n_components")
    refused(stats(ok(out=None)), b"null out")
    refused(stats(ok(v=None)), b"null")
    refused(stats(ok(c=None)), b"null")
    refused(stats(ok(out=C.byref(L.fnr_mesh_stats(p, p, p, p, None, p, p, p)))), b"null output")
    refused(stats(ok(ws=None)), b"null workspace")
    refused(stats(ok(n=small - 1)), b"workspace")
    refused(stats(ok(ws=ws + 4)), b"aligned")

    sel = lib.fnr_mesh_select_workspace_bytes(10, 100)
    refused(lib.fnr_mesh_select_count(10, -1, p, p, p, ws, sel, None), b"< 0")
    refused(lib.fnr_mesh_select_count(10, 100, p, None, p, ws, sel, None), b"null")
    refused(lib.fnr_mesh_select_count(10, 100, p, p, None, ws, sel, None), b"null counts")
    refused(lib.fnr_mesh_select_count(10, 100, p, p, p, ws, sel - 1, None), b"workspace")
    refused(lib.fnr_mesh_select_emit(10, 100, p, ws, sel, 11, 5, p, p, p, None), b"new sizes")
    refused(lib.fnr_mesh_select_emit(10, 100, p, ws, sel, 5, -1, p, p, p, None), b"new sizes")
    refused(lib.fnr_mesh_select_emit(10, 100, None, ws, sel, 5, 5, p, p, p, None), b"null faces")
    refused(lib.fnr_mesh_select_emit(10, 100, p, ws, sel, 5, 5, None, p, p, None), b"null")
    refused(lib.fnr_mesh_select_emit(10, 100, p, ws, sel, 5, 5, p, None, p, None), b"null vertex_ids")
    refused(lib.fnr_mesh_select_emit(10, 100, p, None, sel, 5, 5, p, p, p, None), b"null workspace")
    refused(lib.fnr_mesh_select_emit(10, 100, p, ws + 8, sel, 5, 5, p, p, p, None), b"aligned")


def test_mesh_stats_struct_matches_the_header():
    from fruitnerf_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fruitnerf_hip.h")).read()
    body = re.search(r"typedef struct fnr_mesh_stats \{(.*?)\} fnr_mesh_stats;", hdr, flags=re.S).group(1)
    fields = re.findall(r"^\s*(?:int32_t|float|double)\*\s*([a-z_]+);", body, flags=re.M)
    assert fields == [name for name, _ in L.fnr_mesh_stats._fields_] and len(fields) == 8
    assert C.sizeof(L.fnr_mesh_stats) == 8 * C.sizeof(C.c_void_p)
    for name in ("fnr_mesh_workspace_bytes", "fnr_mesh_components", "fnr_mesh_component_stats", "fnr_mesh_select_count",
                 "fnr_mesh_select_emit"):
        assert name in L.SIGNATURES and re.search(r"\b%s\(" % name, hdr)
    assert L.ABI_VERSION == 13


def test_exporter_keywords_default_to_none():
    from fruitnerf_amd.export import exporter_utils as eu
    parameters = inspect.signature(eu.export_tsdf_mesh).parameters
    assert parameters["min_component_faces"].default is None and parameters["largest_components"].default is None
    assert list(parameters)[:2] == ["pipeline", "output_dir"] and parameters["semantic_threshold"].default is None
    fruit = inspect.signature(eu.export_fruit_meshes).parameters
    assert fruit["semantic_threshold"].default == 0.9 and fruit["min_component_faces"].default == 24
    with pytest.raises(TypeError, match="unexpected"):
        eu.export_fruit_meshes(None, "unused", voxels=3)


def test_triangle_mesh_has_no_cpu_path():
    from fruitnerf_amd.export.mesh import TriangleMesh
    from fruitnerf_amd.export.tsdf import TSDF
    with pytest.raises(RuntimeError, match="no CPU path"):
        TriangleMesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    assert callable(getattr(TSDF, "get_triangle_mesh"))
