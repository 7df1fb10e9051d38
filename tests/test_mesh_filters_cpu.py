"""CPU: the float64 restatement of the mesh filters (tests/mesh_filters_reference.py) checked against what the filters have
to do by construction, and against the figures measured on the three-sphere mesh."""
import numpy as np
import pytest

from tests import mesh_components_reference as mr
from tests import mesh_filters_reference as fr


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _rows(offsets, entries):
    return [entries[offsets[r]:offsets[r + 1]].tolist() for r in range(len(offsets) - 1)]


@pytest.mark.parametrize("name", sorted(mr.hand_made()))
def test_rows_are_symmetric_and_duplicate_free(name):
    vertices, faces, _ = mr.hand_made()[name]
    V = vertices.shape[0]
    offsets, nb = fr.vertex_rows(faces, V, fr.NEIGHBOURS)
    assert offsets.dtype == nb.dtype == np.int32 and offsets.shape == (V + 1,) and offsets[-1] == nb.size
    rows = _rows(offsets, nb)
    for a, row in enumerate(rows):
        assert row == sorted(set(row)) and a not in row
        assert all(a in rows[b] for b in row)
        expected = {int(b) for f in faces.tolist() if a in f for b in f if b != a}
        assert set(row) == expected
    offsets, fc = fr.vertex_rows(faces, V, fr.FACES)
    for a, row in enumerate(_rows(offsets, fc)):
        assert row == [i for i, f in enumerate(faces.tolist()) if a in f]


def test_neighbour_rows_do_not_depend_on_the_face_order():
    vertices, faces, _ = mr.strip(501, (200,), seed=3)
    a = fr.vertex_rows(faces, vertices.shape[0], fr.NEIGHBOURS)
    b = fr.vertex_rows(faces[np.random.default_rng(0).permutation(faces.shape[0])], vertices.shape[0], fr.NEIGHBOURS)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("weights", [fr.UNIFORM, fr.INVERSE_DISTANCE])
def test_a_zero_factor_returns_the_input_bits(weights):
    vertices, faces, _ = mr.hand_made()["tets_sharing_an_edge"]
    offsets, nb = fr.vertex_rows(faces, vertices.shape[0], fr.NEIGHBOURS)
    assert np.array_equal(_bits(fr.smooth(vertices, offsets, nb, [0.0], weights)), _bits(vertices))


def test_vertices_without_neighbours_do_not_move():
    vertices, faces, _ = mr.hand_made()["repeated_index"]          # vertex 4 is listed only by the face (4, 4, 4)
    vertices, faces = fr.with_unreferenced(vertices, faces)
    offsets, nb = fr.vertex_rows(faces, vertices.shape[0], fr.NEIGHBOURS)
    still = np.flatnonzero(np.diff(offsets) == 0)
    assert 4 in still and 3 in still and set(range(7, 12)) <= set(still.tolist())
    out = fr.taubin(vertices, faces, 3)
    assert np.array_equal(_bits(out[still]), _bits(vertices[still]))
    moved = np.setdiff1d(np.arange(vertices.shape[0]), still)
    assert (out[moved] != vertices[moved]).any(axis=1).all()


def test_a_mesh_in_a_plane_stays_there():
    rng = np.random.default_rng(5)
    n = 7
    xy = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 2) + rng.uniform(-.3, .3, (n * n, 2))
    vertices = np.concatenate([xy, np.zeros((n * n, 1))], axis=1).astype(np.float32)
    q = np.array([[i * n + j, (i + 1) * n + j, i * n + j + 1, (i + 1) * n + j + 1] for i in range(n - 1) for j in range(n - 1)])
    faces = np.concatenate([q[:, [0, 1, 2]], q[:, [2, 1, 3]]]).astype(np.int32)
    for weights in (fr.UNIFORM, fr.INVERSE_DISTANCE):
        out = fr.taubin(vertices, faces, 4, weights=weights)
        assert (out[:, 2] == 0).all() and (out[:, :2] != vertices[:, :2]).any()
    normals = fr.vertex_normals(vertices, faces)
    assert np.array_equal(normals, np.tile(np.float32([0, 0, 1]), (n * n, 1)))


def test_normals_of_the_spheres_point_outwards():
    m = fr.spheres_mesh()
    normals = fr.vertex_normals(m["vertices"], m["faces"])
    assert normals.dtype == np.float32 and np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-6)
    # on a sphere the normal is the direction from its centre (components 0, 3, 2 by first face; 1 is the speck)
    labels, _ = mr.components(m["faces"])
    for c, centre in zip((0, 3, 2), mr.SPHERES_CENTRES):
        ids = np.unique(m["faces"][labels == c])
        radial = m["vertices"][ids] - np.float32(centre)
        radial /= np.linalg.norm(radial, axis=1, keepdims=True)
        assert (np.sum(normals[ids] * radial, axis=1) > 0.9).all()
    # a vertex nobody lists, and one whose faces have no area, keep (0, 0, 0)
    v, f = fr.with_unreferenced(*mr.hand_made()["repeated_index"][:2])
    n = fr.vertex_normals(v, f)
    assert not n[4].any() and not n[7:].any() and n[0].any()


def test_clustering_with_a_tiny_voxel_is_the_identity():
    m = fr.spheres_mesh()
    nv, nf, nn, nc, c = fr.simplify(m["vertices"], m["faces"], 1e-4, m["normals"], m["colors"])
    assert np.array_equal(c["vertex_cluster"], np.arange(mr.SPHERES_COUNTS[0]))
    assert np.array_equal(_bits(nv), _bits(m["vertices"])) and np.array_equal(nf, m["faces"])
    assert np.array_equal(_bits(nc), _bits(m["colors"])) and np.array_equal(c["face_ids"], np.arange(mr.SPHERES_COUNTS[1]))
    assert np.array_equal(_bits(nn), _bits(fr.vertex_normals(m["vertices"], m["faces"])))


def test_the_duplicate_and_degenerate_rules():
    vertices, faces, face_ids, new_faces = fr.duplicate_case()
    c = fr.cluster(vertices, faces, 1.0)
    assert c["vertex_cluster"].tolist() == [0, 1, 2, 3, 3]
    assert c["offsets"].tolist() == [0, 1, 2, 3, 5] and c["members"].tolist() == [0, 1, 2, 3, 4]
    assert np.array_equal(c["face_ids"], face_ids) and np.array_equal(c["new_faces"], new_faces)
    assert (c["n_degenerate"], c["n_duplicates"]) == (1, 2)
    mean = fr.rows_mean(c["offsets"], c["members"], vertices)
    assert np.array_equal(mean[:3], vertices[:3])
    assert np.array_equal(mean[3], ((vertices[3].astype(np.float64) + vertices[4].astype(np.float64)) / 2.0).astype(np.float32))
    # clusters are numbered by their smallest member, whatever the cells' order in space
    c = fr.cluster(vertices[::-1], np.zeros((0, 3), dtype=np.int32), 1.0)
    assert c["vertex_cluster"].tolist() == [0, 0, 1, 2, 3]
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            fr.cluster(vertices, faces, bad)
    with pytest.raises(ValueError):
        fr.cluster(vertices, faces, 5e-7)                 # 2^21 cells or more on an axis


def _sphere_volumes(vertices, faces):
    labels, n = mr.components(faces)
    s = mr.stats(vertices, faces, labels, n)
    return s["volume"][[0, 3, 2]], s["area"][[0, 3, 2]], n       # the spheres of radius 0.31, 0.27, 0.22 by first face


def test_the_figures_of_the_sphere_mesh():
    m = fr.spheres_mesh()
    vertices, faces = m["vertices"], m["faces"]
    assert (vertices.shape[0], faces.shape[0]) == mr.SPHERES_COUNTS
    volume, area, n = _sphere_volumes(vertices, faces)
    assert n == 4
    t_volume, t_area, _ = _sphere_volumes(fr.taubin(vertices, faces, 10), faces)
    l_volume, l_area, _ = _sphere_volumes(fr.laplacian(vertices, faces, 10), faces)
    print("taubin volume", (t_volume / volume).tolist(), "area", (t_area / area).tolist())
    print("laplacian volume", (l_volume / volume).tolist(), "area", (l_area / area).tolist())
    assert (np.abs(t_volume / volume - 1.0) < 0.02).all()
    assert (l_volume / volume < 0.85).all() and (l_area < area).all()
    nv, nf, _, _, c = fr.simplify(vertices, faces, 0.1)
    assert (nv.shape[0], nf.shape[0], c["n_duplicates"]) == (340, 674, 2)
    assert c["n_degenerate"] == mr.SPHERES_COUNTS[1] - 676
