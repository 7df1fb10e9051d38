"""NumPy float64 restatements of the kNN front-end of the depth point-cloud export (csrc/cloud_knn.hip, fnr_depth_points)
and the cloud the tests run them on.

    knn                  brute force; squared distance ((dx*dx) + dy*dy) + dz*dz, rows ordered by (d2, input index)
    statistical_outlier  Open3D RemoveStatisticalOutliers, sequential ascending sums
    normals              unit eigenvector of the smallest eigenvalue of the centred covariance (np.linalg.eigh)
    depth_points         origins + directions * depth in torch float32, strict box mask
"""
import numpy as np
import torch


def surface_cloud(seed: int = 7) -> np.ndarray:
    """Three noisy spheres of radius 0.05 (1200 points each), 300 clutter points, 32 exact duplicates; n = 3932."""
    rng = np.random.default_rng(seed)
    parts = []
    for c in [(-0.3, 0, 0), (0.1, 0.2, -0.1), (0.35, -0.25, 0.2)]:
        v = rng.normal(size=(1200, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        parts.append(np.array(c) + 0.05 * v + rng.normal(scale=5e-4, size=(1200, 3)))
    parts.append(rng.uniform(-0.5, 0.5, (300, 3)))
    X = np.concatenate(parts)
    X = np.concatenate([X, X[:32]])
    rng.shuffle(X)
    return X


SPHERE_CENTRES = np.array([(-0.3, 0, 0), (0.1, 0.2, -0.1), (0.35, -0.25, 0.2)], dtype=np.float64)


def surface_cloud_labels(seed: int = 7) -> np.ndarray:
    """Per row of surface_cloud(seed): the sphere it was drawn on (0, 1, 2) or -1 for clutter."""
    rng = np.random.default_rng(seed)
    label_of = {}
    for s, c in enumerate(SPHERE_CENTRES):           # the recipe again, to know which rows are which
        v = rng.normal(size=(1200, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        for row in np.array(c) + 0.05 * v + rng.normal(scale=5e-4, size=(1200, 3)):
            label_of[row.tobytes()] = s
    return np.array([label_of.get(row.tobytes(), -1) for row in surface_cloud(seed)])


def knn(X: np.ndarray, k: int):
    """-> (dist2 [n,k] float64, index [n,k] int32); with n < k the tail of a row is +inf / -1."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    n = X.shape[0]
    dist2 = np.full((n, k), np.inf)
    index = np.full((n, k), -1, dtype=np.int32)
    ids = np.arange(n)
    for i in range(n):
        d = X[i] - X
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        order = np.lexsort((ids, d2))[:k]
        dist2[i, :len(order)] = d2[order]
        index[i, :len(order)] = order
    return dist2, index


_cache = {}


def surface_knn(k: int, seed: int = 7):
    """(X, dist2 [n,k], index [n,k]) of surface_cloud(seed): the 32-neighbour brute force is computed once per process
    (a row for a smaller k is its prefix) and must not be written to."""
    if seed not in _cache:
        X = surface_cloud(seed)
        _cache[seed] = (X,) + knn(X, 32)
    X, d2, idx = _cache[seed]
    return X, d2[:, :k], idx[:, :k]


def mean_distances(dist2: np.ndarray) -> np.ndarray:
    """avg[i]: the square roots of row i's valid entries summed in ascending order, over their number."""
    n, k = dist2.shape
    avg = np.zeros(n)
    for i in range(n):
        s, c = 0.0, 0
        for j in range(k):
            if np.isfinite(dist2[i, j]):
                s = s + np.sqrt(dist2[i, j])
                c += 1
        avg[i] = s / c
    return avg


def statistical_outlier(X: np.ndarray, nb_neighbors: int, std_ratio: float, dist2=None):
    """-> (avg [n], keep [n] bool, (mean, std, threshold)); dist2: knn(X, nb_neighbors)[0] when already at hand."""
    avg = mean_distances(knn(X, nb_neighbors)[0] if dist2 is None else dist2)
    valid = avg > 0
    s = 0.0
    for a in avg[valid]:
        s = s + a
    n_valid = int(valid.sum())
    mean = s / n_valid
    q = 0.0
    for a in avg[valid]:
        q = q + (a - mean) * (a - mean)
    std = np.sqrt(q / (n_valid - 1))
    threshold = mean + std_ratio * std
    return avg, valid & (avg < threshold), (mean, std, threshold)


def covariances(X: np.ndarray, k: int, index=None) -> np.ndarray:
    """[n,3,3] centred covariance of every point's k nearest points (self included); index: knn(X, k)[1] if at hand."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    if index is None:
        _, index = knn(X, k)
    cov = np.zeros((X.shape[0], 3, 3))
    for i in range(X.shape[0]):
        nb = X[index[i][index[i] >= 0]]
        d = nb - nb.mean(axis=0)
        cov[i] = d.T @ d / len(nb)
    return cov


def eigen_gaps(cov: np.ndarray) -> np.ndarray:
    """(l1 - l0) / trace per covariance (0 for a zero matrix)."""
    w = np.linalg.eigvalsh(cov)
    tr = w.sum(axis=1)
    return np.where(tr > 0, (w[:, 1] - w[:, 0]) / np.where(tr > 0, tr, 1.0), 0.0)


def normals(X: np.ndarray, k: int, index=None):
    """-> (normals [n,3], relative eigen-gap [n]); fewer than 3 neighbours: (0, 0, 1)."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    cov = covariances(X, k, index)
    _, v = np.linalg.eigh(cov)
    out = v[:, :, 0].copy()
    if min(X.shape[0], k) < 3:
        out[:] = (0.0, 0.0, 1.0)
    return out, eigen_gaps(cov)


def depth_points(origins: torch.Tensor, directions: torch.Tensor, depth: torch.Tensor, rgb: torch.Tensor, box_min=None,
                 box_max=None):
    """Nerfstudio's generate_point_cloud body in torch float32 -> (points [m,3], colours [m,3]) in ray order."""
    point = origins.float() + directions.float() * depth.float().reshape(-1, 1)
    rgb = rgb.float().reshape(-1, 3)
    if box_min is None:
        return point, rgb
    lo = torch.tensor(box_min, dtype=torch.float32, device=point.device)
    hi = torch.tensor(box_max, dtype=torch.float32, device=point.device)
    mask = torch.all(point > lo, dim=-1) & torch.all(point < hi, dim=-1)
    return point[mask], rgb[mask]
