"""The per-edge sampler jitter of use_single_jitter=False, restated in numpy on the Philox4x32-10 of
tests/composite_background_reference.py (itself pinned on the Random123 known answers): what include/fruitnerf_hip.h states
for fnr_edge_jitter, fnr_train_prologue_edges and fnr_weights_pdf_edges.

The jitter of edge j of ray r at sampling level l (0 = the spaced sampler, 1.. = the PDF samplers) is
  u01(word (j & 3) of Philox4x32-10(counter, key)),
  counter = (uint32 r, uint32(r >> 32) ^ ((3 + l) << 24) ^ ((j >> 2) << 8), uint32 offset, uint32(offset >> 32)),
  key = (uint32 seed, uint32(seed >> 32)),  u01(x) = (x >> 8) 2^-24.
Shared by tests/test_per_sample_jitter_cpu.py and tests/test_gpu_per_sample_jitter.py."""
import numpy as np

from tests.composite_background_reference import philox4x32_10

EDGE_JITTER_GROUP0 = 3          # word groups 0, 1: fnr_train_prologue; 2: fnr_random_background; 3 + level: the edges
EDGE_JITTER_MAX_LEVELS = 5


def edge_jitter_words(seed: int, offset: int, level: int, n_rays: int, n_edges: int, first_ray: int = 0) -> np.ndarray:
    """[n_rays, n_edges] uint32: the Philox word behind every number (rays first_ray .. first_ray + n_rays - 1)."""
    r = (np.arange(n_rays, dtype=np.uint64) + np.uint64(first_ray))[:, None]
    j = np.arange(n_edges, dtype=np.uint64)[None, :]
    m32 = np.uint64(0xFFFFFFFF)
    c1 = (r >> np.uint64(32)) ^ np.uint64(((EDGE_JITTER_GROUP0 + level) << 24) & 0xFFFFFFFF) ^ ((j >> np.uint64(2)) << np.uint64(8))
    shape = (n_rays, n_edges)
    counter = np.stack([np.broadcast_to(r & m32, shape), c1 & m32,
                        np.full(shape, offset & 0xFFFFFFFF, np.uint64), np.full(shape, (offset >> 32) & 0xFFFFFFFF, np.uint64)],
                       -1).astype(np.uint32)
    words = philox4x32_10(counter, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    pick = np.broadcast_to((j & np.uint64(3)).astype(np.int64), shape)
    return np.take_along_axis(words, pick[..., None], -1)[..., 0]


def edge_jitter(seed: int, offset: int, level: int, n_rays: int, n_edges: int, first_ray: int = 0) -> np.ndarray:
    """[n_rays, n_edges] float32 in [0, 1): what fnr_edge_jitter writes."""
    words = edge_jitter_words(seed, offset, level, n_rays, n_edges, first_ray)
    return ((words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
