"""fnr_weights_pdf after its kernel was specialised per samples-per-lane and the previous level's bin edges were staged into
LDS (ex[below] / ex[above] were gathers from memory): against the float64 oracle pieces of
tests/test_gpu_ray_kernels.py::test_weights_pdf_every_stage, with that test's bars and its stage-by-stage references.

S_prev = 1, 63, 64 (one sample per lane, partial and full), 65 (two), 256 (four, full — a training step's first level), 512
(eight, the LDS rows full to their last float); S_new = 0 (weights only: no resampling input is read), 1, 48, 96 (two strides
of the wave over the new bins: the second comes from a register too); anneal 1 and 0.5; `rand` given and null; the median depth
wanted and not.  R = 5: a workgroup with one ray and three idle waves behind a full one; the rays are the first five of the
other file's batch — empty, opaque at the first / last sample, a surface spike, zero-width bins."""
import pytest
import torch

from oracle import ns_torch as ns
from tests import test_gpu_ray_kernels as rk

pytestmark = pytest.mark.gpu

F8 = torch.float64
R = 5
NEAR, FAR = 0.05, 1000.0


@pytest.fixture(scope="module")
def batches():
    """S_prev -> (edges, density, spacing_prev per kind, float64 weights, weight bound): built once, never modified."""
    cache = {}

    def get(S_prev):
        if S_prev not in cache:
            edges, dens, _, _ = rk._batch(S_prev, seed=3)
            edges, dens = edges[:R].contiguous(), dens[:R].contiguous()
            g = torch.Generator().manual_seed(S_prev)
            sps = []
            for _ in (0, 1):
                sp = torch.sort(torch.rand(R, S_prev + 1, generator=g), 1).values
                sp[:, 0], sp[:, -1] = 0.0, 1.0
                sps.append(sp.contiguous())
            w64 = rk._samples64(edges).get_weights(dens.double()[..., None])[..., 0]
            cache[S_prev] = (edges, dens, sps, w64, rk._weight_arith(edges, dens), torch.rand(R, generator=g))
        return cache[S_prev]
    return get


@pytest.mark.parametrize("S_new", [0, 1, 48, 96])
@pytest.mark.parametrize("S_prev", [1, 63, 64, 65, 256, 512])
def test_weights_pdf_with_staged_bin_edges(dev, batches, S_prev, S_new):
    K = rk._K()
    edges, dens, sps, w64, A, rand_cpu = batches(S_prev)
    E = (S_prev + 63) // 64
    worst = {}
    rb = ns.RayBundle(torch.zeros(R, 3, dtype=F8), torch.zeros(R, 3, dtype=F8), torch.ones(R, 1, dtype=F8))
    for kind in (0, 1):
        fn, inv = rk._spacing_fns(kind)
        lo, hi = (float(fn(torch.tensor(v, dtype=torch.float32).double())) for v in (NEAR, FAR))
        spacing_prev = sps[kind]

        def to_euclid(x):
            return inv(x * hi + (1 - x) * lo)
        rs_prev = ns.RaySamples(frustums=None, spacing_starts=spacing_prev.double()[:, :-1, None],
                                spacing_ends=spacing_prev.double()[:, 1:, None], spacing_to_euclidean_fn=to_euclid)
        for anneal in (1.0, 0.5):
            for training in (True, False):
                for want_depth in (True, False):
                    rand = rand_cpu if training else None
                    w, depth, sp_new, eu_new = K.weights_pdf(rk._rays(R, dev, NEAR, FAR), kind, S_prev, S_new, dens.to(dev),
                                                             spacing_prev.to(dev), edges.to(dev), anneal,
                                                             None if rand is None else rand.to(dev), want_depth=want_depth)
                    w = w.cpu()
                    wmax = w64.max(1, keepdim=True).values
                    worst.setdefault("w", []).append(((w.double() - w64).abs() / (2e-6 * wmax + A + 1e-300)).max())
                    if want_depth:
                        rk._check_median(f"weights_pdf S_prev={S_prev}", depth.cpu(), edges, w64)
                    else:
                        assert depth is None
                    if S_new == 0:
                        assert sp_new is None and eu_new is None
                        continue
                    sp_new, eu_new = sp_new.cpu(), eu_new.cpu()
                    smp = ns.PDFSampler(num_samples=S_new, include_original=False, single_jitter=True)
                    smp.train(training)
                    wa = torch.pow(w.double(), anneal)      # the resampling stage on the kernel's own weights
                    out = smp(rb, rs_prev, wa[..., None], rand=None if rand is None else rand.double()[:, None])
                    ref_sp = torch.cat([out.spacing_starts[..., 0], out.spacing_ends[..., -1:, 0]], -1)
                    b = 2e-6 + rk._inverse_cdf_slope(spacing_prev, wa, ref_sp) * (E + 8) * rk.U
                    worst.setdefault("spacing", []).append(((sp_new.double() - ref_sp).abs() / b).max())
                    e_ref = to_euclid(sp_new.double())
                    b = 2e-6 * e_ref.abs() + (2.0 ** -21 * e_ref ** 2 if kind == 1 else 0.0)
                    worst.setdefault("euclid", []).append(((eu_new.double() - e_ref).abs() / b).max())
                    assert torch.isfinite(sp_new).all() and sp_new.shape == (R, S_new + 1)
    for k, v in worst.items():
        assert rk._worst(f"weights_pdf staged [{S_prev}->{S_new}].{k}", torch.stack(v)) <= 1.0, k
