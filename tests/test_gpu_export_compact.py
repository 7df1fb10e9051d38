"""fnr_export_compact (csrc/export.hip: k_export_count -> k_export_scan -> k_export_write) called directly on synthetic arrays,
against tests/export_reference.py: counts, ordered points and colours of the three sets, bit for bit; colour channel 3 (the
device's float32 sigmoid) within 4 x the error of the same formula evaluated in float32 on the CPU.  The output buffers are
views buf[:cap] of longer tensors filled with a sentinel: every row at or past min(count, cap) must still hold it, so a write
past the capacity, a write below the running total's start and a stray row all show.

Sizes: up to 2 * 1024 * 1024 + 3 * 1024 + 5 samples = 2052 tiles = three trips of the scan's 1024-tile loop (the carry
between chunks, the hand-over by thread 1023, the ragged last chunk).  tests/test_export_reference_cpu.py checks the reference
and the inputs (every logit at least 16 ulp of 0.9 from the colormap cut: no sample is excluded anywhere).

Channel 3, worst |err| / (u s), u = 2^-24, s the float64 sigmoid, over all cases: float32 on the CPU 1.640, so the kernel is
granted 6.56; MI355X 1.522 (random N = 1 048 577; every case prints its own).  Times on an MI355X: N = 2 100 229 0.14 s,
N = 1 048 577 0.06 s, everything selected at 1 048 577 0.16 s (the longest), the module 3 s with the yardstick's 0.4 s.
"""
import numpy as np
import pytest
import torch

from tests import export_reference as er
from tests import util

pytestmark = pytest.mark.gpu

PAD = 64        # sentinel rows past the largest total of a case: every position the kernel could write to is inside the tensor


class Streams:
    """Three point and three colour buffers of `rows` rows filled with the sentinel; export_compact sees their first `cap`."""

    def __init__(self, dev, rows, cap=None, start=(0, 0, 0)):
        self.rows, self.cap = rows, rows if cap is None else cap
        assert self.cap <= rows
        self.points = [torch.full((rows, 3), er.SENTINEL, device=dev) for _ in range(3)]
        self.colors = [torch.full((rows, 4), er.SENTINEL, device=dev) for _ in range(3)]
        self.counts = torch.tensor(list(start), dtype=torch.int64, device=dev)
        self.start = list(start)
        self.worst = 0.0

    def call(self, K, dev, density, rgb, logit, positions=None, lat=None, ray_begin=0, n_rays=0):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        K.export_compact(lat, ray_begin, n_rays, None if positions is None else t(positions), t(density), t(rgb), t(logit),
                         [p[:self.cap] for p in self.points], [c[:self.cap] for c in self.colors], self.counts)

    def check(self, refs, bound):
        """refs: the reference results of the calls so far, in order.  Asserts counts, rows and sentinels of every set."""
        torch.cuda.synchronize()
        counts = self.counts.tolist()
        for s in range(3):
            idx_n = sum(r["sets"][s]["idx"].size for r in refs)
            assert counts[s] == self.start[s] + idx_n, f"set {s}: count {counts[s]}, reference {self.start[s]} + {idx_n}"
            want_p = np.concatenate([r["sets"][s]["points"] for r in refs])
            want_c = np.concatenate([r["sets"][s]["rgb"] for r in refs])
            want_a = np.concatenate([r["sets"][s]["alpha"] for r in refs])
            lo, hi = self.start[s], min(counts[s], self.cap)
            n = max(hi - lo, 0)
            got_p, got_c = self.points[s].cpu(), self.colors[s].cpu()
            assert torch.equal(got_p[lo:lo + n], torch.from_numpy(want_p[:n])), f"set {s}: points differ"
            assert torch.equal(got_c[lo:lo + n, :3], torch.from_numpy(want_c[:n])), f"set {s}: rgb differs"
            alpha = got_c[lo:lo + n, 3].numpy()
            if s == 2:
                assert np.all(alpha == np.float32(1.0)), "set 2: sigmoid(density >= 70) is 1"
            else:
                ratio = er.alpha_ratio(alpha, want_a[:n])
                self.worst = max(self.worst, ratio)
                assert ratio <= bound, f"set {s}: channel 3 off by {ratio:.3f} u s, granted {bound:.3f}"
            end = max(hi, lo)
            for name, got in (("points", got_p), ("colors", got_c)):
                assert bool((got[:min(lo, self.rows)] == er.SENTINEL).all()), f"set {s}: {name} written below the start"
                assert bool((got[end:] == er.SENTINEL).all()), \
                    f"set {s}: {name} written at or past min(count, cap) = {end} (cap {self.cap})"
        return counts


@pytest.fixture(scope="module")
def bound():
    cpu = er.alpha_yardstick()
    print(f"[export channel 3] float32 CPU worst |err| / (u s) = {cpu:.3f}; granted to the kernel: {4 * cpu:.3f}")
    return 4.0 * cpu


def _one_call(dev, density, rgb, logit, positions, bound, name):
    from fruitnerf_amd import _kernels as K
    ref = er.reference(density, rgb, logit, positions)
    rows = max(r["idx"].size for r in ref["sets"]) + PAD
    st = Streams(dev, rows)
    st.call(K, dev, density, rgb, logit, positions)
    counts = st.check([ref], bound)
    print(f"[export {name}] counts {counts}, channel 3 worst |err| / (u s) = {st.worst:.3f}")
    return ref, st


@pytest.mark.parametrize("N", er.SIZES)
def test_sizes_against_the_reference(dev, bound, N):
    """Random inputs, 30 % pass the density cut; the two largest sizes take the scan's loop a second and a third time."""
    _one_call(dev, *er.make_inputs(N, "random", seed=er.RANDOM_SEED), bound, f"random N={N}")


@pytest.mark.parametrize("N", er.PATTERN_SIZES)
@pytest.mark.parametrize("pattern", er.PATTERNS)
def test_selection_patterns_against_the_reference(dev, bound, pattern, N):
    ref, st = _one_call(dev, *er.make_inputs(N, pattern, seed=2), bound, f"{pattern} N={N}")
    if pattern == "none":
        assert st.counts.tolist() == [0, 0, 0]
        assert all(bool((b == er.SENTINEL).all()) for b in st.points + st.colors)


def test_threshold_edges(dev, bound):
    """density in {70-, 70, 70+, NaN, +-inf, 0, -1} x logit in {3-, 3, 3+, ln 9 -+ 2e-5, ln 9 -+ 1e-3, NaN, +-inf, +-100}."""
    density, rgb, logit, positions = er.make_edge_inputs()
    ref, st = _one_call(dev, density, rgb, logit, positions, bound, "edges")
    assert [r["idx"].size for r in ref["sets"]] == [3 * 7, 3 * 4, 3 * 12]      # logit >= 3: {3, 3+, +inf, 100}
    for s in (0, 1):                    # logit = +inf: in both semantic sets, channel 3 exactly 1
        at_inf = np.isposinf(logit[ref["sets"][s]["idx"]])
        assert at_inf.sum() == 3
        assert np.all(st.colors[s].cpu().numpy()[:at_inf.size, 3][at_inf] == np.float32(1.0))


def _running_inputs():
    return [er.make_inputs(N, "random", seed=10 + i) for i, N in enumerate(er.RUNNING_SIZES)]


def test_running_totals_append_from_nonzero_counts(dev, bound):
    """Four calls (one of them empty) into the same buffers and counts, from counts = [5, 0, 17]: the rows below the initial
    counts keep the sentinel, the rows from there on are the four reference lists back to back."""
    from fruitnerf_amd import _kernels as K
    calls = _running_inputs()
    refs = [er.reference(*c) for c in calls]
    total = [er.RUNNING_START[s] + sum(r["sets"][s]["idx"].size for r in refs) for s in range(3)]
    st = Streams(dev, max(total) + PAD, start=er.RUNNING_START)
    for i, (density, rgb, logit, positions) in enumerate(calls):
        st.call(K, dev, density, rgb, logit, positions)
        st.check(refs[:i + 1], bound)
    assert st.counts.tolist() == total and min(r["sets"][0]["idx"].size for r in refs if r["flags"].shape[1]) > 0


def test_capacity_guard(dev, bound):
    """cap in {max(c), max(c) - 1, min(c), 1}: counts report the full totals, the first min(c[s], cap) rows are right, nothing
    at or past cap is written (the tail of the tensor behind the view takes every position the kernel could reach)."""
    from fruitnerf_amd import _kernels as K
    density, rgb, logit, positions = er.make_inputs(er.CAPACITY_N, "random", seed=3)
    ref = er.reference(density, rgb, logit, positions)
    c = [r["idx"].size for r in ref["sets"]]
    assert 1 < min(c) < max(c) - 1
    for cap in (max(c), max(c) - 1, min(c), 1):
        st = Streams(dev, max(c) + PAD, cap=cap)
        st.call(K, dev, density, rgb, logit, positions)
        assert st.check([ref], bound) == c, cap


def test_capacity_overflow_in_the_third_call_of_a_sequence(dev, bound):
    """The running sequence with a capacity that sets 0 and 1 stay under while set 2 passes it in the third call; the fourth
    call, entirely past the capacity in set 2, still counts and still appends to sets 0 and 1."""
    from fruitnerf_amd import _kernels as K
    calls = _running_inputs()
    refs = [er.reference(*c) for c in calls]
    after = [[er.RUNNING_START[s] + sum(r["sets"][s]["idx"].size for r in refs[:i + 1]) for s in range(3)] for i in range(4)]
    cap = (after[1][2] + after[2][2]) // 2
    assert after[1][2] < cap < after[2][2] and max(after[3][0], after[3][1]) < cap
    st = Streams(dev, max(after[3]) + PAD, cap=cap, start=er.RUNNING_START)
    for i, (density, rgb, logit, positions) in enumerate(calls):
        st.call(K, dev, density, rgb, logit, positions)
        assert st.check(refs[:i + 1], bound) == after[i]


@pytest.mark.parametrize("name,shape,ray_begin,n_rays", er.lattice_cases(), ids=[c[0] for c in er.lattice_cases()])
def test_lattice_path(dev, bound, name, shape, ray_begin, n_rays):
    """Implicit positions (xs[ix], ys[iy], zs[k]): equal to the reference's index arithmetic bit for bit, and the whole result
    equal to the positions path fed with the materialised positions."""
    from fruitnerf_amd import _kernels as K
    xs, ys, zs = er.make_lattice(*shape)
    density, rgb, logit, _ = er.make_inputs(n_rays * shape[2], "random", seed=4)
    ref = er.reference(density, rgb, logit, lattice=(xs, ys, zs, ray_begin))
    assert ref["sets"][0]["idx"].size > 0
    lat = K.LatticeArg(torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev), torch.from_numpy(zs).to(dev))
    rows = ref["sets"][2]["idx"].size + PAD
    a, b = Streams(dev, rows), Streams(dev, rows)
    a.call(K, dev, density, rgb, logit, lat=lat, ray_begin=ray_begin, n_rays=n_rays)
    a.check([ref], bound)
    b.call(K, dev, density, rgb, logit, positions=er.lattice_positions(xs, ys, zs, ray_begin, n_rays))
    b.check([ref], bound)
    assert torch.equal(a.counts, b.counts)
    for s in range(3):
        assert torch.equal(a.points[s], b.points[s]) and torch.equal(a.colors[s], b.colors[s])


def test_lattice_ray_range_past_the_end_is_an_error(dev):
    from fruitnerf_amd import _kernels as K
    xs, ys, zs = er.make_lattice(*er.LATTICE)
    lat = K.LatticeArg(torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev), torch.from_numpy(zs).to(dev))
    n_rays = 25                                     # 11 + 25 = 36 > 7 * 5
    density, rgb, logit, _ = er.make_inputs(n_rays * er.LATTICE[2], "random", seed=4)
    st = Streams(dev, density.size + PAD)
    with pytest.raises(RuntimeError, match="ray range outside lattice"):
        st.call(K, dev, density, rgb, logit, lat=lat, ray_begin=11, n_rays=n_rays)
    torch.cuda.synchronize()
    assert st.counts.tolist() == [0, 0, 0] and all(bool((b == er.SENTINEL).all()) for b in st.points + st.colors)


@pytest.fixture(scope="module")
def export_pipe(dev):
    """The small model and lattice of test_export_counts_and_points_identical (tests/test_gpu_forward_parity.py)."""
    from fruitnerf_amd.data.fruit_datamanager import ExportDataManager
    cfg = util.small_config(log2=15)
    om = util.make_oracle(cfg, seed=4, test_mode="export")
    util.randomize_(om, 9, density_boost=3.0)
    om.field.test_mode = "export"
    aabb = ((-1.0, -0.6, -1.0), (1.0, 0.6, 1.0))
    util.straddle_export_thresholds(om, aabb)
    om.eval()
    hm = util.make_hip_like(om, dev, test_mode="export")
    hm.eval()

    def make(fused, N=40):
        class Pipe:
            pass
        pipe = Pipe()
        pipe.model = hm
        pipe.datamanager = ExportDataManager(dev, eval_num_rays_per_batch=333)
        hm.setup_inference(True, N, deterministic=True)
        num_rays = pipe.datamanager.setup_inference(aabb=aabb, num_points=N)
        if not fused:
            pipe.datamanager.export_lattice = None
        return pipe, num_rays
    return make


@pytest.mark.parametrize("fused", [True, False])
def test_sample_volume_regrows_its_buffers(dev, export_pipe, monkeypatch, fused):
    """sample_volume started with 64 rows per stream (INITIAL_CAPACITY) returns exactly the arrays of the run with the
    default capacity: the fused path repeats its whole pass with larger buffers, the generic path repeats the batch."""
    from fruitnerf_amd import _kernels as K
    from fruitnerf_amd.export import exporter_utils as eu
    assert eu.INITIAL_CAPACITY == 1 << 20
    caps = []
    real = K.export_compact

    def counted(lat, ray_begin, n_rays, positions, density, rgb, logit, points, colors, counts):
        caps.append(points[0].shape[0])
        return real(lat, ray_begin, n_rays, positions, density, rgb, logit, points, colors, counts)
    monkeypatch.setattr(K, "export_compact", counted)
    pipe, num_rays = export_pipe(fused)
    want = eu.sample_volume(pipe, num_rays, transform_json={"scale": 0.7})
    calls_default, caps_default = len(caps), set(caps)
    del caps[:]
    monkeypatch.setattr(eu, "INITIAL_CAPACITY", 64)
    pipe, num_rays = export_pipe(fused)
    got = eu.sample_volume(pipe, num_rays, transform_json={"scale": 0.7})
    largest = max(want[name]["points"].shape[0] for name in eu.SET_NAMES)
    print(f"[export regrow fused={fused}] {calls_default} calls at {sorted(caps_default)} rows; from 64 rows: {len(caps)} calls, "
          f"capacities {sorted(set(caps))}; largest set {largest} points")
    assert caps_default == {1 << 20} and largest > 64
    assert caps[0] == 64 and len(caps) > calls_default and max(caps) > 64      # grown, and something was repeated
    assert all(c == 64 << int(np.log2(c // 64)) for c in caps)                 # by doubling
    for name in eu.SET_NAMES:
        assert want[name]["points"].shape[0] > 0, name
        assert np.array_equal(got[name]["points"], want[name]["points"]), name
        assert np.array_equal(got[name]["colors"], want[name]["colors"]), name
