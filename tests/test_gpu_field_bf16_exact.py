"""The plain bf16 field MLP kernels (mlp_mode 1: the NS = 1 instantiations of field_bf16.hpp / field_mlp_bf16.hip /
field_mlp_bwd_pw.hip, `fruit_nerf_big`'s cooperative semantic branch, bf_build_T, BR_SEM_DX) held to their contract BIT FOR BIT:
acc = bias (fp32), both operands rounded to bf16 (round to nearest even), fp32 accumulate.  tests/test_gpu_bf16.py compares this
mode with the fp32 kernels at 3e-2 .. 2e-1 of a batch maximum and 20 % L2 per tensor; here every element is compared.

How: on dyadic ("lattice") networks and batches (field_reference.make_lattice_net / make_lattice_batch: weights of one or two
bits, features in multiples of 1/8 — variant "b": of 1/512 with coarser weights, so that the first two layers' conversions
round and tie as well —, biases and upstream gradients in multiples of 1/4, zero SH columns, an embedding in multiples of 1/64)
every partial sum of every accumulation is a float32 number in whatever order it is formed, so any correct accumulator returns
the exact value and a float64 reference that rounds the same operands must agree bit for bit.  The comment above
field_reference.round8 says where the kernels round, where each bias gradient is formed, where the saved h is reused and what is
recomputed; tests/test_field_bf16_exact_cpu.py asserts the preconditions (the exactness condition for every accumulation of
every sample of every case here, that the conversions do round and tie, the guard's share) and that seven mutations of the
emulation are caught.

Forward (bf16): h, geo_out, logit and ray_bias torch.equal to the rounded-operand reference, rows with the selector false
included, train and eval path; density and rgb against float64 exp / sigmoid of the EXACT h0 / c3 (3 u relative;
2 u s (1 - s) + 2 u s).  Forward (fp32, bf16x3), same inputs: torch.equal to the UNROUNDED float64 result (weights of <= 3 bits:
w2 = w3 = 0, the six kept piece products are the whole product).  No sample is left out of a forward comparison.
Backward (bf16; plain, semgrad at (7,40) and (21,8), and into a pre-filled arena): d_feats torch.equal; a weight, bias or
embedding entry whose own sum satisfies the condition torch.equal, every other one within (n - 1) 2^-23 sum|addends| — the
worst case of any summation order, doubled because it is not documented whether the matrix pipe's accumulator rounds or
truncates (an assumption).  d_c3 and d_h0 come out of a transcendental: the reference forms them in float32, in the kernel's
order, from the RETURNED rgb and density, and a sample whose value would round to another bf16 under +-2 ulp gets that upstream
row zeroed (at most 1 %, none below N = 100; printed).

MI355X, first device run (nothing is tuned from these).  Every forward and backward comparison passed as written; samples
guarded: 1 of 280 at `fruit_nerf`/a (7,40), 0 everywhere else; no sample left out of a forward comparison.  Forward, all
three arithmetics, grid-stride case (N = 131 159) included: worst |err| / bound density 0.43, rgb 0.73.  Backward, per tensor
class, [worst |err| / bound of the entries under the bound; share of the non-empty entries compared exactly]:
  tensor      plain, every case (4 shape x variant)   semgrad                        into a pre-filled arena
  d_feats     equal                                   equal                          equal
  base W      [0.023;  0.56 - 0.95]                   [0.0016; 0.29 - 0.93]          [0.0027;  0.06 - 0.07]
  base b      [0.024;  0.77 - 0.99]                   [0.0010; 0.52 - 0.99]          [0.0011;  0.04]
  sem W       [0;      1.00]                          [0;      1.00]                 [0.0035;  0.41 - 0.44]
  sem b       [0;      1.00]                          [0;      1.00]                 [0.0030;  0.25 - 0.34]
  col W       [0.55;   0.61 - 0.69]                   [0.028;  0.47 - 0.60]          [0.011;   0.31 - 0.32]
  col b       [0.021;  0.97]                          [0.0006; 0.97]                 [0.0022;  0.26 - 0.27]
  embedding   [0;      0.82 - 1.00]                   [0;      0.72 - 1.00]          [0.00007; 0.23]
(col W's 0.55 is the same in all four networks, which share the directions: consistent with the one rounded product of an SH
column of col0 at R = 1, n = 2 in its bound; the other col W entries stay below 0.03.  A pre-filled entry is
exact only where the 0.05 randn prefill happens to share the sum's bits, hence the small shares of the last column.)  Every
test takes under a second.
"""
import pytest
import torch

from tests import field_reference as fr
from tests.test_gpu_field_kernels import CLAMP, MODE_ID, Device   # noqa: F401  (CLAMP, MODE_ID: the shared device side)

pytestmark = pytest.mark.gpu

EXACT_FWD = ("h_pad", "geo_out", "logit", "ray_bias")
_REF = {}


def _reference(shape, R, S, variant, arith, mean=None):
    """The float64 forward of a lattice case (rounded operands: "bf16"; unrounded: "f64"), computed once."""
    key = (shape, R, S, variant, arith, None if mean is None else tuple(mean.tolist()))
    if key not in _REF:
        if len(_REF) > 24:
            _REF.clear()
        c = fr.prepare_lattice(shape, R, S, variant)
        with torch.no_grad():
            _REF[key] = fr.forward(c["net"], c["batch"], fr.Arith(arith), mean_embedding=mean)
    return _REF[key]


def _check_forward(name, got, f, batch, worst):
    want = fr.exact_outputs(f)
    for k in EXACT_FWD:
        if k in got:
            bad = int((got[k] != want[k]).sum())
            assert torch.equal(got[k], want[k]), f"{name}: {k}: {bad} of {want[k].numel()} entries differ from the exact value"
    assert torch.equal(got["density"] != 0, batch["sel"]), f"{name}: the density is 0 at the unselected samples and only there"
    for k, v in fr.transcendental_ratios(got, f, batch["sel"]).items():
        worst[k] = max(worst.get(k, 0.0), v)
        assert v <= 1.0, f"{name}: {k}: worst |err| / bound = {v:.3g}"


def _lattice_mean():
    g = torch.Generator().manual_seed(8)
    return torch.randint(-48, 49, (32,), generator=g).float() / 64.0


@pytest.mark.parametrize("mode", ["bf16", "fp32", "bf16x3"])
@pytest.mark.parametrize("variant", fr.LATTICE_VARIANTS)
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_forward_is_exact(dev, shape, variant, mode):
    """Every case of fr.CASES, train path and eval path (mean_embedding: zeros and a lattice vector; want_h on and off):
    bf16 against the rounded-operand reference, fp32 and bf16x3 against the unrounded one."""
    arith = "bf16" if mode == "bf16" else "f64"
    worst = {}
    for R, S in fr.CASES:
        c = fr.prepare_lattice(shape, R, S, variant)
        D = Device(dev, c["net"], c["batch"], mode)
        name = f"{shape}/{variant}[{R}x{S},{mode}]"
        got, _ = D.forward()
        _check_forward(name, got, _reference(shape, R, S, variant, arith), c["batch"], worst)
        if (R, S) in ((7, 40), (37, 1)):
            for mean in (torch.zeros(32), _lattice_mean()):
                f = _reference(shape, R, S, variant, arith, mean)
                for want_h in (True, False):
                    ev, _ = D.forward(mean_embedding=mean, want_h=want_h)
                    _check_forward(name + " eval", ev, f, c["batch"], worst)
    print(f"[bf16 exact] forward {shape}/{variant} {mode}: worst |err| / bound of the transcendentals {worst}")


@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_forward_grid_stride(dev, shape):
    """N = R x 41 just above 512 x CUs (field_reference.grid_stride_shape), odd, forward only, variant "b": every forward
    kernel's grid-stride loop makes whole passes and a ragged last one; the three arithmetics against two float64 forwards."""
    from fruitnerf_amd import _lib as L
    R, S, passes = fr.grid_stride_shape(int(L.device_check()["cus"]))
    N = R * S
    assert N % 16 != 0 and all(N > p and N % p != 0 for p in passes.values()), (N, passes)
    c = fr.prepare_lattice(shape, R, S, "b")
    worst = {}
    for mode in ("bf16", "fp32", "bf16x3"):
        got, _ = Device(dev, c["net"], c["batch"], mode).forward()
        _check_forward(f"{shape}/b[{R}x{S},{mode}]", got, _reference(shape, R, S, "b", "bf16" if mode == "bf16" else "f64"),
                       c["batch"], worst)
    print(f"[bf16 exact] grid-stride {shape}: N = {N}, worst |err| / bound of the transcendentals {worst}")


def _backward_case(dev, shape, R, S, variant, semgrad, prefill, total):
    c = fr.prepare_lattice(shape, R, S, variant)
    net, batch, N = c["net"], c["batch"], R * S
    name = f"{shape}/{variant}[{R}x{S}{',semgrad' if semgrad else ''}{',prefill' if prefill else ''}]"
    D = Device(dev, net, batch, "bf16", prefill=prefill)
    got_f, saved = D.forward()
    _check_forward(name, got_f, _reference(shape, R, S, variant, "bf16"), batch, {})
    up, guarded = fr.guard(c["up"], got_f["density"], got_f["rgb"])
    n_g = int(guarded.sum())
    print(f"[bf16 exact] {name}: {n_g} of {N} samples guarded")
    assert n_g <= 0.01 * N and (N >= 100 or n_g == 0), f"{name}: {n_g} of {N} samples guarded"
    got = D.backward(saved, up, semgrad=semgrad)
    _, ref = fr.bf16_backward(net, batch, up, fr.Arith("bf16"), semgrad, returned=(got_f["density"], got_f["rgb"]))
    res = fr.exact_compare(net, got, ref, prefill=D.pre if prefill else None)
    for k, v in res.items():
        cls = k if k in ("d_feats", "embedding") else fr._class(k)
        t = total.setdefault(cls, dict(compared=0, exact=0, ratio=0.0))
        t["compared"], t["exact"], t["ratio"] = t["compared"] + v["compared"], t["exact"] + v["exact"], max(t["ratio"], v["ratio"])
    fails = fr.exact_failures(res)
    assert not fails, f"{name}: (exactly compared entries that differ, worst |err| / bound of the others) {fails}"
    emb = got["embedding"] if not prefill else got["embedding"] - D.pre["embedding"]
    assert float(emb[fr.UNUSED_CAM].abs().max()) == 0.0, f"{name}: the embedding row of an image no ray has seen"
    silent = (up["dd"] == 0) & (up["dl"] == 0) & (up["dr"] == 0).all(1)
    assert float(got["d_feats"][:, silent].abs().max() if silent.any() else 0.0) == 0.0, f"{name}: d_feats without upstream gradient"
    return got


def _report(what, total):
    for k, t in sorted(total.items()):
        print(f"[bf16 exact] {what} {k}: worst |err| / bound = {t['ratio']:.3g}, exactly compared {t['exact']} of {t['compared']}"
              f" = {t['exact'] / max(t['compared'], 1):.2f}")


@pytest.mark.parametrize("variant", fr.LATTICE_VARIANTS)
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_backward_is_exact(dev, shape, variant):
    """Every case of fr.CASES: d_feats per sample and level, every weight, bias and embedding entry."""
    total = {}
    for R, S in fr.CASES:
        _backward_case(dev, shape, R, S, variant, False, False, total)
    _report(f"backward {shape}/{variant}", total)


@pytest.mark.parametrize("variant", fr.LATTICE_VARIANTS)
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_semgrad_backward_is_exact(dev, shape, variant):
    """semgrad=True at (7,40) and (21,8): BR_SEM_DX (`fruit_nerf`) and the fifth phase of the cooperative kernel
    (`fruit_nerf_big`, bf_build_T) add the semantic input gradient into d_h: d_feats and the base layers change and stay exact."""
    total = {}
    for R, S in fr.SEMGRAD_CASES:
        got = _backward_case(dev, shape, R, S, variant, True, False, total)
        plain = _backward_case(dev, shape, R, S, variant, False, False, {})
        assert not torch.equal(got["d_feats"], plain["d_feats"]) and not torch.equal(got["base0"][0], plain["base0"][0])
    _report(f"semgrad {shape}/{variant}", total)


@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_gradients_are_added_to_a_prefilled_arena(dev, shape):
    """Every gradient tensor pre-filled with 0.05 randn, (7,40) and (9,16), variant "a": the prefill is one more addend of every
    entry's sum; the unused image's row keeps its prefill bit for bit."""
    total = {}
    for R, S in ((7, 40), (9, 16)):
        _backward_case(dev, shape, R, S, "a", False, True, total)
    _report(f"prefill {shape}", total)
