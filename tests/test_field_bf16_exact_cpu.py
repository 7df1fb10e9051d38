"""The lattice inputs and the plain bf16 emulation of tests/field_reference.py checked on the reference alone, without a GPU:
what tests/test_gpu_field_bf16_exact.py relies on before it may ask a device for identical bits.

  * round8("rne") is torch.bfloat16's rounding, ties included;
  * for every case of the GPU file, both shapes, both lattice variants: every forward accumulation of every sample satisfies
    the exactness condition (log2 sum|addends| - lowest set bit < 24) in all three arithmetics (bf16 operands; unrounded
    operands = fp32; the bf16x3 pieces, with w2 = w3 = 0), every accumulation of the dX chain does with bf16 operands (plain,
    and semgrad at its cases), the guard leaves out at most 1 % (none below N = 100), at least 25 % of every layer's
    weight-gradient entries are compared, and the conversions round (>= 10 % of the nonzero inputs of every layer, >= 100
    exact ties at the largest non-grid case: variant "b" in every layer, variant "a" from the third layer of a branch on,
    whose first two see features in multiples of 1/8);
  * a float32 evaluation of the same rounded operands (torch's own order of summation) returns the float64 values bit for
    bit: the condition does what it says;
  * every mutation of the emulation that stands for a real mistake breaks an exact comparison or exceeds a bound at (21, 8).
"""
import pytest
import torch

from tests import field_reference as fr

GRID = fr.grid_stride_shape(4)[:2]
LARGEST = (3, 129)


def _pieces_entry(e):
    """A traced float64 forward accumulation as the bf16x3 kernels form it: the three pieces of x against w1 (w2 = w3 = 0)."""
    xs, ws = fr._split(e["x"].float()), fr._split(e["w"].float())
    assert float(ws[1].abs().max()) == 0.0 and float(ws[2].abs().max()) == 0.0, "weights of at most 8 bits: w2 = w3 = 0"
    assert torch.equal((xs[0].double() + xs[1].double() + xs[2].double()), e["x"])
    return dict(e, x=torch.cat([p.double() for p in xs], 1), w=torch.cat([ws[0].double()] * 3, 1))


def _assert_bits(what, entries):
    for kind, layer, bits in entries:
        assert bool((bits < 24.0).all()), f"{what}: {kind} {layer}: {int((bits >= 24).sum())} accumulations, worst {float(bits.max()):.1f} bits"
    return max(float(b.max()) for _, _, b in entries)


@pytest.mark.parametrize("rule", ["rne"])
def test_round8_is_torch_bfloat16(rule):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(20000, generator=g, dtype=torch.float64).float()
    ties = (torch.randint(-2 ** 9, 2 ** 9, (4000,), generator=g) * 2 + 1).float() * 2.0 ** torch.randint(-12, 4, (4000,), generator=g)
    x = torch.cat([x, ties, torch.zeros(3)])
    assert torch.equal(fr.round8(x, rule), x.bfloat16().float())
    assert torch.equal(fr.lowbit(torch.tensor([0.75, -3.0, 2.0 ** -20, 0.0])), torch.tensor([-2.0, 0.0, -20.0, fr.BIG_LB], dtype=fr.F8))


@pytest.mark.parametrize("variant", fr.LATTICE_VARIANTS)
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_the_lattice_holds_the_edges(shape, variant):
    """Zero SH columns, a lattice embedding and ray_bias, some selector rows false, an all-zero feature row, LONE_CAM on one ray
    and UNUSED_CAM on none, h0 inside the clamp."""
    c = fr.prepare_lattice(shape, 7, 40, variant)
    net, b = c["net"], c["batch"]
    assert float(net["col0"][0][:, :16].abs().max()) == 0.0
    assert 0.05 < float((~b["sel"]).float().mean()) < 0.25 and float(b["feats"][:, 3].abs().max()) == 0.0
    assert int((b["cam"] == fr.LONE_CAM).sum()) == 1 and int((b["cam"] == fr.UNUSED_CAM).sum()) == 0
    q = 8 if variant == "a" else 512
    assert torch.equal((b["feats"] * q).round(), b["feats"] * q) and float(b["feats"].abs().max()) == 0.75
    with torch.no_grad():
        f = fr.forward(net, b, fr.Arith("bf16"))
    assert torch.equal((f["ray_bias"] * 256).round(), f["ray_bias"] * 256) and float(f["h"][:, 0].abs().max()) < 15.0
    for k in ("dd", "dr", "dl"):
        assert torch.equal((c["up"][k] * 4).round(), c["up"][k] * 4)


@pytest.mark.parametrize("case", fr.CASES + [GRID], ids=lambda c: "%dx%d" % c)
@pytest.mark.parametrize("variant", fr.LATTICE_VARIANTS)
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_preconditions(shape, variant, case):
    R, S = case
    c = fr.prepare_lattice(shape, R, S, variant)
    net, batch, N = c["net"], c["batch"], R * S
    name = f"{shape}/{variant} {R}x{S}"
    # forward, three arithmetics
    worst = {}
    for arith in ("bf16", "f64"):
        ar = fr.Arith(arith, trace=True)
        with torch.no_grad():
            f = fr.forward(net, batch, ar)
        worst[arith] = _assert_bits(f"{name} forward {arith}", fr.exactness(ar.log))
        fr.exact_outputs(f)
        if arith == "f64":
            worst["bf16x3"] = _assert_bits(f"{name} forward bf16x3", fr.exactness([_pieces_entry(e) for e in ar.log]))
        else:
            # a float32 accumulator in torch's order returns the same bits
            a4 = fr.Arith("bf16")
            a4.dtype = fr.F4
            with torch.no_grad():
                f4 = fr.forward(net, batch, a4)
            for k in ("h", "logit", "c3", "ray_bias"):
                assert torch.equal(f4[k].double(), f[k]), f"{name}: float32 evaluation of {k}"
    print(f"[bf16 exact cpu] {name}: forward bits (worst) {worst}")
    if case == GRID:
        return                                                            # forward only on the device
    # the dX chain, the guard, the weight-gradient coverage
    for semgrad in ([False, True] if case in fr.SEMGRAD_CASES else [False]):
        ar = fr.Arith("bf16", trace=True)
        with torch.no_grad():
            f = fr.forward(net, batch, fr.Arith("bf16"))
        up, guarded = fr.guard(c["up"], (torch.exp(f["h"][:, 0]) * batch["sel"].double()).float(), f["rgb"].float())
        n_g = int(guarded.sum())
        assert n_g <= 0.01 * N and (N >= 100 or n_g == 0), f"{name}: {n_g} of {N} samples guarded"
        f, out = fr.bf16_backward(net, batch, up, ar, semgrad)
        chain = [e for e in fr.exactness(ar.log) if e[0] != "fwd"]
        w = _assert_bits(f"{name} dX chain semgrad={semgrad}", chain)
        res = fr.exact_compare(net, fr.sums_to_tensors(out), out)
        assert not fr.exact_failures(res)
        for k in fr.layer_names(shape):
            r = res[k + ".w"]
            assert r["compared"] >= 0.25 * r["entries"] or N < 100, f"{name}: {k}: {r}"
        share = {k: round(v["exact"] / max(v["compared"], 1), 2) for k, v in res.items() if k.endswith(".w")}
        print(f"[bf16 exact cpu] {name} semgrad={semgrad}: guarded {n_g} of {N}, dX chain worst {w:.1f} bits, exact share of dW {share}")
        if N >= 100 and not semgrad:
            st = fr.rounding_stats(ar.log)
            first_two = {"base0", "base1"}
            for (kind, layer), (nz, changed, ties) in st.items():
                if kind != "fwd" or (variant == "a" and layer in first_two):
                    continue
                assert changed >= 0.10 * nz, f"{name}: the conversion of {layer}'s input changes {changed} of {nz}"
                if case == LARGEST:
                    assert ties >= 100, f"{name}: {layer}: {ties} exact ties"


def _emulate(c, up, semgrad=False, **kw):
    mut = kw.pop("mut", ())
    ar = fr.Arith("bf16", **kw)
    return fr.bf16_backward(c["net"], c["batch"], up, ar, semgrad, mut)


MUTATIONS = {
    "truncate instead of round to nearest even": dict(rule="trunc"),
    "round half away from zero": dict(rule="away"),
    "the bias through the convert": dict(mut=("bias_converted",)),
    "one layer's input left unrounded": dict(mut=(("unrounded_input", "col1"),)),
    "two K-slots of one 16 x 32 weight block swapped": dict(mut=(("swap_slots", "col1"),)),
    "a 16-sample tile dropped from dW": dict(mut=("drop_tile",)),
    "G unrounded in one dW": dict(mut=(("g_unrounded", "col1"),)),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
@pytest.mark.parametrize("variant", fr.LATTICE_VARIANTS)
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_every_mutation_breaks_a_comparison(shape, variant, name):
    """At (21, 8): the mutated emulation, compared the way the device is, differs in a forward quantity that must be equal,
    differs in an exactly compared gradient entry, or exceeds a bound."""
    c = fr.prepare_lattice(shape, 21, 8, variant)
    with torch.no_grad():
        f0 = fr.forward(c["net"], c["batch"], fr.Arith("bf16"))
    up, _ = fr.guard(c["up"], (torch.exp(f0["h"][:, 0]) * c["batch"]["sel"].double()).float(), f0["rgb"].float())
    f, ref = _emulate(c, up)
    spec = dict(MUTATIONS[name])
    mut = spec.get("mut", ())
    fm, gm = fr.bf16_backward(c["net"], c["batch"], up, fr.Arith("bf16", rule=spec.get("rule", "rne"), mut=mut), False,
                              tuple(m for m in mut if isinstance(m, str)))
    fwd_diff = [k for k in ("h", "logit", "c3") if not torch.equal(fm[k], f[k])]
    fails = fr.exact_failures(fr.exact_compare(c["net"], fr.sums_to_tensors(gm), ref))
    print(f"[bf16 exact cpu mutation {shape}/{variant}] {name}: forward {fwd_diff}, backward {fails}")
    assert fwd_diff or fails, name
    if "dW" in name:
        assert fails and not fwd_diff
