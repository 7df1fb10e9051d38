"""The field MLP's kernels — K.field_mlp_fwd, K.field_mlp_bwd (plain, jacobian=, semgrad=True) and K.embedding_mean, i.e.
field_mlp.hip, field_mlp_bf16.hip, field_mlp_bwd.hip, field_mlp_bwd_pw.hip — against the float64 reference of
tests/field_reference.py (plain torch, not oracle/ns_torch.py's float32 path): per sample, per weight entry and per embedding
row, never against a batch or tensor maximum, for both built shapes (`fruit_nerf`: geo 15, semantic 2 x 64; `fruit_nerf_big`:
geo 30, semantic 3 x 128) in the fp32 and bf16x3 arithmetics.  Plain bf16 gets the structural assertions here; its numerics are
held bit for bit to the rounded-operand reference on lattice inputs by tests/test_gpu_field_bf16_exact.py.

Isolation: the features [16][N][2] (uniform in +-0.8 + an all-zero row and rows of extremes), the selector, directions and
cameras are generated on the CPU; the network is raw tensors behind an fnr_field_net (Kaiming-uniform weights, non-zero biases
and embedding).  The reference upcasts the same float32 values.

Error model, bounds and what is saved / recomputed: the docstring of tests/field_reference.py.  In short every bound is
c (u_mode scale + propagated error) with scale the float64 sum of |terms| the kernel adds up for the element — an ESTIMATE,
not a worst-case bound: roundings are taken as independent: a chain of k accumulations enters as sqrt(k) u, propagated errors add in quadrature (with the worst
case k u and |W| |e| of five chained layers the margins came out ~100 x the errors and put 2 % of the `fruit_nerf_big` samples
next to a kink); bf16x3 adds the dropped piece products: 2^-23 forward (w2 x3 + w3 x2), 3 * 2^-16 in dX / dW (pieces x1, x2
only; bf16 keeps 8 significant bits, round to nearest leaves 2^-8 per piece) — field_bf16.hpp's 2^-27 / 2^-17 are typical
sizes, the emulation of the split reaches 0.3 of 3 * 2^-16 = 2^-16 of the scale in its worst weight entry.

Excluded by construction: samples with a hidden pre-activation (a1, c1, c2, the hidden layers of mlp_semantics) within
c x its margin of 0, or |h0| within c x its margin of 15, in either arithmetic, get all three upstream gradients zero and
stay in the batch.  < 1 % of N, asserted in every test (none below N = 100); measured 0.14 % (`fruit_nerf`) and 0.24 %
(`fruit_nerf_big`) at the grid-stride size.

The constants c (field_reference.C) are 6 x the worst |err| / bound of the SAME reference evaluated on the CPU in the
kernel's arithmetic — float32, and an emulation of the split with torch.bfloat16 pieces — over these tests' own inputs
(tests/test_field_kernels_cpu.py asserts >= 4 x and <= 32 x): the kernels get that factor for their other order of summation
(MFMA blocks, per-wave tiles, per-workgroup partial images, k_finish_weights).  Worst |err| / (c bound) over every test of
this file, [CPU emulation, MI355X], c as (fp32, bf16x3):
  quantity        c (fp32, bf16x3)   fp32 [CPU, MI355X]   bf16x3 [CPU, MI355X]
  density         (1.3, 0.44)        [0.164, 0.152]       [0.167, 0.464]
  rgb             (0.28, 0.13)       [0.170, 0.301]       [0.167, 0.431]
  logit           (0.42, 0.22)       [0.168, 0.263]       [0.163, 0.303]
  geo_out         (1.7, 0.62)        [0.164, 0.186]       [0.166, 0.387]
  h               (1.7, 0.62)        [0.164, 0.186]       [0.166, 0.401]
  ray_bias        (1.8, 1.8)         [0.170, 0.231]       [0.170, 0.231]
  d_feats         (7.3, 5)           [0.167, 0.167]       [0.168, 0.167]
  base W          (4.2, 2)           [0.165, 0.084]       [0.164, 0.164]
  base b          (1.3, 1.4)         [0.168, 0.124]       [0.166, 0.166]
  sem W           (1.6, 1.9)         [0.169, 0.106]       [0.163, 0.160]
  sem b           (1, 1.9)           [0.173, 0.170]       [0.163, 0.153]
  col W           (0.99, 1.6)        [0.167, 0.166]       [0.162, 0.164]
  col b           (0.35, 1.2)        [0.167, 0.168]       [0.161, 0.161]
  embedding       (0.23, 0.49)       [0.170, 0.136]       [0.168, 0.176]
  d_position      1 (34 u sum|d_feats||J|, against the contraction of the RETURNED d_feats; w exactly 0)   MI355X fp32 0.110, bf16x3 0.062
  embedding_mean  1 ((n + 2) u mean|e|)   MI355X 0.159
rgb: c multiplies s (1 - s) m_c3 only; the roundings of the sigmoid itself, 2 u s (1 - s) + 2 u s, stand outside c (attained
at a saturated sigmoid), and the ratio is (|err| - that)+ / (c s (1 - s) m_c3).  d_feats' c is set by the samples behind a
saturated sigmoid (fl(1 - s) carries s's own rounding).  No pair is more than the granted factor 4 apart: the largest, the
bf16x3 forward quantities at 2.4 - 2.8 x, come from the grid-stride case, whose 131 159 samples (the CPU evaluation has
2091 there) push the maximum of the same error distribution further out.  The float64 reference of that case takes 5 - 8 s
of CPU per variant, shared by both arithmetics: those six tests take 5 - 9 s each, all others about a second.
Grid-stride case: N = R x 41 just above 512 x CUs (field_reference.grid_stride_shape: the largest pass of any kernel, a
multiple of every other), N odd.
"""
import ctypes as C

import pytest
import torch

from tests import field_reference as fr

pytestmark = pytest.mark.gpu

F8, U = fr.F8, fr.U
NUMERIC_MODES = ("fp32", "bf16x3")
ALL_MODES = ("fp32", "bf16x3", "bf16")
MODE_ID = {"fp32": 0, "bf16": 1, "bf16x3": 3}
CLAMP = (("h0_scale", 40.0), ("h0_bias", 3.0))
SAT = (("sat", 20.0),)
SENTINEL = -12345.0


def _K():
    from fruitnerf_amd import _kernels as K
    return K


def _L():
    from fruitnerf_amd import _lib as L
    return L


def _worst(name, v):
    print(f"[field kernels] {name}: worst |err| / bound = {v:.3g}")
    return v


def _assert_worst(name, ratios):
    bad = {k: v for k, v in ratios.items() if not _worst(f"{name}.{k}", v) <= 1.0}
    assert not bad, f"{name}: {bad}"


def _cus():
    return int(_L().device_check()["cus"])


# ---------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------

class Device:
    """A network of field_reference.make_net as an fnr_field_net (+ one over gradient tensors) and a batch on the device."""

    def __init__(self, dev, net, batch, mode, prefill=False):
        K = _K()
        self.dev, self.net, self.batch, self.mode = dev, net, batch, mode
        self.names = fr.layer_names(net["shape"])
        self.par = {k: tuple(t.to(dev).contiguous() for t in net[k]) for k in self.names}
        self.par["embedding"] = net["embedding"].to(dev).contiguous()
        g = torch.Generator().manual_seed(99)
        fill = (lambda t: torch.randn(t.shape, generator=g) * 0.05) if prefill else (lambda t: torch.zeros(t.shape))
        self.pre = {k: tuple(fill(t) for t in net[k]) for k in self.names}
        self.pre["embedding"] = fill(net["embedding"])
        self.grad = {k: tuple(t.to(dev).contiguous() for t in self.pre[k]) for k in self.names}
        self.grad["embedding"] = self.pre["embedding"].to(dev).contiguous()
        self._dummy = torch.zeros(64, device=dev)
        self.c_net, self.c_grad = self._struct(self.par), self._struct(self.grad)
        self.rays = K.RaysArg(torch.zeros(batch["R"], 3, device=dev), batch["dirs"].to(dev), None, None, batch["cam"].to(dev))
        self.feats = batch["feats"].to(dev).contiguous()
        self.sel = batch["sel"].to(torch.uint8).to(dev).contiguous()

    def _struct(self, t):
        L, K = _L(), _K()
        geo, hid = fr.SHAPES[self.net["shape"]]
        n = L.fnr_field_net()
        n.grid = K.make_grid(self._dummy, 16, 4, [16] * 16)      # the MLP kernels only read n_levels
        n.geo_feat_dim, n.hidden_dim, n.hidden_dim_color, n.hidden_dim_semantics = geo, 64, 64, hid[0]
        n.num_layers_semantic, n.semantic_out_dim, n.appearance_dim, n.n_images = len(hid) + 1, 64, 32, fr.N_IMAGES
        n.base_w0, n.base_b0 = (L.ptr(x) for x in t["base0"])
        n.base_w1, n.base_b1 = (L.ptr(x) for x in t["base1"])
        for i in range(len(hid) + 1):
            n.sem_w[i], n.sem_b[i] = (L.ptr(x) for x in t["sem%d" % i])
        n.head_w, n.head_b = (L.ptr(x) for x in t["head"])
        for i in range(3):
            n.col_w[i], n.col_b[i] = (L.ptr(x) for x in t["col%d" % i])
        n.embedding = L.ptr(t["embedding"])
        n.mlp_mode = MODE_ID[self.mode]
        return n

    def forward(self, mean_embedding=None, want_h=True):
        """-> {density, rgb, logit, geo_out, h_pad, ray_bias} on the CPU and the saved tuple."""
        out = _K().field_mlp_fwd(self.c_net, self.rays, self.batch["S"], self.feats, self.sel,
                                 None if mean_embedding is None else mean_embedding.to(self.dev).contiguous(), want_geo=True,
                                 want_h=want_h)
        torch.cuda.synchronize()
        got = dict(density=out[0].cpu(), rgb=out[1].cpu(), logit=out[2].cpu(), geo_out=out[3].cpu())
        saved = out[4] if want_h else None
        if want_h:
            got["h_pad"], got["ray_bias"] = saved[0].cpu(), saved[1].cpu()
        return got, saved

    def backward(self, saved, up, jacobian=None, semgrad=False):
        """-> the gradients on the CPU (what the call ADDED is got - self.pre), d_feats, d_position."""
        for k in self.grad:                                           # back to the prefill: calls can be repeated
            for t, p in zip(self.grad[k] if isinstance(self.grad[k], tuple) else (self.grad[k],),
                            self.pre[k] if isinstance(self.pre[k], tuple) else (self.pre[k],)):
                t.copy_(p)
        dd, dr, dl = (up[k].to(self.dev).contiguous() for k in ("dd", "dr", "dl"))
        out = _K().field_mlp_bwd(self.c_net, self.c_grad, self.rays, self.batch["S"], self.feats, saved, self.sel, dd, dr, dl,
                                 jacobian=jacobian, semgrad=semgrad)
        torch.cuda.synchronize()
        got = {k: tuple(t.cpu() for t in self.grad[k]) for k in self.names}
        got["embedding"] = self.grad["embedding"].cpu()
        got["d_feats"] = (out[0] if jacobian is not None else out).cpu()
        got["d_position"] = out[1].cpu() if jacobian is not None else None
        return got


def _jacobian(batch, dev):
    g = torch.Generator().manual_seed(batch["N"] + 5)
    return torch.randn(16, 3, batch["N"], 2, generator=g).to(dev).contiguous()


def _flat(got):
    """Every gradient of a backward as one list of tensors (bit comparisons)."""
    out = []
    for k, v in got.items():
        if v is not None:
            out += list(v) if isinstance(v, tuple) else [v]
    return out


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(_flat(a) if isinstance(a, dict) else a, _flat(b) if isinstance(b, dict) else b)):
        assert torch.equal(x, y), f"{what}: tensor {i}: {int((x != y).sum())} of {x.numel()} entries differ"


# ---------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------

def _merge(worst, ratios):
    for k, v in ratios.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _check_forward(name, worst, case, mode, got, m=None, f=None):
    batch, f, m = case["batch"], (case["f"] if f is None else f), (case["m"][mode] if m is None else m)
    N, geo = batch["N"], case["net"]["geo"]
    assert got["density"].shape == (N,) and got["rgb"].shape == (N, 3) and got["logit"].shape == (N,), name
    assert got["geo_out"].shape == (N, geo), name
    assert torch.equal(got["density"] != 0, batch["sel"]), f"{name}: the density is 0 at the unselected samples and only there"
    if "h_pad" in got:
        assert got["h_pad"].shape == f["h_pad"].shape and got["ray_bias"].shape == (batch["R"], 64), name
        assert not bool(got["h_pad"][:, 1 + geo:].any()), f"{name}: the padding columns of h"
        assert torch.equal(got["h_pad"][:, 1:1 + geo], got["geo_out"]), f"{name}: geo_out is h[1:1 + geo]"
    r = fr.scaled(fr.forward_ratios(got, f, m), mode)
    _merge(worst, r)


def _check_backward(name, worst, case, mode, got, pre=None, jac=None):
    batch, net = case["batch"], case["net"]
    r = fr.scaled(fr.backward_ratios(net, got, case["ref"], case["b"][mode], prefill=pre), mode)
    _merge(worst, r)
    emb = got["embedding"] if pre is None else got["embedding"] - pre["embedding"]
    assert float(emb[fr.UNUSED_CAM].abs().max()) == 0.0, f"{name}: the embedding row of an image no ray has seen"
    if float(case["ref"]["embedding"][fr.LONE_CAM].abs().max()) > 0.0:
        assert float(emb[fr.LONE_CAM].abs().max()) > 0.0, f"{name}: the embedding row of the image one ray has seen"
    silent = (case["up"]["dd"] == 0) & (case["up"]["dl"] == 0) & (case["up"]["dr"] == 0).all(1)
    assert float(got["d_feats"][:, silent].abs().max() if silent.any() else 0.0) == 0.0, f"{name}: d_feats without upstream gradient"
    assert got["d_feats"].shape == (16, batch["N"], 2), name
    if jac is not None:
        dp = got["d_position"]
        assert dp.shape == (batch["N"], 4) and float(dp[:, 3].abs().max()) == 0.0, f"{name}: d_position[:, 3]"
        ref, scale = fr.position_contract(got["d_feats"], jac.cpu())
        _merge(worst, {"d_position": float(((dp[:, :3].double() - ref).abs() / (fr.C_POS * 34 * U * scale + 1e-300)).max())})


def _cap(case, name):
    n = int(case["kink"].sum())
    print(f"[field kernels] {name}: {n} of {case['batch']['N']} samples excluded")
    assert fr.excluded_share_ok(case), f"{name}: {n} of {case['batch']['N']} samples excluded"


def _run_case(dev, worst, shape, R, S, mode, semgrad=False, which=(1, 1, 1), net_kw=(), jacobian=False, prefill=False):
    """Forward + backward of one case in one arithmetic against the shared float64 reference."""
    case = fr.prepare(shape, R, S, semgrad, which, net_kw)
    name = f"{shape}[{R}x{S},{mode}{',semgrad' if semgrad else ''}]"
    _cap(case, name)
    D = Device(dev, case["net"], case["batch"], mode, prefill=prefill)
    got_f, saved = D.forward()
    _check_forward(name, worst, case, mode, got_f)
    jac = _jacobian(case["batch"], dev) if jacobian else None
    got_b = D.backward(saved, case["up"], jacobian=jac, semgrad=semgrad)
    _check_backward(name, worst, case, mode, got_b, pre=D.pre if prefill else None, jac=jac)
    return case, D, got_f, saved, got_b


# ---------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", NUMERIC_MODES)
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_forward_and_backward_per_sample_and_per_entry(dev, shape, mode):
    """(1,1) (1,17) (37,1) (21,8) (7,40) (9,16) (3,129): N = 1, a tile boundary inside a ray, partial tiles and 32-groups,
    tiles that straddle rays (gsum_extra) and tiles that do not (gsum_tile), a partial 128-batch, one ray over nine tiles.
    Forward: density (relative), rgb, logit, geo_out, h and ray_bias per element, exact zeros at unselected samples and in h's
    padding.  Backward with the Jacobian: d_feats per element, every weight, bias and embedding entry, d_position against the
    contraction of the returned d_feats; exact zeros: the unused image's row, d_feats of samples without upstream gradient."""
    worst = {}
    for R, S in fr.CASES:
        _run_case(dev, worst, shape, R, S, mode, jacobian=True)
    _assert_worst(f"per_sample[{shape},{mode}]", worst)


@pytest.mark.parametrize("mode", NUMERIC_MODES)
@pytest.mark.parametrize("which", [(0, 0, 1), (1, 1, 1)], ids=["isolated", "all"])
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_semgrad_per_sample_and_per_entry(dev, shape, which, mode):
    """semgrad=True at (7,40) and (21,8), the reference not detaching geo: in isolation (d_density = d_rgb = 0: d_feats and the
    base layers come from the semantic loss alone) and with everything non-zero; with the Jacobian."""
    worst = {}
    for R, S in fr.SEMGRAD_CASES:
        case, _, _, _, got = _run_case(dev, worst, shape, R, S, mode, semgrad=True, which=which, jacobian=True)
        assert float(got["d_feats"].abs().max()) > 0 and float(got["base0"][0].abs().max()) > 0
    _assert_worst(f"semgrad[{shape},{mode}]", worst)


@pytest.mark.parametrize("variant", ["plain", "semgrad", "semgrad-isolated"])
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_grid_stride_second_pass(dev, shape, variant):
    """N = R x 41 just above 512 x CUs, odd: every kernel's grid-stride loop makes whole passes and a last ragged one (the
    caps of field_mlp_fwd_launch, fwd_launch_bf16, field_mlp_fwd_sem_big_bf16, field_mlp_bwd_launch and field_mlp_bwd_pw
    times waves and tiles per wave, field_reference.grid_stride_shape; CUs from the library's device info).  Every sample
    and entry is checked (N < 150 000), both arithmetics against one reference."""
    R, S, passes = fr.grid_stride_shape(_cus())
    N = R * S
    assert N % 16 != 0 and all(N > p and N % p != 0 for p in passes.values()), (N, passes)
    assert torch.cuda.get_device_properties(dev).multi_processor_count == _cus()
    print(f"[field kernels] grid-stride: CUs {_cus()}, N = {R} x {S} = {N}; samples per pass {passes}")
    for mode in NUMERIC_MODES:
        worst = {}
        _run_case(dev, worst, shape, R, S, mode, semgrad=variant != "plain",
                  which=(0, 0, 1) if variant == "semgrad-isolated" else (1, 1, 1), jacobian=True)
        _assert_worst(f"grid_stride[{shape},{variant},{mode}]", worst)


@pytest.mark.parametrize("mode", NUMERIC_MODES)
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_the_clamp_of_trunc_exp_and_saturated_colours(dev, shape, mode):
    """base1's density row times 40, bias 3: h0 beyond +15 and beyond -15 on >= 5 % of the samples each, next to >= 20 % well
    inside (asserted on the CPU): the forward density is the unclamped exp, the backward uses exp(+-15).  The last colour
    layer times 20: pre-activations beyond +-20, where fl(1 - s) carries s's own rounding."""
    worst = {}
    _run_case(dev, worst, shape, 21, 8, mode, net_kw=CLAMP)
    case = _run_case(dev, worst, shape, 7, 40, mode, semgrad=True, net_kw=CLAMP)[0]
    h0 = case["f"]["h"][:, 0]
    assert float((h0 > 15).double().mean()) >= 0.05 and float((h0 < -15).double().mean()) >= 0.05
    case = _run_case(dev, worst, shape, 7, 40, mode, net_kw=SAT)[0]
    assert int((case["f"]["c3"] > 20).sum()) >= 3 and int((case["f"]["c3"] < -20).sum()) >= 3
    _assert_worst(f"clamp_and_saturation[{shape},{mode}]", worst)


@pytest.mark.parametrize("mode", NUMERIC_MODES)
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_gradients_are_added_to(dev, shape, mode):
    """Every gradient tensor pre-filled with 0.05 randn: got - prefill against the reference, the bounds + u |prefill + ref|
    for the final rounding; the unused image's row keeps its prefill bit for bit."""
    worst = {}
    for R, S in ((7, 40), (9, 16)):
        case, D, _, _, got = _run_case(dev, worst, shape, R, S, mode, prefill=True)
        assert torch.equal(got["embedding"][fr.UNUSED_CAM], D.pre["embedding"][fr.UNUSED_CAM])
    _assert_worst(f"accumulate[{shape},{mode}]", worst)


@pytest.mark.parametrize("mode", NUMERIC_MODES)
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_eval_path_and_embedding_mean(dev, shape, mode):
    """mean_embedding given — zeros, and K.embedding_mean of the table ([32], per entry against the float64 mean): rgb within
    the bounds of the reference with that vector; density and logit bit-identical to the training path's."""
    worst = {}
    case = fr.prepare(shape, 7, 40)
    net, batch = case["net"], case["batch"]
    D = Device(dev, net, batch, mode)
    train, _ = D.forward()
    mean = _K().embedding_mean(D.par["embedding"]).cpu()
    e64 = net["embedding"].double()
    ratio = float(((mean.double() - e64.mean(0)).abs() / ((fr.N_IMAGES + 2) * U * e64.abs().mean(0))).max())
    assert mean.shape == (32,) and _worst(f"embedding_mean[{shape}]", ratio) <= 1.0
    for name, vec in (("zeros", torch.zeros(32)), ("mean", mean)):
        with torch.no_grad():
            f = fr.forward(net, batch, mean_embedding=vec)
        m = fr.forward_bounds(net, batch, f, mode, mean_embedding=vec)
        for want_h in (True, False):
            got, _ = D.forward(mean_embedding=vec, want_h=want_h)
            _check_forward(f"eval[{shape},{mode},{name}]", worst, case, mode, got, m=m, f=f)
            assert torch.equal(got["density"], train["density"]) and torch.equal(got["logit"], train["logit"]), name
            assert not torch.equal(got["rgb"], train["rgb"]), name
    _assert_worst(f"eval[{shape},{mode}]", worst)


def _sentinel(n, dev):
    return torch.full((n + 64,), SENTINEL, device=dev)


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_nothing_is_written_past_n(dev, shape, mode):
    """The library entries called directly with every output 64 elements longer than it has to be and pre-filled with a
    sentinel, at N = 37, 168, 280 and 387 (ragged last tile, 32-group and 128-batch): the first N rows are what the wrapper
    returns, bit for bit, the 64 elements behind them keep the sentinel.  Forward, backward with the Jacobian, semgrad."""
    L, K = _L(), _K()
    lib = L.load()
    for R, S in ((37, 1), (21, 8), (7, 40), (3, 129)):
        case = fr.prepare(shape, R, S, True)
        batch, geo, N = case["batch"], case["net"]["geo"], case["batch"]["N"]
        D = Device(dev, case["net"], batch, mode)
        ref_f, saved = D.forward()
        hdim = ref_f["h_pad"].shape[1]
        out = dict(density=_sentinel(N, dev), rgb=_sentinel(3 * N, dev), logit=_sentinel(N, dev), geo_out=_sentinel(N * geo, dev),
                   h_pad=_sentinel(N * hdim, dev), ray_bias=_sentinel(R * 64, dev))
        ws = torch.empty(lib.fnr_field_mlp_fwd_workspace_bytes(0), dtype=torch.uint8, device=dev)
        L.check(lib.fnr_field_mlp_fwd(C.byref(D.c_net), D.rays.ref, S, L.ptr(D.feats), L.ptr(D.sel), None, L.ptr(out["density"]),
                                      L.ptr(out["rgb"]), L.ptr(out["logit"]), L.ptr(out["geo_out"]), L.ptr(out["h_pad"]),
                                      L.ptr(out["ray_bias"]), L.ptr(ws), ws.numel(), L.stream_ptr(dev)), "field_mlp_fwd")
        torch.cuda.synchronize()
        for k, t in out.items():
            n = ref_f[k].numel()
            assert torch.equal(t[:n].cpu(), ref_f[k].reshape(-1)), f"{shape} {mode} N={N}: {k}"
            assert bool((t[n:] == SENTINEL).all()), f"{shape} {mode} N={N}: {k} written past its end"
        jac = _jacobian(batch, dev)
        up = {k: v.to(dev).contiguous() for k, v in case["up"].items()}
        for semgrad in (False, True):
            ref_b = D.backward(saved, case["up"], jacobian=jac, semgrad=semgrad)
            d_feats, d_pos = _sentinel(32 * N, dev), _sentinel(4 * N, dev)
            nbytes = lib.fnr_field_mlp_bwd_workspace_bytes(R, S)
            bws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            args = (C.byref(D.c_net), C.byref(D.c_grad), D.rays.ref, S, L.ptr(D.feats), L.ptr(saved[0]), L.ptr(saved[1]),
                    L.ptr(saved[2]), L.ptr(D.sel), L.ptr(up["dd"]), L.ptr(up["dr"]), L.ptr(up["dl"]), L.ptr(d_feats), L.ptr(jac),
                    L.ptr(d_pos))
            if semgrad:
                L.check(lib.fnr_field_mlp_bwd_semgrad(*args, None, None, L.ptr(bws), nbytes, L.stream_ptr(dev)), "bwd_semgrad")
            else:
                L.check(lib.fnr_field_mlp_bwd_rays(*args, L.ptr(bws), nbytes, L.stream_ptr(dev)), "bwd_rays")
            torch.cuda.synchronize()
            for k, t, n in (("d_feats", d_feats, 32 * N), ("d_position", d_pos, 4 * N)):
                assert torch.equal(t[:n].cpu(), ref_b[k].reshape(-1)), f"{shape} {mode} N={N} semgrad={semgrad}: {k}"
                assert bool((t[n:] == SENTINEL).all()), f"{shape} {mode} N={N} semgrad={semgrad}: {k} written past its end"


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("shape", list(fr.SHAPES))
def test_structure_in_every_arithmetic(dev, shape, mode):
    """At (7,40) and (37,1), plain and semgrad, plain bf16 included: exact zeros (density at unselected samples, the unused
    image's row, d_feats and d_position of samples without upstream gradient), exactly N rows; two calls give identical bits
    (forward and backward); a bare h as h_saved (ray bias and fragment image recomputed) gives the bits of the saved tuple;
    own h and ray bias with the workspace of a forward in ANOTHER arithmetic (the wrapper repacks) give the bits of the own
    tuple; want_h=False gives the outputs of want_h=True; gradients are added: a prefilled arena yields prefill + the
    gradients of a zeroed arena to one rounding of the sum."""
    other = "bf16x3" if mode == "fp32" else "fp32"
    for R, S in ((7, 40), (37, 1)):
        for semgrad in (False, True):
            case = fr.prepare(shape, R, S, semgrad)
            batch, N = case["batch"], case["batch"]["N"]
            D = Device(dev, case["net"], batch, mode)
            got_f, saved = D.forward()
            again, saved2 = D.forward()
            _same_bits(list(got_f.values()), list(again.values()), "two forward calls")
            lean, _ = D.forward(want_h=False)
            _same_bits([got_f[k] for k in lean], list(lean.values()), "want_h=False")
            assert got_f["density"].shape == (N,) and torch.equal(got_f["density"] != 0, batch["sel"])
            assert bool(torch.isfinite(got_f["rgb"]).all()) and bool(torch.isfinite(got_f["logit"]).all())
            jac = _jacobian(batch, dev)
            got = D.backward(saved, case["up"], jacobian=jac, semgrad=semgrad)
            _same_bits(got, D.backward(saved, case["up"], jacobian=jac, semgrad=semgrad), "two backward calls")
            _same_bits(got, D.backward(saved[0], case["up"], jacobian=jac, semgrad=semgrad), "a bare h as h_saved")
            _, foreign = Device(dev, case["net"], batch, other).forward()
            _same_bits(got, D.backward((saved[0], saved[1], foreign[2], foreign[3]), case["up"], jacobian=jac, semgrad=semgrad),
                       "the workspace of a forward in another arithmetic")
            assert got["d_feats"].shape == (16, N, 2) and got["d_position"].shape == (N, 4)
            assert float(got["embedding"][fr.UNUSED_CAM].abs().max()) == 0.0 and float(got["embedding"].abs().max()) > 0.0
            silent = (case["up"]["dd"] == 0) & (case["up"]["dl"] == 0) & (case["up"]["dr"] == 0).all(1)
            assert bool(silent.any()) or N < 64
            if silent.any():
                assert float(got["d_feats"][:, silent].abs().max()) == 0.0 and float(got["d_position"][silent].abs().max()) == 0.0
            assert float(got["d_position"][:, 3].abs().max()) == 0.0
            P = Device(dev, case["net"], batch, mode, prefill=True)
            _, psaved = P.forward()
            added = P.backward(psaved, case["up"], jacobian=jac, semgrad=semgrad)
            for k in P.pre:
                for a, p, g in zip(*(x[k] if isinstance(x[k], tuple) else (x[k],) for x in (added, P.pre, got))):
                    want = p.double() + g.double()
                    assert bool(((a.double() - want).abs() <= U * want.abs()).all()), f"{k}: not prefill + gradient"
            _same_bits([added["d_feats"], added["d_position"]], [got["d_feats"], got["d_position"]], "prefill changes d_feats")
