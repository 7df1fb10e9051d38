"""The proposal networks' kernels — k_prop_density (forward), k_prop_bwd, k_prop_reduce / k_prop_reduce2 and the binned
scatter behind them — against a float64 reference written here in plain torch (not oracle/ns_torch.py's float32 path),
per sample, per weight entry and per table row, never against a batch maximum, at every built L = 1..8.

The reference takes the float32 unit-cube position x of every sample as given and upcasts it (table and weights are
float32 values upcast too): corners from ceil / floor of x * scaling with HashEncoding.hash_fn's hash, offset = scaled -
floor, Linear(2L,16) ReLU Linear(16,1), density = exp(out) * selector, backward of exp = g exp(clamp(out, -15, 15)),
gradients by float64 autograd w.r.t. table, w0, b0, w1, b1 and x.  Scalings are floor(16 * 32^(l / (L - 1))): coarsest 16,
finest 512, both powers of two (x * scaling is exact in float32 there: the lattice samples below really sit on lattice
planes), the levels between are not.

Geometries.  POINTS: warp mode 1 with aabb [0,1]^3, S = 1, directions 0, origins = the wanted positions: (o - 0) / 1 and
o + (0 * (t0 + t1)) / 2 are exact (common.hpp, ray_position and warp_position: fsub, fdiv by 1.0, fadd of 0), so x = origin bit for bit.
Samples 0..27 (N >= 255) are the edges: on lattice points of the coarsest and the finest level on one, two and three
axes, one float32 ulp either side of a lattice plane, on the faces x = 0 and x = 1 (selector false), one ulp inside them
(selector true; at 0 that is the smallest subnormal).  RAYS: warp mode 0, random rays with bins out to t = 1000, x from
the oracle's SceneContraction in float32.

What a float64 reference and a float32 kernel may legitimately disagree on is removed by construction:
  * the grid cell: fl32(x s) can round ONTO an integer that x s lies just below or above.  Features and table records are
    continuous there, the position gradient is not.  Samples with |x s - rint(x s)| <= 4 ulp32(x s) at some level and axis
    get d_density = 0 and leave the forward check (rays: all of them; points: those whose float32 product is inexact —
    where it is exact both sides see the same cell, and the lattice / one-ulp edge samples stay in).  < 1 % of N, asserted.
  * the side of a kink: samples with a hidden pre-activation |a_o| <= m_a,o or | |out| - 15 | <= m_out get d_density = 0
    and stay in the batch (zero upstream gradient).  < 1 % of N, asserted.

Error model, u = 2^-24, first order, per sample (sc_a = |x_a s_l|, W_k the 8 corner weights, W'_a,k / W''_ab,k the weight
with the factor of axis a / of axes a and b left out, v_k the corner rows):
  E_f   = u (9 sum_k W_k |v_k| + sum_a sc_a sum_k W'_a,k |v_k|)
          three nested lerps, each path through <= 3 roundings per lerp (1 - o, product, sum); fl32(x s) carries
          |d sc| <= u sc, offset = sc - floor is exact, the feature is multilinear in the offsets.
  m_a,o = (2L + 1) u (|b0_o| + sum_k |w0_ok| |f_k|) + sum_k |w0_ok| E_f,k       the fma chain of 2L + 1 terms + its inputs
  m_out = 17 u (|b1| + sum_o |w1_o| relu(a_o)) + sum_o |w1_o| m_a,o             (relu is 1-Lipschitz)
  r     = 3 u + m_out [|out| < 15]        relative error of d_out = g exp(clamp(out)): expf (<= 2 ulp), one product, and
          exp turns the ABSOLUTE error of out into a RELATIVE one — its own term in every gradient bound
  E_df,k = (17 u + r) sum_o |dh_o| |w0_ok|                                     fma chain of 16 over dh_o = d_out w1_o [a_o > 0]

Bounds: c * (u * scale + stated terms); scale = the float64 sum of |terms| the kernel adds up for that element.  c per
quantity is NOT guessed: the same reference evaluated in float32 on the CPU over these tests' own inputs has its worst
|err| / bound between 1/32 and 1/4 — the kernel gets >= 4x over that for its other order of summation (MFMA over 4
samples, per-wave tiles, per-workgroup partials, 64-bit fixed point in the scatter).  The worst cases over every test of
this file, [CPU float32, MI355X]; the two agree because the largest terms (fl32(x s), the fma chains per sample) do not
depend on the order of a sum.  C_FEAT = 8, C_DENS = 1, C_POS = 2, C_W0 = 4, C_B0 = 0.3, C_W1 = 1, C_B1 = 0.15, C_TAB = 8
(below 1 where the worst-case m_out, which assumes every rounding of a sample aligned, dominates the bound):
  features   C_FEAT E_f                                                                                   [0.107, 0.107]
  density    C_DENS ref (2 u + expm1(m_out))                                                               [0.047, 0.047]
  d_position C_POS sum_l s_l (sum_k W'_a,k sum_j (u |df_j| + E_df,j) |v_kj| + sum_{b != a} u sc_b sum_k W''_ab,k sum_j |df_j| |v_kj|)
                                                                                                           [0.051, 0.051]
  grad w0    C_W0 sum_n |dh_o| (|f_k| (u + r) + E_f,k)                                                      [0.045, 0.045]
  grad b0    C_B0 sum_n |dh_o| (u + r)                                                                      [0.051, 0.054]
  grad w1    C_W1 sum_n |d_out| (relu(a_o) (u + r) + m_a,o [a_o > 0])                                       [0.049, 0.050]
  grad b1    C_B1 sum_n |d_out| (u + r)                                                                     [0.050, 0.048]
  grad table C_TAB sum_records (u W_k |df| + |df| sum_a W'_a,k u sc_a + W_k E_df) + cnt_row 2^(nb + e_l - 56)
             the last term is the scatter's fixed point: a record is rounded to 2^-S, S = 62 - nb - e with n < 2^nb the
             bin's records (<= 8 N) and vmax < 2^e the level's largest emitted value — e_l of the reference's largest
             record + 1 for a maximum next to a power of two + 6 for the emit's pre-summed runs of up to 64 lanes; it
             matters only where records differ by ~2^40, i.e. in the clamp batch (exp(-15) next to exp(15)).    [0.11, 0.11]
  accumulate tests: + u |prefill + ref| for the final rounding of prefill + sum, outside c: round-to-nearest attains it
             (a sum just above a power of two), so where the prefill dwarfs a row's gradient the ratio is that of one
             rounding and the same on both sides.                                          [table 0.78, 0.78; the weights as above]
"""
import math

import pytest
import torch

from oracle import ns_torch as ns

pytestmark = pytest.mark.gpu

F8 = torch.float64
U = 2.0 ** -24
H = 16
P1, P2 = 2654435761, 805459861
C_FEAT, C_DENS, C_POS, C_W0, C_B0, C_W1, C_B1, C_TAB = 8.0, 1.0, 2.0, 4.0, 0.3, 1.0, 0.15, 8.0
C_OF = {"d_position": C_POS, "w0": C_W0, "b0": C_B0, "w1": C_W1, "b1": C_B1, "table": C_TAB}
# corner k of the oracle's order h0..h7 = ccc cfc ffc fcc ccf cff fff fcf: 1 = ceil side (weight o), 0 = floor side (1 - o)
SIDES = torch.tensor([[1, 1, 1], [1, 0, 1], [0, 0, 1], [0, 1, 1], [1, 1, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0]])
UNIT_BOX = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
N_EDGE = 28
FACE_IDX, INSIDE_IDX, LATTICE_IDX = range(16, 22), range(22, 28), range(0, 12)


def _K():
    from fruitnerf_amd import _kernels as K
    return K


def _worst(name, ratio):
    v = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[proposal kernels] {name}: worst |err| / bound = {v:.3g}")
    return v


# ---------------------------------------------------------------------------------------------------------------------
# networks and batches (float32, CPU)
# ---------------------------------------------------------------------------------------------------------------------

def _scalings(L):
    return [16] if L == 1 else [int(math.floor(16.0 * 32.0 ** (l / (L - 1)) + 1e-9)) for l in range(L)]


_NETS = {}


def _net(L, log2_T=17, seed=0, out_scale=1.0, b1=0.3):
    """Trained-like table (uniform in +-0.8), Kaiming-uniform weights (w1 times out_scale), non-zero biases."""
    key = (L, log2_T, seed, out_scale, b1)
    if key not in _NETS:
        if len(_NETS) > 6:
            _NETS.clear()
        g = torch.Generator().manual_seed(1000 * L + log2_T + 77 * seed)
        r = lambda *s: torch.rand(*s, generator=g) * 2 - 1   # noqa: E731
        _NETS[key] = dict(L=L, log2_T=log2_T, scal=_scalings(L), table=(r(L << log2_T, 2) * 0.8).contiguous(),
                          w0=(r(H, 2 * L) * math.sqrt(6.0 / (2 * L))).contiguous(), b0=(r(H) * 0.5).contiguous(),
                          w1=(r(H) * math.sqrt(6.0 / H) * out_scale).contiguous(),
                          b1=torch.tensor([b1]))
    return _NETS[key]


def _points(L, N, seed=0):
    """-> geometry dict: mode 1, S = 1, origins = x [N,3] in the unit cube.  N >= 255: samples 0..27 are the edges."""
    g = torch.Generator().manual_seed(31 * N + L + 1009 * seed)
    x = torch.rand(N, 3, generator=g) * 0.98 + 0.01
    if N >= 255:
        s_f = float(_scalings(L)[-1])
        one, zero = torch.tensor(1.0), torch.tensor(0.0)
        c = [3 / 16, 5 / 16, 7 / 16]                                                # lattice planes of the coarsest level
        f = [max(1, round(0.07 * s_f)) / s_f, round(0.39 * s_f) / s_f, round(0.65 * s_f) / s_f]      # ... of the finest
        for i, p in enumerate((c, f)):
            x[6 * i + 0, 0] = p[0]                                                   # offset 0 on one axis,
            x[6 * i + 1, :2] = torch.tensor(p[:2])                                   # two,
            x[6 * i + 2] = torch.tensor(p)                                           # three
            x[6 * i + 3, 1] = p[1]
            x[6 * i + 4, 1:] = torch.tensor(p[1:])
            x[6 * i + 5, 2] = p[2]
            x[12 + 2 * i, 0] = torch.nextafter(torch.tensor(p[0]), zero)             # one ulp below / above a plane
            x[13 + 2 * i, 1] = torch.nextafter(torch.tensor(p[1]), one)
        x[16, 0], x[17, 1], x[18, 2] = 0.0, 1.0, 0.0                                 # on the faces: selector false
        x[19] = 0.0
        x[20] = 1.0
        x[21, 0], x[21, 2] = 1.0, 0.0
        tiny, below = torch.nextafter(zero, one), torch.nextafter(one, zero)         # one ulp inside: selector true
        x[22, 0], x[23, 1], x[24, 2] = tiny, below, below
        x[25] = tiny
        x[26] = below
        x[27, 0], x[27, 2] = below, tiny
    return dict(mode=1, R=N, S=1, o=x.contiguous(), d=torch.zeros(N, 3), t=torch.tensor([[0.5, 1.5]]).repeat(N, 1),
                x=x.contiguous(), exempt_exact=True, n_edge=N_EDGE if N >= 255 else 0)


def _rays(R, S, seed=0):
    """Random rays with bins out to t = 1000 (test_gpu_ray_kernels._ray_geometry); x = the oracle's float32 contraction."""
    g = torch.Generator().manual_seed(7 * R + 1009 * seed)                           # the rays depend on R and seed alone
    o = torch.randn(R, 3, generator=g) * 0.5
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    g = torch.Generator().manual_seed(7 * R + S + 1009 * seed)
    t = torch.sort(torch.rand(R, S + 1, generator=g) ** 3 * 1000.0, 1).values
    t[0] = torch.linspace(0, 0.5, S + 1)                                             # a ray inside the unit ball
    pos = o[:, None, :] + d[:, None, :] * (t[:, :-1, None] + t[:, 1:, None]) / 2     # Frustums.get_positions, float32
    x = ((ns.SceneContraction()(pos) + 2.0) / 4.0).reshape(-1, 3)
    return dict(mode=0, R=R, S=S, o=o.contiguous(), d=d.contiguous(), t=t.contiguous(), x=x.contiguous(), exempt_exact=False, n_edge=0)


RAY_SHAPES = {1: (1, 1), 255: (15, 17), 256: (16, 16), 257: (257, 1), 1000: (40, 25)}


def _geometry(kind, L, N, seed=0):
    return _points(L, N, seed) if kind == "points" else _rays(*RAY_SHAPES[N], seed=seed + L)


def _selector(x):
    return ((x > 0.0) & (x < 1.0)).all(dim=-1)


def _near_lattice(geom, scal):
    """Samples whose x s lies within 4 float32 ulps of an integer at some level and axis (module docstring)."""
    sel = _selector(geom["x"])
    xm = geom["x"] * sel[:, None]
    s = torch.tensor(scal, dtype=torch.float32)[:, None, None]
    p32 = xm[None] * s
    p64 = xm.double()[None] * s.double()
    ulp = torch.ldexp(torch.ones_like(p64), torch.frexp(p64)[1] - 24)
    near = (p64 - torch.round(p64)).abs() <= 4 * ulp
    if geom["exempt_exact"]:
        near &= p32.double() != p64
    return near.any(2).any(0) & sel


# ---------------------------------------------------------------------------------------------------------------------
# the reference (any dtype: float64 is the reference, float32 the yardstick the constants c are chosen by)
# ---------------------------------------------------------------------------------------------------------------------

class _TruncExp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        return g * torch.exp(ctx.saved_tensors[0].clamp(-15.0, 15.0))


def _encode(table, x, scal, log2_T):
    """table [L T, 2], x [N,3] (selector applied) -> features [L,N,2] and the pieces the bounds are made of."""
    L, T = len(scal), 1 << log2_T
    s = torch.tensor(scal, dtype=x.dtype)[:, None, None]
    scaled = x[None] * s
    fl, ce = torch.floor(scaled).detach(), torch.ceil(scaled).detach()
    off = scaled - fl
    fac = torch.stack([1 - off, off], -1)                                             # [L,N,3,side]
    cf = torch.stack([fl, ce], -1).long()
    cx, cy, cz = (cf[:, :, a, :][..., SIDES[:, a]] for a in range(3))                 # [L,N,8]
    idx = ((cx ^ (cy * P1) ^ (cz * P2)) & (T - 1)) + torch.arange(L)[:, None, None] * T
    wa = [fac[:, :, a, :][..., SIDES[:, a]] for a in range(3)]
    W = wa[0] * wa[1] * wa[2]
    v = table[idx]                                                                    # [L,N,8,2]
    return dict(feat=(W[..., None] * v).sum(2), idx=idx, W=W, wa=wa, v=v, sc=scaled.detach().abs())


def _encode_scales(e):
    """-> |f| scale sum_k W |v| and the offset term sum_a sc_a sum_k W'_a,k |v_k|, both [L,N,2]; E_f [N,2L]."""
    wa, av = [w.detach() for w in e["wa"]], e["v"].detach().abs()
    absf = (e["W"].detach()[..., None] * av).sum(2)
    offerr = sum(e["sc"][..., a, None] * ((wa[(a + 1) % 3] * wa[(a + 2) % 3])[..., None] * av).sum(2) for a in range(3))
    return _flat(U * (9 * absf + offerr))


def _flat(f):
    return f.permute(1, 0, 2).reshape(f.shape[1], -1)                                 # [L,N,2] -> [N,2L], k = 2 l + j


def _mlp(net, f, dtype):
    w0, b0, w1, b1 = (net[k].to(dtype) for k in ("w0", "b0", "w1", "b1"))
    a = f @ w0.T + b0
    return a, torch.relu(a) @ w1 + b1


def _margins(net, f, E_f, a, out):
    """m_a [N,16], m_out [N] (module docstring), float64."""
    L = net["L"]
    w0, b0, w1, b1 = (net[k].double().abs() for k in ("w0", "b0", "w1", "b1"))
    m_a = (2 * L + 1) * U * (b0 + f.abs() @ w0.T) + E_f @ w0.T
    m_out = (H + 1) * U * (b1 + torch.relu(a) @ w1) + m_a @ w1
    return m_a, m_out


def _forward_ref(net, geom):
    """float64 forward + margins + the samples to leave out: everything the checks need that does not depend on d_density."""
    x32 = geom["x"]
    sel = _selector(x32)
    with torch.no_grad():
        f_parts, E_parts = [], []
        xm = (x32 * sel[:, None]).double()
        table = net["table"].double()
        for i in range(0, x32.shape[0], 32768):                                      # bounded memory at 4e5 samples
            e = _encode(table, xm[i:i + 32768], net["scal"], net["log2_T"])
            f_parts.append(_flat(e["feat"]))
            E_parts.append(_encode_scales(e))
        f, E_f = torch.cat(f_parts), torch.cat(E_parts)
        a, out = _mlp(net, f, F8)
        m_a, m_out = _margins(net, f, E_f, a, out)
        kink = ((a.abs() <= m_a).any(1) | ((out.abs() - 15.0).abs() <= m_out)) & sel
        near = _near_lattice(geom, net["scal"])
    # the cap on the samples left out counts the random ones: the edge samples one ulp inside x = 1 are, by design, next to
    # the last lattice plane of every level whose scaling is no power of two
    n_near = int(near[geom["n_edge"]:].sum())
    return dict(sel=sel, f=f, E_f=E_f, a=a, out=out, dens=torch.exp(out) * sel, m_a=m_a, m_out=m_out, kink=kink, near=near, n_near=n_near)


def _d_density(fr, seed):
    """1e-2 randn; a few exactly 0, a few 1e3 times the rest; 0 at the kink and near-lattice samples (asserted < 1 % each)."""
    N = fr["sel"].shape[0]
    g = torch.Generator().manual_seed(seed)
    dd = 1e-2 * torch.randn(N, generator=g)
    if N >= 64:
        dd[torch.randint(0, N, (max(2, N // 200),), generator=g)] = 0.0
        dd[torch.randint(0, N, (max(2, N // 200),), generator=g)] *= 1e3
        assert int(fr["kink"].sum()) < 0.01 * N, f"{int(fr['kink'].sum())} of {N} samples sit on a kink"
        assert fr["n_near"] < 0.01 * N, f"{fr['n_near']} of {N} samples sit next to a lattice plane"
    dd[fr["kink"] | fr["near"]] = 0.0
    return dd.contiguous()


def _backward(net, geom, dd, dtype, table_grad=True, subset=None):
    """Autograd of sum(d_density * density) in `dtype` w.r.t. w0, b0, w1, b1, x (optionally of a subset of the samples only:
    a sample's position gradient depends on no other sample) and the table.  -> dict of gradients (+ the encode pieces)."""
    x32 = geom["x"]
    sel = _selector(x32)
    par = {k: net[k].detach().clone().to(dtype).requires_grad_(True) for k in ("w0", "b0", "w1", "b1")}
    table = net["table"].detach().clone().to(dtype).requires_grad_(table_grad)
    xm = (x32 * sel[:, None]).to(dtype)

    def density(xs, sl, tab):
        e = _encode(tab, xs, net["scal"], net["log2_T"])
        a = _flat(e["feat"]) @ par["w0"].T + par["b0"]
        return _TruncExp.apply(torch.relu(a) @ par["w1"] + par["b1"]) * sel[sl].to(dtype), e

    out = {}
    if subset is None:
        xs = xm.clone().requires_grad_(True)
        dens, e = density(xs, slice(None), table)
        wrt = dict(par, d_position=xs, **({"table": table} if table_grad else {}))
        out.update(zip(wrt, torch.autograd.grad((dens * dd.to(dtype)).sum(), list(wrt.values()))))
        out["enc"] = e
    else:
        total = [torch.zeros_like(par[k]) for k in ("w0", "b0", "w1", "b1")]
        for i in range(0, x32.shape[0], 65536):                                       # weights: chunked, bounded memory
            sl = slice(i, i + 65536)
            dens, _ = density(xm[sl], sl, table.detach())
            for t, gk in zip(total, torch.autograd.grad((dens * dd[sl].to(dtype)).sum(), list(par.values()))):
                t += gk
        out.update(zip(("w0", "b0", "w1", "b1"), total))
        xs = xm[subset].clone().requires_grad_(True)
        dens, e = density(xs, subset, table.detach())
        out["d_position"] = torch.autograd.grad((dens * dd[subset].to(dtype)).sum(), xs)[0]
        out["enc"] = e
    return out


def _backward_bounds(net, fr, dd, enc, subset=None, table=True):
    """The bounds of the module docstring WITHOUT their constants c, float64: d_position [n,3] (of `subset`), w0 [16,2L],
    b0 [16], w1 [16], b1 [1], table [L T, 2]."""
    L, N = net["L"], fr["sel"].shape[0]
    w0, w1 = net["w0"].double(), net["w1"].double()
    a, out, f = fr["a"], fr["out"], fr["f"]
    dout = dd.double() * torch.exp(out.clamp(-15.0, 15.0)) * fr["sel"]
    r = 3 * U + fr["m_out"] * (out.abs() < 15.0)
    gate = (a > 0).double()
    dh = dout[:, None] * w1 * gate
    ur = (U + r)[:, None]
    b = {"b1": (dout.abs() * (U + r)).sum().reshape(1),
         "w1": (dout.abs()[:, None] * (torch.relu(a) * ur + fr["m_a"] * gate)).sum(0),
         "b0": (dh.abs() * ur).sum(0),
         "w0": (dh.abs() * ur).T @ f.abs() + dh.abs().T @ fr["E_f"]}
    sub = slice(None) if subset is None else subset
    df = (dh @ w0)[sub]                                                               # [n,2L]
    E_df = ((17 * U + r)[:, None] * (dh.abs() @ w0.abs()))[sub]
    n = df.shape[0]
    df3, E3 = df.view(n, L, 2).permute(1, 0, 2), E_df.view(n, L, 2).permute(1, 0, 2)  # [L,n,2]
    wa, W, av, sc = [w.detach().double() for w in enc["wa"]], enc["W"].detach().double(), enc["v"].detach().double().abs(), enc["sc"].double()
    s = torch.tensor(net["scal"], dtype=F8)[:, None]
    pos = []
    for ax in range(3):
        o1, o2 = (ax + 1) % 3, (ax + 2) % 3
        first = ((wa[o1] * wa[o2])[..., None] * av * (U * df3.abs() + E3)[:, :, None, :]).sum((2, 3))
        second = sum(U * sc[..., bx] * (wa[3 - ax - bx][..., None] * av * df3.abs()[:, :, None, :]).sum((2, 3)) for bx in (o1, o2))
        pos.append((s * (first + second)).sum(0))
    b["d_position"] = torch.stack(pos, 1)
    if table:
        assert subset is None
        T2 = (L << net["log2_T"])
        Wp_sc = sum((wa[(ax + 1) % 3] * wa[(ax + 2) % 3]) * sc[..., ax, None] for ax in range(3))      # [L,N,8]
        rec = (U * W[..., None] * df3.abs()[:, :, None, :] + U * Wp_sc[..., None] * df3.abs()[:, :, None, :] +
               W[..., None] * E3[:, :, None, :])                                                      # [L,N,8,2]
        absrec = W[..., None] * df3.abs()[:, :, None, :]
        idx = enc["idx"].reshape(-1)
        tb = torch.zeros(T2, 2, dtype=F8).index_add_(0, idx, rec.reshape(-1, 2))
        cnt = torch.zeros(T2, 2, dtype=F8).index_add_(0, idx, (absrec.reshape(-1, 2) > 0).double())
        nb = (8 * N).bit_length()
        e_l = torch.frexp(absrec.amax((1, 2, 3)).clamp_min(1e-300))[1]                                # [L]
        quantum = torch.ldexp(torch.ones(L, dtype=F8), e_l + nb - 56).repeat_interleave(1 << net["log2_T"])[:, None]
        b["table"] = tb
        b["table_floor"] = cnt * quantum
    return b


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------

def _struct(net, dev, tensors):
    from fruitnerf_amd import _lib as Lb
    K = _K()
    pn = Lb.fnr_prop_net()
    pn.grid = K.make_grid(tensors["table"], net["L"], net["log2_T"], net["scal"])
    pn.hidden_dim = H
    pn.w0, pn.b0, pn.w1, pn.b1 = (Lb.ptr(tensors[k]) for k in ("w0", "b0", "w1", "b1"))
    return pn


def _device_side(net, geom, dev):
    K = _K()
    par = {k: net[k].to(dev).contiguous() for k in ("table", "w0", "b0", "w1", "b1")}
    rays = K.RaysArg(geom["o"].to(dev), geom["d"].to(dev), None, None)
    return dict(par=par, net=_struct(net, dev, par), rays=rays, warp=K.make_warp(geom["mode"], UNIT_BOX), euclid=geom["t"].to(dev).contiguous())


def _kernel_forward(dev, net, geom, save_feats):
    """-> density [N], feats [L,N,2] | None (CPU)."""
    D = _device_side(net, geom, dev)
    dens, feats = _K().prop_density_fwd(D["net"], D["warp"], D["rays"], D["euclid"], geom["S"], save_feats=save_feats)
    return dens.reshape(-1).cpu(), None if feats is None else feats.cpu()


def _grad_tensors(net, dev, prefill):
    g = torch.Generator().manual_seed(99)
    out = {}
    for k in ("table", "w0", "b0", "w1", "b1"):
        out[k] = (torch.randn(net[k].shape, generator=g) * 0.05 if prefill else torch.zeros(net[k].shape)).to(dev).contiguous()
    return out


def _kernel_backward(dev, net, geom, dd, want_position_grad=True, prefill=False):
    """prop_density_fwd(save_feats) + fnr_prop_density_bwd -> dict of gradients (CPU), `prefill` (CPU) when asked for."""
    K = _K()
    D = _device_side(net, geom, dev)
    _, feats = K.prop_density_fwd(D["net"], D["warp"], D["rays"], D["euclid"], geom["S"], save_feats=True)
    gt = _grad_tensors(net, dev, prefill)
    pre = {k: v.cpu().clone() for k, v in gt.items()}
    d_pos = K.prop_density_bwd(D["net"], _struct(net, dev, gt), D["warp"], D["rays"], D["euclid"], geom["S"], feats,
                               dd.to(dev).contiguous(), want_position_grad=want_position_grad)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in gt.items()}
    got["d_position"] = None if d_pos is None else d_pos.cpu()
    return got, pre


def _kernel_backward_pair(dev, nets, geoms, dds):
    K = _K()
    Ds = [_device_side(n, g, dev) for n, g in zip(nets, geoms)]
    feats = [K.prop_density_fwd(D["net"], D["warp"], D["rays"], D["euclid"], g["S"], save_feats=True)[1] for D, g in zip(Ds, geoms)]
    gts = [_grad_tensors(n, dev, False) for n in nets]
    d_pos = K.prop_density_bwd_pair([D["net"] for D in Ds], [_struct(n, dev, gt) for n, gt in zip(nets, gts)],
                                    [D["warp"] for D in Ds], Ds[0]["rays"], [D["euclid"] for D in Ds], [g["S"] for g in geoms],
                                    feats, [dd.to(dev).contiguous() for dd in dds], want_position_grad=True)
    torch.cuda.synchronize()
    out = []
    for gt, dp in zip(gts, d_pos):
        got = {k: v.cpu() for k, v in gt.items()}
        got["d_position"] = dp.cpu()
        out.append(got)
    return out


def _cap():
    from fruitnerf_amd import _lib as Lb
    return 3 * Lb.device_check()["cus"]


# ---------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------

def _check_forward(name, worst, net, fr, dens, feats):
    L, sel, keep = net["L"], fr["sel"], fr["sel"] & ~fr["near"]
    N = sel.shape[0]
    if feats is not None:
        got = _flat(feats.double())
        if keep.any():
            worst.setdefault("features", []).append(((got - fr["f"]).abs() / (C_FEAT * fr["E_f"] + 1e-300))[keep].max())
        row0 = torch.stack([net["table"][l << net["log2_T"]] for l in range(L)]).reshape(-1)        # hash(0,0,0) = 0
        assert torch.equal(_flat(feats)[~sel], row0[None].expand(int((~sel).sum()), -1)), f"{name}: features of unselected samples"
    assert dens.shape[0] == N and torch.equal(dens != 0, sel), f"{name}: the density is 0 at the unselected samples and only there"
    bound = C_DENS * fr["dens"] * (2 * U + torch.expm1(fr["m_out"]))
    if keep.any():
        worst.setdefault("density", []).append(((dens.double() - fr["dens"]).abs() / (bound + 1e-300))[keep].max())


def _check_backward(name, worst, net, fr, dd, got, ref, subset=None, prefill=None, table=True):
    """got: the kernel's gradients (float32), ref: _backward(..., float64)."""
    b = _backward_bounds(net, fr, dd, ref["enc"], subset, table)
    sub = slice(None) if subset is None else subset
    dp = got["d_position"]
    assert torch.equal(dp[:, 3], torch.zeros(dp.shape[0])), f"{name}: d_position[:, 3]"
    assert torch.equal(dp[~fr["sel"], :3], torch.zeros(int((~fr["sel"]).sum()), 3)), f"{name}: d_position of unselected samples"
    worst.setdefault("d_position", []).append(((dp[sub, :3].double() - ref["d_position"]).abs() / (C_POS * b["d_position"] + 1e-300)).max())
    for k in ("w0", "b0", "w1", "b1") + (("table",) if table else ()):
        r64 = ref[k].reshape(net[k].shape)
        bound = C_OF[k] * b[k].reshape(net[k].shape)
        if k == "table":
            bound = bound + b["table_floor"]
        g = got[k].double()
        if prefill is not None:
            bound = bound + U * (prefill[k].double() + r64).abs()
            g = g - prefill[k].double()
        worst.setdefault(k, []).append(((g - r64).abs() / (bound + 1e-300)).max())
        assert float(r64.abs().max()) > 0 or not bool(fr["sel"].any()), f"{name}: the reference gradient of {k} is all zero"


def _assert_worst(name, worst):
    for k, v in worst.items():
        assert _worst(f"{name}.{k}", torch.stack([torch.as_tensor(x, dtype=F8) for x in v])) <= 1.0, f"{name}: {k}"


# ---------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------

def test_the_box_and_the_edge_samples_are_what_the_docstring_says():
    """(no kernel) The unit box is exact, the lattice samples have offset 0 in float32 AND float64 at their level, the face
    samples are unselected, the one-ulp-inside samples selected, and no edge sample counts as 'near a lattice plane'."""
    for L in (1, 5, 8):
        geom, scal = _points(L, 255), _scalings(L)
        x, sel = geom["x"], _selector(geom["x"])
        assert not sel[list(FACE_IDX)].any() and sel[list(INSIDE_IDX)].all() and sel[list(LATTICE_IDX)].all()
        for i, s in ((0, scal[0]), (6, scal[-1])):
            p32, p64 = x[i:i + 6] * float(s), x[i:i + 6].double() * s
            on = torch.tensor([[1, 0, 0], [1, 1, 0], [1, 1, 1], [0, 1, 0], [0, 1, 1], [0, 0, 1]], dtype=torch.bool)
            assert torch.equal(p32.double(), p64) and bool(((p64 == torch.round(p64)) == on).all()), (L, i)
        assert not _near_lattice(geom, scal)[:N_EDGE if L == 1 else INSIDE_IDX[0]].any()
        assert (scal[0], scal[-1]) == (16, 16 if L == 1 else 512) and sorted(scal) == scal


@pytest.mark.parametrize("kind", ["points", "rays"])
@pytest.mark.parametrize("L", range(1, 9))
def test_forward_per_sample(dev, L, kind):
    """k_prop_density<L> at N = 1, 255, 256, 257, 1000: saved features per sample and level, density per sample (relative,
    with exp's amplification of out's error), exact zeros and the features of position 0 at unselected samples,
    save_feats=False bit-identical.  [CPU float32 / MI355X: features 0.107 / 0.107, density 0.047 / 0.047]"""
    worst = {}
    net = _net(L)
    for N in (1, 255, 256, 257, 1000):
        geom = _geometry(kind, L, N)
        fr = _forward_ref(net, geom)
        dens, feats = _kernel_forward(dev, net, geom, True)
        _check_forward(f"forward[{kind},L={L},N={N}]", worst, net, fr, dens, feats)
        dens2, none = _kernel_forward(dev, net, geom, False)
        assert none is None and torch.equal(dens, dens2), "save_feats=False changes the densities"
        assert fr["n_near"] < 0.01 * N or N == 1
    _assert_worst(f"forward[{kind},L={L}]", worst)


@pytest.mark.parametrize("kind", ["points", "rays"])
@pytest.mark.parametrize("log2_T", [17, 13])
@pytest.mark.parametrize("L", range(1, 9))
def test_backward_per_sample_and_per_entry(dev, L, log2_T, kind):
    """k_prop_bwd<L, posgrad>, k_prop_reduce and the scatter (2^17: corner pairs, 2^13: per corner) at N = 1000 = three full
    passes of 256 and a ragged one: d_position per sample and component, the weight gradients per entry, the table
    gradient per row and feature, exact zeros on rows without a record.
    [d_position 0.011 / 0.011, w0 0.045 / 0.045, b0 0.051 / 0.054, w1 0.049 / 0.050, b1 0.050 / 0.041, table 0.11 / 0.11]"""
    worst = {}
    net = _net(L, log2_T)
    geom = _geometry(kind, L, 1000, seed=1)
    fr = _forward_ref(net, geom)
    dd = _d_density(fr, 5 + L)
    got, _ = _kernel_backward(dev, net, geom, dd)
    ref = _backward(net, geom, dd, F8)
    _check_backward(f"backward[{kind},L={L},T=2^{log2_T}]", worst, net, fr, dd, got, ref)
    _assert_worst(f"backward[{kind},L={L},T=2^{log2_T}]", worst)


def test_the_clamp_of_trunc_exp(dev):
    """w1 times 40 and b1 = 6, so that out spans about +-35 (>= 5 % of the samples beyond each of +15 and -15): the forward density is
    the unclamped exp(out), the backward uses exp(+-15) there.  Same checks, L = 5, both geometries.
    [features 0.080 / 0.080, density 0.029 / 0.028, d_position 0.051 / 0.051, w0 0.006 / 0.007, b0 0.032 / 0.030, w1 0.022 / 0.022,
    b1 0.047 / 0.048, table 0.10 / 0.10]"""
    worst = {}
    net = _net(5, 17, seed=3, out_scale=40.0, b1=6.0)
    for kind in ("points", "rays"):
        geom = _geometry(kind, 5, 1000, seed=2)
        fr = _forward_ref(net, geom)
        sel = fr["sel"]
        assert float((fr["out"][sel] > 15).double().mean()) >= 0.05 and float((fr["out"][sel] < -15).double().mean()) >= 0.05
        dens, feats = _kernel_forward(dev, net, geom, True)
        _check_forward(f"clamp[{kind}]", worst, net, fr, dens, feats)
        dd = _d_density(fr, 17)
        got, _ = _kernel_backward(dev, net, geom, dd)
        _check_backward(f"clamp[{kind}]", worst, net, fr, dd, got, _backward(net, geom, dd, F8))
    _assert_worst("clamp", worst)


WG_CASES = [(L, b) for L in (5, 7) for b in ("1", "2", "63", "64", "65", "449", "513", "cap")] + [(5, "2 cap + 300 samples")]


@pytest.mark.parametrize("L,blocks", WG_CASES)
def test_workgroup_counts_of_the_reduction(dev, L, blocks):
    """k_prop_bwd on 1, 2, 63, 64, 65, 449, 513 and cap = 3 x CUs (from the library's device info) workgroups, the last one
    ragged, and on cap workgroups with two and a bit passes each (N = 2 cap 256 + 300; L = 5 only: 4e5 samples of float64
    reference) — k_prop_reduce's unrolled-by-8 loop, its tail loop, k_prop_bwd's persistent loop: the weight gradients per
    entry, d_position on 4096 random samples and the last 300.
    [d_position 0.012 / 0.012, w0 0.022 / 0.022, b0 0.023 / 0.021, w1 0.026 / 0.025, b1 0.024 / 0.023]"""
    worst = {}
    net = _net(L)
    cap = _cap()
    assert cap > 513
    N = 2 * cap * 256 + 300 if blocks.startswith("2 cap") else (cap if blocks == "cap" else int(blocks)) * 256 - 56
    geom = _points(L, N, seed=3)
    fr = _forward_ref(net, geom)
    dd = _d_density(fr, N)
    g = torch.Generator().manual_seed(N)
    subset = torch.unique(torch.cat([torch.randint(0, N, (min(N, 4096),), generator=g), torch.arange(max(0, N - 300), N)]))
    got, _ = _kernel_backward(dev, net, geom, dd)
    ref = _backward(net, geom, dd, F8, table_grad=False, subset=subset)
    _check_backward(f"workgroups[L={L},N={N}]", worst, net, fr, dd, got, ref, subset=subset, table=False)
    _assert_worst(f"workgroups[L={L},{blocks}]", worst)


def test_gradients_are_added_to(dev):
    """include/fruitnerf_hip.h: `+= into grads (table, w0, b0, w1, b1)`.  Every gradient tensor pre-filled with 0.05 randn:
    got - prefill against the reference, the bounds + u |prefill + ref| for the final rounding.
    [w0 0.017 / 0.017, table 0.78 / 0.78: the final rounding alone, see the module docstring]"""
    worst = {}
    for L, kind in ((5, "rays"), (3, "points")):
        net = _net(L)
        geom = _geometry(kind, L, 1000, seed=4)
        fr = _forward_ref(net, geom)
        dd = _d_density(fr, 23)
        got, pre = _kernel_backward(dev, net, geom, dd, prefill=True)
        ref = _backward(net, geom, dd, F8)
        _check_backward(f"accumulate[{kind},L={L}]", worst, net, fr, dd, got, ref, prefill=pre)
        untouched = _backward_bounds(net, fr, dd, ref["enc"])["table"] == 0
        assert torch.equal(got["table"][untouched], pre["table"][untouched]), "rows without a record changed"
    _assert_worst("accumulate", worst)


@pytest.mark.parametrize("L", [2, 5, 7])
def test_want_position_grad_false_changes_no_gradient(dev, L):
    """k_prop_bwd<L, false> against <L, true> at the same N (same workgroups, same sums): every gradient bit-identical."""
    net = _net(L)
    geom = _geometry("rays", L, 1000, seed=5)
    dd = _d_density(_forward_ref(net, geom), 29)
    with_pos, _ = _kernel_backward(dev, net, geom, dd, want_position_grad=True)
    without, _ = _kernel_backward(dev, net, geom, dd, want_position_grad=False)
    assert without["d_position"] is None
    for k in ("table", "w0", "b0", "w1", "b1"):
        assert float(with_pos[k].abs().max()) > 0 and torch.equal(with_pos[k], without[k]), k


def test_pair_of_an_L5_and_an_L7_level(dev):
    """fnr_prop_density_bwd_pair on the `fruit_nerf_big` pair (L = 5 and L = 7, different S, the same 40 rays): each
    level's per-sample and per-entry results within the bounds of the single call.
    [d_position 0.008 / 0.008, w0 0.009 / 0.009, b0 0.010 / 0.010, w1 0.020 / 0.020, b1 0.013 / 0.012, table 0.11 / 0.11]"""
    worst = {}
    nets = [_net(5), _net(7)]
    geoms = [_rays(40, 25, seed=6), _rays(40, 17, seed=6)]                          # same seed and R: the same origins, directions
    assert torch.equal(geoms[0]["o"], geoms[1]["o"]) and torch.equal(geoms[0]["d"], geoms[1]["d"])
    frs = [_forward_ref(n, g) for n, g in zip(nets, geoms)]
    dds = [_d_density(fr, 31 + i) for i, fr in enumerate(frs)]
    gots = _kernel_backward_pair(dev, nets, geoms, dds)
    for q in range(2):
        _check_backward(f"pair[{q}]", worst, nets[q], frs[q], dds[q], gots[q], _backward(nets[q], geoms[q], dds[q], F8))
    _assert_worst("pair", worst)
