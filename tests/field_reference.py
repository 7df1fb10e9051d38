"""Shared by tests/test_gpu_field_kernels.py and tests/test_field_kernels_cpu.py: FruitField's MLP stack (fruit_field.py:132-281)
as plain torch in any arithmetic, the running error bounds of every quantity the field kernels return, and the batches.

The operation (float32 inputs upcast; `x` [N,32] = the hash features, column 2 l + j):
  a1 = x W_b0^T + b_b0, h = relu(a1) W_b1^T + b_b1 [N, 1 + geo], density = exp(h0) selector (backward g exp(clamp(h0, -15, 15)))
  logit = head(mlp_semantics(h[1:1 + geo]))      (geo detached unless semgrad)
  c_ray = [SH16((d + 1) / 2) | embedding[camera] or the mean embedding]; ray_bias = b_c0 + W_c0[:, const columns] c_ray  [R,64]
  c1 = ray_bias[ray] + W_c0[:, geo columns] geo, c2 = W_c1 relu(c1) + b_c1, c3 = W_c2 relu(c2) + b_c2, rgb = sigmoid(c3)
What the kernels save and recompute (csrc/field_mlp_bwd_fp32.hip, field_mlp_bwd_pw.hip, field_mlp_bf16.hip): h [N, 16 | 32] and ray_bias are SAVED by
the forward; the backward recomputes a1 and h from the features (base branch, for the gates and trunc_exp), the colour and
semantic activations from the saved h, and the sigmoid s from the recomputed c3, forming d_c3 = d_rgb * s * (1 - s) in float32.
ray_bias, the per-ray sums of the colour branch's first-layer gradient, the ray-constant columns of W_c0, its bias and the
embedding rows are float32 fmaf / add chains in every arithmetic.

Arithmetics.  u = 2^-24.  A product-sum of chain length k in mode
  fp32    errs by at most k u sum|w||x| (fmaf chain / MFMA blocks, any order); the ESTIMATE used below takes the k roundings
          as independent: sqrt(k) u sum|w||x|
  bf16x3  forward and the backward's forward recompute: x = x1 + x2 + x3 exactly (8 bits each, |x2| <= 2^-8 |x|, |x3| <= 2^-16 |x|),
          the six products with p + q <= 2 are kept, w2 x3 + w3 x2 + w3 x3 dropped: <= (2^-24 + 2^-24 + 2^-32) sum|w||x| —
          EPS_F3 = 2^-23.  (bf16 keeps 8 significant bits, so round to nearest leaves |x - x1| <= 2^-8 |x|: half an ulp of
          2^-7.  field_bf16.hpp's 2^-27 is what typical pieces give, not the worst case.)
          dX / dW: pieces x1, x2 only (|x - x1 - x2| <= 2^-16 |x|), products w1 x1 + w1 x2 + w2 x1: the error is
          w r_x + r_w x + w2 x2 <= (2^-16 + 2^-16 + 2^-16) sum|w||x| — EPS_B3 = 3 * 2^-16 (the header's 2^-17 is the typical
          size; the emulation's worst weight entry reaches 0.3 of EPS_B3 = 2^-16 of its scale);
          + k u for the float32 accumulation either way.
The constants c of the tests absorb the distance between these worst cases and what aligned roundings really reach; they
are measured (tests/test_field_kernels_cpu.py), not guessed.

Running error ESTIMATE, not a worst-case bound (first order; relu and the gates are exact once the samples next to a kink
are left out, see kink_of).  It has the form of the standard running error bound, c (u_mode scale + propagated error) with
scale = the float64 sum of |terms|, but roundings are taken as independent: a chain of k enters as sqrt(k) u, and errors
that meet add in quadrature, q(e, W) = sqrt(e^2 (W^2)^T).  (With k u and |e| |W|^T five chained layers gave margins ~100 x
the errors seen, and 2 % of the `fruit_nerf_big` samples sat "next to a kink": over the 1 % cap.)  It holds only together
with the measured constants c below.
  m_out = ef(in + 1) (|b| + |act_in| |W|^T) + q(m_in, W)                 per layer, ef(k) = sqrt(k) u (+ EPS_F3)
  density: relative 3 u + expm1(m_h0);  rgb: c s (1 - s) m_c3 + [2 u s (1 - s) + 2 u s], the bracket (the roundings of
  expf, 1 + e and the quotient, attained at a saturated sigmoid) outside c
  E_dX = eb(out + 1) |G| |W| + q(E_G, W^T), eb(k) = sqrt(k) u (+ EPS_B3)
  dW entry: EPS_B sqrt((G^2)^T act^2) + sqrt(k_sum(N)) u |G|^T |act| + sqrt((E_G^2)^T act^2 + (G^2)^T m_act^2)
  bias entry: sqrt(k_sum(N)) u sum|G| + sqrt(sum E_G^2) (+ 2^-16 sqrt(sum G^2) in bf16x3: the row sums are products with
  ones on the matrix pipe, k_field_mlp_bwd_sem_big_bf16's cs_bias, G cut to two pieces)
  k_sum(n) = 32 + min(ceil(n / 64), 256): 16 samples of a tile, the tiles of a
  persistent wave, 8 waves, and at most one partial image per compute unit (<= 256) summed in order
  d_c3: |d_rgb| (ds + ds^2 + 3 u s (1 - s)), ds the error of s: at a saturated sigmoid fl(1 - s) loses s's own rounding
  d_h0 = d_density exp(clamp(h0)) selector: relative 4 u + m_h0 [|h0| < 15]

Plain bf16 (Arith("bf16"), the NS = 1 kernels) is not held to such bounds — u = 2^-9 per operand would put nearly every sample
next to a kink — but EXACTLY, on dyadic inputs: the last section of this file (make_lattice_net, make_lattice_batch, exactness,
guard, bf16_backward, exact_compare).  Its comment states where the kernels round, where each bias gradient is formed (a row
sum on the matrix pipe with G rounded, or a float32 sum of the unrounded G), and where the saved h is reused or recomputed.
"""
import math

import torch

F8 = torch.float64
F4 = torch.float32
U = 2.0 ** -24
EPS_F3 = 2.0 ** -23
EPS_B3 = 3.0 * 2.0 ** -16
N_IMAGES = 7
LONE_CAM, UNUSED_CAM = 5, 6          # an image seen by exactly one ray, an image seen by none
SHAPES = {"fruit_nerf": (15, (64,)), "fruit_nerf_big": (30, (128, 128))}   # geo, hidden widths of mlp_semantics

# (R, S) of the issue's table; "grid" is derived from the launch code by grid_stride_shape()
CASES = [(1, 1), (1, 17), (37, 1), (21, 8), (7, 40), (9, 16), (3, 129)]
SEMGRAD_CASES = [(7, 40), (21, 8)]


def k_sum(n):
    return 32 + min((n + 63) // 64, 256)


def grid_stride_shape(cus):
    """-> (R, S, per-kernel samples per pass).  Workgroup caps x waves x tiles per wave x 16 samples, from the launch code:
    field_mlp_fwd_launch 2 CUs x 8 x 16 (PART_SEM: CUs x 16 x 16), fwd_launch_bf16 (1 | 2) CUs x 8 x 32,
    field_mlp_fwd_sem_big_bf16 CUs x 128, field_mlp_bwd_launch CUs x 8 x 16 (k_field_mlp_bwd_sem_big: CUs x 4 x 16),
    field_mlp_bwd_pw CUs x 8 x (1 | 2) x 16, k_field_mlp_bwd_sem_big_bf16 CUs x 128.  The largest pass, 512 CUs, is a
    multiple of every other: N = 512 CUs + a ragged rest gives every kernel whole passes and a last, ragged one."""
    passes = {"fwd_fp32": 256 * cus, "fwd_fp32_sem_big": 256 * cus, "fwd_bf16": 512 * cus, "fwd_bf16_big": 256 * cus,
              "fwd_sem_big_bf16": 128 * cus, "bwd_fp32": 128 * cus, "bwd_fp32_sem_big": 64 * cus, "bwd_pw_nt1": 128 * cus,
              "bwd_pw_nt2": 256 * cus, "bwd_sem_big_bf16": 128 * cus}
    S = 41
    R = (512 * cus + 24 + S - 1) // S
    R += 1 - R % 2                                           # R and S odd: N is odd, S % 16 != 0
    return R, S, passes


# ---------------------------------------------------------------------------------------------------------------------
# networks, batches, upstream gradients (float32, CPU)
# ---------------------------------------------------------------------------------------------------------------------

def layer_names(shape):
    sem = ["sem%d" % i for i in range(len(SHAPES[shape][1]) + 1)]
    return ["base0", "base1"] + sem + ["head", "col0", "col1", "col2"]


def layer_dims(shape):
    geo, hid = SHAPES[shape]
    d = {"base0": (64, 32), "base1": (1 + geo, 64), "head": (1, 64), "col0": (64, 16 + geo + 32), "col1": (64, 64),
         "col2": (3, 64)}
    widths = (geo,) + hid + (64,)
    for i in range(len(hid) + 1):
        d["sem%d" % i] = (widths[i + 1], widths[i])
    return d


_NETS = {}


def make_net(shape, seed=0, h0_scale=1.0, h0_bias=0.3, sat=1.0):
    """Kaiming-uniform weights, non-zero biases, a non-zero embedding (nn.Linear layout).  h0_scale / h0_bias: the density
    row of base1 (the clamp cases); sat: the last colour layer's weights times `sat` (saturated sigmoids)."""
    key = (shape, seed, h0_scale, h0_bias, sat)
    if key not in _NETS:
        g = torch.Generator().manual_seed(4242 + 17 * seed + (1000 if shape == "fruit_nerf_big" else 0))
        r = lambda *s: torch.rand(*s, generator=g, dtype=F4) * 2 - 1   # noqa: E731
        net = {"shape": shape, "geo": SHAPES[shape][0]}
        for name, (o, i) in layer_dims(shape).items():
            net[name] = ((r(o, i) * math.sqrt(6.0 / i)).contiguous(), (r(o) * 0.3).contiguous())
        net["base1"][0][0] *= h0_scale
        net["base1"][1][0] = h0_bias
        net["embedding"] = (r(N_IMAGES, 32) * 0.8).contiguous()
        net["col2"][0].mul_(sat)
        _NETS[key] = net
    return _NETS[key]


def make_batch(R, S, seed=0):
    """feats [16,N,2] uniform in +-0.8 (N >= 64: an all-zero row, rows of +0.8, -0.8 and alternating extremes), selector [N]
    (N >= 64: ~12 % false), unit directions [R,3], cameras [R]: image LONE_CAM on exactly one ray (R >= 2), UNUSED_CAM on none."""
    N = R * S
    g = torch.Generator().manual_seed(100003 * R + 101 * S + seed)
    feats = (torch.rand(16, N, 2, generator=g, dtype=F4) * 2 - 1) * 0.8
    sel = torch.ones(N, dtype=torch.bool)
    if N >= 64:
        feats[:, 3] = 0.0
        feats[:, 4] = 0.8
        feats[:, 5] = -0.8
        feats[:, 6] = 0.8 * (1 - 2 * (torch.arange(32) % 2).to(F4)).view(16, 2)
        sel = torch.rand(N, generator=g, dtype=F4) > 0.12
        sel[N - 1], sel[3] = True, False
    d = torch.randn(R, 3, generator=g, dtype=F4)
    d = d / d.norm(dim=-1, keepdim=True)
    cam = torch.randint(0, 5, (R,), generator=g)
    if R >= 2:
        cam[R // 2] = LONE_CAM
    return dict(R=R, S=S, N=N, feats=feats.contiguous(), sel=sel, dirs=d.contiguous(), cam=cam)


def make_upstream(batch, seed=0, which=(1, 1, 1)):
    """d_density [N], d_rgb [N,3], d_logit [N]: randn (x `which`); N >= 64: a few samples, and with R >= 3 a whole ray, zero."""
    N, R, S = batch["N"], batch["R"], batch["S"]
    g = torch.Generator().manual_seed(77 * N + seed)
    dd, dr, dl = (torch.randn(*sh, generator=g, dtype=F4) for sh in ((N,), (N, 3), (N,)))
    dd = dd * 1e-2
    keep = torch.ones(N, dtype=F4)
    if N >= 64:
        keep[torch.randint(0, N, (max(2, N // 100),), generator=g)] = 0.0
        if R >= 3:
            keep[S:2 * S] = 0.0
    return dict(dd=(dd * keep * which[0]).contiguous(), dr=(dr * keep[:, None] * which[1]).contiguous(),
                dl=(dl * keep * which[2]).contiguous())


def zero_excluded(up, kink):
    return {k: (v * (~kink).to(v.dtype).view(-1, *([1] * (v.dim() - 1)))).contiguous() for k, v in up.items()}


# ---------------------------------------------------------------------------------------------------------------------
# arithmetics
# ---------------------------------------------------------------------------------------------------------------------

def _split(a):
    a1 = a.bfloat16().float()
    r = a - a1
    a2 = r.bfloat16().float()
    return a1, a2, (r - a2).bfloat16().float()


class Arith:
    """name: "f64" | "f32" | "bf16x3" | "bf16".  bf16x3: the piece products with p + q <= level (forward 2: six, backward 1:
    three of the pieces x1, x2), each exact in float32, float32 accumulate, smallest terms first.
    bf16 (the NS = 1 kernels, "Plain bf16" below): a float64 product of operands that were each rounded through torch.bfloat16;
    the accumulator start (bias, ray_bias) is not rounded.  rule / mut: the sensitivity mutations of
    tests/test_field_bf16_exact_cpu.py.  trace=True keeps every accumulation's operands in .log (exactness, rounding_stats)."""

    def __init__(self, name, fwd_level=2, bwd_level=1, rule="rne", mut=(), trace=False):
        self.name, self.fwd_level, self.bwd_level = name, fwd_level, bwd_level
        self.dtype = F4 if name in ("f32", "bf16x3") else F8
        self.rule, self.mut, self.log = rule, tuple(mut), ([] if trace else None)

    def rnd(self, a):
        """The operand conversion of the plain bf16 mode: round to nearest even through torch.bfloat16."""
        if self.name != "bf16":
            return a
        return a.float().bfloat16().to(a.dtype) if self.rule == "rne" else round8(a, self.rule)

    def _mm(self, a, b, level):
        if self.name != "bf16x3":
            return a @ b
        pa, pb = _split(a), _split(b)
        out = None
        for s in range(level, -1, -1):
            for p in range(s + 1):
                t = pa[p] @ pb[s - p]
                out = t if out is None else out + t
        return out

    def _note(self, kind, layer, x, w, xu, start=None):
        if self.log is not None:
            self.log.append(dict(kind=kind, layer=layer, x=x.detach().double(), w=w.detach().double(), xu=xu.detach().double(),
                                 start=None if start is None else start.detach().double()))

    def fwd(self, x, w, layer=None, start=None):
        xr, wr = self.rnd(x), self.rnd(w)
        if ("unrounded_input", layer) in self.mut:
            xr = x
        if ("swap_slots", layer) in self.mut:            # K-slots 1 and 2 of the layer's first 16 x 32 weight block
            wr = wr.clone()
            wr[:16, 1], wr[:16, 2] = wr[:16, 2].clone(), wr[:16, 1].clone()
        self._note("fwd", layer, xr, wr, x, start)
        return self._mm(xr, wr.T, self.fwd_level)

    def affine(self, x, w, start, layer=None):
        """start + x w^T: the accumulator starts at the bias (the per-ray bias in the colour branch's first layer)."""
        y = self.fwd(x, w, layer, start)
        return y + (self.rnd(start) if "bias_converted" in self.mut else start)

    def dx(self, g, w, layer=None):
        gr, wr = self.rnd(g), self.rnd(w)
        self._note("dx", layer, gr, wr.T, g)
        return self._mm(gr, wr, self.bwd_level)

    def dw(self, g, x, layer=None):
        gr = g if ("g_unrounded", layer) in self.mut else self.rnd(g)
        return self._mm(gr.T.contiguous(), self.rnd(x), self.bwd_level)


REF = Arith("f64")


class _TruncExp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        return g * torch.exp(ctx.saved_tensors[0].clamp(-15.0, 15.0))


def sh16(d, absolute=False):
    """SHEncoding(levels=4) on the shifted direction d [R,3]; absolute: the sum of the absolute values of each component's terms."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    a = (lambda p, q: p.abs() + q.abs()) if absolute else (lambda p, q: p - q)
    one = torch.ones_like(x)
    c = [0.28209479177387814 * one, 0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x,
         1.0925484305920792 * x * y, 1.0925484305920792 * y * z, a(0.9461746957575601 * zz, 0.31539156525251999 * one),
         1.0925484305920792 * x * z, 0.5462742152960396 * a(xx, yy), 0.5900435899266435 * y * a(3 * xx, yy),
         2.890611442640554 * x * y * z, 0.4570457994644658 * y * a(5 * zz, one), 0.3731763325901154 * z * a(5 * zz, 3 * one),
         0.4570457994644658 * x * a(5 * zz, one), 1.445305721320277 * z * a(xx, yy), 0.5900435899266435 * x * a(xx, 3 * yy)]
    c = torch.stack(c, 1)
    return c.abs() if absolute else c


def feats_to_x(feats):
    return feats.permute(1, 0, 2).reshape(feats.shape[1], -1)              # [16,N,2] -> [N,32], column 2 l + j


def x_to_feats(x):
    return x.reshape(x.shape[0], 16, 2).permute(1, 0, 2)


def _cols(geo):
    return list(range(16)) + list(range(16 + geo, 48 + geo)), list(range(16, 16 + geo))      # ray-constant, geo


def params(net, dtype, grad=False):
    p = {}
    for k in layer_names(net["shape"]):
        p[k] = tuple(t.detach().clone().to(dtype).requires_grad_(grad) for t in net[k])
    p["embedding"] = net["embedding"].detach().clone().to(dtype).requires_grad_(grad)
    return p


def forward(net, batch, ar=REF, mean_embedding=None, semgrad=False, p=None, x=None):
    """-> dict of every activation, in ar's arithmetic.  With p / x that require grad (float64) autograd runs through it."""
    dt, geo, S = ar.dtype, net["geo"], batch["S"]
    p = params(net, dt) if p is None else p
    x = feats_to_x(batch["feats"]).to(dt) if x is None else x
    sel = batch["sel"].to(dt)
    ray = torch.arange(batch["N"]) // S
    f = {"x": x}
    f["a1"] = ar.affine(x, *p["base0"], "base0")
    f["h"] = ar.affine(torch.relu(f["a1"]), *p["base1"], "base1")
    f["density"] = _TruncExp.apply(f["h"][:, 0]) * sel
    f["geo"] = f["h"][:, 1:]
    s = f["geo"] if semgrad else f["geo"].detach()
    sem = [k for k in layer_names(net["shape"]) if k.startswith("sem")]
    for i, k in enumerate(sem):
        f["in_" + k] = s
        f["pre_" + k] = ar.affine(s, *p[k], k)
        s = f["pre_" + k] if i == len(sem) - 1 else torch.relu(f["pre_" + k])
    f["in_head"] = s
    f["logit"] = ar.affine(s, *p["head"], "head")[:, 0]
    const, gcol = _cols(geo)
    f["sh"] = sh16((batch["dirs"].to(dt) + 1.0) / 2.0)
    emb = p["embedding"][batch["cam"]] if mean_embedding is None else mean_embedding.to(dt)[None].expand(batch["R"], 32)
    f["c_ray"] = torch.cat([f["sh"], emb], 1)
    w0, b0 = p["col0"]
    f["ray_bias"] = f["c_ray"] @ w0[:, const].T + b0                       # a float32 chain in every arithmetic
    f["c1"] = ar.affine(f["geo"], w0[:, gcol], f["ray_bias"][ray], "col0")
    f["c2"] = ar.affine(torch.relu(f["c1"]), *p["col1"], "col1")
    f["c3"] = ar.affine(torch.relu(f["c2"]), *p["col2"], "col2")
    f["rgb"] = torch.sigmoid(f["c3"]) if dt == F8 else 1.0 / (1.0 + torch.exp(-f["c3"]))
    pad = 16 * ((1 + geo + 15) // 16) - (1 + geo)
    f["h_pad"] = torch.cat([f["h"], torch.zeros(batch["N"], pad, dtype=dt)], 1)
    return f


def reference_backward(net, batch, up, semgrad=False):
    """float64 autograd of sum(d_density density + d_rgb rgb + d_logit logit) -> (forward dict, {layer: (gW, gb), embedding,
    d_feats [16,N,2]})."""
    p = params(net, F8, grad=True)
    x = feats_to_x(batch["feats"]).double().requires_grad_(True)
    f = forward(net, batch, REF, semgrad=semgrad, p=p, x=x)
    loss = (f["density"] * up["dd"].double()).sum() + (f["rgb"] * up["dr"].double()).sum() + (f["logit"] * up["dl"].double()).sum()
    names = layer_names(net["shape"])
    leaves = [t for k in names for t in p[k]] + [p["embedding"], x]
    gr = torch.autograd.grad(loss, leaves, allow_unused=True)
    gr = [torch.zeros_like(l) if g is None else g for g, l in zip(gr, leaves)]
    out = {k: (gr[2 * i], gr[2 * i + 1]) for i, k in enumerate(names)}
    out["embedding"], out["d_feats"] = gr[-2], x_to_feats(gr[-1]).contiguous()
    return {k: v.detach() for k, v in f.items()}, out


def _seg(t, R, S):
    return t.reshape(R, S, -1).sum(1)


def manual_backward(net, batch, up, ar, semgrad=False, mut=()):
    """The backward as the kernels organise it, in ar's arithmetic (float32 element-wise; matrix products through ar).
    mut: the sensitivity mutations of tests/test_field_kernels_cpu.py.  Plain bf16 has its roundings, its two kinds of bias
    sums and `fruit_nerf_big`'s factored head gradient written out in bf16_backward (below); here as plain tensors."""
    if ar.name == "bf16":
        f, out = bf16_backward(net, batch, up, ar, semgrad, mut)
        return f, sums_to_tensors(out)
    dt, geo, R, S, N = ar.dtype, net["geo"], batch["R"], batch["S"], batch["N"]
    with torch.no_grad():
        p = params(net, dt)
        f = forward(net, batch, ar, p=p)
        dd, dr, dl = (up[k].to(dt) for k in ("dd", "dr", "dl"))
        keep = torch.ones(N, 1, dtype=dt)
        if "drop_tile" in mut:
            t0 = 16 * ((N // 16) // 2)
            keep[t0:t0 + 16] = 0.0
        dw = lambda g, a: ar.dw(g * keep, a)   # noqa: E731
        ones = torch.ones(N, 1, dtype=dt)
        db = lambda g: ar.dw(g * keep, ones)[:, 0]   # noqa: E731  (bf16x3: the row sums come out of the matrix pipe too)
        const, gcol = _cols(geo)
        out = {}
        s = f["rgb"]
        G3 = dr * s * (1.0 - s)
        r1c, r2c = torch.relu(f["c1"]), torch.relu(f["c2"])
        out["col2"] = (dw(G3, r2c), db(G3))
        G2 = ar.dx(G3, p["col2"][0]) * (f["c2"] > 0)
        out["col1"] = (dw(G2, r1c), db(G2))
        G1 = ar.dx(G2, p["col1"][0]) * (f["c1"] > 0)
        w0 = p["col0"][0]
        g_ray = _seg(G1 * keep, R, S)                                        # [R,64]
        gw0 = torch.zeros_like(w0)
        gw0[:, gcol] = dw(G1, f["geo"])
        gw0[:, const] = g_ray.T @ f["c_ray"]
        out["col0"] = (gw0, g_ray.sum(0))
        g_emb_ray = g_ray @ w0[:, const[16:]]
        if "lose_ray" in mut:
            g_emb_ray[R - 1] = 0.0
        out["embedding"] = torch.zeros(N_IMAGES, 32, dtype=dt).index_add_(0, batch["cam"], g_emb_ray)
        Gh = torch.zeros(N, 1 + geo, dtype=dt)
        Gh[:, 1:] = ar.dx(G1, w0[:, gcol])
        Gs = dl[:, None]
        out["head"] = (dw(Gs, f["in_head"]), db(Gs))
        Gs = ar.dx(Gs, p["head"][0])
        sem = [k for k in layer_names(net["shape"]) if k.startswith("sem")]
        for i, k in reversed(list(enumerate(sem))):
            if i != len(sem) - 1:
                Gs = Gs * (f["pre_" + k] > 0)
            out[k] = (dw(Gs, f["in_" + k]), db(Gs))
            if i > 0 or (semgrad and "detach_geo" not in mut):
                Gs = ar.dx(Gs, p[k][0])
        if semgrad and "detach_geo" not in mut:
            Gh[:, 1:] += Gs
        h0 = f["h"][:, 0]
        hc = h0 if "no_clamp" in mut else h0.clamp(-14.0, 14.0) if "clamp14" in mut else h0.clamp(-15.0, 15.0)
        Gh[:, 0] = dd * torch.exp(hc) * (1.0 if "no_selector" in mut else batch["sel"].to(dt))
        r1 = torch.relu(f["a1"])
        out["base1"] = (dw(Gh, r1), db(Gh))
        Ga = ar.dx(Gh, p["base1"][0]) * (f["a1"] > 0)
        out["base0"] = (dw(Ga, f["x"]), db(Ga))
        out["d_feats"] = x_to_feats(ar.dx(Ga, p["base0"][0])).contiguous()
        if "copy_last" in mut and N >= 2:
            out["d_feats"][:, N - 1] = out["d_feats"][:, N - 2]
            for k in ("density", "rgb", "logit"):
                f[k][N - 1] = f[k][N - 2]
    return f, out


def position_contract(d_feats, jac):
    """d_feats [16,N,2], jac [16,3,N,2] (float32) -> float64 contraction [N,3] and its scale sum |d_feats| |jac|."""
    df, j = d_feats.double()[:, None], jac.double()
    return (df * j).sum((0, 3)).T, (df.abs() * j.abs()).sum((0, 3)).T


# ---------------------------------------------------------------------------------------------------------------------
# bounds (float64, WITHOUT the constants c)
# ---------------------------------------------------------------------------------------------------------------------

def _ef(mode, k):
    return math.sqrt(k) * U + (EPS_F3 if mode == "bf16x3" else 0.0)


def _eb(mode, k):
    return math.sqrt(k) * U + (EPS_B3 if mode == "bf16x3" else 0.0)


def _q(e, w):
    """Independent errors e [n,in] through weights w [out,in]: root of the sum of squares, [n,out]."""
    return torch.sqrt((e * e) @ (w * w).T)


def forward_bounds(net, batch, f, mode, mean_embedding=None):
    """f: forward(..., REF).  -> margins m[...] of every activation and the output bounds (module docstring), without c."""
    geo, S, N = net["geo"], batch["S"], batch["N"]
    A = {k: (net[k][0].double().abs(), net[k][1].double().abs()) for k in layer_names(net["shape"])}
    ray = torch.arange(N) // S
    m = {}

    def layer(k, act, m_in):
        w, b = A[k]
        return _ef(mode, w.shape[1] + 1) * (b + act.abs() @ w.T) + (_q(m_in, w) if m_in is not None else 0.0)

    m["a1"] = layer("base0", f["x"], None)
    m["h"] = layer("base1", torch.relu(f["a1"]), m["a1"])
    m_in = m["h"][:, 1:]
    sem = [k for k in layer_names(net["shape"]) if k.startswith("sem")]
    for k in sem:
        m["pre_" + k] = layer(k, f["in_" + k], m_in)
        m_in = m["pre_" + k]
    m["logit"] = layer("head", f["in_head"], m_in)[:, 0]
    const, gcol = _cols(geo)
    d = (batch["dirs"].double() + 1.0) / 2.0
    sh_abs = sh16(d, absolute=True)
    emb = net["embedding"].double()[batch["cam"]] if mean_embedding is None else mean_embedding.double()[None].expand(batch["R"], 32)
    m["c_abs"] = torch.cat([sh_abs, emb.abs()], 1)
    m["c_ray"] = torch.cat([4 * U * sh_abs, torch.zeros_like(emb)], 1)     # the shift, <= 3 factors, the constant, the difference
    w0, b0 = A["col0"]
    m["ray_bias"] = 7 * U * (b0 + m["c_abs"] @ w0[:, const].T) + _q(m["c_ray"], w0[:, const])      # fmaf chain of 49
    local = _ef(mode, geo + 2) * (f["ray_bias"].abs()[ray] + f["geo"].abs() @ w0[:, gcol].T)
    m["c1"] = local + torch.sqrt(m["ray_bias"][ray] ** 2 + _q(m["h"][:, 1:], w0[:, gcol]) ** 2)
    m["c2"] = layer("col1", torch.relu(f["c1"]), m["c1"])
    m["c3"] = layer("col2", torch.relu(f["c2"]), m["c2"])
    s = f["rgb"]
    m["rgb"] = s * (1 - s) * m["c3"]
    # the roundings of s = 1 / (1 + expf(-c3)) itself — expf (<= 2 ulp, through e s^2 = s (1 - s)), the sum 1 + e, the quotient —
    # are worst cases that round-to-nearest attains at a saturated sigmoid: added OUTSIDE the constant c
    m["rgb_det"] = 2 * U * s * (1 - s) + 2 * U * s
    m["density"] = f["density"] * (3 * U + torch.expm1(m["h"][:, 0]))
    pad = f["h_pad"].shape[1] - (1 + geo)
    m["h_pad"] = torch.cat([m["h"], torch.zeros(N, pad, dtype=F8)], 1)
    m["geo_out"] = m["h"][:, 1:]
    return m


def backward_bounds(net, batch, f, m, up, mode, semgrad=False):
    """f, m: forward(REF) and forward_bounds of `mode`.  -> {layer: (bound W, bound b), embedding, d_feats} of the module
    docstring, without c."""
    geo, R, S, N = net["geo"], batch["R"], batch["S"], batch["N"]
    W = {k: net[k][0].double() for k in layer_names(net["shape"])}
    dd, dr, dl = (up[k].double() for k in ("dd", "dr", "dl"))
    KN, KR = math.sqrt(k_sum(N)) * U, math.sqrt(k_sum(R) + 2) * U
    eps = EPS_B3 if mode == "bf16x3" else 0.0
    eps_1 = 2.0 ** -16 if mode == "bf16x3" else 0.0          # a bias entry is dW against ones: only G is cut to two pieces
    out = {}

    def grads(k, G, E, act, m_act):
        Ga, G2, a2 = G.abs(), G * G, act * act
        prop = (E * E).T @ a2 + (G2.T @ (m_act * m_act) if m_act is not None else 0.0)
        out[k] = (eps * torch.sqrt(G2.T @ a2) + KN * (Ga.T @ act.abs()) + torch.sqrt(prop),
                  eps_1 * torch.sqrt(G2.sum(0)) + KN * Ga.sum(0) + torch.sqrt((E * E).sum(0)))

    def dx(G, E, w):
        return G @ w, _eb(mode, w.shape[0] + 1) * (G.abs() @ w.abs()) + _q(E, w.T)

    const, gcol = _cols(geo)
    s, ds = f["rgb"], m["rgb"] + m["rgb_det"]
    G3, E3 = dr * s * (1 - s), dr.abs() * (ds + ds * ds + 3 * U * s * (1 - s))
    grads("col2", G3, E3, torch.relu(f["c2"]), m["c2"])
    G2, E2 = dx(G3, E3, W["col2"])
    g2 = (f["c2"] > 0).double()
    G2, E2 = G2 * g2, E2 * g2
    grads("col1", G2, E2, torch.relu(f["c1"]), m["c1"])
    G1, E1 = dx(G2, E2, W["col1"])
    g1 = (f["c1"] > 0).double()
    G1, E1 = G1 * g1, E1 * g1
    grads("col0", G1, E1, f["geo"], m["h"][:, 1:])
    bw_geo, _ = out["col0"]
    g_abs = _seg(G1.abs(), R, S)
    E_ray = torch.sqrt(_seg(E1 * E1, R, S)) + math.sqrt(S + 16) * U * g_abs
    w0 = W["col0"]
    bw0 = torch.zeros_like(w0)
    bw0[:, gcol] = bw_geo
    bw0[:, const] = torch.sqrt((E_ray ** 2).T @ m["c_abs"] ** 2 + (g_abs ** 2).T @ m["c_ray"] ** 2) + KR * (g_abs.T @ m["c_abs"])
    out["col0"] = (bw0, torch.sqrt((E_ray ** 2).sum(0)) + KR * g_abs.sum(0))
    we = w0[:, const[16:]].T                                              # [32,64]
    z = lambda: torch.zeros(N_IMAGES, 32, dtype=F8)   # noqa: E731
    out["embedding"] = torch.sqrt(z().index_add_(0, batch["cam"], _q(E_ray, we) ** 2)) \
        + z().index_add_(0, batch["cam"], (8 * U + KR) * (g_abs @ we.abs().T))
    Gh, Eh = torch.zeros(N, 1 + geo, dtype=F8), torch.zeros(N, 1 + geo, dtype=F8)
    Gh[:, 1:], Eh[:, 1:] = dx(G1, E1, w0[:, gcol])
    sem = [k for k in layer_names(net["shape"]) if k.startswith("sem")]
    Gs, Es = dl[:, None], torch.zeros(N, 1, dtype=F8)
    grads("head", Gs, Es, f["in_head"], m["pre_" + sem[-1]])
    Gs, Es = dx(Gs, Es, W["head"])
    for i, k in reversed(list(enumerate(sem))):
        if i != len(sem) - 1:
            gate = (f["pre_" + k] > 0).double()
            Gs, Es = Gs * gate, Es * gate
        grads(k, Gs, Es, f["in_" + k], m["h"][:, 1:] if i == 0 else m["pre_" + sem[i - 1]])
        if i > 0 or semgrad:
            Gs, Es = dx(Gs, Es, W[k])
    if semgrad:
        Eh[:, 1:] = torch.sqrt(Eh[:, 1:] ** 2 + Es ** 2) + U * (Gh[:, 1:] + Gs).abs()
        Gh[:, 1:] += Gs
    h0 = f["h"][:, 0]
    Gh[:, 0] = dd * torch.exp(h0.clamp(-15.0, 15.0)) * batch["sel"].double()
    Eh[:, 0] = Gh[:, 0].abs() * (4 * U + m["h"][:, 0] * (h0.abs() < 15.0))
    grads("base1", Gh, Eh, torch.relu(f["a1"]), m["a1"])
    Ga, Ea = dx(Gh, Eh, W["base1"])
    ga = (f["a1"] > 0).double()
    Ga, Ea = Ga * ga, Ea * ga
    grads("base0", Ga, Ea, f["x"], None)
    _, Ex = dx(Ga, Ea, W["base0"])
    out["d_feats"] = x_to_feats(Ex).contiguous()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------

FWD_QUANTITIES = ("density", "rgb", "logit", "geo_out", "h_pad", "ray_bias")


def pre_names(net):
    sem = [k for k in layer_names(net["shape"]) if k.startswith("sem")]
    return ["a1", "c1", "c2"] + ["pre_" + k for k in sem[:-1]]


def forward_ratios(got, f, m, net=None):
    """got: {quantity: tensor}; -> {quantity: worst |err| / bound (without c)}; with net, the hidden pre-activations too
    ("pre.a1", "pre.c1", "pre.c2", "pre.sem0", "pre.sem1": what the kink margins are scaled by)."""
    ref = dict(f, geo_out=f["geo"])
    # err <= c m + det  <=>  (err - det)+ / m <= c: what is returned for a quantity with a worst-case term outside c
    det = lambda k: m.get(k + "_det", 0.0)   # noqa: E731
    out = {k: float((((got[k].double() - ref[k]).abs() - det(k)).clamp_min(0.0) / (m[k] + 1e-300)).max())
           for k in FWD_QUANTITIES if k in got}
    if net is not None:
        for k in pre_names(net):
            out["pre." + k.replace("pre_", "")] = float(((got[k].double() - f[k]).abs() / (m[k] + 1e-300)).max())
    return out


def _class(k):
    layer, suffix = k.split(".")
    return ("base" if layer.startswith("base") else "col" if layer.startswith("col") else "sem") + "." + suffix


def backward_ratios(net, got, ref, b, prefill=None):
    """-> {"d_feats", "embedding", "base.w", "base.b", "sem.w" (mlp_semantics + head), "sem.b", "col.w", "col.b": worst
    |err| / bound (without c) over every entry}; prefill: the gradients were added to these (float32) values: + u |prefill + ref|
    for the final rounding."""
    out = {}

    def one(name, g, r, bound, pre):
        g = g.double()
        if pre is not None:
            bound = bound + U * (pre.double() + r).abs()
            g = g - pre.double()
        out[name] = max(out.get(name, 0.0), float(((g - r).abs() / (bound + 1e-300)).max()))

    for k in layer_names(net["shape"]):
        for j, suffix in enumerate((".w", ".b")):
            one(_class(k + suffix), got[k][j], ref[k][j], b[k][j], None if prefill is None else prefill[k][j])
    one("embedding", got["embedding"], ref["embedding"], b["embedding"], None if prefill is None else prefill["embedding"])
    if "d_feats" in got:
        one("d_feats", got["d_feats"], ref["d_feats"], b["d_feats"], None)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the constants c: >= 4 x the worst |err| / bound of the CPU evaluation in the same arithmetic over every case of the two
# test files (tests/test_field_kernels_cpu.py measures and asserts that factor; the GPU file's docstring has the pairs)
# ---------------------------------------------------------------------------------------------------------------------

C = {
    "fp32": {"density": 1.3, "rgb": 0.28, "logit": 0.42, "geo_out": 1.7, "h_pad": 1.7, "ray_bias": 1.8, "pre.a1": 4.1,
             "pre.c1": 1.2, "pre.c2": 1.2, "pre.sem0": 1.4, "pre.sem1": 0.79, "base.w": 4.2, "base.b": 1.3,
             "sem.w": 1.6, "sem.b": 1, "col.w": 0.99, "col.b": 0.35, "embedding": 0.23, "d_feats": 7.3},
    "bf16x3": {"density": 0.44, "rgb": 0.13, "logit": 0.22, "geo_out": 0.62, "h_pad": 0.62, "ray_bias": 1.8, "pre.a1": 1.5,
               "pre.c1": 0.99, "pre.c2": 0.46, "pre.sem0": 0.62, "pre.sem1": 0.33, "base.w": 2, "base.b": 1.4,
               "sem.w": 1.9, "sem.b": 1.9, "col.w": 1.6, "col.b": 1.2, "embedding": 0.49, "d_feats": 5},
}
C_POS = 1.0        # d_position against the contraction of the RETURNED d_feats: a chain of 33 float32 fmas, bound 34 u sum|df||J|


def kink_of(net, f, margins):
    """Samples with a hidden pre-activation within c x its margin of 0, or |h0| within c x its margin of 15, in either
    arithmetic.  margins: {mode: forward_bounds(...)}"""
    kink = torch.zeros(f["x"].shape[0], dtype=torch.bool)
    for mode, m in margins.items():
        c = C[mode]
        for k in pre_names(net):
            cm = c["pre." + k.replace("pre_", "")]
            kink |= (f[k].abs() <= cm * m[k]).any(1)
        kink |= (f["h"][:, 0].abs() - 15.0).abs() <= c["h_pad"] * m["h"][:, 0]
    return kink


_PREPARED = {}


# batch seeds of the cases in which seed 0 puts more than 1 % of the samples (two of 144) next to a kink
CASE_SEED = {("fruit_nerf_big", 9, 16): 1}


def prepare(shape, R, S, semgrad=False, which=(1, 1, 1), net_kw=(), seed=None):
    """Everything of a case that does not depend on the code under test, computed once and shared: the network, the batch,
    the float64 forward, the margins of both arithmetics, the excluded samples, the upstream gradients (zero there), the
    float64 autograd gradients and the bounds of both arithmetics."""
    seed = CASE_SEED.get((shape, R, S), 0) if seed is None else seed
    key = (shape, R, S, semgrad, which, tuple(net_kw), seed)
    if key not in _PREPARED:
        if len(_PREPARED) > 4:
            _PREPARED.clear()
        net = make_net(shape, 0, **dict(net_kw))
        batch = make_batch(R, S, seed)
        with torch.no_grad():
            f = forward(net, batch)
        margins = {mode: forward_bounds(net, batch, f, mode) for mode in ("fp32", "bf16x3")}
        kink = kink_of(net, f, margins)
        up = zero_excluded(make_upstream(batch, seed, which), kink)
        f, ref = reference_backward(net, batch, up, semgrad)
        bounds = {mode: backward_bounds(net, batch, f, margins[mode], up, mode, semgrad) for mode in margins}
        _PREPARED[key] = dict(net=net, batch=batch, f=f, m=margins, kink=kink, up=up, ref=ref, b=bounds, semgrad=semgrad)
    return _PREPARED[key]


def excluded_share_ok(case):
    """< 1 % of N (so none below N = 100)."""
    return int(case["kink"].sum()) < 0.01 * case["batch"]["N"]


def scaled(ratios, mode):
    """worst |err| / bound -> worst |err| / (c bound)."""
    return {k: v / C[mode][k] for k, v in ratios.items()}


# ---------------------------------------------------------------------------------------------------------------------
# Plain bf16 (mlp_mode 1, the NS = 1 kernels), tested EXACTLY on dyadic ("lattice") inputs:
# tests/test_field_bf16_exact_cpu.py, tests/test_gpu_field_bf16_exact.py
# ---------------------------------------------------------------------------------------------------------------------
# The mode's contract.  Every layer is acc = start (fp32: the bias, or ray_bias[ray] in the colour branch's first layer), both
# operands rounded to bf16 (round to nearest even: v_cvt_pk_bf16_f32 for activations and gradients, bf_piece(w, 0) for the
# weights, once, when the fragment image is packed or bf_build_T builds sem0's transposed fragments), products accumulated in
# float32 by the matrix pipe.  Where the NS = 1 kernels convert (k_field_mlp_fwd_bf16, k_field_mlp_fwd_sem_big_bf16,
# field_mlp_bwd_pw.hip, k_field_mlp_bwd_sem_big_bf16):
#   forward   rounded: the hash features, the input of every layer (relu first), h as the input of sem0 and col0 (the SAVED h
#             is the unrounded accumulator), `fruit_nerf_big`: s3 = sem2's output as the head's input.  Never rounded: biases,
#             ray_bias (a float32 fmaf chain of its own kernel), accumulators, h, geo_out, logit; density = expf(h0),
#             rgb = 1 / (1 + expf(-c3)) in float32.
#   backward  the saved h is REUSED by the colour branch (input of col0, X of col0's dW), the semantic branch (input of sem0,
#             X of sem0's dW) and the base branch (h0 of trunc_exp'); RECOMPUTED from it with the forward's roundings: c1, c2,
#             c3 (and s = sigmoid(c3) in float32, d_c3 = (d_rgb s) (1 - s) in float32), s1, s2; recomputed from the features:
#             a1 (base0 only: base1 is not run again).  Rounded: every G that enters a transposed layer (dX = W^T G) and both
#             operands of every dW product (G and the same rounded activation the forward multiplied).  The relu gates read the
#             sign of the rounded activation (= the sign of the activation).  d_h (colour dX, + the semantic dX under semgrad: a
#             float32 add) and d_h0 = d_density expf(clamp(h0)) [selector] are float32.
#   bias gradients  per-wave kernels (every branch of `fruit_nerf`, colour and base of `fruit_nerf_big`): float32 sums of the
#             UNROUNDED G.  `fruit_nerf_big`'s semantic branch (cs_bias): row sums on the matrix pipe, G ROUNDED.  col0: the
#             per-ray sums g_ray are matrix-pipe row sums of the ROUNDED G1 when S >= 16 (SelOperand) and float32 atomic sums of
#             the UNROUNDED G1 when S < 16; the bias is their float32 sum over the rays, the ray-constant columns
#             g_ray^T [SH16 | embedding row] an fmaf chain, the embedding rows sum_o W_c0[o, k] (sum of the camera's g_ray)[o]
#             with the UNROUNDED float32 weights.
#   `fruit_nerf_big`'s head: dW_head = W_sem2 v + b_sem2 sum(bf(dlogit)), v = bf(dlogit)^T bf(s2) on the matrix pipe, the rest
#             a float32 fmaf chain over the UNROUNDED W_sem2: s3 is NOT rounded here (it is in the forward); `fruit_nerf`'s
#             head: bf(dlogit)^T bf(s2), s2 its rounded input.
# Exactness.  A sum whose every partial sum, in whatever order, is a float32 number comes out exact from any correct
# accumulator: sufficient is log2(sum|addends|) - (exponent of the lowest set bit among the addends) < 24 (`bits` below).
# Sums that miss it are held to (n - 1) 2^-23 sum|addends|, n the number of addends: the worst case of any summation order
# ((n - 1) roundings of at most 2^-24 each), doubled because the guides do not say whether the matrix pipe's accumulator rounds
# or truncates — an assumption, not a measurement.  The SH columns of col0's weight gradient have a float32 SH basis as one
# factor (not on the lattice, evaluated on the device): n 2^-23 sum|addends| + sum|g| 4 u |SH terms| there (the product is
# rounded too, and the basis carries the 4 u of forward_bounds' c_ray).

BIG_LB = 1.0e6          # "no set bit": the lowbit of 0
LATTICE_VARIANTS = ("a", "b")


def round8(a, rule="rne"):
    """a (any float dtype, normal range) rounded to 8 significant bits: "rne" (= torch.bfloat16), "trunc", "away" (half away
    from zero)."""
    m, e = torch.frexp(a.double())
    y = m * 256.0
    r = torch.round(y) if rule == "rne" else torch.trunc(y) if rule == "trunc" else torch.sign(y) * torch.floor(y.abs() + 0.5)
    return torch.ldexp(r, e - 8).to(a.dtype)


def lowbit(t):
    """Exponent of the lowest set bit of every entry (float64 tensor of the same shape; BIG_LB at 0)."""
    t = t.double()
    m, e = torch.frexp(t)
    v = (m.abs() * 2.0 ** 53).to(torch.int64)
    tz = torch.log2((v & -v).clamp_min(1).double()).round()
    return torch.where(t == 0, torch.full_like(t, BIG_LB), e.double() - 53.0 + tz)


def _minplus(a, b, chunk=64):
    """a [n,p], b [n,q] -> min over n of a[n,i] + b[n,j]  [p,q]."""
    out = torch.full((a.shape[1], b.shape[1]), 4 * BIG_LB, dtype=F8)
    for i in range(0, a.shape[0], chunk):
        out = torch.minimum(out, (a[i:i + chunk, :, None] + b[i:i + chunk, None, :]).amin(0))
    return out


def bits_of(mag, lb):
    """log2(sum|addends|) - lowest set bit; -inf for an empty sum."""
    return torch.where(mag > 0, torch.log2(mag.clamp_min(1e-300)) - lb, torch.full_like(mag, -math.inf))


def exactness(log, conservative=False, kinds=("fwd", "dx", "add")):
    """log: Arith(..., trace=True).log -> [(kind, layer, bits [n,out])]: per accumulation acc = start + sum_k x[n,k] w[out,k]
    the bit count of the condition.  conservative: min lowbit(w[out]) + min lowbit(x[n]) instead of the minimum over k of the
    sums (large N)."""
    out = []
    for e in log:
        if e["kind"] not in kinds:
            continue
        x, w = e["x"], e["w"]
        mag = x.abs() @ w.abs().T
        lx, lw = lowbit(x), lowbit(w)
        if conservative:
            lb = lx.amin(1, keepdim=True) + lw.amin(1)[None]
        else:
            lb = torch.cat([_minplus(lw.T.contiguous(), lx[i:i + 256].T.contiguous()).T for i in range(0, x.shape[0], 256)])
        if e["start"] is not None:
            st = e["start"].expand(x.shape[0], w.shape[0])
            mag, lb = mag + st.abs(), torch.minimum(lb, lowbit(st))
        out.append((e["kind"], e["layer"], bits_of(mag, lb)))
    return out


def rounding_stats(log, kinds=("fwd", "dx")):
    """-> {(kind, layer): (nonzero inputs, changed by the conversion, exact ties)} of every traced operand conversion."""
    out = {}
    for e in log:
        if e["kind"] not in kinds:
            continue
        xu = e["xu"]
        m, _ = torch.frexp(xu)
        y = (m * 256.0).abs()
        tie = (y - torch.floor(y)) == 0.5
        key = (e["kind"], e["layer"])
        prev = out.get(key, (0, 0, 0))
        out[key] = (prev[0] + int((xu != 0).sum()), prev[1] + int((round8(xu) != xu).sum()), prev[2] + int(tie.sum()))
    return out


_LNETS = {}


def make_lattice_net(shape, variant="a"):
    """Dyadic networks.  "a": weights in {0, +-1/4, +-1/2} at 50 % density, biases multiples of 1/4, the embedding multiples
    of 1/64; "b": coarser weights ({0, +-1} at 8 per row, base0: {0, +-1/2, +-1} at 1/4) for the finer features of
    make_lattice_batch(variant="b"), so that base0's and base1's conversions round and tie as well.  The 16 SH columns of col0
    are zero: ray_bias = b_c0 + W_c0[:, embedding columns] embedding[camera] is on the lattice too."""
    key = (shape, variant)
    if key not in _LNETS:
        g = torch.Generator().manual_seed(90210 + (1000 if shape == "fruit_nerf_big" else 0) + (7 if variant == "b" else 0))
        geo = SHAPES[shape][0]

        def pick(values, density, *s):
            v = torch.tensor(values, dtype=F4)[torch.randint(0, len(values), s, generator=g)]
            return (v * (torch.rand(*s, generator=g) < density)).contiguous()

        net = {"shape": shape, "geo": geo, "variant": variant}
        for name, (o, i) in layer_dims(shape).items():
            if name == "col2":      # small: |c3| stays small, s (1 - s) within a few octaves over the three channels
                w = pick([-0.125, 0.125], 0.25, o, i)
            elif name == "head":    # dense (every unit of mlp_semantics receives a gradient) and small (under semgrad the
                w = pick([-1.0, -0.5, 0.5, 1.0], 0.5, o, i) / 64.0   # semantic dX meets the colour dX in one float32 add)
            elif variant == "a":
                w = pick([-0.5, -0.25, 0.25, 0.5], 0.5, o, i)
            elif name == "base0":
                w = pick([-1.0, -0.5, 0.5, 1.0], 0.25, o, i)
            else:
                w = pick([-1.0, 1.0], 5.0 / i if i >= 32 else 0.2, o, i)
            net[name] = (w, pick([-0.5, -0.25, 0.25, 0.5, 0.75], 0.9, o))
        w0 = net["col0"][0]                             # [SH 16 | geo | embedding 32]
        w0[:, 16 + geo:] = pick([-0.5, -0.25, 0.25, 0.5], 0.5, 64, 32)   # either variant: ray_bias gets more than 8 bits
        if variant == "a":                              # (fewer terms per dX sum of the colour gradient's first layer)
            w0[:, 16:16 + geo] *= (torch.rand(64, geo, generator=g) < 0.5)
        w0[:, :16] = 0.0
        net["base1"][0][0] *= 0.25                      # the density logit stays small: exp(h0) within a few octaves
        net["embedding"] = (torch.randint(-48, 49, (N_IMAGES, 32), generator=g).to(F4) / 64.0).contiguous()
        _LNETS[key] = net
    return _LNETS[key]


def make_lattice_batch(R, S, variant="a"):
    """feats [16,N,2]: multiples of 1/8 ("b": of 1/512) within +-0.75; N >= 64: an all-zero feature row, rows of extremes, ~12 %
    of the selector false; directions and cameras as make_batch (LONE_CAM on exactly one ray, UNUSED_CAM on none)."""
    N = R * S
    base = make_batch(R, S)
    g = torch.Generator().manual_seed(31337 * R + 11 * S + (5 if variant == "b" else 0))
    q = 8 if variant == "a" else 512
    feats = torch.randint(-(3 * q) // 4, (3 * q) // 4 + 1, (16, N, 2), generator=g).to(F4) / q
    if N >= 64:
        feats[:, 3] = 0.0
        feats[:, 4] = 0.75
        feats[:, 5] = -0.75
    return dict(base, feats=feats.contiguous(), variant=variant)


def make_lattice_upstream(batch):
    """d_density [N] in {0, +-1/4} (exp(h0) multiplies it), d_rgb [N,3], d_logit [N]: multiples of 1/4 within +-1; N >= 64: a few samples, and with R >= 3 a whole
    ray, zero."""
    N, R, S = batch["N"], batch["R"], batch["S"]
    g = torch.Generator().manual_seed(55 * N + 3)
    dd, dr, dl = (torch.randint(-k, k + 1, sh, generator=g).to(F4) / 4.0 for k, sh in ((1, (N,)), (4, (N, 3)), (4, (N,))))
    keep = torch.ones(N, dtype=F4)
    if N >= 64:
        keep[torch.randint(0, N, (max(2, N // 100),), generator=g)] = 0.0
        if R >= 3:
            keep[S:2 * S] = 0.0
    return dict(dd=(dd * keep).contiguous(), dr=(dr * keep[:, None]).contiguous(), dl=(dl * keep).contiguous())


def exact_outputs(f):
    """forward(..., Arith("bf16" | "f64")) on lattice inputs -> what the device must return bit for bit (float32)."""
    for k in ("h_pad", "geo", "logit", "ray_bias"):
        assert torch.equal(f[k].float().double(), f[k]), k + ": not a float32 number"
    return dict(h_pad=f["h_pad"].float(), geo_out=f["geo"].float(), logit=f["logit"].float(), ray_bias=f["ray_bias"].float())


def transcendental_ratios(got, f, sel):
    """density and rgb against float64 exp / sigmoid of the exact h0 / c3: the formulas of forward_bounds at zero propagated
    error (density: relative 3 u; rgb: 2 u s (1 - s) + 2 u s) -> worst |err| / bound of each."""
    d = torch.exp(f["h"][:, 0]) * sel.double()
    s = torch.sigmoid(f["c3"])
    return {"density": float(((got["density"].double() - d).abs() / (3 * U * d + 1e-300)).max()),
            "rgb": float(((got["rgb"].double() - s).abs() / (2 * U * s * (1 - s) + 2 * U * s)).max())}


def _stable(v32):
    """Whether the bf16 rounding of a float32 value survives a perturbation of +-2 ulp."""
    up = dn = v32
    for _ in range(2):
        up = torch.nextafter(up, torch.full_like(up, math.inf))
        dn = torch.nextafter(dn, torch.full_like(dn, -math.inf))
    r = v32.bfloat16()
    return (up.bfloat16() == r) & (dn.bfloat16() == r)


def transcendental_grads(up, density, rgb):
    """d_c3 = (d_rgb s) (1 - s) and d_h0 = d_density density in float32, the kernels' operation order, from the RETURNED
    float32 rgb and density (density = expf(h0) [selector], and |h0| < 15 on the lattice: expf(clamp(h0)) is the same call)."""
    return (up["dr"] * rgb) * (1.0 - rgb), up["dd"] * density


def guard(up, density, rgb):
    """The fair-question guard: a sample whose d_h0 (or a d_c3 channel) would round to another bf16 value under +-2 ulp gets its
    d_density (its d_rgb row) zeroed and stays in the batch.  -> (upstream, guarded samples [N] bool)."""
    d_c3, d_h0 = transcendental_grads(up, density, rgb)
    bad_c, bad_h = ~_stable(d_c3).all(1), ~_stable(d_h0)
    new = dict(dd=(up["dd"] * (~bad_h)).contiguous(), dr=(up["dr"] * (~bad_c)[:, None]).contiguous(), dl=up["dl"])
    return new, bad_c | bad_h


class Sum:
    """A gradient entry as the sum the device forms: value (float64), sum of |addends|, lowest set bit among the addends,
    number of addends; extra: a bound term outside the summation's own (the SH columns)."""

    def __init__(self, val, mag, lb, n, extra=None):
        n = n if torch.is_tensor(n) else torch.full_like(val, float(n))
        self.val, self.mag, self.lb, self.n, self.extra = val, mag, lb, n, torch.zeros_like(val) if extra is None else extra

    def plus(self, pre, mask=None):
        """... added to a pre-filled float32 gradient (mask: where the device adds at all)."""
        pre = pre.double()
        m = torch.ones_like(pre, dtype=torch.bool) if mask is None else mask
        return Sum(self.val + pre, self.mag + pre.abs(), torch.where(m, torch.minimum(self.lb, lowbit(pre)), self.lb),
                   self.n + m.double(), self.extra)

    def exact(self):
        return bits_of(self.mag, self.lb) < 24.0

    def bound(self):
        return (self.n - 1).clamp_min(0) * 2.0 ** -23 * self.mag + self.extra


def _dw_sum(ar, G, X, layer, keep):
    Gr = (G if ("g_unrounded", layer) in ar.mut else ar.rnd(G)) * keep
    Xr = ar.rnd(X)
    return Sum(Gr.T @ Xr, Gr.abs().T @ Xr.abs(), _minplus(lowbit(Gr), lowbit(Xr)), G.shape[0])


def _row_sum(ar, G, pipe, keep):
    Gq = (ar.rnd(G) if pipe else G) * keep
    return Sum(Gq.sum(0), Gq.abs().sum(0), lowbit(Gq).amin(0), G.shape[0])


def bf16_backward(net, batch, up, ar, semgrad=False, mut=(), returned=None):
    """The backward of the NS = 1 kernels on lattice inputs (the comment above says where every rounding sits).  returned: the
    device's float32 (density, rgb), else the reference's own rounded to float32.  -> (forward dict, {layer: (Sum W, Sum b),
    "embedding": Sum, "d_feats": float64 [16,N,2]}); ar.log (trace) receives the dX chain."""
    geo, S, N = net["geo"], batch["S"], batch["N"]
    big = len(SHAPES[net["shape"]][1]) == 2
    with torch.no_grad():
        p = params(net, F8)
        f = forward(net, batch, ar, p=p)
        assert float(f["h"][:, 0].abs().max()) < 15.0, "the lattice keeps h0 inside trunc_exp's clamp"
        sel = batch["sel"].double()
        density, rgb = returned if returned is not None else ((torch.exp(f["h"][:, 0]) * sel).float(), f["rgb"].float())
        d_c3, d_h0 = transcendental_grads(up, density, rgb)
        keep = torch.ones(N, 1, dtype=F8)
        if "drop_tile" in mut:
            t0 = 16 * ((N // 16) // 2)
            keep[t0:t0 + 16] = 0.0
        const, gcol = _cols(geo)
        ray = torch.arange(N) // S
        out = {}
        # colour branch
        G3 = d_c3.double()
        r1c, r2c = torch.relu(f["c1"]), torch.relu(f["c2"])
        out["col2"] = (_dw_sum(ar, G3, r2c, "col2", keep), _row_sum(ar, G3, False, keep))
        G2 = ar.dx(G3, p["col2"][0], "col2") * (f["c2"] > 0)
        out["col1"] = (_dw_sum(ar, G2, r1c, "col1", keep), _row_sum(ar, G2, False, keep))
        G1 = ar.dx(G2, p["col1"][0], "col1") * (f["c1"] > 0)
        w0 = p["col0"][0]
        Gq = (ar.rnd(G1) if S >= 16 else G1) * keep                        # what the per-ray sums add up
        lq = lowbit(Gq)
        c_ray = f["c_ray"][ray]                                            # [N,48]
        wg = _dw_sum(ar, G1, f["geo"], "col0", keep)
        val, mag, lb = (torch.zeros(64, 48 + geo, dtype=F8) for _ in range(3))
        nn, extra = torch.full((64, 48 + geo), float(N), dtype=F8), torch.zeros(64, 48 + geo, dtype=F8)
        val[:, gcol], mag[:, gcol], lb[:, gcol] = wg.val, wg.mag, wg.lb
        val[:, const], mag[:, const] = Gq.T @ c_ray, Gq.abs().T @ c_ray.abs()
        lb[:, const] = _minplus(lq, lowbit(c_ray))
        sh_abs = sh16((batch["dirs"].double() + 1.0) / 2.0, absolute=True)[ray]
        extra[:, :16] = 4 * U * (Gq.abs().T @ sh_abs)
        nn[:, :16] = N + 1.0
        out["col0"] = (Sum(val, mag, lb, nn, extra), Sum(Gq.sum(0), Gq.abs().sum(0), lq.amin(0), N))
        # embedding row c, column k: sum over o and the samples s of camera c's rays of W_c0[o, 16 + geo + k] Gq[s, o]
        we = w0[:, const[16:]]                                             # [64,32], not rounded
        cam_s = batch["cam"][ray]
        z = lambda: torch.zeros(N_IMAGES, 64, dtype=F8)   # noqa: E731
        g_cam, a_cam = z().index_add_(0, cam_s, Gq), z().index_add_(0, cam_s, Gq.abs())
        l_cam = torch.stack([lq[cam_s == c].amin(0) if bool((cam_s == c).any()) else torch.full((64,), BIG_LB, dtype=F8)
                             for c in range(N_IMAGES)])
        n_cam = 64.0 * torch.bincount(cam_s, minlength=N_IMAGES).double()[:, None].expand(N_IMAGES, 32)
        out["embedding"] = Sum(g_cam @ we, a_cam @ we.abs(), _minplus(l_cam.T.contiguous(), lowbit(we)), n_cam)
        Gh = torch.zeros(N, 1 + geo, dtype=F8)
        Gh[:, 1:] = ar.dx(G1, w0[:, gcol], "col0")
        # semantic branch
        sem = [k for k in layer_names(net["shape"]) if k.startswith("sem")]
        Gs = up["dl"].double()[:, None]
        if big:                    # W_sem2 v + b_sem2 sum(bf(dlogit)): s3 is not rounded, W_sem2 is the float32 tensor
            dl, s2 = ar.rnd(Gs) * keep, ar.rnd(f["in_" + sem[-1]])
            w2, b2 = p[sem[-1]]
            mag = (dl.abs().T @ s2.abs()) @ w2.abs().T + b2.abs()[None] * dl.abs().sum()
            lb = lowbit(dl).amin() + torch.minimum(_minplus(lowbit(s2).amin(0, keepdim=True).T.contiguous(), lowbit(w2).T.contiguous()),
                                                   lowbit(b2)[None])
            out["head"] = (Sum((dl.T @ s2) @ w2.T + b2[None] * dl.sum(), mag, lb, N * (w2.shape[1] + 1)), _row_sum(ar, Gs, True, keep))
        else:
            out["head"] = (_dw_sum(ar, Gs, f["in_head"], "head", keep), _row_sum(ar, Gs, False, keep))
        Gs = ar.dx(Gs, p["head"][0], "head")
        for i, k in reversed(list(enumerate(sem))):
            if i != len(sem) - 1:
                Gs = Gs * (f["pre_" + k] > 0)
            out[k] = (_dw_sum(ar, Gs, f["in_" + k], k, keep), _row_sum(ar, Gs, big, keep))
            if i > 0 or semgrad:
                Gs = ar.dx(Gs, p[k][0], k)
        if semgrad:
            ar._note("add", "d_h", torch.stack([Gh[:, 1:].reshape(-1), Gs.reshape(-1)], 1), torch.ones(1, 2, dtype=F8), Gs)
            Gh[:, 1:] += Gs
        Gh[:, 0] = d_h0.double() * sel
        # base branch
        r1 = torch.relu(f["a1"])
        out["base1"] = (_dw_sum(ar, Gh, r1, "base1", keep), _row_sum(ar, Gh, False, keep))
        Ga = ar.dx(Gh, p["base1"][0], "base1") * (f["a1"] > 0)
        out["base0"] = (_dw_sum(ar, Ga, f["x"], "base0", keep), _row_sum(ar, Ga, False, keep))
        out["d_feats"] = x_to_feats(ar.dx(Ga, p["base0"][0], "base0")).contiguous()
    return f, out


def sums_to_tensors(out):
    """bf16_backward's result as plain gradients (what a device that forms every sum exactly would return)."""
    return {k: (tuple(s.val for s in v) if isinstance(v, tuple) else v.val if isinstance(v, Sum) else v) for k, v in out.items()}


def exact_compare(net, got, ref, prefill=None):
    """got: the device's (or a mutated emulation's) gradients; ref: bf16_backward's.  -> {tensor: dict(entries, compared =
    entries with a non-empty sum, exact = of those under the condition, wrong = exact entries that differ, ratio = worst
    |err| / bound of the others)} for "d_feats", "embedding" and "<layer>.w" / "<layer>.b"."""
    res = {}

    def one(name, g, s, pre, mask=None):
        if pre is not None:
            s = s.plus(pre, mask)
        g = g.double()
        ex = s.exact()
        err = (g - s.val).abs()
        rest = ~ex
        ratio = float((err[rest] / s.bound()[rest].clamp_min(1e-300)).max()) if bool(rest.any()) else 0.0
        res[name] = dict(entries=g.numel(), compared=int((s.mag > 0).sum()), exact=int((ex & (s.mag > 0)).sum()),
                         wrong=int((err[ex] != 0).sum()), ratio=ratio)

    for k in layer_names(net["shape"]):
        for j, suffix in enumerate((".w", ".b")):
            one(k + suffix, got[k][j], ref[k][j], None if prefill is None else prefill[k][j])
    e = ref["embedding"]
    one("embedding", got["embedding"], e, None if prefill is None else prefill["embedding"], e.val != 0)   # `if (s != 0) +=`
    d = got["d_feats"].double()
    res["d_feats"] = dict(entries=d.numel(), compared=d.numel(), exact=d.numel(), wrong=int((d != ref["d_feats"]).sum()), ratio=0.0)
    return res


def exact_failures(res):
    return {k: (v["wrong"], round(v["ratio"], 3)) for k, v in res.items() if v["wrong"] or not v["ratio"] <= 1.0}


_LPREP = {}


def prepare_lattice(shape, R, S, variant="a"):
    """Network, batch and upstream gradients of a lattice case, made once."""
    key = (shape, R, S, variant)
    if key not in _LPREP:
        batch = make_lattice_batch(R, S, variant)
        _LPREP[key] = dict(net=make_lattice_net(shape, variant), batch=batch, up=make_lattice_upstream(batch))
    return _LPREP[key]
