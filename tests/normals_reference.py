"""Shared by tests/test_normals_cpu.py and tests/test_gpu_normals.py: the analytic normals of FruitField (fnr_field_normals,
fnr_render_normals; csrc/field_normals.hip) as float64 torch, a float32 emulation of the kernel's arithmetic, the running
error estimate of the gradient and the cases.  The network, the batches and the kink margins are tests/field_reference.py's.

Per sample, x [32] the hash features (column 2 l + j), J [16][3][N][2] the encode's input Jacobian:
  a1 = W_b0 x + b_b0,  v = 1[a1 > 0] * W_b1[row, :] (row 0: the density logit),  df = W_b0^T v  [32]
  g[a] = sum_{l,j} J[l][a][n][j] df[2 l + j],  normal = -g / max(||g||, 1e-12);  unselected samples: g = 0, normal = 0

Error estimate (first order, roundings independent, in the style of field_reference; u = 2^-24).  The gates are exact once
the samples next to a kink of a1 are left out (kink_of_a1).  v is exact (a copy of weights), so
  E_df[k] = sqrt(65) u sum_h |v_h| |W_b0[h, k]|                            a chain of 64 fmas
  E_g[a]  = sqrt(34) u sum_{l,j} |J| |df| + sqrt(sum_{l,j} (J E_df)^2)      a chain of 32 fmas + the propagated E_df
  E = ||E_g||_2 over the three axes
and the normal, n = -g / ||g||, errs by at most 2 |dg| / ||g|| (the change of g plus the change of its norm) plus the
roundings of the three squares, two sums, the root and the quotient: the bound of a sample is
  ||n_got - n_ref||_2 <= C_NORMALS (2 E / ||g|| + 4 u).
C_NORMALS is measured on the float32 emulation (tests/test_normals_cpu.py asserts the factor 4), not guessed.
"""
import math

import torch

from tests import field_reference as fr

F8, F4, U = fr.F8, fr.F4, fr.U
SHAPE_LIST = list(fr.SHAPES)
CASES = list(fr.CASES) + [(33, 48)]

# >= 4 x the worst ||err|| / (2 E / ||g|| + 4 u) of the float32 emulation over CASES x both shapes (measured: see the
# docstring of tests/test_gpu_normals.py)
C_NORMALS = 0.25


def case_inputs(shape, R, S):
    """-> net, batch (field_reference's, with its per-case seed), jac [16,3,N,2] float32 uniform in +-64 seeded per case."""
    net = fr.make_net(shape, 0)
    batch = fr.make_batch(R, S, fr.CASE_SEED.get((shape, R, S), 0))
    g = torch.Generator().manual_seed(7919 * R + 31 * S + 1000003 * SHAPE_LIST.index(shape))
    jac = ((torch.rand(16, 3, batch["N"], 2, generator=g, dtype=F4) * 2 - 1) * 64.0).contiguous()
    return net, batch, jac


def kink_of_a1(net, batch, f):
    """Samples with a base-layer pre-activation within C["fp32"]["pre.a1"] x its margin of 0 (the kernel's one arithmetic is
    a float32 fmaf chain): their gate, hence their normal, may legitimately flip."""
    m = fr.forward_bounds(net, batch, f, "fp32")
    return (f["a1"].abs() <= fr.C["fp32"]["pre.a1"] * m["a1"]).any(1)


def formula(w0, b0, w1_row, x, J):
    """The formulas of the module docstring in the arguments' dtype: w0 [64,32], b0 [64], w1_row [64], x [N,32],
    J [16,3,N,2] -> g [N,3], df [N,32], v [N,64], a1 [N,64] (no selector)."""
    a1 = x @ w0.T + b0
    v = (a1 > 0).to(x.dtype) * w1_row
    df = v @ w0
    g = (fr.x_to_feats(df)[:, None] * J).sum((0, 3)).T
    return g, df, v, a1


def reference(net, batch, jac, row=0, swap_axes=None):
    """float64 -> dict(g [N,3], normals [N,3], E [N], bound [N] (without C_NORMALS), scale [N,3] = sum |df| |J|, f).
    row / swap_axes: the wrong references of the teeth tests (another row of W_b1; two Jacobian axes exchanged)."""
    with torch.no_grad():
        f = fr.forward(net, batch)
        w0 = net["base0"][0].double()
        J = jac.double()
        _, df, v, a1 = formula(w0, net["base0"][1].double(), net["base1"][0][row].double(), f["x"], J)
        assert torch.equal(a1, f["a1"])
        if swap_axes is not None:
            perm = [0, 1, 2]
            perm[swap_axes[0]], perm[swap_axes[1]] = perm[swap_axes[1]], perm[swap_axes[0]]
            J = J[:, perm]
        sel = batch["sel"].double()[:, None]
        g, scale = fr.position_contract(fr.x_to_feats(df), J)
        g = g * sel
        e_df = math.sqrt(65) * U * (v.abs() @ w0.abs())                             # [N,32]
        prop = ((fr.x_to_feats(e_df)[:, None] * J) ** 2).sum((0, 3)).T              # [N,3]
        e_g = math.sqrt(34) * U * scale + torch.sqrt(prop)
        E = e_g.norm(dim=1)
        norm = g.norm(dim=1)
        normals = -g / norm.clamp_min(1e-12)[:, None]
        bound = 2 * E / norm.clamp_min(1e-300) + 4 * U
    return dict(g=g, normals=normals, E=E, bound=bound, scale=scale, norm=norm, f=f)


def _fma(a, b, c):
    """fmaf on float32 tensors: the product is exact in float64, one rounding to float64 ahead of the one to float32."""
    return (a.double() * b.double() + c.double()).float()


def emulate(net, batch, jac):
    """The kernel's float32 arithmetic, chain for chain (csrc/field_normals.hip) -> normals [N,3], g [N,3] (float32)."""
    with torch.no_grad():
        x = fr.feats_to_x(batch["feats"])                                           # [N,32]
        w0, b0 = net["base0"]
        w1 = net["base1"][0][0]
        N = x.shape[0]
        a = b0[None].expand(N, 64).contiguous()
        for k in range(32):
            a = _fma(w0[:, k][None], x[:, k:k + 1], a)
        v = torch.where(a > 0, w1[None].expand(N, 64), torch.zeros(N, 64))
        df = torch.zeros(N, 32)
        for h in range(64):
            df = _fma(v[:, h:h + 1], w0[h][None], df)
        g = torch.zeros(N, 3)
        for l in range(16):
            for ax in range(3):
                for j in range(2):
                    g[:, ax] = _fma(jac[l, ax, :, j], df[:, 2 * l + j], g[:, ax])
        norm = torch.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        n = -(g / norm.clamp_min(1e-12)[:, None])
        sel = batch["sel"][:, None]
        zero = torch.zeros(N, 3)
        return torch.where(sel, n, zero), torch.where(sel, g, zero)


def ratios(got_normals, ref, keep):
    """-> ||got - ref||_2 / bound per kept sample (without C_NORMALS)."""
    err = (got_normals.double() - ref["normals"]).norm(dim=1)
    return (err / ref["bound"])[keep]


def render_reference(weights, normals, shade):
    """NormalsRenderer + safe_normalize (+ NormalsShader) in float64: weights [R,S], normals [R,S,3] -> [R,3]."""
    n = (weights.double()[..., None] * normals.double()).sum(1)
    n = n / (n.norm(dim=1, keepdim=True) + 1e-10)
    return (n + 1.0) / 2.0 if shade else n


def grid_jacobian(encoding, x):
    """d features / d position of an oracle HashEncoding at x [N,3] (its dtype) by autograd, one feature at a time ->
    [16,3,N,2] (the layout fnr_hash_encode_fwd saves)."""
    x = x.detach().clone().requires_grad_(True)
    feats = encoding(x)                                                            # [N,32]
    cols = [torch.autograd.grad(feats[:, k].sum(), x, retain_graph=True)[0] for k in range(feats.shape[1])]
    J = torch.stack(cols, 0)                                                        # [32,N,3]
    return J.view(16, 2, x.shape[0], 3).permute(0, 3, 2, 1).contiguous(), feats.detach()


def autograd_normals(field, x):
    """nerfstudio Field.get_normals on masked unit-cube positions x [N,3] through an oracle FruitField (in x's dtype):
    -> normals [N,3], gradient [N,3]."""
    x = x.detach().clone().requires_grad_(True)
    h0 = field.mlp_base(x)[:, 0]
    g = torch.autograd.grad(h0.sum(), x)[0]
    return -torch.nn.functional.normalize(g, dim=-1), g
