// composite_math.hpp — what the per-ray compositing kernels share: the loss gradients and lane-form helpers of train.hip
// (k_train_losses) and composite_bwd.hip, the per-ray forward of render.hip (k_composite_fwd) and composite_bwd.hip
// (k_composite_fwd_bwd), and the backward from the wave scans to the stores that every kernel of composite_bwd.hip ends with.
#pragma once
#include "common.hpp"

namespace fnr {

// The per-ray gradients of the two image losses, unit upstream: d MSELoss(mean over 3 R values) / d rgb_c and
// d (w * BCEWithLogitsLoss(mean over R)) / d logit.  ONE definition for every kernel that forms them — losses_block,
// k_train_losses and the composite backward that takes the targets itself (k_composite_bwd<TARGETS>): the bit-identity of
// those paths (tests/test_gpu_training_parity.py::test_composite_bwd_targets_is_losses_then_composite_bwd) rests on it.
__device__ __forceinline__ float mse_grad(float diff, float inv3r) { return 2.0f * diff * inv3r; }
__device__ __forceinline__ float bce_logit_grad(float x, float y, float sem_weight, float invr) {
  const float sg = 1.0f / (1.0f + expf(-x));
  return sem_weight * (sg - y) * invr;
}

constexpr int WB_MAXE = 8;   // samples per lane in the per-ray weight kernels (S <= 512)
static_assert(WB_MAXE == RAY_MAX_LANE_ELEMS, "with_lane_elems picks the kernel");

// The per-ray weight kernels are compiled per ME, the samples a lane's register arrays hold (common.hpp: with_lane_elems).  A
// narrower form does what the eight-wide one does: the elements it drops are zeros, added to sums that start from +0.0 or
// behind the live elements (no effect), with one exception — `suffix += 0 * 0` AHEAD of the live elements turns a suffix of
// -0.0 into +0.0.  padded_suffix() keeps that one addition (x + 0.0 + 0.0 == x + 0.0; at ME = 8 a full lane never had it).
template <int ME>
__device__ __forceinline__ float padded_suffix(float suffix) {
  if constexpr (ME < WB_MAXE) suffix += 0.0f;
  return suffix;
}

// TARGETS (fnr_composite_bwd_targets): the per-ray loss gradients are not read from memory but formed here from the
// composited outputs and the batch — g_rgb = 2 (rgb - image) / (3 R), g_sem = w_sem (sigmoid(sem) - mask) / R: the very
// expressions of k_train_losses, so the same bits — which makes this launch independent of the losses launch: a training
// step runs the MLP backward straight behind the forward while the loss VALUES (and the interlevel loss with the proposal
// levels' weights backward) are summed on the second stream.
struct LossTargets {
  const float* out_rgb;    // [R,3] composited colour
  const float* image;      // [R,3]
  const float* out_sem;    // [R]   composited logit
  const float* mask;       // [R]
  float sem_weight;
};
// SEMGRAD (pass_semantic_gradients, fruit_nerf.py:344-345): the semantic renderer's weights are NOT detached, so the semantic
// term joins the upstream gradient of the weights, gw[k] += g_sem logit_k, and the rest of the kernel carries it into d_density.
// BG (background_color "white" / "black" / "random"): the background is an explicit triple, row r * bg_stride of `bg`, a
// constant of the pass — it takes the last sample's place in dL/dw_k = g_rgb . (c_k - b) and sample S-1 gets no background share.
// SCALE (use_gradient_scaling, nerfstudio scale_gradients_by_distance_squared): every gradient that leaves towards the field —
// d_density, d_rgb, d_logit of sample k — is multiplied by s_k = clamp(m_k^2, 0, 1), m_k the bin's Euclidean midpoint.
// <.., false, false> is the code it was: the two switches only add to it.
__device__ __forceinline__ float distance_squared_scale(float e0, float e1) {
  const float m = fdiv(fadd(e0, e1), 2.0f);
  return fminf(fmaxf(fmul(m, m), 0.0f), 1.0f);
}

// fnr_composite_options on the host: {last sample, no scaling} is the entry point without options (its launch, its name in a
// step program), with the semantic weights detached or attached.
static inline bool composite_options_plain(const fnr_composite_options* o) {
  return o->background == FNR_BACKGROUND_LAST_SAMPLE && !o->gradient_scaling;
}
#define FNR_CHECK_COMPOSITE_OPTIONS(what, o)                                                                             \
  FNR_CHECK_ARG(composite_options_ok(o), what ": options NULL or background %d (0 = last sample, 1 = explicit with a "   \
                "buffer of row stride 0 or 3)", (o) ? (int)(o)->background : -1)

// ---------------------------------------------------------------------------------------------------
// The forward of one ray by its wave: RaySamples.get_weights, the weighted sums of the renderers and the median sample.  Lane
// `lane` holds samples lane * E + e, e < E = ceil(S / 64) <= ME.  Writes the weights; leaves them in w[] (zero beyond S), the
// five sums (accumulation, colour without its background term, logit) in every lane, and the first sample at which the
// cumulative weight reaches 0.5 (S - 1 if none) in `first`.  training = 0: the colours go through nan_to_num.
// ---------------------------------------------------------------------------------------------------
template <int ME>
__device__ __forceinline__ void composite_fwd_ray(long long r, int S, int lane, const float* eb, const float* dn,
                                                  const float* cs, const float* lg, int training,
                                                  float* __restrict__ weights, float (&w)[ME], float& acc, float& cr,
                                                  float& cg, float& cb, float& sm, int& first) {
  const int E = (S + 63) >> 6;
  float dd[ME];
  float local = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    dd[e] = 0.0f;
    if (e < E && k < S) dd[e] = fmul(fsub(eb[k + 1], eb[k]), dn[k]);
    local += dd[e];
  }
  float excl = wave_excl_scan(local, lane);
  float acc_l = 0.0f;
  cr = 0.0f, cg = 0.0f, cb = 0.0f, sm = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    const float T = expf(-excl);
    const float alpha = 1.0f - expf(-dd[e]);
    w[e] = nan_to_num(alpha * T);
    excl += dd[e];
    if (e < E && k < S) {
      weights[r * S + k] = w[e];
      float c0 = cs[3 * k], c1 = cs[3 * k + 1], c2 = cs[3 * k + 2];
      if (!training) {
        c0 = nan_to_num(c0);
        c1 = nan_to_num(c1);
        c2 = nan_to_num(c2);
      }
      acc_l += w[e];
      cr = fmaf(w[e], c0, cr);
      cg = fmaf(w[e], c1, cg);
      cb = fmaf(w[e], c2, cb);
      sm = fmaf(w[e], lg[k], sm);
    } else {
      w[e] = 0.0f;
    }
  }
  // median depth before the reductions destroy the per-lane partials
  float cw = wave_excl_scan(acc_l, lane);
  first = 0x7fffffff;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    cw += w[e];
    if (e < E && k < S && cw >= 0.5f && first == 0x7fffffff) first = k;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) first = min(first, __shfl_xor(first, d, 64));
  if (first > S - 1) first = S - 1;

  acc = wave_sum(acc_l);
  cr = wave_sum(cr);
  cg = wave_sum(cg);
  cb = wave_sum(cb);
  sm = wave_sum(sm);
}

// ---------------------------------------------------------------------------------------------------
// backward of w_i = (1 - exp(-d_i s_i)) exp(-sum_{j<i} d_j s_j):
//   dL/ds_k = d_k [ g_k T_{k+1} - sum_{i>k} g_i w_i ],  T_{k+1} = exp(-sum_{j<=k} d_j s_j)
// from the wave scans to the stores, for a ray whose wave holds delta = the bin widths, gw = dL/dw_k, wk = the weights (all
// zero beyond S) and the lane's sums of delta * density, gw * wk and wk.  COMPOSITE: d_rgb and d_logit too, from the per-ray
// gradients (gr, gg, gb, gs).  ACCUM (k_distortion_bwd): the finished (scaled) density term is ADDED to what d_density holds,
// one float32 addition; false is the code it was.
// ---------------------------------------------------------------------------------------------------
template <bool COMPOSITE, bool BG, bool SCALE, int ME, bool ACCUM = false>
__device__ __forceinline__ void weights_bwd_ray(long long r, int S, int lane, const float* eb, const float* dn,
                                                const float (&delta)[ME], const float (&gw)[ME], const float (&wk)[ME],
                                                float dd_local, float gww_local, float wsum_local, float gr, float gg,
                                                float gb, float gs, float* __restrict__ d_density,
                                                float* __restrict__ d_rgb, float* __restrict__ d_logit) {
  const int E = (S + 63) >> 6;
  float bgw = 0.0f;
  float cum_dd = wave_excl_scan(dd_local, lane);     // sum_{j<first k of lane}
  // sum_{i>k} g_i w_i as a true SUFFIX sum (reverse scan), not `total - prefix`: behind a surface the suffix is a sum of
  // tiny terms while total and prefix agree to 7 digits, and dL/dsigma there is multiplied by sigma (up to e^15) in the
  // trunc_exp backward — the cancellation error was comparable to the real gradient (autograd's cumsum backward is a
  // reverse cumsum, i.e. exact in this sense).
  float suffix =
      padded_suffix<ME>(wave_bcast_lane(wave_excl_scan(wave_bcast_lane(gww_local, 63 - lane), lane), 63 - lane));
  if (COMPOSITE && !BG) bgw = 1.0f - wave_sum(wsum_local);
  float suf[ME];   // suffix AFTER element e of this lane's chunk
#pragma unroll
  for (int e = ME - 1; e >= 0; --e) {
    suf[e] = suffix;
    suffix += gw[e] * wk[e];   // gw / wk are 0 for e >= E or k >= S
  }
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    if (e < E && k < S) {
      cum_dd += delta[e] * dn[k];   // inclusive of k
      const float T_next = expf(-cum_dd);
      float s = 1.0f;
      if constexpr (SCALE) s = distance_squared_scale(eb[k], eb[k + 1]);
      const auto leaving = [s](float g) { return SCALE ? s * g : g; };   // a gradient on its way to the field
      const float dk = leaving(delta[e] * (gw[e] * T_next - suf[e]));
      if constexpr (ACCUM) d_density[r * S + k] = d_density[r * S + k] + dk;
      else d_density[r * S + k] = dk;
      if (COMPOSITE) {
        float f = wk[e];
        if (!BG && k == S - 1) f += bgw;  // background = last sample's colour (RGBRenderer "last_sample")
        float* o = d_rgb + (r * S + k) * 3;
        o[0] = leaving(gr * f);
        o[1] = leaving(gg * f);
        o[2] = leaving(gb * f);
        d_logit[r * S + k] = leaving(gs * wk[e]);
      }
    }
  }
}

}  // namespace fnr
