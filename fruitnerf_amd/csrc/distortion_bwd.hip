// distortion_bwd.hip — backward of Nerfacto's distortion loss (use_distortion_loss; nerfstudio 0.3.2 distortion_loss /
// lossfun_distortion on the FINAL level) for gfx950, one wave per ray:
//   loss = mult * mean_r D_r,  D_r = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 ds_i
// with m_i / ds_i the midpoint / width of spacing bin i (detached) and w the field's compositing weights, so
//   dL/dw_k = (mult / R) g (2 sum_j w_j |m_k - m_j| + (2/3) w_k ds_k),  g = the upstream scalar,
// which RaySamples.get_weights carries into the field's density: the weights backward of composite_math.hpp runs in the same
// wave and its result is ADDED to the d_density the compositing backward left.  The forward value is fnr_distortion's /
// fnr_train_losses' (train.hip: distortion_wave).
#include "common.hpp"
#include "composite_math.hpp"
#include "sequencer.hpp"

namespace fnr {

// SCALE: use_gradient_scaling — the density term is multiplied by s_k = clamp(m_euclid_k^2, 0, 1) before it is added.
// ME: samples per lane the register arrays hold (with_lane_elems).  Lane `lane` holds samples lane * E + e, e < E.
template <bool SCALE, int ME>
__global__ __launch_bounds__(256) void k_distortion_bwd(long long R, int S, const float* __restrict__ spacing,
                                                        const float* __restrict__ euclid,
                                                        const float* __restrict__ density,
                                                        const float* __restrict__ weights, float mult,
                                                        const float* __restrict__ upstream,   // optional device scalar
                                                        float* __restrict__ d_weights,        // optional [R,S]
                                                        float* __restrict__ d_density) {      // [R,S] in/out
  static_assert(ME <= WB_MAXE, "the lane layout of the per-ray family");
  // per wave: midpoints and weights of its ray, 64 ME floats each (S <= 64 ME), read back in groups of four
  __shared__ __attribute__((aligned(16))) float lds[4 * 2 * 64 * ME];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * 4 + wave;
  if (r >= R) return;
  const int E = (S + 63) >> 6;
  float* s_m = lds + wave * (2 * 64 * ME);
  float* s_w = s_m + 64 * ME;
  const float* t = spacing + r * (S + 1);
  const float* eb = euclid + r * (S + 1);
  const float* dn = density + r * S;
  const float* w = weights + r * S;
  const float coef = mult / (float)R * (upstream ? upstream[0] : 1.0f);
  float mk[ME], ds[ME], delta[ME], wk[ME];
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    mk[e] = 0.0f;
    ds[e] = 0.0f;
    delta[e] = 0.0f;
    wk[e] = 0.0f;
    if (e < E && k < S) {
      const float t0 = t[k], t1 = t[k + 1];
      mk[e] = (t1 + t0) / 2.0f;
      ds[e] = t1 - t0;
      delta[e] = eb[k + 1] - eb[k];
      wk[e] = w[k];
      s_m[k] = mk[e];
      s_w[k] = wk[e];
    }
  }
  const int S4 = (S + 3) & ~3;   // <= 64 ME; the tail of the last group of four weighs nothing
  if (lane < S4 - S) {
    s_m[S + lane] = 0.0f;
    s_w[S + lane] = 0.0f;
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  // sum_j w_j |m_k - m_j| directly: S terms >= 0 per sample, no cancellation (the prefix-sum form subtracts nearly equal
  // totals); every lane reads the same four (m_j, w_j) — an LDS broadcast — into four partial sums per sample
  float acc[ME][4];
#pragma unroll
  for (int e = 0; e < ME; ++e) acc[e][0] = acc[e][1] = acc[e][2] = acc[e][3] = 0.0f;
  for (int j = 0; j < S4; j += 4) {
    const float4 mj = *reinterpret_cast<const float4*>(s_m + j);
    const float4 wj = *reinterpret_cast<const float4*>(s_w + j);
#pragma unroll
    for (int e = 0; e < ME; ++e) {
      acc[e][0] = fmaf(wj.x, fabsf(mk[e] - mj.x), acc[e][0]);
      acc[e][1] = fmaf(wj.y, fabsf(mk[e] - mj.y), acc[e][1]);
      acc[e][2] = fmaf(wj.z, fabsf(mk[e] - mj.z), acc[e][2]);
      acc[e][3] = fmaf(wj.w, fabsf(mk[e] - mj.w), acc[e][3]);
    }
  }
  float gw[ME];
  float dd_local = 0.0f, gww_local = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    gw[e] = 0.0f;
    if (e < E && k < S) {
      const float inner = (acc[e][0] + acc[e][1]) + (acc[e][2] + acc[e][3]);
      gw[e] = coef * (2.0f * inner + 2.0f * wk[e] * ds[e] / 3.0f);
      if (d_weights) d_weights[r * S + k] = gw[e];
      dd_local += delta[e] * dn[k];
      gww_local += gw[e] * wk[e];
    }
  }
  weights_bwd_ray<false, false, SCALE, ME, true>(r, S, lane, eb, dn, delta, gw, wk, dd_local, gww_local, 0.0f, 0.0f, 0.0f,
                                                 0.0f, 0.0f, d_density, nullptr, nullptr);
}

static auto distortion_bwd_kernel(bool scale, int S) {
  decltype(&k_distortion_bwd<false, 1>) kernel = nullptr;
  with_lane_elems(S, [&](auto me) {
    kernel = scale ? k_distortion_bwd<true, decltype(me)::value> : k_distortion_bwd<false, decltype(me)::value>;
  });
  return kernel;
}

}  // namespace fnr

using namespace fnr;

extern "C" int fnr_distortion_bwd(int64_t n_rays, int S, const float* spacing, const float* euclid_bins,
                                  const float* density, const float* weights, float mult, const float* upstream,
                                  int gradient_scaling, float* d_weights, float* d_density, void* stream) {
  FNR_SEQ_RECORD(fnr_distortion_bwd, n_rays, S, spacing, euclid_bins, density, weights, mult, upstream, gradient_scaling,
                 d_weights, d_density, stream);
  FNR_CHECK_ARG(n_rays >= 0 && spacing && euclid_bins && density && weights && d_density, "distortion_bwd: null argument");
  FNR_CHECK_ARG(S > 0 && S <= 64 * WB_MAXE, "distortion_bwd: S %d out of range", S);
  if (n_rays == 0) return FNR_OK;
  FNR_PROF(OP_DISTORTION, n_rays * (long long)S);
  hipLaunchKernelGGL(distortion_bwd_kernel(gradient_scaling != 0, S), dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0,
                     as_stream(stream), (long long)n_rays, S, spacing, euclid_bins, density, weights, mult, upstream,
                     d_weights, d_density);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}
