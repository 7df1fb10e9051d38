// render.hip — alpha compositing for gfx950: RaySamples.get_weights + RGBRenderer("last_sample") +
// AccumulationRenderer + DepthRenderer("median") + SemanticRenderer (fruit_nerf.py:325-348), one wave per ray.
#include "common.hpp"
#include "composite_math.hpp"
#include "sequencer.hpp"

namespace fnr {

constexpr int CMP_MAXE = 8;  // S <= 512

// BG: the background colour is not the last sample's but an explicit triple, row r * bg_stride of `bg` (RGBRenderer with
// background_color "white" / "black" / "random": bg_stride 0 = one triple for every ray, 3 = one per ray); it is a constant
// of the pass — never nan_to_num'ed, no gradient.  Everything ahead of the background term is the same code.
template <bool BG>
__device__ __forceinline__ void composite_fwd_body(RaysDev rays, int S, const float* __restrict__ euclid,
                                                   const float* __restrict__ density,
                                                   const float* __restrict__ rgb, const float* __restrict__ logit,
                                                   int training, float* __restrict__ weights,
                                                   float* __restrict__ out_rgb, float* __restrict__ out_acc,
                                                   float* __restrict__ out_depth, float* __restrict__ out_sem,
                                                   long long* __restrict__ out_label, const float* __restrict__ bg,
                                                   int bg_stride) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * 4 + wave;
  if (r >= rays.n_rays) return;
  const float* eb = euclid + r * (S + 1);
  const float* dn = density + r * S;
  const float* cs = rgb + r * S * 3;
  const float* lg = logit + r * S;

  float w[CMP_MAXE];
  float acc, cr, cg, cb, sm;
  int first;
  composite_fwd_ray<CMP_MAXE>(r, S, lane, eb, dn, cs, lg, training, weights, w, acc, cr, cg, cb, sm, first);
  if (lane == 0) {
    // background_color = "last_sample": rgb[..., -1, :] * (1 - accumulated_weight)
    float l0, l1, l2;
    if constexpr (BG) {
      const float* b = bg + r * bg_stride;
      l0 = b[0], l1 = b[1], l2 = b[2];
    } else {
      l0 = cs[3 * (S - 1)], l1 = cs[3 * (S - 1) + 1], l2 = cs[3 * (S - 1) + 2];
      if (!training) {
        l0 = nan_to_num(l0);
        l1 = nan_to_num(l1);
        l2 = nan_to_num(l2);
      }
    }
    const float bgw = 1.0f - acc;
    float o0 = cr + l0 * bgw, o1 = cg + l1 * bgw, o2 = cb + l2 * bgw;
    if (!training) {
      o0 = fminf(fmaxf(o0, 0.0f), 1.0f);
      o1 = fminf(fmaxf(o1, 0.0f), 1.0f);
      o2 = fminf(fmaxf(o2, 0.0f), 1.0f);
    }
    out_rgb[3 * r] = o0;
    out_rgb[3 * r + 1] = o1;
    out_rgb[3 * r + 2] = o2;
    out_acc[r] = acc;
    out_sem[r] = sm;
    // heaviside(sigmoid(semantics) - 0.9, 0) (fruit_nerf.py:309-311, 351-353)
    if (out_label) out_label[r] = (fsub(1.0f / (1.0f + expf(-sm)), 0.9f) > 0.0f) ? 1 : 0;
    out_depth[r] = fdiv(fadd(eb[first], eb[first + 1]), 2.0f);
  }
}

__global__ __launch_bounds__(256) void k_composite_fwd(RaysDev rays, int S, const float* __restrict__ euclid,
                                                       const float* __restrict__ density,
                                                       const float* __restrict__ rgb, const float* __restrict__ logit,
                                                       int training, float* __restrict__ weights,
                                                       float* __restrict__ out_rgb, float* __restrict__ out_acc,
                                                       float* __restrict__ out_depth, float* __restrict__ out_sem,
                                                       long long* __restrict__ out_label) {
  composite_fwd_body<false>(rays, S, euclid, density, rgb, logit, training, weights, out_rgb, out_acc, out_depth, out_sem,
                            out_label, nullptr, 0);
}
__global__ __launch_bounds__(256) void k_composite_fwd_bg(RaysDev rays, int S, const float* __restrict__ euclid,
                                                          const float* __restrict__ density,
                                                          const float* __restrict__ rgb, const float* __restrict__ logit,
                                                          int training, float* __restrict__ weights,
                                                          float* __restrict__ out_rgb, float* __restrict__ out_acc,
                                                          float* __restrict__ out_depth, float* __restrict__ out_sem,
                                                          long long* __restrict__ out_label, const float* __restrict__ bg,
                                                          int bg_stride) {
  composite_fwd_body<true>(rays, S, euclid, density, rgb, logit, training, weights, out_rgb, out_acc, out_depth, out_sem,
                           out_label, bg, bg_stride);
}

}  // namespace fnr

using namespace fnr;

extern "C" int fnr_composite_fwd(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                 const float* rgb, const float* logit, int training, float* weights, float* out_rgb,
                                 float* out_accumulation, float* out_depth, float* out_semantics,
                                 int64_t* out_label, void* stream) {
  FNR_SEQ_RECORD(fnr_composite_fwd, rays, S, euclid_bins, density, rgb, logit, training, weights, out_rgb, out_accumulation,
                 out_depth, out_semantics, out_label, stream);
  FNR_CHECK_ARG(rays && euclid_bins && density && rgb && logit && weights && out_rgb && out_accumulation &&
                    out_depth && out_semantics,
                "composite_fwd: null argument");
  FNR_CHECK_ARG(S > 0 && S <= 64 * CMP_MAXE, "composite_fwd: S %d out of range", S);
  if (rays->n_rays == 0) return FNR_OK;
  FNR_PROF(OP_COMPOSITE_FWD, rays->n_rays * (long long)S);
  hipLaunchKernelGGL(k_composite_fwd, dim3((unsigned)((rays->n_rays + 3) / 4)), dim3(256), 0, as_stream(stream),
                     make_rays(rays), S, euclid_bins, density, rgb, logit, training, weights, out_rgb,
                     out_accumulation, out_depth, out_semantics, reinterpret_cast<long long*>(out_label));
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

// fnr_composite_fwd under fnr_composite_options: the forward values depend on the background alone (gradient scaling and
// the semantic switch are backward-only), so with the last sample as background this IS fnr_composite_fwd.
extern "C" int fnr_composite_fwd_opt(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                     const float* rgb, const float* logit, int training, const fnr_composite_options* opt,
                                     float* weights, float* out_rgb, float* out_accumulation, float* out_depth,
                                     float* out_semantics, int64_t* out_label, void* stream) {
  if (composite_options_ok(opt) && opt->background == FNR_BACKGROUND_LAST_SAMPLE)
    return fnr_composite_fwd(rays, S, euclid_bins, density, rgb, logit, training, weights, out_rgb, out_accumulation,
                             out_depth, out_semantics, out_label, stream);
  FNR_SEQ_RECORD(fnr_composite_fwd_opt, rays, S, euclid_bins, density, rgb, logit, training, opt, weights, out_rgb,
                 out_accumulation, out_depth, out_semantics, out_label, stream);
  FNR_CHECK_COMPOSITE_OPTIONS("composite_fwd_opt", opt);
  FNR_CHECK_ARG(rays && euclid_bins && density && rgb && logit && weights && out_rgb && out_accumulation && out_depth &&
                    out_semantics,
                "composite_fwd_opt: null argument");
  FNR_CHECK_ARG(S > 0 && S <= 64 * CMP_MAXE, "composite_fwd_opt: S %d out of range", S);
  if (rays->n_rays == 0) return FNR_OK;
  FNR_PROF(OP_COMPOSITE_FWD, rays->n_rays * (long long)S);
  hipLaunchKernelGGL(k_composite_fwd_bg, dim3((unsigned)((rays->n_rays + 3) / 4)), dim3(256), 0, as_stream(stream),
                     make_rays(rays), S, euclid_bins, density, rgb, logit, training, weights, out_rgb, out_accumulation,
                     out_depth, out_semantics, reinterpret_cast<long long*>(out_label), opt->background_rgb,
                     (int)opt->background_stride);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}
