// composite_bwd.hip — backward of RaySamples.get_weights + renderers (fruit_nerf.py:325-348) for gfx950, one wave per ray:
//   k_weights_bwd        a proposal level's weights backward (fnr_weights_bwd)
//   k_composite_bwd      the final level's compositing backward, from given per-ray gradients or from the loss targets
//   k_composite_fwd_bwd  the compositing forward and that backward in one launch
// and their ten entry points, which share one launch path.  The per-ray arithmetic is composite_math.hpp's.
#include "common.hpp"
#include "composite_math.hpp"
#include "sequencer.hpp"

namespace fnr {

// TARGETS, SEMGRAD, BG, SCALE: composite_math.hpp.  ME: samples per lane the register arrays hold (with_lane_elems).
template <bool COMPOSITE, bool TARGETS, bool SEMGRAD, bool BG, bool SCALE, int ME>
__device__ __forceinline__ void weights_bwd_body(long long R, int S, const float* __restrict__ euclid,
                                                 const float* __restrict__ density, const float* __restrict__ weights,
                                                 const float* __restrict__ d_w_in,    // !COMPOSITE: [R,S]
                                                 const float* __restrict__ upstream,  // optional device scalar
                                                 const float* __restrict__ rgb,       // COMPOSITE: samples [N,3]
                                                 const float* __restrict__ g_rgb,     // COMPOSITE: [R,3]
                                                 const float* __restrict__ g_sem,     // COMPOSITE: [R]
                                                 float* __restrict__ d_density, float* __restrict__ d_rgb,
                                                 float* __restrict__ d_logit, const LossTargets& tg,
                                                 const float* __restrict__ logit,     // SEMGRAD: samples [N]
                                                 const float* __restrict__ bg,        // BG: rows of 3, stride bg_stride
                                                 int bg_stride) {
  static_assert(COMPOSITE || !SEMGRAD, "the semantic term belongs to the compositing backward");
  static_assert(COMPOSITE || !(BG || SCALE), "background and gradient scaling belong to the compositing backward");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * 4 + wave;
  if (r >= R) return;
  const int E = (S + 63) >> 6;
  const float* eb = euclid + r * (S + 1);
  const float* dn = density + r * S;
  const float* w = weights + r * S;
  const float up = upstream ? upstream[0] : 1.0f;
  float gr = 0.0f, gg = 0.0f, gb = 0.0f, gs = 0.0f, l0 = 0.0f, l1 = 0.0f, l2 = 0.0f;
  if (COMPOSITE) {
    if constexpr (TARGETS) {
      const float inv3r = 1.0f / (float)(3 * R), invr = 1.0f / (float)R;   // (k_train_losses, rgb / semantic role)
      const float d0 = tg.out_rgb[3 * r] - tg.image[3 * r], d1 = tg.out_rgb[3 * r + 1] - tg.image[3 * r + 1],
                  d2 = tg.out_rgb[3 * r + 2] - tg.image[3 * r + 2];
      gr = mse_grad(d0, inv3r);
      gg = mse_grad(d1, inv3r);
      gb = mse_grad(d2, inv3r);
      gs = bce_logit_grad(tg.out_sem[r], tg.mask[r], tg.sem_weight, invr);
    } else {
      gr = g_rgb[3 * r];
      gg = g_rgb[3 * r + 1];
      gb = g_rgb[3 * r + 2];
      gs = g_sem[r];
    }
    const float* cl = BG ? bg + r * bg_stride : rgb + (r * S + (S - 1)) * 3;
    l0 = cl[0];
    l1 = cl[1];
    l2 = cl[2];
  }
  float delta[ME], gw[ME], wk[ME];
  float dd_local = 0.0f, gww_local = 0.0f, wsum_local = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    delta[e] = 0.0f;
    gw[e] = 0.0f;
    wk[e] = 0.0f;
    if (e < E && k < S) {
      delta[e] = eb[k + 1] - eb[k];
      wk[e] = w[k];
      if (COMPOSITE) {
        const float* c = rgb + (r * S + k) * 3;
        gw[e] = gr * (c[0] - l0) + gg * (c[1] - l1) + gb * (c[2] - l2);  // semantic weights are detached unless SEMGRAD
        if constexpr (SEMGRAD) gw[e] += gs * logit[r * S + k];
      } else {
        gw[e] = d_w_in[r * S + k] * up;
      }
      dd_local += delta[e] * dn[k];
      gww_local += gw[e] * wk[e];
      wsum_local += wk[e];
    }
  }
  weights_bwd_ray<COMPOSITE, BG, SCALE, ME>(r, S, lane, eb, dn, delta, gw, wk, dd_local, gww_local, wsum_local, gr, gg, gb,
                                            gs, d_density, d_rgb, d_logit);
}

template <int ME>
__global__ __launch_bounds__(256) void k_weights_bwd(long long R, int S, const float* __restrict__ euclid,
                                                     const float* __restrict__ density,
                                                     const float* __restrict__ weights,
                                                     const float* __restrict__ d_w_in,    // [R,S]
                                                     const float* __restrict__ upstream,  // optional device scalar
                                                     float* __restrict__ d_density) {
  weights_bwd_body<false, false, false, false, false, ME>(R, S, euclid, density, weights, d_w_in, upstream, nullptr, nullptr,
                                                          nullptr, d_density, nullptr, nullptr, LossTargets{}, nullptr,
                                                          nullptr, 0);
}
// The six standalone compositing backward entry points: what a form does not read (logit without SEMGRAD, g_rgb / g_sem with
// TARGETS, tg without, bg without BG) is passed as nullptr / 0.
template <bool TARGETS, bool SEMGRAD, bool BG, bool SCALE, int ME>
__global__ __launch_bounds__(256) void k_composite_bwd(long long R, int S, const float* __restrict__ euclid,
                                                       const float* __restrict__ density,
                                                       const float* __restrict__ weights, const float* __restrict__ rgb,
                                                       const float* __restrict__ logit,     // SEMGRAD: samples [N]
                                                       const float* __restrict__ g_rgb,     // !TARGETS: [R,3]
                                                       const float* __restrict__ g_sem,     // !TARGETS: [R]
                                                       float* __restrict__ d_density, float* __restrict__ d_rgb,
                                                       float* __restrict__ d_logit, LossTargets tg,
                                                       const float* __restrict__ bg, int bg_stride) {
  weights_bwd_body<true, TARGETS, SEMGRAD, BG, SCALE, ME>(R, S, euclid, density, weights, nullptr, nullptr, rgb, g_rgb, g_sem,
                                                          d_density, d_rgb, d_logit, tg, logit, bg, bg_stride);
}

// k_composite_fwd (render.hip, training mode) followed by k_composite_bwd<true> for the same ray, in one wave: everything the
// backward read back from memory (weights, composited colour and logit) stays in registers.
template <bool SEMGRAD, bool BG, bool SCALE, int ME>
__global__ __launch_bounds__(256) void k_composite_fwd_bwd(long long R, int S, const float* __restrict__ euclid,
    const float* __restrict__ density, const float* __restrict__ rgb, const float* __restrict__ logit,
    const float* __restrict__ image, const float* __restrict__ mask, float sem_weight, float* __restrict__ weights,
    float* __restrict__ out_rgb, float* __restrict__ out_acc, float* __restrict__ out_depth, float* __restrict__ out_sem,
    long long* __restrict__ out_label, float* __restrict__ d_density, float* __restrict__ d_rgb, float* __restrict__ d_logit,
    const float* __restrict__ bg, int bg_stride) {
  static_assert(ME <= WB_MAXE, "the forward and the backward chunk a ray the same way");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * 4 + wave;
  if (r >= R) return;
  const int E = (S + 63) >> 6;
  const float* eb = euclid + r * (S + 1);
  const float* dn = density + r * S;
  const float* cs = rgb + r * S * 3;
  const float* lg = logit + r * S;
  // ---- forward: k_composite_fwd with training = 1 -----------------------------------------------------------------------
  float w[ME];
  float acc, cr, cg, cb, sm;
  int first;
  composite_fwd_ray<ME>(r, S, lane, eb, dn, cs, lg, 1, weights, w, acc, cr, cg, cb, sm, first);
  // (every lane: the backward wants the composited colour; wave_sum leaves the same total in all of them)
  const float* cl = BG ? bg + r * bg_stride : cs + 3 * (S - 1);
  const float l0 = cl[0], l1 = cl[1], l2 = cl[2];
  const float o0 = cr + l0 * (1.0f - acc), o1 = cg + l1 * (1.0f - acc), o2 = cb + l2 * (1.0f - acc);
  if (lane == 0) {
    out_rgb[3 * r] = o0;
    out_rgb[3 * r + 1] = o1;
    out_rgb[3 * r + 2] = o2;
    out_acc[r] = acc;
    out_sem[r] = sm;
    if (out_label) out_label[r] = (fsub(1.0f / (1.0f + expf(-sm)), 0.9f) > 0.0f) ? 1 : 0;
    out_depth[r] = fdiv(fadd(eb[first], eb[first + 1]), 2.0f);
  }
  // ---- backward: k_composite_bwd<true> -----------------------------------------------------------------------------------
  const float inv3r = 1.0f / (float)(3 * R), invr = 1.0f / (float)R;
  const float gr = mse_grad(o0 - image[3 * r], inv3r), gg = mse_grad(o1 - image[3 * r + 1], inv3r),
              gb = mse_grad(o2 - image[3 * r + 2], inv3r);
  const float gs = bce_logit_grad(sm, mask[r], sem_weight, invr);
  float delta[ME], gw[ME], wk[ME];
  float dd_local = 0.0f, gww_local = 0.0f, wsum_local = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    delta[e] = 0.0f;
    gw[e] = 0.0f;
    wk[e] = 0.0f;
    if (e < E && k < S) {
      delta[e] = eb[k + 1] - eb[k];
      wk[e] = w[e];
      const float* c = cs + 3 * k;
      gw[e] = gr * (c[0] - l0) + gg * (c[1] - l1) + gb * (c[2] - l2);  // semantic weights are detached unless SEMGRAD
      if constexpr (SEMGRAD) gw[e] += gs * lg[k];
      dd_local += delta[e] * dn[k];
      gww_local += gw[e] * wk[e];
      wsum_local += wk[e];
    }
  }
  weights_bwd_ray<true, BG, SCALE, ME>(r, S, lane, eb, dn, delta, gw, wk, dd_local, gww_local, wsum_local, gr, gg, gb, gs,
                                       d_density, d_rgb, d_logit);
}

// ---- the kernel of a call: every combination of the switches at every lane form ----------------------------------------------
// f(std::bool_constant...) with run-time switches as compile-time constants, as with_lane_elems does for ME
template <class F>
static inline void with_switches(F&& f) {
  f();
}
template <class F, class... Rest>
static inline void with_switches(F&& f, bool first, Rest... rest) {
  if (first) with_switches([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_switches([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
static auto composite_bwd_kernel(bool targets, bool semgrad, bool bg, bool scale, int S) {
  decltype(&k_composite_bwd<false, false, false, false, 1>) kernel = nullptr;
  with_switches(
      [&](auto t, auto sg, auto b, auto sc) {
        with_lane_elems(S, [&](auto me) {
          kernel = k_composite_bwd<decltype(t)::value, decltype(sg)::value, decltype(b)::value, decltype(sc)::value,
                                   decltype(me)::value>;
        });
      },
      targets, semgrad, bg, scale);
  return kernel;
}
static auto composite_fwd_bwd_kernel(bool semgrad, bool bg, bool scale, int S) {
  decltype(&k_composite_fwd_bwd<false, false, false, 1>) kernel = nullptr;
  with_switches(
      [&](auto sg, auto b, auto sc) {
        with_lane_elems(S, [&](auto me) {
          kernel = k_composite_fwd_bwd<decltype(sg)::value, decltype(b)::value, decltype(sc)::value, decltype(me)::value>;
        });
      },
      semgrad, bg, scale);
  return kernel;
}
static auto weights_bwd_kernel(int S) {
  decltype(&k_weights_bwd<1>) kernel = nullptr;
  with_lane_elems(S, [&](auto me) { kernel = k_weights_bwd<decltype(me)::value>; });
  return kernel;
}

// ---- the launch path of the ten entry points below ------------------------------------------------------------------------------
// `name`: the entry point's, which its error strings start with; `have_args`: every pointer it cannot do without is there;
// `op`: its FNR_PROF operation; `kernel`: its pick from the three families, for this S; `args`: what follows (R, S) in the
// kernel's parameter list.  One wave per ray, four rays per workgroup.
template <class... Params, class... Args>
static int launch_per_ray_bwd(const char* name, bool have_args, long long n_rays, int S, int op, void* stream,
                              void (*kernel)(long long, int, Params...), Args... args) {
  FNR_CHECK_ARG(have_args, "%s: null argument", name);
  FNR_CHECK_ARG(S > 0 && S <= 64 * WB_MAXE, "%s: S %d out of range", name, S);
  if (n_rays == 0) return FNR_OK;
  FNR_PROF(op, n_rays * (long long)S);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, as_stream(stream), n_rays, S,
                     static_cast<Params>(args)...);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}
// the six standalone compositing backward calls: given gradients (tg == nullptr) or targets, with the options `opt`
// (nullptr: last sample, no scaling, semantic weights as `semgrad` says)
static int launch_composite_bwd(const char* name, const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                const float* rgb, const float* logit, const float* weights, const float* g_rgb,
                                const float* g_semantics, const LossTargets* tg, bool semgrad,
                                const fnr_composite_options* opt, float* d_density, float* d_rgb, float* d_logit,
                                void* stream) {
  const bool bg = opt && opt->background == FNR_BACKGROUND_EXPLICIT, scale = opt && opt->gradient_scaling;
  const bool have_grads = tg ? tg->out_rgb && tg->image && tg->out_sem && tg->mask : g_rgb && g_semantics;
  return launch_per_ray_bwd(name,
                            rays && euclid_bins && density && rgb && (logit || !semgrad) && weights && have_grads &&
                                d_density && d_rgb && d_logit,
                            rays ? rays->n_rays : 0, S, OP_COMPOSITE_BWD, stream,
                            composite_bwd_kernel(tg != nullptr, semgrad, bg, scale, S), euclid_bins, density, weights, rgb,
                            logit, g_rgb, g_semantics, d_density, d_rgb, d_logit, tg ? *tg : LossTargets{},
                            bg ? opt->background_rgb : nullptr, bg ? (int)opt->background_stride : 0);
}
// the three fused forward + backward calls
static int launch_composite_fwd_bwd(const char* name, const fnr_rays* rays, int S, const float* euclid_bins,
                                    const float* density, const float* rgb, const float* logit, const float* image,
                                    const float* mask, float semantic_loss_weight, bool semgrad,
                                    const fnr_composite_options* opt, float* weights, float* out_rgb,
                                    float* out_accumulation, float* out_depth, float* out_semantics, int64_t* out_label,
                                    float* d_density, float* d_rgb, float* d_logit, void* stream) {
  const bool bg = opt && opt->background == FNR_BACKGROUND_EXPLICIT, scale = opt && opt->gradient_scaling;
  return launch_per_ray_bwd(name,
                            rays && euclid_bins && density && rgb && logit && image && mask && weights && out_rgb &&
                                out_accumulation && out_depth && out_semantics && d_density && d_rgb && d_logit,
                            rays ? rays->n_rays : 0, S, OP_COMPOSITE_FWD, stream,
                            composite_fwd_bwd_kernel(semgrad, bg, scale, S), euclid_bins, density, rgb, logit, image, mask,
                            semantic_loss_weight, weights, out_rgb, out_accumulation, out_depth, out_semantics,
                            reinterpret_cast<long long*>(out_label), d_density, d_rgb, d_logit,
                            bg ? opt->background_rgb : nullptr, bg ? (int)opt->background_stride : 0);
}

}  // namespace fnr

using namespace fnr;

extern "C" int fnr_composite_bwd(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                 const float* rgb, const float* weights, const float* g_rgb, const float* g_semantics,
                                 float* d_density, float* d_rgb, float* d_logit, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_composite_bwd");
  return launch_composite_bwd("composite_bwd", rays, S, euclid_bins, density, rgb, nullptr, weights, g_rgb, g_semantics,
                              nullptr, false, nullptr, d_density, d_rgb, d_logit, stream);
}

extern "C" int fnr_composite_bwd_targets(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                         const float* rgb, const float* weights, const float* out_rgb, const float* image,
                                         const float* out_semantics, const float* mask, float semantic_loss_weight,
                                         float* d_density, float* d_rgb, float* d_logit, void* stream) {
  FNR_SEQ_RECORD(fnr_composite_bwd_targets, rays, S, euclid_bins, density, rgb, weights, out_rgb, image, out_semantics, mask,
                 semantic_loss_weight, d_density, d_rgb, d_logit, stream);
  const LossTargets tg{out_rgb, image, out_semantics, mask, semantic_loss_weight};
  return launch_composite_bwd("composite_bwd_targets", rays, S, euclid_bins, density, rgb, nullptr, weights, nullptr, nullptr,
                              &tg, false, nullptr, d_density, d_rgb, d_logit, stream);
}

// fnr_composite_fwd (training) and fnr_composite_bwd_targets as ONE launch (ABI 13): a wave composites its ray and, with the
// outputs still in registers, forms the per-ray loss gradients and runs the backward — the same operations on the same values in
// the same order as the two kernels (tests/test_gpu_training_parity.py: bit-identical), one launch ramp less on the chain
// forward -> MLP backward of every training step.
extern "C" int fnr_composite_fwd_bwd_targets(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                             const float* rgb, const float* logit, const float* image, const float* mask,
                                             float semantic_loss_weight, float* weights, float* out_rgb,
                                             float* out_accumulation, float* out_depth, float* out_semantics,
                                             int64_t* out_label, float* d_density, float* d_rgb, float* d_logit,
                                             void* stream) {
  FNR_SEQ_RECORD(fnr_composite_fwd_bwd_targets, rays, S, euclid_bins, density, rgb, logit, image, mask, semantic_loss_weight,
                 weights, out_rgb, out_accumulation, out_depth, out_semantics, out_label, d_density, d_rgb, d_logit, stream);
  return launch_composite_fwd_bwd("composite_fwd_bwd_targets", rays, S, euclid_bins, density, rgb, logit, image, mask,
                                  semantic_loss_weight, false, nullptr, weights, out_rgb, out_accumulation, out_depth,
                                  out_semantics, out_label, d_density, d_rgb, d_logit, stream);
}

// ---- pass_semantic_gradients (fruit_nerf.py:56, 344-345): the three compositing backward calls with the semantic renderer's
// weights NOT detached — d_density also carries g_sem * logit_k; d_rgb and d_logit are the parents' bit for bit.
extern "C" int fnr_composite_bwd_semgrad(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                         const float* rgb, const float* logit, const float* weights, const float* g_rgb,
                                         const float* g_semantics, float* d_density, float* d_rgb, float* d_logit,
                                         void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_composite_bwd_semgrad");
  return launch_composite_bwd("composite_bwd_semgrad", rays, S, euclid_bins, density, rgb, logit, weights, g_rgb, g_semantics,
                              nullptr, true, nullptr, d_density, d_rgb, d_logit, stream);
}

extern "C" int fnr_composite_bwd_targets_semgrad(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                                 const float* rgb, const float* logit, const float* weights,
                                                 const float* out_rgb, const float* image, const float* out_semantics,
                                                 const float* mask, float semantic_loss_weight, float* d_density,
                                                 float* d_rgb, float* d_logit, void* stream) {
  FNR_SEQ_RECORD(fnr_composite_bwd_targets_semgrad, rays, S, euclid_bins, density, rgb, logit, weights, out_rgb, image,
                 out_semantics, mask, semantic_loss_weight, d_density, d_rgb, d_logit, stream);
  const LossTargets tg{out_rgb, image, out_semantics, mask, semantic_loss_weight};
  return launch_composite_bwd("composite_bwd_targets_semgrad", rays, S, euclid_bins, density, rgb, logit, weights, nullptr,
                              nullptr, &tg, true, nullptr, d_density, d_rgb, d_logit, stream);
}

extern "C" int fnr_composite_fwd_bwd_targets_semgrad(const fnr_rays* rays, int S, const float* euclid_bins,
                                                     const float* density, const float* rgb, const float* logit,
                                                     const float* image, const float* mask, float semantic_loss_weight,
                                                     float* weights, float* out_rgb, float* out_accumulation,
                                                     float* out_depth, float* out_semantics, int64_t* out_label,
                                                     float* d_density, float* d_rgb, float* d_logit, void* stream) {
  FNR_SEQ_RECORD(fnr_composite_fwd_bwd_targets_semgrad, rays, S, euclid_bins, density, rgb, logit, image, mask,
                 semantic_loss_weight, weights, out_rgb, out_accumulation, out_depth, out_semantics, out_label, d_density, d_rgb,
                 d_logit, stream);
  return launch_composite_fwd_bwd("composite_fwd_bwd_targets_semgrad", rays, S, euclid_bins, density, rgb, logit, image, mask,
                                  semantic_loss_weight, true, nullptr, weights, out_rgb, out_accumulation, out_depth,
                                  out_semantics, out_label, d_density, d_rgb, d_logit, stream);
}

// ---- background_color / use_gradient_scaling (fnr_composite_options): the compositing backward calls once more, the options
// in one struct.  {last sample, no scaling} is the entry point above (its launch, its name in a step program), with the
// semantic weights detached or attached; the other six combinations of {semantic weights attached, explicit background,
// scaling} are further instantiations of the same kernels.
extern "C" int fnr_composite_bwd_opt(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                     const float* rgb, const float* logit, const float* weights, const float* g_rgb,
                                     const float* g_semantics, const fnr_composite_options* opt, float* d_density,
                                     float* d_rgb, float* d_logit, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_composite_bwd_opt");
  FNR_CHECK_COMPOSITE_OPTIONS("composite_bwd_opt", opt);
  if (composite_options_plain(opt))
    return opt->semantic_gradients ? fnr_composite_bwd_semgrad(rays, S, euclid_bins, density, rgb, logit, weights, g_rgb,
                                                               g_semantics, d_density, d_rgb, d_logit, stream)
                                   : fnr_composite_bwd(rays, S, euclid_bins, density, rgb, weights, g_rgb, g_semantics,
                                                       d_density, d_rgb, d_logit, stream);
  return launch_composite_bwd("composite_bwd_opt", rays, S, euclid_bins, density, rgb, logit, weights, g_rgb, g_semantics,
                              nullptr, opt->semantic_gradients, opt, d_density, d_rgb, d_logit, stream);
}

extern "C" int fnr_composite_bwd_targets_opt(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                             const float* rgb, const float* logit, const float* weights,
                                             const float* out_rgb, const float* image, const float* out_semantics,
                                             const float* mask, float semantic_loss_weight,
                                             const fnr_composite_options* opt, float* d_density, float* d_rgb,
                                             float* d_logit, void* stream) {
  if (opt && composite_options_ok(opt) && composite_options_plain(opt))
    return opt->semantic_gradients
               ? fnr_composite_bwd_targets_semgrad(rays, S, euclid_bins, density, rgb, logit, weights, out_rgb, image,
                                                   out_semantics, mask, semantic_loss_weight, d_density, d_rgb, d_logit, stream)
               : fnr_composite_bwd_targets(rays, S, euclid_bins, density, rgb, weights, out_rgb, image, out_semantics, mask,
                                           semantic_loss_weight, d_density, d_rgb, d_logit, stream);
  FNR_SEQ_RECORD(fnr_composite_bwd_targets_opt, rays, S, euclid_bins, density, rgb, logit, weights, out_rgb, image,
                 out_semantics, mask, semantic_loss_weight, opt, d_density, d_rgb, d_logit, stream);
  FNR_CHECK_COMPOSITE_OPTIONS("composite_bwd_targets_opt", opt);
  const LossTargets tg{out_rgb, image, out_semantics, mask, semantic_loss_weight};
  return launch_composite_bwd("composite_bwd_targets_opt", rays, S, euclid_bins, density, rgb, logit, weights, nullptr, nullptr,
                              &tg, opt->semantic_gradients, opt, d_density, d_rgb, d_logit, stream);
}

extern "C" int fnr_composite_fwd_bwd_targets_opt(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                                 const float* rgb, const float* logit, const float* image, const float* mask,
                                                 float semantic_loss_weight, const fnr_composite_options* opt,
                                                 float* weights, float* out_rgb, float* out_accumulation, float* out_depth,
                                                 float* out_semantics, int64_t* out_label, float* d_density, float* d_rgb,
                                                 float* d_logit, void* stream) {
  if (opt && composite_options_ok(opt) && composite_options_plain(opt))
    return (opt->semantic_gradients ? fnr_composite_fwd_bwd_targets_semgrad : fnr_composite_fwd_bwd_targets)(
        rays, S, euclid_bins, density, rgb, logit, image, mask, semantic_loss_weight, weights, out_rgb, out_accumulation,
        out_depth, out_semantics, out_label, d_density, d_rgb, d_logit, stream);
  FNR_SEQ_RECORD(fnr_composite_fwd_bwd_targets_opt, rays, S, euclid_bins, density, rgb, logit, image, mask,
                 semantic_loss_weight, opt, weights, out_rgb, out_accumulation, out_depth, out_semantics, out_label, d_density,
                 d_rgb, d_logit, stream);
  FNR_CHECK_COMPOSITE_OPTIONS("composite_fwd_bwd_targets_opt", opt);
  return launch_composite_fwd_bwd("composite_fwd_bwd_targets_opt", rays, S, euclid_bins, density, rgb, logit, image, mask,
                                  semantic_loss_weight, opt->semantic_gradients, opt, weights, out_rgb, out_accumulation,
                                  out_depth, out_semantics, out_label, d_density, d_rgb, d_logit, stream);
}

extern "C" int fnr_weights_bwd(int64_t n_rays, int S, const float* euclid_bins, const float* density,
                               const float* weights, const float* d_weights, const float* upstream,
                               float* d_density, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_weights_bwd");
  return launch_per_ray_bwd("weights_bwd", euclid_bins && density && weights && d_weights && d_density, n_rays, S,
                            OP_WEIGHTS_BWD, stream, weights_bwd_kernel(S), euclid_bins, density, weights, d_weights, upstream,
                            d_density);
}
