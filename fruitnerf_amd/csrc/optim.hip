// optim.hip — the optimiser's sweeps for gfx950: torch.optim.Adam (incl. its L2 weight_decay, no amsgrad) and
// torch.optim.RAdam (fruit_nerf_big / fruit_nerf_huge use it for every group, fruit_nerf_config.py:97-106,148-160) over
// flat arenas.  One kernel, k_adam_sweep, behind four entry points:
//   fnr_adam_step / fnr_radam_step   one buffer, one step count: the one-span case of
//   fnr_adam_step_spans              several spans of one arena in one launch, each with its own learning rate and step
//   fnr_adam_step_spans_dev          the same with the step counters, the loss scale and the "found inf" flag in device memory
// The rule per element (table_adam_update) and the step-dependent scalars (adam_step_scalars) are adam.hpp's, shared with
// the kernels that take the step where they finish a gradient: bit-identical parameters and moments on every path.
#include "adam.hpp"
#include "sequencer.hpp"

namespace fnr {

// The spans of one sweep: their float4 chunks are numbered consecutively, a thread finds its span by scanning the (<= 8)
// cumulative counts.  Unused spans are empty.  bc1 / bc2_sqrt / rect are filled where the host knows the step counts.
struct AdamSpans {
  int n;
  long long cum4[FNR_MAX_ADAM_SPANS + 1];  // chunk index at which span k starts; cum4[n] = total
  long long off4[FNR_MAX_ADAM_SPANS];      // first float4 of span k in the arena
  float lr[FNR_MAX_ADAM_SPANS], bc1[FNR_MAX_ADAM_SPANS], bc2_sqrt[FNR_MAX_ADAM_SPANS], rect[FNR_MAX_ADAM_SPANS];
};

// ---------------------------------------------------------------------------------------------------
// fnr_adam_step_spans_dev: the spans step with everything a torch.amp.GradScaler decides per step — the loss scale, the
// "found inf" flag — and the spans' step counters in DEVICE memory, so that the call needs no host round trip.
//
// Two launches on the caller's stream, the first of the two choices that keep the counters free of races:
//   1. k_adam_dev_prologue, ONE workgroup, thread k < n owns span k: reads *found_inf, *grad_scale and steps[k]; unless
//      the step is skipped it bumps steps[k] and derives the span's step-dependent scalars from the post-increment count
//      (adam_step_scalars, on the device); writes them to the caller's scalar block.
//   2. k_adam_sweep<., true>: reads the scalar block only (never a counter).  A skipped step touches neither parameters
//      nor moments; with zero_grad it still zeroes the gradient spans, so that an inf / NaN does not leak into the next
//      backward's accumulation.
// No workgroup reads a counter that another workgroup of the same launch writes: the prologue is one workgroup whose
// threads own one counter each, the sweep reads what the (stream-ordered) prologue left in the block.
// ---------------------------------------------------------------------------------------------------
struct AdamDevScalars {   // the caller's scalar block (FNR_ADAM_DEV_SCALAR_FLOATS floats)
  float skip, inv_scale;
  float bc1[FNR_MAX_ADAM_SPANS], bc2_sqrt[FNR_MAX_ADAM_SPANS], rect[FNR_MAX_ADAM_SPANS];
};
static_assert(sizeof(AdamDevScalars) <= FNR_ADAM_DEV_SCALAR_FLOATS * sizeof(float), "scalar block too small");

__global__ __launch_bounds__(64) void k_adam_dev_prologue(int n, int radam, float b1, float b2,
                                                          const float* __restrict__ grad_scale,
                                                          const float* __restrict__ found_inf,
                                                          long long* __restrict__ steps,
                                                          AdamDevScalars* __restrict__ out) {
  const int k = threadIdx.x;
  const bool skip = found_inf != nullptr && *found_inf != 0.0f;
  if (k == 0) {
    out->skip = skip ? 1.0f : 0.0f;
    // GradScaler.unscale_: scale.double().reciprocal().float()
    out->inv_scale = grad_scale != nullptr ? (float)(1.0 / (double)*grad_scale) : 1.0f;
  }
  if (k >= n || skip) return;
  const long long step = steps[k] + 1;
  steps[k] = step;
  const AdamStepScalars s = adam_step_scalars(b1, b2, step, radam != 0);
  out->bc1[k] = s.bc1;
  out->bc2_sqrt[k] = s.bc2_sqrt;
  out->rect[k] = s.rect;
}

// The sweep.  DEV_SCALARS: the step-dependent scalars, the gradient scale and the skip flag come from the prologue's block
// `sc` (else from `sp` and the arguments; `sc` is not read).  ONE_SPAN: sp.n == 1, no thread looks its span up — the whole-
// buffer steps measured 1 - 2 us of 78 slower through the look-up (profiles/optimizer_sweeps.md).
template <bool RADAM, bool DEV_SCALARS, bool ONE_SPAN>
__global__ __launch_bounds__(256) void k_adam_sweep(float4* __restrict__ p, float4* __restrict__ g,
                                                    float4* __restrict__ m, float4* __restrict__ v, AdamSpans sp,
                                                    const AdamDevScalars* __restrict__ sc, float b1, float b2, float eps,
                                                    float grad_scale, float weight_decay, int zero_grad) {
  const long long total = sp.cum4[sp.n];
  bool skip = false;
  if constexpr (DEV_SCALARS) {
    skip = sc->skip != 0.0f;
    if (skip && !zero_grad) return;
    grad_scale = sc->inv_scale;
  }
  TableAdam a{};   // (its pointers are unused here)
  a.b1 = b1, a.b2 = b2, a.eps = eps, a.grad_scale = grad_scale, a.weight_decay = weight_decay, a.radam = RADAM;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < total; c += (long long)gridDim.x * 256) {
    int k = 0;
    if constexpr (!ONE_SPAN) {
#pragma unroll
      for (int q = 1; q < FNR_MAX_ADAM_SPANS; ++q)
        if (q < sp.n && c >= sp.cum4[q]) k = q;
    }
    const long long i = sp.off4[k] + (c - sp.cum4[k]);
    if (skip) {   // the step is not taken; its (non-finite) gradient must not reach the next backward
      ntc_store<NT_MOMENT_ST>(&g[i], make_float4(0.f, 0.f, 0.f, 0.f));
      continue;
    }
    a.lr = sp.lr[k];
    if constexpr (DEV_SCALARS)
      a.bc1 = sc->bc1[k], a.bc2_sqrt = sc->bc2_sqrt[k], a.rect = sc->rect[k];
    else
      a.bc1 = sp.bc1[k], a.bc2_sqrt = sp.bc2_sqrt[k], a.rect = sp.rect[k];
    // moments and gradient: read once, written once per step — streaming, so that the sweep (the exchange path's 88 us over the
    // main table) leaves the table's parameters in the caches for the next encode
    float4 P = p[i], G = ntc_load<NT_MOMENT_LD>(&g[i]), M = ntc_load<NT_MOMENT_LD>(&m[i]), V = ntc_load<NT_MOMENT_LD>(&v[i]);
    table_adam_update(a, G.x, P.x, M.x, V.x);
    table_adam_update(a, G.y, P.y, M.y, V.y);
    table_adam_update(a, G.z, P.z, M.z, V.z);
    table_adam_update(a, G.w, P.w, M.w, V.w);
    p[i] = P;
    ntc_store<NT_MOMENT_ST>(&m[i], M);
    ntc_store<NT_MOMENT_ST>(&v[i], V);
    if (zero_grad) ntc_store<NT_MOMENT_ST>(&g[i], make_float4(0.f, 0.f, 0.f, 0.f));
  }
}

// The layout of a sweep from the caller's spans, for `who` (the prefix of its messages).  host_steps: the spans carry their
// step counts (>= 1), and the step-dependent scalars are derived here.
static int make_adam_spans(const char* who, int n_spans, const fnr_adam_span* spans, bool host_steps, int algorithm,
                           float beta1, float beta2, AdamSpans& sp) {
  FNR_CHECK_ARG(n_spans >= 1 && n_spans <= FNR_MAX_ADAM_SPANS, "%s: %d spans (1..%d)", who, n_spans, FNR_MAX_ADAM_SPANS);
  FNR_CHECK_ARG(algorithm == 0 || algorithm == 1, "%s: algorithm %d (0 = Adam, 1 = RAdam)", who, algorithm);
  sp.n = n_spans;
  sp.cum4[0] = 0;
  for (int k = 0; k < FNR_MAX_ADAM_SPANS; ++k) {
    sp.lr[k] = 0.0f, sp.bc1[k] = 1.0f, sp.bc2_sqrt[k] = 1.0f, sp.rect[k] = -1.0f;
    if (k >= n_spans) {
      sp.cum4[k + 1] = sp.cum4[k];
      sp.off4[k] = 0;
      continue;
    }
    const fnr_adam_span& s = spans[k];
    const bool aligned = s.offset >= 0 && s.count >= 0 && s.offset % 4 == 0 && s.count % 4 == 0;
    if (host_steps)
      FNR_CHECK_ARG(aligned && s.step >= 1, "%s: span %d: offset / count must be multiples of 4, step >= 1", who, k);
    else
      FNR_CHECK_ARG(aligned, "%s: span %d: offset / count must be multiples of 4", who, k);
    sp.off4[k] = s.offset / 4;
    sp.cum4[k + 1] = sp.cum4[k] + s.count / 4;
    sp.lr[k] = s.lr;
    if (host_steps) {
      const AdamStepScalars t = adam_step_scalars(beta1, beta2, s.step, algorithm == 1);
      sp.bc1[k] = t.bc1, sp.bc2_sqrt[k] = t.bc2_sqrt, sp.rect[k] = t.rect;
    }
  }
  return FNR_OK;
}

// min(ceil(total4 / 256), 8192) workgroups of 256; sc: the prologue's block, or null for the scalars in `sp`
static int launch_adam_sweep(bool radam, float* params, float* grads, float* exp_avg, float* exp_avg_sq, const AdamSpans& sp,
                             const AdamDevScalars* sc, float beta1, float beta2, float eps, float grad_scale,
                             float weight_decay, int zero_grad, void* stream) {
  long long blocks = (sp.cum4[sp.n] + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  static constexpr decltype(&k_adam_sweep<false, false, false>) kernels[2][2][2] = {   // [radam][device scalars][one span]
      {{k_adam_sweep<false, false, false>, k_adam_sweep<false, false, true>},
       {k_adam_sweep<false, true, false>, k_adam_sweep<false, true, true>}},
      {{k_adam_sweep<true, false, false>, k_adam_sweep<true, false, true>},
       {k_adam_sweep<true, true, false>, k_adam_sweep<true, true, true>}}};
  hipLaunchKernelGGL(kernels[radam][sc != nullptr][sp.n == 1], dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<float4*>(params), reinterpret_cast<float4*>(grads), reinterpret_cast<float4*>(exp_avg),
                     reinterpret_cast<float4*>(exp_avg_sq), sp, sc, beta1, beta2, eps, grad_scale, weight_decay, zero_grad);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

// fnr_adam_step / fnr_radam_step after their argument checks: the one-span case {offset 0, count n, step, lr}
static int adam_step_one_span(const char* who, bool radam, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                              int64_t n, float lr, float beta1, float beta2, float eps, int64_t step, float grad_scale,
                              float weight_decay, int zero_grad, void* stream) {
  const fnr_adam_span span{0, n, step, lr, 0};
  AdamSpans sp;
  const int rc = make_adam_spans(who, 1, &span, true, radam ? 1 : 0, beta1, beta2, sp);
  if (rc != FNR_OK) return rc;
  FNR_PROF(OP_ADAM, n);
  return launch_adam_sweep(radam, params, grads, exp_avg, exp_avg_sq, sp, nullptr, beta1, beta2, eps, grad_scale,
                           weight_decay, zero_grad, stream);
}

}  // namespace fnr

using namespace fnr;

extern "C" int fnr_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                             float beta1, float beta2, float eps, int64_t step, float grad_scale, float weight_decay,
                             int zero_grad, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_adam_step");
  FNR_CHECK_ARG(params && grads && exp_avg && exp_avg_sq, "adam_step: null argument");
  FNR_CHECK_ARG(n % 4 == 0 && step >= 1, "adam_step: n must be a multiple of 4 (arena is padded) and step >= 1");
  if (n == 0) return FNR_OK;
  return adam_step_one_span("adam_step", false, params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step,
                            grad_scale, weight_decay, zero_grad, stream);
}

extern "C" int fnr_radam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                              float beta1, float beta2, float eps, int64_t step, float grad_scale, float weight_decay,
                              int zero_grad, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_radam_step");
  FNR_CHECK_ARG(params && grads && exp_avg && exp_avg_sq, "radam_step: null argument");
  FNR_CHECK_ARG(n % 4 == 0 && step >= 1, "radam_step: n must be a multiple of 4 (arena is padded) and step >= 1");
  if (n == 0) return FNR_OK;
  return adam_step_one_span("radam_step", true, params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step,
                            grad_scale, weight_decay, zero_grad, stream);
}

extern "C" int fnr_adam_step_spans(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int n_spans,
                                   const fnr_adam_span* spans, int algorithm, float beta1, float beta2, float eps,
                                   float grad_scale, float weight_decay, int zero_grad, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_adam_step_spans");
  FNR_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && spans, "adam_step_spans: null argument");
  AdamSpans sp;
  const int rc = make_adam_spans("adam_step_spans", n_spans, spans, true, algorithm, beta1, beta2, sp);
  if (rc != FNR_OK) return rc;
  if (sp.cum4[n_spans] == 0) return FNR_OK;
  FNR_PROF(OP_ADAM, 4 * sp.cum4[n_spans]);
  return launch_adam_sweep(algorithm == 1, params, grads, exp_avg, exp_avg_sq, sp, nullptr, beta1, beta2, eps, grad_scale,
                           weight_decay, zero_grad, stream);
}

extern "C" int fnr_adam_step_spans_dev(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int n_spans,
                                       const fnr_adam_span* spans, int64_t* steps, int algorithm, float beta1,
                                       float beta2, float eps, const float* grad_scale, const float* found_inf,
                                       float weight_decay, int zero_grad, float* scalars, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_adam_step_spans_dev");
  FNR_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && spans && steps && scalars,
                "adam_step_spans_dev: null argument");
  AdamSpans sp;
  const int rc = make_adam_spans("adam_step_spans_dev", n_spans, spans, false, algorithm, beta1, beta2, sp);
  if (rc != FNR_OK) return rc;
  FNR_PROF(OP_ADAM, 4 * sp.cum4[n_spans]);
  AdamDevScalars* sc = reinterpret_cast<AdamDevScalars*>(scalars);
  // the counters advance even over empty spans: they count optimiser steps, not elements
  hipLaunchKernelGGL(k_adam_dev_prologue, dim3(1), dim3(64), 0, as_stream(stream), n_spans, algorithm, beta1, beta2,
                     grad_scale, found_inf, reinterpret_cast<long long*>(steps), sc);
  FNR_LAUNCH_CHECK();
  if (sp.cum4[n_spans] == 0) return FNR_OK;
  return launch_adam_sweep(algorithm == 1, params, grads, exp_avg, exp_avg_sq, sp, sc, beta1, beta2, eps, 1.0f, weight_decay,
                           zero_grad, stream);
}
