// adam.hpp — torch.optim.Adam / RAdam, written once: the per-element rule (table_adam_update), the step-dependent scalars
// (adam_step_scalars) and the descriptors of the kernels that take the step where a gradient is finished.  The whole-buffer
// and spans sweeps (optim.hip) run the same two functions, so fused and unfused paths cannot drift apart.
#pragma once
#include <math.h>

#include "common.hpp"

namespace fnr {

// What a step count contributes to the rule, derived in double and rounded to float once each: bias_correction1,
// sqrt(bias_correction2), and RAdam's rectification term — `rect` < 0 encodes "not rectified" (rho_t <= 5, plain momentum;
// always for Adam).  The one place these are derived: on the host for the entry points that are handed a step count, on the
// device for fnr_adam_step_spans_dev's counters.
struct AdamStepScalars {
  float bc1, bc2_sqrt, rect;
};
__host__ __device__ inline AdamStepScalars adam_step_scalars(float beta1, float beta2, long long step, bool radam) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double b2t = pow((double)beta2, (double)step);
  const double bc2 = 1.0 - b2t;
  double rect = -1.0;  // not rectified
  if (radam) {
    const double rho_inf = 2.0 / (1.0 - (double)beta2) - 1.0;
    const double rho_t = rho_inf - 2.0 * (double)step * b2t / bc2;
    if (rho_t > 5.0)
      rect = sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t));
  }
  return {(float)bc1, (float)sqrt(bc2), (float)rect};
}

// Optimiser step fused into the kernel that produces a gradient (single-process training).  Hash table: the accumulate
// workgroup that owns a bin has the bin's summed gradient in LDS, so it applies torch.optim.Adam / RAdam to those rows
// right there (hash_scatter.hip); camera poses: the workgroup of a camera finishes its 6 gradients (camera_opt.hip).  The gradient table
// is then neither read-modify-written here nor read and zeroed by the optimiser pass: 40 -> 24 bytes of HBM traffic
// per table parameter and step.  table_adam_update is the rule itself — torch's operations in torch's order — and the only
// place it is written: the sweeps of optim.hip (k_adam_sweep) call it per element too, hence bit-identical parameters and moments.
struct TableAdam {
  float2 *p, *m, *v;  // the table's slices of the parameter / exp_avg / exp_avg_sq arenas, [L << log2_T] rows
  float lr, b1, b2, eps, bc1, bc2_sqrt, rect, grad_scale, weight_decay;
  int radam;
  unsigned* touched;  // one bit per pair of rows: ever received a gradient (nullable; fnr_table_adam.touched)
};
__device__ __forceinline__ void table_adam_update(const TableAdam& a, float g, float& P, float& M, float& V) {
  float gr = g * a.grad_scale;
  if (a.weight_decay != 0.0f) gr = gr + a.weight_decay * P;   // grad.add(param, alpha=weight_decay)
  M = M + (gr - M) * (1.0f - a.b1);                           // exp_avg.lerp_(grad, 1 - beta1)
  V = V * a.b2 + (1.0f - a.b2) * gr * gr;                     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  if (!a.radam) {
    const float step_size = a.lr / a.bc1;
    const float denom = sqrtf(V) / a.bc2_sqrt + a.eps;        // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    P = P - step_size * (M / denom);                          // param.addcdiv_(exp_avg, denom, value=-step_size)
  } else {
    const float mhat = M / a.bc1;                             // bias_corrected_exp_avg
    if (a.rect >= 0.0f) {
      const float adaptive = a.bc2_sqrt / (sqrtf(V) + a.eps); // sqrt(bias_correction2) / (exp_avg_sq.sqrt() + eps)
      P = P - a.lr * (mhat * a.rect * adaptive);
    } else {
      P = P - a.lr * mhat;
    }
  }
}
// The optimiser step of a parameter taken by the thread that finishes its gradient entry (both roles of k_finish_weights in
// field_mlp_bwd.hip, k_prop_reduce in prop_bwd.hip: single writers): the parameter / moment arrays parallel the gradient arena.
struct WeightAdam {
  TableAdam t;               // hyper-parameters and step-dependent scalars (its p / m / v pointers are unused here)
  long long p_off, m_off, v_off;   // element offsets from a GRADIENT address to the parameter / exp_avg / exp_avg_sq entry
};
__device__ __forceinline__ void weight_adam_entry(const WeightAdam& wa, float* __restrict__ g_entry, float s) {
  const float g = *g_entry + s;
  float P = g_entry[wa.p_off], M = g_entry[wa.m_off], V = g_entry[wa.v_off];
  table_adam_update(wa.t, g, P, M, V);
  g_entry[wa.p_off] = P;
  g_entry[wa.m_off] = M;
  g_entry[wa.v_off] = V;
  *g_entry = 0.0f;
}
// host side of TableAdam
static inline int make_table_adam(const fnr_table_adam* a, TableAdam& t) {
  FNR_CHECK_ARG(a && a->params && a->exp_avg && a->exp_avg_sq, "table adam: null argument");
  FNR_CHECK_ARG(a->algorithm == 0 || a->algorithm == 1, "table adam: algorithm %d (0 = Adam, 1 = RAdam)", a->algorithm);
  FNR_CHECK_ARG(a->step >= 1, "table adam: step must be >= 1");
  t.p = reinterpret_cast<float2*>(a->params);
  t.m = reinterpret_cast<float2*>(a->exp_avg);
  t.v = reinterpret_cast<float2*>(a->exp_avg_sq);
  t.lr = a->lr, t.b1 = a->beta1, t.b2 = a->beta2, t.eps = a->eps, t.grad_scale = a->grad_scale, t.weight_decay = a->weight_decay;
  t.radam = a->algorithm;
  t.touched = a->touched;
  FNR_CHECK_ARG(!a->touched || a->weight_decay == 0.0f, "table adam: sparse-touch skipping needs weight_decay = 0");
  const AdamStepScalars s = adam_step_scalars(a->beta1, a->beta2, a->step, a->algorithm == 1);
  t.bc1 = s.bc1, t.bc2_sqrt = s.bc2_sqrt, t.rect = s.rect;
  return FNR_OK;
}

}  // namespace fnr
