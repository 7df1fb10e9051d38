// field_normals.hip — analytic normals of FruitField: nerfstudio's Field.get_normals (-normalize(d density logit / d sample
// location), the reason fruit_field.py:180-186 stores _sample_locations / _density_before_activation) and NormalsRenderer /
// NormalsShader over the compositing weights.  Inference side only: nothing here runs inside a training step.
//
// k_field_normals, one sample per lane.  The density logit is h0 = W_b1[0, :] relu(W_b0 x + b_b0) + b_b1[0], so
//   d h0 / d x = W_b0^T (1[a1 > 0] * W_b1[0, :])                                              [32]
//   g = (d x / d position)^T (d h0 / d x) = the contraction with the Jacobian fnr_hash_encode_fwd saved [3]
// in float32 fmaf chains whatever fnr_field_net.mlp_mode says (a1: bias first, then k = 0..31; d h0 / d x: hidden unit 0..63;
// g: level-major, feature 0 then 1).  The 8 KB of W_b0, b_b0 and the density row of W_b1 are the same addresses for every
// lane: the compiler reads them through the scalar cache and feeds them to the fmas as scalar operands, so no LDS and no
// barrier.  HBM traffic per sample: 128 B features + 1 B selector + 384 B Jacobian (float2 per lane, consecutive lanes =
// consecutive samples) in, 12 B (24 B with `gradient`) out.  Plain loads and stores: the Jacobian is read exactly once, but
// the launch is alone on the device.
#include "common.hpp"
#include "sequencer.hpp"

namespace fnr {

constexpr int FN_BLOCK = 256;
constexpr int FN_IN = 32, FN_HID = 64, FN_LEVELS = 16;

__global__ __launch_bounds__(FN_BLOCK) void k_field_normals(long long N, const float* __restrict__ w0,
                                                            const float* __restrict__ b0, const float* __restrict__ w1,
                                                            const float2* __restrict__ feats,
                                                            const float2* __restrict__ jac,
                                                            const uint8_t* __restrict__ selector,
                                                            float* __restrict__ normals, float* __restrict__ gradient) {
  const long long n = (long long)blockIdx.x * FN_BLOCK + threadIdx.x;
  const bool live = n < N;
  const long long m = live ? n : N - 1;   // lanes past the end redo the last sample and store nothing
  float x[FN_IN];
#pragma unroll
  for (int l = 0; l < FN_LEVELS; ++l) {
    const float2 f = feats[(size_t)l * N + m];
    x[2 * l] = f.x;
    x[2 * l + 1] = f.y;
  }
  float df[FN_IN];
#pragma unroll
  for (int k = 0; k < FN_IN; ++k) df[k] = 0.0f;
  // one hidden unit per trip: unrolled by 2 or 4 the 64 + 64 weights in flight spill scalar registers (profiles/field_normals.md)
#pragma unroll 1
  for (int h = 0; h < FN_HID; ++h) {
    const float* __restrict__ w = w0 + h * FN_IN;
    float a = b0[h];
#pragma unroll
    for (int k = 0; k < FN_IN; ++k) a = fmaf(w[k], x[k], a);
    const float v = a > 0.0f ? w1[h] : 0.0f;
#pragma unroll
    for (int k = 0; k < FN_IN; ++k) df[k] = fmaf(v, w[k], df[k]);
  }
  float g[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int l = 0; l < FN_LEVELS; ++l) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float2 j = jac[((size_t)l * 3 + a) * N + m];
      g[a] = fmaf(j.x, df[2 * l], g[a]);
      g[a] = fmaf(j.y, df[2 * l + 1], g[a]);
    }
  }
  if (!live) return;
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (selector[n]) {
    // -F.normalize(g, dim=-1): g / max(||g||, 1e-12)
    const float norm = sqrtf(fadd(fadd(fmul(g[0], g[0]), fmul(g[1], g[1])), fmul(g[2], g[2])));
    const float d = fmaxf(norm, 1e-12f);
    nx = -fdiv(g[0], d), ny = -fdiv(g[1], d), nz = -fdiv(g[2], d);
  } else {
    g[0] = g[1] = g[2] = 0.0f;   // the masked position is the constant 0: no gradient reaches it
  }
  normals[3 * n] = nx;
  normals[3 * n + 1] = ny;
  normals[3 * n + 2] = nz;
  if (gradient) {
    gradient[3 * n] = g[0];
    gradient[3 * n + 1] = g[1];
    gradient[3 * n + 2] = g[2];
  }
}

// one thread per ray: the S terms are added one after the other, sample 0 first
__global__ __launch_bounds__(FN_BLOCK) void k_render_normals(long long R, int S, const float* __restrict__ weights,
                                                             const float* __restrict__ normals, int shade,
                                                             float* __restrict__ out) {
  const long long r = (long long)blockIdx.x * FN_BLOCK + threadIdx.x;
  if (r >= R) return;
  const float* w = weights + r * S;
  const float* nr = normals + r * S * 3;
  float a[3] = {0.0f, 0.0f, 0.0f};
  for (int s = 0; s < S; ++s) {
    const float ws = w[s];
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = fadd(a[c], fmul(ws, nr[3 * s + c]));
  }
  const float norm = sqrtf(fadd(fadd(fmul(a[0], a[0]), fmul(a[1], a[1])), fmul(a[2], a[2])));
  const float d = fadd(norm, 1e-10f);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = fdiv(a[c], d);
    if (shade) v = fdiv(fadd(v, 1.0f), 2.0f);
    out[3 * r + c] = v;
  }
}

}  // namespace fnr

using namespace fnr;

extern "C" int fnr_field_normals(const fnr_field_net* net, int64_t n_samples, const float* feats, const float* jacobian,
                                 const uint8_t* selector, float* normals, float* gradient, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_field_normals");
  FNR_CHECK_ARG(net && feats && jacobian && selector && normals, "field_normals: null argument");
  FNR_UNSUPPORTED(net->grid.n_levels == FN_LEVELS, "field_normals: num_levels %d not built (16 only)", net->grid.n_levels);
  FNR_UNSUPPORTED(net->hidden_dim == FN_HID && (net->geo_feat_dim == 15 || net->geo_feat_dim == 30),
                  "field_normals: built for the base MLP 32 -> 64 -> 1 + geo with geo 15 or 30; got hidden %d geo %d",
                  net->hidden_dim, net->geo_feat_dim);
  FNR_CHECK_ARG(net->base_w0 && net->base_b0 && net->base_w1, "field_normals: null weight/bias pointer");
  FNR_CHECK_ARG(n_samples >= 0, "field_normals: n_samples < 0");
  if (n_samples == 0) return FNR_OK;
  const long long nblocks = (n_samples + FN_BLOCK - 1) / FN_BLOCK;
  FNR_CHECK_ARG(nblocks < (1ll << 31), "field_normals: batch too large");
  hipLaunchKernelGGL(k_field_normals, dim3((unsigned)nblocks), dim3(FN_BLOCK), 0, as_stream(stream), (long long)n_samples,
                     net->base_w0, net->base_b0, net->base_w1, reinterpret_cast<const float2*>(feats),
                     reinterpret_cast<const float2*>(jacobian), selector, normals, gradient);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

extern "C" int fnr_render_normals(int64_t n_rays, int S, const float* weights, const float* normals, int shade, float* out,
                                  void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_render_normals");
  FNR_CHECK_ARG(weights && normals && out, "render_normals: null argument");
  FNR_CHECK_ARG(n_rays >= 0 && S > 0, "render_normals: n_rays %lld / S %d out of range", (long long)n_rays, S);
  if (n_rays == 0) return FNR_OK;
  const long long nblocks = (n_rays + FN_BLOCK - 1) / FN_BLOCK;
  FNR_CHECK_ARG(nblocks < (1ll << 31), "render_normals: batch too large");
  hipLaunchKernelGGL(k_render_normals, dim3((unsigned)nblocks), dim3(FN_BLOCK), 0, as_stream(stream), (long long)n_rays, S,
                     weights, normals, shade, out);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}
