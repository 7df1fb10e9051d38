// sampler.hip — hierarchical ray sampling for gfx950: SpacedSampler bins, RaySamples.get_weights and the
// inverse-CDF PDFSampler (nerfstudio 0.3.2 semantics, driven from fruit_nerf.py:151-158,318).
// One 64-lane wave owns one ray: per-ray scans are wave scans, the CDF lives in LDS, searchsorted is a
// per-lane binary search.  These kernels are latency-trivial next to the field queries (HBM-bound reads
// of S floats per ray); they exist so the whole sampling chain stays on the device without launches of
// dozens of small elementwise ops.
#include "sampler_math.hpp"
#include "sequencer.hpp"
#include "step_randoms.hpp"

namespace fnr {

__global__ __launch_bounds__(256) void k_sample_spaced(RaysDev rays, int kind, int S,
                                                       const float* __restrict__ base_bins,
                                                       const float* __restrict__ t_rand, int t_rand_per_bin,
                                                       float* __restrict__ spacing, float* __restrict__ euclid) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = rays.n_rays * (long long)(S + 1);
  if (idx >= total) return;
  const long long r = idx / (S + 1);
  const int j = (int)(idx - r * (S + 1));
  // single_jitter: one number per ray; otherwise one per bin edge, t_rand [R, S+1] (ray_samplers.py:79-83)
  const float b = spaced_bin_edge(base_bins, S, j, t_rand != nullptr, t_rand ? t_rand[t_rand_per_bin ? idx : r] : 0.0f);
  const float s_near = spacing_fn(kind, rays.nears[r]), s_far = spacing_fn(kind, rays.fars[r]);
  spacing[idx] = b;
  euclid[idx] = spacing_to_euclid(kind, b, s_near, s_far);
}

constexpr int PDF_MAXE = 8;        // elements per lane -> S_prev <= 512
constexpr int PDF_MAX_PREV = 512;  // LDS cdf capacity per wave
static_assert(PDF_MAXE == RAY_MAX_LANE_ELEMS && PDF_MAX_PREV == 64 * PDF_MAXE, "with_lane_elems picks the kernel");

// ME: elements per lane the register arrays hold (S_prev <= 64 ME; with_lane_elems picks the narrowest).  The elements a
// narrower form drops are zeros added to sums that start from +0.0 behind the live elements, or feed nothing: same bits.
// Everything the wave reads from memory is issued at the top — the resampling's inputs included, the previous level's bin
// edges staged into LDS next to the CDF — so that a wave waits for memory once, not once per phase.  Six waves per SIMD (80
// registers at most) keep a 4096-ray launch one resident generation of workgroups whatever ME.
// EDGES (use_single_jitter = False, fnr_weights_pdf_edges): one jitter per new bin edge instead of one per ray — read from
// rand [R, S_new + 1], or with edges.draw drawn here from the step's generator (step_randoms.hpp: one Philox call per edge; a
// wave's 64 lanes make their calls in one pass, so sharing a call among the four edges of a quad would save no instructions
// below 256 edges and cost four cross-lane reads per pass; measured).  Only the resampling's `u` differs between
// the two forms.
template <int ME, bool EDGES>
__device__ __forceinline__ void weights_pdf_ray(float* cdf, float* ex, const RaysDev& rays, int kind, int S_prev, int S_new,
                                                const float* __restrict__ density, const float* __restrict__ spacing_prev,
                                                const float* __restrict__ euclid_prev, float anneal,
                                                const float* __restrict__ u_base, const float* __restrict__ rand,
                                                const EdgeDraw& edges, float* __restrict__ weights,
                                                float* __restrict__ median_depth, float* __restrict__ spacing_new,
                                                float* __restrict__ euclid_new) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * 4 + wave;
  if (r >= rays.n_rays) return;  // whole wave exits together
  const int E = (S_prev + 63) >> 6;
  const float* eb = euclid_prev + r * (S_prev + 1);
  const float* dn = density + r * S_prev;
  const int nb = S_new + 1;

  // ---- the resampling's inputs: asked for first, used last ------------------------------------------
  float near_r = 0.0f, far_r = 0.0f, rand_r = 0.0f, u0 = 0.0f, u1 = 0.0f;
  [[maybe_unused]] float rand_1 = 0.0f;   // (EDGES: rand_r / rand_1 = the numbers of edges lane, lane + 64)
  float spv[ME + 1];
#pragma unroll
  for (int q = 0; q <= ME; ++q) {
    const int k = lane + 64 * q;
    spv[q] = (S_new > 0 && k <= S_prev) ? spacing_prev[r * (S_prev + 1) + k] : 0.0f;
  }
  if (S_new > 0) {
    near_r = rays.nears[r];
    far_r = rays.fars[r];
    if constexpr (EDGES) {
      if (rand) {
        if (lane < nb) rand_r = rand[r * nb + lane];
        if (lane + 64 < nb) rand_1 = rand[r * nb + lane + 64];
      } else if (edges.draw) {   // drawn where the pointer form loads them, while the loads above are in flight
        if (lane < nb) rand_r = edge_jitter(edges.seed, edges.offset, edges.level, r, lane);
        if (lane + 64 < nb) rand_1 = edge_jitter(edges.seed, edges.offset, edges.level, r, lane + 64);
      }
    } else {
      if (rand) rand_r = rand[r];
    }
    if (lane < nb) u0 = u_base[lane];
    if (lane + 64 < nb) u1 = u_base[lane + 64];
  }

  // ---- RaySamples.get_weights ----------------------------------------------------------------
  float dd[ME], w[ME];
  float local = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    dd[e] = 0.0f;
    if (e < E && k < S_prev) dd[e] = fmul(fsub(eb[k + 1], eb[k]), dn[k]);
    local += dd[e];
  }
  if (S_new > 0) {
#pragma unroll
    for (int q = 0; q <= ME; ++q) {
      const int k = lane + 64 * q;
      if (k <= S_prev) ex[k] = spv[q];   // (read behind the CDF's lgkmcnt(0) + wave barrier)
    }
  }
  float excl = wave_excl_scan(local, lane);  // sum of delta*sigma before this lane's chunk
  float wsum_local = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    const float T = expf(-excl);
    const float alpha = 1.0f - expf(-dd[e]);
    w[e] = nan_to_num(alpha * T);
    excl += dd[e];
    if (e < E && k < S_prev) {
      weights[r * S_prev + k] = w[e];
      wsum_local += w[e];
    } else {
      w[e] = 0.0f;
    }
  }

  // ---- DepthRenderer("median") of this level (fruit_nerf.py:299-300) ----------------------------
  if (median_depth) {
    float cw = wave_excl_scan(wsum_local, lane);
    int first = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < ME; ++e) {
      const int k = lane * E + e;
      cw += w[e];
      if (e < E && k < S_prev && cw >= 0.5f && first == 0x7fffffff) first = k;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) first = min(first, __shfl_xor(first, d, 64));
    if (first > S_prev - 1) first = S_prev - 1;
    if (lane == 0) median_depth[r] = fdiv(fadd(eb[first], eb[first + 1]), 2.0f);
  }
  if (S_new <= 0) return;

  // ---- PDFSampler: annealed, padded histogram -> CDF in LDS --------------------------------------
  float wa[ME];
  float sum_local = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    wa[e] = 0.0f;
    if (e < E && k < S_prev) {
      const float p = (anneal == 1.0f) ? w[e] : powf(w[e], anneal);
      wa[e] = fadd(p, 0.01f);  // histogram_padding
    }
    sum_local += wa[e];
  }
  float wsum = wave_sum(sum_local);
  const float padding = fmaxf(fsub(1e-5f, wsum), 0.0f);
  const float pad_each = fdiv(padding, (float)S_prev);
  wsum = fadd(wsum, padding);
  float pdf_local = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    if (e < E && k < S_prev) {
      wa[e] = fdiv(fadd(wa[e], pad_each), wsum);
      pdf_local += wa[e];
    }
  }
  float run = wave_excl_scan(pdf_local, lane);
  if (lane == 0) cdf[0] = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    if (e < E && k < S_prev) {
      run += wa[e];
      cdf[k + 1] = fminf(1.0f, run);
    }
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes done (in-order LDS queue)
  __builtin_amdgcn_wave_barrier();

  // ---- inverse-CDF resampling ----------------------------------------------------------------------
  const float u_centre = (float)(1.0 / (2.0 * (double)nb));
  const float u_shift = EDGES ? u_centre : rand ? fdiv(rand_r, (float)nb) : u_centre;
  const float s_near = spacing_fn(kind, near_r), s_far = spacing_fn(kind, far_r);
  for (int jj = lane; jj < nb; jj += 64) {
    float shift = u_shift;
    if constexpr (EDGES) {
      if (rand || edges.draw)
        shift = fdiv(jj == lane ? rand_r : jj == lane + 64 ? rand_1 : rand ? rand[r * nb + jj]
                                 : edge_jitter(edges.seed, edges.offset, edges.level, r, jj), (float)nb);
    }
    const float u = fadd(jj == lane ? u0 : jj == lane + 64 ? u1 : u_base[jj], shift);
    // searchsorted(cdf, u, side="right"): number of entries <= u
    int lo = 0, hi = S_prev + 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf[mid] <= u) lo = mid + 1;
      else hi = mid;
    }
    const int below = min(max(lo - 1, 0), S_prev), above = min(max(lo, 0), S_prev);
    const float c0 = cdf[below], c1 = cdf[above];
    float t = fdiv(fsub(u, c0), fsub(c1, c0));
    t = nan_to_num(t);
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const float b0 = ex[below], b1 = ex[above];
    const float b = fadd(b0, fmul(t, fsub(b1, b0)));
    spacing_new[r * nb + jj] = b;
    euclid_new[r * nb + jj] = spacing_to_euclid(kind, b, s_near, s_far);
  }
}

template <int ME>
__global__ __launch_bounds__(256, 6) void k_weights_pdf(RaysDev rays, int kind, int S_prev, int S_new,
                                                        const float* __restrict__ density,
                                                        const float* __restrict__ spacing_prev,
                                                        const float* __restrict__ euclid_prev, float anneal,
                                                        const float* __restrict__ u_base, const float* __restrict__ rand,
                                                        float* __restrict__ weights, float* __restrict__ median_depth,
                                                        float* __restrict__ spacing_new, float* __restrict__ euclid_new) {
  constexpr int CAP = 64 * ME;
  __shared__ float s_cdf[4][CAP + 1];
  __shared__ float s_ex[4][CAP + 1];
  const int wave = threadIdx.x >> 6;
  weights_pdf_ray<ME, false>(s_cdf[wave], s_ex[wave], rays, kind, S_prev, S_new, density, spacing_prev, euclid_prev, anneal,
                             u_base, rand, EdgeDraw{}, weights, median_depth, spacing_new, euclid_new);
}
template <int ME>
__global__ __launch_bounds__(256, 6) void k_weights_pdf_edges(RaysDev rays, int kind, int S_prev, int S_new,
                                                              const float* __restrict__ density,
                                                              const float* __restrict__ spacing_prev,
                                                              const float* __restrict__ euclid_prev, float anneal,
                                                              const float* __restrict__ u_base,
                                                              const float* __restrict__ rand, EdgeDraw edges,
                                                              float* __restrict__ weights, float* __restrict__ median_depth,
                                                              float* __restrict__ spacing_new,
                                                              float* __restrict__ euclid_new) {
  constexpr int CAP = 64 * ME;
  __shared__ float s_cdf[4][CAP + 1];
  __shared__ float s_ex[4][CAP + 1];
  const int wave = threadIdx.x >> 6;
  weights_pdf_ray<ME, true>(s_cdf[wave], s_ex[wave], rays, kind, S_prev, S_new, density, spacing_prev, euclid_prev, anneal,
                            u_base, rand, edges, weights, median_depth, spacing_new, euclid_new);
}

}  // namespace fnr

using namespace fnr;

extern "C" int fnr_sample_spaced(const fnr_rays* rays, int spacing_kind, int S, const float* base_bins,
                                 const float* t_rand, int t_rand_per_bin, float* spacing_bins, float* euclid_bins,
                                 void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_sample_spaced");
  FNR_CHECK_ARG(rays && base_bins && spacing_bins && euclid_bins && S > 0, "sample_spaced: null argument");
  FNR_CHECK_ARG(rays->nears && rays->fars, "sample_spaced: rays.nears/fars must be set (collider, fruit_nerf.py:382)");
  FNR_CHECK_ARG(spacing_kind == 0 || spacing_kind == 1, "sample_spaced: spacing_kind %d", spacing_kind);
  const long long total = rays->n_rays * (long long)(S + 1);
  if (total == 0) return FNR_OK;
  FNR_PROF(OP_SAMPLE_SPACED, total);
  hipLaunchKernelGGL(k_sample_spaced, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream),
                     make_rays(rays), spacing_kind, S, base_bins, t_rand, t_rand_per_bin, spacing_bins, euclid_bins);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

// edges: NULL for fnr_weights_pdf (rand [R] or NULL), the generator's arguments of fnr_weights_pdf_edges otherwise (rand
// [R, S_new + 1] or NULL).  name: the export that was called; a step program lists and replays the call under it.
static int weights_pdf(const char* name, const EdgeDraw* edges, const fnr_rays* rays, int spacing_kind, int S_prev, int S_new,
                       const float* density, const float* spacing_prev, const float* euclid_prev, float anneal,
                       const float* u_base, const float* rand, float* weights, float* median_depth, float* spacing_new,
                       float* euclid_new, void* stream) {
  seq::record(name, &weights_pdf, name, seq::optional(edges), rays, spacing_kind, S_prev, S_new, density, spacing_prev,
              euclid_prev, seq::Anneal{anneal}, u_base, rand, weights, median_depth, spacing_new, euclid_new, stream);
  FNR_CHECK_ARG(rays && density && euclid_prev && weights, "weights_pdf: null argument");
  FNR_CHECK_ARG(!edges || !edges->draw ||
                    (!rand && edges->level >= 1 && edges->level < FNR_EDGE_JITTER_MAX_LEVELS && S_new < FNR_EDGE_JITTER_MAX_EDGES),
                "weights_pdf_edges: draw goes with rand == NULL, a level in 1..%d (level %d) and S_new below %d",
                FNR_EDGE_JITTER_MAX_LEVELS - 1, edges->level, FNR_EDGE_JITTER_MAX_EDGES);
  FNR_CHECK_ARG(S_prev > 0 && S_prev <= PDF_MAX_PREV, "weights_pdf: S_prev %d out of range (1..%d)", S_prev,
                PDF_MAX_PREV);
  FNR_CHECK_ARG(S_new == 0 || (spacing_prev && u_base && spacing_new && euclid_new),
                "weights_pdf: resampling needs spacing_prev/u_base/outputs");
  FNR_CHECK_ARG(spacing_kind == 0 || spacing_kind == 1, "weights_pdf: spacing_kind %d", spacing_kind);
  if (rays->n_rays == 0) return FNR_OK;
  FNR_PROF(OP_WEIGHTS_PDF, rays->n_rays * (long long)S_prev);
  with_lane_elems(S_prev, [&](auto me) {
    if (edges)
      hipLaunchKernelGGL(k_weights_pdf_edges<decltype(me)::value>, dim3((unsigned)((rays->n_rays + 3) / 4)), dim3(256), 0,
                         as_stream(stream), make_rays(rays), spacing_kind, S_prev, S_new, density, spacing_prev, euclid_prev,
                         anneal, u_base, rand, *edges, weights, median_depth, spacing_new, euclid_new);
    else
      hipLaunchKernelGGL(k_weights_pdf<decltype(me)::value>, dim3((unsigned)((rays->n_rays + 3) / 4)), dim3(256), 0,
                         as_stream(stream), make_rays(rays), spacing_kind, S_prev, S_new, density, spacing_prev, euclid_prev,
                         anneal, u_base, rand, weights, median_depth, spacing_new, euclid_new);
  });
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

extern "C" int fnr_weights_pdf(const fnr_rays* rays, int spacing_kind, int S_prev, int S_new, const float* density,
                               const float* spacing_prev, const float* euclid_prev, float anneal, const float* u_base,
                               const float* rand, float* weights, float* median_depth, float* spacing_new,
                               float* euclid_new, void* stream) {
  return weights_pdf("fnr_weights_pdf", nullptr, rays, spacing_kind, S_prev, S_new, density, spacing_prev, euclid_prev, anneal,
                     u_base, rand, weights, median_depth, spacing_new, euclid_new, stream);
}

extern "C" int fnr_weights_pdf_edges(const fnr_rays* rays, int spacing_kind, int S_prev, int S_new, const float* density,
                                     const float* spacing_prev, const float* euclid_prev, float anneal, const float* u_base,
                                     const float* rand, float* weights, float* median_depth, float* spacing_new,
                                     float* euclid_new, uint64_t seed, uint64_t offset, int level, int draw, void* stream) {
  const EdgeDraw edges{seed, offset, level, draw != 0 ? 1 : 0};
  return weights_pdf("fnr_weights_pdf_edges", &edges, rays, spacing_kind, S_prev, S_new, density, spacing_prev, euclid_prev,
                     anneal, u_base, rand, weights, median_depth, spacing_new, euclid_new, stream);
}
