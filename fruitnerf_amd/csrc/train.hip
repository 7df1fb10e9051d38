// train.hip — losses and their gradients for gfx950.
//   get_loss_dict (fruit_nerf.py:359-372): MSELoss, BCEWithLogitsLoss, interlevel_loss
//   get_metrics_dict (fruit_nerf.py:396-401): distortion_loss (metric only)
// (the optimiser's sweeps: optim.hip; the backward of RaySamples.get_weights + renderers: composite_bwd.hip)
// One wave per ray for the per-ray scans; everything here is bandwidth-trivial next to the field kernels.
#include "common.hpp"
#include "composite_math.hpp"
#include "sequencer.hpp"

namespace fnr {

// ---------------------------------------------------------------------------------------------------
// rgb MSE + semantic BCE-with-logits: values and unit gradients (mse_grad, bce_logit_grad: composite_math.hpp)
// ---------------------------------------------------------------------------------------------------
// One workgroup: a training batch is a few thousand rays, and finishing inside the kernel (block reduction, PSNR)
// saves the memset, the atomics and three follow-up elementwise launches per step.
template <int THREADS>
__device__ __forceinline__ void losses_block(long long R, const float* __restrict__ rgb,
                                             const float* __restrict__ image, const float* __restrict__ sem,
                                             const float* __restrict__ mask, float sem_weight,
                                             float* __restrict__ losses, float* __restrict__ d_rgb,
                                             float* __restrict__ d_sem) {
  __shared__ float red[2][16];
  float l_rgb = 0.0f, l_sem = 0.0f;
  const float inv3r = 1.0f / (float)(3 * R), invr = 1.0f / (float)R;
  for (long long r = threadIdx.x; r < R; r += THREADS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = rgb[3 * r + c] - image[3 * r + c];
      l_rgb += d * d;
      d_rgb[3 * r + c] = mse_grad(d, inv3r);
    }
    const float x = sem[r], y = mask[r];
    // BCEWithLogits: max(x,0) - x*y + log1p(exp(-|x|))
    l_sem += fmaxf(x, 0.0f) - x * y + log1pf(expf(-fabsf(x)));
    d_sem[r] = bce_logit_grad(x, y, sem_weight, invr);
  }
  l_rgb = wave_sum(l_rgb);
  l_sem = wave_sum(l_sem);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = l_rgb;
    red[1][threadIdx.x >> 6] = l_sem;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.0f, b = 0.0f;
    for (int w = 0; w < THREADS / 64; ++w) {
      a += red[0][w];
      b += red[1][w];
    }
    const float mse = a * inv3r;
    losses[0] = mse;
    losses[1] = sem_weight * b * invr;
    losses[2] = -10.0f * log10f(mse);  // PeakSignalNoiseRatio(data_range=1.0) of the same batch (fruit_nerf.py:398)
  }
}
__global__ __launch_bounds__(1024) void k_losses(long long R, const float* __restrict__ rgb,
                                                 const float* __restrict__ image, const float* __restrict__ sem,
                                                 const float* __restrict__ mask, float sem_weight,
                                                 float* __restrict__ losses, float* __restrict__ d_rgb,
                                                 float* __restrict__ d_sem) {
  losses_block<1024>(R, rgb, image, sem, mask, sem_weight, losses, d_rgb, d_sem);
}

// ---------------------------------------------------------------------------------------------------
// interlevel loss of one proposal level against the final level (nerfstudio losses.interlevel_loss):
// value (accumulated) + unit gradient w.r.t. the proposal weights.
// ---------------------------------------------------------------------------------------------------
constexpr int IL_MAX_P = 512;

// k_weights_bwd (composite_bwd.hip) for one ray with everything it reads already in registers: the upstream gradient d(loss)/d(w_k) (gw[e]
// belongs to sample lane * E + e, zero beyond S), the weights, delta = the bin widths and the densities.  Same operations in the
// same order -> bit-identical d_density.
template <int ME>
__device__ __forceinline__ void weights_bwd_ray_from_regs(long long r, int S, int lane, const float (&delta)[ME],
                                                          const float (&dnv)[ME], const float (&wk)[ME],
                                                          const float (&gw)[ME], float* __restrict__ d_density) {
  const int E = (S + 63) >> 6;
  float dd_local = 0.0f, gww_local = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    if (e < E && k < S) {
      dd_local += delta[e] * dnv[e];
      gww_local += gw[e] * wk[e];
    }
  }
  float cum_dd = wave_excl_scan(dd_local, lane);
  float suffix =
      padded_suffix<ME>(wave_bcast_lane(wave_excl_scan(wave_bcast_lane(gww_local, 63 - lane), lane), 63 - lane));
  float suf[ME];
#pragma unroll
  for (int e = ME - 1; e >= 0; --e) {
    suf[e] = suffix;
    suffix += gw[e] * wk[e];   // gw / wk are 0 for e >= E or k >= S
  }
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    if (e < E && k < S) {
      cum_dd += delta[e] * dnv[e];
      const float T_next = expf(-cum_dd);
      d_density[r * S + k] = delta[e] * (gw[e] * T_next - suf[e]);
    }
  }
}
constexpr int IL_LDS_FLOATS = 4 * (3 * IL_MAX_P + 4);   // per wave: cp [P+1], cy [P+1], dd [P+2]

__device__ __forceinline__ int searchsorted_right(const float* a, int n, float v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// A wave's contribution to a loss accumulator row (FNR_LOSS_SLOTS floats spread over 32 cache lines: same-line atomics
// serialise).  FIXED (fnr_train_losses): the row is read as 512 64-bit words and the value is added as two's-complement
// fixed point (2^-34 resolution) — integer adds commute, so the logged losses and metrics are bit-identical run to run like
// the gradients.  A contribution that is not finite or above its row's bound raises `flag` instead (the result is then
// NaN): per-ray contributions (interlevel, distortion: already divided by R) |v| <= 2^12, up to 2^17 of them — more than
// any built method launches per row (fruit_nerf_huge: 16 384 rays x 2 proposal levels); the rgb / semantic rows' raw
// per-wave sums |v| <= 2^28 / waves.  At a scale of 2^34 neither a slot nor the total can reach 2^63 and wrap
// (at 2^44 a total of ~5e5, e.g. a diverging semantic BCE sum over a large batch, wrapped silently).
constexpr double TL_FIX_SCALE = 17179869184.0;  // 2^34
constexpr float TL_FIX_MAX = 4096.0f;
template <bool FIXED>
__device__ __forceinline__ void slot_add(float* __restrict__ row, int block, int wave, float v, unsigned* flag = nullptr,
                                         float vmax = TL_FIX_MAX) {
  if constexpr (FIXED) {
    if (!(fabsf(v) <= vmax)) {  // inf / nan / absurd
      if (flag) atomicOr(flag, 1u);
      return;
    }
    const long long q = __double2ll_rn((double)v * TL_FIX_SCALE);
    atomicAdd(reinterpret_cast<unsigned long long*>(row) + (block & 31) * 16 + wave, (unsigned long long)q);
  } else {
    atomicAdd(&row[(block & 31) * 32 + wave], v);
  }
}

// distortion_loss (metric, fruit_nerf.py:400) of one ray, by its wave: sum_ij w_i w_j |m_i - m_j| + sum_i w_i^2 ds_i / 3, the
// wave's total in every lane.  s_m / s_w: S floats of LDS each, this wave's own.  t0, t1, w0: t[lane], t[lane + 1], w[lane],
// loaded by the caller (lanes >= S: anything) — a caller that holds the ray already pays no second round trip to memory.
__device__ __forceinline__ float distortion_wave(int S, const float* __restrict__ t, const float* __restrict__ w,
                                                 float* s_m, float* s_w, int lane, float t0, float t1, float w0) {
  if (lane < S) {
    s_m[lane] = (t1 + t0) / 2.0f;
    s_w[lane] = w0;
  }
  for (int k = lane + 64; k < S; k += 64) {
    s_m[k] = (t[k + 1] + t[k]) / 2.0f;
    s_w[k] = w[k];
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  float acc = 0.0f;
  for (int i = lane; i < S; i += 64) {
    const float mi = s_m[i], wi = s_w[i];
    float inner = 0.0f;
    for (int j = 0; j < S; ++j) inner += s_w[j] * fabsf(mi - s_m[j]);
    const float ds = i == lane ? t1 - t0 : t[i + 1] - t[i];
    acc += wi * inner + wi * wi * ds / 3.0f;
  }
  return wave_sum(acc);
}

// ME: samples per lane the register arrays hold (S_p <= 64 ME).  dist_out (k_train_losses): this wave also sums the
// distortion metric of its ray — it needs only the final level's spacing and weights, which the wave reads anyway — in the
// first 2 S_f floats of its own LDS region, once it has read `dd` for the last time.
template <bool FIXED = false, int ME = WB_MAXE>
__device__ __forceinline__ void interlevel_block(long long R, int S_f, const float* __restrict__ spacing_f,
                                                 const float* __restrict__ w_f, int S_p,
                                                 const float* __restrict__ spacing_p, const float* __restrict__ w_p,
                                                 float mult, float* __restrict__ loss, float* __restrict__ d_wp,
                                                 int block, float* lds, int p_cap,  // lds: 4 * (3 * p_cap + 4) floats
                                                 const float* __restrict__ euclid_p = nullptr,
                                                 const float* __restrict__ density_p = nullptr,
                                                 float* __restrict__ d_density_p = nullptr, unsigned* flag = nullptr,
                                                 float* __restrict__ dist_out = nullptr) {  // needs 2 S_f <= 3 p_cap + 4
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)block * 4 + wave;
  if (r >= R) return;
  float* cp = lds + wave * (3 * p_cap + 4);   // p_cap >= S_p: the launch sizes the buffer for its largest level
  float* cy = cp + p_cap + 1;
  float* dd = cy + p_cap + 1;
  const float* sp = spacing_p + r * (S_p + 1);
  const float* wp = w_p + r * S_p;
  const float* c = spacing_f + r * (S_f + 1);
  const float* w = w_f + r * S_f;
  const int E = (S_p + 63) >> 6;
  // ---- everything the wave reads from memory, issued before anything waits: one round trip, not one per phase ----------
  float wv[ME], spv[ME + 1], delta[ME], dnv[ME];
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    wv[e] = (e < E && k < S_p) ? wp[k] : 0.0f;
  }
#pragma unroll
  for (int q = 0; q <= ME; ++q) {
    const int k = lane + 64 * q;
    spv[q] = k <= S_p ? sp[k] : 0.0f;
  }
  float c0 = 0.0f, c1 = 0.0f, w0 = 0.0f;   // the final level's first 64 samples (all of them at the usual 48)
  if (lane < S_f) {
    c0 = c[lane];
    c1 = c[lane + 1];
    w0 = w[lane];
  }
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    delta[e] = 0.0f;
    dnv[e] = 0.0f;
    if (d_density_p && e < E && k < S_p) {
      const float* eb = euclid_p + r * (S_p + 1);
      delta[e] = eb[k + 1] - eb[k];
      dnv[e] = density_p[r * S_p + k];
    }
  }
  // cy1 = [0, cumsum(wp)] : lane-chunked scan
  float local = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    if (e < E && k < S_p) local += wv[e];
  }
  float run = wave_excl_scan(local, lane);
  if (lane == 0) cy[0] = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    if (e < E && k < S_p) {
      run += wv[e];
      cy[k + 1] = run;
    }
  }
#pragma unroll
  for (int q = 0; q <= ME; ++q) {
    const int k = lane + 64 * q;
    if (k <= S_p) cp[k] = spv[q];
  }
  for (int k = lane; k <= S_p + 1; k += 64) dd[k] = 0.0f;
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();

  const float scale = mult / (float)(R * (long long)S_f);
  float lsum = 0.0f;
  for (int i = lane; i < S_f; i += 64) {
    const bool head = i == lane;
    const float ci = head ? c0 : c[i], ci1 = head ? c1 : c[i + 1];
    int lo = searchsorted_right(cp, S_p, ci) - 1;            // t1_starts = cp[:-1]
    lo = min(max(lo, 0), S_p - 1);
    int hi = searchsorted_right(cp + 1, S_p, ci1);           // t1_ends = cp[1:]
    hi = min(max(hi, 0), S_p - 1);
    const float w_outer = cy[hi + 1] - cy[lo];
    const float wi = head ? w0 : w[i];
    const float diff = fmaxf(wi - w_outer, 0.0f);
    const float den = wi + 1.0e-7f;
    lsum += diff * diff / den;
    const float g = -2.0f * diff / den * scale;  // d loss / d w_outer
    if (g != 0.0f) {
      atomicAdd(&dd[lo], g);
      atomicAdd(&dd[hi + 1], -g);
    }
  }
  lsum = wave_sum(lsum);
  // atomics to one L2 line serialise at ~12 ns each (4096 rays = ~35-50 us): 32 lines, 4 words (waves) per line
  if (lane == 0) slot_add<FIXED>(loss, block, wave, lsum * scale, flag);
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  // d_wp = inclusive scan of the difference array
  float ddv[ME];
  float l2 = 0.0f;
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    ddv[e] = 0.0f;
    if (e < E && k < S_p) {
      ddv[e] = dd[k];
      l2 += ddv[e];
    }
  }
  float run2 = wave_excl_scan(l2, lane);
  // (with d_density_p: the proposal level's weights backward right here — the ray is in this wave's hands, d_wp and the
  // level's weights stay in registers)
  float gw[ME];
#pragma unroll
  for (int e = 0; e < ME; ++e) {
    const int k = lane * E + e;
    gw[e] = 0.0f;
    if (e < E && k < S_p) {
      run2 += ddv[e];
      gw[e] = run2;
      if (d_wp) d_wp[r * S_p + k] = run2;
    }
  }
  if (dist_out) {   // ahead of the backward: its slot atomic is acknowledged while the backward runs
    __builtin_amdgcn_wave_barrier();   // `dd` has been read: the region is free
    const float acc = distortion_wave(S_f, c, w, cp, cp + S_f, lane, c0, c1, w0);
    if (lane == 0) slot_add<FIXED>(dist_out, block, wave, acc / (float)R, flag);
  }
  if (d_density_p) weights_bwd_ray_from_regs<ME>(r, S_p, lane, delta, dnv, wv, gw, d_density_p);
}
__global__ __launch_bounds__(256) void k_interlevel(long long R, int S_f, const float* __restrict__ spacing_f,
                                                    const float* __restrict__ w_f, int S_p,
                                                    const float* __restrict__ spacing_p,
                                                    const float* __restrict__ w_p, float mult,
                                                    float* __restrict__ loss, float* __restrict__ d_wp) {
  __shared__ float lds[IL_LDS_FLOATS];
  interlevel_block(R, S_f, spacing_f, w_f, S_p, spacing_p, w_p, mult, loss, d_wp, blockIdx.x, lds, IL_MAX_P);
}

// distortion_loss (metric, fruit_nerf.py:400): mean over rays of sum_ij w_i w_j |m_i - m_j| + sum_i w_i^2 ds_i / 3
template <bool FIXED = false>
__device__ __forceinline__ void distortion_block(long long R, int S, const float* __restrict__ spacing,
                                                 const float* __restrict__ weights, float* __restrict__ out,
                                                 int block, float* lds, int s_cap, unsigned* flag = nullptr) {  // lds: 8 * s_cap floats, s_cap >= S
  float* s_m_all = lds;
  float* s_w_all = lds + 4 * s_cap;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)block * 4 + wave;
  if (r >= R) return;
  const float* t = spacing + r * (S + 1);
  const float* w = weights + r * S;
  float t0 = 0.0f, t1 = 0.0f, w0 = 0.0f;
  if (lane < S) {
    t0 = t[lane];
    t1 = t[lane + 1];
    w0 = w[lane];
  }
  const float acc = distortion_wave(S, t, w, s_m_all + wave * s_cap, s_w_all + wave * s_cap, lane, t0, t1, w0);
  if (lane == 0) slot_add<FIXED>(out, block, wave, acc / (float)R, flag);
}
__global__ __launch_bounds__(256) void k_distortion(long long R, int S, const float* __restrict__ spacing,
                                                    const float* __restrict__ weights, float* __restrict__ out) {
  __shared__ float lds[4096];
  distortion_block(R, S, spacing, weights, out, blockIdx.x, lds, 512);
}

// Every loss of a training step in ONE launch (fnr_train_losses; five dependent 4-10 us launches before): workgroups
// [0, nbl) = rgb + semantic losses and their gradients (256 rays each), then (R + 3) / 4 workgroups per proposal level
// = interlevel loss, one wave per ray.  The distortion metric of a ray is summed by the wave that holds the ray for the
// proposal level with the fewest samples (dist_host); only where no level can host it — none given, or 2 S_f floats do not
// fit a wave's LDS region — it gets (R + 3) / 4 workgroups of its own at the end.  The kernel is compiled per ME (see
// with_lane_elems) and kept at 64 registers for ME <= 4, eight workgroups per CU: a 4096-ray batch with two proposal
// levels is 2064 workgroups, one resident generation on 256 CUs.  Sums go to accumulator slots in 32 different 128-byte
// lines (same-line atomics serialise at ~12 ns each); the last workgroup to finish — found with a two-level
// completion count for the same reason — adds the slots up and writes the five scalars.
struct LevelLossArgs {
  int n_levels;
  int dist_host;   // the level whose waves sum the distortion metric too; -1: none
  int S_p[FNR_MAX_PROPOSAL_LEVELS];
  const float* spacing_p[FNR_MAX_PROPOSAL_LEVELS];
  const float* w_p[FNR_MAX_PROPOSAL_LEVELS];
  float* d_wp[FNR_MAX_PROPOSAL_LEVELS];
  const float* euclid_p[FNR_MAX_PROPOSAL_LEVELS];   // with d_density_p: the level's weights backward is fused in
  const float* density_p[FNR_MAX_PROPOSAL_LEVELS];
  float* d_density_p[FNR_MAX_PROPOSAL_LEVELS];
};
constexpr int TL_ROWS = 4;                                       // slot rows: interlevel, distortion, rgb, semantic
constexpr int TL_ACCUM_FLOATS = TL_ROWS * FNR_LOSS_SLOTS + 33 * 32;  // + 32 group counters and the top one, a line each
static_assert(TL_ACCUM_FLOATS == FNR_TRAIN_LOSSES_ACCUM_FLOATS, "fruitnerf_hip.h: FNR_TRAIN_LOSSES_ACCUM_FLOATS");
template <int ME>
__global__ __launch_bounds__(256, ME <= 4 ? 8 : 1) void k_train_losses(long long R, const float* __restrict__ rgb,
                                                      const float* __restrict__ image, const float* __restrict__ sem,
                                                      const float* __restrict__ mask, float sem_weight,
                                                      float* __restrict__ d_rgb, float* __restrict__ d_sem, int S_f,
                                                      const float* __restrict__ spacing_f,
                                                      const float* __restrict__ w_f, LevelLossArgs lv, float mult,
                                                      int want_distortion, float* __restrict__ accum,
                                                      float* __restrict__ losses, int p_cap) {
  extern __shared__ float lds[];   // 4 * (3 * p_cap + 4) floats, 8 * S_f for a distortion role: sized by the launch
  __shared__ bool s_last;
  __shared__ unsigned long long s_tot[TL_ROWS];
  static_assert(TL_ROWS == 4 && FNR_LOSS_SLOTS == 1024, "the last workgroup's two rows per thread");
  float* il_slots = accum;
  float* di_slots = accum + FNR_LOSS_SLOTS;
  float* rgb_slots = accum + 2 * FNR_LOSS_SLOTS;
  float* sem_slots = accum + 3 * FNR_LOSS_SLOTS;
  unsigned* cnt = reinterpret_cast<unsigned*>(accum + TL_ROWS * FNR_LOSS_SLOTS);
  unsigned* flag = cnt + 32 * 32 + 1;  // a non-finite contribution was seen (second word of the top counter's line)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nbl = (int)((R + 255) / 256);
  const int per = (int)((R + 3) / 4);
  const float inv3r = 1.0f / (float)(3 * R), invr = 1.0f / (float)R;
  if ((int)blockIdx.x < nbl) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    float l_rgb = 0.0f, l_sem = 0.0f;
    if (r < R) {  // per ray exactly what losses_block does
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float d = rgb[3 * r + c] - image[3 * r + c];
        l_rgb += d * d;
        if (d_rgb) d_rgb[3 * r + c] = mse_grad(d, inv3r);     // (NULL: the composite backward forms them itself)
      }
      const float x = sem[r], y = mask[r];
      l_sem = fmaxf(x, 0.0f) - x * y + log1pf(expf(-fabsf(x)));
      if (d_sem) d_sem[r] = bce_logit_grad(x, y, sem_weight, invr);
    }
    l_rgb = wave_sum(l_rgb);
    l_sem = wave_sum(l_sem);
    if (lane == 0) {
      // these two rows take raw sums over a wave's 64 rays (not divided by R yet), 4 nbl of them: the bound that keeps
      // their total below 2^28 (x 2^34 < 2^63) is 2^28 / waves — 4e6 per wave at 4096 rays
      const float wave_cap = 268435456.0f / (float)(4 * nbl);
      slot_add<true>(rgb_slots, blockIdx.x, wave, l_rgb, flag, wave_cap);
      slot_add<true>(sem_slots, blockIdx.x, wave, l_sem, flag, wave_cap);
    }
  } else {
    const int b = (int)blockIdx.x - nbl;
    const int role = b / per, local = b - role * per;
    if (role < lv.n_levels)
      interlevel_block<true, ME>(R, S_f, spacing_f, w_f, lv.S_p[role], lv.spacing_p[role], lv.w_p[role], mult, il_slots,
                                 lv.d_wp[role], local, lds, p_cap, lv.euclid_p[role], lv.density_p[role],
                                 lv.d_density_p[role], flag, role == lv.dist_host ? di_slots : nullptr);
    else
      distortion_block<true>(R, S_f, spacing_f, w_f, di_slots, local, lds, S_f, flag);
  }
  // Completion count WITHOUT __threadfence(): an agent-scope release fence writes the XCD's L2 back (this kernel's
  // outputs are dirty there) and 3000 workgroups doing that cost 100 us.  The slot sums are agent-scope atomics, performed
  // at the memory side; every wave waits until its own have been acknowledged (vmcnt(0)) before the workgroup's barrier,
  // then one thread counts the workgroup in, and the last workgroup reads the slots back with agent-scope loads.
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned g = blockIdx.x & 31u;
    const unsigned gsize = (gridDim.x - g + 31u) / 32u, ngroups = gridDim.x < 32u ? gridDim.x : 32u;
    bool last = false;
    if (atomicAdd(&cnt[g * 32], 1u) == gsize - 1u) last = atomicAdd(&cnt[32 * 32], 1u) == ngroups - 1u;
    s_last = last;
  }
  if (threadIdx.x < TL_ROWS) s_tot[threadIdx.x] = 0ull;
  __syncthreads();
  if (!s_last) return;
  // The rows hold 64-bit fixed point (slot_add<true>): integer sums, any order.  A row is 512 words of which slot_add uses
  // (block & 31) * 16 + wave, wave < 4: 128.  Two rows per thread, summed with LDS atomics (a handful of cycles against a
  // shuffle tree per row); thread 0 asks for the flag in the same trip to memory.
  const int word = ((threadIdx.x & 127) >> 2) * 16 + (threadIdx.x & 3), q0 = (threadIdx.x >> 7) * 2;
  unsigned bad_bits = 0u;
  if (threadIdx.x == 0) bad_bits = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int q = 0; q < 2; ++q)
    atomicAdd(&s_tot[q0 + q],
              __hip_atomic_load(reinterpret_cast<unsigned long long*>(accum + (q0 + q) * FNR_LOSS_SLOTS) + word,
                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  __syncthreads();
  // self-cleaning: this (last) workgroup has read every slot and every other workgroup is done, so the accumulator goes
  // back to zero here — a caller that keeps the buffer needs no fill launch before the next step
  for (int i = threadIdx.x; i < TL_ACCUM_FLOATS; i += 256) accum[i] = 0.0f;
  if (threadIdx.x == 0) {
    const bool bad = bad_bits != 0u;
    float t[TL_ROWS];
#pragma unroll
    for (int q = 0; q < TL_ROWS; ++q) t[q] = bad ? __builtin_nanf("") : (float)((double)(long long)s_tot[q] / TL_FIX_SCALE);
    const float mse = t[2] * inv3r;
    losses[0] = mse;
    losses[1] = sem_weight * t[3] * invr;
    losses[2] = -10.0f * log10f(mse);  // PeakSignalNoiseRatio(data_range=1.0) of the same batch (fruit_nerf.py:398)
    losses[3] = t[0];
    losses[4] = want_distortion ? t[1] : 0.0f;
  }
}

}  // namespace fnr

using namespace fnr;

extern "C" int fnr_losses_fwd(int64_t n_rays, const float* rgb, const float* image, const float* semantics,
                              const float* fruit_mask, float semantic_loss_weight, float* losses, float* d_rgb,
                              float* d_semantics, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_losses_fwd");
  FNR_CHECK_ARG(rgb && image && semantics && fruit_mask && losses && d_rgb && d_semantics && n_rays > 0,
                "losses_fwd: null argument");
  FNR_PROF(OP_LOSSES, n_rays);
  hipLaunchKernelGGL(k_losses, dim3(1), dim3(1024), 0, as_stream(stream), (long long)n_rays, rgb, image,
                     semantics, fruit_mask, semantic_loss_weight, losses, d_rgb, d_semantics);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

extern "C" int fnr_interlevel_fwd(int64_t n_rays, int S_f, const float* spacing_f, const float* weights_f, int S_p,
                                  const float* spacing_p, const float* weights_p, float mult, float* loss,
                                  float* d_weights_p, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_interlevel_fwd");
  FNR_CHECK_ARG(spacing_f && weights_f && spacing_p && weights_p && loss && d_weights_p, "interlevel_fwd: null argument");
  FNR_CHECK_ARG(S_f > 0 && S_p > 0 && S_p <= IL_MAX_P, "interlevel_fwd: S_p %d out of range", S_p);
  if (n_rays == 0) return FNR_OK;
  FNR_PROF(OP_INTERLEVEL, n_rays * (long long)S_p);
  hipLaunchKernelGGL(k_interlevel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, as_stream(stream),
                     (long long)n_rays, S_f, spacing_f, weights_f, S_p, spacing_p, weights_p, mult, loss, d_weights_p);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

extern "C" int fnr_distortion(int64_t n_rays, int S, const float* spacing, const float* weights, float* out,
                              void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_distortion");
  FNR_CHECK_ARG(spacing && weights && out && S > 0 && S <= 512, "distortion: bad argument");
  if (n_rays == 0) return FNR_OK;
  FNR_PROF(OP_DISTORTION, n_rays * (long long)S);
  hipLaunchKernelGGL(k_distortion, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, as_stream(stream),
                     (long long)n_rays, S, spacing, weights, out);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

extern "C" int fnr_train_losses(int64_t n_rays, const float* rgb, const float* image, const float* semantics,
                                const float* fruit_mask, float semantic_loss_weight, float* d_rgb, float* d_semantics,
                                int S_f, const float* spacing_f, const float* weights_f, int n_levels, const int* S_p,
                                const float* const* spacing_p, const float* const* weights_p, float* const* d_weights_p,
                                const float* const* euclid_p, const float* const* density_p,
                                float* const* d_density_p, float interlevel_mult, int want_distortion, float* accum,
                                float* losses, void* stream) {
  constexpr int M = FNR_MAX_PROPOSAL_LEVELS;
  FNR_SEQ_RECORD(fnr_train_losses, n_rays, rgb, image, semantics, fruit_mask, semantic_loss_weight, d_rgb, d_semantics, S_f,
                 spacing_f, weights_f, n_levels, seq::host_array<M>(S_p, n_levels), seq::host_array<M>(spacing_p, n_levels),
                 seq::host_array<M>(weights_p, n_levels), seq::host_array<M>(d_weights_p, n_levels),
                 seq::host_array<M>(euclid_p, n_levels), seq::host_array<M>(density_p, n_levels),
                 seq::host_array<M>(d_density_p, n_levels), interlevel_mult, want_distortion, accum, seq::Losses{losses},
                 stream);
  FNR_CHECK_ARG(rgb && image && semantics && fruit_mask && spacing_f && weights_f && accum && losses && n_rays > 0,
                "train_losses: null argument");
  FNR_CHECK_ARG((d_rgb == nullptr) == (d_semantics == nullptr), "train_losses: d_rgb and d_semantics go together");
  FNR_CHECK_ARG(n_levels >= 0 && n_levels <= FNR_MAX_PROPOSAL_LEVELS, "train_losses: %d proposal levels (0..%d)",
                n_levels, FNR_MAX_PROPOSAL_LEVELS);
  FNR_CHECK_ARG(S_f > 0 && (!want_distortion || S_f <= 512), "train_losses: S_f %d out of range", S_f);
  LevelLossArgs lv{};
  lv.n_levels = n_levels;
  for (int l = 0; l < n_levels; ++l) {
    FNR_CHECK_ARG(S_p && spacing_p && weights_p && spacing_p[l] && weights_p[l], "train_losses: null proposal level %d", l);
    FNR_CHECK_ARG(S_p[l] > 0 && S_p[l] <= IL_MAX_P, "train_losses: S_p %d out of range", S_p[l]);
    lv.S_p[l] = S_p[l], lv.spacing_p[l] = spacing_p[l], lv.w_p[l] = weights_p[l];
    lv.d_wp[l] = d_weights_p ? d_weights_p[l] : nullptr;
    lv.d_density_p[l] = d_density_p ? d_density_p[l] : nullptr;
    if (lv.d_density_p[l]) {
      FNR_CHECK_ARG(euclid_p && density_p && euclid_p[l] && density_p[l],
                    "train_losses: level %d: d_density_p needs euclid_p and density_p", l);
      lv.euclid_p[l] = euclid_p[l], lv.density_p[l] = density_p[l];
    } else {
      FNR_CHECK_ARG(lv.d_wp[l], "train_losses: level %d: neither d_weights_p nor d_density_p", l);
    }
  }
  int p_cap = 1;
  for (int l = 0; l < n_levels; ++l) p_cap = S_p[l] > p_cap ? S_p[l] : p_cap;
  lv.dist_host = -1;
  if (want_distortion && n_levels > 0 && 2ll * S_f <= 3ll * p_cap + 4) {
    lv.dist_host = 0;
    for (int l = 1; l < n_levels; ++l)
      if (S_p[l] < S_p[lv.dist_host]) lv.dist_host = l;
  }
  const bool distortion_role = want_distortion && lv.dist_host < 0;
  const long long per = (n_rays + 3) / 4;
  const long long blocks = (n_rays + 255) / 256 + per * (n_levels + (distortion_role ? 1 : 0));
  FNR_CHECK_ARG(blocks < (1ll << 31), "train_losses: too many rays");
  FNR_PROF(OP_LOSSES, n_rays);
  size_t lds_floats = 4 * (size_t)(3 * p_cap + 4);
  if (distortion_role && (size_t)8 * S_f > lds_floats) lds_floats = (size_t)8 * S_f;
  // (no one-wide form: two samples per lane fit the 64 registers of eight workgroups per CU already)
  auto kernel = p_cap <= 128 ? k_train_losses<2> : p_cap <= 256 ? k_train_losses<4> : k_train_losses<WB_MAXE>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds_floats * sizeof(float), as_stream(stream),
                     (long long)n_rays, rgb, image, semantics, fruit_mask, semantic_loss_weight, d_rgb, d_semantics, S_f,
                     spacing_f, weights_f, lv, interlevel_mult, want_distortion, accum, losses, p_cap);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}
