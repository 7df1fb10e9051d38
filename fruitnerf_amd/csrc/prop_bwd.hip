// prop_bwd.hip — backward of the proposal networks (autograd of HashMLPDensityField) for gfx950: k_prop_bwd, the weights'
// reduction k_prop_reduce, and the binned scatter of the feature gradients into the hash table (hash_scatter.hpp).
#include <stdlib.h>

#include "hash_scatter.hpp"
#include "sequencer.hpp"

namespace fnr {

// ------------------------------------------------------------------------------------------------
// proposal network backward.  Persistent workgroups; per iteration 256 samples:
//   phase 1 (thread = sample): recompute the MLP from the saved features, d_out = d_sigma * trunc_exp'(out),
//            hidden gradients -> LDS, feature gradients -> d_feats [L][N][2] (scattered by binned_scatter);
//   phase 2 (wave = 64 of the samples): dW0 = dh^T f, db0 = dh^T 1 and dW1 = (relu(h) d_out)^T 1 as 16x16x4 fp32 MFMAs
//            with the samples on the K axis (3 MFMAs per 4 samples; operands are single conflict-light LDS
//            reads).  A thread-per-weight loop over the 256 samples read two LDS words per FMA and was LDS-bound
//            (~45 us of the 73 us this kernel took for 1 M samples).
// Weight gradients leave the workgroup once, at the end (one partial vector per workgroup, summed by k_prop_reduce).
//
// Where things live (profiles/prop_bwd_diet.md):
//   * the 16 (2L + 1) + 17 weights sit in LDS and are read as uniform-address broadcasts next to the FMAs that use them.  As
//     uniform global reads the compiler wanted them in ~100 scalar registers, parked 302 of them in lanes of vector registers
//     (a fifth of the loop was v_readlane) and fetched them through 158 scalar loads behind 122 waits on every launch.
//     Every wave stores the WHOLE copy — the same values to the same words — and waits for its own stores: whichever store
//     a later read sees, it sees the weight.  No workgroup barrier.
//   * phase 2 of a wave reads only the 64 rows its own lanes wrote in phase 1 (row0 = 64 wave + g), so the two phases are
//     ordered by wave_lds_fence(), in both directions (the next pass's writes come behind this pass's reads in the wave's
//     in-order LDS queue).  Only the epilogue, which reuses s_dh across waves, has workgroup barriers: one in front of it
//     (waves arrive at different times), one behind its writes.
//   * the next pass's inputs (saved features, d_density, the ray) are loaded at the top of this pass and are in flight
//     while it computes.  The position gradient's 8 L corner rows stay behind the MLP: gathered ahead of it they do not fit
//     the 168 registers of three waves per SIMD (__launch_bounds__(256, 3): without the bound the scheduler took 256).
// Every per-sample expression, the order in which a wave's MFMA accumulators take its samples, the per-thread db1 sum and
// the (w0 + w1) + (w2 + w3) combination are what they were: tests/test_gpu_prop_bwd_same_bits.py.
// ------------------------------------------------------------------------------------------------
constexpr int PROP_PART = 320;   // floats per workgroup partial: dW0 tile 256 + dW1 16 + db0 16 + db1 (+ pad)

// this wave's LDS traffic so far is done before anything behind this line starts (field_mlp_bwd.hip has the same)
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// what one sample of a pass reads from global memory, as loaded (zeros beyond N: such a sample contributes nothing)
template <int L>
struct PropInputs {
  float2 f[L];
  float dd, o[3], d[3], t0, t1;
};
template <int L>
__device__ __forceinline__ void prop_load(PropInputs<L>& in, const RaySource& src, long long n, long long N,
                                          const float2* __restrict__ feat_save, const float* __restrict__ d_density) {
#pragma unroll
  for (int l = 0; l < L; ++l) in.f[l] = make_float2(0.0f, 0.0f);
  in.dd = in.t0 = in.t1 = 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) in.o[a] = in.d[a] = 0.0f;
  if (n < N) {
    const long long r = n / src.S;   // (RaySource::position's addresses)
    const int k = (int)(n - r * src.S);
    const float* b = src.euclid + r * (src.S + 1) + k;
    in.t0 = b[0];
    in.t1 = b[1];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      in.o[a] = src.rays.origins[3 * r + a];
      in.d[a] = src.rays.directions[3 * r + a];
    }
#pragma unroll
    for (int l = 0; l < L; ++l) in.f[l] = ntc_load<NT_PROP_FEATS>(&feat_save[(size_t)l * N + n]);
    in.dd = d_density[n];
  }
}

template <int L, int H, bool POSGRAD>
__global__ __launch_bounds__(256, 3) void k_prop_bwd(GridDev grid, float4* __restrict__ d_xw, Warp warp, RaySource src,
                                                  long long N, const float* __restrict__ w0,
                                                  const float* __restrict__ b0, const float* __restrict__ w1,
                                                  const float* __restrict__ b1, const float2* __restrict__ feat_save,
                                                  const float* __restrict__ d_density, float2* __restrict__ d_feats,
                                                  float* __restrict__ partials) {
  constexpr int K = 2 * L;
  __shared__ float s_dh[256][H + 1];   // d hidden (pre-activation)
  __shared__ float s_ha[256][H + 1];   // relu(hidden) * d_out  (for dW1)
  __shared__ float s_f[256][K + 1];    // input features
  constexpr int W0 = 0, B0 = H * K, W1 = B0 + H, B1 = W1 + H, NW = B1 + 1;   // the weights' copy: w0 [H][K] | b0 | w1 | b1
  __shared__ __attribute__((aligned(16))) float s_w[(NW + 3) / 4 * 4];
  __shared__ float s_db1[4];           // the waves' db1 sums
  static_assert(H == 16 && K <= 16, "phase 2 is a single 16x16 MFMA tile");
  using f32x4 = __attribute__((ext_vector_type(4))) float;
  const int tid0 = threadIdx.x;
  // accumulators (C layout: lane holds column j, rows 4 g + r): dW0[o][k = j], db0[o] in column 0 of d3,
  // dW1[o] in column 0 of d2; db1 per thread
  f32x4 d1 = {0.f, 0.f, 0.f, 0.f}, d2 = {0.f, 0.f, 0.f, 0.f}, d3 = {0.f, 0.f, 0.f, 0.f};
  float db1 = 0.0f;
  const long long n_iter = (N + 255) / 256;
#pragma unroll
  for (int i = tid0 & 63; i < NW; i += 64) s_w[i] = i < B0 ? w0[i] : i < W1 ? b0[i - B0] : i < B1 ? w1[i - W1] : b1[0];
  PropInputs<L> in;
  prop_load(in, src, (long long)blockIdx.x * 256 + tid0, N, feat_save, d_density);
  wave_lds_fence();
  for (long long it = blockIdx.x; it < n_iter; it += gridDim.x) {
    asm volatile("" ::: "memory");   // the weights are loop-invariant LDS reads: keep them inside the loop (field_mlp.hip)
    // ... and what hangs on the thread id: an opaque copy makes the LDS row addresses per-use VALU ops, not registers held
    // across the pass (field_mlp_bwd.hip)
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const float ones_col0 = (j == 0) ? 1.0f : 0.0f;  // B operand that sums over the samples into column 0
    // ... and on N and the table size: 2 L + L per-level base addresses are scalar arithmetic per pass, not scalar registers
    // held across it (the position-gradient forms ran out of them)
    long long Ns = N;
    int log2_T = grid.log2_T;
    asm volatile("" : "+s"(Ns), "+s"(log2_T));
    const long long n = it * 256 + tid;
    float f[K], dout = 0.0f;
#pragma unroll
    for (int l = 0; l < L; ++l) {
      f[2 * l] = in.f[l].x;
      f[2 * l + 1] = in.f[l].y;
    }
    bool sel = false;
    float x[3] = {0.f, 0.f, 0.f};
    if (n < N) {
      float px, py, pz;
      ray_position(in.o, in.d, in.t0, in.t1, px, py, pz);
      sel = warp_position(warp, px, py, pz, x);
    }
    const float dd = in.dd;
    // the next pass's inputs, in flight behind this pass's work (none beyond the last pass: n >= N there)
    prop_load(in, src, n + gridDim.x * 256ll, Ns, feat_save, d_density);
    float a[H];
    float out = s_w[B1];
#pragma unroll
    for (int o = 0; o < H; ++o) {
      float t = s_w[B0 + o];
#pragma unroll
      for (int k = 0; k < K; ++k) t = fmaf(s_w[W0 + o * K + k], f[k], t);
      a[o] = t;
      out = fmaf(s_w[W1 + o], fmaxf(t, 0.0f), out);
    }
    __builtin_amdgcn_sched_barrier(0);   // phase boundaries for the scheduler (here and behind df): register pressure stays local
    if (n < N && sel) dout = dd * expf(fminf(fmaxf(out, -15.0f), 15.0f));  // trunc_exp backward
    asm volatile("" ::: "memory");   // (read w0 again below, not 16 K registers held from above)
    float df[K];
#pragma unroll
    for (int k = 0; k < K; ++k) df[k] = 0.0f;
#pragma unroll
    for (int o = 0; o < H; ++o) {
      const float dh = (a[o] > 0.0f) ? dout * s_w[W1 + o] : 0.0f;
      s_dh[tid][o] = dh;
      s_ha[tid][o] = fmaxf(a[o], 0.0f) * dout;
#pragma unroll
      for (int k = 0; k < K; ++k) df[k] = fmaf(dh, s_w[W0 + o * K + k], df[k]);
    }
    __builtin_amdgcn_sched_barrier(0);
    // df is formed HERE, by every lane: its only readers sit behind `n < N`, and the compiler sank the 16 K FMAs there and held
    // all of w0 in registers for them (the loads do not sink past the stores above)
#pragma unroll
    for (int k = 0; k < K; ++k) asm volatile("" : "+v"(df[k]));
#pragma unroll
    for (int k = 0; k < K; ++k) s_f[tid][k] = f[k];
    db1 += dout;
    if (n < N) {
#pragma unroll
      for (int l = 0; l < L; ++l) ntc_store<NT_PROP_DFEATS_ST>(&d_feats[(size_t)l * Ns + n], make_float2(df[2 * l], df[2 * l + 1]));
    }
    if constexpr (POSGRAD) {
      // gradient w.r.t. the unit-cube position (camera-pose optimisation): re-gather the corner rows of every level
      // and contract with d(blend weights)/d(offset) (position_grad.hip has the main-field version)
      if (n < N) {
        const uint32_t hmask = (1u << log2_T) - 1u;
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
#pragma unroll
        for (int l = 0; l < L; ++l) {
          int scaling = grid.scalings[l];
          asm volatile("" : "+s"(scaling));   // (float)scaling formed here, not eight vector registers held across the loop
          const GridLevel gl = grid_cell(x, scaling);
          uint32_t hh[8];
          grid_corners(gl, hmask, hh);
          const float2* lt = grid.table + ((size_t)l << log2_T);
          float dk[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float2 v = lt[hh[k]];
            dk[k] = fmaf(df[2 * l], v.x, df[2 * l + 1] * v.y);
          }
          const float ox = gl.o[0], oy = gl.o[1], oz = gl.o[2];
          const float mx = 1.0f - ox, my = 1.0f - oy, mz = 1.0f - oz;
          const float s = sel ? (float)scaling : 0.0f;
          gx += s * (oz * (oy * (dk[0] - dk[3]) + my * (dk[1] - dk[2])) + mz * (oy * (dk[4] - dk[7]) + my * (dk[5] - dk[6])));
          gy += s * (oz * (ox * (dk[0] - dk[1]) + mx * (dk[3] - dk[2])) + mz * (ox * (dk[4] - dk[5]) + mx * (dk[7] - dk[6])));
          gz += s * (oy * (ox * (dk[0] - dk[4]) + mx * (dk[3] - dk[7])) + my * (ox * (dk[1] - dk[5]) + mx * (dk[2] - dk[6])));
          // L > 5: the gathers in two groups of at most four levels (all 16 L rows in flight at once do not fit 168 registers)
          if (L > 5 && l + 1 == (L + 1) / 2) __builtin_amdgcn_sched_barrier(0);
        }
        d_xw[n] = make_float4(gx, gy, gz, 0.0f);
      }
    }
    wave_lds_fence();   // this wave's rows are written
    // phase 2: this wave's 64 samples, 4 per MFMA step.  A[i = o][kk] = dh / ha of sample 4 step + kk,
    // B[kk][j = k] = feature k of that sample (0 beyond K)
    const int row0 = 64 * wave + g;
#pragma unroll 4
    for (int st = 0; st < 16; ++st) {
      const int row = row0 + 4 * st;
      const float a1 = s_dh[row][j], a2 = s_ha[row][j];
      const float bf = (j < K) ? s_f[row][j < K ? j : 0] : 0.0f;
      d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bf, d1, 0, 0, 0);
      d2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, ones_col0, d2, 0, 0, 0);
      d3 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, ones_col0, d3, 0, 0, 0);
    }
    wave_lds_fence();   // ... and read: the next pass may overwrite them
  }
  // combine the 4 waves through LDS (reusing s_dh: rows of EVERY wave, so all of them must have left the loop)
  __syncthreads();
  int tid = tid0;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, g = lane >> 4;
  float* red = &s_dh[0][0];  // [4 waves][3][16 rows][16 cols]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[((wave * 3 + 0) * 16 + 4 * g + r) * 16 + j] = d1[r];
    red[((wave * 3 + 1) * 16 + 4 * g + r) * 16 + j] = d2[r];
    red[((wave * 3 + 2) * 16 + 4 * g + r) * 16 + j] = d3[r];
  }
  db1 = wave_sum(db1);
  if (lane == 0) s_db1[wave] = db1;
  __syncthreads();
  {
    // one partial vector per workgroup: [dW0 16x16 | dW1 16 | db0 16 | db1], summed by k_prop_reduce.  Atomics
    // from 768 workgroups onto the same 13 cache lines of the gradient serialised in L2 (~34 us per call).
    const int o = tid >> 4, k = tid & 15;  // 256 threads = the 16 x 16 tile
    auto total = [&](int which) {
      return (red[((0 * 3 + which) * 16 + o) * 16 + k] + red[((1 * 3 + which) * 16 + o) * 16 + k]) +
             (red[((2 * 3 + which) * 16 + o) * 16 + k] + red[((3 * 3 + which) * 16 + o) * 16 + k]);
    };
    float* part = partials + (size_t)blockIdx.x * PROP_PART;
    part[tid] = total(0);
    if (k == 0) {
      part[256 + o] = total(1);
      part[272 + o] = total(2);
    }
    if (tid == 0) part[288] = (s_db1[0] + s_db1[1]) + (s_db1[2] + s_db1[3]);
  }
}

// gradient += sum over workgroups of their partial vectors, in a FIXED order with one writer per entry (no float
// atomics: bit-reproducible training).  Workgroup = PRD_E entries x PRD_Y slices: slice y sums rows y, y + PRD_Y, ... (a
// few hundred rows: two or three batches of 8 independent loads per thread), the slices meet in LDS and the thread of
// slice 0 adds them up in slice order.
// ADAM (fnr_prop_density_bwd_adam): the owning thread also takes the parameter's optimiser step (weight_adam_entry).
constexpr int PRD_E = 16, PRD_Y = 64;
struct PropReduceArgs {
  const float* partials;
  int nblocks, K;
  float *g_w0, *g_b0, *g_w1, *g_b1;
  WeightAdam wa;
};
template <bool ADAM>
__device__ __forceinline__ void prop_reduce_block(int block, const PropReduceArgs& a) {
  __shared__ float s_part[PRD_Y][PRD_E];
  const float* __restrict__ partials = a.partials;
  const int nblocks = a.nblocks, K = a.K;
  const int t = threadIdx.x % PRD_E, y = threadIdx.x / PRD_E;
  const int e = block * PRD_E + t;
  float s = 0.0f;
  if (e <= 288) {
    int b = y;
    for (; b + 7 * PRD_Y < nblocks; b += 8 * PRD_Y) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = partials[(size_t)(b + u * PRD_Y) * PROP_PART + e];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; b < nblocks; b += PRD_Y) s += partials[(size_t)b * PROP_PART + e];
  }
  s_part[y][t] = s;
  __syncthreads();
  if (y != 0 || e > 288) return;
#pragma unroll 8
  for (int q = 1; q < PRD_Y; ++q) s += s_part[q][t];
  if (!ADAM && s == 0.0f) return;
  float* dst = nullptr;
  if (e < 256) {
    const int o = e >> 4, k = e & 15;
    if (k < K) dst = &a.g_w0[o * K + k];
  } else if (e < 272) {
    dst = &a.g_w1[e - 256];
  } else if (e < 288) {
    dst = &a.g_b0[e - 272];
  } else {
    dst = &a.g_b1[0];
  }
  if (!dst) return;
  if constexpr (ADAM) weight_adam_entry(a.wa, dst, s);
  else *dst += s;
}
template <bool ADAM>
__global__ __launch_bounds__(PRD_E * PRD_Y) void k_prop_reduce(PropReduceArgs a) {
  prop_reduce_block<ADAM>((int)blockIdx.x, a);
}
// both proposal levels' weight reductions as one launch (fnr_prop_density_bwd_pair_split: level 1's MLP backward no longer
// waits for level 0's reduction to start and drain; same sums in the same order by the same single writers)
template <bool ADAM>
__global__ __launch_bounds__(PRD_E * PRD_Y) void k_prop_reduce2(PropReduceArgs a, PropReduceArgs b) {
  constexpr int NB = PROP_PART / PRD_E;
  if ((int)blockIdx.x < NB) prop_reduce_block<ADAM>((int)blockIdx.x, a);
  else prop_reduce_block<ADAM>((int)blockIdx.x - NB, b);
}

// ---- host side: one description per level, two steps (MLP backward, emit), four exports that compose them -------------------
// One level's backward as an export was given it (fnr_prop_density_bwd's arguments); checked once, by prop_level_check.
struct PropLevel {
  const fnr_prop_net *net, *grads;
  const fnr_warp* warp;
  const float* euclid;
  int S;
  const float *feat_save, *d_density;
  float* d_position;
  void* workspace;   // d_feats [L][N][2] | one partial vector per workgroup | the scatter's workspace
  size_t workspace_bytes;
  int workspace_clean;
  const fnr_table_adam* table_adam;   // null: the gradients are left in `grads`
  long long N;                        // rays x S, and the device forms of the optimiser descriptors: set by prop_level_check
  TableAdam ta{};
  WeightAdam wa{};
};

static size_t prop_dfeat_bytes(int L, long long N) { return ((size_t)L * (size_t)N * sizeof(float2) + 255) / 256 * 256; }
static size_t prop_partial_bytes() { return (size_t)3 * device_cu_count() * PROP_PART * sizeof(float); }   // 3 workgroups per CU

// (`who`: the export that was called)
static int prop_level_check(const char* who, PropLevel& lv, const fnr_rays* rays, const fnr_table_adam* weight_adam,
                            const float* grad_arena) {
  FNR_CHECK_ARG(lv.net && lv.grads && lv.warp && rays && lv.euclid && lv.feat_save && lv.d_density && lv.workspace && lv.S > 0,
                "%s: null argument", who);
  if (lv.table_adam) {
    FNR_CHECK_ARG(weight_adam && grad_arena, "%s: weight_adam / grad_arena missing", who);
    int rc = make_table_adam(weight_adam, lv.wa.t);
    if (rc) return rc;
    lv.wa.p_off = weight_adam->params - grad_arena;
    lv.wa.m_off = weight_adam->exp_avg - grad_arena;
    lv.wa.v_off = weight_adam->exp_avg_sq - grad_arena;
    rc = make_table_adam(lv.table_adam, lv.ta);
    if (rc) return rc;
  }
  FNR_UNSUPPORTED(lv.net->hidden_dim == 16, "%s: hidden_dim %d not built (16 only)", who, lv.net->hidden_dim);
  FNR_CHECK_ARG(lv.grads->grid.table && lv.grads->w0 && lv.grads->b0 && lv.grads->w1 && lv.grads->b1,
                "%s: null gradient pointer", who);
  lv.N = rays->n_rays * (long long)lv.S;
  if (lv.N == 0) return FNR_OK;   // (nothing will be launched)
  const int L = lv.net->grid.n_levels;
  FNR_UNSUPPORTED(L >= 1 && L <= 8, "%s: n_levels %d not built (1..8)", who, L);
  FNR_CHECK_ARG(lv.workspace_bytes >= fnr_prop_density_bwd_workspace_bytes(lv.N, L, lv.net->grid.log2_hashmap_size),
                "%s: workspace too small", who);
  return FNR_OK;
}

// Step 1, the MLP backward of one level: k_prop_bwd -> what the weight reduction needs (d_position is final behind it)
static int prop_mlp_bwd(const PropLevel& lv, const fnr_rays* rays, hipStream_t st, PropReduceArgs& red) {
  const int L = lv.net->grid.n_levels;
  // Persistent workgroups, at most the three a CU holds.  A/B knob (round 5): FNR_PROP_BWD_WGS_PER_CU = 1 | 2 caps them
  // below that.  On a second stream the kernel fills every CU for its whole 75 - 140 us and the launch stream's short kernels
  // wait for it to END (kernel trace of the two-stream step, profiles/r04_raw/prof_step_timeline_two_streams.txt:
  // k_color_ray_grads 11 -> 75 us, the base backward 50 -> 95 us next to it); with fewer resident workgroups it runs
  // longer itself but leaves wave slots and LDS to the other queue.  Same partial sums per workgroup, summed by
  // k_prop_reduce in workgroup order: the weight gradients change in the last bits with the workgroup count.
  static const int cap_per_cu = [] { const char* e = getenv("FNR_PROP_BWD_WGS_PER_CU"); const int v = e ? atoi(e) : 0; return (v >= 1 && v <= 3) ? v : 3; }();
  const long long capped = (long long)cap_per_cu * device_cu_count();
  const long long blocks = (lv.N + 255) / 256 < capped ? (lv.N + 255) / 256 : capped;
  float2* d_feats = reinterpret_cast<float2*>(lv.workspace);
  float* partials = reinterpret_cast<float*>(reinterpret_cast<char*>(lv.workspace) + prop_dfeat_bytes(L, lv.N));
  float4* d_xw = reinterpret_cast<float4*>(lv.d_position);
  decltype(&k_prop_bwd<1, 16, true>) kernel = nullptr;
  switch (L) {
#define FNR_PROPB_CASE(LL) case LL: kernel = d_xw ? k_prop_bwd<LL, 16, true> : k_prop_bwd<LL, 16, false>; break;
    FNR_PROPB_CASE(1) FNR_PROPB_CASE(2) FNR_PROPB_CASE(3) FNR_PROPB_CASE(4)
    FNR_PROPB_CASE(5) FNR_PROPB_CASE(6) FNR_PROPB_CASE(7) FNR_PROPB_CASE(8)
#undef FNR_PROPB_CASE
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, make_grid(&lv.net->grid), d_xw, make_warp(lv.warp),
                     RaySource{make_rays(rays), lv.euclid, lv.S}, lv.N, lv.net->w0, lv.net->b0, lv.net->w1, lv.net->b1,
                     reinterpret_cast<const float2*>(lv.feat_save), lv.d_density, d_feats, partials);
  FNR_LAUNCH_CHECK();
  red = PropReduceArgs{partials, (int)blocks, 2 * L, lv.grads->w0, lv.grads->b0, lv.grads->w1, lv.grads->b1, lv.wa};
  return FNR_OK;
}

static int prop_reduce(const PropReduceArgs& red, bool adam, hipStream_t st) {
  hipLaunchKernelGGL((adam ? k_prop_reduce<true> : k_prop_reduce<false>), dim3(PROP_PART / PRD_E), dim3(PRD_E * PRD_Y), 0, st, red);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

// Step 2, the emit of one level: d_feats -> the record queues of the level's table -> what the accumulate launch needs
static int prop_emit(const PropLevel& lv, const fnr_rays* rays, hipStream_t st, AccArgs& acc) {
  const int L = lv.net->grid.n_levels;
  const size_t used = prop_dfeat_bytes(L, lv.N) + prop_partial_bytes();   // d_feats and the partial vectors come first
  const int rc = scatter_emit(&lv.grads->grid, make_warp(lv.warp), RaySource{make_rays(rays), lv.euclid, lv.S}, lv.N,
                              reinterpret_cast<const float2*>(lv.workspace), 0, L, reinterpret_cast<char*>(lv.workspace) + used,
                              lv.workspace_bytes - used, lv.workspace_clean, st, lv.table_adam ? &lv.ta : nullptr, acc);
  acc.kind = 1;
  return rc;
}

// fnr_prop_density_bwd(_adam): MLP backward, weight reduction, emit, accumulate
static int prop_single(const char* who, PropLevel lv, const fnr_rays* rays, const fnr_table_adam* weight_adam,
                       const float* grad_arena, void* stream) {
  int rc = prop_level_check(who, lv, rays, weight_adam, grad_arena);
  if (rc || lv.N == 0) return rc;
  FNR_PROF(OP_PROP_BWD, lv.N);
  const hipStream_t st = as_stream(stream);
  const bool adam = lv.table_adam != nullptr;
  PropReduceArgs red;
  AccArgs acc;
  if ((rc = prop_mlp_bwd(lv, rays, st, red)) || (rc = prop_reduce(red, adam, st)) || (rc = prop_emit(lv, rays, st, acc))) return rc;
  return scatter_accumulate(acc, adam, st);
}

// A per-level array of the paired exports, as a step program keeps it (sequencer.hpp): the replay patches the optimiser
// descriptors among them from its scalars.
template <class T>
static auto both(const T* per_level) {
  return seq::host_array<2>(per_level, 2);
}

// What the paired exports share behind their recording hooks: the checks of the pair and, if there are rays, of its levels -> lv.
static int pair_begin(const char* name, PropLevel (&lv)[2], const fnr_prop_net* const* nets, const fnr_prop_net* const* grads,
                      const fnr_warp* const* warps, const fnr_rays* rays, const float* const* euclid_bins, const int* S,
                      const float* const* feat_save, const float* const* d_density, float* const* d_position,
                      const fnr_table_adam* const* table_adam, const fnr_table_adam* weight_adam, const float* grad_arena,
                      void* const* workspace, const size_t* workspace_bytes, const int* workspace_clean) {
  const char* who = name + 4;   // the messages name the export without its prefix
  FNR_CHECK_ARG(nets && grads && warps && rays && euclid_bins && S && feat_save && d_density && d_position && workspace &&
                    workspace_bytes && workspace_clean,
                "%s: null argument", who);
  FNR_CHECK_ARG(nets[0] != nets[1] && grads[0] != grads[1] && workspace[0] != workspace[1],
                "%s: the two levels must have their own network, gradients and workspace", who);
  const bool adam = table_adam && table_adam[0] && table_adam[1];
  FNR_CHECK_ARG(adam || !(table_adam && (table_adam[0] || table_adam[1])), "%s: one table_adam missing", who);
  for (int q = 0; q < 2 && rays->n_rays != 0; ++q) {
    lv[q] = PropLevel{nets[q], grads[q], warps[q], euclid_bins[q], S[q], feat_save[q], d_density[q], d_position[q], workspace[q],
                      workspace_bytes[q], workspace_clean[q], adam ? table_adam[q] : nullptr};
    const int rc = prop_level_check(who, lv[q], rays, weight_adam, grad_arena);
    if (rc) return rc;
  }
  return FNR_OK;
}

// one accumulate launch over both levels' bins, the level with more samples per ray first
static int pair_accumulate(const PropLevel (&lv)[2], const AccArgs (&acc)[2], hipStream_t st) {
  const bool first_longer = lv[0].S >= lv[1].S;
  return scatter_accumulate2(first_longer ? acc[0] : acc[1], first_longer ? acc[1] : acc[0], lv[0].table_adam != nullptr, st);
}

}  // namespace fnr

using namespace fnr;

extern "C" size_t fnr_prop_density_bwd_workspace_bytes(int64_t n_samples, int n_levels, int log2_hashmap_size) {
  return prop_dfeat_bytes(n_levels, n_samples) + prop_partial_bytes() +
         fnr_hash_scatter_workspace_bytes(n_samples, n_levels, log2_hashmap_size);
}

extern "C" int fnr_prop_density_bwd(const fnr_prop_net* net, const fnr_prop_net* grads, const fnr_warp* warp,
                                    const fnr_rays* rays, const float* euclid_bins, int S, const float* feat_save,
                                    const float* d_density, float* d_position, void* workspace,
                                    size_t workspace_bytes, int workspace_clean, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_prop_density_bwd");
  return prop_single("prop_density_bwd", PropLevel{net, grads, warp, euclid_bins, S, feat_save, d_density, d_position, workspace,
                                                   workspace_bytes, workspace_clean, nullptr},
                     rays, nullptr, nullptr, stream);
}

extern "C" int fnr_prop_density_bwd_adam(const fnr_prop_net* net, const fnr_prop_net* grads, const fnr_warp* warp,
                                         const fnr_rays* rays, const float* euclid_bins, int S, const float* feat_save,
                                         const float* d_density, float* d_position, const fnr_table_adam* table_adam,
                                         const fnr_table_adam* weight_adam, const float* grad_arena, void* workspace,
                                         size_t workspace_bytes, int workspace_clean, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_prop_density_bwd_adam");
  FNR_CHECK_ARG(table_adam && weight_adam && grad_arena, "prop_density_bwd_adam: optimiser descriptors missing");
  return prop_single("prop_density_bwd_adam", PropLevel{net, grads, warp, euclid_bins, S, feat_save, d_density, d_position,
                                                        workspace, workspace_bytes, workspace_clean, table_adam},
                     rays, weight_adam, grad_arena, stream);
}

// Both proposal levels of a training step (two networks, two sets of samples) as one entry point: their MLP backward,
// weight reduction and emit launches run one after the other, their accumulate launches as ONE (k_scatter_accumulate2:
// 160 workgroups of 64 KiB each per level on 256 CUs — side by side instead of one after the other).  table_adam /
// weight_adam all NULL (gradients are left in `grads`) or all set (fnr_prop_density_bwd_adam semantics per network).
extern "C" int fnr_prop_density_bwd_pair(const fnr_prop_net* const* nets, const fnr_prop_net* const* grads,
                                         const fnr_warp* const* warps, const fnr_rays* rays,
                                         const float* const* euclid_bins, const int* S, const float* const* feat_save,
                                         const float* const* d_density, float* const* d_position,
                                         const fnr_table_adam* const* table_adam, const fnr_table_adam* weight_adam,
                                         const float* grad_arena, void* const* workspace, const size_t* workspace_bytes,
                                         const int* workspace_clean, void* stream) {
  PropLevel lv[2];
  FNR_SEQ_RECORD(fnr_prop_density_bwd_pair, both(nets), both(grads), both(warps), rays, both(euclid_bins), both(S),
                 both(feat_save), both(d_density), both(d_position), both(table_adam), seq::optional(weight_adam), grad_arena,
                 both(workspace), both(workspace_bytes), both(workspace_clean), stream);
  int rc = pair_begin("fnr_prop_density_bwd_pair", lv, nets, grads, warps, rays, euclid_bins, S, feat_save, d_density, d_position,
                      table_adam, weight_adam, grad_arena, workspace, workspace_bytes, workspace_clean);
  if (rc || rays->n_rays == 0) return rc;
  FNR_PROF(OP_PROP_BWD, rays->n_rays * ((long long)S[0] + (long long)S[1]));   // one scope: both levels + the joint accumulate
  const hipStream_t st = as_stream(stream);
  AccArgs acc[2];
  for (int q = 0; q < 2; ++q) {
    PropReduceArgs red;
    if ((rc = prop_mlp_bwd(lv[q], rays, st, red)) || (rc = prop_reduce(red, lv[q].table_adam != nullptr, st)) ||
        (rc = prop_emit(lv[q], rays, st, acc[q])))
      return rc;
  }
  return pair_accumulate(lv, acc, st);
}

// fnr_prop_density_bwd_pair with the launches in two groups: both levels' MLP backward + weight reduction first — after
// them d_position[0..1] are final and `position_ready_event` (a hipEvent_t, optional) is recorded on `stream` — then both
// levels' emit launches and the joint accumulate.  A caller with a second stream can finish the ray gradients and take
// the camera optimiser's step next to the ~210 us of scatter that follow.  Same launches, same results.
extern "C" int fnr_prop_density_bwd_pair_split(const fnr_prop_net* const* nets, const fnr_prop_net* const* grads,
                                               const fnr_warp* const* warps, const fnr_rays* rays,
                                               const float* const* euclid_bins, const int* S, const float* const* feat_save,
                                               const float* const* d_density, float* const* d_position,
                                               const fnr_table_adam* const* table_adam, const fnr_table_adam* weight_adam,
                                               const float* grad_arena, void* const* workspace, const size_t* workspace_bytes,
                                               const int* workspace_clean, void* stream, void* position_ready_event) {
  PropLevel lv[2];
  FNR_SEQ_RECORD(fnr_prop_density_bwd_pair_split, both(nets), both(grads), both(warps), rays, both(euclid_bins), both(S),
                 both(feat_save), both(d_density), both(d_position), both(table_adam), seq::optional(weight_adam), grad_arena,
                 both(workspace), both(workspace_bytes), both(workspace_clean), stream, position_ready_event);
  int rc = pair_begin("fnr_prop_density_bwd_pair_split", lv, nets, grads, warps, rays, euclid_bins, S, feat_save, d_density,
                      d_position, table_adam, weight_adam, grad_arena, workspace, workspace_bytes, workspace_clean);
  if (rc) return rc;
  const hipStream_t st = as_stream(stream);
  const hipEvent_t position_ready = reinterpret_cast<hipEvent_t>(position_ready_event);
  if (rays->n_rays == 0) {
    if (position_ready) FNR_HIP(hipEventRecord(position_ready, st));
    return FNR_OK;
  }
  FNR_PROF(OP_PROP_BWD, rays->n_rays * ((long long)S[0] + (long long)S[1]));   // one scope: both groups + the joint accumulate
  PropReduceArgs red[2];
  for (int q = 0; q < 2; ++q)
    if ((rc = prop_mlp_bwd(lv[q], rays, st, red[q]))) return rc;
  // d_position is final behind the two MLP backward launches; their weight reductions (+ optimiser steps) are ONE launch
  if (position_ready) FNR_HIP(hipEventRecord(position_ready, st));
  hipLaunchKernelGGL((lv[0].table_adam ? k_prop_reduce2<true> : k_prop_reduce2<false>), dim3(2 * (PROP_PART / PRD_E)),
                     dim3(PRD_E * PRD_Y), 0, st, red[0], red[1]);
  FNR_LAUNCH_CHECK();
  AccArgs acc[2];
  for (int q = 0; q < 2; ++q)
    if ((rc = prop_emit(lv[q], rays, st, acc[q]))) return rc;
  return pair_accumulate(lv, acc, st);
}
