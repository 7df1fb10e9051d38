// field_mlp_bf16.hip — FruitField's MLP stack, forward and backward, on the bf16 matrix pipe of gfx950
// (v_mfma_f32_16x16x32_bf16).  Two modes of fnr_field_net.mlp_mode, see field_bf16.hpp:
//   FNR_MLP_BF16X3 (3)  exact 3-way bf16 split of every fp32 operand (FruitField's default): 6 piece products per
//                       product in the forward pass and in the backward's forward recompute, 3 in dX / dW — fp32-grade
//                       results at 16/6 resp. 16/3 of the fp32-MFMA issue rate;
//   FNR_MLP_BF16   (1)  plain bf16 operands, fp32 accumulate — throughput mode, not parity grade.
// Same entry points, buffers and partial-gradient image as the fp32 kernels (field_mlp.hip, field_mlp_bwd_fp32.hip):
// the per-ray colour bias and the backward's per-ray and weight finish (k_color_ray_grads, k_finish_weights:
// field_mlp_bwd.hip, which also runs the backward's branches in order) are shared.
// Replaces the same reference code: fruit_field.py:132-166,187-281 and its autograd.
// This file: the forward pass of both shapes (one wave = one PAIR of 16-sample tiles sharing every LDS fragment) and the
// 128-wide semantic branch of `fruit_nerf_big`, forward and backward: one tile per wave, 8 waves = a 128-sample batch,
// weight streaming because its fragments exceed the LDS, COOPERATIVE dW (every 16 x 16 block of a layer's weight gradient
// owned by one wave over the batch).  Every other branch's backward is per-wave: field_mlp_bwd_pw.hip.
// That one backward kernel stays next to the forward kernels ON PURPOSE: what hipcc emits for a kernel of this file depends
// on which others the module holds (shared helper instantiations and dynamic-LDS symbol; the IR first differs after the
// inliner).  Without the backward kernel k_field_mlp_fwd_sem_big_bf16 becomes other code (170 instead of 208 registers at
// three pieces), without both k_field_mlp_fwd_bf16 of `fruit_nerf_big` does: splitting the file is a kernel change.
#include <type_traits>

#include "field_bf16.hpp"

namespace fnr {

// ---- segment lists ------------------------------------------------------------------------------------------------
template <class Cfg>
struct SegsFwdAll {  // every layer, forward only
  static constexpr int N = Cfg::NLAYERS;
  static constexpr int layer(int i) { return i; }
  static constexpr bool isT(int) { return false; }
};

template <class Cfg>
struct SegsFwdBaseColor {  // base + colour MLPs, forward only (`fruit_nerf_big`: its semantic branch is weight-streamed)
  static constexpr int N = 5;
  static constexpr int layer(int i) {
    return i == 0 ? Cfg::L_BASE0 : i == 1 ? Cfg::L_BASE1 : i == 2 ? Cfg::L_COL0 : i == 3 ? Cfg::L_COL1 : Cfg::L_COL2;
  }
  static constexpr bool isT(int) { return false; }
};

// the 16 x 2 hash features of sample nn as the single K-block of mlp_base layer 0 (slot (g, e): level 4 (e>>1) + g,
// feature e & 1 — the KM_HASH column map of field_layers.hpp with s = e)
__device__ __forceinline__ void load_hash_block(const float2* __restrict__ feats, long long N, long long nn, int g,
                                                f32x4 (&x0)[2]) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const float2 v = feats[(size_t)(4 * m + g) * N + nn];
    x0[m >> 1][2 * (m & 1)] = v.x;
    x0[m >> 1][2 * (m & 1) + 1] = v.y;
  }
}

template <int N>
__device__ __forceinline__ void relu2_(f32x4 (&a)[N], f32x4 (&b)[N]) {
  relu_(a);
  relu_(b);
}

// =====================================================================================================================
// forward
// =====================================================================================================================
// WITH_SEM: the `fruit_nerf` shape, every branch in this kernel.  !WITH_SEM: base + colour only (`fruit_nerf_big`, whose
// 128-wide semantic branch runs in k_field_mlp_fwd_sem_big_bf16 from the h this kernel saves).
template <class Cfg, int NS, int WAVES, bool WITH_SEM>
__global__ __launch_bounds__(64 * WAVES, WAVES / 4) void k_field_mlp_fwd_bf16(
    const float* __restrict__ packed, const __bf16* __restrict__ image, const float* __restrict__ ray_bias, RaysDev rays,
    int S, long long N, const float2* __restrict__ feats, const uint8_t* __restrict__ selector,
    float* __restrict__ density, float* __restrict__ rgb, float* __restrict__ logit, float* __restrict__ geo_out,
    float* __restrict__ h_buf) {
  constexpr int HB = Cfg::HB;
  static_assert(HB == 1 || HB == 2, "built shapes");
  static_assert(!WITH_SEM || (HB == 1 && Cfg::NSEM == 2), "all-in-one kernel: `fruit_nerf` shape");
  using Segs = typename std::conditional<WITH_SEM, SegsFwdAll<Cfg>, SegsFwdBaseColor<Cfg>>::type;
  using Lds = BfLds<Cfg, Segs, NS>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16x8* lds = reinterpret_cast<bf16x8*>(smem);
  float* bias = reinterpret_cast<float*>(smem + Lds::BYTES);  // Cfg::B_TOTAL floats, the fp32 image's bias block
  Lds::template stage<64 * WAVES>(lds, image);
  for (int i = threadIdx.x; i < Cfg::B_TOTAL; i += blockDim.x) bias[i] = packed[Cfg::W_TOTAL + i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const long long n_pairs = (N + 31) / 32;
  for (long long pr = (long long)blockIdx.x * WAVES + wave; pr < n_pairs; pr += (long long)gridDim.x * WAVES) {
    asm volatile("" ::: "memory");  // keep the LDS fragment reads inside the loop (field_mlp.hip)
    const long long na = pr * 32 + j, nb = na + 16;
    const bool va = na < N, vb = nb < N;
    const long long nna = va ? na : N - 1, nnb = vb ? nb : N - 1;
    const long long raya = nna / S, rayb = nnb / S;

    f32x4 ha[HB], hb[HB];
    {
      f32x4 xa[2], xb[2], a1a[4], a1b[4];
      load_hash_block(feats, N, nna, g, xa);
      load_hash_block(feats, N, nnb, g, xb);
      bf_layer<NS, 4, 2>(Lds::template seg<Cfg::L_BASE0, false>(lds), bias + Cfg::boff(Cfg::L_BASE0), xa, xb, a1a, a1b, lane);
      relu2_(a1a, a1b);
      bf_layer<NS, HB, 4>(Lds::template seg<Cfg::L_BASE1, false>(lds), bias + Cfg::boff(Cfg::L_BASE1), a1a, a1b, ha, hb, lane);
    }
    if constexpr (WITH_SEM) {  // semantic branch
      f32x4 s1a[4], s1b[4], s2a[4], s2b[4], hda[1], hdb[1];
      bf_layer<NS, 4, 1>(Lds::template seg<Cfg::L_SEM0, false>(lds), bias + Cfg::boff(Cfg::L_SEM0), ha, hb, s1a, s1b, lane);
      relu2_(s1a, s1b);
      bf_layer<NS, 4, 4>(Lds::template seg<Cfg::L_SEM1, false>(lds), bias + Cfg::boff(Cfg::L_SEM1), s1a, s1b, s2a, s2b, lane);
      bf_layer<NS, 1, 4>(Lds::template seg<Cfg::L_HEAD, false>(lds), bias + Cfg::boff(Cfg::L_HEAD), s2a, s2b, hda, hdb, lane);
      if (g == 0 && va) logit[na] = hda[0][0];
      if (g == 0 && vb) logit[nb] = hdb[0][0];
    }
    {  // colour branch; the ray-constant inputs of layer 0 arrive as the per-ray bias (fp32, k_color_ray_bias)
      f32x4 c1a[4], c1b[4], c2a[4], c2b[4], c3a[1], c3b[1];
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) {
        c1a[ob] = *reinterpret_cast<const f32x4*>(ray_bias + (size_t)raya * 64 + 16 * ob + 4 * g);
        c1b[ob] = *reinterpret_cast<const f32x4*>(ray_bias + (size_t)rayb * 64 + 16 * ob + 4 * g);
      }
      {
        bf16x8 xa[1][NS], xb[1][NS];   // h: one K-block of 32 holds both 16-wide blocks of the big shape
        bf_operand<NS, HB>(ha, xa);
        bf_operand<NS, HB>(hb, xb);
        bf_layer_acc<NS, 4, 1>(Lds::template seg<Cfg::L_COL0, false>(lds), xa, xb, c1a, c1b, lane);
      }
      relu2_(c1a, c1b);
      bf_layer<NS, 4, 4>(Lds::template seg<Cfg::L_COL1, false>(lds), bias + Cfg::boff(Cfg::L_COL1), c1a, c1b, c2a, c2b, lane);
      relu2_(c2a, c2b);
      bf_layer<NS, 1, 4>(Lds::template seg<Cfg::L_COL2, false>(lds), bias + Cfg::boff(Cfg::L_COL2), c2a, c2b, c3a, c3b, lane);
      auto finish = [&](long long n, bool valid, const f32x4 (&h)[HB], const f32x4 (&c3)[1]) {
        if (!valid) return;
#pragma unroll
        for (int b = 0; b < HB; ++b) {
          if (h_buf) *reinterpret_cast<f32x4*>(h_buf + (size_t)n * (16 * HB) + 16 * b + 4 * g) = h[b];
          if (geo_out) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int k = 16 * b + 4 * g + r;
              if (k >= 1 && k <= Cfg::GEO) geo_out[(size_t)n * Cfg::GEO + (k - 1)] = h[b][r];
            }
          }
        }
        if (g == 0) {
          const bool sel = selector ? (selector[n] != 0) : true;
          density[n] = sel ? expf(h[0][0]) : 0.0f;  // trunc_exp forward * selector (fruit_field.py:191-192)
          rgb[3 * n + 0] = 1.0f / (1.0f + expf(-c3[0][0]));
          rgb[3 * n + 1] = 1.0f / (1.0f + expf(-c3[0][1]));
          rgb[3 * n + 2] = 1.0f / (1.0f + expf(-c3[0][2]));
        }
      };
      finish(na, va, ha, c3a);
      finish(nb, vb, hb, c3b);
    }
  }
}

// ---- helper of the backward kernel -----------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void zero_vec_bf(f32x4 (&a)[N]) {
#pragma unroll
  for (int b = 0; b < N; ++b) a[b] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// =====================================================================================================================
// `fruit_nerf_big` semantic branch, backward: mlp_semantics 30 -> 128 -> 128 -> 64 + SemanticFieldHead
// (fruit_field.py:144-156,263-268 with fruit_nerf_config.py:82-95).  Its 119 KB of fp32 weights, 464 accumulator
// registers of dW and 128-wide activations made the fp32 path two launches of 4 waves x 512 registers that each repeat
// the forward and most of the dX chain (field_mlp_bwd_fp32.hip: 2.26 ms of a 7.06 ms step at 8192 rays).  Here:
//   * WEIGHT STREAMING: a workgroup of 8 waves takes a batch of 8 tiles (128 samples) through the branch layer by layer;
//     the bf16 fragment pieces of the layer(s) in use are re-staged from L2 into the SAME LDS region per phase
//     (forward sem0+sem1 at three pieces, 120 KB | transposed head+sem2 | transposed sem1 at two: ~1.8 KB of L2 reads per sample);
//   * COOPERATIVE dW: dW = dY^T X is not accumulated per wave.  All waves write their tile's dY and X columns (bf16
//     pieces) into one [feature row][128 samples] LDS scratch (it overlays the weight region between phases), and every
//     output block (16 x 16 weights) of the layer is owned by ONE wave, which sums it over the batch's 128 samples (four
//     K = 32 MFMAs per piece product).  116 blocks / 8 waves = 15 accumulator blocks (60 registers) per wave instead of
//     464, no cross-wave reduction at the end, and the whole branch runs once, at two waves per SIMD;
//   * the head's dW needs s3 = sem2(s2), which is not recomputed: dW_head = sum_s dlogit_s s3_s = W2 (sum_s dlogit_s s2_s)
//     + b2 sum_s dlogit_s is linear in a 128-vector that falls out of the sem2 round as one more block per wave.
// =====================================================================================================================
template <class Cfg>
struct SegsBigP1 {  // forward sem0, sem1
  static constexpr int N = 2;
  static constexpr int layer(int i) { return i == 0 ? Cfg::L_SEM0 : Cfg::L_SEM1; }
  static constexpr bool isT(int) { return false; }
};
template <class Cfg>
struct SegsBigP2 {  // transposed head, sem2
  static constexpr int N = 2;
  static constexpr int layer(int i) { return i == 0 ? Cfg::L_HEAD : Cfg::L_SEM2; }
  static constexpr bool isT(int) { return true; }
};
template <class Cfg>
struct SegsBigP4 {  // transposed sem1
  static constexpr int N = 1;
  static constexpr int layer(int) { return Cfg::L_SEM1; }
  static constexpr bool isT(int) { return true; }
};

constexpr int CS_LD = 72;     // words per scratch row: 64 hold the batch's 128 bf16 samples; 72 keeps the b128 reads conflict-free
constexpr int CS_ROWS = 128;  // feature rows per operand
template <int NS>
constexpr int cs_words() { return 2 * NS * CS_ROWS * CS_LD; }  // [G | X][piece][row][CS_LD]

// this wave's tile (NB accumulator blocks) -> rows ROW0.. of operand array `arr`, columns 16 wave + j, as bf16 pieces
template <int NS, int NB>
__device__ __forceinline__ void cs_write(uint32_t* __restrict__ arr, int row0, const f32x4 (&a)[NB], int lane, int wave) {
  const int j = lane & 15, g = lane >> 4;
  __bf16* base = reinterpret_cast<__bf16*>(arr);
#pragma unroll
  for (int blk = 0; blk < NB; ++blk)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = a[blk][r];
#pragma unroll
      for (int pc = 0; pc < NS; ++pc) {
        const __bf16 pv = (__bf16)v;
        base[(size_t)((pc * CS_ROWS + row0 + 16 * blk + 4 * g + r) * (2 * CS_LD)) + 16 * wave + j] = pv;
        if (pc + 1 < NS) v -= (float)pv;
      }
    }
}

// acc[s] += (G rows of block ob0 + s ob_step)^T (X rows of block ib) over the batch's 128 samples
template <int NS, int NOBW>
__device__ __forceinline__ void cs_dw(const uint32_t* __restrict__ sG, const uint32_t* __restrict__ sX, int ob0,
                                      int ob_step, int ib, f32x4 (&acc)[NOBW], int lane) {
  const int i = lane & 15, g = lane >> 4;
  // steps (kk, s), K-block outermost (one X fragment set live at a time); explicit double buffer of the G fragments
  // pinned by scheduling barriers (see bf_layer_acc1)
  constexpr int T = 4 * NOBW;
  bf16x8 ga[2][NS], xb[NS];
  auto load_g = [&](int t, bf16x8 (&dst)[NS]) {
    const int kk = t / NOBW, ob = ob0 + (t % NOBW) * ob_step;
#pragma unroll
    for (int pc = 0; pc < NS; ++pc)
      dst[pc] = *reinterpret_cast<const bf16x8*>(sG + (pc * CS_ROWS + 16 * ob + i) * CS_LD + 16 * kk + 4 * g);
  };
  load_g(0, ga[0]);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int kk = t / NOBW, s = t % NOBW;
    if (s == 0) {
#pragma unroll
      for (int pc = 0; pc < NS; ++pc)
        xb[pc] = *reinterpret_cast<const bf16x8*>(sX + (pc * CS_ROWS + 16 * ib + i) * CS_LD + 16 * kk + 4 * g);
    }
    if (t + 1 < T) load_g(t + 1, ga[(t + 1) & 1]);
#pragma unroll
    for (int sp = NS - 1; sp >= 0; --sp)
#pragma unroll
      for (int pg = 0; pg <= sp; ++pg)
        acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga[t & 1][pg], xb[sp - pg], acc[s], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}
// bacc += (G rows of block ob)^T 1: every column of the block ends up with the rows' sums over the batch
template <int NS>
__device__ __forceinline__ void cs_bias(const uint32_t* __restrict__ sG, int ob, f32x4& bacc, int lane) {
  const int i = lane & 15, g = lane >> 4;
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int pc = NS - 1; pc >= 0; --pc) {
      const bf16x8 ga = *reinterpret_cast<const bf16x8*>(sG + (pc * CS_ROWS + 16 * ob + i) * CS_LD + 16 * kk + 4 * g);
      bacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga, ones, bacc, 0, 0, 0);
    }
}
// one owned block of dW -> the workgroup's fp32 partial image (index space of field_layers.hpp / flush_dw)
__device__ __forceinline__ void store_dw_block(float* __restrict__ W, int ob, int ib, int nib_stride, const f32x4& acc,
                                               int lane) {
  const int jn = lane & 15, g = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    W[((ob * nib_stride + ib) * 64 + swz_slot(4 * g + r, jn >> 2)) * 4 + (jn & 3)] = acc[r];
}
__device__ __forceinline__ void store_bias_block(float* __restrict__ B, int ob, const f32x4& bacc, int lane) {
  if ((lane & 15) == 0) {
    const int g = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) B[16 * ob + 4 * g + r] = bacc[r];
  }
}

// NSF = pieces of the forward recompute, NS = pieces of the dX chain and of dW.  bf16x3 mode: NSF = 3, NS = 2 — the
// recomputed activations decide the ReLU gates, and a gate that flips against the forward pass
// changes a whole sample's contribution to a dW row: with two pieces (2^-17) that happened ~1000x more often
// than with three (2^-27) and single flips showed as ~5e-3 of max |g| under random zero-mean upstream gradients.
// SEMGRAD (pass_semantic_gradients, fruit_field.py:202-203, 263-264): geo is not detached — a fifth phase per batch forms
// Gh = W_sem0^T Gs1 and adds it into the samples' rows of d_h [N,32] (behind the colour kernel that wrote them, ahead of the
// base kernel that reads them, one writer per row).  sem0's transposed fragments are not in the bf16 image: built into the
// shared region from the fp32 image (bf_build_T).  Slot 0, the density logit, receives nothing.
template <class Cfg, int NSF, int NS, bool SEMGRAD = false, class... DH>
__global__ __launch_bounds__(512, 2) void k_field_mlp_bwd_sem_big_bf16(
    const float* __restrict__ packed, const __bf16* __restrict__ image, const float* __restrict__ w_sem2,
    const float* __restrict__ b_sem2, long long N, const float* __restrict__ h_saved, const float* __restrict__ d_logit,
    float* __restrict__ partials, DH... d_h_semgrad) {  // SEMGRAD: float* d_h
  static_assert(sizeof...(DH) == (SEMGRAD ? 1 : 0), "d_h comes with SEMGRAD");
  static_assert(Cfg::NSEM == 3 && Cfg::HB == 2 && Cfg::SEMB == 8, "fruit_nerf_big semantic shape");
  constexpr int WAVES = 8, THREADS = 64 * WAVES;
  constexpr int LS0 = Cfg::L_SEM0, LS1 = Cfg::L_SEM1, LS2 = Cfg::L_SEM2, LH = Cfg::L_HEAD;
  static_assert(LS1 == LS0 + 1 && LS2 == LS1 + 1 && LH == LS2 + 1, "the branch's layers are adjacent in the fp32 image");
  using P1 = BfLds<Cfg, SegsBigP1<Cfg>, NSF>;
  using P2 = BfLds<Cfg, SegsBigP2<Cfg>, NS>;
  using P4 = BfLds<Cfg, SegsBigP4<Cfg>, NS>;
  constexpr int REGION = cs_words<NS>() * 4;  // weights of a phase and the dW scratch share this region
  static_assert(P1::BYTES <= REGION && P2::BYTES <= REGION && P4::BYTES <= REGION, "phase weights exceed the shared region");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16x8* wl = reinterpret_cast<bf16x8*>(smem);
  uint32_t* sG = reinterpret_cast<uint32_t*>(smem);
  uint32_t* sX = sG + NS * CS_ROWS * CS_LD;
  float* fbias = reinterpret_cast<float*>(smem + REGION);  // forward biases: sem0 [128] | sem1 [128]
  float* vhead = fbias + 256;                              // epilogue: sum_s dlogit_s s2_s [128] and sum_s dlogit_s
  for (int i = threadIdx.x; i < 256; i += THREADS) fbias[i] = packed[Cfg::W_TOTAL + Cfg::boff(LS0) + i];
  const int lane0 = threadIdx.x & 63, wave = threadIdx.x >> 6;

  // dW blocks owned by this wave: sem0 (ob = (w>>1) + 4 s, ib = w & 1), sem1 (ob = s, ib = w), sem2 (ob = s, ib = w),
  // the virtual head block (dlogit^T s2, ib = w); bias blocks: sem0 / sem1 ob = w, sem2 ob = w (waves 0..3), head (wave 4)
  f32x4 acc0[2], acc1[8], acc2[4], accV[1];
  f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0, b2 = b0;
  zero_vec_bf(acc0);
  zero_vec_bf(acc1);
  zero_vec_bf(acc2);
  zero_vec_bf(accV);

  const long long n_batches = (N + 127) / 128;
  for (long long batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    asm volatile("" ::: "memory");
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int j = lane & 15, g = lane >> 4;
    const long long n = batch * 128 + 16 * wave + j;
    const bool valid = n < N;
    const long long nn = valid ? n : N - 1;
    f32x4 h[2];
    h[0] = *reinterpret_cast<const f32x4*>(h_saved + (size_t)nn * 32 + 4 * g);
    h[1] = *reinterpret_cast<const f32x4*>(h_saved + (size_t)nn * 32 + 16 + 4 * g);
    f32x4 Gl[1];
    Gl[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (g == 0 && valid) Gl[0][0] = d_logit[n];

    // phase 1: forward sem0, sem1
    __syncthreads();  // the previous batch's last scratch reads
    P1::template stage<THREADS>(wl, image);
    __syncthreads();
    f32x4 s1[8], s2[8];
    bf_layer1<NSF, 8, 2>(P1::template seg<LS0, false>(wl), fbias, h, s1, lane);
    relu_(s1);
    bf_layer1<NSF, 8, 8>(P1::template seg<LS1, false>(wl), fbias + 128, s1, s2, lane);
    relu_(s2);
    // phase 2: dlogit -> Gs3 (mlp_semantics' output has no activation) -> Gs2.  The transposed head / sem2 fragments are
    // staged into the X half of the region, so that Gs3 and dlogit can go to the G half of the scratch as soon as they
    // exist (16 registers less at the kernel's register peak)
    __syncthreads();
    bf16x8* wl2 = reinterpret_cast<bf16x8*>(sX);
    static_assert(P2::BYTES <= NS * CS_ROWS * CS_LD * 4, "phase-2 fragments must fit the X half");
    P2::template stage<THREADS>(wl2, image);
    __syncthreads();
    f32x4 Gs2[8];
    {
      f32x4 Gs3[4];
      bf_layer_T1<NS, 4, 1>(P2::template seg<LH, true>(wl2), Gl, Gs3, lane);
      // round 1, G side: [Gs3 (blocks 0..3) | dlogit (block 4)]
      cs_write<NS, 4>(sG, 0, Gs3, lane, wave);
      cs_write<NS, 1>(sG, 64, Gl, lane, wave);
      bf_layer_T1<NS, 8, 4>(P2::template seg<LS2, true>(wl2), Gs3, Gs2, lane);
    }
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) Gs2[b][r] = (s2[b][r] > 0.0f) ? Gs2[b][r] : 0.0f;
    // round 1, X side: s2 -> dW sem2, the head's 128-vector, db sem2, db head
    __syncthreads();  // the fragments of phase 2 are dead
    cs_write<NS, 8>(sX, 0, s2, lane, wave);
    __syncthreads();
    cs_dw<NS, 4>(sG, sX, 0, 1, wave, acc2, lane);
    cs_dw<NS, 1>(sG, sX, 4, 0, wave, accV, lane);
    if (wave < 4) cs_bias<NS>(sG, wave, b2, lane);
    if (wave == 4) cs_bias<NS>(sG, 4, b2, lane);  // wave 4's b2 is the head's bias gradient
    // round 2: G = Gs2, X = s1 -> dW sem1, db sem1
    __syncthreads();
    cs_write<NS, 8>(sG, 0, Gs2, lane, wave);
    cs_write<NS, 8>(sX, 0, s1, lane, wave);
    __syncthreads();
    cs_dw<NS, 8>(sG, sX, 0, 1, wave, acc1, lane);
    cs_bias<NS>(sG, wave, b1, lane);
    // phase 4: Gs2 -> Gs1
    __syncthreads();
    P4::template stage<THREADS>(wl, image);
    __syncthreads();
    f32x4 Gs1[8];
    bf_layer_T1<NS, 8, 8>(P4::template seg<LS1, true>(wl), Gs2, Gs1, lane);
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) Gs1[b][r] = (s1[b][r] > 0.0f) ? Gs1[b][r] : 0.0f;
    // round 3: G = Gs1, X = h -> dW sem0, db sem0 (the input is the detached geo: no dX unless SEMGRAD)
    __syncthreads();
    cs_write<NS, 8>(sG, 0, Gs1, lane, wave);
    {
      f32x4 hx[2];  // re-read (L2-resident) instead of keeping 8 registers live across the whole batch
      hx[0] = *reinterpret_cast<const f32x4*>(h_saved + (size_t)nn * 32 + 4 * g);
      hx[1] = *reinterpret_cast<const f32x4*>(h_saved + (size_t)nn * 32 + 16 + 4 * g);
      cs_write<NS, 2>(sX, 0, hx, lane, wave);
    }
    __syncthreads();
    cs_dw<NS, 2>(sG, sX, wave >> 1, 4, wave & 1, acc0, lane);
    cs_bias<NS>(sG, wave, b0, lane);
    if constexpr (SEMGRAD) {  // phase 5: Gs1 -> Gh, d_h += Gh
      constexpr int T0_BYTES = NS * Cfg::nib(LS0) * ((Cfg::nob(LS0) + 1) / 2) * 1024;
      static_assert(T0_BYTES <= REGION, "sem0's transposed fragments exceed the shared region");
      __syncthreads();  // round 3's scratch reads
      bf_build_T<Cfg, LS0, NS, THREADS>(wl, packed);
      __syncthreads();
      f32x4 Gh[2];
      bf_layer_T1<NS, 2, 8>(wl, Gs1, Gh, lane);
      if (g == 0) Gh[0][0] = 0.0f;  // the density logit is not an input of mlp_semantics
      if (valid) {
        float* const d_h = only(d_h_semgrad...);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          f32x4* row = reinterpret_cast<f32x4*>(d_h + (size_t)n * 32 + 16 * b + 4 * g);
          *row = *row + Gh[b];
        }
      }
    }
  }

  // ---- this workgroup's partial image: every block of the branch's layers is written by its owner -------------------
  const int lane = lane0;
  float* part = partials + (size_t)blockIdx.x * (Cfg::W_TOTAL + Cfg::B_TOTAL);
  float* pb = part + Cfg::W_TOTAL;
#pragma unroll
  for (int s = 0; s < 2; ++s) store_dw_block(part + Cfg::woff(LS0), (wave >> 1) + 4 * s, wave & 1, 2, acc0[s], lane);
#pragma unroll
  for (int s = 0; s < 8; ++s) store_dw_block(part + Cfg::woff(LS1), s, wave, 8, acc1[s], lane);
#pragma unroll
  for (int s = 0; s < 4; ++s) store_dw_block(part + Cfg::woff(LS2), s, wave, 8, acc2[s], lane);
  store_bias_block(pb + Cfg::boff(LS0), wave, b0, lane);
  store_bias_block(pb + Cfg::boff(LS1), wave, b1, lane);
  if (wave < 4) store_bias_block(pb + Cfg::boff(LS2), wave, b2, lane);
  // SemanticFieldHead: dW = W2 v + b2 sum(dlogit), v = row 0 of the virtual blocks, sum(dlogit) = row 0 of wave 4's b2
  __syncthreads();
  if ((lane >> 4) == 0) vhead[16 * wave + (lane & 15)] = accV[0][0];
  if (wave == 4 && lane == 0) vhead[128] = b2[0];
  for (int i = threadIdx.x; i < Cfg::nob(LH) * Cfg::nib(LH) * 256; i += THREADS) part[Cfg::woff(LH) + i] = 0.0f;
  for (int i = threadIdx.x; i < 16; i += THREADS) pb[Cfg::boff(LH) + i] = 0.0f;
  __syncthreads();
  if (threadIdx.x < 64) {
    const int k = threadIdx.x;  // head input k = output k of mlp_semantics' last layer
    float dw = b_sem2[k] * vhead[128];
    for (int m = 0; m < 128; ++m) dw = fmaf(w_sem2[k * 128 + m], vhead[m], dw);
    const int ib = k >> 4, kk = k & 15;
    part[Cfg::woff(LH) + (ib * 64 + swz_slot(0, kk >> 2)) * 4 + (kk & 3)] = dw;
    if (k == 0) pb[Cfg::boff(LH)] = vhead[128];
  }
}

// ---- `fruit_nerf_big` semantic branch, forward (h [N,32] -> logit): the same weight streaming in two phases ------------
template <class Cfg>
struct SegsBigF2 {  // forward sem2, head
  static constexpr int N = 2;
  static constexpr int layer(int i) { return i == 0 ? Cfg::L_SEM2 : Cfg::L_HEAD; }
  static constexpr bool isT(int) { return false; }
};

template <class Cfg, int NS, int WAVES>
__global__ __launch_bounds__(64 * WAVES, WAVES / 4) void k_field_mlp_fwd_sem_big_bf16(
    const float* __restrict__ packed, const __bf16* __restrict__ image, long long N, const float* __restrict__ h_buf,
    float* __restrict__ logit) {
  static_assert(Cfg::NSEM == 3 && Cfg::HB == 2 && Cfg::SEMB == 8, "fruit_nerf_big semantic shape");
  constexpr int THREADS = 64 * WAVES;
  constexpr int LS0 = Cfg::L_SEM0, LS1 = Cfg::L_SEM1, LS2 = Cfg::L_SEM2, LH = Cfg::L_HEAD;
  using F1 = BfLds<Cfg, SegsBigP1<Cfg>, NS>;
  using F2 = BfLds<Cfg, SegsBigF2<Cfg>, NS>;
  constexpr int REGION = F1::BYTES > F2::BYTES ? F1::BYTES : F2::BYTES;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16x8* wl = reinterpret_cast<bf16x8*>(smem);
  float* fbias = reinterpret_cast<float*>(smem + REGION);  // sem0 [128] | sem1 [128] | sem2 [64] | head [16]
  for (int i = threadIdx.x; i < 336; i += THREADS) fbias[i] = packed[Cfg::W_TOTAL + Cfg::boff(LS0) + i];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const long long per_batch = 16 * WAVES;
  const long long n_batches = (N + per_batch - 1) / per_batch;
  for (long long batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
    asm volatile("" ::: "memory");
    const long long n = batch * per_batch + 16 * wave + j;
    const bool valid = n < N;
    const long long nn = valid ? n : N - 1;
    f32x4 h[2];
    h[0] = *reinterpret_cast<const f32x4*>(h_buf + (size_t)nn * 32 + 4 * g);
    h[1] = *reinterpret_cast<const f32x4*>(h_buf + (size_t)nn * 32 + 16 + 4 * g);
    __syncthreads();
    F1::template stage<THREADS>(wl, image);
    __syncthreads();
    f32x4 s1[8], s2[8];
    bf_layer1<NS, 8, 2>(F1::template seg<LS0, false>(wl), fbias, h, s1, lane);
    relu_(s1);
    bf_layer1<NS, 8, 8>(F1::template seg<LS1, false>(wl), fbias + 128, s1, s2, lane);
    relu_(s2);
    __syncthreads();
    F2::template stage<THREADS>(wl, image);
    __syncthreads();
    f32x4 s3[4], hd[1];
    bf_layer1<NS, 4, 8>(F2::template seg<LS2, false>(wl), fbias + 256, s2, s3, lane);
    bf_layer1<NS, 1, 4>(F2::template seg<LH, false>(wl), fbias + 320, s3, hd, lane);
    if (g == 0 && valid) logit[n] = hd[0][0];
  }
}

int field_mlp_fwd_sem_big_bf16(int mode, const FieldPtrs& p, void* image_ws, const float* packed, long long N,
                               const float* h_buf, float* logit, hipStream_t st) {
  using Cfg = FieldCfgBig;
  __bf16* image = reinterpret_cast<__bf16*>(image_ws);  // packed by the caller (k_prepare_field)
  constexpr int WAVES = 8;
  const long long n_batches = (N + 16 * WAVES - 1) / (16 * WAVES);
  long long blocks = n_batches;
  if (blocks > (long long)device_cu_count()) blocks = device_cu_count();
  auto launch = [&](int once, auto kern, int bytes) -> int {
    if (once) return once;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64 * WAVES), bytes, st, packed, image, N, h_buf, logit);
    FNR_LAUNCH_CHECK();
    return FNR_OK;
  };
  if (mode == MLP_BF16) {
    constexpr int bytes = BfLds<Cfg, SegsBigP1<Cfg>, 1>::BYTES + 336 * 4;
    constexpr auto kern = k_field_mlp_fwd_sem_big_bf16<Cfg, 1, WAVES>;
    return launch(ensure_dyn_lds<kern>(bytes), kern, bytes);
  }
  constexpr int bytes = BfLds<Cfg, SegsBigP1<Cfg>, 3>::BYTES + 336 * 4;
  static_assert(bytes <= 160 * 1024, "fruit_nerf_big forward fragments exceed the LDS");
  constexpr auto kern = k_field_mlp_fwd_sem_big_bf16<Cfg, 3, WAVES>;
  return launch(ensure_dyn_lds<kern>(bytes), kern, bytes);
}

template <int NSF, int NS>  // pass_semantic_gradients: the SEMGRAD instantiation, which takes d_h as one more argument
static int bwd_launch(const FieldBwdArgs& a) {
  using Cfg = FieldCfgBig;
  constexpr int bytes = cs_words<NS>() * 4 + (256 + 144) * 4;
  static_assert(bytes <= 160 * 1024, "fruit_nerf_big semantic branch exceeds the LDS");
  auto go = [&](int once, auto kern, auto... d_h) -> int {
    if (once) return once;
    hipLaunchKernelGGL(kern, dim3((unsigned)a.blocks), dim3(512), bytes, a.st, a.packed, a.image, a.p.w[Cfg::L_SEM2],
                       a.p.b[Cfg::L_SEM2], a.N, a.h_saved, a.d_logit, a.partials, d_h...);
    FNR_LAUNCH_CHECK();
    return FNR_OK;
  };
  constexpr auto kern = k_field_mlp_bwd_sem_big_bf16<Cfg, NSF, NS>;
  constexpr auto kern_sg = k_field_mlp_bwd_sem_big_bf16<Cfg, NSF, NS, true, float*>;
  return a.semgrad ? go(ensure_dyn_lds<kern_sg>(bytes), kern_sg, a.d_h) : go(ensure_dyn_lds<kern>(bytes), kern);
}

int field_mlp_bwd_sem_big_bf16(const FieldBwdArgs& a) { return a.mode == MLP_BF16 ? bwd_launch<1, 1>(a) : bwd_launch<3, 2>(a); }

// ---- forward launch (called from field_mlp.hip when fnr_field_net.mlp_mode != 0) -----------------------------------
template <class Cfg, int NS>
static int fwd_launch_bf16(const float* packed, const __bf16* image, const float* ray_bias, const RaysDev& rd, int S,
                           long long N, const float2* feats, const uint8_t* selector, float* density, float* rgb,
                           float* logit, float* geo_out, float* h_buf, hipStream_t st) {
  constexpr bool WITH_SEM = Cfg::NSEM == 2;
  using Segs = typename std::conditional<WITH_SEM, SegsFwdAll<Cfg>, SegsFwdBaseColor<Cfg>>::type;
  using Lds = BfLds<Cfg, Segs, NS>;
  constexpr int WAVES = 8;
  constexpr int bytes = Lds::BYTES + Cfg::B_TOTAL * 4;
  static_assert(bytes <= 160 * 1024, "forward fragments exceed the LDS");
  constexpr auto kern = k_field_mlp_fwd_bf16<Cfg, NS, WAVES, WITH_SEM>;
  const int once = ensure_dyn_lds<kern>(bytes);
  if (once) return once;
  const long long n_pairs = (N + 31) / 32;
  long long blocks = (n_pairs + WAVES - 1) / WAVES;
  const long long max_blocks = (long long)device_cu_count() * (bytes <= 80 * 1024 ? 2 : 1);
  if (blocks > max_blocks) blocks = max_blocks;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64 * WAVES), bytes, st, packed, image, ray_bias, rd, S, N, feats,
                     selector, density, rgb, logit, geo_out, h_buf);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

// cfg 0: `fruit_nerf` (all branches); cfg 1: `fruit_nerf_big`'s base + colour MLPs (logit untouched: the caller runs
// field_mlp_fwd_sem_big_bf16 on the saved h afterwards)
int field_mlp_fwd_bf16(int cfg, int mode, const FieldPtrs& p, const float* packed, void* image_ws, const float* ray_bias,
                       const RaysDev& rd, int S, long long N, const float2* feats, const uint8_t* selector, float* density,
                       float* rgb, float* logit, float* geo_out, float* h_buf, hipStream_t st) {
  __bf16* image = reinterpret_cast<__bf16*>(image_ws);  // packed by the caller (k_prepare_field)
#define FNR_FWD16(C, NSV) \
  fwd_launch_bf16<C, NSV>(packed, image, ray_bias, rd, S, N, feats, selector, density, rgb, logit, geo_out, h_buf, st)
  if (cfg == 0) return mode == MLP_BF16 ? FNR_FWD16(FieldCfgBase, 1) : FNR_FWD16(FieldCfgBase, 3);
  return mode == MLP_BF16 ? FNR_FWD16(FieldCfgBig, 1) : FNR_FWD16(FieldCfgBig, 3);
#undef FNR_FWD16
}

size_t field_bf16_image_bytes() {
  const size_t a = BfImage<FieldCfgBase>::bytes(BF_MAX_PIECES), b = BfImage<FieldCfgBig>::bytes(BF_MAX_PIECES);
  return (a > b ? a : b) + 256;
}

}  // namespace fnr
