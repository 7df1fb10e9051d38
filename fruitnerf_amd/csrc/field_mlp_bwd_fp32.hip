// field_mlp_bwd_fp32.hip — the branch kernels of FruitField's MLP backward on fp32 MFMA (v_mfma_f32_16x16x4_f32), mlp_mode
// FNR_MLP_FP32.  The branch schedule, the per-ray and weight finish and the entry points, shared with the bf16 modes: field_mlp_bwd.hip.
//
// Structure (per 16-sample tile, one wave; see field_layers.hpp for the forward layout):
//   * forward activations are RECOMPUTED from the saved hash features (128 B/sample) instead of being
//     stored (1.3 KB/sample) — MFMA time is cheaper than HBM traffic here;
//   * dX^T = W^T dY^T reuses the forward LDS weight image: lane (i', kg) reads W[16 ob + 4 kg + r][col(ib, i')]
//     with one conflict-free ds_read_b32 (that is what the XOR swizzle of the image is for), dY^T stays in
//     registers as the B operand;
//   * dW = dY^T X needs the samples on the K axis: both operands are transposed through a per-wave LDS
//     scratch (2 x 64 rows x 20 floats) and accumulated in registers across all tiles of the (persistent) wave;
//   * weight gradients leave the workgroup once: LDS reduction over its waves -> one partial image per
//     workgroup -> k_finish_weights sums the partials deterministically and un-permutes into nn.Linear layout.
// The branches are separate instantiations so that the dW accumulators fit next to the recomputed activations:
//   FieldCfgBase (`fruit_nerf`):      colour / semantic / base with 144 / 96 / 48 accumulator registers, 8 waves each;
//   FieldCfgBig  (`fruit_nerf_big`):  colour (160) and base (64) as above with a 32-wide h; the semantic branch
//     30 -> 128 -> 128 -> 64 -> 1 needs 464 accumulator registers and 119 KB of weights, so it runs as TWO launches
//     of 4 waves x <= 512 registers with all four layers in LDS: SEM_A owns dW of sem0, sem2 and the head (208
//     registers), SEM_B owns the 128 x 128 layer (256 registers); SEM_B repeats the forward up to s2 and the dX chain
//     down to Gs2 (1.35x the algorithmic MACs of the branch, no activations through HBM).
#include "field_layers.hpp"
#include "field_bf16.hpp"

namespace fnr {

enum { BR_SEM_A = 4, BR_SEM_B = 5 };  // the two launches of `fruit_nerf_big`'s BR_SEM (BR_*: field_bf16.hpp)

// padded row length of the transpose scratch: 20 makes both the C-layout writes (bank 16 g + 20 r + j) and the
// fragment reads (bank 20 j + 4 ks + g) conflict-free; 17 had 2-way conflicts between lane groups on the writes
constexpr int SCR_LD = 20;
constexpr int SCR_FLOATS = 2 * 64 * SCR_LD;  // G^T and X^T, 64 feature rows each

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);  // phase boundary for the scheduler too (keeps register pressure local)
}

// out (C-layout blocks IB0..IB0+NIBO-1 of the layer INPUT) = W^T * G^T
// LDS reads are issued in batches of 4*NIBO (one output block of the layer) ahead of their MFMAs: with one
// ds_read_b32 per MFMA the un-batched loop exposed one LDS round trip (~100 clk) per 4 MFMAs (128 clk).
template <int NOB, int NIB_TOTAL, int IB0, int NIBO>
__device__ __forceinline__ void mlp_layer_T(const float* __restrict__ P, const f32x4 (&G)[NOB], f32x4 (&out)[NIBO],
                                            int lane) {
  const int ip = lane & 15, kg = lane >> 4;
  const int a = ip >> 2, b = ip & 3;
  constexpr int QC = (NIBO > 2) ? 2 : NIBO;  // input blocks per pass: 2 keeps the double buffer at 16 registers
  static_assert(NIBO % QC == 0, "input blocks must split evenly");
#pragma unroll
  for (int q0 = 0; q0 < NIBO; q0 += QC) {
#pragma unroll
    for (int q = 0; q < QC; ++q) out[q0 + q] = f32x4{0.f, 0.f, 0.f, 0.f};
    float w[2][4][QC];
    auto load_ob = [&](int ob, float (&dst)[4][QC]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int slot = ((4 * kg + r) ^ a) + 16 * a;
#pragma unroll
        for (int q = 0; q < QC; ++q) dst[r][q] = P[((ob * NIB_TOTAL + (IB0 + q0 + q)) * 64 + slot) * 4 + b];
      }
    };
    load_ob(0, w[0]);
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) {
      if (ob + 1 < NOB) load_ob(ob + 1, w[(ob + 1) & 1]);  // next block's weights in flight during these MFMAs
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < QC; ++q)
          out[q0 + q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[ob & 1][r][q], G[ob][r], out[q0 + q], 0, 0, 0);
    }
  }
}

// acc[OB0 + ob][IB0 + ib] += sum over the tile's samples of G^T[16 ob + .][s] * X^T[16 ib + .][s], ob < NOB <= 4,
// ib < NIB <= 4 (G, X point at the first of NOB / NIB blocks; wider layers call this per 4 x 4 group of blocks so
// that the scratch stays at 2 x 64 rows per wave).  BIAS: also add the tile's row sums of G to bsum (lane = row).
template <int NOB, int NIB, int NOBT, int NIBT, int OB0, int IB0, bool BIAS>
__device__ __forceinline__ void dw_accumulate_sub(float* __restrict__ scr, const f32x4* __restrict__ G,
                                                  const f32x4* __restrict__ X, f32x4 (&acc)[NOBT][NIBT], float& bsum,
                                                  int lane) {
  static_assert(NOB <= 4 && NIB <= 4 && OB0 + NOB <= NOBT && IB0 + NIB <= NIBT, "block group out of range");
  const int j = lane & 15, g = lane >> 4;
  float* sG = scr;
  float* sX = scr + 64 * SCR_LD;
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
    for (int r = 0; r < 4; ++r) sG[(16 * ob + 4 * g + r) * SCR_LD + j] = G[ob][r];
#pragma unroll
  for (int ib = 0; ib < NIB; ++ib)
#pragma unroll
    for (int r = 0; r < 4; ++r) sX[(16 * ib + 4 * g + r) * SCR_LD + j] = X[ib][r];
  wave_lds_fence();
  // bias gradient of the layer: lane = feature row of G^T, summed over the tile's 16 samples (4 conflict-free
  // ds_read_b128); replaces 4 NOB (DPP row sum + branch + LDS atomic) sequences that cut the tile loop into
  // ~36 basic blocks
  if constexpr (BIAS) {
    const f32x4* row = reinterpret_cast<const f32x4*>(sG + lane * SCR_LD);
    const f32x4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
    const float t = ((r0[0] + r0[1]) + (r0[2] + r0[3])) + ((r1[0] + r1[1]) + (r1[2] + r1[3])) +
                    ((r2[0] + r2[1]) + (r2[2] + r2[3])) + ((r3[0] + r3[1]) + (r3[2] + r3[3]));
    bsum += (lane < 16 * NOB) ? t : 0.0f;
  }
  __builtin_amdgcn_sched_barrier(0);
  // fragment reads in two batches of 2*(NOB+NIB), each followed by its 2*NOB*NIB MFMAs: one LDS round trip per
  // batch instead of per k-step, at half the registers of a single batch (the colour branch was spilling)
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    float av[2][NOB], bv[2][NIB];
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      const int ks = 2 * half + k2;
#pragma unroll
      for (int ob = 0; ob < NOB; ++ob) av[k2][ob] = sG[(16 * ob + j) * SCR_LD + 4 * ks + g];
#pragma unroll
      for (int ib = 0; ib < NIB; ++ib) bv[k2][ib] = sX[(16 * ib + j) * SCR_LD + 4 * ks + g];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
      for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
        for (int ib = 0; ib < NIB; ++ib)
          acc[OB0 + ob][IB0 + ib] =
              __builtin_amdgcn_mfma_f32_16x16x4f32(av[k2][ob], bv[k2][ib], acc[OB0 + ob][IB0 + ib], 0, 0, 0);
  }
  wave_lds_fence();
}

template <int NOB, int NIB>
__device__ __forceinline__ void dw_accumulate(float* __restrict__ scr, const f32x4 (&G)[NOB], const f32x4 (&X)[NIB],
                                              f32x4 (&acc)[NOB][NIB], float& bsum, int lane) {
  dw_accumulate_sub<NOB, NIB, NOB, NIB, 0, 0, true>(scr, G, X, acc, bsum, lane);
}

// sum over the 16 lanes of a DPP row (= the 16 samples of the tile) without touching the LDS crossbar:
// quad xor 1, quad xor 2, row_half_mirror, row_mirror — every lane ends up with the row total
__device__ __forceinline__ float row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true));
  return v;
}

template <int N>
__device__ __forceinline__ void relu_mask_(f32x4 (&G)[N], const f32x4 (&act)[N]) {
#pragma unroll
  for (int b = 0; b < N; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) G[b][r] = (act[b][r] > 0.0f) ? G[b][r] : 0.0f;
}

// add this wave's dW accumulators of a layer into the workgroup's LDS image (`W` = the layer's block in LDS, same
// index space as the weights).  Plain read-add-write: the caller serialises the waves (ds_add_f32 retires ~1 lane per
// 3 clocks on gfx950 — 74k float atomics per workgroup cost 92 us here; 8 barrier-separated rounds cost ~4 us).
template <int NOB, int NIB, int NIB_STRIDE = NIB>
__device__ __forceinline__ void flush_dw(float* __restrict__ W, const f32x4 (&acc)[NOB][NIB], int lane) {
  const int jn = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
    for (int ib = 0; ib < NIB; ++ib)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int slot = swz_slot(4 * g + r, jn >> 2);
        W[((ob * NIB_STRIDE + ib) * 64 + slot) * 4 + (jn & 3)] += acc[ob][ib][r];
      }
}

template <class A>
__device__ __forceinline__ void zero_acc(A& acc) {
#pragma unroll
  for (auto& row : acc)
#pragma unroll
    for (auto& v : row) v = f32x4{0.f, 0.f, 0.f, 0.f};
}

// the layers a branch keeps in LDS (forward recompute + transposed reads) = the layers whose gradients it owns: a
// contiguous range of the fragment image for both shapes (FieldCfgBase used to stage the whole 75 KB image per branch)
template <class Cfg, int BRANCH>
struct BwdRange;
template <class Cfg>
struct BwdRange<Cfg, BR_COLOR> { using type = LdsRange<Cfg, Cfg::L_COL0, Cfg::L_COL2 + 1>; };
template <class Cfg>
struct BwdRange<Cfg, BR_BASE> { using type = LdsRange<Cfg, Cfg::L_BASE0, Cfg::L_BASE1 + 1>; };
template <class Cfg>
struct BwdRange<Cfg, BR_SEM> { using type = LdsRange<Cfg, Cfg::L_SEM0, Cfg::L_HEAD + 1>; };
template <class Cfg>
struct BwdRange<Cfg, BR_SEM_A> { using type = LdsRange<Cfg, Cfg::L_SEM0, Cfg::L_HEAD + 1>; };
template <class Cfg>
struct BwdRange<Cfg, BR_SEM_B> { using type = LdsRange<Cfg, Cfg::L_SEM0, Cfg::L_HEAD + 1>; };

// ---- colour branch: mlp_head (fruit_field.py:158-166,270-281) -----------------------------------------------------
template <class Cfg, int WAVES>
__global__ __launch_bounds__(64 * WAVES, WAVES / 4) void k_field_mlp_bwd_color(
    const float* __restrict__ packed, const float* __restrict__ ray_bias, RaysDev rays, int S, long long N,
    const float* __restrict__ h_saved, const float* __restrict__ d_rgb, float* __restrict__ d_h,
    float* __restrict__ gsum_tile, float* __restrict__ gsum_extra, float* __restrict__ partials) {
  using R = typename BwdRange<Cfg, BR_COLOR>::type;
  constexpr int HB = Cfg::HB;
  constexpr int LC0 = Cfg::L_COL0, LC1 = Cfg::L_COL1, LC2 = Cfg::L_COL2;
  __shared__ __attribute__((aligned(16))) float lds[R::FLOATS + WAVES * SCR_FLOATS + 80];
  float* scr_all = lds + R::FLOATS;
  float* lds_bias = scr_all + WAVES * SCR_FLOATS;  // bias-gradient accumulators of col1 (64) and col2 (16)
  R::template stage<64 * WAVES>(lds, packed);
  for (int i = threadIdx.x; i < 80; i += blockDim.x) lds_bias[i] = 0.0f;
  __syncthreads();
  const int lane0 = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* scr = scr_all + wave * SCR_FLOATS;

  f32x4 accA[4][HB];  // col0, h blocks
  f32x4 accB[4][4];   // col1
  f32x4 accC[1][4];   // col2
  float bsB = 0.0f, bsC = 0.0f;
  zero_acc(accA);
  zero_acc(accB);
  zero_acc(accC);

  const long long n_tiles = (N + 15) / 16;
  for (long long tile = (long long)blockIdx.x * WAVES + wave; tile < n_tiles; tile += (long long)gridDim.x * WAVES) {
    asm volatile("" ::: "memory");  // keep the LDS weight reads inside the loop (see field_mlp.hip)
    // ... and their addresses: hoisted out of the loop, the ~50 lane-dependent LDS offsets of the layers stayed
    // live across the whole body and were spilled; an opaque copy of the lane id makes them per-use VALU ops
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int j = lane & 15, g = lane >> 4;
    const long long n = tile * 16 + j;
    const bool valid = n < N;
    const long long nn = valid ? n : N - 1;
    const long long ray = nn / S;

    f32x4 h[HB];
#pragma unroll
    for (int b = 0; b < HB; ++b) h[b] = *reinterpret_cast<const f32x4*>(h_saved + (size_t)nn * (16 * HB) + 16 * b + 4 * g);

    // colour MLP; its first layer only multiplies the h blocks, the ray-constant inputs come in as ray_bias
    // (field_layers.hpp: color_layer0)
    f32x4 c1[4], c2[4], c3[1];
    color_layer0<Cfg>(R::w(lds, LC0), ray_bias, ray, h, c1, lane);
    relu_(c1);
    mlp_layer<4, 4>(R::w(lds, LC1), R::b(lds, LC1), c1, c2, lane);
    relu_(c2);
    mlp_layer<1, 4>(R::w(lds, LC2), R::b(lds, LC2), c2, c3, lane);
    // d(pre-sigmoid) = d_rgb * rgb * (1 - rgb) on rows 0..2 (lane group 0), zero elsewhere
    f32x4 G3[1];
    G3[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (g == 0 && valid) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float s = 1.0f / (1.0f + expf(-c3[0][r]));
        G3[0][r] = d_rgb[3 * n + r] * s * (1.0f - s);
      }
    }
    dw_accumulate<1, 4>(scr, G3, c2, accC, bsC, lane);
    f32x4 G2[4];
    mlp_layer_T<1, 4, 0, 4>(R::w(lds, LC2), G3, G2, lane);
    relu_mask_(G2, c2);
    dw_accumulate<4, 4>(scr, G2, c1, accB, bsB, lane);
    f32x4 G1[4];
    mlp_layer_T<4, 4, 0, 4>(R::w(lds, LC1), G2, G1, lane);
    relu_mask_(G1, c1);
    // layer 0: dW of the h blocks here; for the 48 ray-constant inputs (and the bias) the gradient is the outer
    // product (sum over the ray's samples of G1) x c_ray, so only the tile's 64 row sums of G1 leave the kernel
    // and k_color_ray_grads finishes the job per ray (weights, bias, appearance embedding).
    float gs = 0.0f;
    dw_accumulate<4, HB>(scr, G1, h, accA, gs, lane);
    const long long ray0 = __shfl(ray, lane & 48, 64);
    const bool uniform = __all(ray == ray0);  // invalid lanes were clamped to the last sample's ray
    if (uniform) {
      gsum_tile[(size_t)tile * 64 + lane] = gs;
    } else if (valid) {  // tile straddles rays (S % 16 != 0): per-sample contributions
#pragma unroll
      for (int ob = 0; ob < 4; ++ob)
#pragma unroll
        for (int r = 0; r < 4; ++r) atomicAdd(&gsum_extra[(size_t)ray * 64 + 16 * ob + 4 * g + r], G1[ob][r]);
    }
    f32x4 Gh[HB];
    mlp_layer_T<4, HB + 3, 0, HB>(R::w(lds, LC0), G1, Gh, lane);
    if (valid) {
#pragma unroll
      for (int b = 0; b < HB; ++b) *reinterpret_cast<f32x4*>(d_h + (size_t)n * (16 * HB) + 16 * b + 4 * g) = Gh[b];
    }
  }

  // ---- workgroup reduction of the weight gradients, then this branch's part of the workgroup's partial image ----
  const int lane = lane0;
  __syncthreads();  // every wave is done with the weight image
  float* acc_lds = R::w(lds, LC0);
  constexpr int ACC_FLOATS = Cfg::woff(LC2 + 1) - Cfg::woff(LC0);
  for (int i = threadIdx.x; i < ACC_FLOATS; i += blockDim.x) acc_lds[i] = 0.0f;
  __syncthreads();
  for (int turn = 0; turn < WAVES; ++turn) {
    if (wave == turn) {
      flush_dw<4, HB, HB + 3>(R::w(lds, LC0), accA, lane);
      flush_dw<4, 4>(R::w(lds, LC1), accB, lane);
      flush_dw<1, 4>(R::w(lds, LC2), accC, lane);
      lds_bias[lane] += bsB;
      if (lane < 16) lds_bias[64 + lane] += bsC;
    }
    __syncthreads();
  }
  float* part = partials + (size_t)blockIdx.x * (Cfg::W_TOTAL + Cfg::B_TOTAL);
  for (int i = threadIdx.x; i < ACC_FLOATS; i += blockDim.x) part[Cfg::woff(LC0) + i] = acc_lds[i];
  // col0's bias slot belongs to k_color_ray_grads (which owns some workgroups' images only): zero it here
  for (int i = threadIdx.x; i < 64; i += blockDim.x) part[Cfg::W_TOTAL + Cfg::boff(LC0) + i] = 0.0f;
  for (int i = threadIdx.x; i < 64; i += blockDim.x) part[Cfg::W_TOTAL + Cfg::boff(LC1) + i] = lds_bias[i];
  for (int i = threadIdx.x; i < 16; i += blockDim.x) part[Cfg::W_TOTAL + Cfg::boff(LC2) + i] = lds_bias[64 + i];
}

// ---- base branch: mlp_base_mlp (fruit_field.py:132-140,187-193) ----------------------------------------------------
template <class Cfg, int WAVES>
__global__ __launch_bounds__(64 * WAVES, WAVES / 4) void k_field_mlp_bwd_base(
    const float* __restrict__ packed, long long N, const float2* __restrict__ feats,
    const uint8_t* __restrict__ selector, const float* __restrict__ d_density, const float* __restrict__ d_h,
    float2* __restrict__ d_feats, float* __restrict__ partials) {
  using R = typename BwdRange<Cfg, BR_BASE>::type;
  constexpr int HB = Cfg::HB;
  constexpr int LB0 = Cfg::L_BASE0, LB1 = Cfg::L_BASE1;
  __shared__ __attribute__((aligned(16))) float lds[R::FLOATS + WAVES * SCR_FLOATS + 64 + 16 * HB];
  float* scr_all = lds + R::FLOATS;
  float* lds_bias = scr_all + WAVES * SCR_FLOATS;
  R::template stage<64 * WAVES>(lds, packed);
  for (int i = threadIdx.x; i < 64 + 16 * HB; i += blockDim.x) lds_bias[i] = 0.0f;
  __syncthreads();
  const int lane0 = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* scr = scr_all + wave * SCR_FLOATS;

  f32x4 accA[4][2];   // base0
  f32x4 accB[HB][4];  // base1
  float bsA = 0.0f, bsB = 0.0f;
  zero_acc(accA);
  zero_acc(accB);

  const long long n_tiles = (N + 15) / 16;
  for (long long tile = (long long)blockIdx.x * WAVES + wave; tile < n_tiles; tile += (long long)gridDim.x * WAVES) {
    asm volatile("" ::: "memory");
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int j = lane & 15, g = lane >> 4;
    const long long n = tile * 16 + j;
    const bool valid = n < N;
    const long long nn = valid ? n : N - 1;

    // the hidden layer is recomputed from the hash features
    f32x4 x0[2], a1[4], h[HB];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float2 v = feats[(size_t)(4 * m + g) * N + nn];
      x0[m >> 1][2 * (m & 1)] = v.x;
      x0[m >> 1][2 * (m & 1) + 1] = v.y;
    }
    mlp_layer<4, 2>(R::w(lds, LB0), R::b(lds, LB0), x0, a1, lane);
    relu_(a1);
    mlp_layer<HB, 4>(R::w(lds, LB1), R::b(lds, LB1), a1, h, lane);

    // dL/dh = colour-branch gradient (+ density through trunc_exp on row 0)
    f32x4 Gh[HB];
#pragma unroll
    for (int b = 0; b < HB; ++b) Gh[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (valid) {
#pragma unroll
      for (int b = 0; b < HB; ++b) Gh[b] = *reinterpret_cast<const f32x4*>(d_h + (size_t)n * (16 * HB) + 16 * b + 4 * g);
      if (g == 0) {
        const bool sel = selector ? (selector[n] != 0) : true;
        const float te = expf(fminf(fmaxf(h[0][0], -15.0f), 15.0f));  // trunc_exp backward (fruit_field.py:191)
        Gh[0][0] = sel ? d_density[n] * te : 0.0f;                   // colour block has a zero row 0
      }
    }
    dw_accumulate<HB, 4>(scr, Gh, a1, accB, bsB, lane);
    f32x4 Ga[4];
    mlp_layer_T<HB, 4, 0, 4>(R::w(lds, LB1), Gh, Ga, lane);
    relu_mask_(Ga, a1);
    dw_accumulate<4, 2>(scr, Ga, x0, accA, bsA, lane);
    f32x4 Gx[2];
    mlp_layer_T<4, 2, 0, 2>(R::w(lds, LB0), Ga, Gx, lane);
    if (valid) {
#pragma unroll
      for (int m = 0; m < 4; ++m)
        d_feats[(size_t)(4 * m + g) * N + n] = make_float2(Gx[m >> 1][2 * (m & 1)], Gx[m >> 1][2 * (m & 1) + 1]);
    }
  }

  const int lane = lane0;
  __syncthreads();
  float* acc_lds = R::w(lds, LB0);
  constexpr int ACC_FLOATS = Cfg::woff(LB1 + 1) - Cfg::woff(LB0);
  for (int i = threadIdx.x; i < ACC_FLOATS; i += blockDim.x) acc_lds[i] = 0.0f;
  __syncthreads();
  for (int turn = 0; turn < WAVES; ++turn) {
    if (wave == turn) {
      flush_dw<4, 2>(R::w(lds, LB0), accA, lane);
      flush_dw<HB, 4>(R::w(lds, LB1), accB, lane);
      lds_bias[lane] += bsA;
      if (lane < 16 * HB) lds_bias[64 + lane] += bsB;
    }
    __syncthreads();
  }
  float* part = partials + (size_t)blockIdx.x * (Cfg::W_TOTAL + Cfg::B_TOTAL);
  for (int i = threadIdx.x; i < ACC_FLOATS; i += blockDim.x) part[Cfg::woff(LB0) + i] = acc_lds[i];
  for (int i = threadIdx.x; i < 64; i += blockDim.x) part[Cfg::W_TOTAL + Cfg::boff(LB0) + i] = lds_bias[i];
  for (int i = threadIdx.x; i < 16 * HB; i += blockDim.x) part[Cfg::W_TOTAL + Cfg::boff(LB1) + i] = lds_bias[64 + i];
}

// ---- semantic branch, `fruit_nerf` shape: 15 -> 64 -> 64 -> head (fruit_field.py:144-156,263-268) ----------------------
// SEMGRAD (pass_semantic_gradients): geo is not detached, so dX of sem0, Gh = W_sem0^T Gs1, is added into the samples' rows
// of d_h — behind the colour kernel that wrote them, ahead of the base kernel that reads them, one writer per row.  The column
// of the density logit h[0] is a structural zero of sem0 (KM_GEO) and is masked besides: slot 0 receives nothing.
template <class Cfg, int WAVES, bool SEMGRAD = false, class... DH>
__global__ __launch_bounds__(64 * WAVES, WAVES / 4) void k_field_mlp_bwd_sem(
    const float* __restrict__ packed, long long N, const float* __restrict__ h_saved,
    const float* __restrict__ d_logit, float* __restrict__ partials, DH... d_h_semgrad) {  // SEMGRAD: float* d_h
  static_assert(sizeof...(DH) == (SEMGRAD ? 1 : 0), "d_h comes with SEMGRAD");
  static_assert(Cfg::NSEM == 2 && Cfg::HB == 1, "the single-launch semantic branch is the fruit_nerf shape");
  using R = typename BwdRange<Cfg, BR_SEM>::type;
  constexpr int LS0 = Cfg::L_SEM0, LS1 = Cfg::L_SEM1, LH = Cfg::L_HEAD;
  __shared__ __attribute__((aligned(16))) float lds[R::FLOATS + WAVES * SCR_FLOATS + 144];
  float* scr_all = lds + R::FLOATS;
  float* lds_bias = scr_all + WAVES * SCR_FLOATS;  // sem0 (64), sem1 (64), head (16)
  R::template stage<64 * WAVES>(lds, packed);
  for (int i = threadIdx.x; i < 144; i += blockDim.x) lds_bias[i] = 0.0f;
  __syncthreads();
  const int lane0 = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* scr = scr_all + wave * SCR_FLOATS;

  f32x4 accA[4][1], accB[4][4], accC[1][4];
  float bsA = 0.0f, bsB = 0.0f, bsC = 0.0f;
  zero_acc(accA);
  zero_acc(accB);
  zero_acc(accC);

  const long long n_tiles = (N + 15) / 16;
  for (long long tile = (long long)blockIdx.x * WAVES + wave; tile < n_tiles; tile += (long long)gridDim.x * WAVES) {
    asm volatile("" ::: "memory");
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int j = lane & 15, g = lane >> 4;
    const long long n = tile * 16 + j;
    const bool valid = n < N;
    const long long nn = valid ? n : N - 1;
    f32x4 h[1];
    h[0] = *reinterpret_cast<const f32x4*>(h_saved + (size_t)nn * 16 + 4 * g);
    f32x4 s1[4], s2[4];
    mlp_layer<4, 1>(R::w(lds, LS0), R::b(lds, LS0), h, s1, lane);
    relu_(s1);
    mlp_layer<4, 4>(R::w(lds, LS1), R::b(lds, LS1), s1, s2, lane);
    f32x4 Gl[1];
    Gl[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (g == 0 && valid) Gl[0][0] = d_logit[n];
    dw_accumulate<1, 4>(scr, Gl, s2, accC, bsC, lane);   // SemanticFieldHead
    f32x4 Gs2[4];
    mlp_layer_T<1, 4, 0, 4>(R::w(lds, LH), Gl, Gs2, lane);  // no activation on mlp_semantics' last layer
    dw_accumulate<4, 4>(scr, Gs2, s1, accB, bsB, lane);
    f32x4 Gs1[4];
    mlp_layer_T<4, 4, 0, 4>(R::w(lds, LS1), Gs2, Gs1, lane);
    relu_mask_(Gs1, s1);
    dw_accumulate<4, 1>(scr, Gs1, h, accA, bsA, lane);   // input = detached geo: no dX unless SEMGRAD
    if constexpr (SEMGRAD) {
      f32x4 Gh[1];
      mlp_layer_T<4, 1, 0, 1>(R::w(lds, LS0), Gs1, Gh, lane);
      if (g == 0) Gh[0][0] = 0.0f;  // the density logit is not an input of mlp_semantics
      if (valid) {
        float* const d_h = only(d_h_semgrad...);
        f32x4* row = reinterpret_cast<f32x4*>(d_h + (size_t)n * 16 + 4 * g);
        *row = *row + Gh[0];
      }
    }
  }

  const int lane = lane0;
  __syncthreads();
  float* acc_lds = R::w(lds, LS0);
  constexpr int ACC_FLOATS = Cfg::woff(LH + 1) - Cfg::woff(LS0);
  static_assert(LS1 == LS0 + 1 && LH == LS1 + 1, "the branch's layers are adjacent in the image");
  for (int i = threadIdx.x; i < ACC_FLOATS; i += blockDim.x) acc_lds[i] = 0.0f;
  __syncthreads();
  for (int turn = 0; turn < WAVES; ++turn) {
    if (wave == turn) {
      flush_dw<4, 1>(R::w(lds, LS0), accA, lane);
      flush_dw<4, 4>(R::w(lds, LS1), accB, lane);
      flush_dw<1, 4>(R::w(lds, LH), accC, lane);
      lds_bias[lane] += bsA;
      lds_bias[64 + lane] += bsB;
      if (lane < 16) lds_bias[128 + lane] += bsC;
    }
    __syncthreads();
  }
  float* part = partials + (size_t)blockIdx.x * (Cfg::W_TOTAL + Cfg::B_TOTAL);
  for (int i = threadIdx.x; i < ACC_FLOATS; i += blockDim.x) part[Cfg::woff(LS0) + i] = acc_lds[i];
  for (int i = threadIdx.x; i < 144; i += blockDim.x) part[Cfg::W_TOTAL + Cfg::boff(LS0) + i] = lds_bias[i];
}

// ---- semantic branch, `fruit_nerf_big` shape: 30 -> 128 -> 128 -> 64 -> head, two launches (see the file header) ----
// PHASE_A: dW/db of sem0, sem2 and the head;  PHASE_B: dW/db of sem1 (the 128 x 128 layer).
// SEMGRAD (see k_field_mlp_bwd_sem): PHASE_A, which holds Gs1, owns the dX of sem0.
template <class Cfg, bool PHASE_A, int WAVES, bool SEMGRAD = false, class... DH>
__global__ __launch_bounds__(64 * WAVES, 1) void k_field_mlp_bwd_sem_big(
    const float* __restrict__ packed, long long N, const float* __restrict__ h_saved,
    const float* __restrict__ d_logit, float* __restrict__ partials, DH... d_h_semgrad) {  // SEMGRAD: float* d_h
  static_assert(sizeof...(DH) == (SEMGRAD ? 1 : 0), "d_h comes with SEMGRAD");
  static_assert(PHASE_A || !SEMGRAD, "the input gradient of mlp_semantics belongs to phase A");
  static_assert(Cfg::NSEM == 3 && Cfg::HB == 2 && Cfg::SEMB == 8, "fruit_nerf_big semantic shape");
  using R = typename BwdRange<Cfg, PHASE_A ? BR_SEM_A : BR_SEM_B>::type;
  constexpr int LS0 = Cfg::L_SEM0, LS1 = Cfg::L_SEM1, LS2 = Cfg::L_SEM2, LH = Cfg::L_HEAD;
  constexpr int NBIAS = PHASE_A ? 128 + 64 + 16 : 128;
  __shared__ __attribute__((aligned(16))) float lds[R::FLOATS + WAVES * SCR_FLOATS + NBIAS];
  float* scr_all = lds + R::FLOATS;
  float* lds_bias = scr_all + WAVES * SCR_FLOATS;
  R::template stage<64 * WAVES>(lds, packed);
  for (int i = threadIdx.x; i < NBIAS; i += blockDim.x) lds_bias[i] = 0.0f;
  __syncthreads();
  const int lane0 = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* scr = scr_all + wave * SCR_FLOATS;

  // PHASE_A: acc0 = sem0 [8][2], acc2 = sem2 [4][8], accH = head [1][4];  PHASE_B: acc1 = sem1 [8][8]
  f32x4 acc0[PHASE_A ? 8 : 1][PHASE_A ? 2 : 1];
  f32x4 acc2[PHASE_A ? 4 : 1][PHASE_A ? 8 : 1];
  f32x4 accH[1][PHASE_A ? 4 : 1];
  f32x4 acc1[PHASE_A ? 1 : 8][PHASE_A ? 1 : 8];
  float bs_lo = 0.0f, bs_hi = 0.0f;  // rows 0..63 / 64..127 of the 128-wide layer this phase owns (sem0 | sem1)
  float bs2 = 0.0f, bsH = 0.0f;
  zero_acc(acc0);
  zero_acc(acc1);
  zero_acc(acc2);
  zero_acc(accH);

  const long long n_tiles = (N + 15) / 16;
  for (long long tile = (long long)blockIdx.x * WAVES + wave; tile < n_tiles; tile += (long long)gridDim.x * WAVES) {
    asm volatile("" ::: "memory");
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int j = lane & 15, g = lane >> 4;
    const long long n = tile * 16 + j;
    const bool valid = n < N;
    const long long nn = valid ? n : N - 1;
    f32x4 h[2];
    h[0] = *reinterpret_cast<const f32x4*>(h_saved + (size_t)nn * 32 + 4 * g);
    h[1] = *reinterpret_cast<const f32x4*>(h_saved + (size_t)nn * 32 + 16 + 4 * g);
    f32x4 s1[8], s2[8];
    mlp_layer<8, 2>(R::w(lds, LS0), R::b(lds, LS0), h, s1, lane);
    relu_(s1);
    mlp_layer<8, 8>(R::w(lds, LS1), R::b(lds, LS1), s1, s2, lane);
    relu_(s2);
    f32x4 Gl[1];
    Gl[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (g == 0 && valid) Gl[0][0] = d_logit[n];
    f32x4 Gs3[4];
    mlp_layer_T<1, 4, 0, 4>(R::w(lds, LH), Gl, Gs3, lane);  // no activation on mlp_semantics' last layer
    if constexpr (PHASE_A) {
      f32x4 s3[4];
      mlp_layer<4, 8>(R::w(lds, LS2), R::b(lds, LS2), s2, s3, lane);
      dw_accumulate<1, 4>(scr, Gl, s3, accH, bsH, lane);  // SemanticFieldHead
      dw_accumulate_sub<4, 4, 4, 8, 0, 0, true>(scr, Gs3, s2, acc2, bs2, lane);
      dw_accumulate_sub<4, 4, 4, 8, 0, 4, false>(scr, Gs3, s2 + 4, acc2, bs2, lane);
    }
    f32x4 Gs2[8];
    mlp_layer_T<4, 8, 0, 8>(R::w(lds, LS2), Gs3, Gs2, lane);
    relu_mask_(Gs2, s2);
    if constexpr (PHASE_A) {
      f32x4 Gs1[8];
      mlp_layer_T<8, 8, 0, 8>(R::w(lds, LS1), Gs2, Gs1, lane);
      relu_mask_(Gs1, s1);
      dw_accumulate_sub<4, 2, 8, 2, 0, 0, true>(scr, Gs1, h, acc0, bs_lo, lane);  // input = detached geo: no dX unless SEMGRAD
      dw_accumulate_sub<4, 2, 8, 2, 4, 0, true>(scr, Gs1 + 4, h, acc0, bs_hi, lane);
      if constexpr (SEMGRAD) {
        f32x4 Gh[2];
        mlp_layer_T<8, 2, 0, 2>(R::w(lds, LS0), Gs1, Gh, lane);
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
    } else {
      dw_accumulate_sub<4, 4, 8, 8, 0, 0, true>(scr, Gs2, s1, acc1, bs_lo, lane);
      dw_accumulate_sub<4, 4, 8, 8, 0, 4, false>(scr, Gs2, s1 + 4, acc1, bs_lo, lane);
      dw_accumulate_sub<4, 4, 8, 8, 4, 0, true>(scr, Gs2 + 4, s1, acc1, bs_hi, lane);
      dw_accumulate_sub<4, 4, 8, 8, 4, 4, false>(scr, Gs2 + 4, s1 + 4, acc1, bs_hi, lane);
    }
  }

  const int lane = lane0;
  __syncthreads();
  float* part = partials + (size_t)blockIdx.x * (Cfg::W_TOTAL + Cfg::B_TOTAL);
  if constexpr (PHASE_A) {
    for (int i = threadIdx.x; i < Cfg::nob(LS0) * Cfg::nib(LS0) * 256; i += blockDim.x) R::w(lds, LS0)[i] = 0.0f;
    for (int i = threadIdx.x; i < Cfg::woff(LH + 1) - Cfg::woff(LS2); i += blockDim.x) R::w(lds, LS2)[i] = 0.0f;
    static_assert(LH == LS2 + 1, "sem2 and the head are adjacent in the image");
    __syncthreads();
    for (int turn = 0; turn < WAVES; ++turn) {
      if (wave == turn) {
        flush_dw<8, 2>(R::w(lds, LS0), acc0, lane);
        flush_dw<4, 8>(R::w(lds, LS2), acc2, lane);
        flush_dw<1, 4>(R::w(lds, LH), accH, lane);
        lds_bias[lane] += bs_lo;
        lds_bias[64 + lane] += bs_hi;
        lds_bias[128 + lane] += bs2;
        if (lane < 16) lds_bias[192 + lane] += bsH;
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < Cfg::nob(LS0) * Cfg::nib(LS0) * 256; i += blockDim.x)
      part[Cfg::woff(LS0) + i] = R::w(lds, LS0)[i];
    for (int i = threadIdx.x; i < Cfg::woff(LH + 1) - Cfg::woff(LS2); i += blockDim.x)
      part[Cfg::woff(LS2) + i] = R::w(lds, LS2)[i];
    for (int i = threadIdx.x; i < 128; i += blockDim.x) part[Cfg::W_TOTAL + Cfg::boff(LS0) + i] = lds_bias[i];
    for (int i = threadIdx.x; i < 64; i += blockDim.x) part[Cfg::W_TOTAL + Cfg::boff(LS2) + i] = lds_bias[128 + i];
    for (int i = threadIdx.x; i < 16; i += blockDim.x) part[Cfg::W_TOTAL + Cfg::boff(LH) + i] = lds_bias[192 + i];
  } else {
    for (int i = threadIdx.x; i < Cfg::nob(LS1) * Cfg::nib(LS1) * 256; i += blockDim.x) R::w(lds, LS1)[i] = 0.0f;
    __syncthreads();
    for (int turn = 0; turn < WAVES; ++turn) {
      if (wave == turn) {
        flush_dw<8, 8>(R::w(lds, LS1), acc1, lane);
        lds_bias[lane] += bs_lo;
        lds_bias[64 + lane] += bs_hi;
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < Cfg::nob(LS1) * Cfg::nib(LS1) * 256; i += blockDim.x)
      part[Cfg::woff(LS1) + i] = R::w(lds, LS1)[i];
    for (int i = threadIdx.x; i < 128; i += blockDim.x) part[Cfg::W_TOTAL + Cfg::boff(LS1) + i] = lds_bias[i];
  }
}

// one branch (every branch runs a.blocks workgroups: one partial-image buffer); semgrad: the SEMGRAD kernel takes d_h too
template <class Cfg>
static int launch(int branch, const FieldBwdArgs& a) {
  const dim3 grid((unsigned)a.blocks);
  if (branch == BR_COLOR) {
    hipLaunchKernelGGL((k_field_mlp_bwd_color<Cfg, 8>), grid, dim3(512), 0, a.st, a.packed, a.ray_bias, a.rd, a.S, a.N, a.h_saved,
                       a.d_rgb, a.d_h, a.gsum_tile, a.gsum_extra, a.partials);
  } else if (branch == BR_BASE) {
    hipLaunchKernelGGL((k_field_mlp_bwd_base<Cfg, 8>), grid, dim3(512), 0, a.st, a.packed, a.N, a.feats, a.selector, a.d_density,
                       a.d_h, a.d_feats, a.partials);
  } else if constexpr (Cfg::NSEM == 2) {
    if (a.semgrad)
      hipLaunchKernelGGL((k_field_mlp_bwd_sem<Cfg, 8, true, float*>), grid, dim3(512), 0, a.st, a.packed, a.N, a.h_saved,
                         a.d_logit, a.partials, a.d_h);
    else
      hipLaunchKernelGGL((k_field_mlp_bwd_sem<Cfg, 8>), grid, dim3(512), 0, a.st, a.packed, a.N, a.h_saved, a.d_logit,
                         a.partials);
  } else {
    if (a.semgrad)
      hipLaunchKernelGGL((k_field_mlp_bwd_sem_big<Cfg, true, 4, true, float*>), grid, dim3(256), 0, a.st, a.packed, a.N,
                         a.h_saved, a.d_logit, a.partials, a.d_h);
    else
      hipLaunchKernelGGL((k_field_mlp_bwd_sem_big<Cfg, true, 4>), grid, dim3(256), 0, a.st, a.packed, a.N, a.h_saved, a.d_logit,
                         a.partials);
    FNR_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_field_mlp_bwd_sem_big<Cfg, false, 4>), grid, dim3(256), 0, a.st, a.packed, a.N, a.h_saved, a.d_logit,
                       a.partials);
  }
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

int field_mlp_bwd_fp32(int branch, const FieldBwdArgs& a) {
  return a.cfg == 0 ? launch<FieldCfgBase>(branch, a) : launch<FieldCfgBig>(branch, a);
}

}  // namespace fnr

