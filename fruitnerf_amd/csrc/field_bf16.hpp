// field_bf16.hpp — FruitField's MLP stack (fruit_field.py:132-166) on the gfx950 bf16 matrix pipe
// (v_mfma_f32_16x16x32_bf16, fp32 accumulate), as ONE kernel family with a compile-time split count NS:
//
//   NS = 1  "bf16":    operands rounded to bf16 (8 significant bits) — the mode BASELINE config 2 names; NOT parity
//                      grade (outputs ~1e-2 relative), judged at matched PSNR / IoU.
//   NS = 3  "bf16x3":  every fp32 operand x is split EXACTLY into three bf16 pieces x = x1 + x2 + x3 (x1 = bf16(x),
//                      x2 = bf16(x - x1), x3 = bf16(x - x1 - x2); 3 x 8 significant bits cover the 24 of fp32) and the
//                      product is formed from the six piece products whose weight is above fp32 rounding,
//                          w x  ~=  w1 x1 + (w1 x2 + w2 x1) + (w1 x3 + w2 x2 + w3 x1)        (dropped terms <= 2^-27 |w x|),
//                      each exact in the fp32 accumulator.  fp32-grade results (~1e-6, against the 1e-4 bar) at 6 bf16
//                      MFMAs per fp32-equivalent K-block: the fp32 MFMA runs at 1/16 of the bf16 rate on gfx950
//                      (MI355X_MICROARCH: 157 vs 2500 TFLOP/s), so this is 16/6 = 2.7x the fp32-MFMA roofline.
//   NS = 2             three products (w1 x1 + w1 x2 + w2 x1, error 2^-17): used by the bf16x3 mode for the BACKWARD
//                      pass, whose bar is 5e-4 of max |g|.
//
// Formulation (per pair of 16-sample tiles, one wave), transposed like the fp32 path (field_layers.hpp):
//     Y^T[out][sample] = W[out][in] X^T[in][sample],     A = W fragment (LDS), B = X^T fragment (registers)
//   A[i][k]: lane l supplies i = l&15 and the 8 K-slots (g = l>>4, e = 0..7);  B[k][j]: same slots, j = l&15;
//   D[row][col]: lane l holds col = l&15, rows 4 g + r.
// A K-block covers two 16-wide input blocks; slot (g, e) is input block 2 kb + (e >> 2), element 4 g + (e & 3) of it:
// exactly the 8 accumulator values lane (g, j) holds for those two blocks, so the accumulator of layer n becomes the
// B operand of layer n+1 with a conversion and no data movement.  (The hardware's own k numbering inside a lane
// group is irrelevant: A and B agree on the slot -> k map and the sum over k is order-free.)
// Both tiles of the pair share every A fragment: one ds_read_b128 feeds 2 NS(NS+1)/2 MFMAs.
#pragma once
#include "field_layers.hpp"

namespace fnr {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x8 = __attribute__((ext_vector_type(8))) float;

enum { MLP_FP32 = 0, MLP_BF16 = 1, MLP_BF16X3 = 3 };

// ---- fragment image: [piece][block][64 lanes] x bf16x8 ----------------------------------------------------------
// forward blocks of layer l: (ob, kb) -> W[16 ob + i][col(2 kb + (e>>2), g, e&3)]
// transposed blocks of layer l (dX^T = W^T dY^T): (ib, kbT) -> W[16 (2 kbT + (e>>2)) + 4 g + (e&3)][col(ib, i>>2, i&3)]
template <class Cfg>
struct BfImage {
  static constexpr int NL = Cfg::NLAYERS;
  // mlp_head layer 0 only multiplies the h blocks per sample (per-ray factoring, field_layers.hpp: color_layer0)
  static constexpr int nib_used(int l) { return l == Cfg::L_COL0 ? Cfg::HB : Cfg::nib(l); }
  static constexpr int nkb(int l) { return (nib_used(l) + 1) / 2; }
  static constexpr int nkbT(int l) { return (Cfg::nob(l) + 1) / 2; }
  // mlp_semantics' input is detached: no dX — unless pass_semantic_gradients, whose kernels build the transposed fragments of
  // sem0 themselves (bf_build_T) and leave this image as it is
  static constexpr bool hasT(int l) { return l != Cfg::L_SEM0; }
  static constexpr int fblocks(int l) { return Cfg::nob(l) * nkb(l); }
  static constexpr int tblocks(int l) { return hasT(l) ? nib_used(l) * nkbT(l) : 0; }
  static constexpr int foff(int l) {
    int o = 0;
    for (int i = 0; i < l; ++i) o += fblocks(i);
    return o;
  }
  static constexpr int F_TOTAL = foff(NL);
  static constexpr int toff(int l) {
    int o = F_TOTAL;
    for (int i = 0; i < l; ++i) o += tblocks(i);
    return o;
  }
  static constexpr int BLOCKS = toff(NL);
  static constexpr size_t piece_elems() { return (size_t)BLOCKS * 64 * 8; }
  static constexpr size_t bytes(int ns) { return (size_t)ns * piece_elems() * 2; }
};
constexpr int BF_MAX_PIECES = 3;

// piece p of the exact bf16 split of w (p < 3)
__device__ __forceinline__ __bf16 bf_piece(float w, int p) {
  const __bf16 a = (__bf16)w;
  if (p == 0) return a;
  const float r1 = w - (float)a;
  const __bf16 b = (__bf16)r1;
  if (p == 1) return b;
  return (__bf16)(r1 - (float)b);
}

template <class Cfg>
__device__ __forceinline__ void pack_field_weights_bf16_block(const FieldPtrs& p, int ns, __bf16* __restrict__ image,
                                                              int block) {
  using Img = BfImage<Cfg>;
  const int idx = block * 256 + threadIdx.x;  // (block, lane)
  if (idx >= Img::BLOCKS * 64) return;
  const int blk = idx >> 6, lane = idx & 63;
  const int i = lane & 15, g = lane >> 4;
  float w[8];
  if (blk < Img::F_TOTAL) {
    int l = 0;
#pragma unroll
    for (int q = 1; q < Cfg::NLAYERS; ++q)
      if (blk >= Img::foff(q)) l = q;
    const int local = blk - Img::foff(l);
    const int nkb = Img::nkb(l), kb = local % nkb, ob = local / nkb;
    const int out = 16 * ob + i;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ib = 2 * kb + (e >> 2);
      const int col = (ib < Img::nib_used(l)) ? kmap<Cfg>(Cfg::km(l), ib, g, e & 3, Cfg::in_dim(l)) : -1;
      w[e] = (out < Cfg::out_dim(l) && col >= 0) ? p.w[l][out * Cfg::in_dim(l) + col] : 0.0f;
    }
  } else {
    int l = 0;
#pragma unroll
    for (int q = 1; q < Cfg::NLAYERS; ++q)
      if (blk >= Img::toff(q)) l = q;
    const int local = blk - Img::toff(l);
    const int nk = Img::nkbT(l), kb = local % nk, ib = local / nk;
    const int col = kmap<Cfg>(Cfg::km(l), ib, i >> 2, i & 3, Cfg::in_dim(l));
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ob = 2 * kb + (e >> 2);
      const int out = 16 * ob + 4 * g + (e & 3);
      w[e] = (ob < Cfg::nob(l) && out < Cfg::out_dim(l) && col >= 0) ? p.w[l][out * Cfg::in_dim(l) + col] : 0.0f;
    }
  }
  for (int pc = 0; pc < ns; ++pc) {
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = bf_piece(w[e], pc);
    reinterpret_cast<bf16x8*>(image)[(size_t)pc * Img::BLOCKS * 64 + idx] = v;
  }
}

template <class Cfg>
constexpr int pack_field_weights_bf16_blocks() { return (BfImage<Cfg>::BLOCKS * 64 + 255) / 256; }

// the launch of k_pack_field_weights_bf16 (the bf16 pieces of the fragment image): field_mlp.hip, like launch_pack_field_weights
template <class Cfg>
void launch_pack_field_weights_bf16(const FieldPtrs& p, int ns, __bf16* image, hipStream_t st);

// ---- what a kernel keeps in LDS: an ordered list of (layer, forward | transposed) segments, NS pieces each -------
// Segs: struct with  static constexpr int N;  static constexpr int layer(int i);  static constexpr bool isT(int i);
template <class Cfg, class Segs, int NS>
struct BfLds {
  using Img = BfImage<Cfg>;
  static constexpr int blocks(int s) { return Segs::isT(s) ? Img::tblocks(Segs::layer(s)) : Img::fblocks(Segs::layer(s)); }
  static constexpr int off(int s) {  // in fragments of 64 x bf16x8 (1 KiB)
    int o = 0;
    for (int i = 0; i < s; ++i) o += blocks(i) * NS;
    return o;
  }
  static constexpr int FRAGS = off(Segs::N);
  static constexpr int BYTES = FRAGS * 1024;
  static constexpr int find(int layer, bool isT) {
    for (int i = 0; i < Segs::N; ++i)
      if (Segs::layer(i) == layer && Segs::isT(i) == isT) return i;
    return -1;
  }
  // first fragment (piece 0, block 0) of a segment; piece p starts blocks() fragments later
  template <int LAYER, bool IS_T>
  __device__ static __forceinline__ const bf16x8* seg(const bf16x8* lds) {
    constexpr int s = find(LAYER, IS_T);
    static_assert(s >= 0, "layer not staged by this kernel");
    return lds + off(s) * 64;
  }
  template <int LAYER, bool IS_T>
  static constexpr int seg_blocks() { return blocks(find(LAYER, IS_T)); }
  // global image -> LDS.  The LDS layout is the concatenation of the (segment, piece) chunks, each contiguous in the
  // global image too: flat LDS vector f comes from global vector f + delta(chunk of f).  All loads of a thread are
  // issued before its first LDS store (see stage_copy in field_layers.hpp).
  static constexpr int chunk_begin(int c) { return off(c / NS) * 64 + (c % NS) * blocks(c / NS) * 64; }
  static constexpr long long chunk_src(int c) {
    const int s = c / NS, pc = c % NS;
    return (long long)pc * Img::BLOCKS * 64 + (Segs::isT(s) ? Img::toff(Segs::layer(s)) : Img::foff(Segs::layer(s))) * 64;
  }
  template <int THREADS>
  __device__ static __forceinline__ void stage(bf16x8* __restrict__ lds, const __bf16* __restrict__ image) {
    constexpr int T = FRAGS * 64, NCH = Segs::N * NS;
    constexpr int PER = (T + THREADS - 1) / THREADS;
    static_assert(PER <= 32, "staging batch too large");
    const f32x4* img = reinterpret_cast<const f32x4*>(image);
    f32x4* dst = reinterpret_cast<f32x4*>(lds);
    f32x4 v[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int f = (int)threadIdx.x + u * THREADS;
      long long delta = chunk_src(0) - chunk_begin(0);
#pragma unroll
      for (int c = 1; c < NCH; ++c) delta = (f >= chunk_begin(c)) ? chunk_src(c) - chunk_begin(c) : delta;
      if (f < T) v[u] = img[f + delta];
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int f = (int)threadIdx.x + u * THREADS;
      if (f < T) dst[f] = v[u];
    }
  }
};

// The transposed segment of layer L ([piece][ib * nkbT + kb][64 lanes], what BfLds::seg<L, true> would point at) built in LDS
// from the fp32 fragment image `packed` by a workgroup of THREADS threads: the same values and the same split as
// pack_field_weights_bf16_block's transposed branch.  For the one layer whose transposed blocks the bf16 image does not carry
// (L_SEM0), used by the pass_semantic_gradients kernels only.  The caller puts a barrier on both sides.
template <class Cfg, int L, int NS, int THREADS>
__device__ __forceinline__ void bf_build_T(bf16x8* __restrict__ lds, const float* __restrict__ packed) {
  constexpr int NIB = Cfg::nib(L), NKT = (Cfg::nob(L) + 1) / 2, TB = NIB * NKT;
  for (int idx = threadIdx.x; idx < TB * 64; idx += THREADS) {
    const int blk = idx >> 6, lane = idx & 63;
    const int i = lane & 15, g = lane >> 4;
    const int kb = blk % NKT, ib = blk / NKT;
    float w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ob = 2 * kb + (e >> 2), row = 4 * g + (e & 3);  // W[16 ob + row][col(ib, i >> 2, i & 3)] in the fp32 image
      w[e] = ob < Cfg::nob(L) ? packed[Cfg::woff(L) + ((ob * NIB + ib) * 64 + swz_slot(row, i >> 2)) * 4 + (i & 3)] : 0.0f;
    }
#pragma unroll
    for (int pc = 0; pc < NS; ++pc) {
      bf16x8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = bf_piece(w[e], pc);
      lds[pc * TB * 64 + idx] = v;
    }
  }
}

// ---- operands ---------------------------------------------------------------------------------------------------
// Two floats -> one dword of two bf16 (round to nearest even), ONE instruction: the TWO-wide vector conversion is what hipcc
// turns into a single v_cvt_pk_bf16_f32 with both sources.  The eight-wide __builtin_convertvector(f32x8 -> bf16x8) becomes one
// v_cvt_pk_bf16_f32 per VALUE (second source unused) plus a v_perm_b32 per pair to pack: 3.5 instructions per value and piece
// where 2.5 do (round 6: the MLP kernels are vector-ALU bound, not MFMA bound — 14.7 M vector against 2.5 M matrix
// wave-instructions in the forward kernel; profiles/r06_raw/per_wave_mlp_bwd.md).  No inline assembly: the compiler keeps
// seeing the instruction (hazards, constant folding).
using bf_f32x2 = __attribute__((ext_vector_type(2))) float;
using bf_bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
  const bf_f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf_bf16x2));
}
using bf_u32x4 = __attribute__((ext_vector_type(4))) unsigned;
// the exact split x = x1 + x2 + x3 of eight values, pairwise: same roundings (same bits) as the scalar form bf_piece
template <int NS>
__device__ __forceinline__ void bf_split(const f32x8 v, bf16x8 (&p)[NS]) {
  bf_u32x4 out[NS];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    float a = v[2 * d], b = v[2 * d + 1];
#pragma unroll
    for (int pc = 0; pc < NS; ++pc) {
      const unsigned w = cvt_pk_bf16(a, b);
      out[pc][d] = w;
      if (pc + 1 < NS) {
        a -= __builtin_bit_cast(float, w << 16);
        b -= __builtin_bit_cast(float, w & 0xffff0000u);
      }
    }
  }
#pragma unroll
  for (int pc = 0; pc < NS; ++pc) p[pc] = __builtin_bit_cast(bf16x8, out[pc]);
}
// ... of four values (the upper half of the K-block is structurally zero)
template <int NS>
__device__ __forceinline__ void bf_split_half(const f32x4 v, bf16x8 (&p)[NS]) {
  bf_u32x4 out[NS];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    float a = v[2 * d], b = v[2 * d + 1];
#pragma unroll
    for (int pc = 0; pc < NS; ++pc) {
      const unsigned w = cvt_pk_bf16(a, b);
      out[pc][d] = w;
      if (pc + 1 < NS) {
        a -= __builtin_bit_cast(float, w << 16);
        b -= __builtin_bit_cast(float, w & 0xffff0000u);
      }
    }
  }
#pragma unroll
  for (int pc = 0; pc < NS; ++pc) {
    out[pc][2] = out[pc][3] = 0u;
    p[pc] = __builtin_bit_cast(bf16x8, out[pc]);
  }
}

// B operand pieces of an activation held as NB accumulator blocks (C layout): K-block kb = blocks 2 kb, 2 kb + 1
template <int NS, int NB>
__device__ __forceinline__ void bf_operand(const f32x4 (&act)[NB], bf16x8 (&x)[(NB + 1) / 2][NS]) {
#pragma unroll
  for (int kb = 0; kb < (NB + 1) / 2; ++kb) {
    if (2 * kb + 1 < NB) {
      f32x8 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = act[2 * kb][e];
        v[4 + e] = act[(2 * kb + 1 < NB) ? 2 * kb + 1 : 0][e];
      }
      bf_split<NS>(v, x[kb]);
    } else {
      bf_split_half<NS>(act[2 * kb], x[kb]);
    }
  }
}

// out (NOB accumulator blocks, both tiles of the pair) += W * X.  `seg` = the layer's segment in LDS
// ([piece][NOB * NKB blocks][64]); works for forward (W) and transposed (W^T) segments alike.
template <int NS, int NOB, int NKB>
__device__ __forceinline__ void bf_layer_acc(const bf16x8* __restrict__ seg, const bf16x8 (&xa)[NKB][NS],
                                             const bf16x8 (&xb)[NKB][NS], f32x4 (&oa)[NOB], f32x4 (&ob_)[NOB], int lane) {
  constexpr int PB = NOB * NKB * 64;  // fragments' stride between pieces
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) {
      bf16x8 w[NS];
#pragma unroll
      for (int pc = 0; pc < NS; ++pc) w[pc] = seg[pc * PB + (ob * NKB + kb) * 64 + lane];
      // smallest terms first
#pragma unroll
      for (int s = NS - 1; s >= 0; --s)
#pragma unroll
        for (int pw = 0; pw <= s; ++pw) {
          oa[ob] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[pw], xa[kb][s - pw], oa[ob], 0, 0, 0);
          ob_[ob] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[pw], xb[kb][s - pw], ob_[ob], 0, 0, 0);
        }
    }
  }
}

// one layer on the tile pair: out = W in + b (bias from the fp32 fragment image's bias block `B`)
template <int NS, int NOB, int NIB>
__device__ __forceinline__ void bf_layer(const bf16x8* __restrict__ seg, const float* __restrict__ B,
                                         const f32x4 (&ina)[NIB], const f32x4 (&inb)[NIB], f32x4 (&oa)[NOB],
                                         f32x4 (&ob_)[NOB], int lane) {
  const int g = lane >> 4;
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob) oa[ob] = ob_[ob] = *reinterpret_cast<const f32x4*>(B + 16 * ob + 4 * g);
  bf16x8 xa[(NIB + 1) / 2][NS], xb[(NIB + 1) / 2][NS];
  bf_operand<NS, NIB>(ina, xa);
  bf_operand<NS, NIB>(inb, xb);
  bf_layer_acc<NS, NOB, (NIB + 1) / 2>(seg, xa, xb, oa, ob_, lane);
}

// out = W^T G (no bias): NIBO input blocks of the layer from its NOB output-gradient blocks
template <int NS, int NIBO, int NOB>
__device__ __forceinline__ void bf_layer_T(const bf16x8* __restrict__ segT, const f32x4 (&Ga)[NOB], const f32x4 (&Gb)[NOB],
                                           f32x4 (&oa)[NIBO], f32x4 (&ob_)[NIBO], int lane) {
#pragma unroll
  for (int ib = 0; ib < NIBO; ++ib) oa[ib] = ob_[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 xa[(NOB + 1) / 2][NS], xb[(NOB + 1) / 2][NS];
  bf_operand<NS, NOB>(Ga, xa);
  bf_operand<NS, NOB>(Gb, xb);
  bf_layer_acc<NS, NIBO, (NOB + 1) / 2>(segT, xa, xb, oa, ob_, lane);
}

// ---- single-tile variants (one 16-sample tile per wave: kernels whose activations are 128 wide) -------------------
template <int NS, int NOB, int NKB>
__device__ __forceinline__ void bf_layer_acc1(const bf16x8* __restrict__ seg, const bf16x8 (&x)[NKB][NS], f32x4 (&o)[NOB],
                                              int lane) {
  constexpr int PB = NOB * NKB * 64, T = NOB * NKB;
  // explicit double buffer over the (kb, ob) steps, pinned by scheduling barriers: left alone, the scheduler hoists
  // the LDS reads of MANY steps above the MFMAs (8 registers per step) and the 128-wide layers spill
  bf16x8 w[2][NS];
  auto load = [&](int t, bf16x8 (&dst)[NS]) {
    const int kb = t / NOB, ob = t % NOB;
#pragma unroll
    for (int pc = 0; pc < NS; ++pc) dst[pc] = seg[pc * PB + (ob * NKB + kb) * 64 + lane];
  };
  load(0, w[0]);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (t + 1 < T) load(t + 1, w[(t + 1) & 1]);
    const int kb = t / NOB, ob = t % NOB;
#pragma unroll
    for (int s = NS - 1; s >= 0; --s)
#pragma unroll
      for (int pw = 0; pw <= s; ++pw)
        o[ob] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[t & 1][pw], x[kb][s - pw], o[ob], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}
template <int NS, int NOB, int NIB>
__device__ __forceinline__ void bf_layer1(const bf16x8* __restrict__ seg, const float* __restrict__ B,
                                          const f32x4 (&in)[NIB], f32x4 (&o)[NOB], int lane) {
  const int g = lane >> 4;
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob) o[ob] = *reinterpret_cast<const f32x4*>(B + 16 * ob + 4 * g);
  bf16x8 x[(NIB + 1) / 2][NS];
  bf_operand<NS, NIB>(in, x);
  bf_layer_acc1<NS, NOB, (NIB + 1) / 2>(seg, x, o, lane);
}
template <int NS, int NIBO, int NOB>
__device__ __forceinline__ void bf_layer_T1(const bf16x8* __restrict__ segT, const f32x4 (&G)[NOB], f32x4 (&o)[NIBO],
                                            int lane) {
#pragma unroll
  for (int ib = 0; ib < NIBO; ++ib) o[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 x[(NOB + 1) / 2][NS];
  bf_operand<NS, NOB>(G, x);
  bf_layer_acc1<NS, NIBO, (NOB + 1) / 2>(segT, x, o, lane);
}

// ---- host entry points of the bf16-pipe modes (fnr_field_net.mlp_mode != 0), forward: called from field_mlp.hip ----------
// cfg: 0 `fruit_nerf`, 1 `fruit_nerf_big`; mode: MLP_BF16 | MLP_BF16X3; image_ws: the fragment image the caller has packed
// (k_prepare_field / launch_pack_field_weights_bf16), field_bf16_image_bytes() covers both shapes at BF_MAX_PIECES.
size_t field_bf16_image_bytes();  // field_mlp_bf16.hip, like the next two
int field_mlp_fwd_bf16(int cfg, int mode, const FieldPtrs& p, const float* packed, void* image_ws, const float* ray_bias,
                       const RaysDev& rd, int S, long long N, const float2* feats, const uint8_t* selector, float* density,
                       float* rgb, float* logit, float* geo_out, float* h_buf, hipStream_t st);
int field_mlp_fwd_sem_big_bf16(int mode, const FieldPtrs& p, void* image_ws, const float* packed, long long N,
                               const float* h_buf, float* logit, hipStream_t st);

// ---- the backward: one argument block for the whole family, host side only (the kernels keep their loose pointer parameters).
// field_mlp_bwd_entry (field_mlp_bwd.hip) validates the call and fills it once; the launch path and the launchers below take it.
struct WeightAdam;  // adam.hpp
struct FieldBwdArgs {
  int cfg, mode;             // 0 `fruit_nerf` | 1 `fruit_nerf_big`; FNR_MLP_FP32 | FNR_MLP_BF16 | FNR_MLP_BF16X3
  FieldPtrs p, gp;           // the nn.Linear tensors and their gradients
  const float* embedding;    // appearance embedding [n_images, 32] and its gradient
  float* g_embedding;
  int n_images, n_levels;
  const WeightAdam* wadam;   // NULL: gradients are added into gp / g_embedding; else the weight finish takes the optimiser step
  const float* packed;       // fp32 fragment image: the forward pass's (saved) or the workspace's (pack_images)
  const __bf16* image;       // ... and its bf16 pieces
  const float* ray_bias;     // saved by the forward pass, or the workspace's (make_ray_bias)
  bool pack_images, make_ray_bias, semgrad;  // semgrad (pass_semantic_gradients): the semantic branch adds its dX into d_h
  RaysDev rd;
  int S;
  long long N;
  const float2* feats;
  const float* h_saved;
  const uint8_t* selector;
  const float *d_density, *d_rgb, *d_logit;
  float2* d_feats;
  float *d_h, *gsum_tile, *gsum_extra, *g_ray, *partials;  // gsum_extra: NULL unless tiles straddle rays (S % 16 != 0)
  long long blocks;          // workgroups = partial images, the same for every branch
  const float2* jac;         // the encode's input Jacobian and the position gradient: both or neither
  float4* d_pos;
  hipStream_t st;
};
// One launcher per arithmetic, one branch per call.  BR_SEM_DX (`fruit_nerf`, bf16 modes, semgrad): d_h += the input gradient
// of mlp_semantics, a kernel of its own ahead of BR_SEM; everywhere else the semantic kernel forms it itself.
enum { BR_COLOR = 0, BR_SEM = 1, BR_BASE = 2, BR_SEM_DX = 3 };
int field_mlp_bwd_fp32(int branch, const FieldBwdArgs& a);  // field_mlp_bwd_fp32.hip; `fruit_nerf_big`'s BR_SEM is two launches
// bf16 modes, every branch but `fruit_nerf_big`'s BR_SEM; with a.jac, BR_BASE also writes the position gradient
int field_mlp_bwd_pw(int branch, const FieldBwdArgs& a);    // field_mlp_bwd_pw.hip
int field_mlp_bwd_sem_big_bf16(const FieldBwdArgs& a);      // bf16 modes, `fruit_nerf_big`'s BR_SEM: field_mlp_bf16.hip

}  // namespace fnr
