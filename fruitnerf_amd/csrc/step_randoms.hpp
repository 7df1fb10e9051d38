// step_randoms.hpp — the counter-based random numbers of a training step (Philox4x32-10, Salmon et al. 2011), shared by
// pixel_sampler.hip (the prologue's numbers, the random backgrounds, the per-edge jitter of level 0) and sampler.hip (the
// per-edge jitter of the PDF levels).  counter = (ray, word group, step offset), key = seed: every kernel derives the numbers
// it consumes itself, nothing is written to memory for another launch to read.
#pragma once
#include "common.hpp"

namespace fnr {

__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0, c[1] = lo1, c[2] = n2, c[3] = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
}
__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-08f; }  // [0, 1), 24 bits
// the step's random numbers of ray r: words 0-2 = (image, y, x) of the pixel, words 3-5 = the samplers' single jitters
__device__ __forceinline__ void prologue_randoms(unsigned long long seed, unsigned long long offset, long long r, int group,
                                                 float (&out)[4]) {
  uint32_t c[4] = {(uint32_t)r, (uint32_t)((unsigned long long)r >> 32) ^ ((uint32_t)group << 24), (uint32_t)offset,
                   (uint32_t)(offset >> 32)};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = u01(c[i]);
}

// use_single_jitter = False: one number per bin edge.  The four jitters of edges 4q .. 4q + 3 of ray r at sampling level
// `level` (0 = the spaced sampler, 1.. = the PDF samplers) are the words of word group 3 + level, with the quad index in bits
// 8.. of the counter's second word: groups 0 and 1 stay the prologue's, 2 the random background's, and a quad index below 2^16
// (FNR_EDGE_JITTER_MAX_LEVELS levels) never reaches the group's bits.
constexpr int EDGE_JITTER_GROUP0 = 3;
__device__ __forceinline__ void edge_jitter_quad(unsigned long long seed, unsigned long long offset, int level, long long r,
                                                 int quad, float (&out)[4]) {
  uint32_t c[4] = {(uint32_t)r,
                   (uint32_t)((unsigned long long)r >> 32) ^ ((uint32_t)(EDGE_JITTER_GROUP0 + level) << 24) ^ ((uint32_t)quad << 8),
                   (uint32_t)offset, (uint32_t)(offset >> 32)};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = u01(c[i]);
}
// the jitter of edge j alone (word j & 3 of its quad)
__device__ __forceinline__ float edge_jitter(unsigned long long seed, unsigned long long offset, int level, long long r, int j) {
  float w[4];
  edge_jitter_quad(seed, offset, level, r, j >> 2, w);
  const int k = j & 3;
  return k == 0 ? w[0] : k == 1 ? w[1] : k == 2 ? w[2] : w[3];
}

// the generator's arguments of a kernel that draws its own per-edge jitter (draw != 0; sampler.hip)
struct EdgeDraw {
  unsigned long long seed, offset;
  int level, draw;
};
// replayed from a step program (sequencer.hpp): a draw continues at the step's counter
static inline EdgeDraw patched(EdgeDraw e, const fnr_step_scalars* s) {
  if (s && e.draw) e.offset = s->prologue_offset;
  return e;
}

}  // namespace fnr
