// field_mlp_bwd.hip — backward of FruitField's MLP stack: what every arithmetic shares.
//
// Autograd of fruit_field.py:187-281 for the training path (get_outputs): rgb loss flows through mlp_head into
// the geo features, the appearance embedding and the base MLP; the semantic loss only reaches mlp_semantics
// + SemanticFieldHead (geo is detached, fruit_field.py:263-265) unless pass_semantic_gradients (fruit_field.py:202-203,
// 263-264: then the semantic kernels' SEMGRAD form adds dX of mlp_semantics' first layer to dL/dh); dL/dsigma enters
// through trunc_exp.
//
// The branch kernels (colour, semantic, base) live by arithmetic: field_mlp_bwd_fp32.hip (fp32 MFMA chains),
// field_mlp_bwd_pw.hip (bf16 modes, per wave), field_mlp_bf16.hip (bf16 modes, `fruit_nerf_big`'s semantic branch); each
// leaves one partial weight-gradient image per workgroup.  Here: the kernels behind them (k_color_ray_grads,
// k_finish_weights), the workspace carve, the ONE schedule of the branches (field_mlp_bwd_launch) and the entry points.
#include "adam.hpp"
#include "field_layers.hpp"
#include "field_bf16.hpp"
#include "sequencer.hpp"

namespace fnr {

// sum the per-workgroup partial images and add them into the nn.Linear-layout gradients.  FIXED summation order and a
// single writer per gradient entry (no float atomics: training is bit-reproducible run to run): a workgroup is
// RD_IDX entries x RD_Y slices; slice y sums the images y, y + RD_Y, ... (8 independent loads in flight), the slices
// meet in LDS and are added up in slice order by the thread of slice 0.
// ADAM (single-process training, fnr_field_mlp_bwd_adam): the thread that owns a gradient entry also takes that
// parameter's optimiser step (torch.optim.Adam / RAdam exactly as fnr_adam_step / fnr_radam_step: same operations in the
// same order) and leaves the gradient entry zero — the ~20 k weights of the field's MLPs no longer need a launch of
// their own, and a step that does not train the proposal networks ends without any optimiser launch.
constexpr int RD_IDX = 128, RD_Y = 8;
template <class Cfg, bool ADAM>
__device__ __forceinline__ void reduce_dw_block(int block, const float* __restrict__ partials, int nblocks, const FieldPtrs& grads,
                                                const WeightAdam& wa) {
  __shared__ float s_part[RD_Y][RD_IDX];
  const int t = threadIdx.x % RD_IDX, y = threadIdx.x / RD_IDX;
  const int idx = block * RD_IDX + t;
  constexpr int TOT = Cfg::W_TOTAL + Cfg::B_TOTAL;
  float s = 0.0f;
  if (idx < TOT) {
    int b = y;
    for (; b + 7 * RD_Y < nblocks; b += 8 * RD_Y) {  // 8 independent loads in flight (a plain loop is one latency per row)
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = partials[(size_t)(b + u * RD_Y) * TOT + idx];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; b < nblocks; b += RD_Y) s += partials[(size_t)b * TOT + idx];
  }
  s_part[y][t] = s;
  __syncthreads();
  if (y != 0 || idx >= TOT) return;
#pragma unroll
  for (int q = 1; q < RD_Y; ++q) s += s_part[q][t];
  if (!ADAM && s == 0.0f) return;
  if (idx < Cfg::W_TOTAL) {
    int l = 0;
#pragma unroll
    for (int q = 1; q < Cfg::NLAYERS; ++q)
      if (idx >= Cfg::woff(q)) l = q;
    const int local = idx - Cfg::woff(l);
    const int r = local & 3, slot = (local >> 2) & 63, blk = local >> 8;
    const int nib = Cfg::nib(l);
    const int ib = blk % nib, ob = blk / nib;
    const int g = slot >> 4, i = (slot & 15) ^ g;
    const int out = 16 * ob + i;
    const int col = kmap<Cfg>(Cfg::km(l), ib, g, r, Cfg::in_dim(l));
    if (out < Cfg::out_dim(l) && col >= 0) {
      float* dst = const_cast<float*>(grads.w[l]) + out * Cfg::in_dim(l) + col;
      if constexpr (ADAM) weight_adam_entry(wa, dst, s);
      else *dst += s;  // sole writer of this entry
    }
  } else {
    const int bi = idx - Cfg::W_TOTAL;
    int l = 0;
#pragma unroll
    for (int q = 1; q < Cfg::NLAYERS; ++q)
      if (bi >= Cfg::boff(q)) l = q;
    const int o = bi - Cfg::boff(l);
    if (o < Cfg::out_dim(l)) {
      float* dst = const_cast<float*>(grads.b[l]) + o;
      if constexpr (ADAM) weight_adam_entry(wa, dst, s);
      else *dst += s;
    }
  }
}

// Per-ray finish of mlp_head layer 0 (see the colour branch kernels).  For every ray: g = sum of its tiles' G1 row
// sums (+ the per-sample contributions of tiles that straddle rays), written to g_ray [n_rays, 64] for the
// embedding gradient; c = [SH16(direction) | Embedding[camera]].  The workgroup accumulates g (x) c (64 x 48) and
// sum g (bias) over its 16 rays and stores them into ITS partial weight-gradient image (col0: input blocks
// HB..HB+2 and the bias, which the colour kernel left zero), so reduce_dw_block adds them like any other partial.
constexpr int RAYG_RB = 16;  // rays per workgroup pass
template <class Cfg>
__global__ __launch_bounds__(256) void k_color_ray_grads(RaysDev rays, int S, long long N,
                                                         const float* __restrict__ embedding,
                                                         const float* __restrict__ gsum_tile,
                                                         const float* __restrict__ gsum_extra,
                                                         float* __restrict__ g_ray, float* __restrict__ partials) {
  __shared__ float Gs[RAYG_RB][64];
  __shared__ __attribute__((aligned(16))) float Cs[RAYG_RB][COLOR_CONST_K];
  const int t = threadIdx.x, o = t & 63, kq = t >> 6;  // thread owns output o, constant inputs 12 kq .. 12 kq + 11
  const long long R = rays.n_rays;
  f32x4 acc[3];
  float accb = 0.0f;
#pragma unroll
  for (int q = 0; q < 3; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long base = (long long)blockIdx.x * RAYG_RB; base < R; base += (long long)gridDim.x * RAYG_RB) {
#pragma unroll
    for (int i = 0; i < RAYG_RB / 4; ++i) {
      const int rr = kq + 4 * i;
      const long long ray = base + rr;
      float v = 0.0f;
      if (ray < R) {
        const long long s_lo = ray * S, s_hi = s_lo + S;          // the ray's samples [s_lo, s_hi)
        for (long long tl = s_lo >> 4; tl <= (s_hi - 1) >> 4; ++tl) {  // tiles that overlap them
          const long long first = 16 * tl, last = (16 * tl + 15 < N) ? 16 * tl + 15 : N - 1;
          if (first >= s_lo && last < s_hi) v += gsum_tile[(size_t)tl * 64 + o];  // tile inside the ray
        }
        if (gsum_extra) v += gsum_extra[(size_t)ray * 64 + o];
        g_ray[(size_t)ray * 64 + o] = v;
      }
      Gs[rr][o] = v;
    }
#pragma unroll
    for (int u = 0; u < RAYG_RB * COLOR_CONST_K / 256; ++u) {
      const int idx = t + 256 * u;
      const int rr = idx / COLOR_CONST_K, k = idx - rr * COLOR_CONST_K;
      const long long ray = base + rr;
      float v = 0.0f;
      if (ray < R) {
        if (k < 16) {
          float c[16];
          sh16_all(rays.directions + 3 * ray, c);
#pragma unroll
          for (int q = 0; q < 16; ++q) v = (k == q) ? c[q] : v;
        } else {
          v = embedding[(size_t)rays.cam[ray] * 32 + (k - 16)];
        }
      }
      Cs[rr][k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < RAYG_RB; ++rr) {
      const float gv = Gs[rr][o];
      const f32x4* cr = reinterpret_cast<const f32x4*>(&Cs[rr][12 * kq]);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const f32x4 cv = cr[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[q][e] = fmaf(gv, cv[e], acc[q][e]);
      }
      accb += gv;
    }
    __syncthreads();
  }
  float* part = partials + (size_t)blockIdx.x * (Cfg::W_TOTAL + Cfg::B_TOTAL);
  const int ob = o >> 4, i = o & 15;
  constexpr int NIB0 = Cfg::HB + 3;
#pragma unroll
  for (int q = 0; q < 12; ++q) {
    const int k = 12 * kq + q, ib = Cfg::HB + (k >> 4), kk = k & 15;
    part[Cfg::woff(Cfg::L_COL0) + ((ob * NIB0 + ib) * 64 + swz_slot(i, kk >> 2)) * 4 + (kk & 3)] = acc[q >> 2][q & 3];
  }
  if (kq == 0) part[Cfg::W_TOTAL + Cfg::boff(Cfg::L_COL0) + o] = accb;
}
static_assert(RAYG_RB * COLOR_CONST_K % 256 == 0, "staging loop covers the batch exactly");

// appearance-embedding gradient (fruit_field.py:251 Embedding lookup): one workgroup per camera gathers the g rows
// of its rays (each wave tests 64 rays per ballot), then g_embedding[c][k] += sum_o W[o][emb col k] * gcam[o].
// No atomics: direct adds into the [n_images, 32] table serialise at ~12 ns per same-address add (393k adds on
// 90 rows made the colour branch 4x slower than its MFMA time).
template <class Cfg, bool ADAM>
__device__ __forceinline__ void embedding_grad_block(int c, const RaysDev& rays, const float* __restrict__ g_ray,
                                                     const float* __restrict__ packed, float* __restrict__ g_embedding,
                                                     const WeightAdam& wa) {
  __shared__ float red[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc = 0.0f;
  for (long long base = 64 * wave; base < rays.n_rays; base += 1024) {
    const long long r = base + lane;
    unsigned long long match = __ballot(r < rays.n_rays && rays.cam[r] == c);
    while (match) {
      const int bit = __builtin_ctzll(match);
      match &= match - 1;
      acc += g_ray[(size_t)(base + bit) * 64 + lane];
    }
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (threadIdx.x < 64) {
    float s = 0.0f;
#pragma unroll
    for (int w = 0; w < 16; ++w) s += red[w][lane];
    red[0][lane] = s;
  }
  __syncthreads();
  // thread (k = t >> 5, oo = t & 31): two of the 64 products of column k, then a 32-lane butterfly
  const int k = threadIdx.x >> 5, oo = threadIdx.x & 31;
  const float* Wt = packed + Cfg::LDS_FLOATS + (16 + k) * 64;  // transposed slice, row = embedding column k
  float s = fmaf(Wt[oo], red[0][oo], Wt[oo + 32] * red[0][oo + 32]);
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if constexpr (ADAM) {
    if (oo == 0) weight_adam_entry(wa, g_embedding + (size_t)c * 32 + k, s);  // every row takes its step (moment decay)
  } else {
    if (oo == 0 && s != 0.0f) g_embedding[(size_t)c * 32 + k] += s;
  }
}

// The two finishing roles of the MLP backward as ONE launch (round 6): workgroups [0, n_images) take the appearance embedding's
// rows (embedding_grad_block), the rest the weight-gradient images (reduce_dw_block) — both only need the colour kernel's per-ray
// sums (k_color_ray_grads) and every branch's partial images, neither reads what the other writes, both are 1024 threads.
// One launch ramp less on the launch stream's chain and the two roles next to each other instead of one after the other
// (7.4 + 9.7 us -> ~10); the same sums in the same order by the same single writers.
static_assert(RD_IDX * RD_Y == 1024, "k_finish_weights: both roles are 1024-thread workgroups");
template <class Cfg, bool ADAM>
__global__ __launch_bounds__(1024) void k_finish_weights(int n_images, RaysDev rays, const float* __restrict__ g_ray,
                                                         const float* __restrict__ packed, float* __restrict__ g_embedding,
                                                         const float* __restrict__ partials, int nblocks, FieldPtrs grads,
                                                         WeightAdam wa) {
  if ((int)blockIdx.x < n_images) embedding_grad_block<Cfg, ADAM>((int)blockIdx.x, rays, g_ray, packed, g_embedding, wa);
  else reduce_dw_block<Cfg, ADAM>((int)blockIdx.x - n_images, partials, nblocks, grads, wa);
}

int field_ptrs(const fnr_field_net* net, FieldPtrs& p, int* cfg_id);  // field_mlp.hip
size_t field_fwd_ws_image_offset();                                     // field_mlp.hip
int position_contract(long long N, int n_levels, const float2* jac, const float2* d_feats, float4* d_pos, hipStream_t st);

}  // namespace fnr

using namespace fnr;

namespace {
struct BwdWorkspace {
  float *partials, *d_h, *packed, *ray_bias, *gsum_tile, *g_ray, *gsum_extra;
  void* bf16_image;
  size_t bytes;
};
// carve the workspace: per-workgroup partial weight-gradient images (<= one workgroup per CU), dL/dh [N, 16 HB], the
// fragment image, and the per-ray colour terms — sized for the larger of the two built shapes
BwdWorkspace bwd_workspace(void* base, long long n_rays, int S) {
  const long long N = n_rays * (long long)S, n_tiles = (N + 15) / 16;
  uintptr_t p = reinterpret_cast<uintptr_t>(base);
  auto take = [&](size_t floats) {
    p = (p + 255) & ~(uintptr_t)255;
    float* r = reinterpret_cast<float*>(p);
    p += floats * sizeof(float);
    return r;
  };
  BwdWorkspace w;
  w.partials = take((size_t)device_cu_count() * FIELD_MAX_IMAGE_FLOATS);
  w.d_h = take((size_t)N * 16 * FIELD_MAX_HB);
  w.packed = take(FIELD_MAX_PACKED_FLOATS);
  w.ray_bias = take((size_t)n_rays * 64);
  w.gsum_tile = take((size_t)n_tiles * 64);
  w.g_ray = take((size_t)n_rays * 64);
  w.gsum_extra = take((size_t)n_rays * 64);
  w.bf16_image = take((field_bf16_image_bytes() + 3) / 4);
  w.bytes = p - reinterpret_cast<uintptr_t>(base) + 256;
  return w;
}

// The branch schedule, written once for every shape x mode x semgrad x jacobian x weight_adam: images the forward pass did
// not save -> colour -> per-ray finish -> semantic -> base -> weight finish (-> fp32 only: the contraction with the encode's
// Jacobian, which the bf16 modes' base kernel carries itself).  semgrad: the semantic kernel adds its input gradient into
// d_h, between the colour kernel that wrote it and the base kernel that reads it.
template <class Cfg>
int field_mlp_bwd_launch(const FieldBwdArgs& a, const BwdWorkspace& ws) {
  const hipStream_t st = a.st;
  const bool bf16 = a.mode != FNR_MLP_FP32;
  // a branch on the kernels of its arithmetic: fp32 chains | per-wave | `fruit_nerf_big`'s weight-streamed semantic branch
  auto branch = [&](int br) -> int {
    if (!bf16) return field_mlp_bwd_fp32(br, a);
    if (br == BR_SEM && Cfg::NSEM == 3) return field_mlp_bwd_sem_big_bf16(a);
    return field_mlp_bwd_pw(br, a);
  };
  if (a.pack_images) {  // the fragment image of the weights; its bf16 pieces follow the memset, as they always have
    launch_pack_field_weights<Cfg>(a.p, ws.packed, st);
    FNR_LAUNCH_CHECK();
  }
  if (a.make_ray_bias) {
    launch_color_ray_bias<Cfg>(a.packed, a.rd, a.embedding, nullptr, ws.ray_bias, st);
    FNR_LAUNCH_CHECK();
  }
  if (a.gsum_extra) FNR_HIP(hipMemsetAsync(a.gsum_extra, 0, (size_t)a.rd.n_rays * 64 * sizeof(float), st));
  if (a.pack_images && bf16) {
    launch_pack_field_weights_bf16<Cfg>(a.p, a.mode == FNR_MLP_BF16 ? 1 : 3, reinterpret_cast<__bf16*>(ws.bf16_image), st);
    FNR_LAUNCH_CHECK();
  }
  int rc = branch(BR_COLOR);
  if (rc) return rc;
  // per-ray finish of mlp_head layer 0: every workgroup owns one partial image row that exists
  long long rb = (a.rd.n_rays + RAYG_RB - 1) / RAYG_RB;
  if (rb > a.blocks) rb = a.blocks;
  hipLaunchKernelGGL((k_color_ray_grads<Cfg>), dim3((unsigned)rb), dim3(256), 0, st, a.rd, a.S, a.N, a.embedding, a.gsum_tile,
                     a.gsum_extra, a.g_ray, a.partials);
  FNR_LAUNCH_CHECK();
  // (the appearance embedding's rows, which only need g_ray, are taken by the LAST launch: k_finish_weights)
  if (bf16 && a.semgrad && Cfg::NSEM == 2 && (rc = branch(BR_SEM_DX))) return rc;
  if ((rc = branch(BR_SEM)) || (rc = branch(BR_BASE))) return rc;
  constexpr int TOT = Cfg::W_TOTAL + Cfg::B_TOTAL;
  const unsigned finish_blocks = (unsigned)a.n_images + (unsigned)((TOT + RD_IDX - 1) / RD_IDX);
  hipLaunchKernelGGL((a.wadam ? k_finish_weights<Cfg, true> : k_finish_weights<Cfg, false>), dim3(finish_blocks), dim3(1024), 0,
                     st, a.n_images, a.rd, a.g_ray, a.packed, a.g_embedding, a.partials, (int)a.blocks, a.gp,
                     a.wadam ? *a.wadam : WeightAdam{});
  FNR_LAUNCH_CHECK();
  if (a.jac && a.d_pos && !bf16) return position_contract(a.N, a.n_levels, a.jac, a.d_feats, a.d_pos, st);
  return FNR_OK;
}

// the arguments of the four entry points (jacobian .. grad_arena: NULL where an entry point does not take them)
struct BwdCall {
  const fnr_field_net *net, *grads;
  const fnr_rays* rays;
  int S;
  const float *feats, *h_saved, *ray_bias_saved, *packed_saved;
  const uint8_t* selector;
  const float *d_density, *d_rgb, *d_logit;
  float* d_feats;
  const float* jacobian;
  float* d_position;
  const fnr_table_adam* weight_adam;
  const float* grad_arena;
  void* workspace;
  size_t workspace_bytes;
  void* stream;
};

// validates the call, fills the family's argument block once and runs the schedule for the net's shape
int field_mlp_bwd_entry(const BwdCall& c, bool semgrad) {
  const fnr_field_net *net = c.net, *grads = c.grads;
  const fnr_rays* rays = c.rays;
  void* const stream = c.stream;  // (FNR_PROF)
  WeightAdam wa{};
  if (c.weight_adam) {
    FNR_CHECK_ARG(c.grad_arena, "field_mlp_bwd_adam: grad_arena missing");
    const int rca = make_table_adam(c.weight_adam, wa.t);
    if (rca) return rca;
    wa.p_off = c.weight_adam->params - c.grad_arena;
    wa.m_off = c.weight_adam->exp_avg - c.grad_arena;
    wa.v_off = c.weight_adam->exp_avg_sq - c.grad_arena;
  }
  FNR_CHECK_ARG(net && grads && rays && c.feats && c.h_saved && c.d_density && c.d_rgb && c.d_logit && c.d_feats &&
                    c.workspace && c.S > 0, "field_mlp_bwd: null argument");
  FNR_CHECK_ARG(rays->directions && rays->camera_indices && net->embedding && grads->embedding,
                "field_mlp_bwd: training path needs directions, camera indices and the embedding (+ its gradient)");
  FieldBwdArgs a{};
  int gcfg = 0, rc = field_ptrs(net, a.p, &a.cfg);
  if (rc || (rc = field_ptrs(grads, a.gp, &gcfg))) return rc;
  FNR_CHECK_ARG(a.cfg == gcfg, "field_mlp_bwd: net and grads describe different field shapes");
  FNR_CHECK_ARG(net->mlp_mode == FNR_MLP_FP32 || net->mlp_mode == FNR_MLP_BF16 || net->mlp_mode == FNR_MLP_BF16X3,
                "field_mlp_bwd: mlp_mode %d (FNR_MLP_FP32 0 | FNR_MLP_BF16 1 | FNR_MLP_BF16X3 3)", net->mlp_mode);
  const int S = c.S;
  const long long N = rays->n_rays * (long long)S;
  if (N == 0) return FNR_OK;
  FNR_CHECK_ARG(c.workspace_bytes >= fnr_field_mlp_bwd_workspace_bytes(rays->n_rays, S), "field_mlp_bwd: workspace too small");
  const BwdWorkspace ws = bwd_workspace(c.workspace, rays->n_rays, S);
  FNR_PROF(OP_MLP_BWD, N);
  a.mode = net->mlp_mode, a.semgrad = semgrad, a.wadam = c.weight_adam ? &wa : nullptr;
  a.embedding = net->embedding, a.g_embedding = grads->embedding;
  a.n_images = (int)net->n_images, a.n_levels = net->grid.n_levels;
  // the forward pass's fragment image of the same weights, with its bf16 pieces, when it was saved
  a.pack_images = !c.packed_saved, a.make_ray_bias = !c.ray_bias_saved;
  a.packed = a.pack_images ? ws.packed : c.packed_saved;
  a.image = reinterpret_cast<const __bf16*>(
      a.pack_images ? ws.bf16_image : reinterpret_cast<const char*>(c.packed_saved) + field_fwd_ws_image_offset());
  a.ray_bias = a.make_ray_bias ? ws.ray_bias : c.ray_bias_saved;
  a.rd = make_rays(rays), a.S = S, a.N = N;
  a.feats = reinterpret_cast<const float2*>(c.feats), a.h_saved = c.h_saved, a.selector = c.selector;
  a.d_density = c.d_density, a.d_rgb = c.d_rgb, a.d_logit = c.d_logit, a.d_feats = reinterpret_cast<float2*>(c.d_feats);
  a.d_h = ws.d_h, a.gsum_tile = ws.gsum_tile, a.g_ray = ws.g_ray, a.partials = ws.partials;
  a.gsum_extra = (S % 16 != 0) ? ws.gsum_extra : nullptr;  // only tiles that straddle rays use it
  // every branch uses the same number of workgroups so that they share one partial-image buffer
  a.blocks = ((N + 15) / 16 + 3) / 4;
  if (a.blocks > device_cu_count()) a.blocks = device_cu_count();
  a.jac = reinterpret_cast<const float2*>(c.jacobian), a.d_pos = reinterpret_cast<float4*>(c.d_position), a.st = as_stream(stream);
  return a.cfg == 0 ? field_mlp_bwd_launch<FieldCfgBase>(a, ws) : field_mlp_bwd_launch<FieldCfgBig>(a, ws);
}

// _adam / _semgrad while a step program is recorded: `entry`, the export that was called, is what replays, as `name`, on the
// block's members (a call without its host structs, weight_adam among them, is not recorded).  False: nothing was recorded.
bool record_bwd(const char* name, decltype(&fnr_field_mlp_bwd_adam) entry, const BwdCall& c) {
  return seq::record(name, entry, c.net, c.grads, c.rays, c.S, c.feats, c.h_saved, c.ray_bias_saved, c.packed_saved, c.selector,
                     c.d_density, c.d_rgb, c.d_logit, c.d_feats, c.jacobian, c.d_position, c.weight_adam, c.grad_arena,
                     c.workspace, c.workspace_bytes, c.stream);
}
}  // namespace

extern "C" size_t fnr_field_mlp_bwd_workspace_bytes(int64_t n_rays, int S) {
  if (n_rays < 0 || S <= 0) return 0;
  return bwd_workspace(nullptr, n_rays, S).bytes;
}

extern "C" int fnr_field_mlp_bwd(const fnr_field_net* net, const fnr_field_net* grads, const fnr_rays* rays, int S,
                                 const float* feats, const float* h_saved, const float* ray_bias_saved,
                                 const float* packed_saved, const uint8_t* selector, const float* d_density,
                                 const float* d_rgb, const float* d_logit, float* d_feats, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_field_mlp_bwd");
  return field_mlp_bwd_entry({net, grads, rays, S, feats, h_saved, ray_bias_saved, packed_saved, selector, d_density, d_rgb,
                              d_logit, d_feats, nullptr, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream},
                             false);
}

extern "C" int fnr_field_mlp_bwd_adam(const fnr_field_net* net, const fnr_field_net* grads, const fnr_rays* rays, int S,
                                      const float* feats, const float* h_saved, const float* ray_bias_saved,
                                      const float* packed_saved, const uint8_t* selector, const float* d_density,
                                      const float* d_rgb, const float* d_logit, float* d_feats, const float* jacobian,
                                      float* d_position, const fnr_table_adam* weight_adam, const float* grad_arena,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  const BwdCall c{net, grads, rays, S, feats, h_saved, ray_bias_saved, packed_saved, selector, d_density, d_rgb, d_logit,
                  d_feats, jacobian, d_position, weight_adam, grad_arena, workspace, workspace_bytes, stream};
  record_bwd("fnr_field_mlp_bwd_adam", fnr_field_mlp_bwd_adam, c);
  FNR_CHECK_ARG(weight_adam && grad_arena, "field_mlp_bwd_adam: weight_adam / grad_arena missing");
  FNR_CHECK_ARG((jacobian == nullptr) == (d_position == nullptr), "field_mlp_bwd_adam: jacobian and d_position go together");
  return field_mlp_bwd_entry(c, false);
}

extern "C" int fnr_field_mlp_bwd_rays(const fnr_field_net* net, const fnr_field_net* grads, const fnr_rays* rays, int S,
                                      const float* feats, const float* h_saved, const float* ray_bias_saved,
                                      const float* packed_saved, const uint8_t* selector, const float* d_density,
                                      const float* d_rgb, const float* d_logit, float* d_feats, const float* jacobian,
                                      float* d_position, void* workspace, size_t workspace_bytes, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_field_mlp_bwd_rays");
  FNR_CHECK_ARG(jacobian && d_position, "field_mlp_bwd_rays: jacobian / d_position missing");
  return field_mlp_bwd_entry({net, grads, rays, S, feats, h_saved, ray_bias_saved, packed_saved, selector, d_density, d_rgb,
                              d_logit, d_feats, jacobian, d_position, nullptr, nullptr, workspace, workspace_bytes, stream},
                             false);
}

// fnr_field_mlp_bwd / _rays / _adam under pass_semantic_gradients = True (fruit_field.py:202-203, 263-264: the geometry
// feature that feeds mlp_semantics is not detached): one entry point, jacobian / d_position both NULL or both set,
// weight_adam / grad_arena both NULL or both set.  Recordable when the optimiser is fused, like fnr_field_mlp_bwd_adam.
extern "C" int fnr_field_mlp_bwd_semgrad(const fnr_field_net* net, const fnr_field_net* grads, const fnr_rays* rays, int S,
                                         const float* feats, const float* h_saved, const float* ray_bias_saved,
                                         const float* packed_saved, const uint8_t* selector, const float* d_density,
                                         const float* d_rgb, const float* d_logit, float* d_feats, const float* jacobian,
                                         float* d_position, const fnr_table_adam* weight_adam, const float* grad_arena,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  const BwdCall c{net, grads, rays, S, feats, h_saved, ray_bias_saved, packed_saved, selector, d_density, d_rgb, d_logit,
                  d_feats, jacobian, d_position, weight_adam, grad_arena, workspace, workspace_bytes, stream};
  if (!record_bwd("fnr_field_mlp_bwd_semgrad", fnr_field_mlp_bwd_semgrad, c))
    FNR_SEQ_UNRECORDABLE("fnr_field_mlp_bwd_semgrad (without weight_adam)");
  FNR_CHECK_ARG((weight_adam == nullptr) == (grad_arena == nullptr),
                "field_mlp_bwd_semgrad: weight_adam and grad_arena go together");
  FNR_CHECK_ARG((jacobian == nullptr) == (d_position == nullptr), "field_mlp_bwd_semgrad: jacobian and d_position go together");
  return field_mlp_bwd_entry(c, true);
}

