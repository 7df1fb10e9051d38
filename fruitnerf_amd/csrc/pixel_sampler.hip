// pixel_sampler.hip — the caller side of a training step on the device (SURVEY §8f "next" row 1):
// Nerfstudio's PixelSampler + RayGenerator as driven by FruitDataManager.next_train
// (/root/reference/fruit_nerf/data/fruit_datamanager.py:188-197): uniform random (image, y, x) triples ->
// pinhole rays (pixel centre +0.5, camera looks along -z) + the rgb / fruit-mask targets of those pixels.
// One thread per ray; replaces ~15 small elementwise/index launches per step.  HBM-bound, 40 B written per ray.
#include "camera_math.hpp"
#include "sampler_math.hpp"
#include "sequencer.hpp"
#include "step_randoms.hpp"

namespace fnr {

// CAMS: the camera-frame direction comes from the per-image camera table instead of the set-wide pinhole
// (camera_math.hpp::camera_direction); everything else is the same code.
template <bool CAMS>
__global__ __launch_bounds__(256) void k_sample_pixels(ImageSetDev s, CameraTableDev cams,
                                                       const long long* __restrict__ train_ids,
                                                       int n_train, long long n_rays, const float* __restrict__ u,
                                                       const float* __restrict__ c2w_adjusted,
                                                       float* __restrict__ origins, float* __restrict__ directions,
                                                       int* __restrict__ cam_idx, float* __restrict__ image,
                                                       float* __restrict__ mask) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rays) return;
  const Pixel p = pick_pixel(u + 3 * r, n_train, s.grid.H, s.grid.W);
  const long long img = train_ids[p.k];
  float dc[3];
  camera_direction<CAMS>(s.grid, cams, img, p.x, p.y, dc);
  // camera-pose optimisation: the slot's corrected camera (fnr_camera_adjust) replaces the dataset's
  const float* M = c2w_adjusted ? c2w_adjusted + (size_t)p.k * 12 : s.c2w + img * 12;
  world_ray(M, dc, origins + 3 * r, directions + 3 * r);
  cam_idx[r] = p.k;  // camera index = position in the training set (appearance-embedding row)
  gather_target(s, img, p.y, p.x, image + 3 * r, mask + r);
}

// ---- the start of a training step in ONE launch (fnr_train_prologue) ---------------------------------------------------
// Five launches of 4-7 us each before (random numbers for the pixels, camera adjust, pixel sampling, random numbers for
// the sampler's jitter, level-0 spaced sampling), all latency: the random numbers come from a counter-based generator
// (Philox4x32-10, Salmon et al. 2011; counter = (ray, word group, step offset), key = seed), so every role of the launch
// derives the numbers it needs itself (step_randoms.hpp).

// background_color = "random" (fnr_random_background): the ray's background triple = words 0-2 of word group 2 of the step's
// numbers — the prologue keeps groups 0 and 1, so drawing a background changes none of its numbers.
constexpr int RANDOM_BACKGROUND_GROUP = 2;
__global__ __launch_bounds__(256) void k_random_background(unsigned long long seed, unsigned long long offset, long long n_rays,
                                                           float* __restrict__ out) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rays) return;
  float w[4];
  prologue_randoms(seed, offset, r, RANDOM_BACKGROUND_GROUP, w);
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * r + c] = w[c];
}

// EDGES (use_single_jitter = False, fnr_train_prologue_edges): the per-ray role writes no jitter rows, and the level-0 role is
// one thread per QUAD of bin edges — one Philox call gives the jitters of edges 4q .. 4q + 3 (step_randoms.hpp).
template <bool CAMS, int MODE, bool EDGES = false>
__global__ __launch_bounds__(256) void k_train_prologue(PrologueArgs a, CameraTableDev cams) {
  if ((int)blockIdx.x < a.nb_rays) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    // corrected cameras for the pose-gradient kernel: camera k by thread k of the launch (same arithmetic as per ray)
    if (a.pose && r < a.n_train) {
      float adj[12];
      adjusted_camera<MODE>(a.set.c2w + a.train_ids[r] * 12, a.pose + 6 * r, adj);
#pragma unroll
      for (int i = 0; i < 12; ++i) a.c2w_adjusted[12 * r + i] = adj[i];
    }
    if (r >= a.n_rays) return;
    float w0[4], w1[4];
    prologue_randoms(a.seed, a.offset, r, 0, w0);
    prologue_randoms(a.seed, a.offset, r, 1, w1);
    const float rnd[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
#pragma unroll
    for (int i = 0; i < 3; ++i) a.u[3 * r + i] = rnd[i];
    if constexpr (!EDGES)
      for (int i = 0; i < a.n_jitter; ++i) a.jitter[(size_t)i * a.n_rays + r] = rnd[3 + i];
    // pixel sampling + ray generation: what k_sample_pixels does, with the ray's corrected camera formed in place
    const Pixel p = pick_pixel(rnd, a.n_train, a.set.grid.H, a.set.grid.W);
    const long long img = a.train_ids[p.k];
    float dc[3];
    camera_direction<CAMS>(a.set.grid, cams, img, p.x, p.y, dc);
    float M[12];
    if (a.pose) {
      adjusted_camera<MODE>(a.set.c2w + img * 12, a.pose + 6 * p.k, M);
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) M[i] = a.set.c2w[img * 12 + i];
    }
    world_ray(M, dc, a.origins + 3 * r, a.directions + 3 * r);
    a.cam_idx[r] = p.k;
    gather_target(a.set, img, p.y, p.x, a.image + 3 * r, a.mask + r);
    return;
  }
  if constexpr (EDGES) {
    // level-0 bins, one jitter per edge (k_sample_spaced with t_rand_per_bin on fnr_edge_jitter(level 0))
    const int nq = (a.S0 + 4) >> 2;   // quads of S0 + 1 edges
    const long long qidx = ((long long)blockIdx.x - a.nb_rays) * 256 + threadIdx.x;
    if (qidx >= a.n_rays * (long long)nq) return;
    const long long r = qidx / nq;
    const int q = (int)(qidx - r * nq);
    float t[4];
    edge_jitter_quad(a.seed, a.offset, 0, r, q, t);
    const float s_near = spacing_fn(a.kind, a.near), s_far = spacing_fn(a.kind, a.far);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 4 * q + i;
      if (j <= a.S0) {
        const float b = spaced_bin_edge(a.base_bins, a.S0, j, true, t[i]);
        a.spacing0[r * (a.S0 + 1) + j] = b;
        a.euclid0[r * (a.S0 + 1) + j] = spacing_to_euclid(a.kind, b, s_near, s_far);
      }
    }
    return;
  }
  // level-0 bins of the proposal sampler (k_sample_spaced with one jitter per ray = word 3 of the ray's numbers)
  const long long idx = ((long long)blockIdx.x - a.nb_rays) * 256 + threadIdx.x;
  const long long total = a.n_rays * (long long)(a.S0 + 1);
  if (idx >= total) return;
  const long long r = idx / (a.S0 + 1);
  const int j = (int)(idx - r * (a.S0 + 1));
  float w0[4];
  prologue_randoms(a.seed, a.offset, r, 0, w0);
  const float b = spaced_bin_edge(a.base_bins, a.S0, j, true, w0[3]);
  const float s_near = spacing_fn(a.kind, a.near), s_far = spacing_fn(a.kind, a.far);
  a.spacing0[idx] = b;
  a.euclid0[idx] = spacing_to_euclid(a.kind, b, s_near, s_far);
}

// fnr_edge_jitter: the numbers the per-edge forms draw, written out — one thread per quad of edges
__global__ __launch_bounds__(256) void k_edge_jitter(unsigned long long seed, unsigned long long offset, int level,
                                                     long long n_rays, int n_edges, float* __restrict__ out) {
  const int nq = (n_edges + 3) >> 2;
  const long long qidx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (qidx >= n_rays * (long long)nq) return;
  const long long r = qidx / nq;
  const int q = (int)(qidx - r * nq);
  float t[4];
  edge_jitter_quad(seed, offset, level, r, q, t);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (4 * q + i < n_edges) out[r * n_edges + 4 * q + i] = t[i];
}

// ---- full-image rays of ONE camera (fnr_camera_rays): rows [y0, y1) of its H x W pixels, one thread per pixel ----------
// The functions of k_sample_pixels<true> on the pixel itself instead of the `u` that selects it.
__global__ __launch_bounds__(256) void k_camera_rays(const float* __restrict__ c2w, const float* __restrict__ K,
                                                     const float* __restrict__ D, int W, int y0, long long n_pix,
                                                     float* __restrict__ origins, float* __restrict__ directions) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_pix) return;
  const int row = (int)(r / W);
  const int x = (int)(r - (long long)row * W), y = y0 + row;
  float dc[3];
  pixel_direction(K, D, x, y, dc);
  world_ray(c2w, dc, origins + 3 * r, directions + 3 * r);
}

}  // namespace fnr

using namespace fnr;

// fnr_sample_pixels*'s own pointers
struct SamplePixelsArgs {
  const float *u, *c2w_adjusted;
  float *origins, *directions;
  int32_t* camera_indices;
  float *image, *fruit_mask;
};

static int sample_pixels(const CameraCall& c, const SamplePixelsArgs& a) {
  FNR_SEQ_UNRECORDABLE(c.name);
  const bool own = a.u && a.origins && a.directions && a.camera_indices && a.image && a.fruit_mask;
  const int rc = check_camera_call(c, "sample_pixels", own, true);
  if (rc) return rc;
  if (c.n_rays == 0) return FNR_OK;
  const auto kernel = camera_kernel(c, [](auto cams, auto) { return k_sample_pixels<decltype(cams)::value>; });
  hipLaunchKernelGGL(kernel, dim3((unsigned)((c.n_rays + 255) / 256)), dim3(256), 0, as_stream(c.stream), c.set, c.cams,
                     c.train_ids, c.n_train, c.n_rays, a.u, a.c2w_adjusted, a.origins, a.directions, a.camera_indices, a.image,
                     a.fruit_mask);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

extern "C" int fnr_sample_pixels(const fnr_image_set* set, const int64_t* train_ids, int n_train, int64_t n_rays,
                                 const float* u, const float* c2w_adjusted, float* origins, float* directions,
                                 int32_t* camera_indices, float* image, float* fruit_mask, void* stream) {
  return sample_pixels(camera_call("fnr_sample_pixels", set, nullptr, false, FNR_POSE_SO3XR3, train_ids, n_train, n_rays,
                                   stream), {u, c2w_adjusted, origins, directions, camera_indices, image, fruit_mask});
}

extern "C" int fnr_sample_pixels_cams(const fnr_image_set* set, const fnr_camera_table* cams, const int64_t* train_ids,
                                      int n_train, int64_t n_rays, const float* u, const float* c2w_adjusted, float* origins,
                                      float* directions, int32_t* camera_indices, float* image, float* fruit_mask,
                                      void* stream) {
  return sample_pixels(camera_call("fnr_sample_pixels_cams", set, cams, true, FNR_POSE_SO3XR3, train_ids, n_train, n_rays,
                                   stream), {u, c2w_adjusted, origins, directions, camera_indices, image, fruit_mask});
}

extern "C" int fnr_camera_rays(const float* c2w, const float* intrinsics, const float* distortion, int H, int W, int y0,
                               int y1, float* origins, float* directions, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_camera_rays");
  FNR_CHECK_ARG(c2w && intrinsics && origins && directions, "camera_rays: null argument");
  FNR_CHECK_ARG(H > 0 && W > 0 && y0 >= 0 && y0 <= y1 && y1 <= H, "camera_rays: rows [%d, %d) of a %d x %d image", y0, y1,
                H, W);
  const long long n_pix = (long long)(y1 - y0) * W;
  if (n_pix == 0) return FNR_OK;
  hipLaunchKernelGGL(k_camera_rays, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, as_stream(stream), c2w, intrinsics,
                     distortion, W, y0, n_pix, origins, directions);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

// a: the entry point's part of the kernel's arguments;  edges: the per-edge form (fnr_train_prologue_edges; jitter == NULL,
// n_jitter == 0).  A recorded call is replayed from the block and `a` with the step's offset.
static int train_prologue(const CameraCall& c, PrologueArgs a, bool edges) {
  if (c.has_set && (!c.use_cams || c.has_cams)) seq::record(c.name, &train_prologue, c, a, edges);
  const bool own = a.u && (a.jitter || edges) && a.origins && a.directions && a.cam_idx && a.image && a.mask && a.base_bins &&
                   a.spacing0 && a.euclid0;
  const int rc = check_camera_call(c, "train_prologue", own, true);
  if (rc) return rc;
  const int S0 = a.S0;
  FNR_CHECK_ARG(edges || (a.n_jitter >= 1 && a.n_jitter <= FNR_TRAIN_PROLOGUE_MAX_JITTER && S0 >= 1),
                "train_prologue: n_jitter %d (1..%d), S0 %d", a.n_jitter, FNR_TRAIN_PROLOGUE_MAX_JITTER, S0);
  FNR_CHECK_ARG(!edges || (S0 >= 1 && S0 < FNR_EDGE_JITTER_MAX_EDGES), "train_prologue_edges: S0 %d (1..%d)", S0,
                FNR_EDGE_JITTER_MAX_EDGES - 1);
  FNR_CHECK_ARG((a.pose == nullptr) == (a.c2w_adjusted == nullptr), "train_prologue: pose and c2w_adjusted go together");
  FNR_CHECK_ARG(c.n_rays >= c.n_train || !a.pose, "train_prologue: fewer rays than cameras");
  if (c.n_rays == 0) return FNR_OK;
  void* const stream = c.stream;  // (FNR_PROF)
  const long long n_rays = c.n_rays;
  a.set = c.set, a.train_ids = c.train_ids, a.n_train = c.n_train, a.n_rays = n_rays;
  a.nb_rays = (int)((n_rays + 255) / 256);
  // (per edge: one thread per quad of edges)
  const long long nb_bins = ((edges ? n_rays * (long long)((S0 + 4) >> 2) : n_rays * (long long)(S0 + 1)) + 255) / 256;
  FNR_PROF(OP_SAMPLE_SPACED, n_rays * (long long)(S0 + 1));
  const auto kernel = camera_kernel(c, [edges](auto cams, auto mode) {
    constexpr bool CAMS = decltype(cams)::value;
    constexpr int MODE = decltype(mode)::value;
    return edges ? k_train_prologue<CAMS, MODE, true> : k_train_prologue<CAMS, MODE, false>;
  });
  hipLaunchKernelGGL(kernel, dim3((unsigned)(a.nb_rays + nb_bins)), dim3(256), 0, as_stream(stream), a, c.cams);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

extern "C" int fnr_train_prologue(const fnr_image_set* set, const int64_t* train_ids, int n_train, int64_t n_rays,
                                  uint64_t seed, uint64_t offset, const float* pose_adjustment, float* c2w_adjusted, float* u,
                                  float* jitter, int n_jitter, float* origins, float* directions, int32_t* camera_indices,
                                  float* image, float* fruit_mask, float near_plane, float far_plane, int spacing_kind, int S0,
                                  const float* base_bins, float* spacing0, float* euclid0, void* stream) {
  return train_prologue(camera_call("fnr_train_prologue", set, nullptr, false, FNR_POSE_SO3XR3, train_ids, n_train, n_rays,
                                    stream),
                        {seed, offset, pose_adjustment, c2w_adjusted, u, jitter, n_jitter, origins, directions, camera_indices,
                         image, fruit_mask, near_plane, far_plane, spacing_kind, S0, base_bins, spacing0, euclid0}, false);
}

extern "C" int fnr_train_prologue_cams(const fnr_image_set* set, const fnr_camera_table* cams, const int64_t* train_ids,
                                       int n_train, int64_t n_rays, uint64_t seed, uint64_t offset,
                                       const float* pose_adjustment, float* c2w_adjusted, float* u, float* jitter, int n_jitter,
                                       float* origins, float* directions, int32_t* camera_indices, float* image,
                                       float* fruit_mask, float near_plane, float far_plane, int spacing_kind, int S0,
                                       const float* base_bins, float* spacing0, float* euclid0, void* stream) {
  return train_prologue(camera_call("fnr_train_prologue_cams", set, cams, true, FNR_POSE_SO3XR3, train_ids, n_train, n_rays,
                                    stream),
                        {seed, offset, pose_adjustment, c2w_adjusted, u, jitter, n_jitter, origins, directions, camera_indices,
                         image, fruit_mask, near_plane, far_plane, spacing_kind, S0, base_bins, spacing0, euclid0}, false);
}

extern "C" int fnr_train_prologue_mode(const fnr_image_set* set, const fnr_camera_table* cams, int pose_mode,
                                       const int64_t* train_ids, int n_train, int64_t n_rays, uint64_t seed, uint64_t offset,
                                       const float* pose_adjustment, float* c2w_adjusted, float* u, float* jitter, int n_jitter,
                                       float* origins, float* directions, int32_t* camera_indices, float* image,
                                       float* fruit_mask, float near_plane, float far_plane, int spacing_kind, int S0,
                                       const float* base_bins, float* spacing0, float* euclid0, void* stream) {
  return train_prologue(camera_call("fnr_train_prologue_mode", set, cams, cams != nullptr, pose_mode, train_ids, n_train,
                                    n_rays, stream),
                        {seed, offset, pose_adjustment, c2w_adjusted, u, jitter, n_jitter, origins, directions, camera_indices,
                         image, fruit_mask, near_plane, far_plane, spacing_kind, S0, base_bins, spacing0, euclid0}, false);
}

extern "C" int fnr_train_prologue_edges(const fnr_image_set* set, const fnr_camera_table* cams, int pose_mode,
                                        const int64_t* train_ids, int n_train, int64_t n_rays, uint64_t seed, uint64_t offset,
                                        const float* pose_adjustment, float* c2w_adjusted, float* u, float* origins,
                                        float* directions, int32_t* camera_indices, float* image, float* fruit_mask,
                                        float near_plane, float far_plane, int spacing_kind, int S0, const float* base_bins,
                                        float* spacing0, float* euclid0, void* stream) {
  return train_prologue(camera_call("fnr_train_prologue_edges", set, cams, cams != nullptr, pose_mode, train_ids, n_train,
                                    n_rays, stream),
                        {seed, offset, pose_adjustment, c2w_adjusted, u, nullptr, 0, origins, directions, camera_indices, image,
                         fruit_mask, near_plane, far_plane, spacing_kind, S0, base_bins, spacing0, euclid0}, true);
}

extern "C" int fnr_edge_jitter(uint64_t seed, uint64_t offset, int level, int64_t n_rays, int n_edges, float* out,
                               void* stream) {
  FNR_SEQ_RECORD(fnr_edge_jitter, seed, seq::Offset{offset}, level, n_rays, n_edges, out, stream);
  FNR_CHECK_ARG(out && n_rays >= 0, "edge_jitter: null argument or negative ray count");
  FNR_CHECK_ARG(level >= 0 && level < FNR_EDGE_JITTER_MAX_LEVELS, "edge_jitter: level %d (0..%d)", level,
                FNR_EDGE_JITTER_MAX_LEVELS - 1);
  FNR_CHECK_ARG(n_edges >= 1 && n_edges <= FNR_EDGE_JITTER_MAX_EDGES, "edge_jitter: n_edges %d (1..%d)", n_edges,
                FNR_EDGE_JITTER_MAX_EDGES);
  if (n_rays == 0) return FNR_OK;
  const long long quads = n_rays * (long long)((n_edges + 3) >> 2);
  hipLaunchKernelGGL(k_edge_jitter, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, as_stream(stream),
                     (unsigned long long)seed, (unsigned long long)offset, level, (long long)n_rays, n_edges, out);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

extern "C" int fnr_random_background(uint64_t seed, uint64_t offset, int64_t n_rays, float* out, void* stream) {
  FNR_SEQ_RECORD(fnr_random_background, seed, seq::Offset{offset}, n_rays, out, stream);
  FNR_CHECK_ARG(out && n_rays >= 0, "random_background: null argument or negative ray count");
  if (n_rays == 0) return FNR_OK;
  hipLaunchKernelGGL(k_random_background, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, as_stream(stream),
                     (unsigned long long)seed, (unsigned long long)offset, (long long)n_rays, out);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}
