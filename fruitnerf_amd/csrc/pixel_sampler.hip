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

struct ImageSetDev {
  int n_images, H, W;
  const uint8_t* images;  // [M,H,W,3]
  const uint8_t* masks;   // [M,H,W]
  const float* c2w;       // [M,3,4]
  float fx, fy, cx, cy;
};

// CAMS: the camera-frame direction comes from the per-image camera table (camera_math.hpp::pixel_direction) instead of
// the set-wide pinhole; everything after it is the same code.
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
  // indices = floor(rand * [n_train, H, W]) (PixelSampler.sample_method), clamped like the torch mirror
  int k = (int)(u[3 * r] * (float)n_train);
  int y = (int)(u[3 * r + 1] * (float)s.H);
  int x = (int)(u[3 * r + 2] * (float)s.W);
  k = min(k, n_train - 1);
  y = min(y, s.H - 1);
  x = min(x, s.W - 1);
  const long long img = train_ids[k];
  float dx, dy, dz;
  if constexpr (CAMS) {
    float dc[3];
    pixel_direction(cams.intrinsics + 4 * img, cams.distortion ? cams.distortion + 6 * img : nullptr, x, y, dc);
    dx = dc[0], dy = dc[1], dz = dc[2];
  } else {
    dx = fdiv(fsub(fadd((float)x, 0.5f), s.cx), s.fx);
    dy = -fdiv(fsub(fadd((float)y, 0.5f), s.cy), s.fy);
    dz = -1.0f;
  }
  // camera-pose optimisation: the slot's corrected camera (fnr_camera_adjust) replaces the dataset's
  const float* M = c2w_adjusted ? c2w_adjusted + (size_t)k * 12 : s.c2w + img * 12;
  float d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) d[a] = fadd(fadd(fmul(M[4 * a], dx), fmul(M[4 * a + 1], dy)), fmul(M[4 * a + 2], dz));
  const float nrm = fmaxf(sqrtf(fadd(fadd(fmul(d[0], d[0]), fmul(d[1], d[1])), fmul(d[2], d[2]))), 1e-12f);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    directions[3 * r + a] = fdiv(d[a], nrm);
    origins[3 * r + a] = M[4 * a + 3];
  }
  cam_idx[r] = k;  // camera index = position in the training set (appearance-embedding row)
  const size_t pix = ((size_t)img * s.H + y) * s.W + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) image[3 * r + c] = fdiv((float)s.images[3 * pix + c], 255.0f);
  mask[r] = (float)s.masks[pix];
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

struct PrologueArgs {
  ImageSetDev set;
  const long long* train_ids;
  int n_train;
  long long n_rays;
  unsigned long long seed, offset;
  const float* pose;        // [n_train, 6] tangents of the kernel's MODE, or NULL (cameras as they are)
  float* c2w_adjusted;      // [n_train, 3, 4] out (with pose)
  float *u, *jitter;        // [R, 3], [n_jitter, R] out (the per-edge form writes no jitter)
  int n_jitter;             // <= 5
  float *origins, *directions;
  int* cam_idx;
  float *image, *mask;
  float near, far;
  int kind, S0;
  const float* base_bins;   // [S0 + 1]
  float *spacing0, *euclid0;   // [R, S0 + 1] out
  int nb_rays;              // workgroups of the per-ray role
};

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
    // pixel sampling + ray generation: k_sample_pixels, with the ray's corrected camera formed in place
    int k = (int)(rnd[0] * (float)a.n_train);
    int y = (int)(rnd[1] * (float)a.set.H);
    int x = (int)(rnd[2] * (float)a.set.W);
    k = min(k, a.n_train - 1);
    y = min(y, a.set.H - 1);
    x = min(x, a.set.W - 1);
    const long long img = a.train_ids[k];
    float dx, dy, dz;
    if constexpr (CAMS) {
      float dc[3];
      pixel_direction(cams.intrinsics + 4 * img, cams.distortion ? cams.distortion + 6 * img : nullptr, x, y, dc);
      dx = dc[0], dy = dc[1], dz = dc[2];
    } else {
      dx = fdiv(fsub(fadd((float)x, 0.5f), a.set.cx), a.set.fx);
      dy = -fdiv(fsub(fadd((float)y, 0.5f), a.set.cy), a.set.fy);
      dz = -1.0f;
    }
    float M[12];
    if (a.pose) {
      adjusted_camera<MODE>(a.set.c2w + img * 12, a.pose + 6 * k, M);
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) M[i] = a.set.c2w[img * 12 + i];
    }
    float d[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) d[q] = fadd(fadd(fmul(M[4 * q], dx), fmul(M[4 * q + 1], dy)), fmul(M[4 * q + 2], dz));
    const float nrm = fmaxf(sqrtf(fadd(fadd(fmul(d[0], d[0]), fmul(d[1], d[1])), fmul(d[2], d[2]))), 1e-12f);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      a.directions[3 * r + q] = fdiv(d[q], nrm);
      a.origins[3 * r + q] = M[4 * q + 3];
    }
    a.cam_idx[r] = k;
    const size_t pix = ((size_t)img * a.set.H + y) * a.set.W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.image[3 * r + c] = fdiv((float)a.set.images[3 * pix + c], 255.0f);
    a.mask[r] = (float)a.set.masks[pix];
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
// Same arithmetic as k_sample_pixels<true> on the `u` that selects the pixel (tests/test_gpu_camera_models.py).
__global__ __launch_bounds__(256) void k_camera_rays(const float* __restrict__ c2w, const float* __restrict__ K,
                                                     const float* __restrict__ D, int W, int y0, long long n_pix,
                                                     float* __restrict__ origins, float* __restrict__ directions) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_pix) return;
  const int row = (int)(r / W);
  const int x = (int)(r - (long long)row * W), y = y0 + row;
  float dc[3];
  pixel_direction(K, D, x, y, dc);
  const float* M = c2w;
  float d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    d[a] = fadd(fadd(fmul(M[4 * a], dc[0]), fmul(M[4 * a + 1], dc[1])), fmul(M[4 * a + 2], dc[2]));
  const float nrm = fmaxf(sqrtf(fadd(fadd(fmul(d[0], d[0]), fmul(d[1], d[1])), fmul(d[2], d[2]))), 1e-12f);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    directions[3 * r + a] = fdiv(d[a], nrm);
    origins[3 * r + a] = M[4 * a + 3];
  }
}

}  // namespace fnr

using namespace fnr;

// cams: NULL for the set-wide pinhole (fnr_sample_pixels), the camera table of the _cams variant otherwise
static int sample_pixels(const char* name, const fnr_image_set* set, const fnr_camera_table* cams, bool use_cams,
                         const int64_t* train_ids, int n_train, int64_t n_rays, const float* u, const float* c2w_adjusted,
                         float* origins, float* directions, int32_t* camera_indices, float* image, float* fruit_mask,
                         void* stream) {
  FNR_SEQ_UNRECORDABLE(name);
  FNR_CHECK_ARG(!use_cams || (cams && cams->intrinsics), "sample_pixels_cams: null camera table");
  FNR_CHECK_ARG(set && train_ids && u && origins && directions && camera_indices && image && fruit_mask,
                "sample_pixels: null argument");
  FNR_CHECK_ARG(set->images && set->masks && set->c2w && set->n_images > 0 && set->H > 0 && set->W > 0 && n_train > 0,
                "sample_pixels: bad image set");
  if (n_rays == 0) return FNR_OK;
  ImageSetDev s{set->n_images, set->H, set->W, set->images, set->masks, set->c2w, set->fx, set->fy, set->cx, set->cy};
  const CameraTableDev t = use_cams ? CameraTableDev{cams->intrinsics, cams->distortion} : CameraTableDev{nullptr, nullptr};
  const auto kernel = use_cams ? k_sample_pixels<true> : k_sample_pixels<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, as_stream(stream), s, t,
                     reinterpret_cast<const long long*>(train_ids), n_train, (long long)n_rays, u, c2w_adjusted, origins,
                     directions, camera_indices, image, fruit_mask);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

extern "C" int fnr_sample_pixels(const fnr_image_set* set, const int64_t* train_ids, int n_train, int64_t n_rays,
                                 const float* u, const float* c2w_adjusted, float* origins, float* directions,
                                 int32_t* camera_indices, float* image, float* fruit_mask, void* stream) {
  return sample_pixels("fnr_sample_pixels", set, nullptr, false, train_ids, n_train, n_rays, u, c2w_adjusted, origins,
                       directions, camera_indices, image, fruit_mask, stream);
}

extern "C" int fnr_sample_pixels_cams(const fnr_image_set* set, const fnr_camera_table* cams, const int64_t* train_ids,
                                      int n_train, int64_t n_rays, const float* u, const float* c2w_adjusted,
                                      float* origins, float* directions, int32_t* camera_indices, float* image,
                                      float* fruit_mask, void* stream) {
  return sample_pixels("fnr_sample_pixels_cams", set, cams, true, train_ids, n_train, n_rays, u, c2w_adjusted, origins,
                       directions, camera_indices, image, fruit_mask, stream);
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

// name: the entry point that was called, which is what a step program lists for the recorded call
// edges: the per-edge form (fnr_train_prologue_edges; jitter == NULL, n_jitter == 0)
static int train_prologue(const char* name, bool edges, const fnr_image_set* set, const fnr_camera_table* cams, bool use_cams,
                          int pose_mode, const int64_t* train_ids,
                          int n_train, int64_t n_rays, uint64_t seed, uint64_t offset, const float* pose_adjustment,
                          float* c2w_adjusted, float* u, float* jitter, int n_jitter, float* origins, float* directions,
                          int32_t* camera_indices, float* image, float* fruit_mask, float near_plane, float far_plane,
                          int spacing_kind, int S0, const float* base_bins, float* spacing0, float* euclid0,
                          void* stream) {
  if (seq::recording() && set && (!use_cams || cams)) {
    const fnr_image_set set_ = *set;
    const fnr_camera_table cams_ = use_cams ? *cams : fnr_camera_table{nullptr, nullptr};
    seq::push(name, [=](const fnr_step_scalars* sc) {
      return train_prologue(name, edges, &set_, &cams_, use_cams, pose_mode, train_ids, n_train, n_rays, seed,
                            sc ? sc->prologue_offset : offset,
                            pose_adjustment, c2w_adjusted, u, jitter, n_jitter, origins, directions, camera_indices, image,
                            fruit_mask, near_plane, far_plane, spacing_kind, S0, base_bins, spacing0, euclid0, stream);
    });
  }
  FNR_CHECK_ARG(pose_mode == FNR_POSE_SO3XR3 || pose_mode == FNR_POSE_SE3, "train_prologue: pose_mode %d (0 = SO3xR3, 1 = SE3)",
                pose_mode);
  FNR_CHECK_ARG(!use_cams || (cams && cams->intrinsics), "train_prologue_cams: null camera table");
  FNR_CHECK_ARG(set && train_ids && u && (jitter || edges) && origins && directions && camera_indices && image && fruit_mask &&
                    base_bins && spacing0 && euclid0,
                "train_prologue: null argument");
  FNR_CHECK_ARG(set->images && set->masks && set->c2w && set->n_images > 0 && set->H > 0 && set->W > 0 && n_train > 0,
                "train_prologue: bad image set");
  FNR_CHECK_ARG(edges || (n_jitter >= 1 && n_jitter <= FNR_TRAIN_PROLOGUE_MAX_JITTER && S0 >= 1),
                "train_prologue: n_jitter %d (1..%d), S0 %d", n_jitter, FNR_TRAIN_PROLOGUE_MAX_JITTER, S0);
  FNR_CHECK_ARG(!edges || (S0 >= 1 && S0 < FNR_EDGE_JITTER_MAX_EDGES), "train_prologue_edges: S0 %d (1..%d)", S0,
                FNR_EDGE_JITTER_MAX_EDGES - 1);
  FNR_CHECK_ARG((pose_adjustment == nullptr) == (c2w_adjusted == nullptr), "train_prologue: pose and c2w_adjusted go together");
  FNR_CHECK_ARG(n_rays >= n_train || !pose_adjustment, "train_prologue: fewer rays than cameras");
  if (n_rays == 0) return FNR_OK;
  PrologueArgs a;
  a.set = ImageSetDev{set->n_images, set->H, set->W, set->images, set->masks, set->c2w, set->fx, set->fy, set->cx, set->cy};
  a.train_ids = reinterpret_cast<const long long*>(train_ids);
  a.n_train = n_train, a.n_rays = n_rays, a.seed = seed, a.offset = offset;
  a.pose = pose_adjustment, a.c2w_adjusted = c2w_adjusted, a.u = u, a.jitter = jitter, a.n_jitter = n_jitter;
  a.origins = origins, a.directions = directions, a.cam_idx = camera_indices, a.image = image, a.mask = fruit_mask;
  a.near = near_plane, a.far = far_plane, a.kind = spacing_kind, a.S0 = S0, a.base_bins = base_bins;
  a.spacing0 = spacing0, a.euclid0 = euclid0;
  a.nb_rays = (int)((n_rays + 255) / 256);
  // (per edge: one thread per quad of edges)
  const long long nb_bins = ((edges ? n_rays * (long long)((S0 + 4) >> 2) : n_rays * (long long)(S0 + 1)) + 255) / 256;
  FNR_PROF(OP_SAMPLE_SPACED, n_rays * (long long)(S0 + 1));
  const CameraTableDev t = use_cams ? CameraTableDev{cams->intrinsics, cams->distortion} : CameraTableDev{nullptr, nullptr};
  const auto kernel =
      edges ? (pose_mode == FNR_POSE_SE3
                   ? (use_cams ? k_train_prologue<true, FNR_POSE_SE3, true> : k_train_prologue<false, FNR_POSE_SE3, true>)
                   : (use_cams ? k_train_prologue<true, FNR_POSE_SO3XR3, true> : k_train_prologue<false, FNR_POSE_SO3XR3, true>))
            : (pose_mode == FNR_POSE_SE3
                   ? (use_cams ? k_train_prologue<true, FNR_POSE_SE3> : k_train_prologue<false, FNR_POSE_SE3>)
                   : (use_cams ? k_train_prologue<true, FNR_POSE_SO3XR3> : k_train_prologue<false, FNR_POSE_SO3XR3>));
  hipLaunchKernelGGL(kernel, dim3((unsigned)(a.nb_rays + nb_bins)), dim3(256), 0, as_stream(stream), a, t);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

extern "C" int fnr_train_prologue(const fnr_image_set* set, const int64_t* train_ids, int n_train, int64_t n_rays,
                                  uint64_t seed, uint64_t offset, const float* pose_adjustment, float* c2w_adjusted,
                                  float* u, float* jitter, int n_jitter, float* origins, float* directions,
                                  int32_t* camera_indices, float* image, float* fruit_mask, float near_plane,
                                  float far_plane, int spacing_kind, int S0, const float* base_bins, float* spacing0,
                                  float* euclid0, void* stream) {
  return train_prologue("fnr_train_prologue", false, set, nullptr, false, FNR_POSE_SO3XR3, train_ids, n_train, n_rays, seed, offset,
                        pose_adjustment, c2w_adjusted, u, jitter, n_jitter, origins, directions, camera_indices, image,
                        fruit_mask, near_plane, far_plane, spacing_kind, S0, base_bins, spacing0, euclid0, stream);
}

extern "C" int fnr_train_prologue_cams(const fnr_image_set* set, const fnr_camera_table* cams, const int64_t* train_ids,
                                       int n_train, int64_t n_rays, uint64_t seed, uint64_t offset,
                                       const float* pose_adjustment, float* c2w_adjusted, float* u, float* jitter,
                                       int n_jitter, float* origins, float* directions, int32_t* camera_indices,
                                       float* image, float* fruit_mask, float near_plane, float far_plane,
                                       int spacing_kind, int S0, const float* base_bins, float* spacing0, float* euclid0,
                                       void* stream) {
  return train_prologue("fnr_train_prologue_cams", false, set, cams, true, FNR_POSE_SO3XR3, train_ids, n_train, n_rays, seed, offset,
                        pose_adjustment, c2w_adjusted, u, jitter, n_jitter, origins, directions, camera_indices, image,
                        fruit_mask, near_plane, far_plane, spacing_kind, S0, base_bins, spacing0, euclid0, stream);
}

extern "C" int fnr_train_prologue_mode(const fnr_image_set* set, const fnr_camera_table* cams, int pose_mode,
                                       const int64_t* train_ids, int n_train, int64_t n_rays, uint64_t seed, uint64_t offset,
                                       const float* pose_adjustment, float* c2w_adjusted, float* u, float* jitter,
                                       int n_jitter, float* origins, float* directions, int32_t* camera_indices,
                                       float* image, float* fruit_mask, float near_plane, float far_plane,
                                       int spacing_kind, int S0, const float* base_bins, float* spacing0, float* euclid0,
                                       void* stream) {
  return train_prologue("fnr_train_prologue_mode", false, set, cams, cams != nullptr, pose_mode, train_ids, n_train, n_rays, seed,
                        offset, pose_adjustment, c2w_adjusted, u, jitter, n_jitter, origins, directions, camera_indices,
                        image, fruit_mask, near_plane, far_plane, spacing_kind, S0, base_bins, spacing0, euclid0, stream);
}

extern "C" int fnr_train_prologue_edges(const fnr_image_set* set, const fnr_camera_table* cams, int pose_mode,
                                        const int64_t* train_ids, int n_train, int64_t n_rays, uint64_t seed, uint64_t offset,
                                        const float* pose_adjustment, float* c2w_adjusted, float* u, float* origins,
                                        float* directions, int32_t* camera_indices, float* image, float* fruit_mask,
                                        float near_plane, float far_plane, int spacing_kind, int S0, const float* base_bins,
                                        float* spacing0, float* euclid0, void* stream) {
  return train_prologue("fnr_train_prologue_edges", true, set, cams, cams != nullptr, pose_mode, train_ids, n_train, n_rays, seed,
                        offset, pose_adjustment, c2w_adjusted, u, nullptr, 0, origins, directions, camera_indices, image,
                        fruit_mask, near_plane, far_plane, spacing_kind, S0, base_bins, spacing0, euclid0, stream);
}

extern "C" int fnr_edge_jitter(uint64_t seed, uint64_t offset, int level, int64_t n_rays, int n_edges, float* out,
                               void* stream) {
  if (seq::recording()) {
    seq::push("fnr_edge_jitter", [=](const fnr_step_scalars* sc) {
      return fnr_edge_jitter(seed, sc ? sc->prologue_offset : offset, level, n_rays, n_edges, out, stream);
    });
  }
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
  if (seq::recording()) {
    seq::push("fnr_random_background", [=](const fnr_step_scalars* sc) {
      return fnr_random_background(seed, sc ? sc->prologue_offset : offset, n_rays, out, stream);
    });
  }
  FNR_CHECK_ARG(out && n_rays >= 0, "random_background: null argument or negative ray count");
  if (n_rays == 0) return FNR_OK;
  hipLaunchKernelGGL(k_random_background, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, as_stream(stream),
                     (unsigned long long)seed, (unsigned long long)offset, (long long)n_rays, out);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}
