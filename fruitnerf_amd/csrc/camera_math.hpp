// camera_math.hpp — SO3xR3 and SE3 exponential maps and pose composition shared by camera_opt.hip (k_camera_adjust,
// k_camera_pose_grad) and pixel_sampler.hip (fnr_train_prologue computes a ray's corrected camera in place).
// nerfstudio 0.3.2 CameraOptimizer(mode="SO3xR3" | "SE3") semantics, see camera_opt.hip.
// pixel -> ray, one function per step, for k_sample_pixels, k_train_prologue, k_camera_rays and the recompute in
// k_camera_pose_grad: pick_pixel (u -> clamped slot, row, column), pixel_direction / camera_direction (camera-frame direction
// through a camera-table row — intrinsics + OpenCV distortion — or the set-wide pinhole, a table row without distortion),
// world_ray (origin + unit direction), gather_target (rgb / 255 and mask).  A change to ray generation is made here, once.
// Host side, at the end: CameraCall, the one argument block of the family's entry points, its validator and kernel selection.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace fnr {

struct SO3 {
  float R[9];
  float theta2_raw, theta, f1, f2;
};

__device__ __forceinline__ SO3 so3_exp(const float* w) {
  SO3 s;
  s.theta2_raw = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const float t2 = fmaxf(s.theta2_raw, 1e-4f);
  s.theta = sqrtf(t2);
  const float inv = 1.0f / s.theta;
  s.f1 = inv * sinf(s.theta);
  s.f2 = inv * inv * (1.0f - cosf(s.theta));
  // K = [[0,-wz,wy],[wz,0,-wx],[-wy,wx,0]];  K^2 = w w^T - |w|^2 I
  const float x = w[0], y = w[1], z = w[2];
  const float K[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
  const float K2[9] = {-(y * y + z * z), x * y, x * z, x * y, -(x * x + z * z), y * z, x * z, y * z, -(x * x + y * y)};
#pragma unroll
  for (int i = 0; i < 9; ++i) s.R[i] = s.f1 * K[i] + s.f2 * K2[i] + ((i % 4 == 0) ? 1.0f : 0.0f);
  return s;
}

// ---- SE3 (nerfstudio 0.3.2 lie_groups.exp_map_SE3, restated) ---------------------------------------------------------------
// tv = (v, w): theta = |w| (no clamp), s = theta^2;
//   R = c I + b_r w w^T + a_r K(w),   t = a_t v + b_t (w x v) + c_t w (w . v)
// theta >= 1e-2:  c = cos, a_r = a_t = sin / theta, b_r = b_t = (1 - cos) / s, c_t = (theta - sin) / theta^3
// theta <  1e-2:  c = 8 / (4 + s) - 1, a_r = c / 2 + 1 / 2, b_r = a_r / 2;  a_t = 1 - s / 6, b_t = 1 / 2 - s / 24,
//                 c_t = 1 / 6 - s / 120   (the library's two different polynomials; threshold and polynomials are semantics)
// The derivatives are in the branch's variable x (theta above the threshold, s below); D = dx/dw without the factor w
// (1 / theta, or 2).  Host-callable: the arithmetic is checked on the CPU as well.
struct SE3Coef {
  float c, ar, br, at, bt, ct;
  float dc, dar, dbr, dat, dbt, dct, D;
};

__host__ __device__ __forceinline__ SE3Coef se3_coef(const float* w) {
  SE3Coef k;
  const float s = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const float th = sqrtf(s);
  if (th < 1e-2f) {
    const float q = 4.0f + s;
    k.c = 8.0f / q - 1.0f;
    k.ar = 0.5f * k.c + 0.5f;
    k.br = 0.5f * k.ar;
    k.at = 1.0f - s / 6.0f;
    k.bt = 0.5f - s / 24.0f;
    k.ct = 1.0f / 6.0f - s / 120.0f;
    k.dc = -8.0f / (q * q);
    k.dar = 0.5f * k.dc;
    k.dbr = 0.25f * k.dc;
    k.dat = -1.0f / 6.0f;
    k.dbt = -1.0f / 24.0f;
    k.dct = -1.0f / 120.0f;
    k.D = 2.0f;
  } else {
    const float inv = 1.0f / th, sn = sinf(th), sh = sinf(0.5f * th);
    k.c = cosf(th);
    k.ar = k.at = sn * inv;
    k.br = k.bt = 2.0f * sh * sh / s;       // (1 - cos) / theta^2 without the cancellation
    k.ct = (th - sn) / (th * s);
    k.dc = -sn;
    k.dar = k.dat = (k.c - k.ar) * inv;     // d(sin t / t)/dt
    k.dbr = k.dbt = (k.ar - 2.0f * k.br) * inv;   // d((1 - cos t) / t^2)/dt
    k.dct = (k.br - 3.0f * k.ct) * inv;     // d((t - sin t) / t^3)/dt
    k.D = inv;
  }
  return k;
}

// exp_map_SE3(tv [6]) -> R [9] row-major, t [3]
__host__ __device__ __forceinline__ void se3_exp(const float* __restrict__ tv, float (&R)[9], float (&t)[3]) {
  const float* v = tv;
  const float* w = tv + 3;
  const SE3Coef k = se3_coef(w);
  const float x = w[0], y = w[1], z = w[2];
  const float K[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) R[3 * a + b] = ((a == b) ? k.c : 0.0f) + k.br * (w[a] * w[b]) + k.ar * K[3 * a + b];
  const float wv = x * v[0] + y * v[1] + z * v[2];
  const float cr[3] = {y * v[2] - z * v[1], z * v[0] - x * v[2], x * v[1] - y * v[0]};  // w x v
#pragma unroll
  for (int a = 0; a < 3; ++a) t[a] = k.at * v[a] + k.bt * cr[a] + k.ct * (w[a] * wv);
}

// Backward of se3_exp: GR [9] = dL/dR, gt [3] = dL/dt  ->  gv [3] = dL/dv, gw [3] = dL/dw.  Finite at w = 0, where
// dL/dw = gK + (v x gt) / 2: a pose table that starts at zero trains.
__host__ __device__ __forceinline__ void se3_exp_bwd(const float* __restrict__ tv, const float (&GR)[9], const float (&gt)[3],
                                                     float (&gv)[3], float (&gw)[3]) {
  const float* v = tv;
  const float* w = tv + 3;
  const SE3Coef k = se3_coef(w);
  const float x = w[0], y = w[1], z = w[2];
  const float wg = x * gt[0] + y * gt[1] + z * gt[2], wv = x * v[0] + y * v[1] + z * v[2];
  const float gv_ = gt[0] * v[0] + gt[1] * v[1] + gt[2] * v[2];
  const float gxw[3] = {gt[1] * z - gt[2] * y, gt[2] * x - gt[0] * z, gt[0] * y - gt[1] * x};              // gt x w
  const float vxg[3] = {v[1] * gt[2] - v[2] * gt[1], v[2] * gt[0] - v[0] * gt[2], v[0] * gt[1] - v[1] * gt[0]};  // v x gt
  // <GR, K(e_i)>;  (GR + GR^T) w;  tr GR;  w^T GR w;  <GR, K(w)> = w . gK;  gt . (w x v) = w . (v x gt)
  const float gK[3] = {GR[7] - GR[5], GR[2] - GR[6], GR[3] - GR[1]};
  const float Sw[3] = {(GR[0] + GR[0]) * x + (GR[1] + GR[3]) * y + (GR[2] + GR[6]) * z,
                       (GR[3] + GR[1]) * x + (GR[4] + GR[4]) * y + (GR[5] + GR[7]) * z,
                       (GR[6] + GR[2]) * x + (GR[7] + GR[5]) * y + (GR[8] + GR[8]) * z};
  const float tr = GR[0] + GR[4] + GR[8];
  const float wGw = 0.5f * (x * Sw[0] + y * Sw[1] + z * Sw[2]);
  const float gkw = x * gK[0] + y * gK[1] + z * gK[2];
  const float gwv = x * vxg[0] + y * vxg[1] + z * vxg[2];
  const float through = k.D * ((k.dc * tr + k.dbr * wGw + k.dar * gkw) + (k.dat * gv_ + k.dbt * gwv + k.dct * (wg * wv)));
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    gv[i] = k.at * gt[i] + k.bt * gxw[i] + k.ct * (w[i] * wg);
    gw[i] = (k.ar * gK[i] + k.br * Sw[i]) + (k.bt * vxg[i] + k.ct * (wv * gt[i] + wg * v[i])) + w[i] * through;
  }
}

// out [3,4] = multiply(M [3,4], exp_map(tv [6])):  R' = R1 R,  t' = t1 + R1 t;  MODE: FNR_POSE_SO3XR3 (t = tv[:3]) or
// FNR_POSE_SE3
template <int MODE = FNR_POSE_SO3XR3>
__device__ __forceinline__ void adjusted_camera(const float* __restrict__ M, const float* __restrict__ tv, float (&out)[12]) {
  float R[9], t[3];
  if constexpr (MODE == FNR_POSE_SE3) {
    se3_exp(tv, R, t);
  } else {
    const SO3 s = so3_exp(tv + 3);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = s.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = tv[i];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b)
      out[4 * a + b] = M[4 * a] * R[b] + M[4 * a + 1] * R[3 + b] + M[4 * a + 2] * R[6 + b];
    out[4 * a + 3] = M[4 * a + 3] + (M[4 * a] * t[0] + M[4 * a + 1] * t[1] + M[4 * a + 2] * t[2]);
  }
}

// ---- per-image cameras (fnr_camera_table) -------------------------------------------------------------------------------
struct CameraTableDev {
  const float* intrinsics;  // [M,4] fx, fy, cx, cy
  const float* distortion;  // [M,6] k1, k2, k3, k4, p1, p2, or NULL
};

// Inverse of the OpenCV forward model  xd = d xu + 2 p1 xu yu + p2 (r + 2 xu^2),  yd = d yu + 2 p2 xu yu + p1 (r + 2 yu^2),
// r = xu^2 + yu^2, d = 1 + r (k1 + r (k2 + r (k3 + r k4))):  exactly 10 Newton steps from (xd, yd) with the analytic 2x2
// Jacobian, a step being zero where |det| <= 1e-9 (the multinerf / Nerfstudio radial_and_tangential_undistort routine as
// recalled).  No early exit: every lane runs the same instructions, a ray's bits do not depend on its
// neighbours.  All-zero coefficients: the first residual is exactly 0 and (x, y) stays (xd, yd) bit for bit.
__device__ __forceinline__ void undistort_opencv(const float* __restrict__ kd, float xd, float yd, float& xu, float& yu) {
  const float k1 = kd[0], k2 = kd[1], k3 = kd[2], k4 = kd[3], p1 = kd[4], p2 = kd[5];
  float x = xd, y = yd;
#pragma unroll 1
  for (int it = 0; it < 10; ++it) {
    const float r = x * x + y * y;
    const float d = 1.0f + r * (k1 + r * (k2 + r * (k3 + r * k4)));
    const float fx = d * x + 2.0f * p1 * x * y + p2 * (r + 2.0f * x * x) - xd;
    const float fy = d * y + 2.0f * p2 * x * y + p1 * (r + 2.0f * y * y) - yd;
    const float d_r = k1 + r * (2.0f * k2 + r * (3.0f * k3 + r * 4.0f * k4));
    const float d_x = 2.0f * x * d_r, d_y = 2.0f * y * d_r;
    const float fx_x = d + d_x * x + 2.0f * p1 * y + 6.0f * p2 * x;
    const float fx_y = d_y * x + 2.0f * p1 * x + 2.0f * p2 * y;
    const float fy_x = d_x * y + 2.0f * p2 * y + 2.0f * p1 * x;
    const float fy_y = d + d_y * y + 2.0f * p2 * x + 6.0f * p1 * y;
    const float det = fx_x * fy_y - fx_y * fy_x;
    const bool ok = fabsf(det) > 1e-9f;
    const float inv = 1.0f / (ok ? det : 1.0f);
    const float sx = (fx * fy_y - fy * fx_y) * inv;
    const float sy = (fy * fx_x - fx * fy_x) * inv;
    x -= ok ? sx : 0.0f;
    y -= ok ? sy : 0.0f;
  }
  xu = x, yu = y;
}

// Camera-frame direction of pixel (x, y) of the camera with intrinsics row K = (fx, fy, cx, cy) and distortion row D
// (NULL = pinhole):  OpenCV image coordinates (y down) -> undistort -> flip to the Nerfstudio camera frame (y up, -z
// forward).  Whether nerfstudio 0.3.2 flips before or after undistorting is recalled-only: undistorting after
// the flip differs by the sign of p1 alone, and THIS is the line to change.
__device__ __forceinline__ void pixel_direction(const float* __restrict__ K, const float* __restrict__ D, int x, int y,
                                                float (&dc)[3]) {
  float xu = fdiv(fsub(fadd((float)x, 0.5f), K[2]), K[0]);
  float yu = fdiv(fsub(fadd((float)y, 0.5f), K[3]), K[1]);
  if (D) undistort_opencv(D, xu, yu, xu, yu);
  dc[0] = xu, dc[1] = -yu, dc[2] = -1.0f;
}

// ---- pixel -> ray: the ONE copy of each step, for every kernel that makes a ray or makes it again -----------------------------
struct PixelGrid {
  int H, W;
  float fx, fy, cx, cy;  // the set-wide pinhole (kernels without a camera table)
};

struct ImageSetDev {
  int n_images;
  PixelGrid grid;         // (all that k_camera_pose_grad takes of the set, next to its cameras)
  const uint8_t* images;  // [M,H,W,3]
  const uint8_t* masks;   // [M,H,W]
  const float* c2w;       // [M,3,4]
};

struct Pixel {
  int k, y, x;  // training slot (camera index = appearance-embedding row), pixel row, pixel column
};

// indices = floor(rand * [n_train, H, W]) (PixelSampler.sample_method), clamped like the torch mirror
__device__ __forceinline__ Pixel pick_pixel(const float* __restrict__ u, int n_train, int H, int W) {
  Pixel p{(int)(u[0] * (float)n_train), (int)(u[1] * (float)H), (int)(u[2] * (float)W)};
  p.k = min(p.k, n_train - 1);
  p.y = min(p.y, H - 1);
  p.x = min(p.x, W - 1);
  return p;
}

// pixel_direction of dataset image `img`: through its camera-table row (CAMS) or the set-wide pinhole
template <bool CAMS>
__device__ __forceinline__ void camera_direction(const PixelGrid& g, const CameraTableDev& cams, long long img, int x, int y,
                                                 float (&dc)[3]) {
  if constexpr (CAMS) {
    pixel_direction(cams.intrinsics + 4 * img, cams.distortion ? cams.distortion + 6 * img : nullptr, x, y, dc);
  } else {
    const float K[4] = {g.fx, g.fy, g.cx, g.cy};
    pixel_direction(K, nullptr, x, y, dc);
  }
}

// camera M [3,4] and camera-frame direction dc -> origin = the translation column, direction = normalize(R dc)
__device__ __forceinline__ void world_ray(const float* __restrict__ M, const float (&dc)[3], float* __restrict__ origin,
                                          float* __restrict__ direction) {
  float d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    d[a] = fadd(fadd(fmul(M[4 * a], dc[0]), fmul(M[4 * a + 1], dc[1])), fmul(M[4 * a + 2], dc[2]));
  const float nrm = fmaxf(sqrtf(fadd(fadd(fmul(d[0], d[0]), fmul(d[1], d[1])), fmul(d[2], d[2]))), 1e-12f);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    direction[a] = fdiv(d[a], nrm);
    origin[a] = M[4 * a + 3];
  }
}

// the training targets of pixel (y, x) of dataset image `img`: rgb / 255 and the fruit mask
__device__ __forceinline__ void gather_target(const ImageSetDev& s, long long img, int y, int x, float* __restrict__ rgb,
                                              float* __restrict__ mask) {
  const size_t pix = ((size_t)img * s.grid.H + y) * s.grid.W + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) rgb[c] = fdiv((float)s.images[3 * pix + c], 255.0f);
  *mask = (float)s.masks[pix];
}

// ---- host side: one argument block for the family (fnr_sample_pixels*, fnr_train_prologue*, fnr_camera_adjust*,
// fnr_camera_pose_grad*, fnr_camera_pose_grad_adam*).  An entry point fills it with what every call shares, puts the
// operation's own pointers in the operation's struct next to it, and calls the operation; the kernels keep their parameters.
struct CameraCall {
  const char* name;        // the entry point that was called: what a step program lists for the recorded call
  ImageSetDev set;         // by value, as the kernels take them: a recorded call outlives the caller's structs
  CameraTableDev cams;     // (NULL rows unless use_cams)
  bool has_set, has_cams;  // the caller's pointers were not NULL
  bool use_cams;           // rays go through the table (a _cams entry point, or a _mode / _edges one given a table)
  int pose_mode;
  const long long* train_ids;
  int n_train;
  long long n_rays;
  void* stream;
};

static inline CameraCall camera_call(const char* name, const fnr_image_set* s, const fnr_camera_table* cams, bool use_cams,
                                     int pose_mode, const int64_t* train_ids, int n_train, int64_t n_rays, void* stream) {
  return {name, s ? ImageSetDev{s->n_images, {s->H, s->W, s->fx, s->fy, s->cx, s->cy}, s->images, s->masks, s->c2w} : ImageSetDev{},
          use_cams && cams ? CameraTableDev{cams->intrinsics, cams->distortion} : CameraTableDev{}, s != nullptr, cams != nullptr,
          use_cams, pose_mode, reinterpret_cast<const long long*>(train_ids), n_train, n_rays, stream};
}

// fnr_train_prologue*'s own arguments (pixel_sampler.hip), as an entry point fills them, then what train_prologue() adds from
// the call's CameraCall.
struct PrologueArgs {
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
  ImageSetDev set;
  const long long* train_ids;
  int n_train;
  long long n_rays;
  int nb_rays;              // workgroups of the per-ray role
};
// replayed from a step program (sequencer.hpp): the step's random-number counter
static inline PrologueArgs patched(PrologueArgs a, const fnr_step_scalars* s) {
  if (s) a.offset = s->prologue_offset;
  return a;
}

// The checks every operation starts with, in this order.  op: the operation, as its messages name it;  own: its own pointers
// are all there;  images: it reads the set's images and masks, not only its cameras.
static inline int check_camera_call(const CameraCall& c, const char* op, bool own, bool images) {
  const ImageSetDev& s = c.set;
  FNR_CHECK_ARG(c.pose_mode == FNR_POSE_SO3XR3 || c.pose_mode == FNR_POSE_SE3, "%s: pose_mode %d (0 = SO3xR3, 1 = SE3)", op,
                c.pose_mode);
  FNR_CHECK_ARG(!c.use_cams || (c.has_cams && c.cams.intrinsics), "%s_cams: null camera table", op);
  FNR_CHECK_ARG(c.has_set && c.train_ids && own && (images || (s.c2w && c.n_train > 0)), "%s: null argument", op);
  FNR_CHECK_ARG(!images || (s.images && s.masks && s.c2w && s.n_images > 0 && s.grid.H > 0 && s.grid.W > 0 && c.n_train > 0),
                "%s: bad image set", op);
  return FNR_OK;
}

// The call's kernel: pick(cams, mode) names it, with decltype(cams)::value = CAMS and decltype(mode)::value = MODE.
template <class Pick>
static inline auto camera_kernel(const CameraCall& c, Pick pick) {
  using SO3xR3 = std::integral_constant<int, FNR_POSE_SO3XR3>;
  using SE3 = std::integral_constant<int, FNR_POSE_SE3>;
  if (c.pose_mode == FNR_POSE_SE3) return c.use_cams ? pick(std::true_type{}, SE3{}) : pick(std::false_type{}, SE3{});
  return c.use_cams ? pick(std::true_type{}, SO3xR3{}) : pick(std::false_type{}, SO3xR3{});
}

}  // namespace fnr
