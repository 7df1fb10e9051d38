// camera_math.hpp — SO3xR3 exponential map and pose composition shared by camera_opt.hip (k_camera_adjust,
// k_camera_pose_grad) and pixel_sampler.hip (fnr_train_prologue computes a ray's corrected camera in place).
// nerfstudio 0.3.2 CameraOptimizer(mode="SO3xR3") semantics, see camera_opt.hip.
// pixel_direction: a pixel's camera-frame direction through a per-image camera table (fnr_camera_table: intrinsics +
// OpenCV distortion), shared by every kernel of the _cams entry points.
#pragma once
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

// out [3,4] = multiply(M [3,4], exp_map_SO3xR3(tv [6])):  R' = R1 R,  t' = t1 + R1 t
__device__ __forceinline__ void adjusted_camera(const float* __restrict__ M, const float* __restrict__ tv, float (&out)[12]) {
  const SO3 s = so3_exp(tv + 3);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b)
      out[4 * a + b] = M[4 * a] * s.R[b] + M[4 * a + 1] * s.R[3 + b] + M[4 * a + 2] * s.R[6 + b];
    out[4 * a + 3] = M[4 * a + 3] + (M[4 * a] * tv[0] + M[4 * a + 1] * tv[1] + M[4 * a + 2] * tv[2]);
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

}  // namespace fnr
