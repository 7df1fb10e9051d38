// cloud_fit.hip — the template fits of the counting stage's second half (clustering/clustering_base.py:260-511),
// batched over all clusters of a cloud, fp64, on gfx950:
//   fnr_cloud_icp        Open3D registration_icp(TransformationEstimationPointToPoint(with_scaling)) (:262-279)
//   fnr_cloud_hausdorff  hausdorff_distance(A, B, "euclidean") (:277, :315) with both witnesses
//
// ICP: one workgroup of 8 waves per problem, persistent over its iterations; convergence is decided on the device.
//   evaluate : every source point (streamed from global memory, one per lane and round) is moved by the current T and
//              searches ALL target points, which sit in LDS (up to FIT_TILE of them stay there for the whole loop; a
//              larger target is passed through the same LDS tile once per round of source points).  Brute force: the
//              search is exact, candidates are visited in ascending index and replace the best only when strictly
//              nearer, so ties go to the lowest target index.  A pair is a correspondence when sqrt(d2) <
//              max_correspondence_distance (STRICT <, like cKDTree's distance_upper_bound and Open3D's hybrid search).
//   estimate : Umeyama on the pairs — means from the evaluate sums, then one pass for the centred 3 x 3 covariance and
//              the source variance; lane 0 of wave 0 takes the SVD (one-sided Jacobi, singular values sorted, third left
//              vector = +-(u1 x u2)), applies the reflection fix and multiplies the update onto T.
//   Every sum is formed in a fixed order: per lane over its own points (ascending), a butterfly over the wave, the 8
//   wave sums in ascending order.  Nothing depends on the other problems of the batch.
//
// Hausdorff: workgroups of 4 waves, each answers 256 queries of one direction of one problem (grid = problems x chunks);
// the other set goes through an LDS tile, the placed template points (source segment + translation, or 4 x 4 transform)
// are formed while the tile is staged and never exist in global memory.  A workgroup leaves (max d2, its query index);
// a second kernel takes the maximum over a problem's chunks in ascending order (strict >: the lowest index on ties).
//
// No atomics, no inter-workgroup communication.
#include <cmath>
#include <vector>

#include "cloud_grid.hpp"
#include "sequencer.hpp"

namespace fnr {
namespace {

constexpr int FIT_TILE = 2048;        // points of the LDS tile (48 KB)
constexpr int ICP_THREADS = 512;
constexpr int ICP_WAVES = ICP_THREADS / 64;
constexpr int HD_THREADS = 256;
constexpr int HD_MAX_CHUNKS = 65535;  // grid.y

struct IcpProb {
  long long t0, s0, c0;   // first target point, first source point, first correspondence
  int nt, ns;
};

struct HdProb {
  long long a0, s0, tr0, part0;   // first point of A, of the source segment, first translation, first partial
  int na, ns, k, use_transform;   // k placements of the segment make B (1 with a transform)
};

struct HdPart {
  double d2;
  int q, pad;
};

// sums of N values over the workgroup, in every thread
template <int N>
__device__ inline void block_sum(double (&v)[N], double* s_red) {
  const int lane = wave_lane(), wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double x = v[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = x + __shfl_xor(x, d, 64);
    v[k] = x;
  }
  __syncthreads();                                              // s_red may still be read from the previous sum
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) s_red[wave * N + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double t = 0.0;
    for (int w = 0; w < ICP_WAVES; ++w) t = t + s_red[w * N + k];
    v[k] = t;
  }
}

// one Hestenes rotation: makes columns P and Q of A orthogonal, V follows
template <int P, int Q>
__device__ inline void hestenes(double (&A)[3][3], double (&V)[3][3]) {
  double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    alpha = alpha + A[r][P] * A[r][P];
    beta = beta + A[r][Q] * A[r][Q];
    gamma = gamma + A[r][P] * A[r][Q];
  }
  if (gamma == 0.0 || !(fabs(gamma) > 1e-17 * sqrt(alpha * beta))) return;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = c * t;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double ap = A[r][P], aq = A[r][Q];
    A[r][P] = c * ap - s * aq;
    A[r][Q] = s * ap + c * aq;
    const double vp = V[r][P], vq = V[r][Q];
    V[r][P] = c * vp - s * vq;
    V[r][Q] = s * vp + c * vq;
  }
}

template <int P, int Q>
__device__ inline void order_columns(double (&A)[3][3], double (&V)[3][3], double (&sig)[3]) {
  if (sig[P] >= sig[Q]) return;
  double t = sig[P]; sig[P] = sig[Q]; sig[Q] = t;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    t = A[r][P]; A[r][P] = A[r][Q]; A[r][Q] = t;
    t = V[r][P]; V[r][P] = V[r][Q]; V[r][Q] = t;
  }
}

__device__ inline double det3(const double (&M)[3][3]) {
  return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
         M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

// Umeyama's similarity from cov = sum (dst - mu_d)(src - mu_s)^T / n and var = sum |src - mu_s|^2 / n, multiplied onto T
__device__ inline void umeyama_onto(const double (&cov)[9], double var, const double (&mu_s)[3], const double (&mu_d)[3],
                                    int with_scaling, double* T) {
  double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) A[r][c] = cov[3 * r + c];
  for (int sweep = 0; sweep < 30; ++sweep) {                     // cov V = U diag(sig): converges in a handful
    hestenes<0, 1>(A, V);
    hestenes<0, 2>(A, V);
    hestenes<1, 2>(A, V);
    double off = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) off = off + fabs(A[r][0] * A[r][1]) + fabs(A[r][0] * A[r][2]) + fabs(A[r][1] * A[r][2]);
    double nrm = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) nrm = nrm + A[r][0] * A[r][0] + A[r][1] * A[r][1] + A[r][2] * A[r][2];
    if (!(off > 1e-17 * nrm)) break;
  }
  double sig[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) sig[c] = sqrt((A[0][c] * A[0][c] + A[1][c] * A[1][c]) + A[2][c] * A[2][c]);
  order_columns<0, 1>(A, V, sig);
  order_columns<1, 2>(A, V, sig);
  order_columns<0, 1>(A, V, sig);

  double U[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  if (sig[0] > 0.0) {
    double u1[3], u2[3], u3[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) u1[r] = A[r][0] / sig[0];
    if (sig[1] > 0.0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) u2[r] = A[r][1] / sig[1];
    } else {                                                      // rank 1: any direction across u1
      const int e = fabs(u1[0]) <= fabs(u1[1]) ? (fabs(u1[0]) <= fabs(u1[2]) ? 0 : 2) : (fabs(u1[1]) <= fabs(u1[2]) ? 1 : 2);
#pragma unroll
      for (int r = 0; r < 3; ++r) u2[r] = r == e ? 1.0 : 0.0;
    }
    const double p = (u1[0] * u2[0] + u1[1] * u2[1]) + u1[2] * u2[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) u2[r] = u2[r] - p * u1[r];
    const double l2 = sqrt((u2[0] * u2[0] + u2[1] * u2[1]) + u2[2] * u2[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) u2[r] = u2[r] / l2;
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    const double side = (u3[0] * A[0][2] + u3[1] * A[1][2]) + u3[2] * A[2][2];
    const double sg = side < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      U[r][0] = u1[r];
      U[r][1] = u2[r];
      U[r][2] = sg * u3[r];
    }
  }
  const double s22 = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;     // the reflection fix
  double scale = 1.0;
  if (with_scaling) scale = var > 0.0 ? ((sig[0] + sig[1]) + s22 * sig[2]) / var : 1.0;
  double up[16];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) up[4 * r + c] = scale * ((U[r][0] * V[c][0] + U[r][1] * V[c][1]) + s22 * U[r][2] * V[c][2]);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
    up[4 * r + 3] = mu_d[r] - ((up[4 * r + 0] * mu_s[0] + up[4 * r + 1] * mu_s[1]) + up[4 * r + 2] * mu_s[2]);
  up[12] = up[13] = up[14] = 0.0;
  up[15] = 1.0;
  double old[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) old[i] = T[i];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      T[4 * r + c] = ((up[4 * r + 0] * old[c] + up[4 * r + 1] * old[4 + c]) + up[4 * r + 2] * old[8 + c]) +
                     up[4 * r + 3] * old[12 + c];
}

// nearest of the m points of the LDS tile (ascending, strict <)
__device__ inline void scan_tile(const double* s_tile, int m, int first, double x, double y, double z, double& best,
                                 int& bi) {
#pragma unroll 4
  for (int j = 0; j < m; ++j) {
    const double dx = x - s_tile[3 * j + 0], dy = y - s_tile[3 * j + 1], dz = z - s_tile[3 * j + 2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 < best) {
      best = d2;
      bi = first + j;
    }
  }
}

__global__ __launch_bounds__(ICP_THREADS) void k_cloud_icp(
    const IcpProb* __restrict__ probs, const double* __restrict__ tgt_xyz, const double* __restrict__ src_xyz,
    const double* __restrict__ init, double max_dist, int with_scaling, int max_iteration, double rel_fitness,
    double rel_rmse, double* __restrict__ T_out, double* __restrict__ fitness_out, double* __restrict__ rmse_out,
    int* __restrict__ iterations_out, int* __restrict__ corr_out) {
  __shared__ double s_tile[3 * FIT_TILE];
  __shared__ double s_red[ICP_WAVES * 10];
  __shared__ double s_T[16];
  const IcpProb P = probs[blockIdx.x];
  const double* tp = tgt_xyz + 3 * P.t0;
  const double* sp = src_xyz + 3 * P.s0;
  int* corr = corr_out + P.c0;
  const int tid = (int)threadIdx.x;
  const bool resident = P.nt <= FIT_TILE;
  if (tid < 16) s_T[tid] = init[16 * (size_t)blockIdx.x + tid];
  if (resident)
    for (int i = tid; i < 3 * P.nt; i += ICP_THREADS) s_tile[i] = tp[i];
  __syncthreads();

  // sum: pairs, sum of the moved source points, of their target points, of d2
  auto evaluate = [&](double (&sum)[8]) {
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = s_T[i];
#pragma unroll
    for (int k = 0; k < 8; ++k) sum[k] = 0.0;
    for (int base = 0; base < P.ns; base += ICP_THREADS) {      // uniform: the tile staging has barriers
      const int i = base + tid;
      const bool valid = i < P.ns;
      double mx = 0.0, my = 0.0, mz = 0.0;
      if (valid) {
        const double x = sp[3 * (size_t)i + 0], y = sp[3 * (size_t)i + 1], z = sp[3 * (size_t)i + 2];
        mx = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
        my = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
        mz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
      }
      double best = __builtin_inf();
      int bi = -1;
      for (int first = 0; first < P.nt; first += FIT_TILE) {
        const int m = P.nt - first < FIT_TILE ? P.nt - first : FIT_TILE;
        if (!resident) {
          __syncthreads();
          for (int j = tid; j < 3 * m; j += ICP_THREADS) s_tile[j] = tp[3 * (size_t)first + j];
          __syncthreads();
        }
        scan_tile(s_tile, m, first, mx, my, mz, best, bi);
      }
      const bool ok = valid && bi >= 0 && sqrt(best) < max_dist;
      if (valid) corr[i] = ok ? bi : -1;
      if (ok) {
        sum[0] = sum[0] + 1.0;
        sum[1] = sum[1] + mx;
        sum[2] = sum[2] + my;
        sum[3] = sum[3] + mz;
        sum[4] = sum[4] + tp[3 * (size_t)bi + 0];
        sum[5] = sum[5] + tp[3 * (size_t)bi + 1];
        sum[6] = sum[6] + tp[3 * (size_t)bi + 2];
        sum[7] = sum[7] + best;
      }
    }
    block_sum<8>(sum, s_red);
  };

  double sum[8];
  evaluate(sum);
  double fitness = P.ns > 0 ? sum[0] / (double)P.ns : 0.0;
  double rmse = sum[0] > 0.0 ? sqrt(sum[7] / sum[0]) : 0.0;
  int it = 0;
  for (int round = 1; round <= max_iteration; ++round) {
    it = round;
    const double cnt = sum[0];
    if (cnt < 3.0) break;
    const double mu_s[3] = {sum[1] / cnt, sum[2] / cnt, sum[3] / cnt};
    const double mu_d[3] = {sum[4] / cnt, sum[5] / cnt, sum[6] / cnt};
    double c[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) c[k] = 0.0;
    {
      double T[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) T[i] = s_T[i];
      for (int i = tid; i < P.ns; i += ICP_THREADS) {
        const int j = corr[i];                                   // this thread's own store
        if (j < 0) continue;
        const double x = sp[3 * (size_t)i + 0], y = sp[3 * (size_t)i + 1], z = sp[3 * (size_t)i + 2];
        const double xs[3] = {(((T[0] * x + T[1] * y) + T[2] * z) + T[3]) - mu_s[0],
                              (((T[4] * x + T[5] * y) + T[6] * z) + T[7]) - mu_s[1],
                              (((T[8] * x + T[9] * y) + T[10] * z) + T[11]) - mu_s[2]};
        const double xd[3] = {tp[3 * (size_t)j + 0] - mu_d[0], tp[3 * (size_t)j + 1] - mu_d[1],
                              tp[3 * (size_t)j + 2] - mu_d[2]};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int q = 0; q < 3; ++q) c[3 * r + q] = c[3 * r + q] + xd[r] * xs[q];
        c[9] = c[9] + ((xs[0] * xs[0] + xs[1] * xs[1]) + xs[2] * xs[2]);
      }
    }
    block_sum<10>(c, s_red);                                     // every read of s_T above is behind its barriers
    if (tid == 0) {
      double cov[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) cov[k] = c[k] / cnt;
      umeyama_onto(cov, c[9] / cnt, mu_s, mu_d, with_scaling, s_T);
    }
    __syncthreads();
    evaluate(sum);
    const double new_fitness = P.ns > 0 ? sum[0] / (double)P.ns : 0.0;
    const double new_rmse = sum[0] > 0.0 ? sqrt(sum[7] / sum[0]) : 0.0;
    const bool done = fabs(fitness - new_fitness) < rel_fitness && fabs(rmse - new_rmse) < rel_rmse;
    fitness = new_fitness;
    rmse = new_rmse;
    if (done) break;
  }
  if (tid < 16) T_out[16 * (size_t)blockIdx.x + tid] = s_T[tid];
  if (tid == 0) {
    fitness_out[blockIdx.x] = fitness;
    rmse_out[blockIdx.x] = rmse;
    iterations_out[blockIdx.x] = it;
  }
}

// ---- Hausdorff -----------------------------------------------------------------------------------------------------
// point i of the source segment under placement p of problem b
__device__ inline void place_point(const HdProb& P, const double* __restrict__ sp, const double* __restrict__ trans,
                                   const double* __restrict__ M, int i, int p, double& x, double& y, double& z) {
  const double sx = sp[3 * (size_t)i + 0], sy = sp[3 * (size_t)i + 1], sz = sp[3 * (size_t)i + 2];
  if (P.use_transform) {
    x = ((M[0] * sx + M[1] * sy) + M[2] * sz) + M[3];
    y = ((M[4] * sx + M[5] * sy) + M[6] * sz) + M[7];
    z = ((M[8] * sx + M[9] * sy) + M[10] * sz) + M[11];
  } else {
    const double* t = trans + 3 * (size_t)(P.tr0 + p);
    x = sx + t[0];
    y = sy + t[1];
    z = sz + t[2];
  }
}

__device__ inline bool farther(double da, int qa, double db, int qb) { return (da > db) | ((da == db) & (qa < qb)); }

__global__ __launch_bounds__(HD_THREADS) void k_cloud_hausdorff(
    const HdProb* __restrict__ probs, const double* __restrict__ a_xyz, const double* __restrict__ src_xyz,
    const double* __restrict__ trans, const double* __restrict__ transforms, HdPart* __restrict__ parts) {
  __shared__ double s_tile[3 * FIT_TILE];
  __shared__ double s_d[HD_THREADS / 64];
  __shared__ int s_q[HD_THREADS / 64];
  const HdProb P = probs[blockIdx.x];
  const long long nb = (long long)P.k * P.ns;
  const int ca = (P.na + HD_THREADS - 1) / HD_THREADS, cb = (int)((nb + HD_THREADS - 1) / HD_THREADS);
  const int chunk = (int)blockIdx.y;
  if (chunk >= ca + cb) return;                                  // the whole workgroup
  const int tid = (int)threadIdx.x;
  const double* ap = a_xyz + 3 * P.a0;
  const double* sp = src_xyz + 3 * P.s0;
  const double* M = transforms ? transforms + 16 * (size_t)blockIdx.x : nullptr;
  const bool from_a = chunk < ca;
  const int q = (from_a ? chunk : chunk - ca) * HD_THREADS + tid;
  const bool valid = from_a ? q < P.na : q < nb;
  double x = 0.0, y = 0.0, z = 0.0;
  double best = __builtin_inf();
  int bi = -1;
  if (from_a) {
    if (valid) {
      x = ap[3 * (size_t)q + 0];
      y = ap[3 * (size_t)q + 1];
      z = ap[3 * (size_t)q + 2];
    }
    for (int p = 0; p < P.k; ++p) {
      for (int first = 0; first < P.ns; first += FIT_TILE) {
        const int m = P.ns - first < FIT_TILE ? P.ns - first : FIT_TILE;
        __syncthreads();
        for (int j = tid; j < m; j += HD_THREADS)
          place_point(P, sp, trans, M, first + j, p, s_tile[3 * j + 0], s_tile[3 * j + 1], s_tile[3 * j + 2]);
        __syncthreads();
        scan_tile(s_tile, m, p * P.ns + first, x, y, z, best, bi);
      }
    }
  } else {
    if (valid) place_point(P, sp, trans, M, q % P.ns, q / P.ns, x, y, z);
    for (int first = 0; first < P.na; first += FIT_TILE) {
      const int m = P.na - first < FIT_TILE ? P.na - first : FIT_TILE;
      __syncthreads();
      for (int j = tid; j < 3 * m; j += HD_THREADS) s_tile[j] = ap[3 * (size_t)first + j];
      __syncthreads();
      scan_tile(s_tile, m, first, x, y, z, best, bi);
    }
  }
  double d = valid ? best : -1.0;                                // d2 >= 0: a lane without a query never wins
  int w = valid ? q : 0x7fffffff;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const double od = __shfl_xor(d, s, 64);
    const int ow = __shfl_xor(w, s, 64);
    if (farther(od, ow, d, w)) {
      d = od;
      w = ow;
    }
  }
  if (wave_lane() == 0) {
    s_d[tid >> 6] = d;
    s_q[tid >> 6] = w;
  }
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < HD_THREADS / 64; ++v)
      if (farther(s_d[v], s_q[v], d, w)) {
        d = s_d[v];
        w = s_q[v];
      }
    HdPart out;
    out.d2 = d;
    out.q = w;
    out.pad = 0;
    parts[P.part0 + chunk] = out;
  }
}

__global__ __launch_bounds__(256) void k_cloud_hausdorff_final(const HdProb* __restrict__ probs, int n_problems,
                                                               const HdPart* __restrict__ parts,
                                                               double* __restrict__ dist, int* __restrict__ witness) {
  const int b = (int)(blockIdx.x * 256u + threadIdx.x);
  if (b >= n_problems) return;
  const HdProb P = probs[b];
  const long long nb = (long long)P.k * P.ns;
  const int ca = (P.na + HD_THREADS - 1) / HD_THREADS, cb = (int)((nb + HD_THREADS - 1) / HD_THREADS);
  double d[2] = {-1.0, -1.0};
  int w[2] = {-1, -1};
  for (int c = 0; c < ca + cb; ++c) {
    const HdPart part = parts[P.part0 + c];
    const int side = c < ca ? 0 : 1;
    if (part.d2 > d[side]) {                                     // chunks ascend in query index: the lowest on ties
      d[side] = part.d2;
      w[side] = part.q;
    }
  }
  if (P.na == 0 || nb == 0) {                                    // the distance to or from an empty set is undefined
    d[0] = d[1] = __builtin_nan("");
    w[0] = w[1] = -1;
  } else {
    d[0] = sqrt(d[0]);
    d[1] = sqrt(d[1]);
  }
  dist[3 * (size_t)b + 0] = d[0];
  dist[3 * (size_t)b + 1] = d[1];
  dist[3 * (size_t)b + 2] = d[0] >= d[1] ? d[0] : (d[1] > d[0] ? d[1] : d[0] + d[1]);
  witness[2 * (size_t)b + 0] = w[0];
  witness[2 * (size_t)b + 1] = w[1];
}

// ---- host side -----------------------------------------------------------------------------------------------------
constexpr long long FIT_MAX_POINTS = 2147483647LL / 4;           // 3 * n fits an int with room to spare

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

static int check_offsets(const char* what, const char* name, const int64_t* offsets, int64_t n_sets, int64_t n_points) {
  FNR_CHECK_ARG(offsets, "%s: null %s", what, name);
  FNR_CHECK_ARG(offsets[0] == 0, "%s: %s[0] must be 0", what, name);
  for (int64_t i = 0; i < n_sets; ++i) {
    FNR_CHECK_ARG(offsets[i + 1] >= offsets[i], "%s: %s are not monotone at %lld", what, name, (long long)i);
    FNR_CHECK_ARG(offsets[i + 1] - offsets[i] <= FIT_MAX_POINTS, "%s: set %lld of %s is too large", what, (long long)i,
                  name);
  }
  FNR_CHECK_ARG(offsets[n_sets] == n_points, "%s: %s end at %lld, not at the %lld points given", what, name,
                (long long)offsets[n_sets], (long long)n_points);
  return FNR_OK;
}

}  // namespace
}  // namespace fnr

using namespace fnr;

extern "C" size_t fnr_cloud_icp_workspace_bytes(int64_t n_problems) {
  return n_problems > 0 ? align256((size_t)n_problems * sizeof(IcpProb)) : 0;
}

extern "C" int fnr_cloud_icp(const double* tgt_xyz, int64_t n_tgt_points, const int64_t* tgt_offsets,
                             int64_t n_problems, const double* src_xyz, int64_t n_src_points,
                             const int64_t* src_offsets, int64_t n_sources, const int32_t* src_id, const double* init,
                             double max_correspondence_distance, int32_t with_scaling, int32_t max_iteration,
                             double relative_fitness, double relative_rmse, double* transformation, double* fitness,
                             double* inlier_rmse, int32_t* iterations, int32_t* correspondences, void* workspace,
                             size_t workspace_bytes, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_cloud_icp");
  FNR_CHECK_ARG(n_problems >= 0 && n_problems < 2147483647LL, "cloud_icp: n_problems out of range");
  FNR_CHECK_ARG(n_tgt_points >= 0 && n_src_points >= 0 && n_sources >= 0, "cloud_icp: negative count");
  FNR_CHECK_ARG(max_correspondence_distance > 0.0, "cloud_icp: max_correspondence_distance must be positive");
  FNR_CHECK_ARG(max_iteration >= 0, "cloud_icp: negative max_iteration");
  if (n_problems == 0) return FNR_OK;
  int rc = check_offsets("cloud_icp", "tgt_offsets", tgt_offsets, n_problems, n_tgt_points);
  if (rc != FNR_OK) return rc;
  rc = check_offsets("cloud_icp", "src_offsets", src_offsets, n_sources, n_src_points);
  if (rc != FNR_OK) return rc;
  FNR_CHECK_ARG(src_id, "cloud_icp: null src_id");
  FNR_CHECK_ARG((tgt_xyz || n_tgt_points == 0) && (src_xyz || n_src_points == 0), "cloud_icp: null points");
  FNR_CHECK_ARG(init && transformation && fitness && inlier_rmse && iterations, "cloud_icp: null init or output");
  std::vector<IcpProb> probs((size_t)n_problems);
  long long c0 = 0;
  for (int64_t b = 0; b < n_problems; ++b) {
    FNR_CHECK_ARG(src_id[b] >= 0 && src_id[b] < n_sources, "cloud_icp: src_id[%lld] = %d outside 0 .. %lld",
                  (long long)b, src_id[b], (long long)n_sources - 1);
    IcpProb& p = probs[(size_t)b];
    p.t0 = tgt_offsets[b];
    p.nt = (int)(tgt_offsets[b + 1] - tgt_offsets[b]);
    p.s0 = src_offsets[src_id[b]];
    p.ns = (int)(src_offsets[src_id[b] + 1] - src_offsets[src_id[b]]);
    p.c0 = c0;
    c0 += p.ns;
  }
  FNR_CHECK_ARG(correspondences || c0 == 0, "cloud_icp: null correspondences");
  FNR_CHECK_ARG(workspace && workspace_bytes >= fnr_cloud_icp_workspace_bytes(n_problems),
                "cloud_icp: workspace too small (need %zu)", fnr_cloud_icp_workspace_bytes(n_problems));
  hipStream_t st = as_stream(stream);
  FNR_PROF(OP_CLOUD, c0);
  FNR_HIP(hipMemcpyWithStream(workspace, probs.data(), probs.size() * sizeof(IcpProb), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_cloud_icp, dim3((unsigned)n_problems), dim3(ICP_THREADS), 0, st, (const IcpProb*)workspace,
                     tgt_xyz, src_xyz, init, max_correspondence_distance, with_scaling ? 1 : 0, max_iteration,
                     relative_fitness, relative_rmse, transformation, fitness, inlier_rmse, iterations, correspondences);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

extern "C" size_t fnr_cloud_hausdorff_workspace_bytes(int64_t n_problems, int64_t n_queries) {
  if (n_problems <= 0 || n_queries < 0) return 0;
  const size_t chunks = (size_t)n_queries / HD_THREADS + 2 * (size_t)n_problems;
  return align256((size_t)n_problems * sizeof(HdProb)) + align256(chunks * sizeof(HdPart));
}

extern "C" int fnr_cloud_hausdorff(const double* a_xyz, int64_t n_a_points, const int64_t* a_offsets, int64_t n_a_sets,
                                   const double* src_xyz, int64_t n_src_points, const int64_t* src_offsets,
                                   int64_t n_sources, int64_t n_problems, const int32_t* a_id, const int32_t* src_id,
                                   const double* translations, int64_t n_translations, const int64_t* trans_offsets,
                                   const double* transforms, double* distances, int32_t* witnesses, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_cloud_hausdorff");
  FNR_CHECK_ARG(n_problems >= 0 && n_problems < 2147483647LL, "cloud_hausdorff: n_problems out of range");
  FNR_CHECK_ARG(n_a_points >= 0 && n_a_sets >= 0 && n_src_points >= 0 && n_sources >= 0 && n_translations >= 0,
                "cloud_hausdorff: negative count");
  if (n_problems == 0) return FNR_OK;
  int rc = check_offsets("cloud_hausdorff", "a_offsets", a_offsets, n_a_sets, n_a_points);
  if (rc != FNR_OK) return rc;
  rc = check_offsets("cloud_hausdorff", "src_offsets", src_offsets, n_sources, n_src_points);
  if (rc != FNR_OK) return rc;
  if (trans_offsets) {
    rc = check_offsets("cloud_hausdorff", "trans_offsets", trans_offsets, n_problems, n_translations);
    if (rc != FNR_OK) return rc;
  } else {
    FNR_CHECK_ARG(n_translations == 0, "cloud_hausdorff: translations without trans_offsets");
  }
  FNR_CHECK_ARG(a_id && src_id, "cloud_hausdorff: null a_id or src_id");
  FNR_CHECK_ARG((a_xyz || n_a_points == 0) && (src_xyz || n_src_points == 0) && (translations || n_translations == 0),
                "cloud_hausdorff: null points");
  FNR_CHECK_ARG(distances && witnesses, "cloud_hausdorff: null output");
  std::vector<HdProb> probs((size_t)n_problems);
  long long part0 = 0, queries = 0;
  int max_chunks = 1;
  for (int64_t b = 0; b < n_problems; ++b) {
    FNR_CHECK_ARG(a_id[b] >= 0 && a_id[b] < n_a_sets, "cloud_hausdorff: a_id[%lld] = %d outside 0 .. %lld",
                  (long long)b, a_id[b], (long long)n_a_sets - 1);
    FNR_CHECK_ARG(src_id[b] >= 0 && src_id[b] < n_sources, "cloud_hausdorff: src_id[%lld] = %d outside 0 .. %lld",
                  (long long)b, src_id[b], (long long)n_sources - 1);
    HdProb& p = probs[(size_t)b];
    p.a0 = a_offsets[a_id[b]];
    p.na = (int)(a_offsets[a_id[b] + 1] - a_offsets[a_id[b]]);
    p.s0 = src_offsets[src_id[b]];
    p.ns = (int)(src_offsets[src_id[b] + 1] - src_offsets[src_id[b]]);
    const long long k = trans_offsets ? trans_offsets[b + 1] - trans_offsets[b] : 0;
    p.tr0 = trans_offsets ? trans_offsets[b] : 0;
    p.use_transform = k == 0 ? 1 : 0;
    FNR_CHECK_ARG(k > 0 || transforms, "cloud_hausdorff: problem %lld has neither translations nor a transform",
                  (long long)b);
    p.k = (int)(k == 0 ? 1 : k);
    const long long nb = (long long)p.k * p.ns;
    FNR_CHECK_ARG(nb <= FIT_MAX_POINTS, "cloud_hausdorff: problem %lld places too many points", (long long)b);
    const long long chunks = (p.na + HD_THREADS - 1) / HD_THREADS + (nb + HD_THREADS - 1) / HD_THREADS;
    FNR_CHECK_ARG(chunks <= HD_MAX_CHUNKS, "cloud_hausdorff: problem %lld is too large", (long long)b);
    p.part0 = part0;
    part0 += chunks;
    queries += p.na + nb;
    if (chunks > max_chunks) max_chunks = (int)chunks;
  }
  FNR_CHECK_ARG(workspace && workspace_bytes >= fnr_cloud_hausdorff_workspace_bytes(n_problems, queries),
                "cloud_hausdorff: workspace too small (need %zu)",
                fnr_cloud_hausdorff_workspace_bytes(n_problems, queries));
  hipStream_t st = as_stream(stream);
  FNR_PROF(OP_CLOUD, queries);
  const HdProb* d_probs = (const HdProb*)workspace;
  HdPart* d_parts = (HdPart*)((char*)workspace + align256((size_t)n_problems * sizeof(HdProb)));
  FNR_HIP(hipMemcpyWithStream(workspace, probs.data(), probs.size() * sizeof(HdProb), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_cloud_hausdorff, dim3((unsigned)n_problems, (unsigned)max_chunks), dim3(HD_THREADS), 0, st,
                     d_probs, a_xyz, src_xyz, translations, transforms, d_parts);
  FNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cloud_hausdorff_final, dim3((unsigned)((n_problems + 255) / 256)), dim3(256), 0, st, d_probs,
                     (int)n_problems, (const HdPart*)d_parts, distances, witnesses);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}
