// cloud_knn.hip — exact k-nearest-neighbour search on a point cloud (fp64) on gfx950, and the two Open3D calls of
// Nerfstudio's `pointcloud` export that are kNN queries:
//   fnr_cloud_knn                  rows of the k nearest points (the point itself included), ascending by
//                                  (squared distance, input index)
//   fnr_cloud_statistical_outlier  Open3D RemoveStatisticalOutliers(nb_neighbors, std_ratio)
//   fnr_cloud_estimate_normals     Open3D EstimateNormals(KDTreeSearchParamKNN(knn))
//
// Search structure: cloud.hip's sort-by-cell-key machinery (cloud_grid.hpp) with ONE change — the key interleaves the
// bits of the three cell coordinates (21 bits per axis, finest cell edge c0 = largest extent / 2^21).  In that order
// the points of a cell of edge c0 * 2^L are one contiguous run of the sorted array FOR EVERY LEVEL L (the cell is the
// key shifted right by 3 L), so a single sort gives a cell hierarchy and every query picks the cell edge that suits ITS
// neighbourhood: a dense surface sampled at lattice pitch searches cells of a few pitches, an isolated clutter point
// searches cells that are large where it sits — without walking through empty shells (which a small global edge would
// cost it) and without thousands of candidates per cell (which a large global edge would cost the surface).
//
// One wave answers one query (waves follow the sorted order, so neighbouring waves read the same runs):
//   1. start level: the smallest L at which the query's own cell holds >= ceil(k / 4) points — read off the sorted
//      keys around the query (the common prefix of a window of that many consecutive keys), no search;
//   2. lanes 0..26 find the runs of the 3 x 3 x 3 block of level-L cells around the query's cell (two binary searches
//      each); fewer than k points in the block -> L + 1, nothing tested;
//   3. the block's points are flattened over the lanes (64 candidates per round, each lane one fp64 distance in the CPU
//      libraries' operation order); the current k best live one per lane, sorted by (d2, index); a candidate below the
//      k-th is inserted with one shift of the lanes behind it;
//   4. exactness: every point outside the block lies beyond one of its faces.  The search ends when the k-th squared
//      distance is no larger than the square of the distance from the query to the nearest face that has cells
//      behind it (shrunk by 2^-20 cell edges, far above the rounding of the cell assignment), or when no face has;
//      otherwise L + 1 and the (eight times larger) block is searched from scratch.
// Every loop is bounded: L only grows and ends at 21, where one cell holds the grid.  No inter-workgroup communication.
// Cost per query ~ (levels tried) x (27 x 2 binary searches over lanes + block points / 64 rounds + ~k ln(block / k)
// insertions); the restarts are a geometric series dominated by the last level.
//
// Statistical outlier removal (Open3D's PointCloud::RemoveStatisticalOutliers, restated as recalled — Open3D is not a
// dependency; tests/cloud_knn_reference.py states the same rule in NumPy):
//   avg[i]  = mean of sqrt(d2) over the valid entries of row i (self included, summed in ascending order)
//   valid   = { i : avg[i] > 0 },  mean = sum(avg over valid) / n_valid,
//   std     = sqrt(sum((avg - mean)^2 over valid) / (n_valid - 1)),  threshold = mean + std_ratio * std
//   keep[i] = avg[i] > 0 && avg[i] < threshold
// The two global sums run in one workgroup in a fixed order (strided partial sums, then a fixed tree).
//
// Normals (Open3D's PointCloud::EstimateNormals, restated as recalled): the covariance of the knn nearest points (self included) about their
// mean; the unit eigenvector of its smallest eigenvalue (cyclic Jacobi rotations in fp64); fewer than 3 points ->
// (0, 0, 1).  The sign is whatever the rotations give — unoriented like Open3D's, and deterministic.
#include <cfloat>
#include <cmath>

#include "cloud_grid.hpp"
#include "sequencer.hpp"

namespace fnr {

constexpr int KNN_LEVELS = 21;                 // bits per axis; level 21 = one cell = the whole grid
constexpr int KNN_NO_INDEX = 0x7fffffff;       // list entry not filled yet

struct KnnGrid {
  double lo[3];
  double c0;   // edge of the finest cell
};

// 21 bits -> every third bit
__device__ inline u64 spread3(u64 v) {
  v &= 0x1fffffull;
  v = (v | (v << 32)) & 0x1f00000000ffffull;
  v = (v | (v << 16)) & 0x1f0000ff0000ffull;
  v = (v | (v << 8)) & 0x100f00f00f00f00full;
  v = (v | (v << 4)) & 0x10c30c30c30c30c3ull;
  v = (v | (v << 2)) & 0x1249249249249249ull;
  return v;
}
__device__ inline u64 morton3(u64 x, u64 y, u64 z) { return spread3(x) | (spread3(y) << 1) | (spread3(z) << 2); }

__device__ inline long long fine_coord(double p, double lo, double c0) {
  const double f = floor((p - lo) / c0);
  if (!(f > 0.0)) return 0;                       // below the grid, or NaN
  return f > 2097151.0 ? 2097151ll : (long long)f;
}

__global__ __launch_bounds__(256) void k_knn_keys(const double* __restrict__ xyz, int n, KnnGrid g,
                                                  u64* __restrict__ keys, int* __restrict__ idx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 cx = (u64)fine_coord(xyz[3 * (size_t)i + 0], g.lo[0], g.c0);
  const u64 cy = (u64)fine_coord(xyz[3 * (size_t)i + 1], g.lo[1], g.c0);
  const u64 cz = (u64)fine_coord(xyz[3 * (size_t)i + 2], g.lo[2], g.c0);
  keys[i] = morton3(cx, cy, cz);
  idx[i] = i;
}

// value of lane l (wave-uniform l) in every lane.  Through ds_bpermute: with v_readlane and a run-time lane
// (__builtin_amdgcn_readlane) this kernel returned wrong rows on gfx950 (candidates went missing from the lists); the
// cause was not established, the bpermute form is exact in the tests.
__device__ inline int lane_read(int v, int l) { return __shfl(v, l, 64); }
__device__ inline double lane_read(double v, int l) {
  return __hiloint2double(lane_read(__double2hiint(v), l), lane_read(__double2loint(v), l));
}
__device__ inline double wave_sum_f64(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
  return v;
}

// smallest level at which two keys share a cell
__device__ inline int common_level(u64 a, u64 b) {
  const u64 x = a ^ b;
  return x == 0 ? 0 : (63 - __clzll((long long)x)) / 3 + 1;
}

// (d2, index) order of the result rows
__device__ inline bool before(double da, int ia, double db, int ib) { return (da < db) | ((da == db) & (ia < ib)); }

template <int P, int Q>
__device__ inline void jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  constexpr int R = 3 - P - Q;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double arp = a[R][P], arq = a[R][Q];
  a[P][P] = a[P][P] - t * apq;
  a[Q][Q] = a[Q][Q] + t * apq;
  a[P][Q] = a[Q][P] = 0.0;
  a[R][P] = a[P][R] = c * arp - s * arq;
  a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double vp = v[i][P], vq = v[i][Q];
    v[i][P] = c * vp - s * vq;
    v[i][Q] = s * vp + c * vq;
  }
}

// unit eigenvector of the smallest eigenvalue of the symmetric matrix (xx xy xz / . yy yz / . . zz)
__device__ inline void smallest_eigenvector(double xx, double xy, double xz, double yy, double yz, double zz,
                                            double (&nrm)[3]) {
  const double big = fmax(fmax(fabs(xx), fabs(yy)), fabs(zz));
  const double sc = big > 0.0 ? 1.0 / big : 1.0;
  double a[3][3] = {{xx * sc, xy * sc, xz * sc}, {xy * sc, yy * sc, yz * sc}, {xz * sc, yz * sc, zz * sc}};
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < 16; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    const double diag = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
    if (!(off > 1e-40 * diag)) break;
    jacobi_rotate<0, 1>(a, v);
    jacobi_rotate<0, 2>(a, v);
    jacobi_rotate<1, 2>(a, v);
  }
  const bool m1 = a[1][1] < a[0][0] && a[1][1] <= a[2][2];
  const bool m2 = a[2][2] < a[0][0] && a[2][2] < a[1][1];
  double e[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) e[i] = m2 ? v[i][2] : (m1 ? v[i][1] : v[i][0]);
  const double len = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) nrm[i] = e[i] / len;
}

enum KnnMode { KNN_ROWS = 0, KNN_MEAN_DISTANCE = 1, KNN_NORMAL = 2 };

template <int MODE>
__global__ __launch_bounds__(256) void k_cloud_knn(const u64* __restrict__ keys, const CloudPoint* __restrict__ sxyz,
                                                   const double* __restrict__ xyz, int n, KnnGrid g, int k,
                                                   double* __restrict__ dist2, int* __restrict__ index,
                                                   double* __restrict__ out) {
  const int lane = wave_lane();
  const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (s >= n) return;                                           // the whole wave
  const CloudPoint p = sxyz[s];
  const double pc[3] = {p.x, p.y, p.z};
  long long fc[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) fc[a] = fine_coord(pc[a], g.lo[a], g.c0);

  // 1. start level: the finest one at which a window of m consecutive sorted keys around s shares a cell
  int L;
  {
    const int m = (k + 3) >> 2;                                 // 1 .. 8
    const int t = s - (m - 1) + lane;                           // lanes 0 .. 2m-2: the keys around s
    const bool have = lane < 2 * m - 1 && t >= 0 && t < n;
    const u64 ka = have ? keys[t] : 0ull;
    const u64 kb = __shfl(ka, (lane + m - 1) & 63, 64);
    const int have_b = __shfl((int)have, (lane + m - 1) & 63, 64);
    int lev = KNN_LEVELS;
    if (lane < m && have && have_b) lev = common_level(ka, kb);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const int o = __shfl_xor(lev, d, 64);
      lev = o < lev ? o : lev;
    }
    L = __builtin_amdgcn_readfirstlane(lev < KNN_LEVELS ? lev : KNN_LEVELS);   // the level loop runs on the scalar unit
  }

  double bd = __builtin_inf();                                  // lane i: the i-th best so far
  int bi = KNN_NO_INDEX;
  const int cell_of_lane = lane == 0 ? 13 : (lane == 13 ? 0 : lane);   // the query's own cell goes first
  for (; L <= KNN_LEVELS; ++L) {                                // bounded: at most 22 rounds
    const long long ncell = 1ll << (KNN_LEVELS - L);
    // 2. runs of the 27 cells
    int b = 0, e = 0;
    if (lane < 27) {
      const long long X = (fc[0] >> L) + (cell_of_lane % 3) - 1;
      const long long Y = (fc[1] >> L) + ((cell_of_lane / 3) % 3) - 1;
      const long long Z = (fc[2] >> L) + (cell_of_lane / 9) - 1;
      if (X >= 0 && X < ncell && Y >= 0 && Y < ncell && Z >= 0 && Z < ncell) {
        const u64 mk = morton3((u64)X, (u64)Y, (u64)Z);
        b = lower_bound_key(keys, 0, n, mk << (3 * L));
        e = lower_bound_key(keys, b, n, (mk + 1ull) << (3 * L));
      }
    }
    const int len = e - b;
    int incl = len;
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
      const int o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    const int off = incl - len;
    const int total = lane_read(incl, 31);                      // lanes 27 .. 31 hold empty runs
    if (total < k && L < KNN_LEVELS) continue;

    // 3. the block's points, 64 per round
    bd = __builtin_inf();
    bi = KNN_NO_INDEX;
    double kd = __builtin_inf();                                // the k-th best (wave-uniform)
    int ki = KNN_NO_INDEX;
    for (int base = 0; base < total; base += 64) {
      const int j = base + lane;
      const bool valid = j < total;
      int r = 0;                                                // the last run that starts at or before j
#pragma unroll
      for (int step = 16; step >= 1; step >>= 1) {
        const int tt = r + step;
        const int o = __shfl(off, tt & 31, 64);
        if (tt < 27 && o <= j) r = tt;
      }
      const int pos = __shfl(b, r, 64) + (j - __shfl(off, r, 64));
      const CloudPoint q = sxyz[valid ? pos : s];
      const double d = pair_d2(p, q);
      u64 mask = __ballot(valid && before(d, q.index, kd, ki));
      while (mask) {
        const int src = __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        const double cd = lane_read(d, src);
        const int ci = lane_read(q.index, src);
        if (!before(cd, ci, kd, ki)) continue;                  // the k-th has moved since the ballot
        const bool stay = before(bd, bi, cd, ci);
        const double ud = __shfl_up(bd, 1, 64);
        const int ui = __shfl_up(bi, 1, 64);
        const int prev_stay = __shfl_up((int)stay, 1, 64);
        if (!stay) {
          const bool first = lane == 0 || prev_stay != 0;
          bd = first ? cd : ud;
          bi = first ? ci : ui;
        }
        kd = lane_read(bd, k - 1);
        ki = lane_read(bi, k - 1);
      }
    }

    // 4. may anything outside the block be nearer than the k-th?
    const double w = ldexp(g.c0, L);
    bool covered = true;
    double dmin = __builtin_inf();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const long long c = fc[a] >> L;
      if (c >= 2) {
        covered = false;
        dmin = fmin(dmin, pc[a] - (g.lo[a] + (double)(c - 1) * w));
      }
      if (c + 2 < ncell) {
        covered = false;
        dmin = fmin(dmin, (g.lo[a] + (double)(c + 2) * w) - pc[a]);
      }
    }
    const double dm = dmin - w * (1.0 / 1048576.0);
    if (covered || (dm > 0.0 && kd <= dm * dm)) break;
  }

  const size_t q = (size_t)p.index;
  const bool filled = lane < k && bi != KNN_NO_INDEX;
  if (MODE == KNN_ROWS) {
    if (lane < k) {
      if (dist2) dist2[q * (size_t)k + lane] = bd;
      if (index) index[q * (size_t)k + lane] = filled ? bi : -1;
    }
  } else if (MODE == KNN_MEAN_DISTANCE) {
    const int cnt = __popcll(__ballot(filled));
    const double r = filled ? sqrt(bd) : 0.0;
    double sum = 0.0;
    for (int i = 0; i < cnt; ++i) sum = sum + lane_read(r, i);  // ascending, like the CPU loop
    if (lane == 0) out[q] = sum / (double)cnt;
  } else {
    const int cnt = __popcll(__ballot(filled));
    double nrm[3] = {0.0, 0.0, 1.0};
    if (cnt >= 3) {
      const size_t nb = filled ? (size_t)bi : q;
      const double x = xyz[3 * nb + 0], y = xyz[3 * nb + 1], z = xyz[3 * nb + 2];
      const double inv = 1.0 / (double)cnt;
      const double mx = wave_sum_f64(filled ? x : 0.0) * inv;
      const double my = wave_sum_f64(filled ? y : 0.0) * inv;
      const double mz = wave_sum_f64(filled ? z : 0.0) * inv;
      const double dx = filled ? x - mx : 0.0, dy = filled ? y - my : 0.0, dz = filled ? z - mz : 0.0;
      smallest_eigenvector(wave_sum_f64(dx * dx) * inv, wave_sum_f64(dx * dy) * inv, wave_sum_f64(dx * dz) * inv,
                           wave_sum_f64(dy * dy) * inv, wave_sum_f64(dy * dz) * inv, wave_sum_f64(dz * dz) * inv, nrm);
    }
    if (lane < 3) out[3 * q + lane] = lane == 0 ? nrm[0] : (lane == 1 ? nrm[1] : nrm[2]);
  }
}

// ---- statistical outlier: the global statistics in ONE workgroup, fixed order -------------------------------------
__device__ inline double block_sum_f64(double v, double* s_part) {
  v = wave_sum_f64(v);
  __syncthreads();                                              // s_part may still be read from the previous sum
  if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < 16; ++w) t = t + s_part[w];
  return t;
}

__global__ __launch_bounds__(1024) void k_knn_statistics(const double* __restrict__ avg, int n, double std_ratio,
                                                         double* __restrict__ stats) {
  __shared__ double s_part[16];
  double sum = 0.0, cnt = 0.0;
  for (int i = (int)threadIdx.x; i < n; i += 1024) {
    const double a = avg[i];
    if (a > 0.0) {
      sum = sum + a;
      cnt = cnt + 1.0;
    }
  }
  const double n_valid = block_sum_f64(cnt, s_part);
  const double mean = block_sum_f64(sum, s_part) / n_valid;
  double sq = 0.0;
  for (int i = (int)threadIdx.x; i < n; i += 1024) {
    const double a = avg[i];
    if (a > 0.0) sq = sq + (a - mean) * (a - mean);
  }
  const double sd = sqrt(block_sum_f64(sq, s_part) / (n_valid - 1.0));
  if (threadIdx.x == 0) {
    stats[0] = mean;
    stats[1] = sd;
    stats[2] = mean + std_ratio * sd;
  }
}

__global__ __launch_bounds__(256) void k_knn_keep(const double* __restrict__ avg, int n,
                                                  const double* __restrict__ stats, uint8_t* __restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double a = avg[i];
  keep[i] = (a > 0.0 && a < stats[2]) ? 1 : 0;
}

// ---- host side -----------------------------------------------------------------------------------------------------
static int knn_check(const char* what, const double* xyz, int64_t n, const double* lo, const double* hi, int k,
                     void* workspace, size_t workspace_bytes, CloudWs* w, KnnGrid* g) {
  FNR_CHECK_ARG(n >= 0 && n < 2147483647LL, "%s: n out of range", what);
  FNR_CHECK_ARG(k >= 1 && k <= FNR_CLOUD_KNN_MAX, "%s: k = %d outside 1 .. %d", what, k, FNR_CLOUD_KNN_MAX);
  if (n == 0) return FNR_OK;
  FNR_CHECK_ARG(xyz, "%s: null xyz", what);
  FNR_CHECK_ARG(lo && hi, "%s: null bounds", what);
  FNR_CHECK_ARG(carve_cloud(workspace, workspace_bytes, n, w), "%s: workspace too small (need %zu)", what,
                fnr_cloud_knn_workspace_bytes(n, k));
  double ext = 0.0;
  for (int a = 0; a < 3; ++a) {
    FNR_CHECK_ARG(hi[a] >= lo[a] && (hi[a] - lo[a]) < 1e300, "%s: bounds must be finite with hi >= lo", what);
    ext = fmax(ext, hi[a] - lo[a]);
    g->lo[a] = lo[a];
  }
  // the largest extent spans cells 0 .. 2^21 - 2; a cloud of one position gets a unit cell
  g->c0 = ext > 0.0 ? fmax(ext / 2097150.0, DBL_MIN) : 1.0;
  return FNR_OK;
}

template <int MODE>
static int knn_run(const double* xyz, int n, const KnnGrid& g, int k, const CloudWs& w, double* dist2, int* index,
                   double* out, hipStream_t st) {
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_knn_keys, dim3(blocks), dim3(256), 0, st, xyz, n, g, w.keys_a, w.idx_a);
  FNR_LAUNCH_CHECK();
  int rc = sort_by_key(w, n, 3 * KNN_LEVELS, st);
  if (rc != FNR_OK) return rc;
  rc = gather_sorted(xyz, w, n, st);
  if (rc != FNR_OK) return rc;
  hipLaunchKernelGGL((k_cloud_knn<MODE>), dim3((unsigned)(((long long)n + 3) / 4)), dim3(256), 0, st, w.keys, w.sxyz,
                     xyz, n, g, k, dist2, index, out);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

}  // namespace fnr

using namespace fnr;

extern "C" size_t fnr_cloud_knn_workspace_bytes(int64_t n_points, int32_t k) {
  (void)k;   // the k best of a query live in its wave's registers
  return fnr_cloud_workspace_bytes(n_points);
}

extern "C" int fnr_cloud_knn(const double* xyz, int64_t n, const double* lo, const double* hi, int32_t k,
                             double* dist2, int32_t* index, void* workspace, size_t workspace_bytes, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_cloud_knn");
  CloudWs w;
  KnnGrid g;
  int rc = knn_check("cloud_knn", xyz, n, lo, hi, k, workspace, workspace_bytes, &w, &g);
  if (rc != FNR_OK || n == 0) return rc;
  FNR_PROF(OP_CLOUD, n);
  return knn_run<KNN_ROWS>(xyz, (int)n, g, k, w, dist2, index, nullptr, as_stream(stream));
}

extern "C" int fnr_cloud_statistical_outlier(const double* xyz, int64_t n, const double* lo, const double* hi,
                                             int32_t nb_neighbors, double std_ratio, double* avg_distance,
                                             uint8_t* keep, double* stats, void* workspace, size_t workspace_bytes,
                                             void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_cloud_statistical_outlier");
  // Open3D: "Illegal input parameters, the number of neighbors and standard deviation ratio must be positive"
  FNR_CHECK_ARG(nb_neighbors >= 1 && std_ratio > 0.0,
                "cloud_statistical_outlier: nb_neighbors and std_ratio must be positive");
  CloudWs w;
  KnnGrid g;
  int rc = knn_check("cloud_statistical_outlier", xyz, n, lo, hi, nb_neighbors, workspace, workspace_bytes, &w, &g);
  if (rc != FNR_OK || n == 0) return rc;
  FNR_CHECK_ARG(avg_distance && keep && stats, "cloud_statistical_outlier: null output");
  hipStream_t st = as_stream(stream);
  FNR_PROF(OP_CLOUD, n);
  rc = knn_run<KNN_MEAN_DISTANCE>(xyz, (int)n, g, nb_neighbors, w, nullptr, nullptr, avg_distance, st);
  if (rc != FNR_OK) return rc;
  hipLaunchKernelGGL(k_knn_statistics, dim3(1), dim3(1024), 0, st, avg_distance, (int)n, std_ratio, stats);
  FNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_knn_keep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, avg_distance, (int)n, stats, keep);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

extern "C" int fnr_cloud_estimate_normals(const double* xyz, int64_t n, const double* lo, const double* hi,
                                          int32_t knn, double* normals, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_cloud_estimate_normals");
  CloudWs w;
  KnnGrid g;
  int rc = knn_check("cloud_estimate_normals", xyz, n, lo, hi, knn, workspace, workspace_bytes, &w, &g);
  if (rc != FNR_OK || n == 0) return rc;
  FNR_CHECK_ARG(normals, "cloud_estimate_normals: null output");
  FNR_PROF(OP_CLOUD, n);
  return knn_run<KNN_NORMAL>(xyz, (int)n, g, knn, w, nullptr, nullptr, normals, as_stream(stream));
}
