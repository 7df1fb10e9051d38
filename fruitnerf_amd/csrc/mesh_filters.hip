// mesh_filters.hip — triangle-mesh filters for the mesh exports (the contract is stated in include/fruitnerf_hip.h,
// "triangle-mesh filters"): per-vertex rows (neighbours / incident faces) through a stable radix sort of 64-bit keys,
// Laplacian / Taubin smoothing and area-weighted vertex normals as sequential float64 sums over those rows, vertex
// clustering on a voxel grid with degenerate and duplicate faces dropped, and the float64 mean of a row.  Everything is
// gather bound; LDS holds only block scans and a block's digits.
//
// Shared-machine rules of this file (those of mesh.hip): no floating-point atomics; no workgroup waits for another — a
// launch boundary is the visibility guarantee; every loop is bounded by an array size; an index outside its array and an
// exceeded bound set a bit in the workspace's error word, which the entry point reads back.  Every index that comes out
// of memory is checked before it is used to address memory.
#include <cmath>

#include "common.hpp"
#include "mesh_common.hpp"
#include "sequencer.hpp"

namespace fnr {

constexpr unsigned long long ROWS_MAGIC = 0x666e72726f777331ull, CLUSTER_MAGIC = 0x666e72636c757331ull;
constexpr double CLUSTER_MAX_CELLS = 2097152.0;     // 2^21 per axis: three axes fit one 63-bit key
enum : unsigned { MF_ERR_INDEX = 1u, MF_ERR_ROWS = 2u, MF_ERR_CELL = 4u, MF_ERR_SORT = 8u };

static inline size_t align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
static inline long long blocks_of(long long n) { return (n + MESH_BLOCK - 1) / MESH_BLOCK; }
// the bytes a value of [0, n) needs
static inline int bytes_for(long long n) {
  int b = 0;
  while (b < 4 && n > 0 && ((n - 1) >> (8 * b)) != 0) ++b;
  return b;
}

// ---- stable radix sort of the elements 0 .. n - 1 by keys[element] -------------------------------------------------------
// The order is a permutation in memory (nullptr: the identity); one pass = count -> scan -> emit over one 8-bit digit, 256
// positions a block.  A position's place among the block's positions of its digit is counted in LDS, in input order, so
// every pass is stable.
__device__ __forceinline__ long long sorted_element(const int* __restrict__ order, long long p, long long n,
                                                    unsigned long long* header) {
  const long long e = order ? (long long)order[p] : p;
  if (e >= 0 && e < n) return e;
  mesh_error(header, MF_ERR_SORT);                        // never: every pass writes a permutation
  return 0;
}

__device__ __forceinline__ int sort_digit(unsigned long long* header, const int* __restrict__ src,
                                          const unsigned long long* __restrict__ keys, long long n, int shift, int* s_digit,
                                          long long& p) {
  p = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  int d = 256;
  if (p < n) d = (int)((keys[sorted_element(src, p, n, header)] >> shift) & 255ull);
  s_digit[threadIdx.x] = d;
  __syncthreads();
  return d;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_filter_sort_count(unsigned long long* header, unsigned* __restrict__ hist,
                                                                  long long nb, long long n, const int* __restrict__ src,
                                                                  const unsigned long long* __restrict__ keys, int shift) {
  __shared__ int s_digit[MESH_BLOCK];
  long long p;
  sort_digit(header, src, keys, n, shift, s_digit, p);
  unsigned c = 0u;
  for (int j = 0; j < MESH_BLOCK; ++j) c += (s_digit[j] == (int)threadIdx.x) ? 1u : 0u;
  hist[(size_t)threadIdx.x * nb + blockIdx.x] = c;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_filter_sort_emit(unsigned long long* header, const unsigned* __restrict__ hist,
                                                                 long long nb, long long n, const int* __restrict__ src,
                                                                 int* __restrict__ dst,
                                                                 const unsigned long long* __restrict__ keys, int shift) {
  __shared__ int s_digit[MESH_BLOCK];
  long long p;
  const int d = sort_digit(header, src, keys, n, shift, s_digit, p);
  unsigned before = 0u;
  for (int j = 0; j < (int)threadIdx.x; ++j) before += (s_digit[j] == d) ? 1u : 0u;
  if (p >= n) return;
  const long long at = (long long)hist[(size_t)d * nb + blockIdx.x] + before;
  if (at < n) dst[at] = (int)sorted_element(src, p, n, header);
  else mesh_error(header, MF_ERR_SORT);
}

struct SortBuffers {
  unsigned long long* header;
  unsigned* hist;              // [256 * blocks_of(n)]
  int* order[2];               // [n] each
};

// n_bytes passes from byte first_byte of the keys upwards; `src` (nullptr: the identity) is the order so far and the
// order afterwards, `turn` the buffer the next pass writes.
static int sort_bytes(hipStream_t st, const SortBuffers& b, long long n, const unsigned long long* keys, int first_byte,
                      int n_bytes, const int*& src, int& turn) {
  const long long nb = blocks_of(n);
  for (int byte = first_byte; byte < first_byte + n_bytes; ++byte) {
    hipLaunchKernelGGL(k_filter_sort_count, dim3((unsigned)nb), dim3(MESH_BLOCK), 0, st, b.header, b.hist, nb, n, src, keys,
                       8 * byte);
    FNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_scan<false>, dim3(1), dim3(SCAN_THREADS), 0, st, b.hist, b.hist, 256 * nb,
                       (unsigned long long*)nullptr, (unsigned long long*)nullptr);
    FNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_filter_sort_emit, dim3((unsigned)nb), dim3(MESH_BLOCK), 0, st, b.header, b.hist, nb, n, src,
                       b.order[turn], keys, 8 * byte);
    FNR_LAUNCH_CHECK();
    src = b.order[turn];
    turn ^= 1;
  }
  return FNR_OK;
}

// ---- vertex rows ----------------------------------------------------------------------------------------------------------
struct RowsWs {
  unsigned long long* header;   // [0] error word, [1] n_entries, [2] n_keys, [3] ROWS_MAGIC + kind
  unsigned long long* keys;     // [N] (row << 32) | entry
  SortBuffers sort;
  unsigned* mark;               // [N] 1: the sorted position holds the first copy of a key that is an entry
  unsigned* pos;                // [N] exclusive scan of mark
  long long N;
  size_t bytes;
};

static inline long long rows_keys(long long F, int kind) { return (kind == FNR_MESH_ROWS_NEIGHBOURS ? 6 : 3) * F; }

static RowsWs rows_layout(void* base, long long F, int kind) {
  RowsWs w;
  w.N = rows_keys(F, kind);
  size_t at = 0;
  char* p = reinterpret_cast<char*>(base);
  auto take = [&](size_t bytes) {
    char* r = p + at;
    at += align16(bytes);
    return r;
  };
  w.header = reinterpret_cast<unsigned long long*>(take(64));
  w.keys = reinterpret_cast<unsigned long long*>(take(8 * (size_t)w.N));
  w.sort.header = w.header;
  w.sort.order[0] = reinterpret_cast<int*>(take(4 * (size_t)w.N));
  w.sort.order[1] = reinterpret_cast<int*>(take(4 * (size_t)w.N));
  w.sort.hist = reinterpret_cast<unsigned*>(take(4 * 256 * (size_t)blocks_of(w.N)));
  w.mark = reinterpret_cast<unsigned*>(take(4 * (size_t)w.N));
  w.pos = reinterpret_cast<unsigned*>(take(4 * (size_t)w.N));
  w.bytes = at;
  return w;
}

// the sorted order the count call left: the passes are a function of the sizes alone
static const int* rows_final_order(const RowsWs& w, long long V, long long F, int kind) {
  const int passes = bytes_for(kind == FNR_MESH_ROWS_NEIGHBOURS ? V : F) + bytes_for(V);
  return passes == 0 ? nullptr : w.sort.order[(passes - 1) & 1];
}

// One thread per key.  NEIGHBOURS: the six ordered pairs (a, b) of a face's slots, a == b included (such a key is sorted
// like the others and never marked).  FACES: (vertex, face) per slot.
__global__ __launch_bounds__(MESH_BLOCK) void k_rows_keys(RowsWs w, long long V, long long F, int kind,
                                                          const int* __restrict__ faces) {
  const long long t = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (t >= w.N) return;
  unsigned long long key = 0ull;
  if (kind == FNR_MESH_ROWS_NEIGHBOURS) {
    const long long f = t / 6;
    const int j = (int)(t - 6 * f), s = j >> 1, o = (s + 1 + (j & 1)) % 3;
    const int a = faces[3 * f + s], b = faces[3 * f + o];
    if (a < 0 || b < 0 || (long long)a >= V || (long long)b >= V) mesh_error(w.header, MF_ERR_INDEX);
    else key = ((unsigned long long)(unsigned)a << 32) | (unsigned)b;
  } else {
    const long long f = t / 3;
    const int a = faces[t];
    if (a < 0 || (long long)a >= V) mesh_error(w.header, MF_ERR_INDEX);
    else key = ((unsigned long long)(unsigned)a << 32) | (unsigned long long)f;
  }
  w.keys[t] = key;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_rows_mark(RowsWs w, int kind, const int* __restrict__ order) {
  const long long p = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (p >= w.N) return;
  const unsigned long long k = w.keys[sorted_element(order, p, w.N, w.header)];
  bool first = true;
  if (p > 0) first = w.keys[sorted_element(order, p - 1, w.N, w.header)] != k;
  const bool entry = kind != FNR_MESH_ROWS_NEIGHBOURS || (k >> 32) != (k & 0xffffffffull);
  w.mark[p] = (first && entry) ? 1u : 0u;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_rows_entries(RowsWs w, long long E, const int* __restrict__ order,
                                                             int* __restrict__ entries) {
  const long long p = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (p >= w.N || !w.mark[p]) return;
  const long long at = (long long)w.pos[p];
  if (at < E) entries[at] = (int)(w.keys[sorted_element(order, p, w.N, w.header)] & 0xffffffffull);
  else mesh_error(w.header, MF_ERR_SORT);
}

// offsets[r] = the entries before the first sorted key of a row >= r: a binary search of at most 33 steps per row
__global__ __launch_bounds__(MESH_BLOCK) void k_rows_offsets(RowsWs w, long long V, long long E, const int* __restrict__ order,
                                                             int* __restrict__ offsets) {
  const long long r = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (r > V) return;
  long long lo = 0, hi = w.N;
  for (int step = 0; step < 40 && lo < hi; ++step) {
    const long long mid = lo + (hi - lo) / 2;
    const long long row = (long long)(w.keys[sorted_element(order, mid, w.N, w.header)] >> 32);
    if (row < r) lo = mid + 1;
    else hi = mid;
  }
  long long at = E;
  if (lo < w.N) at = (long long)w.pos[lo];
  if (at > E) {
    mesh_error(w.header, MF_ERR_SORT);
    at = E;
  }
  offsets[r] = (int)at;
}

// ---- smoothing ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MESH_BLOCK) void k_smooth_load(long long n, const float* __restrict__ in, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (i < n) out[i] = (double)in[i];
}

__global__ __launch_bounds__(MESH_BLOCK) void k_smooth_store(long long n, const double* __restrict__ in, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (i < n) out[i] = (float)in[i];
}

// the row of r: false (and the error word) unless 0 <= begin <= end <= E
__device__ __forceinline__ bool row_range(const int* __restrict__ offsets, long long r, long long E, unsigned long long* header,
                                          long long& begin, long long& end) {
  begin = offsets[r];
  end = offsets[r + 1];
  if (begin >= 0 && begin <= end && end <= E) return true;
  mesh_error(header, MF_ERR_ROWS);
  return false;
}

// One thread per vertex: the neighbours are added in row order, every product and every sum rounded (the build has
// -ffp-contract=off), so the new position has one defined bit pattern.
__global__ __launch_bounds__(MESH_BLOCK) void k_smooth_step(unsigned long long* header, long long V, long long E,
                                                            const int* __restrict__ offsets, const int* __restrict__ neighbours,
                                                            const double* __restrict__ in, double* __restrict__ out,
                                                            double factor, int weights) {
  const long long v = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (v >= V) return;
  const double px = in[3 * v], py = in[3 * v + 1], pz = in[3 * v + 2];
  double ox = px, oy = py, oz = pz;
  long long begin, end;
  if (row_range(offsets, v, E, header, begin, end) && end > begin) {
    double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
    bool ok = true;
    for (long long i = begin; i < end; ++i) {
      const int n = neighbours[i];
      if (n < 0 || (long long)n >= V) {
        mesh_error(header, MF_ERR_ROWS);
        ok = false;
        break;
      }
      const double qx = in[3 * (long long)n], qy = in[3 * (long long)n + 1], qz = in[3 * (long long)n + 2];
      double wn = 1.0;
      if (weights == FNR_MESH_WEIGHTS_INVERSE_DISTANCE) {
        const double dx = px - qx, dy = py - qy, dz = pz - qz;
        wn = 1.0 / (sqrt((dx * dx + dy * dy) + dz * dz) + 1e-12);
      }
      sx = sx + wn * qx;
      sy = sy + wn * qy;
      sz = sz + wn * qz;
      sw = sw + wn;
    }
    if (ok) {
      ox = px + factor * (sx / sw - px);
      oy = py + factor * (sy / sw - py);
      oz = pz + factor * (sz / sw - pz);
    }
  }
  out[3 * v] = ox;
  out[3 * v + 1] = oy;
  out[3 * v + 2] = oz;
}

// ---- vertex normals -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MESH_BLOCK) void k_vertex_normals(unsigned long long* header, long long V, long long F, long long E,
                                                               const float* __restrict__ vertices, const int* __restrict__ faces,
                                                               const int* __restrict__ offsets, const int* __restrict__ face_rows,
                                                               float* __restrict__ normals) {
  const long long v = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (v >= V) return;
  double nx = 0.0, ny = 0.0, nz = 0.0;
  long long begin, end;
  bool ok = row_range(offsets, v, E, header, begin, end);
  for (long long i = begin; ok && i < end; ++i) {
    const int f = face_rows[i];
    if (f < 0 || (long long)f >= F) {
      mesh_error(header, MF_ERR_ROWS);
      ok = false;
      break;
    }
    double p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int idx = faces[3 * (long long)f + k];
      if (idx < 0 || (long long)idx >= V) {
        mesh_error(header, MF_ERR_INDEX);
        ok = false;
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) p[k][a] = ok ? (double)vertices[3 * (long long)idx + a] : 0.0;
    }
    if (!ok) break;
    double e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      e1[a] = p[1][a] - p[0][a];
      e2[a] = p[2][a] - p[0][a];
    }
    nx = nx + (e1[1] * e2[2] - e1[2] * e2[1]);
    ny = ny + (e1[2] * e2[0] - e1[0] * e2[2]);
    nz = nz + (e1[0] * e2[1] - e1[1] * e2[0]);
  }
  const double sq = (nx * nx + ny * ny) + nz * nz;
  float out[3] = {0.0f, 0.0f, 0.0f};
  if (ok && sq > 0.0) {
    const double length = sqrt(sq);
    out[0] = (float)(nx / length);
    out[1] = (float)(ny / length);
    out[2] = (float)(nz / length);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) normals[3 * v + a] = out[a];
}

// ---- row mean -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MESH_BLOCK) void k_rows_mean(unsigned long long* header, long long R, long long E, long long N,
                                                          const int* __restrict__ offsets, const int* __restrict__ members,
                                                          const float* __restrict__ values, float* __restrict__ out) {
  const long long r = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (r >= R) return;
  double s[3] = {0.0, 0.0, 0.0};
  long long begin, end;
  bool ok = row_range(offsets, r, E, header, begin, end);
  for (long long i = begin; ok && i < end; ++i) {
    const int m = members[i];
    if (m < 0 || (long long)m >= N) {
      mesh_error(header, MF_ERR_ROWS);
      ok = false;
      break;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) s[a] = s[a] + (double)values[3 * (long long)m + a];
  }
  const double count = (double)(end - begin);
#pragma unroll
  for (int a = 0; a < 3; ++a) out[3 * r + a] = (ok && end > begin) ? (float)(s[a] / count) : 0.0f;
}

// ---- vertex clustering ----------------------------------------------------------------------------------------------------
struct ClusterWs {
  unsigned long long* header;   // [0] error word, [1] n_clusters, [2] n_new_faces, [3] CLUSTER_MAGIC, [4] V, [5] F
  unsigned long long* cell;     // [V] (cx << 42) | (cy << 21) | cz
  SortBuffers vsort;            // vertices by cell: a cell's vertices ascend
  unsigned* head;               // [V] 1: the sorted position starts a cell
  unsigned* run;                // [V] exclusive scan of head
  unsigned* run_start;          // [V] the sorted position where run r starts
  int* rep;                     // [V] the smallest vertex of the vertex's cell
  unsigned* rank;               // [V] "is its own rep", then its exclusive scan
  int* cluster;                 // [V]
  unsigned long long* kab;      // [F] the re-indexed face rotated to its smallest index: (a << 32) | b ...
  unsigned long long* kc;       // [F] ... and c
  unsigned char* degenerate;    // [F]
  SortBuffers fsort;            // faces by (a, b, c): equal triples ascend by face
  unsigned* fmap;               // [F] kept flag, then new row + 1
  long long V, F;
  size_t bytes;
};

static ClusterWs cluster_layout(void* base, long long V, long long F) {
  ClusterWs w;
  w.V = V;
  w.F = F;
  size_t at = 0;
  char* p = reinterpret_cast<char*>(base);
  auto take = [&](size_t bytes) {
    char* r = p + at;
    at += align16(bytes);
    return r;
  };
  w.header = reinterpret_cast<unsigned long long*>(take(64));
  w.cell = reinterpret_cast<unsigned long long*>(take(8 * (size_t)V));
  w.vsort.header = w.header;
  w.vsort.order[0] = reinterpret_cast<int*>(take(4 * (size_t)V));
  w.vsort.order[1] = reinterpret_cast<int*>(take(4 * (size_t)V));
  w.vsort.hist = reinterpret_cast<unsigned*>(take(4 * 256 * (size_t)blocks_of(V)));
  w.head = reinterpret_cast<unsigned*>(take(4 * (size_t)V));
  w.run = reinterpret_cast<unsigned*>(take(4 * (size_t)V));
  w.run_start = reinterpret_cast<unsigned*>(take(4 * (size_t)V));
  w.rep = reinterpret_cast<int*>(take(4 * (size_t)V));
  w.rank = reinterpret_cast<unsigned*>(take(4 * (size_t)V));
  w.cluster = reinterpret_cast<int*>(take(4 * (size_t)V));
  w.kab = reinterpret_cast<unsigned long long*>(take(8 * (size_t)F));
  w.kc = reinterpret_cast<unsigned long long*>(take(8 * (size_t)F));
  w.degenerate = reinterpret_cast<unsigned char*>(take((size_t)F));
  w.fsort.header = w.header;
  w.fsort.order[0] = reinterpret_cast<int*>(take(4 * (size_t)F));
  w.fsort.order[1] = reinterpret_cast<int*>(take(4 * (size_t)F));
  w.fsort.hist = reinterpret_cast<unsigned*>(take(4 * 256 * (size_t)blocks_of(F)));
  w.fmap = reinterpret_cast<unsigned*>(take(4 * (size_t)F));
  w.bytes = at;
  return w;
}

constexpr int CLUSTER_CELL_BYTES = 8;
static const int* cluster_vertex_order(const ClusterWs& w) { return w.vsort.order[(CLUSTER_CELL_BYTES - 1) & 1]; }

struct Double3 {
  double x, y, z;
};

__global__ __launch_bounds__(MESH_BLOCK) void k_cluster_cells(ClusterWs w, const float* __restrict__ vertices, Double3 origin,
                                                              double voxel_size) {
  const long long v = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (v >= w.V) return;
  const double o[3] = {origin.x, origin.y, origin.z};
  unsigned long long key = 0ull;
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double c = floor(((double)vertices[3 * v + a] - o[a]) / voxel_size);
    if (!(c >= 0.0) || !(c < CLUSTER_MAX_CELLS)) ok = false;           // a NaN fails both
    else key = (key << 21) | (unsigned long long)c;
  }
  if (!ok) {
    mesh_error(w.header, MF_ERR_CELL);
    key = 0ull;
  }
  w.cell[v] = key;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_cluster_heads(ClusterWs w, const int* __restrict__ order) {
  const long long p = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (p >= w.V) return;
  bool head = true;
  if (p > 0) head = w.cell[sorted_element(order, p, w.V, w.header)] != w.cell[sorted_element(order, p - 1, w.V, w.header)];
  w.head[p] = head ? 1u : 0u;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_cluster_runs(ClusterWs w) {
  const long long p = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (p >= w.V || !w.head[p]) return;
  const long long r = (long long)w.run[p];
  if (r < w.V) w.run_start[r] = (unsigned)p;
  else mesh_error(w.header, MF_ERR_SORT);
}

// the run of sorted position p and where it starts; false: the workspace is not what the launches before wrote
__device__ __forceinline__ bool cluster_run(const ClusterWs& w, long long p, long long& r, long long& start) {
  r = (long long)w.run[p] + (long long)w.head[p] - 1;
  if (r >= 0 && r < w.V) {
    start = (long long)w.run_start[r];
    if (start <= p) return true;
  }
  mesh_error(w.header, MF_ERR_SORT);
  return false;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_cluster_reps(ClusterWs w, const int* __restrict__ order) {
  const long long p = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (p >= w.V) return;
  const long long v = sorted_element(order, p, w.V, w.header);
  long long r, start;
  if (!cluster_run(w, p, r, start)) start = p;
  w.rep[v] = (int)sorted_element(order, start, w.V, w.header);     // the run ascends: its first vertex is its smallest
  w.rank[v] = (start == p) ? 1u : 0u;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_cluster_labels(ClusterWs w, int* __restrict__ vertex_cluster) {
  const long long v = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (v >= w.V) return;
  int rep = w.rep[v];
  if (rep < 0 || (long long)rep >= w.V) {
    mesh_error(w.header, MF_ERR_SORT);
    rep = 0;
  }
  const int c = (int)w.rank[rep];
  w.cluster[v] = c;
  vertex_cluster[v] = c;
  if (v == 0) {
    w.header[3] = CLUSTER_MAGIC;
    w.header[4] = (unsigned long long)w.V;
    w.header[5] = (unsigned long long)w.F;
  }
}

// the cluster of face f's slot s; -1 (and the error word) for an index outside [0, V)
__device__ __forceinline__ int cluster_of(const ClusterWs& w, const int* __restrict__ faces, long long f, int s) {
  const int i = faces[3 * f + s];
  if (i < 0 || (long long)i >= w.V) {
    mesh_error(w.header, MF_ERR_INDEX);
    return -1;
  }
  return w.cluster[i];
}

__global__ __launch_bounds__(MESH_BLOCK) void k_cluster_face_keys(ClusterWs w, const int* __restrict__ faces) {
  const long long f = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (f >= w.F) return;
  const int a = cluster_of(w, faces, f, 0), b = cluster_of(w, faces, f, 1), c = cluster_of(w, faces, f, 2);
  const bool degenerate = a < 0 || b < 0 || c < 0 || a == b || b == c || a == c;
  unsigned long long kab = 0ull, kc = 0ull;
  if (!degenerate) {
    int x = a, y = b, z = c;                              // rotated to start at the smallest
    if (b < a && b < c) {
      x = b;
      y = c;
      z = a;
    } else if (c < a && c < b) {
      x = c;
      y = a;
      z = b;
    }
    kab = ((unsigned long long)(unsigned)x << 32) | (unsigned)y;
    kc = (unsigned long long)(unsigned)z;
  }
  w.kab[f] = kab;
  w.kc[f] = kc;
  w.degenerate[f] = degenerate ? 1 : 0;
}

// One thread per sorted position: a face is kept iff it has three different clusters and no earlier face has its triple
// (equal triples are neighbours in the sorted order and ascend by face: the first of a run is the earliest).
__global__ __launch_bounds__(MESH_BLOCK) void k_cluster_face_mark(ClusterWs w, const int* __restrict__ order) {
  const long long p = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (p >= w.F) return;
  const long long f = sorted_element(order, p, w.F, w.header);
  bool keep = !w.degenerate[f];
  if (keep && p > 0) {
    const long long g = sorted_element(order, p - 1, w.F, w.header);
    keep = w.degenerate[g] || w.kab[g] != w.kab[f] || w.kc[g] != w.kc[f];
  }
  w.fmap[f] = keep ? 1u : 0u;
}

// csize[c] = the members of cluster c; every cluster is one run of the sorted vertices
__global__ __launch_bounds__(MESH_BLOCK) void k_cluster_sizes(ClusterWs w, long long n_clusters, const int* __restrict__ order,
                                                              unsigned* __restrict__ csize) {
  const long long p = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (p >= w.V || !w.head[p]) return;
  const long long r = (long long)w.run[p];
  long long end = w.V;
  if (r + 1 < n_clusters) end = (long long)w.run_start[r + 1];
  const int c = w.cluster[sorted_element(order, p, w.V, w.header)];
  if (c < 0 || (long long)c >= n_clusters || end <= p || end > w.V) mesh_error(w.header, MF_ERR_SORT);
  else csize[c] = (unsigned)(end - p);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_cluster_members(ClusterWs w, long long n_clusters, const int* __restrict__ order,
                                                                int* __restrict__ offsets, int* __restrict__ members) {
  const long long p = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (p >= w.V) return;
  if (p == 0) offsets[n_clusters] = (int)w.V;
  const long long v = sorted_element(order, p, w.V, w.header);
  const int c = w.cluster[v];
  long long r, start;
  if (c < 0 || (long long)c >= n_clusters || !cluster_run(w, p, r, start)) {
    mesh_error(w.header, MF_ERR_SORT);
    return;
  }
  const long long at = (long long)offsets[c] + (p - start);
  if (at >= 0 && at < w.V) members[at] = (int)v;
  else mesh_error(w.header, MF_ERR_SORT);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_cluster_faces(ClusterWs w, long long n_clusters, long long n_new_faces,
                                                              const int* __restrict__ faces, int* __restrict__ new_faces,
                                                              int* __restrict__ face_ids) {
  const long long f = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (f >= w.F) return;
  const unsigned m = w.fmap[f];
  if (!m) return;
  if ((long long)m > n_new_faces) {
    mesh_error(w.header, MF_ERR_SORT);
    return;
  }
  face_ids[m - 1u] = (int)f;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int c = cluster_of(w, faces, f, s);
    if (c < 0 || (long long)c >= n_clusters) mesh_error(w.header, MF_ERR_INDEX);
    new_faces[3 * (size_t)(m - 1u) + s] = c;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
static const char* filter_error_text(unsigned bits) {
  if (bits & MF_ERR_INDEX) return "a face index lies outside [0, n_vertices)";
  if (bits & MF_ERR_CELL) return "a vertex is not finite or lies outside the 2^21 cells of an axis";
  if (bits & MF_ERR_ROWS) return "the rows are inconsistent (offsets not ascending within [0, n_entries], or an entry outside its array)";
  return "the workspace does not hold what the count call wrote";
}

// the header back on the host: a synchronisation of the stream
static int filter_header(const char* who, const unsigned long long* header, unsigned long long (&host)[8], hipStream_t st) {
  FNR_HIP(hipMemcpyAsync(host, header, sizeof(host), hipMemcpyDeviceToHost, st));
  FNR_HIP(hipStreamSynchronize(st));
  const unsigned bits = (unsigned)(host[0] & 0xffffffffull);
  if (bits) {
    set_error("%s: %s (error word 0x%x)", who, filter_error_text(bits), bits);
    return FNR_ERR_INVALID;
  }
  return FNR_OK;
}

static int rows_kind_check(const char* who, int64_t n_faces, int kind) {
  FNR_CHECK_ARG(kind == FNR_MESH_ROWS_NEIGHBOURS || kind == FNR_MESH_ROWS_FACES, "%s: kind %d is neither NEIGHBOURS nor FACES",
                who, kind);
  FNR_CHECK_ARG(6 * (long long)n_faces <= 0x7fffffffll, "%s: 6 * n_faces exceeds 2^31 - 1", who);
  return FNR_OK;
}

static int rows_arguments_check(const char* who, int64_t n_rows, int64_t n_entries, const int32_t* offsets, const int32_t* entries) {
  FNR_CHECK_ARG(n_entries >= 0 && n_entries <= 0x7fffffffll, "%s: n_entries outside 0..2^31 - 1", who);
  FNR_CHECK_ARG(n_rows == 0 || offsets, "%s: null offsets", who);
  FNR_CHECK_ARG(n_entries == 0 || entries, "%s: null entries", who);
  return FNR_OK;
}

}  // namespace fnr

using namespace fnr;

extern "C" size_t fnr_mesh_vertex_rows_workspace_bytes(int64_t n_vertices, int64_t n_faces, int32_t kind) {
  if (n_vertices < 0 || n_faces < 0 || n_vertices > 0x7fffffffll || 6 * (long long)n_faces > 0x7fffffffll) return 0;
  if (kind != FNR_MESH_ROWS_NEIGHBOURS && kind != FNR_MESH_ROWS_FACES) return 0;
  return rows_layout(nullptr, n_faces, kind).bytes;
}

extern "C" int fnr_mesh_vertex_rows_count(int64_t n_vertices, int64_t n_faces, const int32_t* faces, int32_t kind,
                                          uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_mesh_vertex_rows_count");
  if (int rc = mesh_sizes_check("mesh_vertex_rows_count", n_vertices, n_faces)) return rc;
  if (int rc = rows_kind_check("mesh_vertex_rows_count", n_faces, kind)) return rc;
  FNR_CHECK_ARG(counts != nullptr, "mesh_vertex_rows_count: null counts");
  FNR_CHECK_ARG(n_faces == 0 || faces, "mesh_vertex_rows_count: null faces");
  if (int rc = mesh_workspace_check("mesh_vertex_rows_count", workspace, workspace_bytes,
                                    fnr_mesh_vertex_rows_workspace_bytes(n_vertices, n_faces, kind)))
    return rc;
  hipStream_t st = as_stream(stream);
  const long long V = n_vertices, F = n_faces;
  const RowsWs w = rows_layout(workspace, F, kind);
  FNR_HIP(hipMemsetAsync(w.header, 0, 64, st));
  FNR_HIP(hipMemsetAsync(counts, 0, sizeof(uint64_t), st));
  if (F == 0) return FNR_OK;
  {
    FNR_PROF(OP_EXPORT_COMPACT, w.N);
    hipLaunchKernelGGL(k_rows_keys, dim3(grid_for(w.N)), dim3(MESH_BLOCK), 0, st, w, V, F, (int)kind, faces);
    FNR_LAUNCH_CHECK();
    const int* src = nullptr;
    int turn = 0;
    if (int rc = sort_bytes(st, w.sort, w.N, w.keys, 0, bytes_for(kind == FNR_MESH_ROWS_NEIGHBOURS ? V : F), src, turn)) return rc;
    if (int rc = sort_bytes(st, w.sort, w.N, w.keys, 4, bytes_for(V), src, turn)) return rc;
    hipLaunchKernelGGL(k_rows_mark, dim3(grid_for(w.N)), dim3(MESH_BLOCK), 0, st, w, (int)kind, src);
    FNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_scan<false>, dim3(1), dim3(SCAN_THREADS), 0, st, w.mark, w.pos, w.N,
                       reinterpret_cast<unsigned long long*>(counts), w.header + 1);
    FNR_LAUNCH_CHECK();
    const unsigned long long tail[2] = {(unsigned long long)w.N, ROWS_MAGIC + (unsigned long long)kind};
    FNR_HIP(hipMemcpyAsync(w.header + 2, tail, sizeof(tail), hipMemcpyHostToDevice, st));
  }
  unsigned long long host[8];
  return filter_header("mesh_vertex_rows_count", w.header, host, st);
}

extern "C" int fnr_mesh_vertex_rows_emit(int64_t n_vertices, int64_t n_faces, int32_t kind, const void* workspace,
                                         size_t workspace_bytes, int64_t n_entries, int32_t* offsets, int32_t* entries,
                                         void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_mesh_vertex_rows_emit");
  if (int rc = mesh_sizes_check("mesh_vertex_rows_emit", n_vertices, n_faces)) return rc;
  if (int rc = rows_kind_check("mesh_vertex_rows_emit", n_faces, kind)) return rc;
  FNR_CHECK_ARG(offsets != nullptr, "mesh_vertex_rows_emit: null offsets");
  FNR_CHECK_ARG(n_entries >= 0 && n_entries <= rows_keys(n_faces, kind), "mesh_vertex_rows_emit: n_entries outside 0..n_keys");
  FNR_CHECK_ARG(n_entries == 0 || entries, "mesh_vertex_rows_emit: null entries");
  hipStream_t st = as_stream(stream);
  const long long V = n_vertices, F = n_faces, E = n_entries;
  if (F == 0) {
    FNR_HIP(hipMemsetAsync(offsets, 0, 4 * ((size_t)V + 1), st));
    return FNR_OK;
  }
  if (int rc = mesh_workspace_check("mesh_vertex_rows_emit", workspace, workspace_bytes,
                                    fnr_mesh_vertex_rows_workspace_bytes(n_vertices, n_faces, kind)))
    return rc;
  const RowsWs w = rows_layout(const_cast<void*>(workspace), F, kind);
  unsigned long long host[8];
  if (int rc = filter_header("mesh_vertex_rows_emit", w.header, host, st)) return rc;
  FNR_CHECK_ARG(host[3] == ROWS_MAGIC + (unsigned long long)kind && host[2] == (unsigned long long)w.N,
                "mesh_vertex_rows_emit: the workspace does not come from fnr_mesh_vertex_rows_count on these sizes and kind");
  FNR_CHECK_ARG(host[1] == (unsigned long long)E, "mesh_vertex_rows_emit: n_entries %lld inconsistent with counts %llu", E, host[1]);
  {
    FNR_PROF(OP_EXPORT_COMPACT, w.N);
    const int* order = rows_final_order(w, V, F, kind);
    if (E > 0) {
      hipLaunchKernelGGL(k_rows_entries, dim3(grid_for(w.N)), dim3(MESH_BLOCK), 0, st, w, E, order, entries);
      FNR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_rows_offsets, dim3(grid_for(V + 1)), dim3(MESH_BLOCK), 0, st, w, V, E, order, offsets);
    FNR_LAUNCH_CHECK();
  }
  return filter_header("mesh_vertex_rows_emit", w.header, host, st);
}

extern "C" size_t fnr_mesh_smooth_workspace_bytes(int64_t n_vertices) {
  if (n_vertices < 0 || n_vertices > 0x7fffffffll) return 0;
  return 64 + 2 * align16(8 * 3 * (size_t)n_vertices);
}

extern "C" int fnr_mesh_smooth(int64_t n_vertices, const float* vertices, int64_t n_entries, const int32_t* offsets,
                               const int32_t* neighbours, int32_t n_steps, const double* factors, int32_t weights, float* out,
                               void* workspace, size_t workspace_bytes, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_mesh_smooth");
  if (int rc = mesh_sizes_check("mesh_smooth", n_vertices, 0)) return rc;
  if (int rc = rows_arguments_check("mesh_smooth", n_vertices, n_entries, offsets, neighbours)) return rc;
  FNR_CHECK_ARG(n_steps >= 0 && (n_steps == 0 || factors), "mesh_smooth: n_steps < 0 or null factors");
  FNR_CHECK_ARG(weights == FNR_MESH_WEIGHTS_UNIFORM || weights == FNR_MESH_WEIGHTS_INVERSE_DISTANCE,
                "mesh_smooth: weights %d is neither UNIFORM nor INVERSE_DISTANCE", weights);
  FNR_CHECK_ARG(n_vertices == 0 || (vertices && out), "mesh_smooth: null vertices / out");
  if (n_vertices == 0) return FNR_OK;
  if (int rc = mesh_workspace_check("mesh_smooth", workspace, workspace_bytes, fnr_mesh_smooth_workspace_bytes(n_vertices)))
    return rc;
  hipStream_t st = as_stream(stream);
  const long long V = n_vertices, E = n_entries;
  char* base = reinterpret_cast<char*>(workspace);
  unsigned long long* header = reinterpret_cast<unsigned long long*>(base);
  double* buffer[2] = {reinterpret_cast<double*>(base + 64),
                       reinterpret_cast<double*>(base + 64 + align16(8 * 3 * (size_t)V))};
  FNR_HIP(hipMemsetAsync(header, 0, 64, st));
  {
    FNR_PROF(OP_EXPORT_COMPACT, V * (long long)(n_steps + 1));
    hipLaunchKernelGGL(k_smooth_load, dim3(grid_for(3 * V)), dim3(MESH_BLOCK), 0, st, 3 * V, vertices, buffer[0]);
    FNR_LAUNCH_CHECK();
    int at = 0;
    for (int s = 0; s < n_steps; ++s) {
      hipLaunchKernelGGL(k_smooth_step, dim3(grid_for(V)), dim3(MESH_BLOCK), 0, st, header, V, E, offsets, neighbours,
                         (const double*)buffer[at], buffer[at ^ 1], factors[s], (int)weights);
      FNR_LAUNCH_CHECK();
      at ^= 1;
    }
    hipLaunchKernelGGL(k_smooth_store, dim3(grid_for(3 * V)), dim3(MESH_BLOCK), 0, st, 3 * V, (const double*)buffer[at], out);
    FNR_LAUNCH_CHECK();
  }
  unsigned long long host[8];
  return filter_header("mesh_smooth", header, host, st);
}

extern "C" int fnr_mesh_vertex_normals(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                                       int64_t n_entries, const int32_t* offsets, const int32_t* face_rows, float* normals,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_mesh_vertex_normals");
  if (int rc = mesh_sizes_check("mesh_vertex_normals", n_vertices, n_faces)) return rc;
  if (int rc = rows_arguments_check("mesh_vertex_normals", n_vertices, n_entries, offsets, face_rows)) return rc;
  FNR_CHECK_ARG(n_vertices == 0 || (vertices && normals), "mesh_vertex_normals: null vertices / normals");
  FNR_CHECK_ARG(n_faces == 0 || faces, "mesh_vertex_normals: null faces");
  if (n_vertices == 0) return FNR_OK;
  if (int rc = mesh_workspace_check("mesh_vertex_normals", workspace, workspace_bytes, 64)) return rc;
  hipStream_t st = as_stream(stream);
  unsigned long long* header = reinterpret_cast<unsigned long long*>(workspace);
  FNR_HIP(hipMemsetAsync(header, 0, 64, st));
  {
    FNR_PROF(OP_EXPORT_COMPACT, n_vertices);
    hipLaunchKernelGGL(k_vertex_normals, dim3(grid_for(n_vertices)), dim3(MESH_BLOCK), 0, st, header, (long long)n_vertices,
                       (long long)n_faces, (long long)n_entries, vertices, faces, offsets, face_rows, normals);
    FNR_LAUNCH_CHECK();
  }
  unsigned long long host[8];
  return filter_header("mesh_vertex_normals", header, host, st);
}

extern "C" int fnr_mesh_rows_mean(int64_t n_rows, int64_t n_entries, const int32_t* offsets, const int32_t* members,
                                  int64_t n_values, const float* values, float* out, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_mesh_rows_mean");
  FNR_CHECK_ARG(n_rows >= 0 && n_rows <= 0x7fffffffll && n_values >= 0 && n_values <= 0x7fffffffll,
                "mesh_rows_mean: n_rows / n_values outside 0..2^31 - 1");
  if (int rc = rows_arguments_check("mesh_rows_mean", n_rows, n_entries, offsets, members)) return rc;
  FNR_CHECK_ARG(n_rows == 0 || out, "mesh_rows_mean: null out");
  FNR_CHECK_ARG(n_values == 0 || values, "mesh_rows_mean: null values");
  if (n_rows == 0) return FNR_OK;
  if (int rc = mesh_workspace_check("mesh_rows_mean", workspace, workspace_bytes, 64)) return rc;
  hipStream_t st = as_stream(stream);
  unsigned long long* header = reinterpret_cast<unsigned long long*>(workspace);
  FNR_HIP(hipMemsetAsync(header, 0, 64, st));
  {
    FNR_PROF(OP_EXPORT_COMPACT, n_rows);
    hipLaunchKernelGGL(k_rows_mean, dim3(grid_for(n_rows)), dim3(MESH_BLOCK), 0, st, header, (long long)n_rows,
                       (long long)n_entries, (long long)n_values, offsets, members, values, out);
    FNR_LAUNCH_CHECK();
  }
  unsigned long long host[8];
  return filter_header("mesh_rows_mean", header, host, st);
}

extern "C" size_t fnr_mesh_cluster_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
  if (n_vertices < 0 || n_faces < 0 || n_vertices > 0x7fffffffll || n_faces > 0x7fffffffll) return 0;
  return cluster_layout(nullptr, n_vertices, n_faces).bytes;
}

extern "C" int fnr_mesh_cluster_count(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                                      double voxel_size, const double* origin, int32_t* vertex_cluster, uint64_t* counts,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_mesh_cluster_count");
  if (int rc = mesh_sizes_check("mesh_cluster_count", n_vertices, n_faces)) return rc;
  FNR_CHECK_ARG(std::isfinite(voxel_size) && voxel_size > 0.0, "mesh_cluster_count: voxel_size %g is not a positive number",
                voxel_size);
  FNR_CHECK_ARG(origin != nullptr, "mesh_cluster_count: null origin");
  FNR_CHECK_ARG(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]),
                "mesh_cluster_count: the origin (%g, %g, %g) is not finite", origin[0], origin[1], origin[2]);
  FNR_CHECK_ARG(counts != nullptr, "mesh_cluster_count: null counts");
  FNR_CHECK_ARG(n_vertices == 0 || (vertices && vertex_cluster), "mesh_cluster_count: null vertices / vertex_cluster");
  FNR_CHECK_ARG(n_faces == 0 || faces, "mesh_cluster_count: null faces");
  if (int rc = mesh_workspace_check("mesh_cluster_count", workspace, workspace_bytes,
                                    fnr_mesh_cluster_workspace_bytes(n_vertices, n_faces)))
    return rc;
  hipStream_t st = as_stream(stream);
  const long long V = n_vertices, F = n_faces;
  const ClusterWs w = cluster_layout(workspace, V, F);
  unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
  FNR_HIP(hipMemsetAsync(w.header, 0, 64, st));
  FNR_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(uint64_t), st));
  if (V == 0 && F == 0) return FNR_OK;
  {
    FNR_PROF(OP_EXPORT_COMPACT, V + F);
    if (V > 0) {
      hipLaunchKernelGGL(k_cluster_cells, dim3(grid_for(V)), dim3(MESH_BLOCK), 0, st, w, vertices,
                         Double3{origin[0], origin[1], origin[2]}, voxel_size);
      FNR_LAUNCH_CHECK();
      const int* src = nullptr;
      int turn = 0;
      if (int rc = sort_bytes(st, w.vsort, V, w.cell, 0, CLUSTER_CELL_BYTES, src, turn)) return rc;
      hipLaunchKernelGGL(k_cluster_heads, dim3(grid_for(V)), dim3(MESH_BLOCK), 0, st, w, src);
      FNR_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_mesh_scan<false>, dim3(1), dim3(SCAN_THREADS), 0, st, w.head, w.run, V, c, w.header + 1);
      FNR_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_cluster_runs, dim3(grid_for(V)), dim3(MESH_BLOCK), 0, st, w);
      FNR_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_cluster_reps, dim3(grid_for(V)), dim3(MESH_BLOCK), 0, st, w, src);
      FNR_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_mesh_scan<false>, dim3(1), dim3(SCAN_THREADS), 0, st, w.rank, w.rank, V,
                         (unsigned long long*)nullptr, (unsigned long long*)nullptr);
      FNR_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_cluster_labels, dim3(grid_for(V)), dim3(MESH_BLOCK), 0, st, w, vertex_cluster);
      FNR_LAUNCH_CHECK();
    }
    if (F > 0) {
      hipLaunchKernelGGL(k_cluster_face_keys, dim3(grid_for(F)), dim3(MESH_BLOCK), 0, st, w, faces);
      FNR_LAUNCH_CHECK();
      const int* src = nullptr;
      int turn = 0;
      const int vb = bytes_for(V);
      if (int rc = sort_bytes(st, w.fsort, F, w.kc, 0, vb, src, turn)) return rc;
      if (int rc = sort_bytes(st, w.fsort, F, w.kab, 0, vb, src, turn)) return rc;
      if (int rc = sort_bytes(st, w.fsort, F, w.kab, 4, vb, src, turn)) return rc;
      hipLaunchKernelGGL(k_cluster_face_mark, dim3(grid_for(F)), dim3(MESH_BLOCK), 0, st, w, src);
      FNR_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_mesh_scan<true>, dim3(1), dim3(SCAN_THREADS), 0, st, w.fmap, w.fmap, F, c + 1, w.header + 2);
      FNR_LAUNCH_CHECK();
    }
  }
  unsigned long long host[8];
  return filter_header("mesh_cluster_count", w.header, host, st);
}

extern "C" int fnr_mesh_cluster_emit(int64_t n_vertices, int64_t n_faces, const int32_t* faces, void* workspace,
                                     size_t workspace_bytes, int64_t n_clusters, int64_t n_new_faces, int32_t* offsets,
                                     int32_t* members, int32_t* new_faces, int32_t* face_ids, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_mesh_cluster_emit");
  if (int rc = mesh_sizes_check("mesh_cluster_emit", n_vertices, n_faces)) return rc;
  FNR_CHECK_ARG(n_clusters >= 0 && n_clusters <= n_vertices && n_new_faces >= 0 && n_new_faces <= n_faces,
                "mesh_cluster_emit: new sizes outside 0..n_vertices / 0..n_faces");
  FNR_CHECK_ARG(offsets != nullptr, "mesh_cluster_emit: null offsets");
  FNR_CHECK_ARG(n_vertices == 0 || members, "mesh_cluster_emit: null members");
  FNR_CHECK_ARG(n_faces == 0 || faces, "mesh_cluster_emit: null faces");
  FNR_CHECK_ARG(n_new_faces == 0 || (new_faces && face_ids), "mesh_cluster_emit: null new_faces / face_ids");
  if (int rc = mesh_workspace_check("mesh_cluster_emit", workspace, workspace_bytes,
                                    fnr_mesh_cluster_workspace_bytes(n_vertices, n_faces)))
    return rc;
  hipStream_t st = as_stream(stream);
  const long long V = n_vertices, F = n_faces, C = n_clusters;
  if (V == 0) {
    FNR_CHECK_ARG(n_new_faces == 0, "mesh_cluster_emit: faces without vertices");
    FNR_HIP(hipMemsetAsync(offsets, 0, 4, st));
    return FNR_OK;
  }
  const ClusterWs w = cluster_layout(workspace, V, F);
  unsigned long long host[8];
  if (int rc = filter_header("mesh_cluster_emit", w.header, host, st)) return rc;
  FNR_CHECK_ARG(host[3] == CLUSTER_MAGIC && host[4] == (unsigned long long)V && host[5] == (unsigned long long)F,
                "mesh_cluster_emit: the workspace does not come from fnr_mesh_cluster_count on these sizes");
  FNR_CHECK_ARG(host[1] == (unsigned long long)C && host[2] == (unsigned long long)n_new_faces,
                "mesh_cluster_emit: n_clusters %lld / n_new_faces %lld inconsistent with counts %llu / %llu", C,
                (long long)n_new_faces, host[1], host[2]);
  {
    FNR_PROF(OP_EXPORT_COMPACT, V + F);
    const int* order = cluster_vertex_order(w);
    unsigned* csize = w.rank;                             // the ranks are in `cluster` by now
    hipLaunchKernelGGL(k_cluster_sizes, dim3(grid_for(V)), dim3(MESH_BLOCK), 0, st, w, C, order, csize);
    FNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_scan<false>, dim3(1), dim3(SCAN_THREADS), 0, st, (const unsigned*)csize,
                       reinterpret_cast<unsigned*>(offsets), C, (unsigned long long*)nullptr, (unsigned long long*)nullptr);
    FNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cluster_members, dim3(grid_for(V)), dim3(MESH_BLOCK), 0, st, w, C, order, offsets, members);
    FNR_LAUNCH_CHECK();
    if (n_new_faces > 0) {
      hipLaunchKernelGGL(k_cluster_faces, dim3(grid_for(F)), dim3(MESH_BLOCK), 0, st, w, C, (long long)n_new_faces, faces,
                         new_faces, face_ids);
      FNR_LAUNCH_CHECK();
    }
  }
  return filter_header("mesh_cluster_emit", w.header, host, st);
}
