// mesh.hip — triangle-mesh connectivity for the mesh exports (the contract is stated in include/fruitnerf_hip.h): edge
// incidences in an open-addressing table, union-find over faces, per-component statistics through a stable radix sort of the
// faces by component and a fixed-shape segmented reduction, and order-preserving selection.  Everything is gather / atomic
// bound; LDS holds only block scans, a block's digits and a block's terms.
//
// Shared-machine rules of this file: no workgroup waits for another (the only retry loops are compare-and-swap retries);
// every probe sequence and pointer chase is bounded by the table size / the face count; a bound that is exceeded, an index
// outside [0, V) or a label outside [0, C) sets a bit in the workspace's error word, which the entry point reads back.
#include "common.hpp"
#include "mesh_common.hpp"
#include "sequencer.hpp"

namespace fnr {

constexpr unsigned long long EDGE_EMPTY = ~0ull;     // never a key: a key's halves are both below 2^31
constexpr int NO_FACE = 0x7fffffff;
constexpr unsigned OFF_UNSET = 0xffffffffu;
constexpr unsigned long long MESH_MAGIC = 0x666e726d65736831ull;
enum : unsigned { MESH_ERR_PROBE = 1u, MESH_ERR_CHASE = 2u, MESH_ERR_INDEX = 4u, MESH_ERR_LABEL = 8u, MESH_ERR_TABLE = 16u };

// the workspace of fnr_mesh_components / fnr_mesh_component_stats, every array 16-byte aligned
struct MeshWs {
  unsigned long long* header;   // [0] error word (low 32 bits), [1] n_components, [2] n_faces, [3] MESH_MAGIC once labelled
  unsigned long long* keys;     // [T] edge keys
  int* first;                   // [T] smallest face of the edge
  unsigned* cnt;                // [T] incidences
  int* parent;                  // [F] union-find
  int* root;                    // [F]
  unsigned* rank;               // [F] exclusive scan over "is root"
  int* order[2];                // [F] faces sorted by component (ping-pong)
  unsigned* hist;               // [256 * nb] digit counts, digit-major
  unsigned* off;                // [F + 1] first sorted position of a component (OFF_UNSET until k_stats_chunk finds it)
  double* bh_sum;               // [nb][5] partial sums of the run that starts a block
  float* bh_box;                // [nb][6]
  long long T, nb;
  size_t bytes;
};

static inline long long mesh_table_size(long long F) {
  long long T = 1024;
  while (T < 4 * F) T <<= 1;
  return T;
}

static MeshWs mesh_layout(void* base, long long F) {
  MeshWs w;
  w.T = mesh_table_size(F);
  w.nb = (F + MESH_BLOCK - 1) / MESH_BLOCK;
  size_t at = 0;
  char* p = reinterpret_cast<char*>(base);
  auto take = [&](size_t bytes) {
    char* r = p + at;
    at += (bytes + 15) & ~(size_t)15;
    return r;
  };
  w.header = reinterpret_cast<unsigned long long*>(take(64));
  w.keys = reinterpret_cast<unsigned long long*>(take(8 * (size_t)w.T));
  w.first = reinterpret_cast<int*>(take(4 * (size_t)w.T));
  w.cnt = reinterpret_cast<unsigned*>(take(4 * (size_t)w.T));
  w.parent = reinterpret_cast<int*>(take(4 * (size_t)F));
  w.root = reinterpret_cast<int*>(take(4 * (size_t)F));
  w.rank = reinterpret_cast<unsigned*>(take(4 * (size_t)F));
  w.order[0] = reinterpret_cast<int*>(take(4 * (size_t)F));
  w.order[1] = reinterpret_cast<int*>(take(4 * (size_t)F));
  w.hist = reinterpret_cast<unsigned*>(take(4 * 256 * (size_t)w.nb));
  w.off = reinterpret_cast<unsigned*>(take(4 * ((size_t)F + 1)));
  w.bh_sum = reinterpret_cast<double*>(take(8 * 5 * (size_t)w.nb));
  w.bh_box = reinterpret_cast<float*>(take(4 * 6 * (size_t)w.nb));
  w.bytes = at;
  return w;
}

// the workspace of fnr_mesh_select_count / fnr_mesh_select_emit
struct SelectWs {
  unsigned long long* header;   // [0] error word
  unsigned* vmap;               // [V] new index + 1 of a kept vertex, 0: dropped
  unsigned* fmap;               // [F] new row + 1 of a kept face, 0: dropped
  size_t bytes;
};

static SelectWs select_layout(void* base, long long V, long long F) {
  SelectWs w;
  char* p = reinterpret_cast<char*>(base);
  const size_t vbytes = (4 * (size_t)V + 15) & ~(size_t)15, fbytes = (4 * (size_t)F + 15) & ~(size_t)15;
  w.header = reinterpret_cast<unsigned long long*>(p);
  w.vmap = reinterpret_cast<unsigned*>(p + 64);
  w.fmap = reinterpret_cast<unsigned*>(p + 64 + vbytes);
  w.bytes = 64 + vbytes + fbytes;
  return w;
}

// ---- edge incidences ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long edge_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// slot s of face f: the edge from index s to index (s + 1) % 3.  false: the slot has no edge (a == b) or a bad index
__device__ __forceinline__ bool edge_key(const int* __restrict__ faces, long long f, int s, long long V,
                                         unsigned long long* header, unsigned long long& key) {
  const int a = faces[3 * f + s], b = faces[3 * f + (s == 2 ? 0 : s + 1)];
  if (a < 0 || b < 0 || (long long)a >= V || (long long)b >= V) {
    mesh_error(header, MESH_ERR_INDEX);
    return false;
  }
  if (a == b) return false;
  const unsigned lo = (unsigned)(a < b ? a : b), hi = (unsigned)(a < b ? b : a);
  key = ((unsigned long long)lo << 32) | hi;
  return true;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_init(MeshWs w, long long F) {
  const long long i = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (i < w.T) {
    w.keys[i] = EDGE_EMPTY;
    w.first[i] = NO_FACE;
    w.cnt[i] = 0u;
  }
  if (i < F) w.parent[i] = (int)i;
}

// One thread per (face, slot).  A slot of the table is claimed by a 64-bit compare-and-swap at device scope; the value the
// swap returns is the only read of a key in this launch.  The probe sequence is linear and at most T long.
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_edges(MeshWs w, long long F, long long V,
                                                           const int* __restrict__ faces) {
  const long long t = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (t >= 3 * F) return;
  const long long f = t / 3;
  unsigned long long key;
  if (!edge_key(faces, f, (int)(t - 3 * f), V, w.header, key)) return;
  const unsigned long long mask = (unsigned long long)w.T - 1ull;
  unsigned long long h = edge_hash(key) & mask;
  for (long long probe = 0; probe < w.T; ++probe) {
    const unsigned long long old = atomicCAS(&w.keys[h], EDGE_EMPTY, key);
    if (old == EDGE_EMPTY || old == key) {
      atomicAdd(&w.cnt[h], 1u);
      atomicMin(&w.first[h], (int)f);
      return;
    }
    h = (h + 1ull) & mask;
  }
  mesh_error(w.header, MESH_ERR_PROBE);
}

// ---- union-find over faces ----------------------------------------------------------------------------------------------
// parent[x] <= x always: a hook puts the larger root under the smaller one, so every chain descends strictly, is at most F
// long, and a tree's root is its smallest face.  Inside the hooking launch the parent words are touched only through
// device-scope atomic loads and compare-and-swap.
__device__ __forceinline__ int uf_load(int* parent, int x) {
  return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool uf_cas(int* parent, int x, int expected, int desired) {
  return __hip_atomic_compare_exchange_strong(&parent[x], &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
}
// the root of x, halving the path on the way (a failed swap is fine: someone else shortened it); -1: bound exceeded
__device__ __forceinline__ int uf_find(int* parent, int x, long long F) {
  for (long long step = 0; step <= F; ++step) {
    const int p = uf_load(parent, x);
    if (p == x) return x;
    const int gp = uf_load(parent, p);
    if (gp != p) uf_cas(parent, x, p, gp);
    x = gp;
  }
  return -1;
}

// One thread per (face, slot): the face is united with the first face of its edge.  The table is read with plain loads:
// the launch boundary made it visible.
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_union(MeshWs w, long long F, long long V,
                                                           const int* __restrict__ faces) {
  const long long t = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (t >= 3 * F) return;
  const long long f = t / 3;
  unsigned long long key;
  if (!edge_key(faces, f, (int)(t - 3 * f), V, w.header, key)) return;
  const unsigned long long mask = (unsigned long long)w.T - 1ull;
  unsigned long long h = edge_hash(key) & mask;
  int g = -1;
  for (long long probe = 0; probe < w.T; ++probe) {
    const unsigned long long k = w.keys[h];
    if (k == key) {
      g = w.first[h];
      break;
    }
    if (k == EDGE_EMPTY) break;
    h = (h + 1ull) & mask;
  }
  if (g < 0 || (long long)g >= F) {        // the edge was inserted by the launch before: it has to be there
    mesh_error(w.header, MESH_ERR_TABLE);
    return;
  }
  int a = (int)f, b = g;
  if (a == b) return;
  // every failed hook means another thread hooked that root: at most F - 1 hooks exist
  for (long long attempt = 0; attempt <= F; ++attempt) {
    a = uf_find(w.parent, a, F);
    b = uf_find(w.parent, b, F);
    if (a < 0 || b < 0) break;
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    if (uf_cas(w.parent, hi, hi, lo)) return;
    a = hi;
    b = lo;
  }
  mesh_error(w.header, MESH_ERR_CHASE);
}

// a later launch: plain loads, nothing is written to parent any more
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_roots(MeshWs w, long long F) {
  const long long f = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (f >= F) return;
  int x = (int)f;
  bool found = false;
  for (long long step = 0; step <= F; ++step) {
    const int p = w.parent[x];
    if (p == x) {
      found = true;
      break;
    }
    if (p < 0 || p > x) break;
    x = p;
  }
  if (!found) {
    mesh_error(w.header, MESH_ERR_CHASE);
    x = (int)f;
  }
  w.root[f] = x;
  w.rank[f] = (x == (int)f) ? 1u : 0u;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_labels(MeshWs w, long long F, int* __restrict__ face_component) {
  const long long f = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (f >= F) return;
  face_component[f] = (int)w.rank[w.root[f]];
  if (f == 0) {
    w.header[2] = (unsigned long long)F;
    w.header[3] = MESH_MAGIC;
  }
}

// ---- statistics ---------------------------------------------------------------------------------------------------------
struct StatsOut {
  int *n_faces, *boundary, *nonmanifold;
  float *lo, *hi;
  double *area, *volume, *moment;
};

// counts[c] += 1 for every active lane; the lanes of a wave that count the same entry send ONE atomic (a mesh is mostly one
// component: without this every lane of every wave would queue on the same word).  All lanes of the wave must call it.
__device__ __forceinline__ void wave_count(int* counts, int c, bool active) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(active);
  while (todo) {                                          // wave-uniform; at most 64 trips
    const int leader = __ffsll((long long)todo) - 1;
    const int c0 = __shfl(c, leader, 64);
    const unsigned long long same = __ballot(active && c == c0);
    if (lane == leader) atomicAdd(&counts[c0], (int)__popcll(same));
    todo &= ~same;
  }
}

// one thread per slot of the table the components call left behind
__global__ __launch_bounds__(MESH_BLOCK) void k_stats_edges(MeshWs w, long long F, long long C,
                                                            const int* __restrict__ comp, StatsOut out) {
  const long long i = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  unsigned n = 0u;
  int c = -1;
  if (i < w.T && w.keys[i] != EDGE_EMPTY) {
    const int f = w.first[i];
    if (f < 0 || (long long)f >= F) {
      mesh_error(w.header, MESH_ERR_TABLE);
    } else {
      c = comp[f];
      if (c < 0 || (long long)c >= C) {
        mesh_error(w.header, MESH_ERR_LABEL);
        c = -1;
      } else {
        n = w.cnt[i];
      }
    }
  }
  wave_count(out.boundary, c, c >= 0 && n == 1u);
  wave_count(out.nonmanifold, c, c >= 0 && n >= 3u);
}

__device__ __forceinline__ int sorted_face(const int* __restrict__ order, long long p) { return order ? order[p] : (int)p; }

// One pass of the least-significant-digit radix sort of the faces by component, 8 bits a pass, 256 faces a block.  A
// face's place among the block's faces of its digit is counted in LDS, in input order: the pass is stable, and so the
// sorted faces of a component ascend.
__device__ __forceinline__ int block_digit(const MeshWs& w, const int* __restrict__ src, const int* __restrict__ comp,
                                           long long F, int shift, int* s_digit, long long& p) {
  p = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  int d = 256;
  if (p < F) {
    const int f = sorted_face(src, p);
    if (f >= 0 && (long long)f < F) {
      d = (int)(((unsigned)comp[f] >> shift) & 255u);
    } else {                                              // never: every pass writes a permutation
      mesh_error(w.header, MESH_ERR_LABEL);
      d = 0;
    }
  }
  s_digit[threadIdx.x] = d;
  __syncthreads();
  return d;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_sort_count(MeshWs w, long long F, const int* __restrict__ src,
                                                           const int* __restrict__ comp, int shift) {
  __shared__ int s_digit[MESH_BLOCK];
  long long p;
  block_digit(w, src, comp, F, shift, s_digit, p);
  unsigned n = 0u;
  for (int j = 0; j < MESH_BLOCK; ++j) n += (s_digit[j] == (int)threadIdx.x) ? 1u : 0u;
  w.hist[(size_t)threadIdx.x * w.nb + blockIdx.x] = n;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_sort_emit(MeshWs w, long long F, const int* __restrict__ src,
                                                          int* __restrict__ dst, const int* __restrict__ comp, int shift) {
  __shared__ int s_digit[MESH_BLOCK];
  long long p;
  const int d = block_digit(w, src, comp, F, shift, s_digit, p);
  unsigned before = 0u;
  for (int j = 0; j < (int)threadIdx.x; ++j) before += (s_digit[j] == d) ? 1u : 0u;
  if (p >= F) return;
  const long long at = (long long)w.hist[(size_t)d * w.nb + blockIdx.x] + before;
  if (at < F) dst[at] = sorted_face(src, p);
  else mesh_error(w.header, MESH_ERR_LABEL);
}

// One thread per sorted position: the face's float64 terms and its box go to LDS, and the first thread of every run of
// one component adds the run up in position order; where a component begins, its first sorted position goes to off[].
// The run that starts the block goes to the block's record; a run that starts inside the block is the first piece of its
// component and goes to the output, where k_stats_combine finds it.
__global__ __launch_bounds__(MESH_BLOCK) void k_stats_chunk(MeshWs w, long long F, long long V, long long C,
                                                            const int* __restrict__ order, const int* __restrict__ comp,
                                                            const float* __restrict__ vertices,
                                                            const int* __restrict__ faces, StatsOut out) {
  __shared__ double s_sum[5][MESH_BLOCK];
  __shared__ float s_box[6][MESH_BLOCK];
  __shared__ int s_comp[MESH_BLOCK];
  const int tid = threadIdx.x;
  const long long p = (long long)blockIdx.x * MESH_BLOCK + tid;
  int c = -1;
  double term[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  float box[6] = {__builtin_inff(), __builtin_inff(), __builtin_inff(), -__builtin_inff(), -__builtin_inff(),
                  -__builtin_inff()};
  if (p < F) {
    const int f = sorted_face(order, p);
    const int label = (f >= 0 && (long long)f < F) ? comp[f] : -1;
    int idx[3] = {0, 0, 0};
    bool ok = label >= 0 && (long long)label < C;
    if (ok) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        idx[k] = faces[3 * (long long)f + k];
        ok = ok && idx[k] >= 0 && (long long)idx[k] < V;
      }
      if (!ok) mesh_error(w.header, MESH_ERR_INDEX);
    } else {
      mesh_error(w.header, MESH_ERR_LABEL);
    }
    if (ok) {
      c = label;
      double v[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float x = vertices[3 * (long long)idx[k] + a];
          v[k][a] = (double)x;
          box[a] = fminf(box[a], x);
          box[3 + a] = fmaxf(box[3 + a], x);
        }
      }
      double e1[3], e2[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        e1[a] = v[1][a] - v[0][a];
        e2[a] = v[2][a] - v[0][a];
      }
      const double nx = e1[1] * e2[2] - e1[2] * e2[1];
      const double ny = e1[2] * e2[0] - e1[0] * e2[2];
      const double nz = e1[0] * e2[1] - e1[1] * e2[0];
      const double area = sqrt((nx * nx + ny * ny) + nz * nz) / 2.0;
      const double cx = v[1][1] * v[2][2] - v[1][2] * v[2][1];
      const double cy = v[1][2] * v[2][0] - v[1][0] * v[2][2];
      const double cz = v[1][0] * v[2][1] - v[1][1] * v[2][0];
      term[0] = area;
      term[1] = ((v[0][0] * cx + v[0][1] * cy) + v[0][2] * cz) / 6.0;
#pragma unroll
      for (int a = 0; a < 3; ++a) term[2 + a] = area * (((v[0][a] + v[1][a]) + v[2][a]) / 3.0);
    }
  }
  s_comp[tid] = c;
#pragma unroll
  for (int q = 0; q < 5; ++q) s_sum[q][tid] = term[q];
#pragma unroll
  for (int q = 0; q < 6; ++q) s_box[q][tid] = box[q];
  __syncthreads();
  if (c < 0) return;
  int before = -1;                                        // the component of the sorted position before this one
  if (tid > 0) {
    before = s_comp[tid - 1];
  } else if (p > 0) {
    const int f = sorted_face(order, p - 1);
    if (f >= 0 && (long long)f < F) before = comp[f];
  }
  if (before != c) w.off[c] = (unsigned)p;                // the faces are sorted: one writer per component
  if (tid > 0 && before == c) return;
  for (int j = tid + 1; j < MESH_BLOCK && s_comp[j] == c; ++j) {
#pragma unroll
    for (int q = 0; q < 5; ++q) term[q] += s_sum[q][j];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      box[a] = fminf(box[a], s_box[a][j]);
      box[3 + a] = fmaxf(box[3 + a], s_box[3 + a][j]);
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < 5; ++q) w.bh_sum[5 * (size_t)blockIdx.x + q] = term[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) w.bh_box[6 * (size_t)blockIdx.x + q] = box[q];
  } else {
    out.area[c] = term[0];
    out.volume[c] = term[1];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      out.moment[3 * (size_t)c + a] = term[2 + a];
      out.lo[3 * (size_t)c + a] = box[a];
      out.hi[3 * (size_t)c + a] = box[3 + a];
    }
  }
}

// One wave per component: lane l adds the block records l, l + 64, ... of the component's later blocks in order, a
// butterfly adds the lanes, and the component's first piece (if it began inside a block) comes first.  The shape depends
// on the component sizes alone.
__global__ __launch_bounds__(MESH_BLOCK) void k_stats_combine(MeshWs w, long long F, long long C, StatsOut out) {
  const int lane = threadIdx.x & 63;
  const long long c = (long long)blockIdx.x * (MESH_BLOCK / 64) + (threadIdx.x >> 6);
  if (c >= C) return;                                     // whole waves leave together
  const unsigned s_raw = w.off[c], e_raw = (c + 1 < C) ? w.off[c + 1] : (unsigned)F;
  const bool present = s_raw != OFF_UNSET && e_raw != OFF_UNSET && (long long)e_raw <= F && s_raw < e_raw;
  if (!present && lane == 0) mesh_error(w.header, MESH_ERR_LABEL);      // a label no face carries
  const long long s = present ? (long long)s_raw : 0, e = present ? (long long)e_raw : 0;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  float box[6] = {__builtin_inff(), __builtin_inff(), __builtin_inff(), -__builtin_inff(), -__builtin_inff(),
                  -__builtin_inff()};
  const bool inside = (s % MESH_BLOCK) != 0;
  if (e > s) {
    const long long first = s / MESH_BLOCK + (inside ? 1 : 0), last = (e - 1) / MESH_BLOCK;
    for (long long b = first + lane; b <= last; b += 64) {
#pragma unroll
      for (int q = 0; q < 5; ++q) acc[q] += w.bh_sum[5 * (size_t)b + q];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        box[a] = fminf(box[a], w.bh_box[6 * (size_t)b + a]);
        box[3 + a] = fmaxf(box[3 + a], w.bh_box[6 * (size_t)b + 3 + a]);
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int q = 0; q < 5; ++q) acc[q] += __shfl_xor(acc[q], d, 64);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      box[a] = fminf(box[a], __shfl_xor(box[a], d, 64));
      box[3 + a] = fmaxf(box[3 + a], __shfl_xor(box[3 + a], d, 64));
    }
  }
  if (lane != 0) return;
  if (inside && e > s) {
    acc[0] = out.area[c] + acc[0];
    acc[1] = out.volume[c] + acc[1];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      acc[2 + a] = out.moment[3 * c + a] + acc[2 + a];
      box[a] = fminf(box[a], out.lo[3 * c + a]);
      box[3 + a] = fmaxf(box[3 + a], out.hi[3 * c + a]);
    }
  }
  out.n_faces[c] = (int)(e - s);
  out.area[c] = acc[0];
  out.volume[c] = acc[1];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    out.moment[3 * c + a] = acc[2 + a];
    out.lo[3 * c + a] = box[a];
    out.hi[3 * c + a] = box[3 + a];
  }
}

// ---- selection ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MESH_BLOCK) void k_select_mark(SelectWs w, long long V, long long F,
                                                            const int* __restrict__ faces,
                                                            const unsigned char* __restrict__ keep) {
  const long long f = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (f >= F) return;
  const unsigned k = keep[f] != 0 ? 1u : 0u;
  w.fmap[f] = k;
  if (!k) return;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int i = faces[3 * f + s];
    if (i < 0 || (long long)i >= V) mesh_error(w.header, MESH_ERR_INDEX);
    else w.vmap[i] = 1u;                                  // every writer stores the same word
  }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_select_vertices(SelectWs w, long long V, long long n_new_vertices,
                                                                int* __restrict__ vertex_ids) {
  const long long v = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (v >= V) return;
  const unsigned m = w.vmap[v];
  if (m && (long long)m <= n_new_vertices) vertex_ids[m - 1u] = (int)v;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_select_faces(SelectWs w, long long V, long long F, long long n_new_vertices,
                                                             long long n_new_faces, const int* __restrict__ faces,
                                                             int* __restrict__ new_faces, int* __restrict__ face_ids) {
  const long long f = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;
  if (f >= F) return;
  const unsigned m = w.fmap[f];
  if (!m || (long long)m > n_new_faces) return;
  face_ids[m - 1u] = (int)f;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int i = faces[3 * f + s];
    unsigned nv = 0u;
    if (i >= 0 && (long long)i < V) nv = w.vmap[i];
    if (nv == 0u || (long long)nv > n_new_vertices) mesh_error(w.header, MESH_ERR_INDEX);
    new_faces[3 * (size_t)(m - 1u) + s] = (int)nv - 1;
  }
}

static const char* mesh_error_text(unsigned bits) {
  if (bits & MESH_ERR_INDEX) return "a face index lies outside [0, n_vertices)";
  if (bits & MESH_ERR_LABEL) return "a component label lies outside [0, n_components)";
  if (bits & MESH_ERR_TABLE) return "the edge table does not belong to these faces";
  if (bits & MESH_ERR_PROBE) return "a probe sequence exceeded the table size";
  return "a parent chain exceeded the face count";
}

// the header back on the host: a synchronisation of the stream
static int read_header(const char* who, const unsigned long long* header, unsigned long long (&host)[4], hipStream_t st) {
  FNR_HIP(hipMemcpyAsync(host, header, sizeof(host), hipMemcpyDeviceToHost, st));
  FNR_HIP(hipStreamSynchronize(st));
  const unsigned bits = (unsigned)(host[0] & 0xffffffffull);
  if (bits) {
    set_error("%s: %s (error word 0x%x)", who, mesh_error_text(bits), bits);
    return FNR_ERR_INVALID;
  }
  return FNR_OK;
}

}  // namespace fnr

using namespace fnr;

extern "C" size_t fnr_mesh_workspace_bytes(int64_t n_faces) {
  if (n_faces < 0 || n_faces > 0x7fffffffll) return 0;
  return mesh_layout(nullptr, n_faces).bytes;
}

extern "C" int fnr_mesh_components(int64_t n_vertices, int64_t n_faces, const int32_t* faces, int32_t* face_component,
                                   uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_mesh_components");
  if (int rc = mesh_sizes_check("mesh_components", n_vertices, n_faces)) return rc;
  FNR_CHECK_ARG(counts != nullptr, "mesh_components: null counts");
  FNR_CHECK_ARG(n_faces == 0 || (faces && face_component), "mesh_components: null faces / face_component");
  if (int rc = mesh_workspace_check("mesh_components", workspace, workspace_bytes, fnr_mesh_workspace_bytes(n_faces)))
    return rc;
  hipStream_t st = as_stream(stream);
  const long long F = n_faces, V = n_vertices;
  const MeshWs w = mesh_layout(workspace, F);
  FNR_HIP(hipMemsetAsync(w.header, 0, 64, st));
  if (F == 0) {
    FNR_HIP(hipMemsetAsync(counts, 0, sizeof(uint64_t), st));
    return FNR_OK;
  }
  {
    FNR_PROF(OP_EXPORT_COMPACT, F);
    hipLaunchKernelGGL(k_mesh_init, dim3(grid_for(w.T > F ? w.T : F)), dim3(MESH_BLOCK), 0, st, w, F);
    FNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_edges, dim3(grid_for(3 * F)), dim3(MESH_BLOCK), 0, st, w, F, V, faces);
    FNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_union, dim3(grid_for(3 * F)), dim3(MESH_BLOCK), 0, st, w, F, V, faces);
    FNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_roots, dim3(grid_for(F)), dim3(MESH_BLOCK), 0, st, w, F);
    FNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_scan<false>, dim3(1), dim3(SCAN_THREADS), 0, st, w.rank, w.rank, F,
                       reinterpret_cast<unsigned long long*>(counts), w.header + 1);
    FNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_labels, dim3(grid_for(F)), dim3(MESH_BLOCK), 0, st, w, F, face_component);
    FNR_LAUNCH_CHECK();
  }
  unsigned long long host[4];
  return read_header("mesh_components", w.header, host, st);
}

extern "C" int fnr_mesh_component_stats(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                                        const int32_t* face_component, int64_t n_components, void* workspace,
                                        size_t workspace_bytes, const fnr_mesh_stats* out, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_mesh_component_stats");
  if (int rc = mesh_sizes_check("mesh_component_stats", n_vertices, n_faces)) return rc;
  FNR_CHECK_ARG(n_components >= 0 && n_components <= n_faces, "mesh_component_stats: n_components %lld outside 0..n_faces",
                (long long)n_components);
  FNR_CHECK_ARG((n_components == 0) == (n_faces == 0), "mesh_component_stats: n_components %lld with %lld faces",
                (long long)n_components, (long long)n_faces);
  FNR_CHECK_ARG(out != nullptr, "mesh_component_stats: null out");
  FNR_CHECK_ARG(n_faces == 0 || (vertices && faces && face_component), "mesh_component_stats: null mesh array");
  FNR_CHECK_ARG(n_components == 0 || (out->n_faces && out->boundary_edges && out->nonmanifold_edges && out->lo && out->hi &&
                                      out->area && out->volume && out->moment),
                "mesh_component_stats: null output array");
  if (int rc = mesh_workspace_check("mesh_component_stats", workspace, workspace_bytes, fnr_mesh_workspace_bytes(n_faces)))
    return rc;
  if (n_faces == 0) return FNR_OK;
  hipStream_t st = as_stream(stream);
  const long long F = n_faces, V = n_vertices, C = n_components;
  const MeshWs w = mesh_layout(workspace, F);
  unsigned long long host[4];
  if (int rc = read_header("mesh_component_stats", w.header, host, st)) return rc;
  FNR_CHECK_ARG(host[3] == MESH_MAGIC && host[2] == (unsigned long long)F,
                "mesh_component_stats: the workspace does not come from fnr_mesh_components on %lld faces", F);
  FNR_CHECK_ARG(host[1] == (unsigned long long)C, "mesh_component_stats: n_components %lld inconsistent with counts %llu", C,
                host[1]);
  const StatsOut o{out->n_faces, out->boundary_edges, out->nonmanifold_edges, out->lo, out->hi,
                   out->area,    out->volume,         out->moment};
  {
    FNR_PROF(OP_EXPORT_COMPACT, F);
    FNR_HIP(hipMemsetAsync(o.boundary, 0, 4 * (size_t)C, st));
    FNR_HIP(hipMemsetAsync(o.nonmanifold, 0, 4 * (size_t)C, st));
    FNR_HIP(hipMemsetAsync(w.off, 0xff, 4 * (size_t)C, st));
    hipLaunchKernelGGL(k_stats_edges, dim3(grid_for(w.T)), dim3(MESH_BLOCK), 0, st, w, F, C, face_component, o);
    FNR_LAUNCH_CHECK();
    int bits = 0;
    while (bits < 32 && ((C - 1) >> bits) != 0) ++bits;
    const int* src = nullptr;                            // identity
    int turn = 0;
    for (int shift = 0; shift < bits; shift += 8) {
      hipLaunchKernelGGL(k_sort_count, dim3((unsigned)w.nb), dim3(MESH_BLOCK), 0, st, w, F, src, face_component, shift);
      FNR_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_mesh_scan<false>, dim3(1), dim3(SCAN_THREADS), 0, st, w.hist, w.hist, 256 * w.nb,
                         (unsigned long long*)nullptr, (unsigned long long*)nullptr);
      FNR_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_sort_emit, dim3((unsigned)w.nb), dim3(MESH_BLOCK), 0, st, w, F, src, w.order[turn], face_component,
                         shift);
      FNR_LAUNCH_CHECK();
      src = w.order[turn];
      turn ^= 1;
    }
    hipLaunchKernelGGL(k_stats_chunk, dim3((unsigned)w.nb), dim3(MESH_BLOCK), 0, st, w, F, V, C, src, face_component, vertices,
                       faces, o);
    FNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_stats_combine, dim3((unsigned)((C + MESH_BLOCK / 64 - 1) / (MESH_BLOCK / 64))), dim3(MESH_BLOCK), 0,
                       st, w, F, C, o);
    FNR_LAUNCH_CHECK();
  }
  return read_header("mesh_component_stats", w.header, host, st);
}

extern "C" size_t fnr_mesh_select_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
  if (n_vertices < 0 || n_faces < 0 || n_vertices > 0x7fffffffll || n_faces > 0x7fffffffll) return 0;
  return select_layout(nullptr, n_vertices, n_faces).bytes;
}

extern "C" int fnr_mesh_select_count(int64_t n_vertices, int64_t n_faces, const int32_t* faces, const uint8_t* face_keep,
                                     uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_mesh_select_count");
  if (int rc = mesh_sizes_check("mesh_select_count", n_vertices, n_faces)) return rc;
  FNR_CHECK_ARG(counts != nullptr, "mesh_select_count: null counts");
  FNR_CHECK_ARG(n_faces == 0 || (faces && face_keep), "mesh_select_count: null faces / face_keep");
  if (int rc = mesh_workspace_check("mesh_select_count", workspace, workspace_bytes,
                                    fnr_mesh_select_workspace_bytes(n_vertices, n_faces)))
    return rc;
  hipStream_t st = as_stream(stream);
  const long long V = n_vertices, F = n_faces;
  const SelectWs w = select_layout(workspace, V, F);
  FNR_HIP(hipMemsetAsync(w.header, 0, 64, st));
  FNR_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(uint64_t), st));
  if (F == 0) return FNR_OK;
  {
    FNR_PROF(OP_EXPORT_COMPACT, F);
    if (V > 0) FNR_HIP(hipMemsetAsync(w.vmap, 0, 4 * (size_t)V, st));
    hipLaunchKernelGGL(k_select_mark, dim3(grid_for(F)), dim3(MESH_BLOCK), 0, st, w, V, F, faces, face_keep);
    FNR_LAUNCH_CHECK();
    unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
    if (V > 0) {
      hipLaunchKernelGGL(k_mesh_scan<true>, dim3(1), dim3(SCAN_THREADS), 0, st, w.vmap, w.vmap, V, c,
                         (unsigned long long*)nullptr);
      FNR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_mesh_scan<true>, dim3(1), dim3(SCAN_THREADS), 0, st, w.fmap, w.fmap, F, c + 1,
                       (unsigned long long*)nullptr);
    FNR_LAUNCH_CHECK();
  }
  unsigned long long host[4];
  return read_header("mesh_select_count", w.header, host, st);
}

extern "C" int fnr_mesh_select_emit(int64_t n_vertices, int64_t n_faces, const int32_t* faces, const void* workspace,
                                    size_t workspace_bytes, int64_t n_new_vertices, int64_t n_new_faces, int32_t* new_faces,
                                    int32_t* vertex_ids, int32_t* face_ids, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_mesh_select_emit");
  if (int rc = mesh_sizes_check("mesh_select_emit", n_vertices, n_faces)) return rc;
  FNR_CHECK_ARG(n_new_vertices >= 0 && n_new_faces >= 0 && n_new_vertices <= n_vertices && n_new_faces <= n_faces,
                "mesh_select_emit: new sizes outside 0..n_vertices / 0..n_faces");
  FNR_CHECK_ARG(n_faces == 0 || faces, "mesh_select_emit: null faces");
  FNR_CHECK_ARG(n_new_vertices == 0 || vertex_ids, "mesh_select_emit: null vertex_ids");
  FNR_CHECK_ARG(n_new_faces == 0 || (new_faces && face_ids), "mesh_select_emit: null new_faces / face_ids");
  if (int rc = mesh_workspace_check("mesh_select_emit", workspace, workspace_bytes,
                                    fnr_mesh_select_workspace_bytes(n_vertices, n_faces)))
    return rc;
  if (n_faces == 0 || (n_new_vertices == 0 && n_new_faces == 0)) return FNR_OK;
  hipStream_t st = as_stream(stream);
  const long long V = n_vertices, F = n_faces;
  const SelectWs w = select_layout(const_cast<void*>(workspace), V, F);
  {
    FNR_PROF(OP_EXPORT_COMPACT, F);
    if (n_new_vertices > 0) {
      hipLaunchKernelGGL(k_select_vertices, dim3(grid_for(V)), dim3(MESH_BLOCK), 0, st, w, V, (long long)n_new_vertices,
                         vertex_ids);
      FNR_LAUNCH_CHECK();
    }
    if (n_new_faces > 0) {
      hipLaunchKernelGGL(k_select_faces, dim3(grid_for(F)), dim3(MESH_BLOCK), 0, st, w, V, F, (long long)n_new_vertices,
                         (long long)n_new_faces, faces, new_faces, face_ids);
      FNR_LAUNCH_CHECK();
    }
  }
  unsigned long long host[4];
  return read_header("mesh_select_emit", w.header, host, st);
}
