// tsdf.hip — TSDF mesh export (Nerfstudio's `ns-export tsdf`; the contract is stated in include/fruitnerf_hip.h):
// depth fusion with the camera loop inside the kernel, and marching tetrahedra as a count -> scan -> emit compaction whose
// output order is a function of the volume alone.  Both are HBM / gather bound; nothing here needs LDS beyond a block scan.
#include "common.hpp"
#include "sequencer.hpp"

namespace fnr {

constexpr int TSDF_BLOCK = 256;        // FNR_TSDF_MESH_WORKSPACE_BYTES holds two offsets per TSDF_BLOCK nodes
static_assert(TSDF_BLOCK == 256, "FNR_TSDF_MESH_WORKSPACE_BYTES counts blocks of 256 nodes");
constexpr int TSDF_MAX_DIM = 2048;

struct TsdfGrid {
  int nx, ny, nz;
  float lo[3], vs[3];
};

static inline TsdfGrid tsdf_grid(const fnr_tsdf_volume* v) {
  TsdfGrid g;
  g.nx = v->dims[0];
  g.ny = v->dims[1];
  g.nz = v->dims[2];
  for (int a = 0; a < 3; ++a) {
    g.lo[a] = v->lo[a];
    g.vs[a] = (v->hi[a] - v->lo[a]) / (float)v->dims[a];
  }
  return g;
}

static int tsdf_volume_check(const char* who, const fnr_tsdf_volume* v) {
  FNR_CHECK_ARG(v != nullptr, "%s: null volume", who);
  FNR_CHECK_ARG(v->values && v->weights && v->colors, "%s: null volume array", who);
  for (int a = 0; a < 3; ++a) {
    FNR_CHECK_ARG(v->dims[a] >= 2 && v->dims[a] <= TSDF_MAX_DIM, "%s: dims[%d] = %d outside 2..%d", who, a, v->dims[a],
                  TSDF_MAX_DIM);
    FNR_CHECK_ARG(v->hi[a] > v->lo[a] && v->hi[a] - v->lo[a] < 3.0e38f, "%s: box needs finite lo[%d] < hi[%d]", who, a, a);
  }
  FNR_CHECK_ARG(v->truncation_margin > 0.0f && v->truncation_margin < 3.0e38f, "%s: truncation_margin must be positive", who);
  FNR_CHECK_ARG(v->max_weight >= 1.0f, "%s: max_weight must be >= 1", who);
  return FNR_OK;
}

__device__ __forceinline__ void node_ijk(const TsdfGrid& g, long long n, int& i, int& j, int& k) {
  const long long r = n / g.nz;
  k = (int)(n - r * g.nz);
  i = (int)(r / g.ny);
  j = (int)(r - (long long)i * g.ny);
}
__device__ __forceinline__ long long node_index(const TsdfGrid& g, int i, int j, int k) {
  return ((long long)i * g.ny + j) * g.nz + k;
}
__device__ __forceinline__ float node_coord(const TsdfGrid& g, int axis, int i) {
  return fadd(g.lo[axis], fmul((float)i, g.vs[axis]));
}

// ---- fusion ---------------------------------------------------------------------------------------------------------
// One thread per node, lanes along z: the volume's five floats move coalesced, once per call.  The camera index is the
// same in every lane, so a camera's 16 floats arrive through scalar loads; depth / rgb are gathers whose addresses are
// close for neighbouring lanes (neighbouring nodes project to neighbouring pixels).
__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_integrate(TsdfGrid g, long long nodes, float truncation, float max_weight,
                                                               int depth_kind, int n_cameras,
                                                               const float* __restrict__ c2w,
                                                               const float* __restrict__ intrinsics, int H, int W,
                                                               const float* __restrict__ depth,
                                                               const float* __restrict__ rgb,
                                                               const unsigned char* __restrict__ mask, float* values,
                                                               float* weights, float* colors) {
  const long long n = (long long)blockIdx.x * TSDF_BLOCK + threadIdx.x;
  if (n >= nodes) return;
  int i, j, k;
  node_ijk(g, n, i, j, k);
  const float px = node_coord(g, 0, i), py = node_coord(g, 1, j), pz = node_coord(g, 2, k);
  float val = values[n], w = weights[n];
  float c0 = colors[3 * n], c1 = colors[3 * n + 1], c2 = colors[3 * n + 2];
  bool touched = false;
  const float fW = (float)W, fH = (float)H;
  for (int c = 0; c < n_cameras; ++c) {
    const float* m = c2w + 12 * (size_t)c;
    const float* in = intrinsics + 4 * (size_t)c;
    const float dx = fsub(px, m[3]), dy = fsub(py, m[7]), dz = fsub(pz, m[11]);
    const float qx = fadd(fadd(fmul(m[0], dx), fmul(m[4], dy)), fmul(m[8], dz));
    const float qy = fadd(fadd(fmul(m[1], dx), fmul(m[5], dy)), fmul(m[9], dz));
    const float qz = fadd(fadd(fmul(m[2], dx), fmul(m[6], dy)), fmul(m[10], dz));
    const float z = -qz;
    if (!(z > 0.0f)) continue;
    const float u = fadd(fdiv(fmul(in[0], qx), z), in[2]);
    const float v = fadd(fdiv(fmul(in[1], -qy), z), in[3]);
    const float fc = rintf(fsub(u, 0.5f)), fr = rintf(fsub(v, 0.5f));     // round to nearest even
    if (!(fc >= 0.0f && fc < fW && fr >= 0.0f && fr < fH)) continue;       // also refuses NaN / inf
    const size_t pix = ((size_t)c * H + (int)fr) * W + (int)fc;
    if (mask && mask[pix] == 0) continue;
    const float sd = depth[pix];
    const float vd = depth_kind == FNR_TSDF_DEPTH_RAY
                         ? sqrtf(fadd(fadd(fmul(qx, qx), fmul(qy, qy)), fmul(qz, qz)))
                         : z;
    const float dist = fsub(sd, vd);
    if (!(sd > 0.0f && dist > -truncation)) continue;
    const float s = fminf(1.0f, fmaxf(-1.0f, fdiv(dist, truncation)));
    const float w1 = fadd(w, 1.0f);
    val = fdiv(fadd(fmul(val, w), s), w1);
    c0 = fdiv(fadd(fmul(c0, w), rgb[3 * pix]), w1);
    c1 = fdiv(fadd(fmul(c1, w), rgb[3 * pix + 1]), w1);
    c2 = fdiv(fadd(fmul(c2, w), rgb[3 * pix + 2]), w1);
    w = fminf(w1, max_weight);
    touched = true;
  }
  if (touched) {
    values[n] = val;
    weights[n] = w;
    colors[3 * n] = c0;
    colors[3 * n + 1] = c1;
    colors[3 * n + 2] = c2;
  }
}

// ---- marching tetrahedra: the 16-case table, derived -------------------------------------------------------------------
// An edge of a tetrahedron is stored as (lower corner id << 3) | direction code m; both are subsets of the three axis bits
// (bit 0: x, 1: y, 2: z) and the upper corner is their union.
struct TetTable {
  unsigned char corner[6][4];       // corner ids c0..c3 of tetrahedron t
  unsigned char ntri[6][16];        // case = sum over walk positions p of (corner p inside) << p
  unsigned char edge[6][16][6];     // two triangles x three edges
};

constexpr int tet_axis(int t, int step) {
  constexpr int order[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  return order[t][step];
}

// twice the midpoint of the edge between two corners of the unit cell
constexpr void tet_mid2(int ca, int cb, int (&p)[3]) {
  for (int a = 0; a < 3; ++a) p[a] = ((ca >> a) & 1) + ((cb >> a) & 1);
}

constexpr TetTable make_tet_table() {
  TetTable T{};
  for (int t = 0; t < 6; ++t) {
    int c[4] = {0, 0, 0, 7};
    c[1] = 1 << tet_axis(t, 0);
    c[2] = c[1] | (1 << tet_axis(t, 1));
    for (int p = 0; p < 4; ++p) T.corner[t][p] = (unsigned char)c[p];
    for (int cs = 0; cs < 16; ++cs) {
      int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, nin = 0, nout = 0;
      for (int p = 0; p < 4; ++p) {
        if ((cs >> p) & 1) in[nin++] = p;
        else out[nout++] = p;
      }
      // triangles as pairs of walk positions (the rules of include/fruitnerf_hip.h)
      int tri[2][3][2] = {};
      int ntri = 0;
      if (nin == 1) {
        for (int e = 0; e < 3; ++e) tri[0][e][0] = in[0], tri[0][e][1] = out[e];
        ntri = 1;
      } else if (nin == 3) {
        for (int e = 0; e < 3; ++e) tri[0][e][0] = out[0], tri[0][e][1] = in[e];
        ntri = 1;
      } else if (nin == 2) {
        const int quad[4][2] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
        const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
        for (int q = 0; q < 2; ++q)
          for (int e = 0; e < 3; ++e) tri[q][e][0] = quad[pick[q][e]][0], tri[q][e][1] = quad[pick[q][e]][1];
        ntri = 2;
      }
      // from the inside corners' centroid to the outside corners' (scaled by nin * nout)
      int dir[3] = {0, 0, 0};
      for (int a = 0; a < 3; ++a) {
        for (int p = 0; p < nout; ++p) dir[a] += nin * ((c[out[p]] >> a) & 1);
        for (int p = 0; p < nin; ++p) dir[a] -= nout * ((c[in[p]] >> a) & 1);
      }
      T.ntri[t][cs] = (unsigned char)ntri;
      for (int q = 0; q < ntri; ++q) {
        int P[3][3] = {};
        for (int e = 0; e < 3; ++e) tet_mid2(c[tri[q][e][0]], c[tri[q][e][1]], P[e]);
        int a1[3] = {}, a2[3] = {};
        for (int a = 0; a < 3; ++a) a1[a] = P[1][a] - P[0][a], a2[a] = P[2][a] - P[0][a];
        const int nrm[3] = {a1[1] * a2[2] - a1[2] * a2[1], a1[2] * a2[0] - a1[0] * a2[2], a1[0] * a2[1] - a1[1] * a2[0]};
        const int towards = nrm[0] * dir[0] + nrm[1] * dir[1] + nrm[2] * dir[2];   // never 0: the cell is not degenerate
        for (int e = 0; e < 3; ++e) {
          const int src = towards > 0 ? e : (e == 0 ? 0 : 3 - e);                 // swap the last two to turn it round
          const int ca = c[tri[q][src][0]], cb = c[tri[q][src][1]];
          const int lower = ca < cb ? ca : cb;                                     // corners on a walk are nested bit sets
          T.edge[t][cs][3 * q + e] = (unsigned char)((lower << 3) | (ca ^ cb));
        }
      }
    }
  }
  return T;
}

__constant__ TetTable c_tet = make_tet_table();

// ---- surface extraction -----------------------------------------------------------------------------------------------
// Per node, one 32-bit word: bits 1..7 the active edges it owns (by direction code), bits 8..18 the number of vertices
// owned by earlier nodes of its block, bits 19..31 the number of faces of earlier cells of its block.  With the scanned
// block totals that is every vertex's index and every face's row, for the node's own thread and for the neighbours that
// look its vertices up.
__device__ __forceinline__ unsigned info_mask(unsigned info) { return info & 0xffu; }
__device__ __forceinline__ unsigned info_vertices(unsigned info) { return (info >> 8) & 0x7ffu; }
__device__ __forceinline__ unsigned info_faces(unsigned info) { return info >> 19; }

// inside flags of the corners of the node's cell (bit = corner id); `present`: the corners that lie in the grid
__device__ __forceinline__ unsigned corner_sides(const TsdfGrid& g, const float* __restrict__ values, int i, int j, int k,
                                                 unsigned& present) {
  unsigned inside = 0;
  present = 0;
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int ii = i + (p & 1), jj = j + ((p >> 1) & 1), kk = k + (p >> 2);
    if (ii < g.nx && jj < g.ny && kk < g.nz) {
      present |= 1u << p;
      if (values[node_index(g, ii, jj, kk)] < 0.0f) inside |= 1u << p;
    }
  }
  return inside;
}

__device__ __forceinline__ unsigned tet_case(int t, unsigned inside) {
  unsigned cs = 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) cs |= ((inside >> c_tet.corner[t][p]) & 1u) << p;
  return cs;
}

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_mesh_count(TsdfGrid g, long long nodes,
                                                                const float* __restrict__ values,
                                                                unsigned* __restrict__ info,
                                                                unsigned long long* __restrict__ block_counts,
                                                                long long nblocks) {
  __shared__ unsigned s_wave[TSDF_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long n = (long long)blockIdx.x * TSDF_BLOCK + threadIdx.x;
  unsigned mask = 0, nv = 0, nf = 0;
  if (n < nodes) {
    int i, j, k;
    node_ijk(g, n, i, j, k);
    unsigned present;
    const unsigned inside = corner_sides(g, values, i, j, k, present);
    const unsigned differs = (inside & 1u) ? ~inside : inside;   // corners on the other side than the node
    mask = differs & present & 0xfeu;                            // corner id p of the cell = direction code m of the edge
    nv = __popc(mask);
    if (present == 0xffu && inside != 0u && inside != 0xffu) {
#pragma unroll
      for (int t = 0; t < 6; ++t) nf += c_tet.ntri[t][tet_case(t, inside)];
    }
  }
  // nv <= 7 and nf <= 12 per node: both block sums fit in 16 bits, one scan carries the pair
  const unsigned own = nv | (nf << 16);
  unsigned incl = own;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  unsigned pre = incl - own;
  for (int q = 0; q < wave; ++q) pre += s_wave[q];
  if (n < nodes) info[n] = mask | ((pre & 0xffffu) << 8) | ((pre >> 16) << 19);
  if (threadIdx.x == TSDF_BLOCK - 1) {
    const unsigned total = pre + own;
    block_counts[blockIdx.x] = total & 0xffffu;
    block_counts[nblocks + blockIdx.x] = total >> 16;
  }
}

// block_counts -> exclusive offsets in place, one workgroup per stream (vertices, faces); totals to counts
__global__ __launch_bounds__(1024) void k_tsdf_mesh_scan(unsigned long long* __restrict__ block_counts, long long nblocks,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s_wave[16];
  __shared__ unsigned long long s_carry;
  unsigned long long* bc = block_counts + (size_t)blockIdx.x * nblocks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_carry = 0ull;
  __syncthreads();
  for (long long start = 0; start < nblocks; start += 1024) {
    const long long i = start + threadIdx.x;
    const unsigned long long v = (i < nblocks) ? bc[i] : 0ull;
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned long long wave_off = 0;
    for (int q = 0; q < wave; ++q) wave_off += s_wave[q];
    const unsigned long long carry = s_carry;
    if (i < nblocks) bc[i] = carry + wave_off + incl - v;
    __syncthreads();
    if (threadIdx.x == 1023) s_carry = carry + wave_off + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = s_carry;
}

// central differences in world units, one-sided at the border (every dim >= 2)
__device__ __forceinline__ void node_gradient(const TsdfGrid& g, const float* __restrict__ values, int i, int j, int k,
                                              float (&grad)[3]) {
  const int idx[3] = {i, j, k}, dim[3] = {g.nx, g.ny, g.nz};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    int lo[3] = {i, j, k}, hi[3] = {i, j, k};
    if (idx[a] > 0) lo[a] -= 1;
    if (idx[a] < dim[a] - 1) hi[a] += 1;
    const float span = fmul((float)(hi[a] - lo[a]), g.vs[a]);
    grad[a] = fdiv(fsub(values[node_index(g, hi[0], hi[1], hi[2])], values[node_index(g, lo[0], lo[1], lo[2])]), span);
  }
}

__global__ __launch_bounds__(TSDF_BLOCK) void k_tsdf_mesh_emit(TsdfGrid g, long long nodes,
                                                               const float* __restrict__ values,
                                                               const float* __restrict__ colors,
                                                               const unsigned* __restrict__ info,
                                                               const unsigned long long* __restrict__ block_offsets,
                                                               long long nblocks, long long n_vertices, long long n_faces,
                                                               float* __restrict__ vertices, float* __restrict__ normals,
                                                               float* __restrict__ vcolors, int* __restrict__ faces) {
  const long long n = (long long)blockIdx.x * TSDF_BLOCK + threadIdx.x;
  if (n >= nodes) return;
  const unsigned mine = info[n];
  int i, j, k;
  node_ijk(g, n, i, j, k);
  // ---- the vertices of the edges this node owns, ascending by direction code
  if (info_mask(mine)) {
    long long at = (long long)block_offsets[blockIdx.x] + info_vertices(mine);
    const float va = values[n];
    const float pa[3] = {node_coord(g, 0, i), node_coord(g, 1, j), node_coord(g, 2, k)};
    float ga[3];
    node_gradient(g, values, i, j, k, ga);
    for (int m = 1; m < 8; ++m) {
      if (!((mine >> m) & 1u)) continue;
      const int bi = i + (m & 1), bj = j + ((m >> 1) & 1), bk = k + (m >> 2);
      const long long b = node_index(g, bi, bj, bk);
      const float vb = values[b];
      const float t = fdiv(fsub(0.0f, va), fsub(vb, va));
      const float pb[3] = {node_coord(g, 0, bi), node_coord(g, 1, bj), node_coord(g, 2, bk)};
      float gb[3];
      node_gradient(g, values, bi, bj, bk, gb);
      float nr[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) nr[a] = fadd(ga[a], fmul(t, fsub(gb[a], ga[a])));
      const float len = sqrtf(fadd(fadd(fmul(nr[0], nr[0]), fmul(nr[1], nr[1])), fmul(nr[2], nr[2])));
      const long long src = fabsf(va) <= fabsf(vb) ? n : b;
      if (at < n_vertices) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          vertices[3 * at + a] = fadd(pa[a], fmul(t, fsub(pb[a], pa[a])));
          normals[3 * at + a] = len > 0.0f ? fdiv(nr[a], len) : 0.0f;
          vcolors[3 * at + a] = colors[3 * src + a];
        }
      }
      ++at;
    }
  }
  // ---- the faces of this node's cell, by tetrahedron and triangle
  if (i >= g.nx - 1 || j >= g.ny - 1 || k >= g.nz - 1) return;
  unsigned present;
  const unsigned inside = corner_sides(g, values, i, j, k, present);
  if (inside == 0u || inside == 0xffu) return;
  long long row = (long long)block_offsets[nblocks + blockIdx.x] + info_faces(mine);
  for (int t = 0; t < 6; ++t) {
    const unsigned cs = tet_case(t, inside);
    const int ntri = c_tet.ntri[t][cs];
    for (int e = 0; e < 3 * ntri; ++e) {
      const unsigned code = c_tet.edge[t][cs][e];
      const unsigned lower = code >> 3, m = code & 7u;
      const long long a = node_index(g, i + (lower & 1), j + ((lower >> 1) & 1), k + (lower >> 2));
      const unsigned other = info[a];
      const long long vid = (long long)block_offsets[a / TSDF_BLOCK] + info_vertices(other) +
                            __popc(info_mask(other) & ((1u << m) - 1u));
      const long long r = row + e / 3;
      if (r < n_faces) faces[3 * r + e % 3] = (int)vid;
    }
    row += ntri;
  }
}

}  // namespace fnr

using namespace fnr;

extern "C" int fnr_tsdf_integrate(const fnr_tsdf_volume* volume, int32_t n_cameras, const float* c2w,
                                  const float* intrinsics, int32_t H, int32_t W, const float* depth, const float* rgb,
                                  const uint8_t* mask, int32_t depth_kind, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_tsdf_integrate");
  if (int rc = tsdf_volume_check("tsdf_integrate", volume)) return rc;
  FNR_CHECK_ARG(n_cameras >= 0, "tsdf_integrate: n_cameras < 0");
  FNR_CHECK_ARG(depth_kind == FNR_TSDF_DEPTH_Z || depth_kind == FNR_TSDF_DEPTH_RAY, "tsdf_integrate: depth_kind %d",
                depth_kind);
  FNR_CHECK_ARG(H >= 1 && W >= 1 && H <= 65536 && W <= 65536, "tsdf_integrate: image size %d x %d", H, W);
  if (n_cameras == 0) return FNR_OK;
  FNR_CHECK_ARG(c2w && intrinsics && depth && rgb, "tsdf_integrate: null argument");
  const TsdfGrid g = tsdf_grid(volume);
  const long long nodes = (long long)g.nx * g.ny * g.nz;
  const long long nblocks = (nodes + TSDF_BLOCK - 1) / TSDF_BLOCK;
  const float truncation = volume->truncation_margin * g.vs[0];
  hipStream_t st = as_stream(stream);
  FNR_PROF(OP_EXPORT_COMPACT, nodes * n_cameras);
  hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)nblocks), dim3(TSDF_BLOCK), 0, st, g, nodes, truncation,
                     volume->max_weight, (int)depth_kind, (int)n_cameras, c2w, intrinsics, (int)H, (int)W, depth, rgb,
                     mask, volume->values, volume->weights, volume->colors);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

static int tsdf_mesh_check(const char* who, const fnr_tsdf_volume* volume, const void* workspace, size_t workspace_bytes,
                           long long& nodes) {
  if (int rc = tsdf_volume_check(who, volume)) return rc;
  nodes = (long long)volume->dims[0] * volume->dims[1] * volume->dims[2];
  FNR_CHECK_ARG(workspace != nullptr, "%s: null workspace", who);
  FNR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "%s: workspace is not 8-byte aligned", who);
  FNR_CHECK_ARG(workspace_bytes >= FNR_TSDF_MESH_WORKSPACE_BYTES(nodes), "%s: workspace %zu < %zu bytes", who,
                workspace_bytes, (size_t)FNR_TSDF_MESH_WORKSPACE_BYTES(nodes));
  return FNR_OK;
}

extern "C" int fnr_tsdf_mesh_count(const fnr_tsdf_volume* volume, uint64_t* counts, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_tsdf_mesh_count");
  long long nodes = 0;
  if (int rc = tsdf_mesh_check("tsdf_mesh_count", volume, workspace, workspace_bytes, nodes)) return rc;
  FNR_CHECK_ARG(counts != nullptr, "tsdf_mesh_count: null counts");
  const TsdfGrid g = tsdf_grid(volume);
  const long long nblocks = (nodes + TSDF_BLOCK - 1) / TSDF_BLOCK;
  unsigned long long* bc = reinterpret_cast<unsigned long long*>(workspace);
  unsigned* info = reinterpret_cast<unsigned*>(bc + 2 * nblocks);
  hipStream_t st = as_stream(stream);
  FNR_PROF(OP_EXPORT_COMPACT, nodes);
  hipLaunchKernelGGL(k_tsdf_mesh_count, dim3((unsigned)nblocks), dim3(TSDF_BLOCK), 0, st, g, nodes, volume->values, info,
                     bc, nblocks);
  FNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_tsdf_mesh_scan, dim3(2), dim3(1024), 0, st, bc, nblocks,
                     reinterpret_cast<unsigned long long*>(counts));
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}

extern "C" int fnr_tsdf_mesh_emit(const fnr_tsdf_volume* volume, const void* workspace, size_t workspace_bytes,
                                  int64_t n_vertices, int64_t n_faces, float* vertices, float* normals, float* colors,
                                  int32_t* faces, void* stream) {
  FNR_SEQ_UNRECORDABLE("fnr_tsdf_mesh_emit");
  long long nodes = 0;
  if (int rc = tsdf_mesh_check("tsdf_mesh_emit", volume, workspace, workspace_bytes, nodes)) return rc;
  FNR_CHECK_ARG(n_vertices >= 0 && n_faces >= 0, "tsdf_mesh_emit: n_vertices / n_faces < 0");
  FNR_CHECK_ARG(n_vertices <= 0x7fffffffll, "tsdf_mesh_emit: %lld vertices do not fit int32 face indices",
                (long long)n_vertices);
  FNR_CHECK_ARG(n_vertices == 0 || (vertices && normals && colors), "tsdf_mesh_emit: null vertex array");
  FNR_CHECK_ARG(n_faces == 0 || faces, "tsdf_mesh_emit: null faces");
  if (n_vertices == 0 && n_faces == 0) return FNR_OK;
  const TsdfGrid g = tsdf_grid(volume);
  const long long nblocks = (nodes + TSDF_BLOCK - 1) / TSDF_BLOCK;
  const unsigned long long* bc = reinterpret_cast<const unsigned long long*>(workspace);
  const unsigned* info = reinterpret_cast<const unsigned*>(bc + 2 * nblocks);
  hipStream_t st = as_stream(stream);
  FNR_PROF(OP_EXPORT_COMPACT, nodes);
  hipLaunchKernelGGL(k_tsdf_mesh_emit, dim3((unsigned)nblocks), dim3(TSDF_BLOCK), 0, st, g, nodes, volume->values,
                     volume->colors, info, bc, nblocks, (long long)n_vertices, (long long)n_faces, vertices, normals,
                     colors, faces);
  FNR_LAUNCH_CHECK();
  return FNR_OK;
}
