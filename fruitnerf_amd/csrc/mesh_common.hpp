// mesh_common.hpp — what mesh.hip (connectivity) and mesh_filters.hip (filters) share: the block size, the error word, the
// one-workgroup exclusive scan, and the host-side argument checks.
#pragma once
#include "common.hpp"

namespace fnr {

constexpr int MESH_BLOCK = 256;
constexpr int SCAN_THREADS = 1024, SCAN_ITEMS = 8;

__device__ __forceinline__ void mesh_error(unsigned long long* header, unsigned bit) {
  atomicOr(reinterpret_cast<unsigned*>(header), bit);
}

// ---- exclusive scan of n 32-bit counts by ONE workgroup (every total here is below 2^31) -----------------------------
// MARK: the input is 0 / 1 flags and the output is "index + 1" for a set flag, 0 for a clear one.  in == out is allowed.
template <bool MARK>
__global__ __launch_bounds__(SCAN_THREADS) void k_mesh_scan(const unsigned* in, unsigned* out, long long n,
                                                            unsigned long long* total_a, unsigned long long* total_b) {
  __shared__ unsigned s_wave[SCAN_THREADS / 64];
  __shared__ unsigned s_carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_carry = 0u;
  __syncthreads();
  for (long long start = 0; start < n; start += (long long)SCAN_THREADS * SCAN_ITEMS) {
    const long long base = start + (long long)threadIdx.x * SCAN_ITEMS;
    unsigned v[SCAN_ITEMS], sum = 0u;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
      v[k] = (base + k < n) ? in[base + k] : 0u;
      sum += v[k];
    }
    unsigned incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned wave_off = 0u;
    for (int q = 0; q < wave; ++q) wave_off += s_wave[q];
    const unsigned carry = s_carry;
    unsigned run = carry + wave_off + incl - sum;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
      if (base + k < n) out[base + k] = MARK ? (v[k] ? run + 1u : 0u) : run;
      run += v[k];
    }
    __syncthreads();
    if (threadIdx.x == SCAN_THREADS - 1) s_carry = carry + wave_off + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (total_a) *total_a = s_carry;
    if (total_b) *total_b = s_carry;
  }
}

static inline unsigned grid_for(long long n) { return (unsigned)((n + MESH_BLOCK - 1) / MESH_BLOCK); }

static int mesh_sizes_check(const char* who, int64_t n_vertices, int64_t n_faces) {
  FNR_CHECK_ARG(n_vertices >= 0 && n_faces >= 0, "%s: n_vertices / n_faces < 0", who);
  FNR_CHECK_ARG(n_vertices <= 0x7fffffffll && n_faces <= 0x7fffffffll, "%s: more than 2^31 - 1 vertices or faces", who);
  return FNR_OK;
}

static int mesh_workspace_check(const char* who, const void* workspace, size_t workspace_bytes, size_t needed) {
  FNR_CHECK_ARG(workspace != nullptr, "%s: null workspace", who);
  FNR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0, "%s: workspace is not 16-byte aligned", who);
  FNR_CHECK_ARG(workspace_bytes >= needed, "%s: workspace %zu < %zu bytes", who, workspace_bytes, needed);
  return FNR_OK;
}

}  // namespace fnr
