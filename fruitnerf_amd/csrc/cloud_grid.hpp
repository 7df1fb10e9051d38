// cloud_grid.hpp — what the point-cloud translation units share: the sorted-by-cell-key search structure of cloud.hip
// (workspace layout, key sort, gather into sorted order; defined there) and the device helpers its sweeps and the kNN
// search of cloud_knn.hip both use.
#pragma once
#include "common.hpp"

namespace fnr {

typedef unsigned long long u64;

// one sorted point: position + what the sweeps need to know about it as a CANDIDATE, so that a candidate is one 32-byte
// scalar load (input index and core flag ride in what would be padding)
struct alignas(32) CloudPoint {
  double x, y, z;
  int index;   // input index (order[s])
  int core;    // DBSCAN core flag, filled in after the count pass
};

struct CloudGrid {
  double lo[3];
  double cell;
  long long dim[3];
};

struct CloudWs {
  u64* keys_a;
  u64* keys;      // sorted
  int* idx_a;
  int* order;     // sorted position -> input index
  CloudPoint* sxyz;  // [n] points in sorted order
  int* aux0;      // per sorted position: core flag / head flag
  int* aux1;      // per input index: union-find parent
  int* aux2;      // per input index: core flag, then root flag
  int* aux3;      // scan output
  int* cell_first;  // [n_cells + 1] first sorted position of every occupied cell
  int* ctrl;      // [0] n_cells, [1..7] work counters of the cell sweeps
  void* temp;
  size_t temp_bytes;
};

// ---- host side (cloud.hip) -----------------------------------------------------------------------------------------
// carves fnr_cloud_workspace_bytes(n) bytes; false when `ws` is null or too short
bool carve_cloud(void* ws, size_t bytes, int64_t n, CloudWs* out);
// (keys_a, idx_a) -> (keys, order), stable, on the low `bits` key bits
int sort_by_key(const CloudWs& w, int n, int bits, hipStream_t st);
// sxyz[s] = point order[s] with its input index
int gather_sorted(const double* xyz, const CloudWs& w, int n, hipStream_t st);

// ---- device helpers ------------------------------------------------------------------------------------------------
__device__ inline int lower_bound_key(const u64* __restrict__ keys, int lo, int hi, u64 k) {
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ inline int upper_bound_key(const u64* __restrict__ keys, int lo, int hi, u64 k) {
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (keys[mid] <= k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// squared distance in the CPU libraries' operation order: ((dx*dx) + dy*dy) + dz*dz, every op rounded
__device__ inline double pair_d2(const CloudPoint& p, const CloudPoint& q) {
  const double dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ inline int wave_lane() { return (int)(threadIdx.x & 63u); }

}  // namespace fnr
