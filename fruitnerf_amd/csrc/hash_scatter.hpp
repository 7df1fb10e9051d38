// hash_scatter.hpp — the binned scatter of hash_scatter.hip as the proposal networks' backward (prop_bwd.hip) uses it.
// Plain host functions: every scatter kernel is instantiated in hash_scatter.hip and nowhere else.
#pragma once
#include "adam.hpp"
#include "hash_sources.hpp"

namespace fnr {

// (TableAdam / table_adam_update: adam.hpp — the optimiser step fused into the accumulate kernel)
// everything one accumulate launch needs about one scatter call (a launch can serve two calls: k_scatter_accumulate2)
struct AccArgs {
  GridDev grid;
  const float2* queue_v;
  const unsigned short* queue_r;
  unsigned *qcount, *qmax, *qdone;
  long long cap;
  int log2_rows, level0, nbins;   // nbins = level_count * bins per level = workgroups of this call
  int kind;                       // 0: the field's table, 1: a proposal network's (g_scatter_records)
  TableAdam adam;
};

#pragma GCC visibility push(hidden)   // (between the library's own files only)
// emit of one scatter call -> the arguments its accumulate launch needs
int scatter_emit(const fnr_grid* grid_grad, const Warp& warp, const RaySource& src, long long N, const float2* d_feats,
                 int level0, int level_count, void* workspace, size_t workspace_bytes, int workspace_clean, hipStream_t st,
                 const TableAdam* adam, AccArgs& acc);
int scatter_accumulate(const AccArgs& a, bool adam, hipStream_t st);
// the accumulate launches of two scatter calls as one (a's queues are the longer ones)
int scatter_accumulate2(const AccArgs& a, const AccArgs& b, bool adam, hipStream_t st);
#pragma GCC visibility pop

}  // namespace fnr
