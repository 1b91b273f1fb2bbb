// Shortest-augmenting-path row insertion on costs -w, shared by the detection evaluator's prefix_assign_kernel
// (det_eval.hip) and the tracking evaluator's mot_kernel (track_eval.hip): one source, so the two match alike.
//
// A workgroup of kEvalThreads threads owns one assignment problem of at most kMaxPred rows and kMaxGt columns, one column
// per thread.  `insert_row` inserts row `cur` into the assignment of the rows inserted before it, after which the
// assignment is optimal for all of them (the Hungarian / Jonker-Volgenant row insertion that matcher.hip and scipy run):
//   - every row has a zero-weight column of its own ("unmatched").  It is adjacent to that row only, so it never enters
//     the search tree once assigned, its dual stays 0, and all that is kept of those columns is the best one seen in the
//     current search (dval / drow): a row of the tree at path cost d may leave to its own column at cost d - u[row].
//   - pairs of weight 0 are no edges.  A search ends at a free column or at an own column; each step before that visits a
//     new column, so an insertion takes at most n_col + 1 steps: the step loop is a counted loop, and a value that is not a
//     finite positive weight is no edge, so no input steers it.
//   - duals are fp64 sums and differences of fp32 weights in [0.5, 1]: exact.
// Column state and duals live in LDS (32 B per column, 16 B per row), weights are read from global memory (a row is one
// coalesced read), the column scan is one column per thread with a block-wide argmin: two barriers per step.
#pragma once
#include "common.h"

#include <math.h>

namespace efg {

constexpr int kEvalThreads = 256;
constexpr int kMaxPred = 1024;  // rows (predictions / tracks of one class in one frame)
constexpr int kMaxGt = 256;     // columns (ground truths of one class in one frame) == kEvalThreads: one column per thread
static_assert(kMaxGt == kEvalThreads, "one column per thread");

struct Cand {
  double val;
  int key;  // (assigned ? 1 << 30 : 0) + column: smaller wins, so a free column ends the search before a longer path
};

__device__ __forceinline__ bool better(const Cand& a, const Cand& b) {
  return a.val < b.val || (a.val == b.val && a.key < b.key);
}

__device__ __forceinline__ Cand wave_min(Cand c) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    Cand o;
    o.val = __shfl_xor(c.val, d, 64);
    o.key = __shfl_xor(c.key, d, 64);
    if (better(o, c)) c = o;
  }
  return c;
}

struct RowInsertLds {
  double u[kMaxPred];   // row duals
  double spc[kMaxGt];   // shortest path cost of the current search
  double v[kMaxGt];     // column duals
  int col4row[kMaxPred];
  int sr[kMaxGt + 1];   // rows of the current search tree
  int path[kMaxGt], row4col[kMaxGt], vis[kMaxGt];
  Cand wave_best[kEvalThreads / 64];
  int i, sink, done, nsr, drow;
  double min_val, dval;
};

// Insert row `cur`.  w: the problem's weights, row stride gf; ng columns, of which this thread's (column tid) takes part iff
// `col_on` (tid < ng, and whatever else the caller asks of a column).  Called by every thread of the workgroup; the
// caller has set v = 0 and row4col = -1 for its columns, with a barrier, before the first insertion.  Ends with a barrier.
__device__ __forceinline__ void insert_row(RowInsertLds& s, const float* __restrict__ w, int gf, int ng, bool col_on,
                                           int cur, int tid) {
  if (col_on) {
    s.spc[tid] = INFINITY;
    s.vis[tid] = 0;
  }
  if (tid == 0) {
    s.i = cur;
    s.sink = -1;
    s.done = 0;
    s.nsr = 0;
    s.min_val = 0.0;
    s.dval = INFINITY;
    s.drow = cur;
    s.u[cur] = 0.0;
    s.col4row[cur] = -1;
  }
  __syncthreads();

  // every step that does not end the search visits a new column: at most ng + 1 steps
  for (int step = 0; step <= ng; ++step) {
    const int i = s.i;
    const double min_val = s.min_val, ui = s.u[i];
    Cand best{INFINITY, 0x7fffffff};
    if (col_on && !s.vis[tid]) {
      const float wt = w[(int64_t)i * gf + tid];
      double c = s.spc[tid];
      if (wt > 0.0f && wt < INFINITY) {  // anything else is no edge
        const double r = min_val - (double)wt - ui - s.v[tid];
        if (r < c) {
          s.path[tid] = i;
          s.spc[tid] = c = r;
        }
      }
      if (c < INFINITY) best = Cand{c, (s.row4col[tid] >= 0 ? (1 << 30) : 0) + tid};
    }
    best = wave_min(best);
    if ((tid & 63) == 0) s.wave_best[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
      Cand b = s.wave_best[0];
#pragma unroll
      for (int wv = 1; wv < kEvalThreads / 64; ++wv)
        if (better(s.wave_best[wv], b)) b = s.wave_best[wv];
      s.sr[s.nsr++] = i;
      const double dv = min_val - ui;  // row i may leave to its own zero-weight column
      if (dv < s.dval) {
        s.dval = dv;
        s.drow = i;
      }
      if (b.val < s.dval) {  // false for NaN: the search then ends at an own column
        const int j = b.key & ((1 << 30) - 1);
        s.min_val = b.val;
        s.vis[j] = 1;
        if (s.row4col[j] < 0) {
          s.sink = j;
          s.done = 1;
        } else {
          s.i = s.row4col[j];
        }
      } else {
        s.min_val = s.dval;
        s.sink = -1;
        s.done = 1;
      }
    }
    __syncthreads();
    if (s.done) break;
  }

  if (s.done) {  // always, by the step count above
    const double min_val = s.min_val;
    const int nsr = s.nsr;
    for (int t = tid; t < nsr; t += kEvalThreads) {
      const int r = s.sr[t], cj = s.col4row[r];  // every tree row but `cur` was reached through its column
      s.u[r] += (r == cur || cj < 0) ? min_val : min_val - s.spc[cj];
    }
    __syncthreads();  // u reads col4row / spc before they change below
    if (col_on && s.vis[tid]) s.v[tid] -= min_val - s.spc[tid];
    if (tid == 0) {  // augment along the path, from the sink back to the inserted row
      int j = s.sink, r = j >= 0 ? s.path[j] : s.drow;
      for (int t = 0; t <= ng; ++t) {
        const int old = s.col4row[r];
        s.col4row[r] = j;
        if (j >= 0) s.row4col[j] = r;
        if (r == cur || old < 0) break;
        j = old;
        r = s.path[j];
      }
    }
  }
  __syncthreads();
}

}  // namespace efg
