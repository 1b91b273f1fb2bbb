// Tracking evaluation (Waymo-protocol CLEAR MOT counts) on the device: DESIGN.md "Tracking evaluation".
//
// Pair weights come from det_eval.hip's pair_weight_kernel (tracks stand where predictions do): the same frame-segmented
// P_f x G_f blocks.  Two kernels here:
//
//   * mot_kernel: one workgroup per (problem, cutoff).  A problem is one class of one segment, a segment a run of
//     consecutive frames of one sequence; the workgroup walks the frames in order and carries the CLEAR MOT state, the
//     map last[g] = track that ground truth g was most recently matched to, in row `cutoff` of a global table indexed by
//     the ground truth's dense id (-1 = never matched).  Only this workgroup touches that row at the ids of its class, so
//     no two workgroups share an entry; the table is input and output, so a sequence can be evaluated in chunks.
//     Per frame:
//       - the tracks of a class are sorted by descending score, so those in play (score >= cutoff) are a prefix; its
//         length is a block-wide count;
//       - carry-over: one ground-truth column per thread.  The column looks its last track up among the rows in play (a
//         counted scan of their ids in LDS); if the pair's weight is a finite positive number it claims the row by an
//         LDS atomicMin of its column index.  Columns stand in dense-id order, so the lowest dense id wins, every run;
//       - residual assignment: the rows that were not claimed are inserted one at a time by the shortest augmenting
//         path of row_insert.h, over the columns that kept nothing (the others are switched off);
//       - counts (match, fp, miss, mismatch, gt at both levels; 1 - w of the matches rounded to a multiple of 2^-30, so
//         that fp64 sums are exact in any order) are reduced over the block and added to the workgroup's running row;
//       - last[g] = track, for every pair.
//     Every loop is counted: frames of the segment, rows in play (<= 1024), search steps (<= G + 1), rows scanned for an
//     id.  No value of the input steers a trip count.
//
//   * accumulate_kernel: adds the per-problem rows to the running totals in problem order, no atomics.
#include "common.h"
#include "row_insert.h"

#include <limits.h>
#include <math.h>

namespace efg {
namespace {

constexpr int kMaxCutoffs = 101;
constexpr int kNumCounts = 9;   // match1, match2, fp, miss1, miss2, mismatch1, mismatch2, gt1, gt2
constexpr int kNumSums = 2;     // cost1, cost2
constexpr int kProbFields = 3;  // first frame, end frame, class
constexpr int kRangeFields = 4; // first track, tracks, first ground truth, ground truths  (per frame and class)

__global__ __launch_bounds__(kEvalThreads) void mot_kernel(
    const float* __restrict__ weights, const int64_t* __restrict__ blk_off, const int* __restrict__ trk_off,
    const int* __restrict__ gt_off, const int* __restrict__ ranges, const int* __restrict__ prob, int n_frames,
    const float* __restrict__ scores, const int* __restrict__ track_ids, const int* __restrict__ gt_ids,
    const int* __restrict__ gt_level, const float* __restrict__ cutoffs, int n_cutoffs, int* last, int capacity,
    int* __restrict__ counts, double* __restrict__ sums) {
  __shared__ RowInsertLds lds;  // row_insert.h
  __shared__ int s_tid[kMaxPred];    // ids of the tracks in play
  __shared__ int s_claim[kMaxPred];  // the column that keeps the row, INT_MAX if none
  __shared__ double red_d[kEvalThreads / 64][kNumSums];
  __shared__ int red_i[kEvalThreads / 64][kNumCounts + 1];

  const int p = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const int f0 = max(prob[p * kProbFields], 0), f1 = min(prob[p * kProbFields + 1], n_frames);
  const int cls = min(max(prob[p * kProbFields + 2], 0), 2);
  const float cut = cutoffs[k];
  int* last_k = last + (int64_t)k * capacity;

  int64_t tot_i[kNumCounts];
  double tot_d[kNumSums] = {0.0, 0.0};
#pragma unroll
  for (int t = 0; t < kNumCounts; ++t) tot_i[t] = 0;

  for (int f = f0; f < f1; ++f) {
    const int* rg = ranges + ((int64_t)f * 3 + cls) * kRangeFields;
    const int r0 = rg[0], g0 = rg[2];
    const int np = min(max(rg[1], 0), kMaxPred), ng = min(max(rg[3], 0), kMaxGt);  // the host refuses larger problems
    const int gf = gt_off[f + 1] - gt_off[f];                                       // row stride of the frame's block
    const float* w = weights + blk_off[f] + (int64_t)(r0 - trk_off[f]) * gf + (g0 - gt_off[f]);

    // tracks in play: a prefix of the sorted scores (NaN and -inf fail the comparison)
    int mine = 0;
    for (int r = tid; r < np; r += kEvalThreads) mine += scores[r0 + r] >= cut ? 1 : 0;
    mine = wave_reduce_sum(mine);
    if ((tid & 63) == 0) red_i[tid >> 6][kNumCounts] = mine;
    __syncthreads();
    int n = 0;
#pragma unroll
    for (int wv = 0; wv < kEvalThreads / 64; ++wv) n += red_i[wv][kNumCounts];
    for (int r = tid; r < n; r += kEvalThreads) {
      s_tid[r] = track_ids[r0 + r];
      s_claim[r] = INT_MAX;
    }
    const bool col = tid < ng;
    int gid = -1, prev = -1, lv = 0;
    if (col) {
      lds.v[tid] = 0.0;
      lds.row4col[tid] = -1;
      gid = gt_ids[g0 + tid];
      lv = gt_level[g0 + tid];
      if (gid >= 0 && gid < capacity) prev = last_k[gid];
    }
    __syncthreads();

    // carry-over: the row of the column's last track, if that track is in play and the pair is an edge
    int keep_row = -1;
    if (col && prev >= 0) {
      for (int r = 0; r < n; ++r)
        if (s_tid[r] == prev) keep_row = r;  // ids are unique within a frame
      if (keep_row >= 0) {
        const float wt = w[(int64_t)keep_row * gf + tid];
        if (wt > 0.0f && wt < INFINITY) atomicMin(&s_claim[keep_row], tid);
        else keep_row = -1;
      }
    }
    __syncthreads();
    const bool kept = keep_row >= 0 && s_claim[keep_row] == tid;
    if (kept) lds.row4col[tid] = keep_row;
    __syncthreads();

    // residual assignment: the rows nobody kept, over the columns that kept nothing
    const bool col_on = col && !kept;
    for (int cur = 0; cur < n; ++cur) {
      if (s_claim[cur] != INT_MAX) continue;  // block-uniform
      insert_row(lds, w, gf, ng, col_on, cur, tid);
    }

    int c[kNumCounts] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double s[kNumSums] = {0.0, 0.0};
    int matched = 0;
    if (col) {
      const int r = lds.row4col[tid];
      c[7] = lv <= 1;
      c[8] = lv <= 2;
      if (r >= 0) {
        matched = 1;
        const int t = s_tid[r];
        const double cost = rint((1.0 - (double)w[(int64_t)r * gf + tid]) * 1073741824.0) / 1073741824.0;
        const int sw = (!kept && prev >= 0 && prev != t) ? 1 : 0;
        if (lv <= 1) c[0] = 1, c[5] = sw, s[0] = cost;
        if (lv <= 2) c[1] = 1, c[6] = sw, s[1] = cost;
        if (gid >= 0 && gid < capacity) last_k[gid] = t;
      } else {
        c[3] = lv <= 1;
        c[4] = lv <= 2;
      }
    }
    c[2] = matched;  // turned into the tracks in no pair below
#pragma unroll
    for (int t = 0; t < kNumCounts; ++t) c[t] = wave_reduce_sum(c[t]);
#pragma unroll
    for (int t = 0; t < kNumSums; ++t) {
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) s[t] += __shfl_xor(s[t], d, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
      for (int t = 0; t < kNumCounts; ++t) red_i[tid >> 6][t] = c[t];
#pragma unroll
      for (int t = 0; t < kNumSums; ++t) red_d[tid >> 6][t] = s[t];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kNumCounts; ++t) {
      int v = 0;
      for (int wv = 0; wv < kEvalThreads / 64; ++wv) v += red_i[wv][t];
      tot_i[t] += t == 2 ? n - v : v;
    }
#pragma unroll
    for (int t = 0; t < kNumSums; ++t) {
      double v = 0.0;
      for (int wv = 0; wv < kEvalThreads / 64; ++wv) v += red_d[wv][t];  // multiples of 2^-30: exact in any order
      tot_d[t] += v;
    }
    __syncthreads();  // the reduction buffers and this frame's writes to `last` are done before the next frame reads
  }

  if (tid == 0) {
    int* out_i = counts + ((int64_t)p * n_cutoffs + k) * kNumCounts;
    double* out_d = sums + ((int64_t)p * n_cutoffs + k) * kNumSums;
#pragma unroll
    for (int t = 0; t < kNumCounts; ++t) out_i[t] = (int)tot_i[t];
#pragma unroll
    for (int t = 0; t < kNumSums; ++t) out_d[t] = tot_d[t];
  }
}

__global__ void accumulate_kernel(const int* __restrict__ counts, const double* __restrict__ sums,
                                  const int* __restrict__ prob, int n_prob, int n_cutoffs,
                                  int64_t* __restrict__ total_counts, double* __restrict__ total_sums) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;  // (class, cutoff)
  if (slot >= 3 * n_cutoffs) return;
  const int cls = slot / n_cutoffs, k = slot % n_cutoffs;
  int64_t c[kNumCounts];
  double s[kNumSums];
  for (int t = 0; t < kNumCounts; ++t) c[t] = total_counts[slot * kNumCounts + t];
  for (int t = 0; t < kNumSums; ++t) s[t] = total_sums[slot * kNumSums + t];
  for (int p = 0; p < n_prob; ++p) {  // problem order: the one order every call uses
    if (prob[(int64_t)p * kProbFields + 2] != cls) continue;
    for (int t = 0; t < kNumCounts; ++t) c[t] += counts[((int64_t)p * n_cutoffs + k) * kNumCounts + t];
    for (int t = 0; t < kNumSums; ++t) s[t] += sums[((int64_t)p * n_cutoffs + k) * kNumSums + t];
  }
  for (int t = 0; t < kNumCounts; ++t) total_counts[slot * kNumCounts + t] = c[t];
  for (int t = 0; t < kNumSums; ++t) total_sums[slot * kNumSums + t] = s[t];
}

}  // namespace
}  // namespace efg

using namespace efg;

extern "C" int efg_track_eval_mot_f32(const float* weights, const int64_t* blk_off, const int32_t* trk_off,
                                      const int32_t* gt_off, const int32_t* ranges, const int32_t* problems,
                                      int n_problems, int n_frames, int max_tracks, int max_gt, const float* scores,
                                      const int32_t* track_ids, const int32_t* gt_ids, const int32_t* gt_level,
                                      const float* cutoffs, int n_cutoffs, int32_t* last, int capacity, int32_t* counts,
                                      double* sums, void* stream) {
  EFG_CHECK_ARG(n_problems >= 0 && n_frames >= 0 && max_tracks >= 0 && max_gt >= 0 && capacity >= 0,
                "efg_track_eval_mot_f32: negative size (%d, %d, %d, %d, %d)", n_problems, n_frames, max_tracks, max_gt,
                capacity);
  EFG_CHECK_ARG(max_tracks <= kMaxPred,
                "efg_track_eval_mot_f32: %d tracks of one class in one frame exceed the limit of %d", max_tracks, kMaxPred);
  EFG_CHECK_ARG(max_gt <= kMaxGt,
                "efg_track_eval_mot_f32: %d ground truths of one class in one frame exceed the limit of %d", max_gt, kMaxGt);
  EFG_CHECK_ARG(n_cutoffs >= 1 && n_cutoffs <= kMaxCutoffs, "efg_track_eval_mot_f32: %d score cutoffs (1 to %d)",
                n_cutoffs, kMaxCutoffs);
  if (n_problems == 0) return EFG_OK;
  EFG_CHECK_ARG(blk_off && trk_off && gt_off && ranges && problems && cutoffs && counts && sums && (last || capacity == 0),
                "efg_track_eval_mot_f32: null pointer");
  hipLaunchKernelGGL(mot_kernel, dim3((unsigned)n_problems, (unsigned)n_cutoffs), dim3(kEvalThreads), 0,
                     (hipStream_t)stream, weights, blk_off, trk_off, gt_off, ranges, problems, n_frames, scores, track_ids,
                     gt_ids, gt_level, cutoffs, n_cutoffs, last, capacity, counts, sums);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

extern "C" int efg_track_eval_accumulate(const int32_t* counts, const double* sums, const int32_t* problems,
                                         int n_problems, int n_cutoffs, int64_t* total_counts, double* total_sums,
                                         void* stream) {
  EFG_CHECK_ARG(n_problems >= 0, "efg_track_eval_accumulate: negative problem count %d", n_problems);
  EFG_CHECK_ARG(n_cutoffs >= 1 && n_cutoffs <= kMaxCutoffs, "efg_track_eval_accumulate: %d score cutoffs (1 to %d)",
                n_cutoffs, kMaxCutoffs);
  if (n_problems == 0) return EFG_OK;
  EFG_CHECK_ARG(counts && sums && problems && total_counts && total_sums, "efg_track_eval_accumulate: null pointer");
  hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)ceil_div(3 * n_cutoffs, 64)), dim3(64), 0, (hipStream_t)stream,
                     counts, sums, problems, n_problems, n_cutoffs, total_counts, total_sums);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}
