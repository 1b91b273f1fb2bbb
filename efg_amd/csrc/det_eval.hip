// Detection evaluation (Waymo-protocol AP / APH counts) on the device: DESIGN.md "Detection evaluation".
//
// Three kernels, one launch each per `process` call of the evaluator:
//
//   * pair_weight_kernel: frame-segmented (CSR) pair weights.  Frame f owns a dense P_f x G_f block; a weight is the 3-D
//     IoU of iou3d_nms.hip (pair_value mode 2 of iou3d_pair.h: the same fp32 operations, so the same bits as
//     boxes_iou3d_gpu) where the labels agree and the IoU reaches the class threshold, and exactly 0 elsewhere.  Same
//     launch structure as boxes_pair_kernel: exact far-apart reject, candidate queue, clipper on full waves.  Boxes of
//     different frames never meet (they share coordinates), so no sum(P) x sum(G) matrix exists.
//
//   * prefix_assign_kernel: one workgroup per (frame, class).  The score cutoffs of the protocol select PREFIXES of the
//     score-sorted predictions, so one incremental solve replaces one optimal assignment per cutoff: rows are inserted
//     one at a time by a shortest augmenting path (the Hungarian / Jonker-Volgenant row insertion that matcher.hip and
//     scipy run, here on costs -w), after which the assignment is optimal for the rows inserted so far; whenever the
//     prefix length passes a cutoff boundary the counts of that cutoff are written.
//     The insertion itself (own zero-weight columns, weight-0 pairs as non-edges, the counted step loop, fp64 duals in
//     LDS, one column per thread with a block-wide argmin) is row_insert.h, shared with track_eval.hip.
//
//   * accumulate_kernel: adds the per-problem tables to the running totals in problem order (one thread per (class,
//     cutoff) slot walks the problems): integers as int64, heading accuracy in fp64.  Heading accuracy of a pair is
//     rounded to a multiple of 2^-30, so that fp64 sums of up to 2^23 of them are exact and the totals do not depend on
//     how frames were grouped into calls or ranks.
#include "common.h"
#include "iou3d_pair.h"
#include "row_insert.h"

#include <math.h>

namespace efg {
namespace {

constexpr int kCutoffs = 101;
constexpr int kNumCounts = 5;   // tp1, tp2, fp, fn1, fn2
constexpr int kNumSums = 3;     // ha1, ha2, matched weight
constexpr int kProbFields = 6;  // frame, first prediction, predictions, first ground truth, ground truths, class

__global__ __launch_bounds__(kPairThreads) void pair_weight_kernel(
    const float* __restrict__ pred_boxes, const int* __restrict__ pred_labels, const int* __restrict__ pred_off,
    const float* __restrict__ gt_boxes, const int* __restrict__ gt_labels, const int* __restrict__ gt_off,
    const int64_t* __restrict__ blk_off, float thr1, float thr2, float thr3, float* __restrict__ weights) {
  __shared__ float pts[3 * kMaxPts * kPairThreads];
  __shared__ int q_rows[kQueueCap], q_cols[kQueueCap];
  const int f = blockIdx.z;
  const int p0 = pred_off[f], na = pred_off[f + 1] - p0;
  const int g0 = gt_off[f], nb = gt_off[f + 1] - g0;
  const int i0 = blockIdx.y * kRowsPerBlock;
  if ((int)(blockIdx.x * kPairThreads) >= nb || i0 >= na) return;  // block-uniform
  const float* boxes_a = pred_boxes + (int64_t)p0 * 7;
  const float* boxes_b = gt_boxes + (int64_t)g0 * 7;
  const int* la = pred_labels + p0;
  float* out = weights + blk_off[f];

  float* px = pts + threadIdx.x;
  float* py = px + kMaxPts * kPairThreads;
  float* pa = py + kMaxPts * kPairThreads;
  PairQueue q{q_rows, q_cols, 0};
  const int j = blockIdx.x * kPairThreads + threadIdx.x;
  const int jc = j < nb ? j : nb - 1;
  const float bx = boxes_b[(int64_t)jc * 7 + 0], by = boxes_b[(int64_t)jc * 7 + 1];
  const float bw = boxes_b[(int64_t)jc * 7 + 3], bh = boxes_b[(int64_t)jc * 7 + 4];
  const float rb = 0.5f * sqrtf(bw * bw + bh * bh);
  const int lb = gt_labels[g0 + jc];

  auto drain = [&]() __attribute__((always_inline)) {
    int i, c;
    if (q.pop(&i, &c)) {
      float a[7], b[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        a[k] = boxes_a[(int64_t)i * 7 + k];
        b[k] = boxes_b[(int64_t)c * 7 + k];
      }
      const float v = pair_value(a, b, 2, px, py, pa);
      const int l = la[i];
      const float t1 = thr1, t2 = thr2, t3 = thr3;  // loaded before the select: a select of captured references keeps the closure in scratch
      const float thr = l == 1 ? t1 : l == 2 ? t2 : t3;
      out[(int64_t)i * nb + c] = (v >= thr && v < INFINITY) ? v : 0.0f;  // NaN fails v >= thr
    }
  };

  const int rows = min(na - i0, kRowsPerBlock);
  for (int r = 0; r < rows; ++r) {
    const int i = i0 + r;
    const float ax = boxes_a[(int64_t)i * 7 + 0], ay = boxes_a[(int64_t)i * 7 + 1];
    const float aw = boxes_a[(int64_t)i * 7 + 3], ah = boxes_a[(int64_t)i * 7 + 4];
    const float ra = 0.5f * sqrtf(aw * aw + ah * ah);
    const float dx = ax - bx, dy = ay - by, rr = ra + rb + 0.05f;  // == far_apart(a, b)
    const bool far = dx * dx + dy * dy > rr * rr;
    const int l = la[i];
    const bool cand = j < nb && !far && l == lb && l >= 1 && l <= 3;
    if (j < nb && !cand) out[(int64_t)i * nb + j] = 0.0f;
    if (q.push(cand, i, j)) drain();
  }
  if (q.n > 0) drain();
}

__device__ __forceinline__ double wave_sum(double v) {  // xor butterfly: every lane ends with the same bits
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__device__ __forceinline__ float cutoff(int k) { return k >= 100 ? 1.0f : (float)(0.01 * (double)k); }

// the last cutoff a score is in play at: max k with score >= cutoff(k); -1 if none (score < 0 or NaN)
__device__ __forceinline__ int last_cutoff(float s) {
  int k = -1;
  for (int t = 0; t < kCutoffs; ++t)
    if (s >= cutoff(t)) k = t;
  return k;
}

__device__ __forceinline__ double heading_accuracy(float yaw_a, float yaw_b) {
  const double two_pi = 6.283185307179586, pi = 3.141592653589793;
  const double m = fmod(fabs((double)yaw_a - (double)yaw_b), two_pi);
  const double acc = 1.0 - fmin(m, two_pi - m) / pi;
  return acc > 0.0 ? rint(acc * 1073741824.0) / 1073741824.0 : 0.0;  // NaN -> 0
}

__global__ __launch_bounds__(kEvalThreads) void prefix_assign_kernel(
    const float* __restrict__ weights, const int64_t* __restrict__ blk_off, const int* __restrict__ pred_off,
    const int* __restrict__ gt_off, const int* __restrict__ prob, const float* __restrict__ scores,
    const float* __restrict__ pred_boxes, const float* __restrict__ gt_boxes, const int* __restrict__ gt_level,
    int* __restrict__ counts, double* __restrict__ sums) {
  __shared__ RowInsertLds lds;  // row_insert.h
  __shared__ double red_d[kEvalThreads / 64][kNumSums];
  __shared__ int red_i[kEvalThreads / 64][kNumCounts];

  const int p = blockIdx.x, tid = threadIdx.x;
  const int* d = prob + (int64_t)p * kProbFields;
  const int f = d[0], r0 = d[1], g0 = d[3];
  const int np = min(max(d[2], 0), kMaxPred), ng = min(max(d[4], 0), kMaxGt);  // the host refuses larger problems
  const int gf = gt_off[f + 1] - gt_off[f];                                     // row stride of the frame's block
  const float* w = weights + blk_off[f] + (int64_t)(r0 - pred_off[f]) * gf + (g0 - gt_off[f]);
  int* out_i = counts + (int64_t)p * kCutoffs * kNumCounts;
  double* out_d = sums + (int64_t)p * kCutoffs * kNumSums;

  if (tid < ng) {
    lds.v[tid] = 0.0;
    lds.row4col[tid] = -1;
  }
  __syncthreads();

  // counts of the current assignment with `len` predictions in play, written to the cutoffs klo..khi
  auto emit = [&](int len, int klo, int khi) {
    int c[kNumCounts] = {0, 0, 0, 0, 0};
    double s[kNumSums] = {0.0, 0.0, 0.0};
    int matched = 0;
    if (tid < ng) {
      const int r = lds.row4col[tid], lv = gt_level[g0 + tid];
      if (r >= 0) {
        matched = 1;
        const double acc = heading_accuracy(pred_boxes[(int64_t)(r0 + r) * 7 + 6], gt_boxes[(int64_t)(g0 + tid) * 7 + 6]);
        if (lv <= 1) c[0] = 1, s[0] = acc;
        if (lv <= 2) c[1] = 1, s[1] = acc;
        s[2] = (double)w[(int64_t)r * gf + tid];
      } else {
        c[3] = lv <= 1;
        c[4] = lv <= 2;
      }
    }
    c[2] = matched;  // turned into the unmatched predictions below
#pragma unroll
    for (int t = 0; t < kNumCounts; ++t) c[t] = wave_reduce_sum(c[t]);
#pragma unroll
    for (int t = 0; t < kNumSums; ++t) s[t] = wave_sum(s[t]);
    if ((tid & 63) == 0) {
      for (int t = 0; t < kNumCounts; ++t) red_i[tid >> 6][t] = c[t];
      for (int t = 0; t < kNumSums; ++t) red_d[tid >> 6][t] = s[t];
    }
    __syncthreads();
    for (int k = klo + tid; k <= khi; k += kEvalThreads) {
      for (int t = 0; t < kNumCounts; ++t) {
        int v = 0;
        for (int wv = 0; wv < kEvalThreads / 64; ++wv) v += red_i[wv][t];
        out_i[k * kNumCounts + t] = t == 2 ? len - v : v;
      }
      for (int t = 0; t < kNumSums; ++t) {
        double v = 0.0;
        for (int wv = 0; wv < kEvalThreads / 64; ++wv) v += red_d[wv][t];  // fixed order
        out_d[k * kNumSums + t] = v;
      }
    }
    __syncthreads();
  };

  // cutoffs above the best score: nothing in play
  const int top = np > 0 ? last_cutoff(scores[r0]) : -1;
  if (top < kCutoffs - 1) emit(0, top + 1, kCutoffs - 1);

  for (int cur = 0; cur < np; ++cur) {
    const int hi = last_cutoff(scores[r0 + cur]);
    if (hi < 0) break;  // sorted by descending score: this row and the ones behind it are never in play
    insert_row(lds, w, gf, ng, tid < ng, cur, tid);

    const int lo = cur + 1 < np ? last_cutoff(scores[r0 + cur + 1]) : -1;
    if (hi > lo) emit(cur + 1, lo + 1, hi);
  }
}

__global__ void accumulate_kernel(const int* __restrict__ counts, const double* __restrict__ sums,
                                  const int* __restrict__ prob, int n_prob, int64_t* __restrict__ total_counts,
                                  double* __restrict__ total_sums) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;  // (class, cutoff)
  if (slot >= 3 * kCutoffs) return;
  const int cls = slot / kCutoffs, k = slot % kCutoffs;
  int64_t c[kNumCounts];
  double s[kNumSums];
  for (int t = 0; t < kNumCounts; ++t) c[t] = total_counts[slot * kNumCounts + t];
  for (int t = 0; t < kNumSums; ++t) s[t] = total_sums[slot * kNumSums + t];
  for (int p = 0; p < n_prob; ++p) {  // problem order: the one order every call uses
    if (prob[(int64_t)p * kProbFields + 5] != cls) continue;
    for (int t = 0; t < kNumCounts; ++t) c[t] += counts[((int64_t)p * kCutoffs + k) * kNumCounts + t];
    for (int t = 0; t < kNumSums; ++t) s[t] += sums[((int64_t)p * kCutoffs + k) * kNumSums + t];
  }
  for (int t = 0; t < kNumCounts; ++t) total_counts[slot * kNumCounts + t] = c[t];
  for (int t = 0; t < kNumSums; ++t) total_sums[slot * kNumSums + t] = s[t];
}

}  // namespace
}  // namespace efg

using namespace efg;

extern "C" int efg_det_eval_max_pred(void) { return kMaxPred; }
extern "C" int efg_det_eval_max_gt(void) { return kMaxGt; }

extern "C" int efg_det_eval_pair_weights_f32(const float* pred_boxes, const int32_t* pred_labels,
                                             const int32_t* pred_off, const float* gt_boxes, const int32_t* gt_labels,
                                             const int32_t* gt_off, const int64_t* blk_off, int n_frames, int max_pred,
                                             int max_gt, float thr_vehicle, float thr_pedestrian, float thr_cyclist,
                                             float* weights, void* stream) {
  EFG_CHECK_ARG(n_frames >= 0 && max_pred >= 0 && max_gt >= 0, "efg_det_eval_pair_weights_f32: negative size (%d, %d, %d)",
                n_frames, max_pred, max_gt);
  if (n_frames == 0 || max_pred == 0 || max_gt == 0) return EFG_OK;  // every block is empty
  EFG_CHECK_ARG(n_frames <= 65535, "efg_det_eval_pair_weights_f32: %d frames in one call (limit 65535)", n_frames);
  EFG_CHECK_ARG(pred_boxes && pred_labels && pred_off && gt_boxes && gt_labels && gt_off && blk_off && weights,
                "efg_det_eval_pair_weights_f32: null pointer");
  const int64_t gy = ceil_div(max_pred, kRowsPerBlock), gx = ceil_div(max_gt, kPairThreads);
  EFG_CHECK_ARG(gy <= 65535, "efg_det_eval_pair_weights_f32: %d predictions in one frame (limit %d)", max_pred,
                65535 * kRowsPerBlock);
  hipLaunchKernelGGL(pair_weight_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)n_frames), dim3(kPairThreads), 0,
                     (hipStream_t)stream, pred_boxes, pred_labels, pred_off, gt_boxes, gt_labels, gt_off, blk_off,
                     thr_vehicle, thr_pedestrian, thr_cyclist, weights);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

extern "C" int efg_det_eval_assign_f32(const float* weights, const int64_t* blk_off, const int32_t* pred_off,
                                       const int32_t* gt_off, const int32_t* problems, int n_problems, int max_pred,
                                       int max_gt, const float* scores, const float* pred_boxes, const float* gt_boxes,
                                       const int32_t* gt_level, int32_t* counts, double* sums, void* stream) {
  EFG_CHECK_ARG(n_problems >= 0 && max_pred >= 0 && max_gt >= 0, "efg_det_eval_assign_f32: negative size (%d, %d, %d)",
                n_problems, max_pred, max_gt);
  EFG_CHECK_ARG(max_pred <= kMaxPred,
                "efg_det_eval_assign_f32: %d predictions of one class in one frame exceed the limit of %d", max_pred,
                kMaxPred);
  EFG_CHECK_ARG(max_gt <= kMaxGt,
                "efg_det_eval_assign_f32: %d ground truths of one class in one frame exceed the limit of %d", max_gt,
                kMaxGt);
  if (n_problems == 0) return EFG_OK;
  EFG_CHECK_ARG(blk_off && pred_off && gt_off && problems && counts && sums, "efg_det_eval_assign_f32: null pointer");
  hipLaunchKernelGGL(prefix_assign_kernel, dim3(n_problems), dim3(kEvalThreads), 0, (hipStream_t)stream, weights, blk_off,
                     pred_off, gt_off, problems, scores, pred_boxes, gt_boxes, gt_level, counts, sums);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

extern "C" int efg_det_eval_accumulate(const int32_t* counts, const double* sums, const int32_t* problems,
                                       int n_problems, int64_t* total_counts, double* total_sums, void* stream) {
  EFG_CHECK_ARG(n_problems >= 0, "efg_det_eval_accumulate: negative problem count %d", n_problems);
  if (n_problems == 0) return EFG_OK;
  EFG_CHECK_ARG(counts && sums && problems && total_counts && total_sums, "efg_det_eval_accumulate: null pointer");
  hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)ceil_div(3 * kCutoffs, 64)), dim3(64), 0, (hipStream_t)stream,
                     counts, sums, problems, n_problems, total_counts, total_sums);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}
