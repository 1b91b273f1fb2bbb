// nuScenes detection evaluation on the device: DESIGN.md "nuScenes detection evaluation" (§5e).
//
// Two kernels, one launch each per `process` call of the evaluator:
//
//   * greedy_match_kernel: one workgroup of 256 threads per (frame, class) problem of the CSR layout det_eval.hip uses.
//     The protocol matches greedily by descending score on the 2-D centre distance, once per distance threshold, so the
//     four waves of a workgroup are the four thresholds: each wave walks the problem's predictions (sorted by descending
//     score on the host) on its own, wave-synchronously -- no block barrier inside the loop.  The ground-truth centres sit
//     in LDS as fp64, written once and shared by the four waves.  Lane l owns the ground-truth columns l + 64 k, k < 16
//     (hence the limit of 1024 ground truths per problem) and keeps their "taken" bits in one 16-bit register mask.  Per
//     prediction a lane finds the minimum (distance, row) over its untaken columns, the wave reduces the pair
//     lexicographically in six xor-shuffle steps (equal distances go to the lowest row), the winner is compared with the
//     wave's threshold (strictly below = true positive), the owning lane sets its bit and lane 0 stores the global
//     ground-truth row, or -1.  No atomics, nothing between workgroups, no dynamic LDS.
//     The distance is sqrt(dx * dx + dy * dy) in fp64 on the float32 centres -- the expression of the host formulation
//     (efg_amd/evaluator/nuscenes.py), in its operation order, built without contraction: the matches are the host's.
//
//   * match_errors_kernel: one thread per prediction.  Packs the four true-positive bits and, for a true positive at the
//     third threshold (2 m in the protocol), computes the five errors (translation, scale, orientation, velocity,
//     attribute) in fp64; NaN where undefined or unmatched.
#include "common.h"

#include <math.h>

namespace efg {
namespace {

constexpr int kMatchThreads = 256;                   // four waves = four thresholds
constexpr int kThresholds = kMatchThreads / kWave;
constexpr int kColsPerLane = 16;
constexpr int kMaxGt = kWave * kColsPerLane;         // 1024
constexpr int kProbFields = 5;                       // first prediction, predictions, first ground truth, ground truths, class
constexpr int kBoxDim = 9;                           // x, y, z, l, w, h, yaw, vx, vy
constexpr int kErrors = 5;                           // trans, scale, orient, vel, attr
constexpr int kNoRow = 0x7fffffff;

__device__ __forceinline__ double centre_distance(double ax, double ay, double bx, double by) {
  const double dx = ax - bx, dy = ay - by;
  return sqrt(dx * dx + dy * dy);
}

__global__ __launch_bounds__(kMatchThreads) void greedy_match_kernel(
    const float* __restrict__ pred_boxes, const float* __restrict__ gt_boxes, const int* __restrict__ prob,
    int64_t n_pred, int64_t n_gt, float thr0, float thr1, float thr2, float thr3, int* __restrict__ match) {
  __shared__ double gx[kMaxGt], gy[kMaxGt];

  const int* d = prob + (int64_t)blockIdx.x * kProbFields;
  const int64_t p0 = d[0], g0 = d[2];
  // the host refuses problems outside the arrays or above the limit; the clamps keep a wrong table inside them anyway
  int np = d[1], ng = d[3];
  if (p0 < 0 || g0 < 0 || p0 > n_pred || g0 > n_gt) return;  // block-uniform
  np = (int)min((int64_t)max(np, 0), n_pred - p0);
  ng = (int)min((int64_t)min(max(ng, 0), kMaxGt), n_gt - g0);

  for (int j = threadIdx.x; j < ng; j += kMatchThreads) {
    gx[j] = (double)gt_boxes[(g0 + j) * kBoxDim + 0];
    gy[j] = (double)gt_boxes[(g0 + j) * kBoxDim + 1];
  }
  __syncthreads();

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double thr = (double)(wave == 0 ? thr0 : wave == 1 ? thr1 : wave == 2 ? thr2 : thr3);
  int* out = match + (int64_t)wave * n_pred + p0;
  const int cols = (ng + kWave - 1) / kWave;  // columns per lane in use (wave-uniform)
  unsigned taken = 0;

  for (int i = 0; i < np; ++i) {
    const double px = (double)pred_boxes[(p0 + i) * kBoxDim + 0], py = (double)pred_boxes[(p0 + i) * kBoxDim + 1];
    double best = INFINITY;
    int row = kNoRow;
    for (int k = 0; k < cols; ++k) {
      const int j = lane + kWave * k;
      if (j < ng && !((taken >> k) & 1u)) {
        const double dist = centre_distance(px, py, gx[j], gy[j]);
        if (dist < best) {  // rows ascend inside a lane: the lowest row of equal distances stays; NaN never wins
          best = dist;
          row = j;
        }
      }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      const double ob = __shfl_xor(best, m, 64);
      const int orow = __shfl_xor(row, m, 64);
      if (ob < best || (ob == best && orow < row)) {
        best = ob;
        row = orow;
      }
    }
    const bool hit = row != kNoRow && best < thr;
    if (hit && (row & 63) == lane) taken |= 1u << (row >> 6);
    if (lane == 0) out[i] = hit ? (int)(g0 + row) : -1;
  }
}

__global__ void match_errors_kernel(const float* __restrict__ pred_boxes, const int* __restrict__ pred_attr,
                                    const int* __restrict__ pred_class, const float* __restrict__ gt_boxes,
                                    const int* __restrict__ gt_attr, const int* __restrict__ match, int64_t n_pred,
                                    int64_t n_gt, int barrier_class, int* __restrict__ tp_bits,
                                    double* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pred) return;
  int bits = 0;
#pragma unroll
  for (int t = 0; t < kThresholds; ++t) bits |= (match[(int64_t)t * n_pred + i] >= 0) << t;
  tp_bits[i] = bits;

  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double e[kErrors] = {nan, nan, nan, nan, nan};
  const int64_t m = match[(int64_t)2 * n_pred + i];
  if (m >= 0 && m < n_gt) {
    double p[kBoxDim], g[kBoxDim];
#pragma unroll
    for (int k = 0; k < kBoxDim; ++k) {
      p[k] = (double)pred_boxes[i * kBoxDim + k];
      g[k] = (double)gt_boxes[m * kBoxDim + k];
    }
    e[0] = centre_distance(p[0], p[1], g[0], g[1]);
    const double inter = fmin(p[3], g[3]) * fmin(p[4], g[4]) * fmin(p[5], g[5]);
    const double vol_p = p[3] * p[4] * p[5], vol_g = g[3] * g[4] * g[5];
    e[1] = 1.0 - inter / (vol_p + vol_g - inter);
    const double pi = 3.141592653589793, two_pi = 6.283185307179586;
    const double period = pred_class[i] == barrier_class ? pi : two_pi;
    double r = fmod(p[6] - g[6] + period / 2.0, period);
    if (r < 0.0) r += period;  // the floored remainder
    double a = fabs(r - period / 2.0);
    if (a > pi) a = two_pi - a;
    e[2] = a;
    const double dvx = p[7] - g[7], dvy = p[8] - g[8];
    e[3] = sqrt(dvx * dvx + dvy * dvy);
    const int ga = gt_attr[m];
    if (ga >= 0) e[4] = pred_attr[i] == ga ? 0.0 : 1.0;
  }
#pragma unroll
  for (int k = 0; k < kErrors; ++k) err[i * kErrors + k] = e[k];
}

}  // namespace
}  // namespace efg

using namespace efg;

extern "C" int efg_nusc_eval_max_gt(void) { return kMaxGt; }

extern "C" int efg_nusc_eval_match_f32(const float* pred_boxes, const float* gt_boxes, const int32_t* problems,
                                       int n_problems, int max_gt, int64_t n_pred, int64_t n_gt, float thr0, float thr1,
                                       float thr2, float thr3, int32_t* match, void* stream) {
  EFG_CHECK_ARG(n_problems >= 0 && max_gt >= 0 && n_pred >= 0 && n_gt >= 0,
                "efg_nusc_eval_match_f32: negative size (%d, %d, %lld, %lld)", n_problems, max_gt, (long long)n_pred,
                (long long)n_gt);
  EFG_CHECK_ARG(max_gt <= kMaxGt,
                "efg_nusc_eval_match_f32: %d ground truths of one class in one frame exceed the limit of %d", max_gt,
                kMaxGt);
  if (n_problems == 0 || n_pred == 0) return EFG_OK;
  EFG_CHECK_ARG(pred_boxes && problems && match && (gt_boxes || n_gt == 0), "efg_nusc_eval_match_f32: null pointer");
  hipLaunchKernelGGL(greedy_match_kernel, dim3((unsigned)n_problems), dim3(kMatchThreads), 0, (hipStream_t)stream,
                     pred_boxes, gt_boxes, problems, n_pred, n_gt, thr0, thr1, thr2, thr3, match);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

extern "C" int efg_nusc_eval_errors_f32(const float* pred_boxes, const int32_t* pred_attr, const int32_t* pred_class,
                                        const float* gt_boxes, const int32_t* gt_attr, const int32_t* match,
                                        int64_t n_pred, int64_t n_gt, int barrier_class, int32_t* tp_bits, double* err,
                                        void* stream) {
  EFG_CHECK_ARG(n_pred >= 0 && n_gt >= 0, "efg_nusc_eval_errors_f32: negative size (%lld, %lld)", (long long)n_pred,
                (long long)n_gt);
  if (n_pred == 0) return EFG_OK;
  EFG_CHECK_ARG(pred_boxes && pred_attr && pred_class && match && tp_bits && err && ((gt_boxes && gt_attr) || n_gt == 0),
                "efg_nusc_eval_errors_f32: null pointer");
  const int64_t blocks = ceil_div(n_pred, 256);
  EFG_CHECK_ARG(blocks <= 0x7fffffff, "efg_nusc_eval_errors_f32: %lld predictions in one call", (long long)n_pred);
  hipLaunchKernelGGL(match_errors_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pred_boxes,
                     pred_attr, pred_class, gt_boxes, gt_attr, match, n_pred, n_gt, barrier_class, tp_bits, err);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}
