// Per-pair arithmetic of the rotated BEV overlap / IoU / 3-D IoU kernels (iou3d_nms.hip) and the candidate queue
// that feeds it, shared with the detection-evaluation pair-weight kernel (det_eval.hip): one source, so that a weight
// there and boxes_iou3d_gpu here are the same fp32 operations in the same order.
#pragma once
#include "common.h"

namespace efg {
namespace {

constexpr int kMaxPts = 16;  // iou3d_nms_kernel.cu:162 (Point cross_points[16])
constexpr int kPairThreads = 64;
constexpr float kEps = 1e-8f;
constexpr float kMargin = 1e-2f;

struct P2 {
  float x, y;
};

__device__ __forceinline__ float cross3(P2 p1, P2 p2, P2 p0) {
  return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

__device__ __forceinline__ bool rect_cross(P2 p1, P2 p2, P2 q1, P2 q2) {
  return fminf(p1.x, p2.x) <= fmaxf(q1.x, q2.x) && fminf(q1.x, q2.x) <= fmaxf(p1.x, p2.x) &&
         fminf(p1.y, p2.y) <= fmaxf(q1.y, q2.y) && fminf(q1.y, q2.y) <= fmaxf(p1.y, p2.y);
}

struct Box {
  float x, y, dx, dy, cs, sn;  // cs/sn of +heading
  P2 c[4];
};

__device__ __forceinline__ Box load_box(const float* b) {
  Box r;
  r.x = b[0];
  r.y = b[1];
  r.dx = b[3];
  r.dy = b[4];
  r.cs = cosf(b[6]);
  r.sn = sinf(b[6]);
  const float hx = r.dx / 2, hy = r.dy / 2;
  const float xs[4] = {r.x - hx, r.x + hx, r.x + hx, r.x - hx};
  const float ys[4] = {r.y - hy, r.y - hy, r.y + hy, r.y + hy};
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // rotate_around_center :99-104
    r.c[k].x = (xs[k] - r.x) * r.cs + (ys[k] - r.y) * (-r.sn) + r.x;
    r.c[k].y = (xs[k] - r.x) * r.sn + (ys[k] - r.y) * r.cs + r.y;
  }
  return r;
}

// check_in_box2d :54-64 rotates by -heading: cos(-a) = cs, sin(-a) = -sn (exact symmetries of cosf/sinf).
__device__ __forceinline__ bool in_box(const Box& b, P2 p) {
  const float c = b.cs, s = -b.sn;
  const float rx = (p.x - b.x) * c + (p.y - b.y) * (-s);
  const float ry = (p.x - b.x) * s + (p.y - b.y) * c;
  return fabsf(rx) < b.dx / 2 + kMargin && fabsf(ry) < b.dy / 2 + kMargin;
}

__device__ __forceinline__ bool seg_intersection(P2 p1, P2 p0, P2 q1, P2 q0, P2* ans) {  // :66-97
  if (!rect_cross(p0, p1, q0, q1)) return false;
  const float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0), s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
  if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
  const float s5 = cross3(q1, p1, p0);
  if (fabsf(s5 - s1) > kEps) {
    ans->x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    ans->y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
    const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
    const float D = a0 * b1 - a1 * b0;
    ans->x = (b0 * c1 - b1 * c0) / D;
    ans->y = (a1 * c0 - a0 * c1) / D;
  }
  return true;
}

// True when the two (margin-inflated) rectangles cannot share a point: every vertex the clipper could emit
// lies inside both inflated rectangles, each of which lies inside the disc of radius half-diagonal +
// sqrt(2) * margin around its centre.  0.05 leaves > 3x slack over that and over fp32 rounding.
__device__ __forceinline__ bool far_apart(const float* a, const float* b) {
  const float ra = 0.5f * sqrtf(a[3] * a[3] + a[4] * a[4]), rb = 0.5f * sqrtf(b[3] * b[3] + b[4] * b[4]);
  const float dx = a[0] - b[0], dy = a[1] - b[1], r = ra + rb + 0.05f;
  return dx * dx + dy * dy > r * r;
}

// Polygon-intersection area.  px/py/pa: this lane's LDS columns (stride = blockDim.x floats).
template <int STRIDE>
__device__ __forceinline__ float box_overlap(const float* box_a, const float* box_b, float* px, float* py, float* pa) {
  if (far_apart(box_a, box_b)) return 0.0f;
  const Box A = load_box(box_a), B = load_box(box_b);
  int cnt = 0;
  float cx = 0.f, cy = 0.f;
  auto push = [&](P2 p) {
    if (cnt < kMaxPts) {
      cx += p.x;
      cy += p.y;
      px[cnt * STRIDE] = p.x;
      py[cnt * STRIDE] = p.y;
      ++cnt;
    }
  };
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      P2 ans;
      if (seg_intersection(A.c[(i + 1) & 3], A.c[i], B.c[(j + 1) & 3], B.c[j], &ans)) push(ans);
    }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (in_box(A, B.c[k])) push(B.c[k]);
    if (in_box(B, A.c[k])) push(A.c[k]);
  }
  if (cnt == 0) return 0.0f;
  cx /= cnt;
  cy /= cnt;
  // stable insertion sort by angle == the reference's bubble sort with a strict '>' (:207-215)
  for (int k = 0; k < cnt; ++k) pa[k * STRIDE] = atan2f(py[k * STRIDE] - cy, px[k * STRIDE] - cx);
  for (int k = 1; k < cnt; ++k) {
    const float a = pa[k * STRIDE], x = px[k * STRIDE], y = py[k * STRIDE];
    int m = k - 1;
    while (m >= 0 && pa[m * STRIDE] > a) {
      pa[(m + 1) * STRIDE] = pa[m * STRIDE];
      px[(m + 1) * STRIDE] = px[m * STRIDE];
      py[(m + 1) * STRIDE] = py[m * STRIDE];
      --m;
    }
    pa[(m + 1) * STRIDE] = a;
    px[(m + 1) * STRIDE] = x;
    py[(m + 1) * STRIDE] = y;
  }
  float area = 0.f;
  const float x0 = px[0], y0 = py[0];
  for (int k = 0; k < cnt - 1; ++k) {
    const float ax = px[k * STRIDE] - x0, ay = py[k * STRIDE] - y0;
    const float bx = px[(k + 1) * STRIDE] - x0, by = py[(k + 1) * STRIDE] - y0;
    area += ax * by - ay * bx;
  }
  return fabsf(area) / 2.0f;
}

template <int STRIDE>
__device__ __forceinline__ float iou_bev(const float* a, const float* b, float* px, float* py, float* pa) {
  const float sa = a[3] * a[4], sb = b[3] * b[4], so = box_overlap<STRIDE>(a, b, px, py, pa);
  return so / fmaxf(sa + sb - so, kEps);
}

// Candidate queue shared by both pair kernels.  Rotated boxes rarely overlap (a fraction of a percent of the
// pairs at detection densities), but one candidate lane drags its whole wave through the clipper.  So the
// lanes first run the cheap exact reject, push the surviving (row, col) pairs into an LDS queue with a
// ballot/popcount, and the clipper only runs on full waves of candidates (plus one final partial wave).
constexpr int kQueueCap = 128;  // < 64 pending + 64 pushed per step

struct PairQueue {
  int* rows;
  int* cols;
  int n;  // wave-uniform
  // every lane of the (single-wave) block calls this; returns true when >= 64 entries are pending
  __device__ __forceinline__ bool push(bool cand, int r, int c) {
    const unsigned long long b = __ballot(cand);
    if (cand) {
      const int pos = n + __popcll(b & ((1ULL << lane_id()) - 1ULL));
      rows[pos] = r;
      cols[pos] = c;
    }
    n += __popcll(b);
    return n >= 64;
  }
  // pops up to 64 entries: lane gets (r, c) and returns whether it holds one
  __device__ __forceinline__ bool pop(int* r, int* c) {
    __syncthreads();  // single-wave block: orders the LDS writes above before the reads below
    const int base = n >= 64 ? n - 64 : 0;
    const int e = base + lane_id();
    const bool has = e < n;
    *r = has ? rows[e] : 0;
    *c = has ? cols[e] : 0;
    n = base;
    __syncthreads();
    return has;
  }
};

// mode 0: BEV overlap area, 1: BEV IoU, 2: 3-D IoU (iou3d_nms.py:54-87 fused: height overlap, volumes).
// One single-wave block owns a 64 (rows of a) x 64 (columns of b) tile: lane <-> b column (registers), the a
// row is wave-uniform (scalar loads); rejected pairs store their exact 0 as 256 B coalesced rows.
constexpr int kRowsPerBlock = 64;

__device__ __forceinline__ float pair_value(const float* a, const float* b, int mode, float* px, float* py, float* pa) {
  if (mode == 1) return iou_bev<kPairThreads>(a, b, px, py, pa);
  float v = box_overlap<kPairThreads>(a, b, px, py, pa);
  if (mode == 2) {
    const float a_max = a[2] + a[5] / 2, a_min = a[2] - a[5] / 2;
    const float b_max = b[2] + b[5] / 2, b_min = b[2] - b[5] / 2;
    const float oh = fmaxf(fminf(a_max, b_max) - fmaxf(a_min, b_min), 0.f);
    const float o3 = v * oh;
    const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
    v = o3 / fmaxf(va + vb - o3, 1e-6f);
  }
  return v;
}

}  // namespace
}  // namespace efg
