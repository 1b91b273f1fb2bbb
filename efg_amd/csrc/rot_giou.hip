// Heading-aware 3-D GIoU of 7-DoF boxes (cx, cy, cz, l, w, h, rad) as fused kernels: the rotated counterpart of giou3d() in
// det_loss.hip for the matching cost and the box loss, plus a paired forward / backward for direct use.
//
//   inter3d = area(rectA ^ rectB) * max(0, z overlap)          union3d = volA + volB - inter3d
//   hull3d  = area(convex hull of the 8 BEV corners) * (z range of both)
//   giou    = inter3d / union3d - (hull3d - union3d) / hull3d
//
// Inputs are the model's normalised codes; a host-side frame (sx, sy, yaw_scale, yaw_offset) maps them to metres and radians:
// centre (cx sx, cy sy), size (l sx, w sy), yaw = rad yaw_scale + yaw_offset.  The z extent is cz +- h / 2 (GIoU does not depend
// on the z scale).
//
// One thread per pair, everything in registers (fixed-trip loops over the 4 + 4 edges and the 8 corners, no dynamically
// indexed array), no atomics.  All BEV geometry is evaluated in the frame of box B -- origin at B's centre, axes along B's
// sides -- entered through the DIFFERENCE of the codes, so a pair 70 m from the origin is as accurate as one at the origin.
//
// Intersection area: Green's theorem over the boundary of the intersection, which is made of the parts of A's edges inside B
// and the parts of B's edges inside A (each found by clipping a segment to a centred rectangle), area = 1/2 sum cross(p0, p1).
// Edges of A are clipped to the CLOSED rectangle B and edges of B to the OPEN rectangle A, so that edges lying on each other
// (identical boxes) are counted once.
// Hull area: gift wrapping from the lowest corner, at most 8 steps, shoelace sum over the steps.
// Backward recomputes the geometry.  For a parameter of A, d area / d p is the integral of the normal velocity over the parts
// of A's edges inside B (translation: length x normal; a side: half the length of the two edges it moves; rotation: -integral
// of the arc coordinate measured from the edge's midpoint); likewise for the sides of B.  The hull is the shoelace sum
// differentiated at its corner vertices.  Both areas depend on the relative pose only: the gradient to B's centre and yaw
// follows from A's (d/dcB = -d/dcA, d/dyawB = -d/dyawA - cross(cA - cB, d/dcA)).
#include "common.h"

namespace efg {
namespace {

__device__ __forceinline__ float nan_to_num(float v) {  // torch.nan_to_num defaults (as det_loss.hip)
  if (v != v) return 0.0f;
  if (v == INFINITY) return 3.4028234663852886e38f;
  if (v == -INFINITY) return -3.4028234663852886e38f;
  return v;
}

struct Frame {
  float sx, sy, yaw_scale, yaw_offset;
};

// [t0, t1] &= { t : |p + t d| <= h }  (kStrict: < h when the segment is parallel to the slab)
template <bool kStrict>
__device__ __forceinline__ void clip_slab(float p, float d, float h, float& t0, float& t1) {
  if (d == 0.f) {
    const bool in = kStrict ? fabsf(p) < h : fabsf(p) <= h;
    if (!in) t1 = -1.f;
  } else {
    const float ta = (-h - p) / d, tb = (h - p) / d;
    t0 = fmaxf(t0, fminf(ta, tb));
    t1 = fminf(t1, fmaxf(ta, tb));
  }
}

// gradient of the two BEV areas to the seven planar parameters, in B's frame
struct Planar {
  float dx = 0.f, dy = 0.f, th = 0.f, la = 0.f, wa = 0.f, lb = 0.f, wb = 0.f;
};

// GIoU of the pair (ap, bp); *iou (optional) receives inter3d / union3d.  kGrad: ga[7] / gb[7] receive d giou / d codes.
template <bool kGrad>
__device__ __forceinline__ float rot_giou3d(const float* __restrict__ ap, const float* __restrict__ bp, Frame f, float* iou,
                                            float* ga, float* gb) {
  float a[7], b[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    a[k] = nan_to_num(ap[k]);
    b[k] = nan_to_num(bp[k]);
  }
  const float al = a[3] * f.sx, aw = a[4] * f.sy, bl = b[3] * f.sx, bw = b[4] * f.sy;
  const float hax = 0.5f * al, hay = 0.5f * aw, hbx = 0.5f * bl, hby = 0.5f * bw;
  // A's centre and heading in B's frame
  const float ddx = (a[0] - b[0]) * f.sx, ddy = (a[1] - b[1]) * f.sy;
  float sb, cb, st, ct;
  sincosf(b[6] * f.yaw_scale + f.yaw_offset, &sb, &cb);
  sincosf((a[6] - b[6]) * f.yaw_scale, &st, &ct);
  const float dx = cb * ddx + sb * ddy, dy = cb * ddy - sb * ddx;
  // corners, counter-clockwise: 0..3 of A (signs (+,+), (-,+), (-,-), (+,-) along its length and width axes), 4..7 of B
  float px[8], py[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float su = (k == 0 || k == 3) ? 1.f : -1.f, sv = k < 2 ? 1.f : -1.f;
    px[k] = dx + su * hax * ct - sv * hay * st;
    py[k] = dy + su * hax * st + sv * hay * ct;
    px[4 + k] = su * hbx;
    py[4 + k] = sv * hby;
  }

  // ---- intersection area ------------------------------------------------------------------------------------------------
  float inter = 0.f;
  Planar gi;
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // edge k of A (corner k -> k + 1) inside the closed B
    const int k1 = (k + 1) & 3;
    const float ex = px[k1] - px[k], ey = py[k1] - py[k];
    float t0 = 0.f, t1 = 1.f;
    clip_slab<false>(px[k], ex, hbx, t0, t1);
    clip_slab<false>(py[k], ey, hby, t0, t1);
    if (t1 > t0) {
      const float x0 = px[k] + t0 * ex, y0 = py[k] + t0 * ey, x1 = px[k] + t1 * ex, y1 = py[k] + t1 * ey;
      inter += 0.5f * (x0 * y1 - y0 * x1);
      if (kGrad) {
        const float side = (k & 1) ? aw : al;              // edges 0, 2 run along the length, 1, 3 along the width
        const float len = (t1 - t0) * side;
        // outward normals: +v, -u, -v, +u  (u = (ct, st), v = (-st, ct))
        const float nx = k == 0 ? -st : (k == 1 ? -ct : (k == 2 ? st : ct));
        const float ny = k == 0 ? ct : (k == 1 ? -st : (k == 2 ? -ct : st));
        gi.dx += len * nx;
        gi.dy += len * ny;
        if (k & 1) gi.la += 0.5f * len; else gi.wa += 0.5f * len;
        gi.th -= 0.5f * side * side * (t1 - t0) * (t1 + t0 - 1.f);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // edge k of B inside the open A: clipped in A's frame, summed in B's
    const int k1 = (k + 1) & 3;
    const float qx = px[4 + k], qy = py[4 + k], ex = px[4 + k1] - qx, ey = py[4 + k1] - qy;
    const float rx = ct * (qx - dx) + st * (qy - dy), ry = ct * (qy - dy) - st * (qx - dx);
    const float fx = ct * ex + st * ey, fy = ct * ey - st * ex;
    float t0 = 0.f, t1 = 1.f;
    clip_slab<true>(rx, fx, hax, t0, t1);
    clip_slab<true>(ry, fy, hay, t0, t1);
    if (t1 > t0) {
      const float x0 = qx + t0 * ex, y0 = qy + t0 * ey, x1 = qx + t1 * ex, y1 = qy + t1 * ey;
      inter += 0.5f * (x0 * y1 - y0 * x1);
      if (kGrad) {
        const float len = (t1 - t0) * ((k & 1) ? bw : bl);
        if (k & 1) gi.lb += 0.5f * len; else gi.wb += 0.5f * len;
      }
    }
  }
  inter = fmaxf(inter, 0.f);

  // ---- hull area: gift wrapping from the lowest (then leftmost) corner -----------------------------------------------------
  float sx0 = px[0], sy0 = py[0];
  int si = 0;
#pragma unroll
  for (int k = 1; k < 8; ++k)
    if (py[k] < sy0 || (py[k] == sy0 && px[k] < sx0)) {
      sx0 = px[k];
      sy0 = py[k];
      si = k;
    }
  float hull = 0.f, cx = sx0, cy = sy0;
  int ci = si;
  bool done = false;
  float hgx[8], hgy[8];  // d hull / d corner
#pragma unroll
  for (int k = 0; k < 8; ++k) hgx[k] = hgy[k] = 0.f;
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    float bx = cx, by = cy;
    int bi = -1;
#pragma unroll
    for (int c = 0; c < 8; ++c) {  // the corner every other corner is to the left of; the farthest of collinear ones
      const float ex = px[c] - cx, ey = py[c] - cy;
      const float fx = bx - cx, fy = by - cy;
      const float cr = fx * ey - fy * ex;
      const bool other = ex != 0.f || ey != 0.f;
      const bool take = other && (bi < 0 || cr < 0.f || (cr == 0.f && ex * ex + ey * ey > fx * fx + fy * fy));
      if (take) {
        bx = px[c];
        by = py[c];
        bi = c;
      }
    }
    if (!done && bi >= 0) {
      hull += 0.5f * (cx * by - cy * bx);
      if (kGrad) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if (k == ci) {
            hgx[k] += 0.5f * by;
            hgy[k] -= 0.5f * bx;
          }
          if (k == bi) {
            hgx[k] -= 0.5f * cy;
            hgy[k] += 0.5f * cx;
          }
        }
      }
    }
    if (bi < 0 || (bx == sx0 && by == sy0)) done = true;
    cx = bx;
    cy = by;
    ci = bi;
  }
  hull = fmaxf(hull, 0.f);

  // ---- z extent, volumes, GIoU -------------------------------------------------------------------------------------------
  const float alo = a[2] - 0.5f * a[5], ahi = a[2] + 0.5f * a[5], blo = b[2] - 0.5f * b[5], bhi = b[2] + 0.5f * b[5];
  const float zo_raw = fminf(ahi, bhi) - fmaxf(alo, blo), zr_raw = fmaxf(ahi, bhi) - fminf(alo, blo);
  const float zo = fmaxf(zo_raw, 0.f), zr = fmaxf(zr_raw, 0.f);
  const float va = al * aw * a[5], vb = bl * bw * b[5];
  const float i3 = inter * zo, u3 = va + vb - i3, h3 = hull * zr;
  const float iou3 = i3 / u3;
  if (iou) *iou = iou3;
  const float giou = iou3 - (h3 - u3) / h3;

  if (kGrad) {
    Planar gh;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float su = (k == 0 || k == 3) ? 1.f : -1.f, sv = k < 2 ? 1.f : -1.f;
      gh.dx += hgx[k];
      gh.dy += hgy[k];
      gh.th += (px[k] - dx) * hgy[k] - (py[k] - dy) * hgx[k];
      gh.la += 0.5f * su * (ct * hgx[k] + st * hgy[k]);
      gh.wa += 0.5f * sv * (ct * hgy[k] - st * hgx[k]);
      gh.lb += 0.5f * su * hgx[4 + k];
      gh.wb += 0.5f * sv * hgy[4 + k];
    }
    // giou = i3 / u3 - 1 + u3 / h3,  u3 = va + vb - i3
    const float c_v = 1.f / h3 - i3 / (u3 * u3), c_i3 = 1.f / u3 - c_v, c_h3 = -u3 / (h3 * h3);
    const float wi = c_i3 * zo, wh = c_h3 * zr;
    const float g_dx = wi * gi.dx + wh * gh.dx, g_dy = wi * gi.dy + wh * gh.dy, g_th = wi * gi.th + wh * gh.th;
    // z: clamp(raw, min = 0) passes the gradient for raw >= 0 and a tie of min / max goes half to each side, as autograd does
    const float zi = zo_raw >= 0.f ? c_i3 * inter : 0.f, zh = zr_raw >= 0.f ? c_h3 * hull : 0.f;
    const float hi_i = ahi < bhi ? 1.f : (ahi == bhi ? 0.5f : 0.f), hi_h = ahi > bhi ? 1.f : (ahi == bhi ? 0.5f : 0.f);
    const float lo_i = alo > blo ? 1.f : (alo == blo ? 0.5f : 0.f), lo_h = alo < blo ? 1.f : (alo == blo ? 0.5f : 0.f);
    const float ga_hi = zi * hi_i + zh * hi_h, ga_lo = -(zi * lo_i + zh * lo_h);
    ga[0] = (cb * g_dx - sb * g_dy) * f.sx;
    ga[1] = (sb * g_dx + cb * g_dy) * f.sy;
    ga[2] = ga_hi + ga_lo;
    ga[3] = (wi * gi.la + wh * gh.la + c_v * aw * a[5]) * f.sx;
    ga[4] = (wi * gi.wa + wh * gh.wa + c_v * al * a[5]) * f.sy;
    ga[5] = 0.5f * (ga_hi - ga_lo) + c_v * al * aw;
    ga[6] = g_th * f.yaw_scale;
    if (gb) {
      const float gb_hi = zi * (1.f - hi_i) + zh * (1.f - hi_h), gb_lo = -(zi * (1.f - lo_i) + zh * (1.f - lo_h));
      gb[0] = -ga[0];
      gb[1] = -ga[1];
      gb[2] = gb_hi + gb_lo;
      gb[3] = (wi * gi.lb + wh * gh.lb + c_v * bw * b[5]) * f.sx;
      gb[4] = (wi * gi.wb + wh * gh.wb + c_v * bl * b[5]) * f.sy;
      gb[5] = 0.5f * (gb_hi - gb_lo) + c_v * bl * bw;
      gb[6] = (-g_th - (dx * g_dy - dy * g_dx)) * f.yaw_scale;
    }
  }
  return giou;
}

// ---- paired ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
rot_giou_paired_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n, Frame f,
                           float* __restrict__ giou, float* __restrict__ iou) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v;
  giou[i] = rot_giou3d<false>(a + i * 7, b + i * 7, f, &v, nullptr, nullptr);
  if (iou) iou[i] = v;
}

__global__ void __launch_bounds__(256)
rot_giou_paired_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n, Frame f,
                           const float* __restrict__ gout, float* __restrict__ grad_a, float* __restrict__ grad_b) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float ga[7], gb[7];
  rot_giou3d<true>(a + i * 7, b + i * 7, f, nullptr, ga, gb);
  const float g = gout[i];
#pragma unroll
  for (int k = 0; k < 7; ++k) grad_a[i * 7 + k] = g * ga[k];
  if (grad_b) {
#pragma unroll
    for (int k = 0; k < 7; ++k) grad_b[i * 7 + k] = g * gb[k];
  }
}

// ---- matching cost: match_cost_kernel of det_loss.hip with the rotated GIoU term ------------------------------------------------
struct CostW {
  float w_class, w_bbox, w_giou, w_rad, alpha, gamma;
};

__global__ void __launch_bounds__(256)
match_cost_rot_kernel(const float* __restrict__ logits, const float* __restrict__ boxes, const long long* __restrict__ tgt_labels,
                      const float* __restrict__ tgt_boxes, int P, int B, int Q, int C, int G, CostW w, Frame f,
                      float* __restrict__ cost) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)P * Q * G) return;
  const int g = (int)(e % G);
  const long long pq = e / G;
  const int q = (int)(pq % Q), p = (int)(pq / Q), b = p % B;
  const float* bx = boxes + ((long long)p * Q + q) * 7;
  const float* tb = tgt_boxes + ((long long)b * G + g) * 7;
  const int lab = (int)tgt_labels[(long long)b * G + g];
  const float x = logits[((long long)p * Q + q) * C + lab];
  const float pr = 1.0f / (1.0f + expf(-x));
  const float neg = (1.f - w.alpha) * powf(pr, w.gamma) * (-logf(1.f - pr + 1e-8f));
  const float pos = w.alpha * powf(1.f - pr, w.gamma) * (-logf(pr + 1e-8f));
  float l1 = 0.f;
#pragma unroll
  for (int k = 0; k < 6; ++k) l1 += fabsf(bx[k] - tb[k]);
  const float rad = fabsf(bx[6] - tb[6]);
  const float giou = rot_giou3d<false>(bx, tb, f, nullptr, nullptr, nullptr);
  cost[e] = w.w_bbox * l1 + w.w_class * (pos - neg) + w.w_giou * (-giou) + w.w_rad * rad;
}

// ---- box losses over matched pairs: box_loss_kernel / box_loss_grad_kernel of det_loss.hip, column 1 = 1 - rotated GIoU --------
__device__ __forceinline__ float block_sum_1024(float v, float* sm) {  // blockDim.x == 1024
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x < 16) r = sm[threadIdx.x];
  if (threadIdx.x < 64) {
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) r += __shfl_xor(r, d, 64);
  }
  __syncthreads();
  return r;  // valid in thread 0
}

__global__ void __launch_bounds__(1024)
box_loss_rot_kernel(const float* __restrict__ boxes, const float* __restrict__ tgt, const long long* __restrict__ li,
                    const long long* __restrict__ bi, const long long* __restrict__ qi, const long long* __restrict__ gi,
                    long long n, int B, int Q, int G, const float* __restrict__ denom, Frame f, float* __restrict__ out) {
  __shared__ float sm[16];
  const int l = blockIdx.x;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (long long i = threadIdx.x; i < n; i += 1024) {
    if (li[i] != l || qi[i] < 0 || qi[i] >= Q) continue;  // unmatched column (infeasible assignment): no pair
    const float* s = boxes + ((li[i] * B + bi[i]) * Q + qi[i]) * 7;
    const float* t = tgt + (bi[i] * G + gi[i]) * 7;
    float l1 = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) l1 += fabsf(s[k] - t[k]);
    a0 += l1;
    a1 += 1.f - rot_giou3d<false>(s, t, f, nullptr, nullptr, nullptr);
    a2 += fabsf(s[6] - t[6]);
  }
  const float s0 = block_sum_1024(a0, sm), s1 = block_sum_1024(a1, sm), s2 = block_sum_1024(a2, sm);
  if (threadIdx.x == 0) {
    out[l * 3 + 0] = s0 / denom[0];
    out[l * 3 + 1] = s1 / denom[0];
    out[l * 3 + 2] = s2 / denom[0];
  }
}

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// gout [L][3]; gboxes [L][B][Q][7] must be zero-filled (only matched rows are written; a row is matched once)
__global__ void __launch_bounds__(256)
box_loss_rot_grad_kernel(const float* __restrict__ boxes, const float* __restrict__ tgt, const long long* __restrict__ li,
                         const long long* __restrict__ bi, const long long* __restrict__ qi, const long long* __restrict__ gi,
                         long long n, int B, int Q, int G, const float* __restrict__ denom, const float* __restrict__ gout,
                         Frame f, float* __restrict__ gboxes) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || qi[i] < 0 || qi[i] >= Q) return;  // unmatched column: nothing to write (never index out of range)
  const long long row = ((li[i] * B + bi[i]) * Q + qi[i]) * 7;
  const float* s = boxes + row;
  const float* t = tgt + (bi[i] * G + gi[i]) * 7;
  const float inv = 1.0f / denom[0];
  const float g_l1 = gout[li[i] * 3 + 0] * inv, g_gi = gout[li[i] * 3 + 1] * inv, g_rd = gout[li[i] * 3 + 2] * inv;
  float ga[7];
  rot_giou3d<true>(s, t, f, nullptr, ga, nullptr);
#pragma unroll
  for (int k = 0; k < 6; ++k) gboxes[row + k] = g_l1 * sgn(s[k] - t[k]) - g_gi * ga[k];   // loss_giou = 1 - giou
  gboxes[row + 6] = g_rd * sgn(s[6] - t[6]) - g_gi * ga[6];
}

inline Frame load_frame(const float* frame) { return Frame{frame[0], frame[1], frame[2], frame[3]}; }

}  // namespace
}  // namespace efg

using namespace efg;

extern "C" int efg_rot_giou_paired_forward_f32(const float* a, const float* b, int64_t n, const float* frame, float* giou,
                                               float* iou, void* stream) {
  EFG_CHECK_ARG(n >= 0 && frame, "rot_giou: bad arguments");
  if (n == 0) return EFG_OK;
  EFG_CHECK_ARG(a && b && giou, "rot_giou: null pointer");
  hipLaunchKernelGGL(rot_giou_paired_fwd_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, a, b,
                     (long long)n, load_frame(frame), giou, iou);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

extern "C" int efg_rot_giou_paired_backward_f32(const float* a, const float* b, int64_t n, const float* frame,
                                                const float* grad_giou, float* grad_a, float* grad_b, void* stream) {
  EFG_CHECK_ARG(n >= 0 && frame, "rot_giou backward: bad arguments");
  if (n == 0) return EFG_OK;
  EFG_CHECK_ARG(a && b && grad_giou && grad_a, "rot_giou backward: null pointer");
  hipLaunchKernelGGL(rot_giou_paired_bwd_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, a, b,
                     (long long)n, load_frame(frame), grad_giou, grad_a, grad_b);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

extern "C" int efg_match_cost_rot_f32(const float* logits, const float* boxes, const int64_t* tgt_labels,
                                      const float* tgt_boxes, int p, int b, int q, int c, int g, float w_class, float w_bbox,
                                      float w_giou, float w_rad, float alpha, float gamma, const float* frame, float* cost,
                                      void* stream) {
  EFG_CHECK_ARG(p >= 0 && b >= 1 && q >= 0 && c >= 1 && g >= 0 && p % b == 0 && frame, "match_cost_rot: bad arguments");
  const long long total = (long long)p * q * g;
  if (total == 0) return EFG_OK;
  EFG_CHECK_ARG(logits && boxes && tgt_labels && tgt_boxes && cost, "match_cost_rot: null pointer");
  hipLaunchKernelGGL(match_cost_rot_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, logits,
                     boxes, (const long long*)tgt_labels, tgt_boxes, p, b, q, c, g,
                     CostW{w_class, w_bbox, w_giou, w_rad, alpha, gamma}, load_frame(frame), cost);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

extern "C" int efg_box_loss_rot_forward_f32(const float* boxes, const float* tgt_boxes, const int64_t* l_idx,
                                            const int64_t* b_idx, const int64_t* q_idx, const int64_t* g_idx, int64_t n,
                                            int layers, int b, int q, int g, const float* denom, const float* frame, float* out,
                                            void* stream) {
  EFG_CHECK_ARG(layers >= 0 && n >= 0 && frame, "box_loss_rot: bad arguments");
  if (layers == 0) return EFG_OK;
  EFG_CHECK_ARG(denom && out && (n == 0 || (boxes && tgt_boxes && l_idx && b_idx && q_idx && g_idx)),
                "box_loss_rot: null pointer");
  hipLaunchKernelGGL(box_loss_rot_kernel, dim3(layers), dim3(1024), 0, (hipStream_t)stream, boxes, tgt_boxes,
                     (const long long*)l_idx, (const long long*)b_idx, (const long long*)q_idx, (const long long*)g_idx,
                     (long long)n, b, q, g, denom, load_frame(frame), out);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

extern "C" int efg_box_loss_rot_backward_f32(const float* boxes, const float* tgt_boxes, const int64_t* l_idx,
                                             const int64_t* b_idx, const int64_t* q_idx, const int64_t* g_idx, int64_t n,
                                             int layers, int b, int q, int g, const float* denom, const float* grad_out,
                                             const float* frame, float* grad_boxes, void* stream) {
  EFG_CHECK_ARG(layers >= 0 && n >= 0 && frame, "box_loss_rot: bad arguments");
  if (n == 0) return EFG_OK;
  EFG_CHECK_ARG(boxes && tgt_boxes && l_idx && b_idx && q_idx && g_idx && denom && grad_out && grad_boxes,
                "box_loss_rot: null pointer");
  hipLaunchKernelGGL(box_loss_rot_grad_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, boxes,
                     tgt_boxes, (const long long*)l_idx, (const long long*)b_idx, (const long long*)q_idx,
                     (const long long*)g_idx, (long long)n, b, q, g, denom, grad_out, load_frame(frame), grad_boxes);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}
