// The 3-D GIoU of 7-DoF boxes (cx, cy, cz, l, w, h, rad) in its two forms, axis-aligned (the reference's: heading ignored)
// and heading-aware, with their gradients: the per-pair arithmetic of the matching cost and the box loss (det_loss.hip, which
// takes the form as a policy, AlignedGIoU or RotatedGIoU, at the end of this file) and of the paired kernels (rot_giou.hip).
// One source, so that a cost, a loss and a paired value of the same boxes are the same fp32 operations in the same order.
#pragma once
#include "common.h"

namespace efg {
namespace {

__device__ __forceinline__ float nan_to_num(float v) {  // torch.nan_to_num defaults
  if (v != v) return 0.0f;
  if (v == INFINITY) return 3.4028234663852886e38f;
  if (v == -INFINITY) return -3.4028234663852886e38f;
  return v;
}

// axis-aligned 3-D GIoU of (centre, size) boxes, as utils.paired_box3d_giou on box_cxcyczlwh_to_xyxyxy
__device__ __forceinline__ float giou3d(const float* s, const float* t) {
  float inter = 1.f, vol = 1.f, v1 = 1.f, v2 = 1.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float slo = nan_to_num(s[k] - 0.5f * s[3 + k]), shi = nan_to_num(s[k] + 0.5f * s[3 + k]);
    const float tlo = nan_to_num(t[k] - 0.5f * t[3 + k]), thi = nan_to_num(t[k] + 0.5f * t[3 + k]);
    v1 *= shi - slo;
    v2 *= thi - tlo;
    inter *= fmaxf(fminf(shi, thi) - fmaxf(slo, tlo), 0.f);
    vol *= fmaxf(fmaxf(shi, thi) - fminf(slo, tlo), 0.f);
  }
  const float uni = v1 + v2 - inter;
  return inter / uni - (vol - uni) / vol;
}

// g[0..5] += g_gi * d loss_giou / d s[0..5],  loss_giou = 1 - giou3d(s, t) = 2 - inter/union - union/vol
__device__ __forceinline__ void giou3d_add_loss_grad(const float* s, const float* t, float g_gi, float* g) {
  // The intersection and enclosing sides are clamp(raw, min = 0), and autograd's clamp passes the gradient for raw >= 0 -- also
  // at raw == 0 exactly, two boxes that touch on a face (the clamped value alone cannot tell that from separated boxes): the
  // unclamped differences are kept and tested with >=, as the PyTorch composite (detection3d/losses.py) differentiates.
  float slo[3], shi[3], tlo[3], thi[3], ik[3], ek[3], iraw[3], eraw[3];
  float inter = 1.f, vol = 1.f, v1 = 1.f, v2 = 1.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    slo[k] = s[k] - 0.5f * s[3 + k];
    shi[k] = s[k] + 0.5f * s[3 + k];
    tlo[k] = t[k] - 0.5f * t[3 + k];
    thi[k] = t[k] + 0.5f * t[3 + k];
    v1 *= shi[k] - slo[k];
    v2 *= thi[k] - tlo[k];
    iraw[k] = fminf(shi[k], thi[k]) - fmaxf(slo[k], tlo[k]);
    eraw[k] = fmaxf(shi[k], thi[k]) - fminf(slo[k], tlo[k]);
    ik[k] = fmaxf(iraw[k], 0.f);
    ek[k] = fmaxf(eraw[k], 0.f);
    inter *= ik[k];
    vol *= ek[k];
  }
  const float uni = v1 + v2 - inter;
  // d loss / d inter, d union, d vol
  const float d_inter_direct = -1.f / uni, d_uni = inter / (uni * uni) - 1.f / vol, d_vol = uni / (vol * vol);
  const float d_inter = d_inter_direct - d_uni;  // union = v1 + v2 - inter
  const float d_v1 = d_uni;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
    float g_hi = 0.f, g_lo = 0.f;
    // vol1 = prod (shi - slo)
    const float dv1 = d_v1 * (shi[k1] - slo[k1]) * (shi[k2] - slo[k2]);
    g_hi += dv1;
    g_lo -= dv1;
    // inter_k = clamp(min(shi, thi) - max(slo, tlo), 0)
    if (iraw[k] >= 0.f) {
      const float di = d_inter * ik[k1] * ik[k2];
      if (shi[k] < thi[k]) g_hi += di; else if (shi[k] == thi[k]) g_hi += 0.5f * di;
      if (slo[k] > tlo[k]) g_lo -= di; else if (slo[k] == tlo[k]) g_lo -= 0.5f * di;
    }
    // enc_k = clamp(max(shi, thi) - min(slo, tlo), 0)
    if (eraw[k] >= 0.f) {
      const float de = d_vol * ek[k1] * ek[k2];
      if (shi[k] > thi[k]) g_hi += de; else if (shi[k] == thi[k]) g_hi += 0.5f * de;
      if (slo[k] < tlo[k]) g_lo -= de; else if (slo[k] == tlo[k]) g_lo -= 0.5f * de;
    }
    g[k] += g_gi * (g_hi + g_lo);
    g[3 + k] += g_gi * 0.5f * (g_hi - g_lo);
  }
}

// ---- heading-aware: the rotated counterpart of giou3d() ---------------------------------------------------------------------
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

inline Frame load_frame(const float* frame) { return Frame{frame[0], frame[1], frame[2], frame[3]}; }

// ---- the two forms as the policy of the det_loss.hip kernels (passed by value as a kernel argument) -----------------------------
// value(s, t): the GIoU of prediction s and target t;  add_loss_grad(s, t, g_gi, g): g[0..6] += g_gi * d (1 - value) / d s
struct AlignedGIoU {
  __device__ __forceinline__ float value(const float* s, const float* t) const { return giou3d(s, t); }
  __device__ __forceinline__ void add_loss_grad(const float* s, const float* t, float g_gi, float* g) const {
    giou3d_add_loss_grad(s, t, g_gi, g);
  }
};

struct RotatedGIoU {
  Frame f;
  __device__ __forceinline__ float value(const float* s, const float* t) const {
    return rot_giou3d<false>(s, t, f, nullptr, nullptr, nullptr);
  }
  __device__ __forceinline__ void add_loss_grad(const float* s, const float* t, float g_gi, float* g) const {
    float ga[7];
    rot_giou3d<true>(s, t, f, nullptr, ga, nullptr);
#pragma unroll
    for (int k = 0; k < 7; ++k) g[k] -= g_gi * ga[k];
  }
};

}  // namespace
}  // namespace efg
