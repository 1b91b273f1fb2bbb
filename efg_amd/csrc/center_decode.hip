// CenterPoint inference with the circular NMS as a device chain: DESIGN.md "CenterPoint circular-NMS inference" (§5f).
//
// Three kernels, one launch each per `predict` call, over the head's maps as NHWC-contiguous fp32 (the channels-last maps
// of the GPU model after permute(0, 2, 3, 1)):
//
//   * candidates_kernel: one thread per (scene, task, cell).  score = max_c sigmoid(hm[c]) (label: the lowest c at the
//     maximum), x = ((ix + reg0) * out_size_factor) * voxel_size[0] + pc_range[0] (y alike, z = height) in exactly this
//     association, built without contraction.  A cell is a candidate iff score > score_threshold and the centre is inside
//     the (inclusive) range; every other cell gets the score -inf, which no later step can pick.  Rows of H * W per
//     (scene, task): score, label, x, y; the position in the row is the cell index.
//
//   * circle_nms_kernel: one workgroup of 1024 threads per segment (= (scene, task) in the chain).  The segment's scores
//     are staged once in LDS as order-preserving integer keys (0 = not a candidate / suppressed / kept), at most
//     kMaxCells = 36 864 of them = 144 KB, the staging of topk.hip.  Then a repeated block-wide arg-max: the candidate
//     with the largest (score, lowest index) still alive is kept; the pass that looks for the next one first suppresses
//     what lies within the radius of the one just kept ((xi-xj)*(xi-xj) + (yi-yj)*(yi-yj) <= radius in fp32: the SQUARED
//     distance against the radius itself, as the reference compares), so one pass over the row and one reduction per kept
//     candidate.  That is the reference's greedy loop exactly (the next kept one is the best unsuppressed one), with its
//     unspecified order among equal scores fixed to the ascending index, for every candidate count 0..H*W, and it stops
//     after post_max kept candidates: no sort, no truncation of the candidates, no atomics, nothing between workgroups.
//
//   * boxes_kernel: one thread per (scene, task, kept slot): decodes the kept cell only -- [x, y, height, exp(dim0..2),
//     (vel0..1,) atan2(rot0, rot1)], its score and label + the task's class offset -- into the scene's padded
//     [tasks * post_max, box_dim] block, task-major, kept order.
#include "common.h"

#include <math.h>

namespace efg {
namespace {

constexpr int kMaxTasks = 8;
constexpr int kMaxCells = 36864;       // keys of one segment in LDS: 144 KB
constexpr int kNmsThreads = 1024;
constexpr int kNmsWaves = kNmsThreads / kWave;

struct TaskMaps {
  const float* hm;       // [B, H, W, ncls]
  const float* reg;      // [B, H, W, 2]
  const float* height;   // [B, H, W, 1]
  const float* dim;      // [B, H, W, 3]
  const float* rot;      // [B, H, W, 2]
  const float* vel;      // [B, H, W, 2] or nullptr
  int ncls;
  int cls_offset;
};

struct TaskTable {
  TaskMaps t[kMaxTasks];
};

struct Radii {
  float r[kMaxTasks];
};

struct Geometry {
  float out_size_factor, vx, vy, px, py, score_threshold;
  float lo[3], hi[3];
  int has_limit;
};

__device__ __forceinline__ unsigned order_key(float x) {   // larger float <=> larger key; never 0 for a non-NaN
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(256) void candidates_kernel(TaskTable tab, Geometry g, int n_tasks, int h, int w,
                                                         float* __restrict__ score, int* __restrict__ label,
                                                         float* __restrict__ xs, float* __restrict__ ys) {
  const int cells = h * w;
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= cells) return;
  const int seg = blockIdx.y, scene = seg / n_tasks, task = seg - scene * n_tasks;   // block-uniform
  const TaskMaps& m = tab.t[task];
  const int64_t at = (int64_t)scene * cells + cell;
  const float* hm = m.hm + at * m.ncls;
  float best = -INFINITY;
  int lab = 0;
  for (int c = 0; c < m.ncls; ++c) {
    const float s = 1.0f / (1.0f + expf(-hm[c]));
    if (s > best) {   // strict: the lowest class of equal scores stays
      best = s;
      lab = c;
    }
  }
  const int iy = cell / w, ix = cell - iy * w;
  const float x = (((float)ix + m.reg[at * 2 + 0]) * g.out_size_factor) * g.vx + g.px;
  const float y = (((float)iy + m.reg[at * 2 + 1]) * g.out_size_factor) * g.vy + g.py;
  bool ok = best > g.score_threshold;
  if (g.has_limit) {
    const float z = m.height[at];
    ok = ok && x >= g.lo[0] && x <= g.hi[0] && y >= g.lo[1] && y <= g.hi[1] && z >= g.lo[2] && z <= g.hi[2];
  }
  const int64_t o = (int64_t)seg * cells + cell;
  score[o] = ok ? best : -INFINITY;
  label[o] = lab;
  xs[o] = x;
  ys[o] = y;
}

// (key, index) as one 64-bit word: the larger word is the larger score, or of equal scores the lower index.  0 = nothing.
__device__ __forceinline__ unsigned long long pack(unsigned key, int i) {
  return ((unsigned long long)key << 32) | (unsigned)(0x7fffffff - i);
}

__global__ __launch_bounds__(kNmsThreads) void circle_nms_kernel(const float* __restrict__ xs, const float* __restrict__ ys,
                                                                 const float* __restrict__ score, int seg_len, Radii radii,
                                                                 int n_radii, int post_max, int* __restrict__ keep,
                                                                 int* __restrict__ count) {
  extern __shared__ unsigned keys[];            // seg_len words
  __shared__ unsigned long long wave_best[kNmsWaves];
  __shared__ unsigned long long s_winner;

  const int seg = blockIdx.x, tid = threadIdx.x;
  const int64_t base = (int64_t)seg * seg_len;
  const float* x = xs + base;
  const float* y = ys + base;
  const float radius = radii.r[seg % n_radii];
  int* out = keep + (int64_t)seg * post_max;

  for (int i = tid; i < seg_len; i += kNmsThreads) {
    const float s = score[base + i];
    keys[i] = s > -INFINITY ? order_key(s) : 0u;   // -inf and NaN take no part
  }
  __syncthreads();

  int kept = 0, cur = -1;          // block-uniform
  float cx = 0.0f, cy = 0.0f;
  while (kept < post_max) {
    unsigned long long best = 0ull;
    for (int i = tid; i < seg_len; i += kNmsThreads) {
      const unsigned key = keys[i];
      if (key == 0u) continue;
      if (cur >= 0) {
        const float dx = cx - x[i], dy = cy - y[i];
        const float dist = dx * dx + dy * dy;
        if (i == cur || dist <= radius) {
          keys[i] = 0u;
          continue;
        }
      }
      const unsigned long long p = pack(key, i);
      best = p > best ? p : best;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      const unsigned long long o = __shfl_xor(best, m, 64);
      best = o > best ? o : best;
    }
    if ((tid & 63) == 0) wave_best[tid >> 6] = best;
    __syncthreads();
    if (tid < kWave) {
      unsigned long long b = tid < kNmsWaves ? wave_best[tid] : 0ull;
#pragma unroll
      for (int m = kNmsWaves / 2; m > 0; m >>= 1) {
        const unsigned long long o = __shfl_xor(b, m, 64);
        b = o > b ? o : b;
      }
      if (tid == 0) s_winner = b;
    }
    __syncthreads();
    const unsigned long long win = s_winner;
    if (win == 0ull) break;        // nothing alive (block-uniform)
    cur = 0x7fffffff - (int)(unsigned)(win & 0xffffffffull);
    cx = x[cur];
    cy = y[cur];
    if (tid == 0) out[kept] = cur;
    ++kept;
    // s_winner and wave_best are rewritten only after the next pass's first barrier, which every thread reaches after
    // this read
  }
  if (tid == 0) count[seg] = kept;
}

__global__ __launch_bounds__(256) void boxes_kernel(TaskTable tab, int n_tasks, int batch, int cells, int post_max,
                                                    int box_dim, const float* __restrict__ xs, const float* __restrict__ ys,
                                                    const float* __restrict__ score, const int* __restrict__ label,
                                                    const int* __restrict__ keep, const int* __restrict__ count,
                                                    float* __restrict__ boxes, float* __restrict__ scores,
                                                    int* __restrict__ labels) {
  const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (scene, task, k): the output row
  if (slot >= (int64_t)batch * n_tasks * post_max) return;
  const int seg = (int)(slot / post_max), k = (int)(slot - (int64_t)seg * post_max);
  if (k >= min(count[seg], post_max)) return;
  const int cell = keep[slot];
  if (cell < 0 || cell >= cells) return;   // (cannot happen: the NMS writes cell indices of its own segment)
  const int scene = seg / n_tasks, task = seg - scene * n_tasks;
  const TaskMaps& m = tab.t[task];
  const int64_t at = (int64_t)scene * cells + cell, o = (int64_t)seg * cells + cell;
  float* b = boxes + slot * box_dim;
  b[0] = xs[o];
  b[1] = ys[o];
  b[2] = m.height[at];
  b[3] = expf(m.dim[at * 3 + 0]);
  b[4] = expf(m.dim[at * 3 + 1]);
  b[5] = expf(m.dim[at * 3 + 2]);
  if (m.vel) {
    b[6] = m.vel[at * 2 + 0];
    b[7] = m.vel[at * 2 + 1];
  }
  b[box_dim - 1] = atan2f(m.rot[at * 2 + 0], m.rot[at * 2 + 1]);
  scores[slot] = score[o];
  labels[slot] = label[o] + m.cls_offset;
}

// maps: host array [n_tasks * 6] of device pointers (hm, reg, height, dim, rot, vel) per task
int fill_table(TaskTable* tab, const void* const* maps, const int32_t* num_classes, int n_tasks, bool* has_vel) {
  int offset = 0;
  *has_vel = maps[5] != nullptr;
  for (int t = 0; t < n_tasks; ++t) {
    const void* const* p = maps + t * 6;
    EFG_CHECK_ARG(p[0] && p[1] && p[2] && p[3] && p[4], "center_decode: null map of task %d", t);
    EFG_CHECK_ARG((p[5] != nullptr) == *has_vel, "center_decode: task %d differs from task 0 in having vel", t);
    EFG_CHECK_ARG(num_classes[t] >= 1, "center_decode: task %d has %d classes", t, num_classes[t]);
    TaskMaps& m = tab->t[t];
    m.hm = (const float*)p[0];
    m.reg = (const float*)p[1];
    m.height = (const float*)p[2];
    m.dim = (const float*)p[3];
    m.rot = (const float*)p[4];
    m.vel = (const float*)p[5];
    m.ncls = num_classes[t];
    m.cls_offset = offset;
    offset += num_classes[t];
  }
  return EFG_OK;
}

}  // namespace
}  // namespace efg

using namespace efg;

extern "C" int efg_center_decode_max_cells(void) { return kMaxCells; }
extern "C" int efg_center_decode_max_tasks(void) { return kMaxTasks; }

extern "C" int efg_center_decode_candidates_f32(const void* const* maps, const int32_t* num_classes, int n_tasks, int batch,
                                                int h, int w, float out_size_factor, float voxel_x, float voxel_y,
                                                float range_x, float range_y, float score_threshold, const float* limit,
                                                float* score, int32_t* label, float* x, float* y, void* stream) {
  EFG_CHECK_ARG(n_tasks >= 1 && n_tasks <= kMaxTasks, "center_decode: %d tasks, the task table holds 1..%d", n_tasks,
                kMaxTasks);
  EFG_CHECK_ARG(batch >= 0 && h >= 1 && w >= 1, "center_decode: bad shape (%d, %d, %d)", batch, h, w);
  EFG_CHECK_ARG((int64_t)h * w <= kMaxCells, "center_decode: %lld cells per map exceed the limit of %d", (long long)h * w,
                kMaxCells);
  EFG_CHECK_ARG((int64_t)batch * n_tasks <= 65535, "center_decode: %lld (scene, task) pairs in one call",
                (long long)batch * n_tasks);
  if (batch == 0) return EFG_OK;
  EFG_CHECK_ARG(maps && num_classes && score && label && x && y, "center_decode: null pointer");
  TaskTable tab = {};
  bool has_vel;
  if (int rc = fill_table(&tab, maps, num_classes, n_tasks, &has_vel)) return rc;
  Geometry g = {};
  g.out_size_factor = out_size_factor, g.vx = voxel_x, g.vy = voxel_y, g.px = range_x, g.py = range_y;
  g.score_threshold = score_threshold;
  g.has_limit = limit != nullptr;
  for (int k = 0; k < 3 && limit; ++k) g.lo[k] = limit[k], g.hi[k] = limit[3 + k];
  const int cells = h * w;
  hipLaunchKernelGGL(candidates_kernel, dim3((unsigned)ceil_div(cells, 256), (unsigned)(batch * n_tasks)), dim3(256), 0,
                     (hipStream_t)stream, tab, g, n_tasks, h, w, score, label, x, y);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

extern "C" int efg_circle_nms_f32(const float* x, const float* y, const float* score, int n_segments, int segment_len,
                                  const float* radius, int n_radius, int post_max, int32_t* keep, int32_t* count,
                                  void* stream) {
  EFG_CHECK_ARG(n_segments >= 0 && segment_len >= 0 && post_max >= 0, "circle_nms: negative size (%d, %d, %d)", n_segments,
                segment_len, post_max);
  EFG_CHECK_ARG(segment_len <= kMaxCells, "circle_nms: %d candidates in one segment exceed the limit of %d", segment_len,
                kMaxCells);
  EFG_CHECK_ARG(radius && n_radius >= 1 && n_radius <= kMaxTasks, "circle_nms: 1..%d radii (got %d)", kMaxTasks, n_radius);
  if (n_segments == 0) return EFG_OK;
  EFG_CHECK_ARG(count && (keep || post_max == 0) && ((x && y && score) || segment_len == 0), "circle_nms: null pointer");
  Radii radii = {};
  for (int k = 0; k < n_radius; ++k) radii.r[k] = radius[k];
  EFG_ALLOW_DYNAMIC_LDS(circle_nms_kernel, kMaxCells * 4);
  hipLaunchKernelGGL(circle_nms_kernel, dim3((unsigned)n_segments), dim3(kNmsThreads), (size_t)segment_len * 4,
                     (hipStream_t)stream, x, y, score, segment_len, radii, n_radius, post_max, keep, count);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

extern "C" int efg_center_decode_boxes_f32(const void* const* maps, const int32_t* num_classes, int n_tasks, int batch, int h,
                                           int w, int post_max, const float* x, const float* y, const float* score,
                                           const int32_t* label, const int32_t* keep, const int32_t* count, float* boxes,
                                           float* scores, int32_t* labels, void* stream) {
  EFG_CHECK_ARG(n_tasks >= 1 && n_tasks <= kMaxTasks, "center_decode: %d tasks, the task table holds 1..%d", n_tasks,
                kMaxTasks);
  EFG_CHECK_ARG(batch >= 0 && h >= 1 && w >= 1 && post_max >= 0, "center_decode: bad shape (%d, %d, %d, %d)", batch, h, w,
                post_max);
  EFG_CHECK_ARG((int64_t)h * w <= kMaxCells, "center_decode: %lld cells per map exceed the limit of %d", (long long)h * w,
                kMaxCells);
  const int64_t slots = (int64_t)batch * n_tasks * post_max;
  if (slots == 0) return EFG_OK;
  EFG_CHECK_ARG(ceil_div(slots, 256) <= 0x7fffffff, "center_decode: %lld output rows in one call", (long long)slots);
  EFG_CHECK_ARG(maps && num_classes && x && y && score && label && keep && count && boxes && scores && labels,
                "center_decode: null pointer");
  TaskTable tab = {};
  bool has_vel;
  if (int rc = fill_table(&tab, maps, num_classes, n_tasks, &has_vel)) return rc;
  hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)ceil_div(slots, 256)), dim3(256), 0, (hipStream_t)stream, tab, n_tasks,
                     batch, h * w, post_max, has_vel ? 9 : 7, x, y, score, label, keep, count, boxes, scores, labels);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}
