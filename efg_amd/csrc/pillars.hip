// PointPillars reader: the one-layer PillarFeatureNet (decorate -> Linear(Cin, 64) -> BatchNorm1d -> ReLU -> max over the
// pillar's rows) and the BEV scatter, DESIGN.md "PointPillars reader" (§5g).
//
// Tiling of the three passes over the points (stats, apply, backward): a workgroup of four waves takes a tile of kTile = 4
// consecutive pillars -- their raw rows [4, N, F] are one contiguous, 16-byte aligned piece of `voxels`, staged in LDS with
// float4 loads (a tail tile with fewer pillars is staged word by word) -- and each wave owns one pillar of the tile.  The lane
// is the output channel: the 64 channels are exactly a wave, W[c, 0..Cin) sits in registers, and the decorated features of a
// row are the same for every lane, so they are read from LDS as broadcasts.  Tiles are dealt to a bounded grid in a
// grid-stride loop.  The pre-activation of a row is always formed by `row_x` -- the same operations in the same order in
// every pass, built without contraction -- so the forward's selection, the saved index and the backward's gate cannot
// disagree.
//
//   * decoration of row n < count: [raw F, xyz - mean, x - cx, y - cy (, |xyz|)], mean = the sum of xyz over ALL N rows
//     (row 0 first) divided by the count, cx = (float)coors[p, 3] * vx + x_offset (y alike from coors[p, 2]).  A row
//     n >= count is zero after decoration whatever it holds: its pre-activation is x = 0.
//   * stats_kernel: per channel sum x and sum x^2 over the real rows in fp64 (the padded rows add only to the count
//     M = P * N), one partial per workgroup; stats_finish_kernel (one workgroup) adds the partials in a fixed order and
//     writes mean, rstd = (var + eps)^-1/2 from the fp64 moments (|x| of 75 m with a spread of centimetres leaves
//     ~1e-10 relative in fp64) and the running statistics (unbiased M / (M - 1)).
//   * apply_kernel: z = (x - mean) * (rstd * gamma) + beta, relu, the max over the N rows including relu(z(0)) of a padded
//     row; of equal values the lowest row wins (strict >, ascending rows).  Writes out [P, 64] and index uint8 [P, 64].
//   * backward_kernel: per (p, c) the gradient enters at the saved row if z > 0 there: g = dy.  Per channel, in fp64:
//     d beta = sum g, d gamma = sum g xhat, G[c, k] = sum g f[n*, k], X[c, k] = sum over all rows of x f[k] (= W S), and
//     F1[k] = sum f[k]; backward_finish_kernel adds the workgroups' partials in a fixed order and forms
//     dW = gamma rstd (G - (d beta / M) F1 - (d gamma / M) rstd (X - mean F1)).
//   * scatter / gather: one wave per pillar copies its row to / from cell (b, y, x) of the channels-last canvas.
//
// No atomics and no tickets anywhere: every sum has a fixed order, two runs agree in every bit.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace efg {
namespace {

constexpr int kTile = 4;              // pillars per workgroup tile = waves per workgroup
constexpr int kThreads = kTile * kWave;
constexpr int kChannels = 64;         // output channels = lanes of a wave
constexpr int kMaxRows = 64;          // N: the index is a uint8 and a pillar's rows are staged in LDS
constexpr int kMaxCin = 16;
constexpr int kMinF = 3, kMaxF = 11;
constexpr int kFwdBlocks = 1024;      // grid caps (the tiles are looped over)
constexpr int kBwdBlocks = 512;
constexpr int kSegments = 16;         // the finish kernels add the partials as 16 runs of consecutive workgroups, then the runs
constexpr int kCopyBlocks = 2048;
// doubles of one workgroup's backward partial: G [16][64], X [16][64], F1 [16], d beta [64], d gamma [64]
constexpr int kBwdPartial = 2 * kMaxCin * kChannels + kMaxCin + 2 * kChannels;

struct PillarArgs {
  const float* voxels;        // [P, N, F]
  const int32_t* num_points;  // [P]
  const int32_t* coors;       // [P, 4] (b, z, y, x)
  const float* weight;        // [64, Cin]
  int64_t p;
  int n;
  float vx, vy, x_offset, y_offset;
};

template <int F, bool DIST>
struct Shape {
  static constexpr int kCin = F + 5 + (DIST ? 1 : 0);
};

// the tile's raw rows -> LDS, laid out as in HBM; returns nothing, the caller synchronises
template <int F>
__device__ __forceinline__ void stage_tile(const PillarArgs& a, int64_t tile, float* s_raw) {
  const int64_t first = tile * kTile;
  const int pillars = (int)((a.p - first < kTile) ? (a.p - first) : kTile);
  const int per = a.n * F;
  const float* src = a.voxels + first * per;
  const int words = pillars * per;
  if (pillars == kTile) {   // 4 * N * F words from a 16-byte aligned start
    const float4* src4 = reinterpret_cast<const float4*>(src);
    float4* dst4 = reinterpret_cast<float4*>(s_raw);
    for (int i = threadIdx.x; i < per; i += kThreads) dst4[i] = src4[i];
  } else {
    for (int i = threadIdx.x; i < words; i += kThreads) s_raw[i] = src[i];
  }
}

struct PillarHead {
  int count;          // rows that are points, clamped to [0, N]
  float mx, my, mz;   // the cluster mean
  float cx, cy;       // the pillar's centre
};

template <int F>
__device__ __forceinline__ PillarHead pillar_head(const PillarArgs& a, int64_t p, const float* rows) {
  PillarHead h;
  const int cnt = a.num_points[p];
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  for (int n = 0; n < a.n; ++n) {   // ALL rows, as the reference sums before it masks
    sx += rows[n * F + 0];
    sy += rows[n * F + 1];
    sz += rows[n * F + 2];
  }
  const float fc = (float)cnt;
  h.mx = sx / fc;
  h.my = sy / fc;
  h.mz = sz / fc;
  h.cx = (float)a.coors[p * 4 + 3] * a.vx + a.x_offset;
  h.cy = (float)a.coors[p * 4 + 2] * a.vy + a.y_offset;
  h.count = cnt < 0 ? 0 : (cnt > a.n ? a.n : cnt);
  return h;
}

template <int F, bool DIST>
__device__ __forceinline__ void decorate(const float* row, const PillarHead& h, float (&f)[Shape<F, DIST>::kCin]) {
#pragma unroll
  for (int k = 0; k < F; ++k) f[k] = row[k];
  f[F + 0] = row[0] - h.mx;
  f[F + 1] = row[1] - h.my;
  f[F + 2] = row[2] - h.mz;
  f[F + 3] = row[0] - h.cx;
  f[F + 4] = row[1] - h.cy;
  if (DIST) f[Shape<F, DIST>::kCin - 1] = sqrtf(row[0] * row[0] + row[1] * row[1] + row[2] * row[2]);
}

// THE pre-activation of a row: every pass calls this and nothing else
template <int CIN>
__device__ __forceinline__ float row_x(const float (&w)[CIN], const float (&f)[CIN]) {
  float x = 0.0f;
#pragma unroll
  for (int k = 0; k < CIN; ++k) x += w[k] * f[k];
  return x;
}

__device__ __forceinline__ float bn_z(float x, float mean, float scale, float beta) { return (x - mean) * scale + beta; }

template <int CIN>
__device__ __forceinline__ void load_weight(const float* weight, int c, float (&w)[CIN]) {
#pragma unroll
  for (int k = 0; k < CIN; ++k) w[k] = weight[c * CIN + k];
}

// ---- statistics ---------------------------------------------------------------------------------------------------------
template <int F, bool DIST>
__global__ __launch_bounds__(kThreads) void stats_kernel(PillarArgs a, double* __restrict__ partial) {
  constexpr int CIN = Shape<F, DIST>::kCin;
  __shared__ __attribute__((aligned(16))) float s_raw[kTile * kMaxRows * F];
  __shared__ double s_sum[kTile][kChannels], s_sq[kTile][kChannels];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  float w[CIN];
  load_weight<CIN>(a.weight, lane, w);
  double sum = 0.0, sq = 0.0;
  const int64_t tiles = (a.p + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    stage_tile<F>(a, tile, s_raw);
    __syncthreads();
    const int64_t p = tile * kTile + wave;
    if (p < a.p) {
      const float* rows = s_raw + wave * a.n * F;
      const PillarHead h = pillar_head<F>(a, p, rows);
      for (int n = 0; n < h.count; ++n) {
        float f[CIN];
        decorate<F, DIST>(rows + n * F, h, f);
        const double x = (double)row_x<CIN>(w, f);
        sum += x;
        sq += x * x;
      }
    }
    __syncthreads();
  }
  s_sum[wave][lane] = sum;
  s_sq[wave][lane] = sq;
  __syncthreads();
  if (wave == 0) {
    double s = 0.0, q = 0.0;
    for (int v = 0; v < kTile; ++v) {
      s += s_sum[v][lane];
      q += s_sq[v][lane];
    }
    partial[(int64_t)blockIdx.x * 2 * kChannels + lane] = s;
    partial[(int64_t)blockIdx.x * 2 * kChannels + kChannels + lane] = q;
  }
}

// one workgroup of kSegments * 64 threads: thread (segment, channel) adds its run of workgroups, then channel threads add the runs
__global__ __launch_bounds__(kSegments * kChannels) void stats_finish_kernel(
    const double* __restrict__ partial, int blocks, double m, float eps, float momentum, float* __restrict__ mean,
    float* __restrict__ rstd, float* __restrict__ running_mean, float* __restrict__ running_var,
    int64_t* __restrict__ num_batches_tracked) {
  __shared__ double s_sum[kSegments][kChannels], s_sq[kSegments][kChannels];
  const int c = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int per = (blocks + kSegments - 1) / kSegments;
  const int b0 = seg * per, b1 = (b0 + per < blocks) ? b0 + per : blocks;
  double s = 0.0, q = 0.0;
  for (int b = b0; b < b1; ++b) {
    s += partial[(int64_t)b * 2 * kChannels + c];
    q += partial[(int64_t)b * 2 * kChannels + kChannels + c];
  }
  s_sum[seg][c] = s;
  s_sq[seg][c] = q;
  __syncthreads();
  if (seg != 0) return;
  s = 0.0;
  q = 0.0;
  for (int v = 0; v < kSegments; ++v) {
    s += s_sum[v][c];
    q += s_sq[v][c];
  }
  const double mu = s / m;
  double var = q / m - mu * mu;
  if (var < 0.0) var = 0.0;
  mean[c] = (float)mu;
  rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean != nullptr) {
    const double unbiased = var * (m / (m > 1.0 ? m - 1.0 : 1.0));
    running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * mu);
    running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unbiased);
  }
  if (num_batches_tracked != nullptr && c == 0) *num_batches_tracked += 1;
}

// ---- apply --------------------------------------------------------------------------------------------------------------
template <int F, bool DIST>
__global__ __launch_bounds__(kThreads) void apply_kernel(PillarArgs a, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ out,
                                                         uint8_t* __restrict__ index) {
  constexpr int CIN = Shape<F, DIST>::kCin;
  __shared__ __attribute__((aligned(16))) float s_raw[kTile * kMaxRows * F];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  float w[CIN];
  load_weight<CIN>(a.weight, lane, w);
  const float mu = mean[lane], scale = rstd[lane] * gamma[lane], b = beta[lane];
  const float zpad = bn_z(0.0f, mu, scale, b);
  const float vpad = zpad > 0.0f ? zpad : 0.0f;
  const int64_t tiles = (a.p + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    stage_tile<F>(a, tile, s_raw);
    __syncthreads();
    const int64_t p = tile * kTile + wave;
    if (p < a.p) {
      const float* rows = s_raw + wave * a.n * F;
      const PillarHead h = pillar_head<F>(a, p, rows);
      float best = -INFINITY;
      int at = 0;
      for (int n = 0; n < h.count; ++n) {
        float f[CIN];
        decorate<F, DIST>(rows + n * F, h, f);
        const float z = bn_z(row_x<CIN>(w, f), mu, scale, b);
        const float v = z > 0.0f ? z : 0.0f;
        if (v > best) {   // strict: the lowest row of equal values stays
          best = v;
          at = n;
        }
      }
      if (h.count < a.n && vpad > best) {   // the first padded row stands for all of them
        best = vpad;
        at = h.count;
      }
      out[p * kChannels + lane] = best;
      index[p * kChannels + lane] = (uint8_t)at;
    }
    __syncthreads();
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------
template <int F, bool DIST>
__global__ __launch_bounds__(kThreads) void backward_kernel(PillarArgs a, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ dy,
                                                            const uint8_t* __restrict__ index, double* __restrict__ partial) {
  constexpr int CIN = Shape<F, DIST>::kCin;
  __shared__ __attribute__((aligned(16))) float s_raw[kTile * kMaxRows * F];
  __shared__ double s_acc[(3 * CIN + 2) * kChannels];   // G, X, F1 [CIN][64] each, d beta, d gamma [64]
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  float w[CIN];
  load_weight<CIN>(a.weight, lane, w);
  const float mu = mean[lane], rs = rstd[lane], scale = rs * gamma[lane], b = beta[lane];
  double g_acc[CIN], x_acc[CIN], f_acc[CIN];
#pragma unroll
  for (int k = 0; k < CIN; ++k) g_acc[k] = x_acc[k] = f_acc[k] = 0.0;
  double dbeta = 0.0, dgamma = 0.0;
  const int64_t tiles = (a.p + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    stage_tile<F>(a, tile, s_raw);
    __syncthreads();
    const int64_t p = tile * kTile + wave;
    if (p < a.p) {
      const float* rows = s_raw + wave * a.n * F;
      const PillarHead h = pillar_head<F>(a, p, rows);
      const int at = index[p * kChannels + lane];
      const double g = (double)dy[p * kChannels + lane];
      for (int n = 0; n < h.count; ++n) {
        float f[CIN];
        decorate<F, DIST>(rows + n * F, h, f);
        const float x = row_x<CIN>(w, f);
#pragma unroll
        for (int k = 0; k < CIN; ++k) {
          x_acc[k] += (double)x * (double)f[k];
          f_acc[k] += (double)f[k];
        }
        if (n == at && bn_z(x, mu, scale, b) > 0.0f) {
          dbeta += g;
          dgamma += g * (((double)x - (double)mu) * (double)rs);
#pragma unroll
          for (int k = 0; k < CIN; ++k) g_acc[k] += g * (double)f[k];
        }
      }
      if (at >= h.count && bn_z(0.0f, mu, scale, b) > 0.0f) {   // a padded row was selected: x = 0, f = 0
        dbeta += g;
        dgamma += g * ((0.0 - (double)mu) * (double)rs);
      }
    }
    __syncthreads();
  }
  // the four waves add their sums in wave order into one LDS buffer (every slot belongs to one lane index)
  for (int v = 0; v < kTile; ++v) {
    if (wave == v) {
#pragma unroll
      for (int k = 0; k < CIN; ++k) {
        double* gs = s_acc + k * kChannels + lane;
        double* xs = s_acc + (CIN + k) * kChannels + lane;
        double* fs = s_acc + (2 * CIN + k) * kChannels + lane;
        *gs = (v == 0 ? 0.0 : *gs) + g_acc[k];
        *xs = (v == 0 ? 0.0 : *xs) + x_acc[k];
        *fs = (v == 0 ? 0.0 : *fs) + f_acc[k];
      }
      double* bs = s_acc + 3 * CIN * kChannels + lane;
      double* cs = s_acc + (3 * CIN + 1) * kChannels + lane;
      *bs = (v == 0 ? 0.0 : *bs) + dbeta;
      *cs = (v == 0 ? 0.0 : *cs) + dgamma;
    }
    __syncthreads();
  }
  if (wave == 0) {
    double* dst = partial + (int64_t)blockIdx.x * kBwdPartial;
#pragma unroll
    for (int k = 0; k < CIN; ++k) {
      dst[k * kChannels + lane] = s_acc[k * kChannels + lane];
      dst[(kMaxCin + k) * kChannels + lane] = s_acc[(CIN + k) * kChannels + lane];
    }
    if (lane < CIN) dst[2 * kMaxCin * kChannels + lane] = s_acc[(2 * CIN + lane) * kChannels];   // F1: the same in every lane
    dst[2 * kMaxCin * kChannels + kMaxCin + lane] = s_acc[3 * CIN * kChannels + lane];
    dst[2 * kMaxCin * kChannels + kMaxCin + kChannels + lane] = s_acc[(3 * CIN + 1) * kChannels + lane];
  }
}

// grid = Cin workgroups (one per input column k) of kSegments * 64 threads
__global__ __launch_bounds__(kSegments * kChannels) void backward_finish_kernel(
    const double* __restrict__ partial, int blocks, int cin, double m, int batch_stats, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    float* __restrict__ dweight, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ double s_part[5][kSegments][kChannels];
  const int k = blockIdx.x, c = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int per = (blocks + kSegments - 1) / kSegments;
  const int b0 = seg * per, b1 = (b0 + per < blocks) ? b0 + per : blocks;
  double g = 0.0, x = 0.0, f1 = 0.0, db = 0.0, dg = 0.0;
  for (int b = b0; b < b1; ++b) {
    const double* src = partial + (int64_t)b * kBwdPartial;
    g += src[k * kChannels + c];
    x += src[(kMaxCin + k) * kChannels + c];
    f1 += src[2 * kMaxCin * kChannels + k];
    db += src[2 * kMaxCin * kChannels + kMaxCin + c];
    dg += src[2 * kMaxCin * kChannels + kMaxCin + kChannels + c];
  }
  s_part[0][seg][c] = g;
  s_part[1][seg][c] = x;
  s_part[2][seg][c] = f1;
  s_part[3][seg][c] = db;
  s_part[4][seg][c] = dg;
  __syncthreads();
  if (seg != 0) return;
  g = x = f1 = db = dg = 0.0;
  for (int v = 0; v < kSegments; ++v) {
    g += s_part[0][v][c];
    x += s_part[1][v][c];
    f1 += s_part[2][v][c];
    db += s_part[3][v][c];
    dg += s_part[4][v][c];
  }
  const double rs = (double)rstd[c], mu = (double)mean[c];
  double dw = g;
  if (batch_stats) dw = g - (db / m) * f1 - (dg / m) * rs * (x - mu * f1);
  dweight[c * cin + k] = (float)((double)gamma[c] * rs * dw);
  if (k == 0) {
    dgamma[c] = (float)dg;
    dbeta[c] = (float)db;
  }
}

// ---- BEV scatter and its gather --------------------------------------------------------------------------------------------
// canvas: [B, ny, nx, C] row-major (the memory of a channels-last [B, C, ny, nx]); one wave per pillar
template <bool GATHER>
__global__ __launch_bounds__(kThreads) void canvas_copy_kernel(float* __restrict__ feats, float* __restrict__ canvas,
                                                               const int32_t* __restrict__ coors, int64_t p_total, int c_total,
                                                               int batch, int ny, int nx) {
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  for (int64_t p = (int64_t)blockIdx.x * kTile + wave; p < p_total; p += (int64_t)gridDim.x * kTile) {
    const int b = coors[p * 4 + 0], y = coors[p * 4 + 2], x = coors[p * 4 + 3];
    const bool inside = b >= 0 && b < batch && y >= 0 && y < ny && x >= 0 && x < nx;   // never write outside the canvas
    float* row = feats + p * c_total;
    float* cell = canvas + (((int64_t)b * ny + y) * nx + x) * c_total;
    for (int c = lane; c < c_total; c += kWave) {
      if (GATHER) {
        row[c] = inside ? cell[c] : 0.0f;
      } else if (inside) {
        cell[c] = row[c];
      }
    }
  }
}

int check_shape(int64_t p, int n, int f, int with_distance, int cout, const void* voxels) {
  EFG_CHECK_ARG(p >= 0, "pillars: P = %lld", (long long)p);
  EFG_CHECK_ARG(cout == kChannels, "pillars: the fused layer has %d output channels, got %d", kChannels, cout);
  EFG_CHECK_ARG(n >= 1 && n <= kMaxRows, "pillars: N = %d rows per pillar, the fused layer takes 1..%d", n, kMaxRows);
  EFG_CHECK_ARG(f >= kMinF && f <= kMaxF && f + 5 + (with_distance ? 1 : 0) <= kMaxCin,
                "pillars: F = %d raw features%s, the fused layer takes %d..%d with Cin = F + 5 (+ 1) <= %d", f,
                with_distance ? " with the distance column" : "", kMinF, kMaxF, kMaxCin);
  EFG_CHECK_ARG((reinterpret_cast<uintptr_t>(voxels) & 15) == 0, "pillars: voxels must be 16-byte aligned");
  return EFG_OK;
}

int grid_for(int64_t p, int cap, int max_blocks) {
  const int64_t tiles = ceil_div(p, kTile);
  if (max_blocks > 0 && max_blocks < cap) cap = max_blocks;
  return (int)(tiles < cap ? tiles : cap);
}

// F = 3..11 x with / without the distance column, Cin <= 16
#define EFG_PILLAR_DISPATCH(F_, DIST_, ...)                                \
  do {                                                                     \
    bool done_ = true;                                                     \
    if (!(DIST_)) {                                                        \
      switch (F_) {                                                        \
        case 3: { constexpr int F = 3; constexpr bool D = false; __VA_ARGS__; } break;   \
        case 4: { constexpr int F = 4; constexpr bool D = false; __VA_ARGS__; } break;   \
        case 5: { constexpr int F = 5; constexpr bool D = false; __VA_ARGS__; } break;   \
        case 6: { constexpr int F = 6; constexpr bool D = false; __VA_ARGS__; } break;   \
        case 7: { constexpr int F = 7; constexpr bool D = false; __VA_ARGS__; } break;   \
        case 8: { constexpr int F = 8; constexpr bool D = false; __VA_ARGS__; } break;   \
        case 9: { constexpr int F = 9; constexpr bool D = false; __VA_ARGS__; } break;   \
        case 10: { constexpr int F = 10; constexpr bool D = false; __VA_ARGS__; } break; \
        case 11: { constexpr int F = 11; constexpr bool D = false; __VA_ARGS__; } break; \
        default: done_ = false;                                            \
      }                                                                    \
    } else {                                                               \
      switch (F_) {                                                        \
        case 3: { constexpr int F = 3; constexpr bool D = true; __VA_ARGS__; } break;    \
        case 4: { constexpr int F = 4; constexpr bool D = true; __VA_ARGS__; } break;    \
        case 5: { constexpr int F = 5; constexpr bool D = true; __VA_ARGS__; } break;    \
        case 6: { constexpr int F = 6; constexpr bool D = true; __VA_ARGS__; } break;    \
        case 7: { constexpr int F = 7; constexpr bool D = true; __VA_ARGS__; } break;    \
        case 8: { constexpr int F = 8; constexpr bool D = true; __VA_ARGS__; } break;    \
        case 9: { constexpr int F = 9; constexpr bool D = true; __VA_ARGS__; } break;    \
        case 10: { constexpr int F = 10; constexpr bool D = true; __VA_ARGS__; } break;  \
        default: done_ = false;                                            \
      }                                                                    \
    }                                                                      \
    EFG_CHECK_ARG(done_, "pillars: no kernel for F = %d", (int)(F_));      \
  } while (0)

}  // namespace
}  // namespace efg

using namespace efg;

extern "C" {

size_t efg_pillar_workspace_bytes(void) {
  const size_t fwd = (size_t)kFwdBlocks * 2 * kChannels * sizeof(double);
  const size_t bwd = (size_t)kBwdBlocks * kBwdPartial * sizeof(double);
  return align_up(fwd > bwd ? fwd : bwd, 256);
}

int efg_pillar_forward_f32(const float* voxels, const int32_t* num_points, const int32_t* coors, const float* weight,
                           const float* gamma, const float* beta, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, float momentum, float eps, int64_t p, int n, int f,
                           int with_distance, int cout, float vx, float vy, float x_offset, float y_offset,
                           int batch_stats, float* mean, float* rstd, float* out, uint8_t* index, void* ws,
                           size_t ws_bytes, int max_blocks, void* stream) {
  if (int rc = check_shape(p, n, f, with_distance, cout, voxels)) return rc;
  if (p == 0) return EFG_OK;
  EFG_CHECK_ARG(voxels && num_points && coors && weight && gamma && beta && mean && rstd && out && index,
                "pillar_forward: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const PillarArgs a{voxels, num_points, coors, weight, p, n, vx, vy, x_offset, y_offset};
  const int grid = grid_for(p, kFwdBlocks, max_blocks);
  if (batch_stats) {
    EFG_CHECK_ARG(ws && ws_bytes >= efg_pillar_workspace_bytes(), "pillar_forward: workspace too small");
    EFG_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "pillar_forward: one running statistic without the other");
    double* partial = static_cast<double*>(ws);
    EFG_PILLAR_DISPATCH(f, with_distance != 0, stats_kernel<F, D><<<dim3(grid), dim3(kThreads), 0, st>>>(a, partial));
    EFG_LAUNCH_CHECK();
    hipLaunchKernelGGL(stats_finish_kernel, dim3(1), dim3(kSegments * kChannels), 0, st, partial, grid, (double)p * (double)n,
                       eps, momentum, mean, rstd, running_mean, running_var, num_batches_tracked);
    EFG_LAUNCH_CHECK();
  }
  EFG_PILLAR_DISPATCH(f, with_distance != 0,
                      apply_kernel<F, D><<<dim3(grid), dim3(kThreads), 0, st>>>(a, mean, rstd, gamma, beta, out, index));
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

int efg_pillar_backward_f32(const float* voxels, const int32_t* num_points, const int32_t* coors, const float* weight,
                            const float* gamma, const float* beta, const float* mean, const float* rstd, const float* dy,
                            const uint8_t* index, int64_t p, int n, int f, int with_distance, int cout, float vx, float vy,
                            float x_offset, float y_offset, int batch_stats, float* dweight, float* dgamma, float* dbeta,
                            void* ws, size_t ws_bytes, int max_blocks, void* stream) {
  if (int rc = check_shape(p, n, f, with_distance, cout, voxels)) return rc;
  EFG_CHECK_ARG(p > 0, "pillar_backward: P = 0 has no launch; the gradients are zero");
  EFG_CHECK_ARG(voxels && num_points && coors && weight && gamma && beta && mean && rstd && dy && index && dweight && dgamma && dbeta,
                "pillar_backward: null pointer");
  EFG_CHECK_ARG(ws && ws_bytes >= efg_pillar_workspace_bytes(), "pillar_backward: workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const PillarArgs a{voxels, num_points, coors, weight, p, n, vx, vy, x_offset, y_offset};
  const int grid = grid_for(p, kBwdBlocks, max_blocks);
  const int cin = f + 5 + (with_distance ? 1 : 0);
  double* partial = static_cast<double*>(ws);
  EFG_PILLAR_DISPATCH(f, with_distance != 0,
                      backward_kernel<F, D><<<dim3(grid), dim3(kThreads), 0, st>>>(a, mean, rstd, gamma, beta, dy, index, partial));
  EFG_LAUNCH_CHECK();
  hipLaunchKernelGGL(backward_finish_kernel, dim3(cin), dim3(kSegments * kChannels), 0, st, partial, grid, cin,
                     (double)p * (double)n, batch_stats, mean, rstd, gamma, dweight, dgamma, dbeta);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

static int canvas_copy(bool gather, float* feats, float* canvas, const int32_t* coors, int64_t p, int c, int batch, int ny,
                       int nx, void* stream) {
  EFG_CHECK_ARG(p >= 0 && c >= 1 && batch >= 1 && ny >= 1 && nx >= 1, "pillar_scatter: P = %lld, C = %d, canvas %d x %d x %d",
                (long long)p, c, batch, ny, nx);
  EFG_CHECK_ARG((int64_t)batch * ny * nx * c < ((int64_t)1 << 40), "pillar_scatter: canvas too large");
  if (p == 0) return EFG_OK;
  EFG_CHECK_ARG(feats && canvas && coors, "pillar_scatter: null pointer");
  const int64_t blocks = ceil_div(p, kTile);
  const int grid = (int)(blocks < kCopyBlocks ? blocks : kCopyBlocks);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (gather)
    hipLaunchKernelGGL(canvas_copy_kernel<true>, dim3(grid), dim3(kThreads), 0, st, feats, canvas, coors, p, c, batch, ny, nx);
  else
    hipLaunchKernelGGL(canvas_copy_kernel<false>, dim3(grid), dim3(kThreads), 0, st, feats, canvas, coors, p, c, batch, ny, nx);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

int efg_pillar_scatter_f32(const float* feats, const int32_t* coors, int64_t p, int c, int batch, int ny, int nx,
                           float* canvas, void* stream) {
  return canvas_copy(false, const_cast<float*>(feats), canvas, coors, p, c, batch, ny, nx, stream);
}

int efg_pillar_gather_f32(const float* canvas, const int32_t* coors, int64_t p, int c, int batch, int ny, int nx,
                          float* feats, void* stream) {
  return canvas_copy(true, feats, const_cast<float*>(canvas), coors, p, c, batch, ny, nx, stream);
}

}  // extern "C"
