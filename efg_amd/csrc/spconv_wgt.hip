// Weight gradient of a sparse convolution over a TILE PLAN (spconv_tiles.hip), for gfx950.
//
//   dW[co][k][ci] = sum_o G[o][co] * X[nbr[k][o]][ci]
// (reference: spconv's indice-conv backward -- the pair-gathered GEMM  dW_k = G_pairs^T . X_pairs  per kernel offset,
// called from efg/modeling/backbones/sparse_net.py through spconv.SparseConv3d / SubMConv3d).
//
// The table-walking kernel (spconv_conv.hip: conv_wgrad_kernel, which stays for the widths this one does not cover and
// as the reference this one is tested against) walks the neighbour table, compacts the valid
// (out row, in row) pairs of 256 rows through an LDS queue with ballots and workgroup barriers, stages 32-pair tiles
// of both operands in LDS and reads MFMA fragments back: three barriers per 1024 MFMA cycles, 0.31 of the fp32 MFMA
// peak in the training step.  Here the reduction dimension of the product IS the row dimension, so a 16-row tile of
// the plan is four K-steps of v_mfma_f32_16x16x4_f32 whose operands can come straight from HBM / L2 in fragment layout:
// lane (m = lane & 15, kk = lane >> 4) of K-step q supplies A[m][kk] = G[row(4 kk + q)][channel of m] and
// B[kk][m] = X[nbr(4 kk + q)][channel of m] -- and since WHICH channel an M / N index stands for is free, a lane takes 4
// consecutive channels of its row for the 4 tiles of the block: one 16-byte load per operand and K-step, the 16 lanes of
// a row reading its 256 bytes contiguously.  No LDS, no transposition, no barrier.
// The plan has already sorted the rows by neighbour mask, so a (tile, offset) unit is either absent (skipped: one mask
// word per tile) or nearly full (x1.10-1.15 the exact pair count); a lane's four row numbers of a unit are ONE 16-byte
// load (rows 4 kk .. 4 kk + 3 of the tile's row list / neighbour column).
//
// Launch: one workgroup = (slot of the schedule below: ONE kernel offset and a range of tiles holding ~80 active ones,
// 16 NCO x 16 NCI block of dW: 64 x 64 from 64 channels up); its four waves deal the active tiles of the range
// round-robin, each accumulating the whole block privately over a register pipeline (row numbers of unit u + 2 and
// operands of unit u + 1 in flight during the 4 NCO NCI MFMAs of unit u); the four partial blocks are summed through LDS
// in wave order and the workgroup's block goes to the workspace, which wgt_reduce_kernel folds over the slots of each
// offset in a fixed order (bit-reproducible run to run, as before).
#include "common.h"
#include "tile_plan.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace efg {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

struct WgtArgs {
  const float* in;     // [m_in][cin]
  const float* go;     // [m_out][cout]
  const int* rows;     // plan
  const int* nb;
  const unsigned* vm;
  const int4* entry;   // schedule, in DISPATCH order: (offset, first tile, end tile, slot) per workgroup; offset < 0: unused
  float* partial;      // [slots][cout][cin_pad]
  long long n_tiles;   // multiple of 64
  int cin, cout, kvol;
  int cin_pad;          // row length of a partial block: cin, or 16 for a reduction width below 16 (the first layer's 5 / 6)
  int nci_blk;          // blocks along cin
  // pair (efg_spconv_wgrad_tiled_pair_f32): the blocks [ny1, 2 ny1) of the launch are a SECOND layer of the same shape over the
  // same input rows, plan and schedule -- its gradient rows `go2`, its workspace `partial2` (ny1 = 0: one layer)
  const float* go2;
  float* partial2;
  int ny1;
};

// ---- schedule ---------------------------------------------------------------------------------------------------
// A unit of work is an ACTIVE (tile, offset) pair, and the offsets differ a lot: the centre of a 3 x 3 x 3 window has
// every tile active, a corner a fifth of them.  With one workgroup per (equal tile range, offset) the launch is 2.5
// rounds of workgroups whose lengths differ 5x: PMC on the 64-channel level -- wave slots occupied 60 % of the kernel's
// cycles, the matrix pipe 84 % busy while two waves share a SIMD, 50 % overall.  The schedule is the fix: per plan,
// computed on the device (no host round trip) and a pure function of the plan (reproducible): offset k gets
// S_k ~ T * U_k / sum U slots (U_k = its active tiles; T ~ one slot per 80 units) and its tiles are cut where the
// running count of ACTIVE tiles crosses j * U_k / S_k -- every slot of the launch has the same number of units.
// Slots of one offset are contiguous and in tile order (the reduction walks them in order); the order the workgroups
// are DISPATCHED in is a different one (wgt_order_kernel, below).
// The number of slots is fixed by the HOST from what it knows (tiles, window, the layer's block count, how many
// workgroups of the kernel the device holds at once): slots x blocks is a whole number of device fills -- with equal
// slots, a launch of 2 fills + 6 workgroups costs 3 (PMC: wave slots occupied 68 % of the 64-channel level's launch) --
// and the device deals exactly that many slots to the offsets by their unit counts (largest remainders).
// buffer: int4 dispatch[8 ceil(slots / 8)] | int kfirst[36] | int4 entry[slots]   (dispatch: wgt_order_kernel)
constexpr int kUnitsPerSlot = 80;
constexpr int kMaxSlots = 2048;

inline int sched_slots(long long n_tiles, int kvol, int nblk, int resident) {
  // ~0.55 of the (tile, offset) pairs of a submanifold window are active, fewer on strided tables: an estimate is enough,
  // it only sets the slot size
  const double want = (double)n_tiles * kvol * 0.55 / kUnitsPerSlot * nblk;      // workgroups
  const long long fills = std::max<long long>(1, (long long)(want / resident + 0.5));
  long long slots = fills * resident / nblk;
  slots = std::max<long long>(slots, kvol);
  return (int)std::min<long long>(slots, kMaxSlots);
}
inline int sched_dispatch(int slots) { return (slots + 7) / 8 * 8; }
__device__ inline int sched_dispatch_dev(int slots) { return (slots + 7) / 8 * 8; }
inline size_t sched_bytes(int slots) { return (size_t)sched_dispatch(slots) * 16 + 36 * 4 + (size_t)slots * 16; }

__global__ void __launch_bounds__(256) wgt_schedule_kernel(const unsigned* __restrict__ vm, long long n_tiles, int kvol, int slots,
                                                            int4* __restrict__ entry, int* __restrict__ kfirst) {
  __shared__ int U[32], S[32], KF[33];
  __shared__ int sm[17];
  __shared__ int lo[kMaxSlots + 8];
  constexpr int kStage = 8192;
  __shared__ unsigned wl[kStage];
  const int tid = threadIdx.x, k = blockIdx.x;
  if (tid < 32) U[tid] = 0;
  __syncthreads();
  // The tiles' active-offset words (vm[t][31]) are staged in LDS, 8 loads in flight per thread (one dependent 128-byte
  // strided load per loop trip had made this kernel 50 us); both passes read them there.
  auto stage = [&](long long c0, int cn) {
    for (int i0 = tid; i0 < cn; i0 += 256 * 8) {
      unsigned w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) w[u] = vm[(c0 + min(i0 + u * 256, cn - 1)) * 32 + 31];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (i0 + u * 256 < cn) wl[i0 + u * 256] = w[u];
    }
    __syncthreads();
  };
  // Pass 1: active tiles per offset (every workgroup counts all offsets: it needs the total).  Counters in registers, one
  // wave reduction and one LDS atomic per wave and offset (an LDS atomic per set bit: 64 lanes on <= 27 addresses).
  int cnt[31];
#pragma unroll
  for (int q = 0; q < 31; ++q) cnt[q] = 0;
  for (long long c0 = 0; c0 < n_tiles; c0 += kStage) {
    const int cn = (int)min((long long)kStage, n_tiles - c0);
    if (c0 > 0) __syncthreads();
    stage(c0, cn);
    for (int i = tid; i < cn; i += 256) {
      const unsigned w = wl[i];
#pragma unroll
      for (int q = 0; q < 31; ++q) cnt[q] += (int)((w >> q) & 1u);
    }
  }
#pragma unroll
  for (int q = 0; q < 31; ++q) {
    const int c = wave_reduce_sum(cnt[q]);
    if ((tid & 63) == 0 && c) atomicAdd(&U[q], c);
  }
  __syncthreads();
  if (tid < 64) {
    // Exactly `slots` slots (>= kvol) over the offsets, lane q = offset q: one slot for every offset that has units, the
    // rest in proportion to the unit counts (floor + largest remainder; ties: lowest offset) -- integer arithmetic, the same
    // on every workgroup (slots <= 2048 and U < 2^20: the products fit 32 bits).
    const int q = tid;
    const int uq = (q < kvol) ? U[q] : 0;
    const int total = wave_reduce_sum(uq);
    const int nact = wave_reduce_sum(uq > 0 ? 1 : 0);
    const int spare = slots - nact;
    const unsigned share = (unsigned)spare * (unsigned)uq;
    const int f = total > 0 ? (int)(share / (unsigned)total) : 0;
    const int r = total > 0 ? (int)(share % (unsigned)total) : 0;
    const int left = spare - wave_reduce_sum(f);   // < nact
    int rank = 0;   // offsets with units whose remainder comes before this one's
    for (int p = 0; p < 32; ++p) {
      const int rp = __shfl(r, p, 64), up = __shfl(uq, p, 64);
      if (up > 0 && (rp > r || (rp == r && p < q))) ++rank;
    }
    const int sq = uq > 0 ? 1 + f + (rank < left ? 1 : 0) : 0;
    const int inc = wave_inclusive_scan(sq);
    if (q < 32) S[q] = sq;
    if (q <= 32) KF[q] = inc - sq;   // KF[kvol] == slots (0 for an empty plan)
  }
  __syncthreads();
  const int sk = S[k];
  const unsigned uk = (unsigned)U[k];
  for (int j = tid; j <= sk; j += 256) lo[j] = (int)n_tiles;
  __syncthreads();
  // Pass 2: this workgroup's offset.  Rank r of its active tiles starts range j when j(r) != j(r - 1), j(r) = r S / U;
  // four consecutive tiles per thread and scan step.
  int carry = 0;
  for (long long c0 = 0; c0 < n_tiles; c0 += kStage) {
    const int cn = (int)min((long long)kStage, n_tiles - c0);
    if (n_tiles > kStage) {   // (a single chunk is still staged from pass 1)
      __syncthreads();
      stage(c0, cn);
    }
    for (int base = 0; base < cn; base += 1024) {
      const int i0 = base + tid * 4;
      int flag[4], mine = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        flag[u] = (i0 + u < cn) ? (int)((wl[i0 + u] >> k) & 1u) : 0;
        mine += flag[u];
      }
      int tot;
      int r = carry + block_exclusive_scan(mine, sm, &tot);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (flag[u]) {   // (sk >= 1 whenever uk > 0)
          const int j = (int)(((unsigned)r * (unsigned)sk) / uk);
          const int jp = r > 0 ? (int)(((unsigned)(r - 1) * (unsigned)sk) / uk) : -1;
          for (int jj = jp + 1; jj <= j; ++jj) lo[jj] = (int)(c0 + i0 + u);
          ++r;
        }
      carry += tot;
    }
  }
  __syncthreads();
  for (int j = tid; j < sk; j += 256) entry[KF[k] + j] = make_int4(k, lo[j], lo[j + 1], KF[k] + j);
  if (k == 0) {
    for (int q = tid; q <= kvol; q += 256) kfirst[q] = KF[q];
    for (int e = KF[kvol] + tid; e < slots; e += 256) entry[e] = make_int4(-1, 0x7fffffff, 0x7fffffff, e);
  }
}

// Dispatch order.  The slots of the table above are grouped by offset (the reduction needs that), but consecutive
// workgroups go round-robin to the 8 XCDs and every offset of a tile range reads the SAME grad_out rows and neighbouring
// input rows: launched in table order, each XCD's L2 sees every row once per offset it happens to draw -- PMC: 192 MB
// fetched past L2 per launch of the 64-channel kernel for ~21 MB of rows, 282-372 MB on the 16-channel level.  Here the
// slots are sorted by their first tile (all offsets together) and dealt in eighths: XCD x walks the x-th eighth of the
// rows in tile order with the offsets of a range next to each other in time (workgroup 8 q + x = q-th slot of the x-th
// eighth).  One workgroup, an LDS bitonic sort of <= 2048 keys.
__global__ void __launch_bounds__(1024) wgt_order_kernel(const int4* __restrict__ entry, int slots, int4* __restrict__ dispatch) {
  __shared__ unsigned long long key[kMaxSlots];
  const int tid = threadIdx.x;
  int n2 = 1;
  while (n2 < slots) n2 <<= 1;
  for (int i = tid; i < n2; i += 1024) {
    unsigned long long kx = ~0ull;
    if (i < slots) {
      const int4 e = entry[i];
      // empty ranges (and unused slots) last; ties: table order (offset, then range)
      const unsigned lo = (e.x >= 0 && e.z > e.y) ? (unsigned)e.y : 0x7fffffffu;
      kx = ((unsigned long long)lo << 16) | (unsigned)i;
    }
    key[i] = kx;
  }
  __syncthreads();
  for (int size = 2; size <= n2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += 1024) {
        const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
        const int j = i | stride;
        const unsigned long long x = key[i], y = key[j];
        if ((x > y) == ((i & size) == 0)) {
          key[i] = y;
          key[j] = x;
        }
      }
      __syncthreads();
    }
  const int d_n = sched_dispatch_dev(slots), per = d_n >> 3;
  for (int d = tid; d < d_n; d += 1024) dispatch[d] = make_int4(-1, 0, 0, 0);
  __syncthreads();
  for (int s = tid; s < slots; s += 1024) dispatch[8 * (s % per) + s / per] = entry[(int)(key[s] & 0xffffu)];
}

template <int NCO, int NCI>
__global__ void __launch_bounds__(256) conv_wgrad_tile_kernel(WgtArgs a) {
  constexpr int kAcc = NCO * NCI * 4;          // accumulator registers per lane
  static_assert((NCO == 4 || NCO == 2 || NCO == 1) && (NCI == 4 || NCI == 2 || NCI == 1), "block: 16 NCO x 16 NCI channels");
  typedef float VA __attribute__((ext_vector_type(NCO)));
  typedef float VB __attribute__((ext_vector_type(NCI)));
  constexpr int kGroup = 256;                  // tiles per pass over the range (<= 64 units per wave and pass)
  __shared__ float red[3][kAcc * 64];          // the partial blocks of waves 1..3
  __shared__ int lst[4][kGroup / 4];           // per wave: its active tiles of the current group
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int4 ent = a.entry[blockIdx.x];   // (the schedule: which offset, which tiles, which slot of the workspace)
  if (ent.x < 0) return;
  const bool second = a.ny1 > 0 && (int)blockIdx.y >= a.ny1;   // (uniform: the pair's second layer)
  const int k = ent.x, yb = second ? (int)blockIdx.y - a.ny1 : (int)blockIdx.y;
  const float* go = second ? a.go2 : a.go;
  const int co0 = (yb / a.nci_blk) * (NCO * 16), ci0 = (yb % a.nci_blk) * (NCI * 16);
  const int m = lane & 15, kk = lane >> 4;
  const int t_lo = ent.y, t_hi = ent.z;

  f32x4 acc[NCO][NCI];
#pragma unroll
  for (int ct = 0; ct < NCO; ++ct)
#pragma unroll
    for (int it = 0; it < NCI; ++it) acc[ct][it] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto load_idx = [&](int t, i32x4& ro, i32x4& rn) {
    ro = *reinterpret_cast<const i32x4*>(a.rows + (long long)t * 16 + kk * 4);
    rn = *reinterpret_cast<const i32x4*>(a.nb + ((long long)t * a.kvol + k) * 16 + kk * 4);
  };
  // operands of one unit, in fragment order; returns the validity of the lane's four pairs (an absent neighbour -- and
  // with it every padding row of the tile -- reads row 0 and is multiplied by zero).  The M / N index of the MFMA is a
  // free bijection onto the block's channels: tile t of the block holds channels {NC * m + t}, so that a lane's NC
  // operands of a K-step are NC CONSECUTIVE channels of its row -- one 16-byte (8-byte for 32 channels) load, and the 16
  // lanes of a row read its 256 bytes contiguously: 4 + 4 load instructions per unit instead of 16 + 16 four-byte gathers.
  auto load_data = [&](const i32x4& ro, const i32x4& rn, VA (&A)[4], VB (&B)[4]) -> unsigned {
    unsigned ok = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // 32-bit byte offsets (saddr + voffset loads; the host checks both tensors are below 4 GB)
      const unsigned ao = ((unsigned)max(ro[q], 0) * (unsigned)a.cout + (unsigned)(co0 + NCO * m)) * 4u;
      const unsigned bo = ((unsigned)max(rn[q], 0) * (unsigned)a.cin + (unsigned)min(ci0 + NCI * m, a.cin - NCI)) * 4u;
      A[q] = *reinterpret_cast<const VA*>(reinterpret_cast<const char*>(go) + ao);
      B[q] = *reinterpret_cast<const VB*>(reinterpret_cast<const char*>(a.in) + bo);
      ok |= (rn[q] >= 0 ? 1u : 0u) << q;
    }
    if (ci0 + NCI * m >= a.cin) ok = 0;   // (a reduction width below 16: the lanes past it multiply zeros)
    return ok;
  };
  auto mfmas = [&](const VA (&A)[4], const VB (&B)[4], unsigned ok) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float b[NCI];
#pragma unroll
      for (int t = 0; t < NCI; ++t) b[t] = ((ok >> q) & 1u) ? B[q][t] : 0.f;
#pragma unroll
      for (int ct = 0; ct < NCO; ++ct)
#pragma unroll
        for (int it = 0; it < NCI; ++it) acc[ct][it] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[q][ct], b[it], acc[ct][it], 0, 0, 0);
    }
  };

  // The range is walked in groups of kGroup tiles.  Phase 1: the wave's list of active tiles of the group at this offset
  // (lane l looks at the validity words of tiles l, l + 64, ..; ballot + popcount give each active tile its rank in the
  // workgroup's order, the four waves take every fourth) goes to a wave-private LDS list.  Phase 2: a register pipeline
  // two units deep over that list -- row numbers of unit u + 2 and operands of unit u + 1 in flight during the MFMAs of
  // unit u.  Every memory instruction of phase 2 is issued UNCONDITIONALLY (past the end of the list it repeats the
  // last unit's loads; only the MFMAs are skipped): with a load inside a branch the compiler can no longer count the
  // loads in flight at the join and waits for all of them (s_waitcnt vmcnt(0)) in front of every MFMA block -- measured:
  // the pipeline then does not overlap anything.
  VA A[2][4];
  VB B[2][4];
  i32x4 RO[2], RN[2];
  unsigned OK[2];
  int* my_list = lst[wv];
  for (int g0 = t_lo; g0 < t_hi; g0 += kGroup) {
    unsigned v[kGroup / 64];
#pragma unroll
    for (int j = 0; j < kGroup / 64; ++j) {
      const int t = g0 + j * 64 + lane;
      v[j] = a.vm[(long long)min(t, t_hi - 1) * 32 + k];
      if (t >= t_hi) v[j] = 0u;
    }
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < kGroup / 64; ++j) {
      const unsigned long long mask = __ballot(v[j] != 0u);
      const int rank = cnt + __popcll(mask & ((1ull << lane) - 1ull));
      if (v[j] != 0u && (rank & 3) == wv) my_list[rank >> 2] = g0 + j * 64 + lane;
      cnt += __popcll(mask);
    }
    const int n = (cnt + 3 - wv) >> 2;   // this wave's units of the group (wave-uniform)
    __builtin_amdgcn_wave_barrier();
    if (n == 0) continue;
    auto unit = [&](int u) { return my_list[min(u, n - 1)]; };
    load_idx(unit(0), RO[0], RN[0]);
    load_idx(unit(1), RO[1], RN[1]);
    OK[0] = load_data(RO[0], RN[0], A[0], B[0]);
    for (int u = 0; u < n; u += 2) {
      // (the scheduling barriers keep the loads IN FRONT of the MFMA block: left alone, the scheduler sinks them to the end
      // of the block to shorten live ranges, and every second unit then waits out a full memory latency)
      OK[1] = load_data(RO[1], RN[1], A[1], B[1]);   // unit u + 1
      load_idx(unit(u + 2), RO[0], RN[0]);           // unit u + 2
      __builtin_amdgcn_sched_barrier(0);
      mfmas(A[0], B[0], OK[0]);
      __builtin_amdgcn_sched_barrier(0);
      OK[0] = load_data(RO[0], RN[0], A[0], B[0]);   // unit u + 2
      load_idx(unit(u + 3), RO[1], RN[1]);           // unit u + 3
      __builtin_amdgcn_sched_barrier(0);
      if (u + 1 < n) mfmas(A[1], B[1], OK[1]);
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_wave_barrier();   // the list is rewritten by the next group
  }

  // the four waves' blocks, summed in wave order
  if (wv > 0) {
#pragma unroll
    for (int ct = 0; ct < NCO; ++ct)
#pragma unroll
      for (int it = 0; it < NCI; ++it)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wv - 1][((ct * NCI + it) * 4 + r) * 64 + lane] = acc[ct][it][r];
  }
  __syncthreads();
  if (wv > 0) return;
  float* p = (second ? a.partial2 : a.partial) + (long long)ent.w * a.cout * a.cin_pad;
  // C/D layout of 16x16x4: M = (lane >> 4) * 4 + reg, N = lane & 15; with the channel bijection of load_data
  // co = co0 + NCO * M + ct and ci = ci0 + NCI * N + it: a lane's NCI values of (ct, reg) are consecutive in memory
#pragma unroll
  for (int ct = 0; ct < NCO; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      VB v;
#pragma unroll
      for (int it = 0; it < NCI; ++it) {
        const int e = ((ct * NCI + it) * 4 + r) * 64 + lane;
        v[it] = ((acc[ct][it][r] + red[0][e]) + red[1][e]) + red[2][e];
      }
      const int co = co0 + NCO * (kk * 4 + r) + ct;
      *reinterpret_cast<VB*>(p + (long long)co * a.cin_pad + ci0 + NCI * m) = v;
    }
}

// gw[co][k][ci] = sum over the slots of offset k of partial[slot][co][ci], in slot order; 4 consecutive ci per thread
// (partial rows are cin_pad long: 16 for a reduction width below 16)
__global__ void __launch_bounds__(256) wgt_reduce_kernel(const float* __restrict__ partial,
                                                          const int* __restrict__ kfirst, int kvol, int cout, int cin, int cin_pad,
                                                          float* __restrict__ gw, const float* __restrict__ partial2,
                                                          float* __restrict__ gw2) {
  __shared__ f32x4 sm[4][64];
  const long long blk = (long long)cout * cin_pad, per = (long long)kvol * blk;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (blockIdx.y) {   // (a pair's second layer: the same fold over its own workspace)
    partial = partial2;
    gw = gw2;
  }
  const long long e = ((long long)blockIdx.x * 64 + lane) * 4;   // (k, co, ci); blk is a multiple of 256: k is block-uniform
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
  int k = 0;
  long long rem = 0;
  if (e < per) {
    k = (int)(e / blk);
    rem = e - (long long)k * blk;
    const int s_end = kfirst[k + 1];
    int sp = kfirst[k] + wv;
    auto term = [&](int slot) { return *reinterpret_cast<const f32x4*>(partial + (long long)slot * blk + rem); };
    for (; sp + 4 < s_end; sp += 8) {   // two loads in flight
      s0 += term(sp);
      s1 += term(sp + 4);
    }
    for (; sp < s_end; sp += 4) s0 += term(sp);
  }
  sm[wv][lane] = s0 + s1;
  __syncthreads();
  if (wv == 0 && e < per) {
    const f32x4 s = (sm[0][lane] + sm[1][lane]) + (sm[2][lane] + sm[3][lane]);
    const int co = (int)(rem / cin_pad), ci = (int)(rem - (long long)co * cin_pad);
    float* g = gw + ((long long)co * kvol + k) * cin + ci;
    if (cin_pad == cin) {
      *reinterpret_cast<f32x4*>(g) = s;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (ci + u < cin) g[u] = s[u];
    }
  }
}

// Covered: output widths of 16, 32 or a multiple of 64; reduction widths of 1 .. 16 (the first layer's 5 / 6 point features:
// one 16-wide tile whose lanes past the width multiply zeros), 32 or a multiple of 64 -- every convolution of the res18 /
// res34 and CenterPoint backbones.
bool wgt_width_ok(int c) { return c == 16 || c == 32 || (c >= 64 && c % 64 == 0); }
bool wgt_ok(int cin, int cout, int kvol) {
  return kvol >= 1 && kvol <= kSpconvMaxKvol && wgt_width_ok(cout) && ((cin >= 1 && cin <= 16) || wgt_width_ok(cin));
}
inline int wgt_tiles(int c) { return c >= 64 ? 4 : (c + 15) / 16; }   // 16-channel tiles of a block along one side
inline int wgt_cin_pad(int cin) { return cin < 16 ? 16 : cin; }

// workgroups of `kernel` the device holds at once
template <typename K>
int resident_workgroups(K kernel) {
  int per_cu = 0, dev = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1) per_cu = 2;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
    cus = 256;
  return per_cu * cus;
}

struct WgtLayout {
  int slots, nco_blk, nci_blk;
  size_t bytes;
};

// the (NCO, NCI) instantiation of a layer: f(kernel) for its kernel
template <typename F>
auto with_kernel(int cin, int cout, F f) {
  const int nco = wgt_tiles(cout), nci = wgt_tiles(cin);
#define EFG_WGT_CASE(A, B) \
  if (nco == A && nci == B) return f(conv_wgrad_tile_kernel<A, B>);
  EFG_WGT_CASE(4, 4) EFG_WGT_CASE(4, 2) EFG_WGT_CASE(4, 1) EFG_WGT_CASE(2, 4) EFG_WGT_CASE(2, 2) EFG_WGT_CASE(2, 1)
  EFG_WGT_CASE(1, 4) EFG_WGT_CASE(1, 2)
#undef EFG_WGT_CASE
  return f(conv_wgrad_tile_kernel<1, 1>);
}

// ONE definition of the slot count of a (rows, window, channels) layer for the schedule, the workspace and the launch
WgtLayout wgt_layout(int64_t m_out, int cin, int cout, int kvol) {
  static int resident[5][5] = {};   // per (NCO, NCI): workgroups the device holds (asked once)
  const int nco = wgt_tiles(cout), nci = wgt_tiles(cin);
  if (!resident[nco][nci]) resident[nco][nci] = with_kernel(cin, cout, [](auto kern) { return resident_workgroups(kern); });
  WgtLayout L;
  L.nco_blk = cout >= 64 ? cout / 64 : 1;
  L.nci_blk = cin >= 64 ? cin / 64 : 1;
  L.slots = sched_slots(plan_tiles(m_out), kvol, L.nco_blk * L.nci_blk, resident[nco][nci]);
  L.bytes = (size_t)L.slots * cout * wgt_cin_pad(cin) * 4;
  return L;
}

}  // namespace
}  // namespace efg

using namespace efg;

extern "C" int efg_spconv_wgrad_tiled_ok(int cin, int cout, int kvol) { return wgt_ok(cin, cout, kvol) ? 1 : 0; }

extern "C" size_t efg_spconv_wgrad_tiled_workspace_bytes(int64_t m_out, int cin, int cout, int kvol) {
  if (m_out < 0 || !wgt_ok(cin, cout, kvol)) return 0;
  return wgt_layout(m_out, cin, cout, kvol).bytes + 256;
}

extern "C" size_t efg_spconv_wgrad_sched_bytes(int64_t m_out, int cin, int cout, int kvol) {
  if (m_out < 0 || !wgt_ok(cin, cout, kvol)) return 0;
  return sched_bytes(wgt_layout(m_out, cin, cout, kvol).slots) + 256;
}

extern "C" int efg_spconv_wgrad_sched(const void* plan, int64_t m_out, int cin, int cout, int kvol, void* sched,
                                      size_t sched_bytes_given, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  // (the schedule kernel multiplies tile counts in 32 bits: fewer than 2^21 16-row tiles)
  EFG_CHECK_ARG(m_out >= 0 && m_out < (1ll << 25) && wgt_ok(cin, cout, kvol), "wgrad_sched: bad sizes (m=%lld, %d -> %d, kvol=%d)",
                (long long)m_out, cin, cout, kvol);
  if (m_out == 0) return EFG_OK;
  const int slots = wgt_layout(m_out, cin, cout, kvol).slots;
  EFG_CHECK_ARG(plan && sched && sched_bytes_given >= sched_bytes(slots), "wgrad_sched: null pointer / buffer too small");
  EFG_CHECK_ARG((reinterpret_cast<uintptr_t>(sched) & 15) == 0, "wgrad_sched: buffer must be 16-byte aligned");
  const PlanView pv = plan_view(const_cast<void*>(plan), m_out, kvol);
  int4* dispatch = static_cast<int4*>(sched);
  int* kfirst = reinterpret_cast<int*>(dispatch + sched_dispatch(slots));
  int4* entry = reinterpret_cast<int4*>(kfirst + 36);
  hipLaunchKernelGGL(wgt_schedule_kernel, dim3(kvol), dim3(256), 0, stream, pv.vm, pv.n_tiles, kvol, slots, entry, kfirst);
  // (dispatched in table order instead: the losing A/B arm of round 3, profiles/r03_wgrad_dispatch_order_ab.txt)
  hipLaunchKernelGGL(wgt_order_kernel, dim3(1), dim3(1024), 0, stream, entry, slots, dispatch);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}

namespace {
int run_wgrad_tiled(const float* in_feat, int64_t m_in, int cin, const float* grad_out, const float* grad_out2, int64_t m_out,
                    int cout, int kvol, const void* plan, const void* sched, float* grad_w, float* grad_w2, void* ws,
                    size_t ws_bytes, hipStream_t stream) {
  const bool pair = grad_out2 != nullptr;
  EFG_CHECK_ARG(wgt_ok(cin, cout, kvol), "spconv wgrad tiled: %d -> %d channels, kvol %d not covered (ask efg_spconv_wgrad_tiled_ok)",
                cin, cout, kvol);
  EFG_CHECK_ARG(m_in >= 0 && m_out >= 0 && (unsigned long long)m_in * cin * 4ull < (1ull << 32) &&
                    (unsigned long long)m_out * cout * 4ull < (1ull << 32),
                "spconv wgrad tiled: feature tensors must be smaller than 4 GB");
  const size_t gw_bytes = (size_t)cout * kvol * cin * 4;
  if (m_out == 0 || m_in == 0) {
    EFG_HIP_TRY(hipMemsetAsync(grad_w, 0, gw_bytes, stream));
    if (pair) EFG_HIP_TRY(hipMemsetAsync(grad_w2, 0, gw_bytes, stream));
    return EFG_OK;
  }
  EFG_CHECK_ARG(plan && sched && in_feat && grad_out && grad_w && (!pair || grad_w2), "spconv wgrad tiled: null pointer");
  EFG_CHECK_ARG((reinterpret_cast<uintptr_t>(in_feat) & 15) == 0 && (reinterpret_cast<uintptr_t>(grad_out) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(grad_out2) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(ws) & 15) == 0 && (reinterpret_cast<uintptr_t>(plan) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(sched) & 15) == 0,
                "spconv wgrad tiled: feature tensors, plan, schedule and workspace must be 16-byte aligned");
  const WgtLayout L = wgt_layout(m_out, cin, cout, kvol);
  const size_t need = pair ? 2 * align_up(L.bytes, 256) : L.bytes;
  if (!ws || ws_bytes < need) {
    set_error("spconv wgrad tiled workspace too small: need %zu bytes, got %zu", need + 256, ws_bytes);
    return EFG_E_WORKSPACE;
  }
  const PlanView pv = plan_view(const_cast<void*>(plan), m_out, kvol);
  WgtArgs a;
  a.in = in_feat;
  a.go = grad_out;
  a.rows = pv.rows;
  a.nb = pv.nb;
  a.vm = pv.vm;
  a.entry = static_cast<const int4*>(sched);
  a.partial = static_cast<float*>(ws);
  a.n_tiles = pv.n_tiles;
  a.cin = cin;
  a.cout = cout;
  a.kvol = kvol;
  a.cin_pad = wgt_cin_pad(cin);
  a.nci_blk = L.nci_blk;
  a.go2 = grad_out2;
  a.partial2 = pair ? reinterpret_cast<float*>(static_cast<char*>(ws) + align_up(L.bytes, 256)) : nullptr;
  a.ny1 = pair ? L.nco_blk * L.nci_blk : 0;
  const dim3 grid(sched_dispatch(L.slots), L.nco_blk * L.nci_blk * (pair ? 2 : 1));
  with_kernel(cin, cout, [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, a);
    return 0;
  });
  EFG_LAUNCH_CHECK();
  const long long per = (long long)kvol * cout * a.cin_pad;
  const int* kfirst = reinterpret_cast<const int*>(a.entry + sched_dispatch(L.slots));
  hipLaunchKernelGGL(wgt_reduce_kernel, dim3((unsigned)ceil_div(per, 256), pair ? 2 : 1), dim3(256), 0, stream, a.partial, kfirst,
                     kvol, cout, cin, a.cin_pad, grad_w, a.partial2, grad_w2);
  EFG_LAUNCH_CHECK();
  return EFG_OK;
}
}  // namespace

extern "C" int efg_spconv_wgrad_tiled_f32(const float* in_feat, int64_t m_in, int cin, const float* grad_out, int64_t m_out,
                                          int cout, int kvol, const void* plan, const void* sched, float* grad_w, void* ws,
                                          size_t ws_bytes, void* stream_) {
  return run_wgrad_tiled(in_feat, m_in, cin, grad_out, nullptr, m_out, cout, kvol, plan, sched, grad_w, nullptr, ws, ws_bytes,
                         (hipStream_t)stream_);
}

extern "C" int efg_spconv_wgrad_tiled_pair_f32(const float* in_feat, int64_t m_in, int cin, const float* grad_out_a,
                                               const float* grad_out_b, int64_t m_out, int cout, int kvol, const void* plan,
                                               const void* sched, float* grad_w_a, float* grad_w_b, void* ws, size_t ws_bytes,
                                               void* stream_) {
  EFG_CHECK_ARG(grad_out_b && grad_w_b, "spconv wgrad tiled pair: null pointer");
  return run_wgrad_tiled(in_feat, m_in, cin, grad_out_a, grad_out_b, m_out, cout, kvol, plan, sched, grad_w_a, grad_w_b, ws,
                         ws_bytes, (hipStream_t)stream_);
}
