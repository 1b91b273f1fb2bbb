// Split-precision GEMM for the A/B arm of the bench (EFG_GEMM_ARM=bf16x3; NOT the headline path, which stays exact fp32):
// gemm_split_bf16.h with TWO bf16 pieces per operand, x = hi + lo (16 of the 24 significand bits), and three bf16 MFMA
// products accumulated in fp32:  lo.hi + hi.lo + hi.hi  (lo.lo, 2^-16 of the result, is dropped).  fp32-input MFMA peaks at
// 157 TFLOP/s on gfx950 and bf16 at 2.5 PFLOP/s: three bf16 products cost 3/16 of the fp32 product, which turns the encoder's
// [70 688 x 256] x [256 x {256, 1024}] products from MFMA-bound (83 / 300 us in hipBLASLt fp32, 71-80 % of that peak) into
// HBM-bound ones.  One 32 KB LDS stage, 4 bytes per packed weight element.
#include "gemm_split_bf16.h"

namespace efg {
namespace {

constexpr int kPieces = 2;

__global__ void __launch_bounds__(256) gemm_bf16x3_pack_kernel(const float* __restrict__ w, long long sk, long long sn, int k,
                                                               int n, int kp, int np, __bf16* __restrict__ out) {
  pack_body<kPieces>(w, sk, sn, k, n, kp, np, out);
}

__global__ void __launch_bounds__(256) gemm_bf16x3_pack_linear_kernel(const float* __restrict__ w, int n_out, int n_in,
                                                                      __bf16* __restrict__ fwd, __bf16* __restrict__ dgrad) {
  pack_linear_body<kPieces>(w, n_out, n_in, fwd, dgrad);
}

__global__ void __launch_bounds__(256) gemm_bf16x3_kernel(GemmArgs g) { gemm_body<kPieces>(g); }

__global__ void __launch_bounds__(256) gemm_bf16x3_tn_kernel(WgradArgs a) { wgrad_body<kPieces>(a); }

__global__ void __launch_bounds__(256) gemm_bf16x3_tn_reduce_kernel(const float* __restrict__ part, int chunks, long long elems,
                                                                    float* __restrict__ out) {
  wgrad_reduce_body(part, chunks, elems, out);
}

constexpr SplitArm kArm = {"gemm_bf16x3", gemm_bf16x3_pack_kernel, gemm_bf16x3_pack_linear_kernel, gemm_bf16x3_kernel,
                           gemm_bf16x3_tn_kernel, gemm_bf16x3_tn_reduce_kernel};

}  // namespace
}  // namespace efg

using namespace efg;

extern "C" size_t efg_gemm_bf16x3_pack_bytes(int k, int n) { return pack_bytes<kPieces>(k, n); }

extern "C" int efg_gemm_bf16x3_pack_f32(const float* w, int64_t stride_k, int64_t stride_n, int k, int n, void* packed,
                                        void* stream) {
  return pack(kArm, w, stride_k, stride_n, k, n, packed, stream);
}

extern "C" int efg_gemm_bf16x3_pack_linear_f32(const float* w, int n_out, int n_in, void* packed_fwd, void* packed_dgrad,
                                               void* stream) {
  return pack_linear(kArm, w, n_out, n_in, packed_fwd, packed_dgrad, stream);
}

extern "C" int efg_gemm_bf16x3_f32(const float* a, int64_t m, int k, int64_t lda, const void* packed_b, int n,
                                   const float* bias, int relu, float* c, int64_t ldc, void* stream) {
  return gemm(kArm, a, m, k, lda, packed_b, n, bias, relu, c, ldc, stream);
}

extern "C" size_t efg_gemm_bf16x3_wgrad_workspace_bytes(int64_t m, int n, int k) { return wgrad_workspace_bytes(m, n, k); }

extern "C" int efg_gemm_bf16x3_wgrad_f32(const float* g, int64_t ldg, const float* x, int64_t ldx, int64_t m, int n, int k,
                                         float* dw, void* ws, size_t ws_bytes, void* stream) {
  return wgrad(kArm, g, ldg, x, ldx, m, n, k, dw, ws, ws_bytes, stream);
}
