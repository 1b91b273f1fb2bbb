// fp32-EQUIVALENT split-precision GEMM (EFG_GEMM_ARM=bf16x6; the sibling of gemm_bf16x3.hip, same contract, same tiling):
// gemm_split_bf16.h with THREE bf16 pieces per operand, x = p0 + p1 + p2 exactly (3 x 8 = all 24 significand bits), and the
// SIX leading bf16 MFMA products accumulated in fp32:
//   p0.p0  +  p0.p1 + p1.p0  +  p0.p2 + p1.p1 + p2.p0        (orders 1, 2^-8, 2^-16 of the result)
// The three dropped products (p1.p2, p2.p1, p2.p2) are 2^-24 and below: under the rounding of the fp32 accumulator itself.
// Six bf16 products cost 6/16 of the fp32 MFMA time and twice the MFMA work of gemm_bf16x3.hip.  One 48 KB LDS stage (A
// image 24 KB + B image 24 KB), 6 bytes per packed weight element; per k-step a wave reads 12 fragments for 24 MFMAs.
#include "gemm_split_bf16.h"

namespace efg {
namespace {

constexpr int kPieces = 3;

__global__ void __launch_bounds__(256) gemm_bf16x6_pack_kernel(const float* __restrict__ w, long long sk, long long sn, int k,
                                                               int n, int kp, int np, __bf16* __restrict__ out) {
  pack_body<kPieces>(w, sk, sn, k, n, kp, np, out);
}

__global__ void __launch_bounds__(256) gemm_bf16x6_pack_linear_kernel(const float* __restrict__ w, int n_out, int n_in,
                                                                      __bf16* __restrict__ fwd, __bf16* __restrict__ dgrad) {
  pack_linear_body<kPieces>(w, n_out, n_in, fwd, dgrad);
}

__global__ void __launch_bounds__(256) gemm_bf16x6_kernel(GemmArgs g) { gemm_body<kPieces>(g); }

// (waves_per_eu: left alone the compiler takes 172 registers, one granule over the 168 of three waves per SIMD -- three
// workgroups per CU is what the 48 KB stage allows; at 168 it spills nothing)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) gemm_bf16x6_tn_kernel(WgradArgs a) {
  wgrad_body<kPieces>(a);
}

__global__ void __launch_bounds__(256) gemm_bf16x6_tn_reduce_kernel(const float* __restrict__ part, int chunks, long long elems,
                                                                    float* __restrict__ out) {
  wgrad_reduce_body(part, chunks, elems, out);
}

constexpr SplitArm kArm = {"gemm_bf16x6", gemm_bf16x6_pack_kernel, gemm_bf16x6_pack_linear_kernel, gemm_bf16x6_kernel,
                           gemm_bf16x6_tn_kernel, gemm_bf16x6_tn_reduce_kernel};

}  // namespace
}  // namespace efg

using namespace efg;

extern "C" size_t efg_gemm_bf16x6_pack_bytes(int k, int n) { return pack_bytes<kPieces>(k, n); }

extern "C" int efg_gemm_bf16x6_pack_f32(const float* w, int64_t stride_k, int64_t stride_n, int k, int n, void* packed,
                                        void* stream) {
  return pack(kArm, w, stride_k, stride_n, k, n, packed, stream);
}

extern "C" int efg_gemm_bf16x6_pack_linear_f32(const float* w, int n_out, int n_in, void* packed_fwd, void* packed_dgrad,
                                               void* stream) {
  return pack_linear(kArm, w, n_out, n_in, packed_fwd, packed_dgrad, stream);
}

extern "C" int efg_gemm_bf16x6_f32(const float* a, int64_t m, int k, int64_t lda, const void* packed_b, int n,
                                   const float* bias, int relu, float* c, int64_t ldc, void* stream) {
  return gemm(kArm, a, m, k, lda, packed_b, n, bias, relu, c, ldc, stream);
}

extern "C" size_t efg_gemm_bf16x6_wgrad_workspace_bytes(int64_t m, int n, int k) { return wgrad_workspace_bytes(m, n, k); }

extern "C" int efg_gemm_bf16x6_wgrad_f32(const float* g, int64_t ldg, const float* x, int64_t ldx, int64_t m, int n, int k,
                                         float* dw, void* ws, size_t ws_bytes, void* stream) {
  return wgrad(kArm, g, ldg, x, ldx, m, n, k, dw, ws, ws_bytes, stream);
}
