// Heading-aware 3-D GIoU of 7-DoF boxes (cx, cy, cz, l, w, h, rad) for direct use: a paired forward / backward over
// rot_giou3d() of giou3d.h, one thread per pair.  The matching cost and the box loss take the same function through
// det_loss.hip.
#include "common.h"
#include "giou3d.h"

namespace efg {
namespace {

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
