"""fp32-equivalent split-precision (bf16 x 6) products -- csrc/gemm_bf16x6.hip (csrc/gemm_split_bf16.h with three pieces per
operand) through the C ABI; the functions are operators/gemm_split.py's.

Never the default: `EFG_GEMM_ARM=bf16x6` swaps it in where `EFG_GEMM_ARM=bf16x3` swaps operators/gemm_bf16x3.py in
(operators/linear.py, the neck's 3 x 3 convolution in operators/conv2d.py), with the same functions and signatures.  Three
bf16 pieces per operand hold all 24 significand bits and six MFMA products are summed in fp32: the error of an fp32
product (tests/test_gemm_bf16x6_gpu.py) at twice the matrix work of the x3 arm.  The packed layouts of the two modules
differ (three pieces per element here): a buffer packed by one is not an argument for the other."""
from .gemm_split import bind

pack, pack_linear, pack_linear_both, gemm, wgrad = bind("efg_gemm_bf16x6")
