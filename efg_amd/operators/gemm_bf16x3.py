"""Split-precision (bf16 x 3) products for the A/B arm of the bench -- csrc/gemm_bf16x3.hip (csrc/gemm_split_bf16.h with two
pieces per operand) through the C ABI; the functions are operators/gemm_split.py's.

Never the default: `EFG_GEMM_ARM=bf16x3` swaps it in for the forward and the data-gradient product of the encoder-sized
`nn.Linear` layers (operators/linear.py) -- forward, data gradient and (via `wgrad`) the weight gradient; everything
else stays exact fp32."""
from .gemm_split import bind

pack, pack_linear, pack_linear_both, gemm, wgrad = bind("efg_gemm_bf16x3")
