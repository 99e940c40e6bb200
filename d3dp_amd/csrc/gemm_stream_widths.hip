// The streaming 2-byte Linear (gemm.hip gemm_bf16_stream_kernel) at the k-depths of channels 192 / 320 / 384 / 448 -- K / 64 in
// {3, 5, 6, 7} for qkv and fc1, {6, 10, 12, 14} for fc2 -- for FAST / FAST16 contexts under D3DP_FAST_IMPL=mfma, as a translation unit
// of its own: the kernels are the template of gemm.hip at new NK, and d3dp_linear_stream_widths is all this file exports to the
// library.  Apart from them the existing instantiations of gemm.hip keep their device code, and the two files compile side by side.
#define D3DP_STREAM_WIDTHS_TU 1
#include "gemm.hip"
