// The streaming 2-byte Linear (gemm.hip gemm_bf16_stream_kernel) with the SCALED epilogue of FAST16 contexts under
// D3DP_FAST16_RANGE=scale -- fp16 operands and rows, K / 64 in {1, 2, 4, 8, 16} -- as a translation unit of its own: the kernels are the
// template of gemm.hip with the epilogue's three power-of-two multipliers as by-value arguments, and d3dp_linear_stream_scaled is
// all this file exports to the library.  The existing instantiations of gemm.hip keep their device code, and the files compile
// side by side.
#define D3DP_STREAM_SCALED_TU 1
#include "gemm.hip"
