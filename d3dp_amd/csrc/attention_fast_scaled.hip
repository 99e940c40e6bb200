// The scaled forms of the FAST16 attention kernels (q, k and v rows at a power-of-two multiple 2^-s of their value: FAST16 contexts under
// D3DP_FAST16_RANGE=scale, head dims 64 / 32 / 16) as a translation unit of their own: the kernels are the templates of attention_fast.hip
// with the exponent scale as a run-time argument, and d3dp_attn_fast_scaled is all this file exports to the library.  The existing
// instantiations of attention_fast.hip keep their device code, and the files compile side by side.
#define D3DP_FAST_SCALED_TU 1
#include "attention_fast.hip"
