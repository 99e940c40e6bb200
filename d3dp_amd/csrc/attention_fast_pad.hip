// The padded-head forms of the FAST / FAST16 attention kernels (head dims 24 and 40 / 48 / 56 in rows padded to 32 and 64: `-cs` 192 and
// 320 / 384 / 448 under D3DP_FAST_IMPL=mfma) as a translation unit of their own: the kernels are the templates of attention_fast.hip with
// the true head dim as one more parameter, and d3dp_attn_fast_padded is all this file exports to the library.  Apart from them the
// existing instantiations of attention_fast.hip keep their device code, and the two files compile side by side.
#define D3DP_FAST_PAD_TU 1
#include "attention_fast.hip"
