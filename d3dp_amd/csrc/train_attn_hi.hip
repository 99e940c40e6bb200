// The forward kernels of the training attention that write the proj Linear's operand as hi-only rows (D3DP_TRAIN_ROWS=hi: OPHI = true;
// head dims 64 / 32 at both pass counts) as a translation unit of their own: the kernels are the templates of train_attn.hip, and
// d3dp_train_attn_x2_fwd_hi is all this file exports to the library.  Apart from them the existing instantiations of train_attn.hip,
// train_attn_pad.hip and train_attn_1p.hip keep their device code, and the four files compile side by side.
#define D3DP_TA_HI_TU 1
#include "train_attn.hip"
