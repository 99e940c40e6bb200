// The one-pass forms of the training attention kernels (D3DP_TRAIN_ATTN_PASSES=1: every product -- S, O, dP, dQ, dK, dV -- as ONE
// fp16-MFMA pass on operands rounded once to fp16 at their scale, one-plane LDS images; head dims 64 / 32 / 16) as a translation
// unit of their own: the kernels are the templates of train_attn.hip with PASSES = 1, and d3dp_train_attn_x2_1p is all this file
// exports to the library.  Apart from them the existing instantiations of train_attn.hip and train_attn_pad.hip keep their device
// code, and the three files compile side by side.
#define D3DP_TA_1P_TU 1
#include "train_attn.hip"
