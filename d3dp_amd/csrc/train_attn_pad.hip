// The padded-head forms of the training attention kernels (head dims 24 and 40 / 48 / 56 in the images of 32 and 64: `-cs` 192 and
// 320 / 384 / 448 under D3DP_TRAIN_IMPL=f16x2) as a translation unit of their own: the kernels are the templates of train_attn.hip with
// PAD = true, and d3dp_train_attn_x2_padded is all this file exports to the library.  Apart from them the existing instantiations of
// train_attn.hip keep their device code, and the two files compile side by side.
#define D3DP_TA_PAD_TU 1
#include "train_attn.hip"
