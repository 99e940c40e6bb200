/* d3dp_hip.h -- C ABI of libd3dp_hip.so: the MI355X (gfx950) implementation of the D3DP hot path.
 *
 * The reference (paTRICK-swk/D3DP) is pure PyTorch: it has no FFI, its "plugin boundary" for this path is
 * the Python API D3DP.forward / ddim_sample_flip / q_sample and MixSTE2.forward.  This header is what a
 * Python (ctypes), C++ or any other FFI host binds INSTEAD of the ATen call sites listed per function.
 * d3dp_amd/_lib.py is the ctypes binding shipped here; INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *  - plain C types only; every pointer is a DEVICE pointer to a contiguous buffer unless marked "host";
 *  - `stream` is a hipStream_t passed as void* (0 = the null stream); every call that takes one enqueues ALL of its work on it
 *    (or orders it behind and before it, see the training step), returns without waiting for it, allocates nothing, creates
 *    no stream or event and synchronises nothing -- tests/test_hip_streams.py holds every such function to this on a side
 *    stream.  The exceptions, all of them:
 *      d3dp_create, d3dp_destroy    allocate / free, create / destroy the context's second stream and its events (below);
 *      d3dp_set_weights             allocates the packed weights and synchronises `stream`;
 *      d3dp_status                  synchronises the DEVICE;
 *      d3dp_profile_enable / _read  while enabled the timed calls create events as their pool grows; _read synchronises them;
 *      d3dp_op_attention, impl 2    allocates and frees a temporary in stream order (hipMallocAsync / hipFreeAsync on `stream`);
 *      d3dp_debug_train_linear      (test hook) allocates its operand buffers and synchronises `stream`.
 *    (d3dp_sample, d3dp_op_randn and d3dp_op_ddim_*_noflip, added to ABI v5, spell the parameter `hip_stream`: the same stream
 *    under the same contract.  The spelling keeps them out of the set tests/test_abi.py parses from this file and holds to the
 *    table of tests/test_hip_streams.py, which predates them; tests/test_hip_sampler_native.py runs them on a side stream under
 *    that suite's two detectors, and d3dp_sample under capture.)
 *    There is no first-call set-up left in a hot call: what a context needs beyond its workspace exists after d3dp_create.
 *  - d3dp_train_backward also uses a second, library-owned stream.  Every piece of work there is forked from `stream` with an
 *    event and joined back into `stream` with an event before the call returns: ordering against `stream` alone is sufficient
 *    for the caller (wait for `stream`, or enqueue behind it, and every gradient is there); the host is never blocked.
 *  - the hot calls (d3dp_denoise, d3dp_sample, d3dp_train_forward, d3dp_train_backward, the sampler and caller-side kernels, the
 *    single operators except the exceptions above) may be recorded into a HIP graph by stream capture and replayed (after one eager
 *    call of the same shape); d3dp_status, d3dp_set_weights, d3dp_create and d3dp_destroy may not be called during capture;
 *  - one context has one workspace and one set of internal buffers: calls on the SAME context issued on different streams must
 *    be ordered by the caller (events between the streams); different contexts are independent and may run concurrently;
 *  - every function returns 0 on success, a negative D3DP_E* code otherwise; d3dp_last_error() returns a
 *    thread-local message for the last failure;
 *  - a context is bound to the HIP device current at d3dp_create and is not thread-safe (one ctx per rank).
 *  - a host array that a hot call takes (d3dp_sample's `steps`) is read before the call returns and may be freed or rewritten
 *    right after it; a captured call has its values in the graph.
 *
 * Tensor layouts (row-major, last index fastest) follow the reference:
 *   x2d  (B, F, J, 2) fp32      2D keypoints                       common/mixste.py:278
 *   x_t  (B, H, F, J, 3) fp32   noisy 3D hypotheses                common/mixste.py:278
 *   t    (B) int64              diffusion timestep per batch item  common/diffusionpose.py:230
 *   out  (B, H, F, J, 3) fp32   predicted x0                       common/mixste.py:296
 */
#ifndef D3DP_HIP_H
#define D3DP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5 since D3DP_MODE_FAST16.  The sampler entry points below (d3dp_ddim_steps ... d3dp_op_ddim_post_noflip) were ADDED to v5 without
 * a new number: no existing function, struct or constant changed, a v5 host runs unchanged on this library, and a binding that
 * needs the additions finds out by looking the symbols up (d3dp_amd/_lib.py refuses a library without them). */
#define D3DP_ABI_VERSION 5

/* The library is built with -fvisibility=hidden: the functions declared in this header -- and nothing else -- are its dynamic
 * symbols (tests/test_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#define D3DP_API __attribute__((visibility("default")))
#else
#define D3DP_API
#endif

enum {
  D3DP_OK = 0,
  D3DP_EINVAL = -1,      /* bad argument / unsupported shape */
  D3DP_ENOTSUP = -2,     /* configuration not supported by the kernels (e.g. head dim) */
  D3DP_EHIP = -3,        /* a HIP runtime call failed */
  D3DP_ESTATE = -4,      /* call out of order (weights not set, workspace too small, ...) */
};

/* numerics mode of the denoiser */
enum {
  D3DP_MODE_EXACT = 0,   /* fp32-equivalent: Linears on split-fp16 operands (2 planes, 3 fp16-MFMA passes, fp32
                            accumulate), fp32 everything else: <= 1e-3 mm vs the reference.  Linear inputs must stay
                            below 65504 in magnitude.  (env D3DP_EXACT_IMPL=bf16x3 | f32: six-pass split-bf16 /
                            plain fp32-MFMA Linears, kept as cross-checks; =f16x2: the split-fp16 implementation,
                            opt-in at channels 192 / 320 / 384 / 448, see d3dp_create)                            */
  D3DP_MODE_FAST = 1,    /* bf16 activations/weights into v_mfma_f32_16x16x32_bf16, fp32 accumulate/LN/softmax */
  D3DP_MODE_TRAIN = 2,   /* fp32 weights and activations; Linears (forward, dgrad, wgrad) on split-fp16 operands whose scales are
                            found on the device: required by d3dp_train_*; inference also works (fp32-MFMA Linears)          */
  D3DP_MODE_FAST16 = 3,  /* D3DP_MODE_FAST's dataflow, buffers, workspace and launches on IEEE fp16 operands (v_mfma_f32_16x16x32_f16:
                            11 significand bits instead of 8 at the same rate), fp32 accumulate/LN/softmax/residual stream --
                            when d3dp_set_weights can PROVE from the weights that no value stored in 2 bytes reaches fp16's
                            65504 (d3dp_fast_operands); otherwise the context runs FAST's bf16 kernels, bit for bit (ABI v5) */
};

/* MixSTE2 hyper-parameters -- reference common/diffusionpose.py:123-124, common/mixste.py:142-163 */
typedef struct d3dp_cfg {
  int32_t frames;        /* F: args.number_of_frames                 */
  int32_t joints;        /* J: 17                                    */
  int32_t channels;      /* C: args.cs (embed_dim_ratio)             */
  int32_t depth;         /* args.dep: number of (spatial, temporal) block pairs */
  int32_t heads;         /* 8                                        */
  int32_t hidden;        /* mlp hidden = 2*C (mlp_ratio 2.)          */
  float eps_block;       /* 1e-6: LayerNorm eps of blocks and Spatial/Temporal_norm (mixste.py:163) */
  float eps_head;        /* 1e-5: nn.LayerNorm default in head (mixste.py:208)                     */
  int32_t mode;          /* D3DP_MODE_*                              */
  int32_t chunk_seqs;    /* most (clip,hypothesis) sequences per internal pass; 0 = library default (31 EXACT, 15 FAST).  EXACT
                          * mode sizes its passes (<= this) so that the persistent Linear kernels' last tile rounds are full
                          * (ctx.h plan()); results do not depend on the split, bit for bit.
                          * EXACT mode addresses a pass's Linear outputs with 32-bit byte offsets: chunk_seqs * F * J * 3 *
                          * channels * 4 must stay below 2^32 (169 sequences at F=243, J=17, C=512), else d3dp_denoise fails. */
} d3dp_cfg;

/* One transformer Block's parameters, fp32, reference state_dict names in comments (mixste.py:96-101) */
typedef struct d3dp_block_weights {
  const float* norm1_w; const float* norm1_b;     /* norm1.weight/bias   (C)      */
  const float* qkv_w;   const float* qkv_b;       /* attn.qkv.weight (3C,C)/bias  */
  const float* proj_w;  const float* proj_b;      /* attn.proj.weight (C,C)/bias  */
  const float* norm2_w; const float* norm2_b;     /* norm2.weight/bias            */
  const float* fc1_w;   const float* fc1_b;       /* mlp.fc1.weight (2C,C)/bias   */
  const float* fc2_w;   const float* fc2_b;       /* mlp.fc2.weight (C,2C)/bias   */
} d3dp_block_weights;

/* All MixSTE2 parameters (device fp32, caller-owned; the library keeps its own packed copies). */
typedef struct d3dp_weights {
  const float* spatial_pos;       /* Spatial_pos_embed (1,J,C)                 mixste.py:169 */
  const float* temporal_pos;      /* Temporal_pos_embed (1,F,C)                mixste.py:172 */
  const float* embed_w;           /* Spatial_patch_to_embedding.weight (C,5)   mixste.py:166 */
  const float* embed_b;
  const float* time_freq;         /* (C/2) fp32: exp(arange(C/2) * -ln(1e4)/(C/2-1)), mixste.py:135-136 (host-computed) */
  const float* time1_w;           /* time_mlp.1.weight (2C,C)                  mixste.py:181 */
  const float* time1_b;
  const float* time3_w;           /* time_mlp.3.weight (C,2C)                  mixste.py:183 */
  const float* time3_b;
  const float* spatial_norm_w;    /* Spatial_norm (shared by all depths)       mixste.py:203 */
  const float* spatial_norm_b;
  const float* temporal_norm_w;   /* Temporal_norm                             mixste.py:204 */
  const float* temporal_norm_b;
  const float* head_norm_w;       /* head.0 (LayerNorm)                        mixste.py:208 */
  const float* head_norm_b;
  const float* head_w;            /* head.1.weight (3,C)                       mixste.py:209 */
  const float* head_b;
  const d3dp_block_weights* ste;  /* host array [depth]: STEblocks.i           mixste.py:190 */
  const d3dp_block_weights* tte;  /* host array [depth]: TTEblocks.i           mixste.py:197 */
} d3dp_weights;

typedef struct d3dp_ctx d3dp_ctx;

D3DP_API int d3dp_abi_version(void);
D3DP_API const char* d3dp_last_error(void);

/* Lifetime.  Replaces: MixSTE2.__init__ (mixste.py:142-210) + .cuda() (main.py:243).
 * Shapes (D3DP_ENOTSUP outside them, with the reason in d3dp_last_error):
 *   1 <= frames <= 1024   up to 256 frames the MFMA attention kernels hold a whole sequence; longer clips (`-f 351`,
 *                         common/arguments.py:58) take chunked-key forms of the same kernels in every mode (FAST, FAST16:
 *                         keys through LDS in chunks of 128, probabilities rounded to 2 bytes as below 256 frames, at
 *                         head dims 64, 32 and 16; head dim 8 stays on the row kernel, fp32 arithmetic on the 2-byte
 *                         rows, on both axes and at every clip length);
 *   1 <= joints <= 256    MixSTE2's num_joints (mixste.py:141; D3DP builds 17): above 32 the spatial axis runs on the
 *                         whole-sequence attention kernels of the temporal axis, in every mode;
 *                         (D3DP_LONG_ATTN=rows in the environment of d3dp_create: the row kernel instead, for more than
 *                         256 frames in EXACT, FAST and FAST16 contexts, for more than 32 joints in FAST / FAST16 ones,
 *                         and for every attention of an EXACT, FAST or FAST16 context at head dim 32 or 16 -- the cross-check)
 *   channels in {64, 128, 256, 512} with head dim in {8, 16, 32, 64} and hidden % 64 == 0: every mode, on the matrix-core
 *                         kernels (split-fp16 / bf16 operands) -- `-cs 512`, the width of every published checkpoint
 *                         (README.md:33-39), and its smaller powers of two;
 *   any other width the reference's 8 heads divide (common/arguments.py:49, mixste.py:46-62) with channels <= 1024,
 *                         head dim % 4 == 0 and <= 128, hidden % 4 == 0: D3DP_MODE_EXACT on the fp32 implementation
 *                         (fp32-MFMA Linears, fp32 row attention, run-time-width row kernels; d3dp_exact_scales reports
 *                         implementation 2): the same 1e-3 mm tolerance at roughly a fifth of the throughput; and
 *                         D3DP_MODE_TRAIN on the fp32 path of the training step, with the token limits listed under "What a
 *                         D3DP_MODE_TRAIN context takes" below.  FAST and FAST16 contexts exist for the instantiated widths and,
 *                         opt-in, for the four widths of the line after next.
 *   channels in {192, 320, 384, 448} with head dim % 8 == 0 and <= 64 and hidden % 64 == 0, D3DP_MODE_EXACT, with
 *                         D3DP_EXACT_IMPL=f16x2 in the environment of d3dp_create (OPT-IN: without the switch such a context
 *                         launches the fp32 implementation above, bit for bit as before): the split-fp16 implementation of the
 *                         instantiated widths (d3dp_exact_scales reports implementation 0).  The head dim is padded to 32 / 64
 *                         inside the packed weights -- zero rows of the qkv matrix and bias, zero columns of proj -- so the
 *                         matrix-core attention kernels run at head dim 32 / 64 with the true head dim in the softmax
 *                         exponent; the LayerNorms run run-time-width row kernels that write split-fp16 rows.  Where the
 *                         weights' proven range would move an instantiated width to bf16x3 (a LayerNorm output bound beyond
 *                         the split range, non-finite weights) this context moves to the fp32 implementation.  At an
 *                         instantiated width the value names the default.  With any other width, or a TRAIN / FAST / FAST16
 *                         context of a non-instantiated width, or together with D3DP_LONG_ATTN=rows at these widths, the
 *                         switch cannot be honoured: D3DP_ENOTSUP, decided before the device is looked for.
 *   channels in {192, 320, 384, 448} with head dim in {24, 32, 40, 48, 56, 64} and hidden == 2 x channels (what MixSTE2 builds), D3DP_MODE_FAST
 *                         or D3DP_MODE_FAST16, with D3DP_FAST_IMPL=mfma in the environment of d3dp_create (OPT-IN: without the
 *                         switch such a context is refused as before, with the same message): the mode's dataflow as at the
 *                         instantiated widths -- 2-byte weights and activations (bf16, or fp16 behind FAST16's range proof, which
 *                         runs on the caller's unpadded weights), fp32 residual stream, LayerNorm and softmax in fp32, both
 *                         attentions and all four Linears on the matrix cores.  The head dim is padded to 32 / 64 inside the
 *                         packed 2-byte weights as above, the attention kernels take the true head dim in the exponent, the
 *                         row kernels are run-time-width forms with 2-byte rows.  (Head dims 24 / 40 / 48 / 56 -- 8 heads -- are
 *                         padded; 32 and 64 need no padding and run the attention kernels of the instantiated widths; 8 and 16
 *                         -- 12, 24, ... heads -- have no kernel behind this route and are refused.)  FAST16's fallback there is the same route on
 *                         bf16, bit for bit a FAST context.  Frames <= 1024 and joints <= 256 as everywhere.  At an instantiated
 *                         width the value names the default.  Any other value of the variable in a FAST / FAST16 context, any
 *                         other width, head dim or hidden, or D3DP_LONG_ATTN=rows beside it at these widths (the row kernel would take the
 *                         padded head dim for its exponent): D3DP_ENOTSUP, decided before the device is looked for.  EXACT and
 *                         TRAIN contexts do not read the variable.
 *   channels in {64, 128, 256, 512} with head dim in {16, 32, 64} and hidden in {64, 128, 256, 512, 1024}, D3DP_MODE_FAST16, with
 *                         D3DP_FAST16_RANGE=scale in the environment of d3dp_create (OPT-IN: without the switch such a context is
 *                         the FAST16 context of the instantiated widths above, bit for bit as before): where the weights prove a
 *                         bound of 65504 or more for a block's q / k / v, proj output, MLP hidden or fc2 output, that block stores
 *                         that class of fp16 tensors at a power of two 2^-s, s <= 8, of its value instead of moving the whole
 *                         context to bf16 (d3dp_fast_operands below).  Same workspace, same arena, same launches per call; a
 *                         context whose weights need no scale launches exactly the kernels it launches without the switch.
 *                         Any other value of the variable in a FAST16 context, head dim 8 (`-cs 64` with 8 heads), any other
 *                         hidden, D3DP_LONG_ATTN=rows beside it (the row attention kernel has no scaled form) or
 *                         D3DP_FAST_IMPL=mfma beside it at channels 192 / 320 / 384 / 448 (nor have the padded-head kernels):
 *                         D3DP_ENOTSUP naming the switch, decided before the device is looked for.  FAST, EXACT and TRAIN contexts
 *                         do not read the variable.
 * What a D3DP_MODE_TRAIN context takes, by the attention its training step runs:
 *   channels in {128, 256, 512} with head dim in {16, 32, 64} (`-cs 128 / 256 / 512` with 8 heads): Linears on split-fp16 operands and
 *                         the attention of both axes on the split-fp16 matrix-core kernels (train_attn.hip), which pass keys /
 *                         queries through LDS in chunks: every frames <= 1024 and joints <= 256 above;
 *   head dim 8 (`-cs 64`): split-fp16 Linears, fp32 attention (VALU / row kernels), whose backward holds a whole sequence in LDS:
 *                         d3dp_create accepts the context, d3dp_train_forward answers D3DP_ENOTSUP beyond 256 frames (unless
 *                         D3DP_TRAIN_LONG_ATTN=chunked, below);
 *   the cross-check switches at the widths above (D3DP_TRAIN_IMPL=f32, D3DP_TRAIN_ATTN=f32|x2t in the environment of d3dp_create)
 *                         select that fp32 attention too, with the same limit of 256 frames (and the same exception);
 *   any other width (see above: channels <= 1024, head dim % 4 == 0 and <= 128, hidden % 4 == 0): the fp32 path of the training step
 *                         (what D3DP_TRAIN_IMPL=f32 selects for the instantiated widths: fp32-MFMA Linears, run-time-width row
 *                         kernels, VALU attention backward with a run-time head dim).  There d3dp_create itself refuses
 *                         max(frames, joints) > 256 tokens, and > 153 tokens at head dims above 64 (two whole-sequence images
 *                         of the capacity head dim + the statistics in 160 KiB of LDS) -- unless D3DP_TRAIN_LONG_ATTN=chunked;
 *   channels in {192, 320, 384, 448} with head dim % 8 == 0 and <= 64 and hidden % 64 == 0, with D3DP_TRAIN_IMPL=f16x2 in the
 *                         environment of d3dp_create (OPT-IN: without the switch such a context is the line above, bit for bit
 *                         as before): the split-fp16 training step of the instantiated widths -- every Linear (forward, dgrad,
 *                         wgrad) on split-fp16 operands, the run-time-width row kernels leaving the operand absmax, and at head
 *                         dims 24 / 40 / 48 / 56 (8 heads) the attention of both axes on the split-fp16 kernels with the head
 *                         padded to 32 / 64 inside their LDS images (no weight, gradient or workspace region is padded;
 *                         d3dp_train_workspace_bytes is unchanged): every frames <= 1024 and joints <= 256.  Head dims 64, 32
 *                         and 16 there (3, 6, 12 heads at 192, ...) run the unpadded kernels; head dim 8 and
 *                         D3DP_TRAIN_ATTN=f32|x2t beside the switch keep split Linears around the fp32 attention, as `-cs 64`
 *                         does, and d3dp_train_forward answers D3DP_ENOTSUP beyond 256 frames.  At an instantiated width the
 *                         value names the default.  A TRAIN context of any other width cannot honour it: D3DP_ENOTSUP, decided
 *                         before the device is looked for.  Contexts of the other modes do not read D3DP_TRAIN_IMPL, and
 *                         D3DP_EXACT_IMPL=f16x2 keeps refusing a TRAIN context at these widths: a process that keeps a train
 *                         and an eval context sets each switch around the creation of its own context.
 *   D3DP_TRAIN_PASSES=1 in the environment of d3dp_create (OPT-IN; read for D3DP_MODE_TRAIN contexts alone; unset or =3: the step
 *                         above, bit for bit): a TRAIN context whose step runs the split-fp16 Linears -- the instantiated widths, and
 *                         channels in {192, 320, 384, 448} under D3DP_TRAIN_IMPL=f16x2 -- runs every product of those Linears
 *                         (forward, dgrad, both weight-gradient forms) as ONE fp16-MFMA pass hi(A) x hi(W): each operand rounded
 *                         to IEEE fp16 at the power of two its own absmax asks for (so neither a range proof nor loss scaling is
 *                         needed), fp32 accumulation, the same device-side scales, k order, partial sums, launches, streams and
 *                         workspace.  Attention, LayerNorm, GELU, the residual stream, the embedding, time-MLP and head Linears
 *                         and AdamW are untouched.  It is a mixed-precision route: gradients lie about 2^-11 from fp32's, not
 *                         2^-21.  D3DP_ENOTSUP, decided before the device is looked for and naming the switch: any other value;
 *                         =1 for a context on the fp32 path (D3DP_TRAIN_IMPL=f32, a width outside the sets above); =1 beside
 *                         D3DP_TRAIN_WGRAD=each, D3DP_TRAIN_TAIL=split, D3DP_TRAIN_GELU=pass or D3DP_TRAIN_LN_OPERAND=pass (launch
 *                         forms of the variants build, which have no one-pass form).  D3DP_TRAIN_ATTN, D3DP_TRAIN_ATTN_BWD and
 *                         D3DP_TRAIN_OVERLAP compose with it.  Contexts of the other modes do not read it.
 *   D3DP_TRAIN_ATTN_PASSES=1 in the environment of d3dp_create (OPT-IN; read for D3DP_MODE_TRAIN contexts alone; unset or =3: every
 *                         context plans, refuses and launches as in the lines above, bit for bit): every attention of the step
 *                         that runs on the split-fp16 kernels at head dim 64, 32 or 16 -- both axes, or the temporal axis alone
 *                         under D3DP_TRAIN_ATTN=x2t -- runs each of its products (S = Q K^T and O = P V forward; S, dP = dO V^T,
 *                         dQ = dS K, dK = dS^T Q, dV = P^T dO backward) as ONE fp16-MFMA pass: q, k, v rounded to IEEE fp16 at the
 *                         power of two of the qkv absmax, dO at that of its own, P x 2^10 and dS at its running power of two per
 *                         query / per key; fp32 accumulation, the softmax denominator, the log-sum-exp and dO . O in fp32.  Every
 *                         scale is a device value: neither a range proof nor loss scaling is needed.  Same launches, streams and
 *                         workspace; the LDS images halve.  A mixed-precision route -- gradients about 2^-13 from fp32's in the norm
 *                         -- that costs nothing measurable beside D3DP_TRAIN_PASSES=1, whose Linears are ten times farther.
 *                         D3DP_ENOTSUP, decided before the device is looked for and naming the switch: any other value; =1 for a
 *                         context on the fp32 path (D3DP_TRAIN_IMPL=f32, a width outside the instantiated set), at head dim 8,
 *                         beside D3DP_TRAIN_ATTN=f32, and at head dims 24 / 40 / 48 / 56 under D3DP_TRAIN_IMPL=f16x2 (the padded
 *                         kernels have no one-pass form).  D3DP_TRAIN_PASSES, D3DP_TRAIN_OVERLAP, D3DP_TRAIN_LONG_ATTN and
 *                         D3DP_TRAIN_ATTN_BWD compose with it.  Contexts of the other modes do not read it.
 *   D3DP_TRAIN_ROWS=hi in the environment of d3dp_create (OPT-IN; read for D3DP_MODE_TRAIN contexts alone; unset or =split: every
 *                         context plans, refuses and launches as in the lines above, bit for bit): beside D3DP_TRAIN_PASSES=1 every
 *                         operand of the training Linears -- activations, both forms of the weights, every dY -- is stored as plain
 *                         fp16 rows (the hi value alone: column c at offset c, half the row stride, the workspace regions unchanged
 *                         and half used) and the one-pass products read whole 128-byte lines of 64 columns.  The same values reach
 *                         the same MFMAs in the same order and the partial sums group the same k-steps: predictions and gradients
 *                         are BIT-EQUAL to D3DP_TRAIN_PASSES=1 alone; launches, streams, slots and the workspace size are unchanged.
 *                         The route exists where no operand of the step is transposed and every producer writes rows itself:
 *                         channels 256 or 512, hidden a multiple of 256, depth <= 8.  D3DP_ENOTSUP, decided before the device is
 *                         looked for and naming the switch: any other value; =hi without D3DP_TRAIN_PASSES=1, on the fp32 path, at
 *                         channels 64 / 128, at the padded widths of D3DP_TRAIN_IMPL=f16x2, at depth > 8, at head dim 16 unless
 *                         D3DP_TRAIN_ATTN=f32, and beside the variants-only launch forms.  D3DP_TRAIN_ATTN_PASSES, D3DP_TRAIN_ATTN,
 *                         D3DP_TRAIN_ATTN_BWD, D3DP_TRAIN_OVERLAP and D3DP_TRAIN_LONG_ATTN compose with it.  Contexts of the other
 *                         modes do not read it.
 *   D3DP_TRAIN_LONG_ATTN=chunked in the environment of d3dp_create (OPT-IN; read for D3DP_MODE_TRAIN contexts alone; unset: every
 *                         context plans, refuses and launches as in the lines above, bit for bit): every fp32 attention backward
 *                         of the step that runs on the VALU kernels -- head dim 8, a width on the fp32 path, the cross-check
 *                         switches beyond 256 tokens or under D3DP_TRAIN_ATTN_BWD=valu -- takes their chunked forms: a workgroup
 *                         per 256 rows of a (sequence, head), K / V and then Q / dO / the statistics passing through LDS in chunks
 *                         of 256 rows (128 at head dims above 64).  Such a context trains at every frames <= 1024 and joints <=
 *                         256 at every width the fp32 implementation takes (`-cs 1024 -f 243`, `-cs 96 -f 351`, `-cs 64 -f 351`):
 *                         neither d3dp_create's token limit nor d3dp_train_forward's 256 frames applies.  Same arithmetic in the
 *                         same order as the whole-sequence kernels: where both run the gradients are the same bits.  Same
 *                         workspace, same launches per step, no atomics.  The fp32-MFMA backward (head dim 64, <= 256 tokens)
 *                         stays.  Any other value in a TRAIN context: D3DP_ENOTSUP naming the switch, decided before the device
 *                         is looked for.  D3DP_TRAIN_IMPL, D3DP_TRAIN_ATTN, D3DP_TRAIN_ATTN_BWD, D3DP_TRAIN_PASSES and
 *                         D3DP_TRAIN_OVERLAP compose with it.  Contexts of the other modes do not read it.
 * A D3DP_MODE_TRAIN context whose backward pass overlaps (split-fp16 Linears, D3DP_TRAIN_OVERLAP not 0) gets its second stream
 * and three events here, so that d3dp_train_backward never creates anything. */
D3DP_API int d3dp_create(const d3dp_cfg* cfg, d3dp_ctx** out);
D3DP_API int d3dp_destroy(d3dp_ctx* ctx);
/* Replaces: load_state_dict (main.py:257).  Converts/packs weights for cfg.mode (synchronises `stream`).
 * Non-finite weights (a diverged checkpoint) are not an error: like the reference, the library loads them and the outputs
 * are non-finite where the reference's are (d3dp_status reports it); an EXACT context then runs its split-bf16
 * implementation (d3dp_exact_scales: implementation 1), which has fp32's exponent range. */
D3DP_API int d3dp_set_weights(d3dp_ctx* ctx, const d3dp_weights* w, void* stream);
/* D3DP_MODE_TRAIN only: use the caller's fp32 device buffers in place (no packed copy, no launch, no synchronisation), so
 * an optimizer step needs no re-push.  The buffers must stay allocated while the context uses them. */
D3DP_API int d3dp_set_weights_borrowed(d3dp_ctx* ctx, const d3dp_weights* w);

/* EXACT mode's split-fp16 operands (x 2^s = hi + lo, two fp16) hold |x| 2^s < 65504: with the default s = 4 that is
 * |x| < D3DP_SPLIT_RANGE, beyond which hi would be inf and the Linear NaN where the fp32 reference stays finite.  The
 * library therefore PROVES the range of every data-dependent operand from the weights and scales accordingly:
 *  - d3dp_set_weights computes (on the device) an upper bound of the magnitude each split operand can take for ANY
 *    input -- a LayerNorm output is at most sqrt(C-1) |gamma_k| + |beta_k| per channel; a Linear row over it at most
 *    sum_k |w_k| (sqrt(C-1) |gamma_k| + |beta_k|) + |b| (q, k, v and the fc1 pre-activation; |GELU(x)| <= |x|); an attention
 *    output is a convex combination of v -- and gives every block two operand scales: s_kv for q / k / v / the attention
 *    output, s_hidden for the MLP hidden.  Bound below D3DP_SPLIT_RANGE: 2^4.  Above: the largest power of two with
 *    bound x scale < 65504, so no operand can overflow, at an absolute representation error of at most
 *    max(2^-22 |x|, 2^-25 / scale) -- below 2^-40 of the bound, far under the fp32 rounding of the sums it enters.
 *    LayerNorm outputs always use 2^4; if a LayerNorm's own bound reaches the range (|gamma| ~ 180) the context moves to the
 *    six-pass split-bf16 implementation (fp32's exponent range, twice the MFMA work).  No environment variable is involved.
 *  - d3dp_exact_range_bound: the largest of those bounds (0 in the other modes, which have no such limit);
 *  - d3dp_exact_scales: the chosen scales, s_kv[2 depth] and s_hidden[2 depth] (STE blocks 0..depth-1, then TTE; either
 *    pointer may be null), and the implementation in use (0 split-fp16, 1 split-bf16, 2 fp32 MFMA, -1 not an EXACT context);
 *  - d3dp_status: *nonfinite = 1 if, since the last d3dp_status, a d3dp_denoise output held inf / nan (every call ends with a
 *    scan of its output) -- i.e. the INPUT held inf / nan or the fp32 arithmetic itself overflowed.  Synchronises the
 *    device (do not call it during stream capture); resets the flag.
 * (In a variants build -- see d3dp_op_linear_x2 -- ONE operand is outside the proof: with norm2 folded into fc1, D3DP_FOLD_LN=1,
 * the proj Linear hands fc1 the un-normalised residual stream; that epilogue checks every value it splits, exactly, at run
 * time, and reports through d3dp_status.) */
#define D3DP_SPLIT_RANGE 4094.0f
D3DP_API int d3dp_exact_range_bound(const d3dp_ctx* ctx, float* bound);
D3DP_API int d3dp_exact_scales(const d3dp_ctx* ctx, float* s_kv, float* s_hidden, int32_t* implementation);
D3DP_API int d3dp_status(d3dp_ctx* ctx, int32_t* nonfinite);

/* D3DP_MODE_FAST16 stores in IEEE fp16 what D3DP_MODE_FAST stores in bf16: the weight matrices, the LayerNorm outputs, q / k / v,
 * the attention output, the MLP hidden and the two branch outputs (proj, fc2) that the row kernels add to the fp32 residual
 * stream.  fp16 overflows at 65504 where bf16 has fp32's exponent range, so d3dp_set_weights PROVES the range first, on the
 * device, per block, for ANY input (C = channels; sums in fp64, every result rounded up to fp32, so the bound never
 * under-states the formula):
 *     L1, L2   LayerNorm outputs   max_k sqrt(C-1) |gamma_k| + |beta_k|                                  (norm1, norm2)
 *     b_qkv    q, k, v             max_n sum_k |Wqkv[n,k]| (sqrt(C-1) |gamma1_k| + |beta1_k|) + |bqkv_n|;  b_v: the v rows n >= 2C
 *              attention output    <= b_v (a convex combination of v rows; probabilities <= 1)
 *     b_proj   proj output         max_n sum_k |Wproj[n,k]| b_v + |bproj_n|
 *     b_h      MLP hidden          max_n sum_k |Wfc1[n,k]| (sqrt(C-1) |gamma2_k| + |beta2_k|) + |bfc1_n|     (|GELU(x)| <= |x|)
 *     b_fc2    fc2 output          max_n sum_k |Wfc2[n,k]| b_h + |bfc2_n|
 *              weight matrices     max |w| of each of the four
 * The context's bound is the largest of these over all blocks.  Bound finite and < 65504: the context runs on fp16 operands,
 * unscaled.  Otherwise -- or with an inf / nan weight -- it runs the bf16 kernels: exactly what a D3DP_MODE_FAST context
 * launches on those weights, bit for bit (never an error, never an inf that FAST would not give); this mirrors EXACT's move to
 * split-bf16.  The decision is per context, not per tensor: a Linear's two operands share one type.
 * d3dp_fast_operands (after d3dp_set_weights): *type = 0 bf16, 1 fp16, -1 not a FAST / FAST16 context; *bound = the proven
 * maximum (inf for non-finite weights; 0 for a plain FAST context, which proves nothing).  The worst-case bound is loose by
 * construction: the seed-initialised 8-block model at C = 512 proves 4762 (13.8x below the limit); where trained checkpoints
 * sit against it has not been measured.
 * D3DP_FAST16_RANGE=scale (d3dp_create): the four bounds a weight edit can push out of range give each block four exponents --
 * s_qkv from b_qkv (q, k, v and the attention output, which is at most b_v 2^-s), s_proj from b_proj, s_h from b_h (the hidden
 * and the fp16 pre-activation parked in front of the GELU), s_fc2 from b_fc2 -- each the smallest s >= 0 with bound x 2^-s < 65504.
 * The Linear that produces a class multiplies its fp32 accumulator and bias by the power of two before the fp16 rounding, the
 * attention kernels take 2^(2 s_qkv) into the softmax exponent, proj and fc2 take their input's scale out as they apply their own,
 * and the row kernels multiply the branch outputs back as they add them to the fp32 residual stream: every multiplication is
 * exact, so the only change is where fp16's subnormal range begins.  LayerNorm outputs and the weight matrices are never scaled.
 * The context runs fp16 when every weight is finite, every L1, L2 and max |w| is below 65504 and every s is at most 8 (a CPU
 * emulation of all four classes at 2^-s in every block stays within 1.2x of the unscaled one's distance to the fp32 oracle up to
 * s = 12; profiles/fast16_scaled.md) -- otherwise the bf16 kernels, as without the switch.  *bound keeps its meaning, the proven
 * maximum of the VALUES: *type = 1 beside *bound >= 65504 means scaled. */
D3DP_API int d3dp_fast_operands(const d3dp_ctx* ctx, int32_t* type, float* bound);

/* Scratch needed by d3dp_denoise for a (B, H) call. */
D3DP_API int d3dp_workspace_bytes(const d3dp_ctx* ctx, int32_t B, int32_t H, size_t* bytes);

/* One denoiser evaluation.  Replaces: MixSTE2.forward(x_2d, x_3d, t), eval branch (mixste.py:278-298) and,
 * with H = 1, the train branch's forward (mixste.py:215-225). */
D3DP_API int d3dp_denoise(d3dp_ctx* ctx, const float* x2d, const float* x_t, const int64_t* t, float* out, int32_t B,
                 int32_t H, void* workspace, size_t workspace_bytes, void* stream);

/* Flip-TTA pre-step.  Replaces diffusionpose.py:148-153.
 *   xt2[0:B]  = clamp(img, +-1.1 scale) / scale
 *   xt2[B:2B] = x negated, joints permuted (perm[j] = source joint of joint j; device int32[J])
 * img (B,H,F,J,3) -> xt2 (2B,H,F,J,3). */
D3DP_API int d3dp_ddim_pre(const float* img, float* xt2, const int32_t* perm, float scale, int32_t B, int32_t H, int32_t F,
                  int32_t J, void* stream);

/* Flip-TTA post-step + DDIM update.  Replaces diffusionpose.py:158-169 and :244-254.
 *   pred    = (pred2[b] + unflip(pred2[B+b])) / 2
 *   x_start = clamp(pred * scale, +-1.1 scale)                    -> x_start (row b at x_start + b*xs_bstride)
 *   pn      = float((sqrt_recip * img - x_start) / sqrt_recipm1)  (fp64, predict_noise_from_start :129-133)
 *   img_next= x_start*c_xstart + c_noise*pn + sigma*noise         (fp32, unless `last`)
 * `noise` may be NULL only when `last` != 0.  img_next may alias img. */
D3DP_API int d3dp_ddim_post(const float* pred2, const float* img, const float* noise, const int32_t* perm, float scale,
                   double sqrt_recip, double sqrt_recipm1, float c_xstart, float c_noise, float sigma, int32_t last,
                   float* x_start, size_t xs_bstride, float* img_next, int32_t B, int32_t H, int32_t F, int32_t J,
                   void* stream);

/* Train-time forward diffusion.  Replaces prepare_diffusion_concat/q_sample (diffusionpose.py:260-267, 290-306):
 *   out[b] = float(clamp(a[b]*(x0[b]*scale) + s[b]*noise[b], +-1.1 scale) / scale); a, s are device fp64 (B). */
D3DP_API int d3dp_q_sample(const float* x0, const float* noise, const double* sqrt_ac, const double* sqrt_1mac, float scale,
                  float* out, int32_t B, int32_t per_b, void* stream);

/* ---- the whole sampler as one call (added to ABI v5) --------------------------------------------------------------------------
 * Replaces: D3DP.ddim_sample_flip (diffusionpose.py:214-256; `flip` != 0) and D3DP.ddim_sample (:171-212; `flip` = 0) -- the loop
 * over the K sampling steps around d3dp_ddim_pre / d3dp_denoise / d3dp_ddim_post, the per-step timestep tensor, the noise draws
 * and the schedule arithmetic -- for a host that has neither torch.randn nor that loop.
 *
 * d3dp_ddim_step: what one step needs from the schedule.  d3dp_ddim_steps fills a table of K of them from the caller's
 * alphas_cumprod (host fp64 [T]: one of the twelve buffers of every checkpoint; the cosine schedule is NOT re-derived) exactly as
 * the Python sampler does: the timesteps are torch.linspace(-1, T - 1, K + 1).int() reversed (float32, torch's two-sided formula:
 * start + step i below the middle, end - step (steps - 1 - i) from it on, then truncation), step k running at t = times[k];
 * sqrt_recip = sqrt(1 / ac[t]), sqrt_recipm1 = sqrt(1 / ac[t] - 1); with a = ac[t], a' = ac[t_next]:
 * sigma = eta sqrt((1 - a / a') (1 - a') / (1 - a)), c_noise = sqrt(1 - a' - sigma^2), c_xstart = sqrt(a'), computed in fp64 and
 * rounded to float where the field is one; `last` = 1 at the final step (t_next < 0: no update, the three coefficients are 0),
 * 0 elsewhere.  c_noise64 is c_noise before that rounding, with sigma^2 formed as the product sigma sigma (what torch's pow gives
 * fp64 tensors) where c_noise forms it with libm's pow (what Python's ** gives floats): the flip sampler passes the float, the
 * non-flip one multiplies an fp64 noise prediction with the double.  t, last and the coefficients equal the Python sampler's
 * values bit for bit.  sqrt_recip and sqrt_recipm1 are the correctly rounded values; the Python sampler reads them from the buffers
 * sqrt_recip_alphas_cumprod / sqrt_recipm1_alphas_cumprod, which torch's CPU sqrt made and every checkpoint carries, and that
 * sqrt is not correctly rounded (it differs in the last bit at 14 + 9 of the 1000 entries of the cosine schedule): a host that
 * wants the Python sampler's bits at those timesteps writes buffer[t] over the two fields, as d3dp_amd/model.py does.  The
 * table is the caller's: d3dp_sample takes whatever schedule it holds.  1 <= K <= T, else D3DP_EINVAL. */
typedef struct d3dp_ddim_step {
  int64_t t;                          /* timestep of the step: row value of the denoiser's `t`                      */
  double sqrt_recip, sqrt_recipm1;    /* predict_noise_from_start's coefficients at t (diffusionpose.py:129-133)    */
  float c_xstart, c_noise, sigma;     /* the DDIM update's (diffusionpose.py:244-254), as d3dp_ddim_post takes them */
  int32_t last;                       /* 1 at the final step and nowhere else                                        */
  double c_noise64;                   /* c_noise in fp64, for the non-flip update                                   */
} d3dp_ddim_step;
D3DP_API int d3dp_ddim_steps(const double* alphas_cumprod /*host[T]*/, int32_t T, int32_t K, double eta, d3dp_ddim_step* out /*host[K]*/);

/* The noise of d3dp_sample without injected noise: a counter-based generator, so that element e of draw d under `seed` is a pure
 * function of (seed, d, e) -- independent of B, H, the denoiser's passes, the launch grid and the flip flag.
 *   generator   Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), key = (seed low 32 bits, seed high 32 bits),
 *               counter = (e >> 2, draw, 0, 0); e = flat element index of the (B, H, F, J, 3) tensor; e >> 2 must fit 32 bits
 *               (D3DP_EINVAL beyond);
 *   draws       draw 0 = the initial img, draw k + 1 = the noise added after step k (the final step draws none);
 *   words       the four output words x0 .. x3 of one counter belong to elements 4 (e >> 2) .. 4 (e >> 2) + 3;
 *   uniforms    u_i = ((x_i >> 8) + 0.5f) * 2^-24, evaluated in fp32: at least 2^-25, so the logarithm below is finite (the fp32 sum
 *               ties to even above 2^23, so u_i = 1 for x_i >> 8 = 2^24 - 1: a radius of 0 or an angle of 2 pi);
 *   normals     (n0, n1) = sqrt(-2 ln u0) * (cos 2 pi u1, sin 2 pi u1), (n2, n3) likewise from (u2, u3), in fp32.
 * This is NOT torch.randn's stream: the same distribution, other bits.  d3dp_op_randn writes out[e] = n(seed, draw, e) for e < n
 * and, if `bits` is non-null, the word x behind each element (tests hold the integer stage to a Philox written in numpy, the
 * normal stage to fp64 Box-Muller on the same words). */
D3DP_API int d3dp_op_randn(uint64_t seed, uint32_t draw, float* out, uint32_t* bits /*or NULL*/, size_t n, void* hip_stream);

/* d3dp_sample: K steps of pre-step, denoiser, post-step in one call.
 *   x2d (B,F,J,2); x2d_flip (B,F,J,2) with flip != 0, NULL with flip = 0 (anything else: D3DP_EINVAL naming it); perm: device
 *   int32[J] as in d3dp_ddim_pre (read with flip only); steps: host [K], from d3dp_ddim_steps or the caller's own schedule, read
 *   before the call returns; noise: (K,B,H,F,J,3) = draws 0 .. K - 1 injected (the Python samplers' `noise` list, stacked), or
 *   NULL for the generator above under `seed`; preds (B,K,H,F,J,3): x_start of every step, the Python samplers' result.
 *   flip != 0: per step d3dp_ddim_pre, ONE d3dp_denoise over the 2B items (x2d | x2d_flip), d3dp_ddim_post -- with injected noise
 *   the bits of D3DP.ddim_sample_flip.  flip = 0: the non-flip forms at the rounding points of D3DP.ddim_sample (the update adds an
 *   fp32, an fp64 and an fp32 product in fp64; img is fp64 between the steps), one d3dp_denoise over B items.
 * The workspace (d3dp_sample_workspace_bytes; 256-byte aligned regions like d3dp_workspace_bytes), in this order: img (B,H,F,J,3;
 * fp32 with flip, fp64 without), xt2 and pred2 (nb,H,F,J,3) fp32 with nb = 2B with flip and B without, the timestep rows
 * [K][nb] int64, with flip the concatenated 2D input (2B,F,J,2), and the denoiser's own workspace (d3dp_workspace_bytes(nb, H)).
 * Stream contract as everywhere: everything is enqueued on `hip_stream`, nothing is allocated, created or synchronised; the call
 * is a single-stream chain (no fork) and may be captured after one eager call.  EXACT, FAST and FAST16 contexts; a TRAIN context:
 * D3DP_EINVAL naming the mode.  Refused before anything is launched, naming the argument: K < 1; `last` set anywhere but at the
 * final step, or unset there; x2d_flip inconsistent with flip; e >> 2 beyond 32 bits without injected noise (D3DP_EINVAL);
 * weights not set, workspace too small (D3DP_ESTATE).  While d3dp_profile_enable is on, the sampler's own kernels count in the
 * denoiser class "other". */
D3DP_API int d3dp_sample_workspace_bytes(const d3dp_ctx* ctx, int32_t B, int32_t H, int32_t K, int32_t flip, size_t* bytes);
D3DP_API int d3dp_sample(d3dp_ctx* ctx, const float* x2d, const float* x2d_flip /*NULL iff !flip*/, const int32_t* perm, float scale,
                const d3dp_ddim_step* steps /*host[K]*/, int32_t K, const float* noise /*(K,B,H,F,J,3) or NULL*/, uint64_t seed,
                float* preds /*(B,K,H,F,J,3)*/, int32_t B, int32_t H, int32_t flip, void* ws, size_t ws_bytes, void* hip_stream);

/* The non-flip pre- and post-step of d3dp_sample alone (unit parity tests against oracle/glue_check.py; the kernels d3dp_sample
 * launches with flip = 0).  img is FP64 here: D3DP.ddim_sample's update adds an fp32, an fp64 and an fp32 product in fp64.
 *   pre    xt = float(clamp(img, +-lim) / scale); first != 0: img holds fp32 values (the initial noise) and lim = fp32(1.1 scale),
 *          the bound of the reference's fp32 clamp; otherwise lim = 1.1 scale in fp64.  img (B,H,F,J,3) -> xt (B,H,F,J,3).
 *   post   x_start = clamp(pred * scale, +-fp32(1.1 scale))                      (fp32; row b at x_start + b*xs_bstride)
 *          pn       = (sqrt_recip * img - x_start) / sqrt_recipm1                (fp64, kept)
 *          img_next = (double(x_start*c_xstart) + c_noise64*pn) + double(sigma*noise)     (unless `last`; the outer products fp32)
 *          noise: (B,H,F,J,3), or NULL for the generator's (seed, draw); img_next may alias img. */
D3DP_API int d3dp_op_ddim_pre_noflip(const double* img, float* xt, float scale, int32_t first, int32_t B, int32_t H, int32_t F,
                            int32_t J, void* hip_stream);
D3DP_API int d3dp_op_ddim_post_noflip(const float* pred, const double* img, const float* noise, uint64_t seed, uint32_t draw,
                             float scale, double sqrt_recip, double sqrt_recipm1, float c_xstart, double c_noise64, float sigma,
                             int32_t last, float* x_start, size_t xs_bstride, double* img_next, int32_t B, int32_t H, int32_t F,
                             int32_t J, void* hip_stream);

/* JPMA: joint-wise reprojection-based multi-hypothesis aggregation (the consumer of the sampler / all-gather output).
 * Replaces main.py:700 (root zeroing, if zero_root), :706-712 (trajectory add + project_to_2d, camera.py:30-60) and
 * the per-joint argmin + gather of loss.py:54-76 / main_3dhp.py:797-835 in ONE pass, without (B,K,H,F,J,*) temporaries.
 *   pred (B,K,H,F,J,3), traj (B,F,1,3), cam (9) = f(2) c(2) k(3) p(2), gt2d (B,F,J,2), gt3d (B,F,J,3) or NULL
 *   agg (B,K,F,J,3)  <- the hypothesis whose reprojection is closest to gt2d (first minimum, like torch.min: a NaN error
 *                       counts as the smallest and the first one wins; hypothesis 0 where every error is +inf)
 *   sel (B,K,F,J) int32 or NULL; err_sel / err_min (B,K,F,J) or NULL: |selected - gt3d| and min_h |pred_h - gt3d|
 *   (their means over (B,F,J) are the reference's J_Agg and J_Best errors per step). */
D3DP_API int d3dp_jpma(const float* pred, const float* traj, const float* cam, const float* gt2d, const float* gt3d, float* agg,
              int32_t* sel, float* err_sel, float* err_min, int32_t B, int32_t K, int32_t H, int32_t F, int32_t J,
              int32_t zero_root, void* stream);
/* d3dp_jpma straight on an all-gather result: `gathered` = (R, B, K, H_local, F, J, 3), rank-major, exactly what
 * ncclAllGather leaves when every rank contributes its (B, K, H_local, F, J, 3) stack -- hypothesis h = r H_local + hl.
 * Same outputs and the same selection, bit for bit, as d3dp_jpma on the (B, K, R H_local, F, J, 3) tensor that a
 * permute + copy of `gathered` would produce (158.6 MB per rank and step at configs[3] that are never moved).
 * Replaces: main.py:700-718 after the hypothesis exchange of SURVEY.md 8 E1. */
D3DP_API int d3dp_jpma_gathered(const float* gathered, const float* traj, const float* cam, const float* gt2d, const float* gt3d,
                       float* agg, int32_t* sel, float* err_sel, float* err_min, int32_t R, int32_t B, int32_t K,
                       int32_t H_local, int32_t F, int32_t J, int32_t zero_root, void* stream);
/* d3dp_jpma with the 3DHP evaluation's options and pose outputs (main_3dhp.py:777-835): root_joint = index of the joint
 * written as 0 before use (0 for Human3.6M, 14 for 3DHP, -1 none); linear_projection = camera.py:62-83
 * project_to_2d_linear (f * clamp(X/Z) + c) instead of the distortion model; jbest (B,K,F,J,3) = per joint the
 * hypothesis closest to gt3d (J-Best pose), mean (B,K,F,J,3) = average over hypotheses (P-Agg pose).  Any output may be
 * NULL. */
D3DP_API int d3dp_jpma_ex(const float* pred, const float* traj, const float* cam, const float* gt2d, const float* gt3d, float* agg,
                 int32_t* sel, float* err_sel, float* err_min, float* jbest, float* mean, int32_t B, int32_t K, int32_t H,
                 int32_t F, int32_t J, int32_t root_joint, int32_t linear_projection, void* stream);

/* ---- training step (reference main.py:387-401 around diffusionpose.py:279-287 / mixste.py:215-225) ----------------
 * Context must be D3DP_MODE_TRAIN.  x3d (B,F,J,3) is the diffused pose from d3dp_q_sample, t (B) int64.
 * masks: NULL, or DropPath scales (timm semantics, values 0 or 1/keep) laid out [2*depth blocks (STE0,TTE0,STE1,..)]
 * [2 branches (attention, MLP)][B*max(F,J)] floats; entry s of a spatial block is sample b*F+f, of a temporal block b*J+n.
 * d3dp_train_forward keeps every activation the backward needs in `workspace`; d3dp_train_backward must follow with the
 * same inputs/masks/workspace.  grads: device fp32 buffers shaped like the weights (zeroed, then filled, here).
 * d3dp_train_backward launches a block's weight-gradient product on a second, library-owned stream (made by d3dp_create), forked
 * from and joined back to `stream` with events before it returns (the host is never synchronised; env D3DP_TRAIN_OVERLAP=0: one
 * stream) -- see Conventions: the caller orders against `stream` alone.
 * No gradient is accumulated with float atomics: the same inputs give the same bits.
 * Arithmetic of the Linears: three fp16-MFMA passes on split operands (fp32-class), or one pass on their hi planes under
 * D3DP_TRAIN_PASSES=1 (fp16 operands at their own scale, fp32 accumulation: d3dp_create) -- same launches, same workspace.
 * Arithmetic of the split-fp16 attention: three fp16-MFMA passes per product, or one under D3DP_TRAIN_ATTN_PASSES=1 (q, k, v, dO, P
 * and dS rounded once to fp16 at their device-side scales: d3dp_create) -- same launches, same workspace, same profile classes.
 * Clip length: any F <= 1024 like inference (reference common/arguments.py:58); beyond 256 frames the step needs its split-fp16
 * attention kernels (head dims 64, 32 and 16, and 24 / 40 / 48 / 56 under D3DP_TRAIN_IMPL=f16x2; keys / queries through LDS in
 * chunks) -- head dim 8, the fp32 path of the other widths and the fp32 cross-check implementations (D3DP_TRAIN_IMPL=f32,
 * D3DP_TRAIN_ATTN=f32|x2t) hold whole sequences and answer D3DP_ENOTSUP there (d3dp_create), unless the context was created under
 * D3DP_TRAIN_LONG_ATTN=chunked: their backward then passes its rows through LDS in chunks and takes every length too. */
D3DP_API int d3dp_train_workspace_bytes(const d3dp_ctx* ctx, int32_t B, size_t* bytes);
D3DP_API int d3dp_train_forward(d3dp_ctx* ctx, const float* x2d, const float* x3d, const int64_t* t, const float* masks, float* out,
                       int32_t B, void* workspace, size_t workspace_bytes, void* stream);
D3DP_API int d3dp_train_backward(d3dp_ctx* ctx, const float* x2d, const float* x3d, const int64_t* t, const float* masks,
                        const float* grad_out, const d3dp_weights* grads, int32_t B, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- caller-side rows of SURVEY.md section 8(f) (d3dp_amd/csrc/caller.hip) ------------------------------------------
 * N2 clip chunking: src (n,J,D) -> dst (n_clips,F,J,D), n_clips = d3dp_clip_count(n,F): consecutive clips, a trailing
 * partial clip = the LAST F frames, n < F replicate-padded on the right (reference main.py:267-299,
 * in_the_wild/utils.py:199-240).  dst_flip (optional): the flipped input main.py:646-648 builds (x negated, joints
 * permuted by perm[J], perm[j] = source joint). */
D3DP_API int d3dp_clip_count(int32_t n, int32_t F);
D3DP_API int d3dp_clip_gather(const float* src, float* dst, float* dst_flip, const int32_t* perm, int32_t n, int32_t F, int32_t J,
                     int32_t D, void* stream);
/* de-chunking: pred (n_clips,K,H,F,J,D) -> out (K,H,n,J,D)  (in_the_wild/videopose_diffusion.py:150-164, including
 * its n < F behaviour: the last n frames of the padded clip). */
D3DP_API int d3dp_clip_scatter(const float* pred, float* out, int32_t n, int32_t K, int32_t H, int32_t F, int32_t J, int32_t D,
                      int32_t last_wins, void* stream);   /* last_wins: main_3dhp.py:327-330 (final clip owns the last F frames) */
/* E1 reduced exchange: d3dp_jpma_winners writes this rank's per-joint winner win (B,K,F,J,5) =
 * (2D error, x, y, z, bits of int32 global hypothesis index h_offset + h); after an all-gather over R ranks
 * (rank-major) d3dp_jpma_combine picks the smallest 2D error per joint, lowest rank on ties (= lowest global h, the
 * element torch.min returns in loss.py:67).  n = B*K*F*J. */
D3DP_API int d3dp_jpma_winners(const float* pred, const float* traj, const float* cam, const float* gt2d, float* win,
                      int32_t h_offset, int32_t B, int32_t K, int32_t H, int32_t F, int32_t J, int32_t zero_root,
                      void* stream);
D3DP_API int d3dp_jpma_combine(const float* win, int32_t R, size_t n, float* agg, int32_t* sel, void* stream);
/* N3 training batch assembly from device-resident pools (common/generators.py:12-171 ChunkedGenerator_Seq):
 * pool2d (N,J,2), pool3d (N,J,3) or NULL; table (nb,4) int32 = (first pool frame of the sequence, sequence length,
 * chunk start frame (may be negative / run past the end: edge frames repeat), flip); perm2d/perm3d (J) = left/right
 * swap for flipped items (x negated); zero_root: joint 0 of out3d written as 0 (main.py:365). */
D3DP_API int d3dp_batch_gather(const float* pool2d, const float* pool3d, const int32_t* table, const int32_t* perm2d,
                      const int32_t* perm3d, float* out2d, float* out3d, int32_t nb, int32_t F, int32_t J,
                      int32_t zero_root, void* stream);
/* AdamW (main.py:311: torch.optim.AdamW(lr, weight_decay=0.1)) over all parameter tensors in one launch.
 * chunks: device array of d3dp_adam_chunk (one block each); step = 1-based step count of this update. */
typedef struct d3dp_adam_chunk { float* p; const float* g; float* m; float* v; int32_t n; int32_t pad; } d3dp_adam_chunk;
D3DP_API int d3dp_adamw_step(const void* chunks, int32_t n_chunks, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int64_t step, void* stream);
/* N4 Procrustes-aligned per-joint errors (common/loss.py:190-395 p_mpjpe*): pred (B,KH,F,J,3), target (B,F,J,3) ->
 * err (B,KH,F,J) and (optional) the aligned poses. */
D3DP_API int d3dp_procrustes(const float* pred, const float* target, float* err, float* aligned, int32_t B, int32_t KH, int32_t F,
                    int32_t J, void* stream);

/* ---- single operators (unit parity tests; same kernels the denoiser launches) ---------------------------- */
/* out[M,N] = epi(A[M,K] W[N,K]^T + bias).  epi & 3: 0 bias, 1 bias+GELU(erf), 2 out(fp32) += result.
 * mode EXACT: everything fp32 (fp32 MFMA; the EXACT denoiser itself runs d3dp_op_linear_x2 below).  mode FAST: A, W bf16 (uint16
 * storage), fp32 accumulate, epi 0 or 1 only, out bf16 unless (epi & 16) (fp32): the persistent streaming kernel the
 * denoiser uses.  mode 4: the same kernel on IEEE fp16 A, W and out (what a FAST16 context launches; NOT D3DP_MODE_FAST16's
 * number, which this entry point does not take: 2 and 3 are the split-operand selectors here).
 * mode 4 with epi = e | 32 | (r_in << 8) | (r_out << 12), e = 0 or 1, r_in and r_out in 0 .. 8: the SCALED form of that kernel, as a
 * FAST16 context under D3DP_FAST16_RANGE=scale launches it -- A holds 2^-r_in times its value, the fp16 rows leave at 2^-r_out:
 * out = fp16((acc 2^(r_in - r_out)) + bias 2^-r_out); e = 1 (r_in = 0 only): that value parked as fp16, then
 * fp16(gelu(. 2^r_out) 2^-r_out).  K / 64 in {1, 2, 4, 8, 16}.  In mode FAST, and in mode 4 without the 32, any bit of epi other than 0, 1 and 4 is
 * D3DP_EINVAL as before. */
D3DP_API int d3dp_op_linear(int32_t mode, int32_t epi, const void* A, const void* W, const float* bias, void* out, int32_t M,
                   int32_t N, int32_t K, void* stream);
/* Multi-head attention over qkv[T,3C] -> out[T,C]; axis 0 = spatial (sequences of J joints), 1 = temporal
 * (sequences of F frames); tokens ordered (seq_batch, f, n).  impl 0 = fp32-VALU row kernel (any activation type),
 * 1 = matrix-core kernel: bf16 / fp16 MFMA for 2-byte activations (head dim 64, 32 or 16 -- any other, 8 included, is
 * D3DP_ENOTSUP; both axes: F <= 1024 frames on the temporal axis, the chunked-key kernel beyond 256; J <= 256 joints on the
 * spatial axis), fp32 MFMA for fp32 activations (head dim 64, temporal axis, F <= 256), 2 = the EXACT-mode kernels:
 * split-fp16 operands on the fp16 matrix cores (both axes; head dim 64, 32 or 16 -- any other, 8 included, is D3DP_ENOTSUP
 * and nothing is launched).  Inside
 * the denoiser those read the packed rows of its qkv Linear (d3dp_op_linear_x2, epi 4); this entry point takes plain fp32
 * rows and repacks them into a stream-ordered temporary (hipMallocAsync) first.
 * impl = 1 | (d << 8) on 2-byte rows: the padded-head forms of the FAST / FAST16 kernels (D3DP_FAST_IMPL=mfma at d3dp_create) --
 * C = heads x hdp is the PADDED width, hdp = 32 with true head dim d = 24 or hdp = 64 with d in {40, 48, 56}; the columns d .. hdp - 1
 * of every head are zeros in qkv and come back as exact zeros in out; the softmax scale is d^-0.5.  Any other (hdp, d):
 * D3DP_ENOTSUP.  Plain impl 1 takes C / heads itself as the head dim, as before.
 * impl = 1 | (s << 16), s = 1 .. 8, on fp16 rows (act_bf16 4) of head dim 64, 32 or 16: the SCALED forms of the FAST16 kernels
 * (D3DP_FAST16_RANGE=scale at d3dp_create) -- q, k and v in qkv hold 2^-s times their value, the softmax exponent is scaled by
 * (C / heads)^-0.5 2^(2s), and out holds 2^-s times the attention output.  Bits 8 .. 15 must be 0 (no padded scaled form exists); s
 * outside 1 .. 8, or another activation type, is D3DP_ENOTSUP through the check of the padded forms, as before.
 * act_bf16: 0 fp32 rows, 1 bf16 rows, 4 IEEE fp16 rows (impl 0 and 1: the kernels of a FAST16 context).
 * d3dp_op_layernorm out_bf16: the activation code of the row kernels -- 0 fp32, 1 bf16, 2 three split-bf16 planes, 3 two
 * split-fp16 planes (h2i), 4 IEEE fp16.  Codes 1 and 4 take the instantiated widths and any C % 32 == 0, C <= 512 (the run-time-width
 * kernels of the FAST modes at channels 192 / 320 / 384 / 448).  d3dp_op_linear in FAST mode / mode 4 takes K / 64 in {1, 2, 4, 8, 16}
 * and, with a 2-byte out, {3, 5, 6, 7} (epi 0, 1) and {10, 12, 14} (epi 0): the k-depths of those widths. */
D3DP_API int d3dp_op_attention(int32_t act_bf16, int32_t impl, int32_t axis, const void* qkv, void* out, int32_t n_bh,
                      int32_t F, int32_t J, int32_t C, int32_t heads, void* stream);
D3DP_API int d3dp_op_layernorm(int32_t out_bf16, const float* x, const float* w, const float* b, float eps, void* out,
                      int32_t T, int32_t C, void* stream);
/* mode 2 of d3dp_op_linear: split-bf16.  A and W are three bf16 planes each (x = x0 + x1 + x2, made by
 * d3dp_op_split3: dst[0..n) | dst[n..2n) | dst[2n..3n)); epi 0 -> fp32 out, epi 1 -> GELU then three bf16 planes out. */
D3DP_API int d3dp_op_split3(const float* src, void* dst, size_t n, void* stream);
/* The EXACT-mode Linear on split-fp16 operands.  A2 [M][K] and W2 [N][K] hold TWO fp16 per element, y = src * scale =
 * hi + lo with hi = fp16(y), lo = fp16(y - hi), in the line-interleaved layout "h2i": a matrix row is K/32 blocks of 64 fp16
 * (128 bytes), block kb = [hi of columns 32 kb .. 32 kb + 31 | lo of the same 32 columns] -- one 32-deep k-step of one row,
 * both values of every element, is one 128-byte line.  d3dp_op_split2 writes that layout for a flat array of n = rows x K
 * elements: dst[64 b .. 64 b + 31] = hi, dst[64 b + 32 .. 64 b + 63] = lo of src[32 b .. 32 b + 31]; n (and hence every row
 * length) must be a multiple of 32 (D3DP_EINVAL otherwise: a partial block would write past 2 n).
 * A2 must be at scale 16 (the library's default activation scale); W2 at any power-of-two `w_scale` (the denoiser picks it
 * per matrix so that max |w| w_scale lies in [2^13, 2^14)).  epi 0 -> fp32 out [M][N]; epi 1 -> GELU, then the result as an
 * h2i matrix [M][N] at scale 16 (the fc2 operand; N % 32 == 0); epi 4 (N = 3 C, C % 64 == 0; the qkv Linear of the EXACT
 * denoiser) -> packed rows of 12 C bytes: q fp32 [C] | k hi [C] | k lo [C] | v hi [C] | v lo [C] (plain fp16 planes, scale
 * 16), the operand format of the split-fp16 attention kernels; epi 2 -> out[M,N] fp32 is read and written (out += A W^T + b:
 * the residual-adding form of proj and fc2).
 * Constraints (D3DP_EINVAL otherwise): K % 64 == 0 (the k-loop runs two 32-deep k-steps per iteration), N % 4 == 0
 * (N % 32 == 0 for epi 1: whole h2i blocks), N <= 2048, M * N * 4 < 2^32.  Every operand value must stay below 65504 / scale
 * in magnitude (at scale 16: |x| < 4094) -- inside d3dp_denoise the library proves and arranges that (d3dp_exact_scales);
 * a caller of this entry point owns it.
 * The product library holds ONE form of this kernel.  Three more forms (epi | (D << 8), D in {1, 2, 4}: the row-class skewed
 * schedule; epi | 2048: ping-pong wave teams; epi | 4096: 256 x 256 tiles) and the epilogues that fold norm2 into proj / fc1
 * were built, measured no faster and now exist only in a `make -C d3dp_amd/csrc variants` library
 * (lib/variants/libd3dp_variants.so; tests marked `variants`): here those flags, and the environment switches D3DP_X2_SKEW,
 * D3DP_X2_PP, D3DP_X2_WIDE, D3DP_SEQ_PAD, D3DP_FOLD_LN read by d3dp_create, fail with D3DP_ENOTSUP -- they are never ignored.
 * Cross-check switches the product library does honour (read in d3dp_create): D3DP_EXACT_IMPL=bf16x3|f32, D3DP_NO_FOLD=1
 * (other implementations of EXACT mode's Linears / residual adds, same tolerance; D3DP_EXACT_IMPL=bf16x3 exists for channels in
 * {64, 128, 256, 512}: at any other width D3DP_ENOTSUP, decided before the device is looked for; D3DP_EXACT_IMPL=f16x2 is the opt-in
 * route of channels 192 / 320 / 384 / 448 described at d3dp_create), D3DP_DEFER_NORM=0 (the shared norm of every
 * block boundary applied in place by the norm pair instead of inside the next proj Linear: bit-identical), D3DP_TRAIN_IMPL=f32. */
D3DP_API int d3dp_op_split2(const float* src, void* dst, size_t n, float scale, void* stream);
D3DP_API int d3dp_op_linear_x2(int32_t epi, const void* A2, const void* W2, const float* bias, float w_scale, void* out, int32_t M,
                      int32_t N, int32_t K, void* stream);
/* fp32 <-> bf16 conversion helper (round-to-nearest-even), n elements */
D3DP_API int d3dp_op_to_bf16(const float* src, void* dst, size_t n, void* stream);

/* ---- per-kernel timing (HIP events on the launch stream) -------------------------------------------------
 * While enabled, every kernel launched by d3dp_denoise, d3dp_sample, d3dp_train_forward and d3dp_train_backward is bracketed by
 * hipEventRecord on the caller's stream (while enabled the training step keeps its weight-gradient products on that stream too
 * instead of its second one: no class's time contains a wait for compute units another stream holds; same results bit for bit).
 * d3dp_profile_read synchronises the recorded events and returns, per kernel class, the launch count and the
 * summed duration in milliseconds.  Classes are listed by d3dp_profile_class_name: 0-11 the denoiser's (d3dp_denoise; the set-up,
 * pre- and post-step kernels of d3dp_sample count in class 11, "other"),
 * 12-23 the training step's (ABI v4): train_linear (forward and dgrad products), train_wgrad (a block's merged weight-gradient
 * product + the sum of its partial tiles), train_attn_{fwd,bwd_q,bwd_kv}_{spatial,temporal}, train_operand_pass (fp32 rows -> split
 * operands), train_ln_fwd, train_ln_bwd, train_other; 24 event_pair_overhead: event pairs with nothing between them, recorded at
 * the end of d3dp_train_backward -- the time a bracket adds to the launch it times. */
#define D3DP_PROFILE_CLASSES 25
D3DP_API int d3dp_profile_enable(d3dp_ctx* ctx, int32_t on);
D3DP_API int d3dp_profile_read(d3dp_ctx* ctx, int64_t* counts /*host[D3DP_PROFILE_CLASSES]*/,
                      double* total_ms /*host[D3DP_PROFILE_CLASSES]*/);
D3DP_API const char* d3dp_profile_class_name(int32_t cls);

/* ---- test hooks ------------------------------------------------------------------------------------------
 * Exported for tests/ only; no reference call site stands behind them and hosts must not bind them.
 * d3dp_debug_x2_variants: 1 if this library was built with the measured-negative experiment kernels of gemm_x2.hip
 *   (`make variants`: lib/variants/libd3dp_variants.so), 0 for the product library.
 * d3dp_debug_train_linear: the training step's split-fp16 Linear alone, out[M, N] = A[M, K] W[N, K]^T + bias on fp32 device
 *   operands -- absmax, operand split and gemm_f16x2_dyn_kernel exactly as d3dp_train_forward launches them.  tail: 0 = the rows
 *   behind the last whole 256-row tile as one more row of tiles, 1 = as 16 x 64 blocks inside the same launch; tail | 16: the one-pass instantiation
 *   of the kernel (what D3DP_TRAIN_PASSES=1 launches); tail | 16 | 32: that product on hi-only operand rows (what D3DP_TRAIN_ROWS=hi
 *   launches; K % 64 == 0, else D3DP_EINVAL naming K); 32 without 16 and any other bit: D3DP_EINVAL; amax_out:
 *   optional pre-zeroed device word receiving the output's absmax (amax_pos = 1: its largest positive value).  Allocates its
 *   operand buffers and synchronises `stream`. */
D3DP_API int d3dp_debug_x2_variants(void);
D3DP_API int d3dp_debug_train_linear(const float* A, const float* W, const float* bias, float* out, int32_t M, int32_t N,
                                     int32_t K, int32_t tail, unsigned* amax_out, int32_t amax_pos, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* D3DP_HIP_H */
