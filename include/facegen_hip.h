/* libfacegen_hip.so -- C ABI of the MI355X-native (gfx950) GAN training hot path of aleju/face-generator.
 *
 * This is the drop-in boundary: the reference has no native code of its own; its Lua
 * modules dispatch into Torch7's THNN/THCUNN/cuDNN through LuaJIT FFI (upstream convention:
 *   THNN_(SpatialConvolutionMM_updateOutput)(state, input, output, weight, bias, finput, ...)
 * called as input.THNN.X(input:cdata(), ...)).  The entry points below are what a LuaJIT `ffi.cdef` (or the
 * ctypes mirror in face_generator_amd/_lib.py) binds instead.  Plain C: opaque context, caller-owned device
 * buffers (raw pointers + explicit workspace), status-code returns, message via fg_last_error().
 * No C++ exceptions cross the ABI; nothing here names a torch type.
 *
 * Conventions
 *   - all tensors fp32; device activations are NHWC ("internal layout"); the reference's NCHW appears only at
 *     the boundary (fg_nchw_to_nhwc / fg_nhwc_to_nchw = the nn.Copy modules of nn_utils.lua:355-362).
 *   - parameter and gradient vectors are ONE flat fp32 vector per net in REFERENCE order and layout
 *     (module order, weight then bias; conv [O][I][kH][kW], linear [out][in]) == Module:getParameters()
 *     (train.lua:151-152).  Tile-packed / tap-folded weight copies are internal.
 *   - every entry is asynchronous on the context's stream; only fg_d2h / fg_stream_sync block.
 *   - a context is bound to one device and is not thread-safe.
 */
#ifndef FACEGEN_HIP_H
#define FACEGEN_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct fg_ctx fg_ctx;
typedef struct fg_net fg_net;
typedef struct fg_comm fg_comm;
typedef struct fg_gan fg_gan;
typedef struct fg_sampler fg_sampler;

enum {
    FG_OK = 0,
    FG_ERR_INVALID = -1,      /* bad argument / shape (the Lua shim turns this into error()) */
    FG_ERR_HIP = -2,          /* HIP runtime error, text in fg_last_error */
    FG_ERR_NOMEM = -3,
    FG_ERR_UNSUPPORTED = -4,  /* layer pattern or kernel variant not built */
    FG_ERR_WORKSPACE = -5     /* caller workspace too small */
};

/* Arithmetic of the large convolution contractions (forward / data-gradient of layers that fill the chip with 256x128
 * tiles).  mode 0 (default): native fp32 MFMA (v_mfma_f32_32x32x2_f32).  mode 6: fp32 emulated on the bf16 matrix pipe --
 * operands split exactly into three bf16 planes, six exact plane products accumulated in fp32 (dropped terms <= 2^-24
 * relative); measured more accurate than mode 0 against fp64 and ~1.7x faster.
 * Value domain (pinned by tests/test_gpu_value_domain.py, derived in tests/VALUE_DOMAIN.md):
 *   mode 0 (fp32 MFMA, thin and gemv kernels): all of fp32.  Subnormal operands and results are exact, nothing is flushed;
 *     infinities and NaNs propagate as IEEE 754 has it (0 * inf = NaN).
 *   mode 6: exact split for 2^-110 <= |x| <= 0x7f7f0000 (3.3895e38, the largest value whose high plane is finite).  Above
 *     that (from 0x7f7f8000 on, infinities included) the high plane rounds to the bf16 infinity and the operand splits into
 *     (inf, -inf, NaN): the result is NaN where mode 0 would give a finite value or inf.  A NaN operand stays a NaN in all three
 *     planes, whatever its payload.  Below 2^-110 the planes are bf16 subnormals, which the matrix pipe honours (measured on
 *     gfx950: no flush of operands or results); they resolve 2^-133, so such an operand enters rounded to the nearest
 *     multiple of 2^-133: absolute error at most 2^-134 (relative 2^-24 at 2^-110, 2^-8 at 2^-126), zero below 2^-134.
 *   Winograd kernels (fp32 pipe in either mode): all of fp32; a value below 2^-124 is divided by up to 4 in the transform
 *     domain and rounds to the fp32 subnormal grid there (absolute error at most 9 x 2^-150 per output); around a non-finite
 *     input the whole 2x2 tile is NaN.
 * Replaces nothing in the reference (its
 * cudnn backend picks algorithms internally, models.lua:1-2); exposed so parity can be run in both modes.
 * PRECEDENCE: the Winograd bits of fg_set_fusion win over this switch -- the forward / data gradient of every layer that
 * FG_FUSE_WINOGRAD / _UP / _5X5 cover (3x3, folded up-convolutions, 5x5: most of the FLOPs of both workloads) runs the fp32 Winograd
 * kernels in either mode, and those round ~1.7x worse than the direct fp32 contraction.  A true mode-6 run (the accuracy contract
 * above on every large contraction) needs fg_set_fusion(flags & ~(FG_FUSE_WINOGRAD | FG_FUSE_WINOGRAD_UP | FG_FUSE_WINOGRAD_5X5 |
 * FG_FUSE_WINOGRAD_WGRAD)) before the nets are created. */
int fg_set_math(fg_ctx* ctx, int mode);
int fg_get_math(fg_ctx* ctx);

/* Optional kernel fusions / variants (results equal to the un-fused path up to the summation order of a reduction; exposed so
 * the parity tests and the bench can run both ways).  Default: FG_FUSE_DEFAULT; FG_FUSE_PRELU=0 / FG_THIN_SLAB=0 / FG_DEFER_WFINISH=0 /
 * FG_THIN_BIAS=0 / FG_WINO=0 / FG_WINO_UP=0 / FG_WINO_5X5=0 / FG_WINO_WGRAD=0 in the environment clear a bit at fg_ctx_create, FG_ADAM_PACK=1 sets that one.  Replaces nothing in the reference. */
enum {
    FG_FUSE_PRELU = 1,      /* an nn.PReLU between two contraction layers (models_c2f.lua:118-130, 242-255) rides on their
                             * epilogues: forward copy behind the producing layer, backward (+ slope-gradient partials) in
                             * the kernel that produces its output gradient (data gradient / max-pool backward) */
    FG_FUSE_THIN_SLAB = 2,  /* 3x3 convolutions with <= 3 output channels (models.lua:73, 385 backward) on the matrix pipe
                             * in one pass instead of the sliding-window VALU kernel */
    FG_FUSE_WFINISH_BATCH = 4, /* the split-K / parity sums of ALL weight gradients of a backward pass in one launch at its end
                                * (the partials stay in the net's workspace until then) instead of one launch per layer; same
                                * order of additions, bit-identical gradients */
    FG_FUSE_ADAM_PACK = 8,  /* fg_step_D / fg_step_G / fg_gan_update with Adam: penalty + clamp + Adam + the re-pack of every
                             * layer's weights into the kernels' layouts in ONE launch (each pack job takes its weights from the
                             * update of that element) instead of two; bit-identical parameters.  OFF by default: the pack's
                             * patch-wise access pattern slows the seven streams of the update down by more than the saved
                             * pass over the weights (cfg2 4.31 vs 4.27 ms, c2f 38.8 vs 38.6 ms per step) */
    FG_FUSE_THIN_BIAS = 16, /* the bias gradient of a convolution with <= 4 input channels (models.lua:385; models_c2f.lua:123, 244)
                             * from the weight-gradient kernel itself: one idle column of its (tap, channel) axis multiplies the
                             * constant 1, so the pass that streams the output gradient anyway also leaves its per-channel sums;
                             * off: a separate column-sum pass re-reads the tensor (134 MB per layer at 64x64, B = 128).  Same
                             * fp64 final reduction; the fp32 partial sums are formed in a different order (FG_THIN_BIAS=0 clears it) */
    FG_FUSE_WINOGRAD = 32,  /* 3x3 / pad 1 / stride 1 convolutions with channel counts % 8 == 0 on even-sized maps (models.lua:390-400,
                             * models_c2f.lua:124, 247-254): forward and data gradient as Winograd F(2x2, 3x3) on the fp32 matrix pipe
                             * (16 multiplies per 2x2 outputs instead of 36; transforms in fp32, results equal to the direct
                             * convolution to a few fp32 roundings) instead of the 9-tap implicit GEMM.  Read when a net is created
                             * (fg_net_create: its packed weights hold the transformed taps) and per call by the module-level
                             * fg_conv2d_* entries; FG_WINO=0 clears it.  The weight gradient: FG_FUSE_WINOGRAD_WGRAD */
    FG_FUSE_WINOGRAD_UP = 64,   /* the same for nn.SpatialUpSamplingNearest(2) + 5x5 / pad 2 convolutions (models.lua:63-64, 68-69): after
                                 * the tap fold every output parity is a 3x3 / pad 1 convolution of the source image, so forward (four
                                 * parities sharing one input transform) and data gradient (four stride-2 input groups) are Winograd
                                 * contractions as well; FG_WINO_UP=0 clears it */
    FG_FUSE_WINOGRAD_5X5 = 128, /* 5x5 / pad 2 / stride 1 convolutions (models_c2f.lua:125-126) as four 3x3 sub-kernels at tap offsets
                                 * (0 | 3, 0 | 3) of the zero-extended 6x6 window: 64 instead of 100 multiplies per 2x2 outputs;
                                 * FG_WINO_5X5=0 clears it */
    FG_FUSE_WINOGRAD_WGRAD = 256, /* the WEIGHT gradient of the layers the three bits above select, in the Winograd domain as well
                                   * (dL/dU = sum over tiles of A dY A^T (.) B^T d B, 16 instead of 36 multiplies per tile and
                                   * channel pair; G^T . G and the tap scatter in the pass that sums the split partials), where the
                                   * tile grid is 2^a x 2^b and the layer has enough tiles to reduce over; else, and with the bit
                                   * cleared (FG_WINO_WGRAD=0), the tap-by-tap contraction.  Read per call */
    FG_FUSE_ALL = 511,
    FG_FUSE_DEFAULT = 503
};
int fg_set_fusion(fg_ctx* ctx, int flags);
int fg_get_fusion(fg_ctx* ctx);
/* Test hook (parity tests only; replaces nothing in the reference): the two planning thresholds that decide where the Winograd-domain
 * weight gradient is taken -- at least `min_chunks` eight-tile chunks per block and `min_blocks` blocks per launch (defaults 24, 192;
 * <= 0 restores a default).  Process-wide, and the only way to change them: no environment variable does.  Lets small shapes reach
 * the kernel's corners (one chunk, ragged last chunk, a single channel block). */
int fg_test_set_wino_wgrad_thresholds(fg_ctx* ctx, long long min_chunks, long long min_blocks);

/* ---- context / memory (replaces cutorch.setDevice / cutorch streams, train.lua:79-80) ----
 * fg_ctx_create(FG_DEVICE_NONE, ...) makes a PLANNING-ONLY context: the process needs no HIP device, no kernel is launched and no
 * HIP runtime call is made, while every host-side decision of the library -- plan building, stage walks, sync-BN pauses, gradient
 * buckets, and the order / size / stream of every collective a step issues (fg_comm_create_dry + fg_comm_schedule) -- runs
 * unchanged.  Device pointers are then opaque tokens (host allocations of the right size that nothing dereferences); fg_malloc
 * returns host memory, fg_h2d / fg_d2h / fg_d2d are plain copies.  A process holds either planning-only contexts or real ones. */
enum { FG_DEVICE_NONE = -1 };
int fg_ctx_create(int device, fg_ctx** out);
int fg_ctx_destroy(fg_ctx* ctx);
int fg_ctx_set_stream(fg_ctx* ctx, void* hip_stream); /* NULL = default stream */
const char* fg_last_error(const fg_ctx* ctx);
const char* fg_version(void);
int fg_stream_sync(fg_ctx* ctx);
/* per-launch HIP-event timing of the contraction kernels on the context's stream (measurement only).
 * fg_prof_report synchronises and writes "label calls total_ms algorithmic_flops executed_flops bytes" lines. */
int fg_prof_enable(fg_ctx* ctx, int on);
int fg_prof_report(fg_ctx* ctx, char* buf, size_t len, int reset);
/* the shader clock the chip grants WHILE other work runs (measurement only): fg_prof_clock_start puts a one-wave probe on a
 * stream of its own that sleeps for about `ms` milliseconds between two readings of the shader-cycle counter (s_memtime) and of
 * the constant 100 MHz counter (s_memrealtime); fg_prof_clock_read waits for it and returns cycles / time in GHz and the time
 * the probe covered.  gfx950 clocks to its power budget: a contraction loop is granted 1.9 - 2.2 GHz of the nominal 2.4. */
int fg_prof_clock_start(fg_ctx* ctx, double ms);
int fg_prof_clock_read(fg_ctx* ctx, double* ghz, double* covered_ms);
int fg_malloc(fg_ctx* ctx, size_t bytes, void** out);
int fg_free(fg_ctx* ctx, void* p);
int fg_h2d(fg_ctx* ctx, void* dst, const void* src, size_t bytes);
int fg_d2h(fg_ctx* ctx, void* dst, const void* src, size_t bytes); /* synchronises */
int fg_d2d(fg_ctx* ctx, void* dst, const void* src, size_t bytes);
int fg_fill(fg_ctx* ctx, float* p, float value, long long n);
int fg_axpby(fg_ctx* ctx, float a, const float* x, float b, float* y, long long n); /* y = a*x + b*y */

/* ---- layout boundary: nn.Copy Float<->device of NN_UTILS.activateCuda (nn_utils.lua:355-362) ---- */
int fg_nchw_to_nhwc(fg_ctx* ctx, const float* src, float* dst, int n, int c, int h, int w);
int fg_nhwc_to_nchw(fg_ctx* ctx, const float* src, float* dst, int n, int c, int h, int w);

/* ---- RNG: torch.Tensor:uniform / :bernoulli / randn (nn_utils.lua:9, 37; nn.Dropout) -- Philox4x32-10 ---- */
/* Values (tests/POINTWISE_DOMAIN.md): u = (word >> 8) * 2^-24 lies in [0, 1 - 2^-24].  fg_rng_uniform = lo + u * (hi - lo) in fp32: lo
 * occurs, and hi ITSELF occurs wherever lo + (1 - 2^-24) (hi - lo) rounds up to it -- (0.5, 1.5) yields 1.5; (0, 1) does not yield
 * 1, and (-1, 1), the noise range of nn_utils.lua:9, does not yield 1 (its largest value is 1 - 2^-23).  fg_rng_bernoulli = u <
 * keep_prob: keep 0 gives all 0, keep 1 all 1.  fg_rng_normal takes u1 = ((word >> 8) + 1) * 2^-24 in (0, 1]: always finite. */
int fg_rng_uniform(fg_ctx* ctx, uint64_t seed, uint64_t offset, float* out, long long n, float lo, float hi);
int fg_rng_bernoulli(fg_ctx* ctx, uint64_t seed, uint64_t offset, float* out, long long n, float keep_prob);
int fg_rng_normal(fg_ctx* ctx, uint64_t seed, uint64_t offset, float* out, long long n, float mean, float std);

/* ---- net-level: an nn.Sequential compiled to a device plan (models.lua:57-81, 382-416) ---- */
enum fg_layer_type {
    FG_LINEAR = 1,          /* nn.Linear(a=in, b=out) */
    FG_VIEW = 2,            /* nn.View(a=C, b=H, c=W)  or nn.View(a=features) with b=c=0 */
    FG_PRELU = 3,           /* nn.PReLU() -- one shared slope */
    FG_UPSAMPLE2X = 4,      /* nn.SpatialUpSamplingNearest(2) */
    FG_CONV = 5,            /* (cudnn|nn).SpatialConvolution(a=nIn, b=nOut, c=k, k, dW, dH, d=pad, pad); p = stride dW=dH (0/1: 1, 2: 2);
                             * stride 2: odd k <= 7, pad (k - 1) / 2, even H and W (else FG_ERR_UNSUPPORTED from fg_net_create, naming
                             * the layer), ANY channel counts -- forward, data gradient and parameter gradients all run;
                             * q = factor f of cudnn.SpatialConvolutionUpsample (0/1: none; f > 1: b = nOutputPlane * f * f planes, the
                             * NCHW output re-viewed as [b / f^2][H * f][W * f], layers/cudnnSpatialConvolutionUpsample.lua:14-31) */
    FG_BATCHNORM = 6,       /* nn.SpatialBatchNormalization(a=nF), p=eps, q=momentum */
    FG_SPATIAL_DROPOUT = 7, /* nn.SpatialDropout(p) */
    FG_AVGPOOL2 = 8,        /* nn.SpatialAveragePooling(2,2,2,2) */
    FG_DROPOUT = 9,         /* nn.Dropout(p) (v2) */
    FG_SIGMOID = 10,        /* nn.Sigmoid */
    FG_LEAKYRELU = 11,      /* LeakyReLU.lua, p = negative slope */
    FG_MAXPOOL2 = 12,       /* nn.SpatialMaxPooling(2,2) (models_c2f.lua:251, 256) */
    /* nn.ConcatTable{nn.Sequential, ...} -> nn.JoinTable(2) (models.lua:110-316, 322-376: the discriminators create_D16*, create_D32)
     * as markers inside the flat spec list:
     *   FG_CONCAT_TABLE(a = n)  FG_BRANCH  <layers of branch 1>  FG_BRANCH  <layers of branch 2> ...  FG_JOIN_TABLE  <tail layers>
     * Every branch sees the net's input; FG_JOIN_TABLE lays the branches' per-sample feature vectors side by side in branch order
     * and the layers behind it read that row.  The markers count as layers for every `layer_index` (fg_net_param_offset reports no
     * parameters for them, fg_net_layer_output is refused for them).  The flat parameter / gradient vector is in the reference's
     * order -- branch 1, branch 2, ..., tail (Module:parameters()) -- and the dropout masks are numbered in module order, branches
     * first.  The gradient wrt the input is the SUM of the branches' input gradients, added in the fixed order
     * ((branch 1 + branch 2) + branch 3) + branch 4 (nn.ConcatTable:updateGradInput).
     * Built: ONE table per net, as its first layer, not nested, 2 to 4 branches, every branch ending in a per-sample feature
     * vector (nn.Linear [+ PReLU [+ Dropout]]), no SpatialBatchNormalization inside a branch.  Anything else is refused by
     * fg_net_create (FG_ERR_UNSUPPORTED / FG_ERR_INVALID, the message names the layer).
     * fg_net_backward_range / fg_net_stage_params and fg_gan_set_comm(..., overlap = 2) work on such a net like on a chain: the
     * stages are [branch 1][branch 2]...[join][tail], the reverse walk splits the gradient at the join stage (which owns no
     * parameters) and sums the input gradients behind stage 0. */
    FG_CONCAT_TABLE = 13,   /* nn.ConcatTable with a = number of branches */
    FG_BRANCH = 14,         /* the next branch (an nn.Sequential) starts; appears `a` times */
    FG_JOIN_TABLE = 15      /* nn.JoinTable(2): closes the table */
};
typedef struct fg_layer_spec {
    int type;
    int a, b, c, d;
    float p, q;
} fg_layer_spec;

/* CALL ORDER (fg_net_*).  A net carries state from call to call -- the plan of the last forward, packed copies of its weights, what
 * a paused or ranged pass has left -- and none of it may show in a result: whatever ran before, a call gives the bits a freshly created
 * net bound to the same vectors gives (tests/CALL_ORDER.md lists every field and the scenario that would see it stale).
 *   Legal, at any batch up to the one the workspace was sized for and in any order: forwards at changing batches and in changing
 *   modes (train / evaluate); a forward without a backward; fg_net_backward any number of times after ONE train forward (the gradient
 *   vector is overwritten, never accumulated, so the second call leaves the bits of the first); FG_BWD_PARAM_GRADS and
 *   FG_BWD_INPUT_GRAD in two calls instead of one; fg_net_backward_range over any descending split of the stages; a NEW forward at any
 *   time -- it abandons a paused pass (FG_PAUSED_SYNC not resumed) and an unfinished range, also when it is itself refused: neither
 *   _resume entry continues over the plan of a forward that never ran; fg_net_forward after fg_net_forward_to
 *   (the output is in the workspace again); fg_set_math and fg_set_fusion between any two calls, also between a forward and its
 *   backward (a PReLU backward that leaves or joins its neighbour's epilogue that way sums its slope gradient in another order; a
 *   net created with FG_FUSE_WFINISH_BATCH cleared keeps reducing per layer when the bit is set later); fg_net_bind to other vectors,
 *   and any write to the parameter vector that is followed by fg_net_params_changed.
 *   Refused with FG_ERR_INVALID, nothing launched: fg_net_backward / fg_net_backward_range unless the LAST forward call was a train
 *   forward at that batch that ran to its end -- not after an evaluate forward, and not after a forward that was itself refused
 *   (FG_ERR_WORKSPACE, a bad batch, missing masks ...), failed or is still paused: the workspace then does not hold that batch's
 *   activations; fg_net_backward_range that does not start at the last stage or continue exactly where the previous call of the SAME
 *   forward stopped; fg_net_forward_resume / fg_net_backward_resume when that pass is not paused; fg_net_layer_output of the last
 *   layer while fg_net_forward_to has redirected it.
 *
 * WHAT IS FUSED, AND WHEN NOT (decided by fg_net_create from what stands next to what; a list that misses a precondition runs as
 * separate stages with the same results -- tests/NET_FUSIONS.md has one small net on each side of every line):
 *   Linear + View(C, H, W)                one stage, output written in NHWC.  Its bias gradient takes one kernel up to batch 1024 and a
 *                                         column sum + transpose above.  A BatchNorm behind it computes its own statistics, and a
 *                                         PReLU + SpatialDropout + AvgPool behind it does not sum its split-K partials.
 *   View(features) + Linear               the Linear reads the map in NHWC; PReLU / Dropout / LeakyReLU may stand between the two.
 *                                         Linear(-> 1) behind a spatial flatten is refused (FG_ERR_UNSUPPORTED).
 *   Linear(-> 1) [+ Sigmoid]              one matrix-vector stage.
 *   UpSamplingNearest(2) + conv           one tap-folded convolution when nIn % 4 == 0, nIn > 4, nOut > 4, k <= 5, stride 1 and no
 *                                         factor; else the upsampled map is materialised.
 *   conv(-> 1 | 3 | 4 planes) + Sigmoid   one stage (the layers fg_thin_layer names; not with a factor > 1: the view stands between).
 *   BatchNorm [+ PReLU]                   one stage; directly behind a convolution or a plain Linear that did not split K (and not in
 *                                         the bf16x6 math mode) the batch statistics come from that layer's epilogue.
 *   PReLU + SpatialDropout + AvgPool      one stage when C % 4 == 0 and H, W are even, also as the net's first stage.
 *   PReLU + MaxPool [+ Dropout]           one stage when C % 4 == 0, H, W are even and the PReLU is not layer 0.
 *   PReLU [+ Dropout]                     forward: written by the producing convolution / Linear (its epilogue when it did not split
 *                                         K and there is no mask, else the pass that sums the splits); backward: folded into the
 *                                         layer behind it (FG_FUSE_PRELU): in that layer's epilogue where it does not split K and
 *                                         runs an fp32 kernel, in the pass that sums its splits (any math mode, C % 4 == 0) where it
 *                                         does; not when the PReLU is the net's first stage or the first of a ranged call. */
int fg_net_create(fg_ctx* ctx, const fg_layer_spec* layers, int n_layers, int in_c, int in_h, int in_w, fg_net** out);
int fg_net_destroy(fg_net* net);
long long fg_net_num_params(const fg_net* net);   /* length of the flat parameter vector (reference order) */
long long fg_net_num_buffers(const fg_net* net);  /* BN running_mean||running_var per BN layer, module order */
int fg_net_num_masks(const fg_net* net);          /* dropout layers, module order */
long long fg_net_mask_elems(const fg_net* net, int mask_index, int batch);
float fg_net_mask_keep(const fg_net* net, int mask_index);   /* Bernoulli keep probability 1 - p of that dropout layer */
int fg_net_out_dims(const fg_net* net, int* c, int* h, int* w);
/* covers fg_net_forward / fg_net_backward at EVERY batch from 1 to max_batch (the need is not monotone in the batch: smaller batches
 * may split their reductions further), so it never shrinks as max_batch grows */
size_t fg_net_workspace_bytes(const fg_net* net, int max_batch);
/* offsets (in floats) of layer `layer_index`'s weight / bias inside the flat vector; -1 if it has none */
int fg_net_param_offset(const fg_net* net, int layer_index, long long* weight_off, long long* weight_n,
                        long long* bias_off, long long* bias_n);
/* persistent device pointers: flat params, flat grads (may be NULL for inference), BN buffers (may be NULL) */
int fg_net_bind(fg_net* net, float* params, float* grads, float* buffers);
int fg_net_params_changed(fg_net* net); /* call after the optimizer touched `params` (re-packs lazily) */
/* Module:forward.  x: NHWC [batch][in_h][in_w][in_c].  masks: one device pointer per dropout layer
 * (0/1 keep masks: SpatialDropout [batch][C]; Dropout [batch][features in internal NHWC order]); ignored when
 * train == 0.  Activations stay in `ws` for fg_net_backward.  *out_offset = float offset of the output
 * (NHWC [batch][out_h][out_w][out_c]) inside ws. */
int fg_net_forward(fg_net* net, int batch, const float* x, void* ws, size_t ws_bytes, int train,
                   const float* const* masks, int n_masks, long long* out_offset);
/* fg_net_forward whose LAST stage writes its output to `out` (device, NHWC, 16-byte aligned) instead of into the workspace:
 * a producer net hands its result straight to the consumer's input buffer (G -> D's batch, adversarial.lua:252-256). */
int fg_net_forward_to(fg_net* net, int batch, const float* x, void* ws, size_t ws_bytes, int train,
                      const float* const* masks, int n_masks, long long* out_offset, float* out);
int fg_net_in_dims(const fg_net* net, int* c, int* h, int* w);
int fg_net_vectors(const fg_net* net, float** params, float** grads, float** buffers);   /* what fg_net_bind attached */
int fg_net_max_bn_channels(const fg_net* net);
enum { FG_BWD_PARAM_GRADS = 1, FG_BWD_INPUT_GRAD = 2 };
/* Module:backward after a train-mode forward with the same (batch, x, ws).  gy: grad wrt the output.
 * FG_BWD_PARAM_GRADS writes (overwrites: the reference zeroes before every feval, adversarial.lua:92, 193)
 * the flat gradient vector; FG_BWD_INPUT_GRAD writes gx (NHWC like x). */
int fg_net_backward(fg_net* net, int batch, const float* x, const float* gy, void* ws, size_t ws_bytes, int flags,
                    float* gx);
/* Bucketed backward for data parallelism: the plan's stages run output -> input; fg_net_backward_range executes stages
 * [stage_from .. stage_to] (descending; the first call starts at fg_net_num_stages()-1 with gy, later calls continue
 * where the previous one stopped and ignore gy), so the host can start the RCCL all-reduce of the gradient range
 * fg_net_stage_params() reports for the finished stages while the remaining stages still compute. */
int fg_net_num_stages(const fg_net* net);
int fg_net_stage_params(const fg_net* net, int stage, long long* param_lo, long long* param_hi);
int fg_net_backward_range(fg_net* net, int batch, const float* x, const float* gy, void* ws, size_t ws_bytes, int flags,
                          float* gx, int stage_from, int stage_to);
/* sync-BN (data parallelism with exact global-batch BatchNorm statistics): with sync on, fg_net_forward /
 * fg_net_backward[_range] return FG_PAUSED_SYNC (= 1) at every SpatialBatchNormalization after leaving
 * fg_net_sync_count() fp64 values [sum x | sum x^2 | rows] (backward: [sum dz | sum dz*xhat | rows]) in `sync_buf`;
 * the host sum-all-reduces that buffer across ranks and calls the matching *_resume, until FG_OK. */
enum { FG_PAUSED_SYNC = 1 };
int fg_net_set_sync_bn(fg_net* net, int on, double* sync_buf_dev, long long capacity_doubles);
long long fg_net_sync_count(const fg_net* net);
int fg_net_forward_resume(fg_net* net, long long* out_offset);
int fg_net_backward_resume(fg_net* net);
/* debugging / parity: activation after reference layer `layer_index` of the last forward (must end a stage) */
int fg_net_layer_output(const fg_net* net, int layer_index, long long* ws_offset, int* c, int* h, int* w);
/* debugging / parity: where the last train-mode forward left the batch mean / 1/sqrt(var + eps) of BatchNorm layer
 * `layer_index` inside ws (c floats each) -- what the backward pass recomputes the PReLU branch from */
int fg_net_bn_saved_stats(const fg_net* net, int layer_index, long long* mean_offset, long long* invstd_offset, int* c);

/* ---- criterion: nn.BCECriterion() (train.lua:148) fused forward+backward, plus D's confusion counts
 *      (adversarial.lua:112-117): confusion[pred*2 + target] ---- */
int fg_bce_forward_backward(fg_ctx* ctx, const float* prob, const float* target, int n, float* loss_dev,
                            float* grad_dev, int* confusion_dev);

/* ---- optimizers on the flat vectors (interruptable_optimizers.lua:7-167) with the penalty and clamp of
 *      adversarial.lua:103-123 / 218-228 fused in:  g' = clamp(gscale*g + l1_mul*sign(p) + l2*p, +-clamp).
 *      Hyper-parameters are doubles (Lua numbers): 1-beta, the bias corrections and the step size are evaluated in
 *      double on the host exactly like interruptable_optimizers.lua:78-88, then rounded to fp32 once.
 *      Alignment: every vector (p, g, m, v, mom_buf, variance, g_out) needs 4 bytes only, at any n >= 0.
 *      Non-finite gradients: the clamp is compare-and-select, as TH's clamp and numpy's clip are.  A NaN gradient stays NaN with
 *      the clamp on or off -- the parameter, the optimizer state and g_out of that element become NaN, under all three rules and
 *      in the fused Adam + re-pack launch of the step level -- and +-inf under a clamp becomes +-clamp.  A finite gradient keeps
 *      its bits.  (A NaN PARAMETER reaches g' only through the penalty term.) ---- */
int fg_adam_fused(fg_ctx* ctx, float* p, const float* g, float* m, float* v, long long n, float gscale, float l1_mul,
                  float l2, float clamp, double lr, double beta1, double beta2, double eps, int t, float* g_out);
int fg_sgd_fused(fg_ctx* ctx, float* p, const float* g, float* mom_buf, long long n, float gscale, float l1_mul,
                 float l2, float clamp, double lr, double momentum, double dampening, double weight_decay, int nesterov,
                 int first_step);
int fg_adagrad_fused(fg_ctx* ctx, float* p, const float* g, float* variance, long long n, float gscale, float l1_mul,
                     float l2, float clamp, double clr);
/* out2[0] = ||p||_1, out2[1] = ||p||_2^2 (torch.norm of adversarial.lua:105-106); scratch >= 1024 floats.  The squares and their
 * partial sums are fp32 (the final sum of the partials is double, stored as fp32): out2[1] is +inf as soon as a square or a block's
 * sum exceeds FLT_MAX -- from |p_i| ~ 1.8e19 on, although ||p||_2 itself is representable -- and squares below 2^-149 count as 0.
 * A NaN element makes both results NaN; an infinite one makes both +inf. */
int fg_norms(fg_ctx* ctx, const float* p, long long n, float* out2_dev, float* scratch);

/* ---- data parallelism: one process (rank) per GPU, RCCL over xGMI (SURVEY.md 8(b) `fg_allreduce_sum(fg_comm*, ...)`, 8(e)).
 *      The reference has no multi-GPU path (train.lua:79 selects one device); BASELINE configs 3 and 5 shard the batch
 *      and sum-all-reduce the flat gradient vector of the net being updated.  librccl is bound at run time (dlopen; an
 *      instance already loaded by the host process is shared; FG_RCCL_LIB overrides the search).
 *      Bootstrap: rank 0 calls fg_comm_unique_id and hands the FG_COMM_ID_BYTES bytes to every rank through any host
 *      channel (file, environment, socket, torch.distributed store); every rank then calls fg_comm_create, which is
 *      collective.  fg_allreduce_sum* / fg_broadcast are in-place and stream-ordered on the context's stream;
 *      fg_allreduce_sum_async runs the exchange on the communicator's own stream after everything enqueued so far and
 *      returns at once -- fg_comm_wait makes the context's stream wait for every exchange issued that way. ---- */
enum { FG_COMM_ID_BYTES = 128 };
int fg_comm_unique_id(fg_ctx* ctx, char* id_out, size_t len);
int fg_comm_create(fg_ctx* ctx, const char* id, size_t len, int rank, int world, fg_comm** out);
int fg_comm_destroy(fg_comm* comm);
int fg_comm_rank(const fg_comm* comm);
int fg_comm_world(const fg_comm* comm);
const char* fg_comm_library(void);   /* which librccl was bound ("" before the first fg_comm_* call) */
int fg_allreduce_sum(fg_comm* comm, float* buf, size_t n);
int fg_allreduce_sum_async(fg_comm* comm, float* buf, size_t n);
int fg_comm_wait(fg_comm* comm);
int fg_allreduce_sum_f64(fg_comm* comm, double* buf, size_t n);   /* sync-BN sums */
int fg_allreduce_sum_i32(fg_comm* comm, int* buf, size_t n);      /* confusion counts of the global batch */
int fg_broadcast(fg_comm* comm, float* buf, size_t n, int root);  /* identical initial replicas */
/* The collective schedule.  fg_comm_set_trace(comm, 1) records every exchange call made on the communicator from then on;
 * fg_comm_schedule writes one line per call, "<seq> <op> <dtype> <count> <stream>" -- op allreduce / broadcast / wait, stream
 * "compute" (the context's stream) or "side" (the communicator's own) -- and optionally clears the record.  Every rank of a job
 * must produce the same text: a mismatch is a hang on real hardware.
 * fg_comm_create_dry builds a communicator of `world` ranks with NO transport underneath: its collectives are recorded (tracing is
 * on from the start) and otherwise skipped, so one process -- with a planning-only context not even a GPU -- can walk the exact
 * exchange path rank `rank` of an N-GPU job takes inside fg_step_D / fg_step_G (bench.py --dry-collective).  It is valid on a
 * device context too: a step then runs every kernel of that path and computes BatchNorm from the LOCAL batch statistics (the
 * skipped f64 sum leaves the rank's own sums and row count), the LOCAL gradient, and the update from that gradient x 1 / world. */
int fg_comm_create_dry(fg_ctx* ctx, int rank, int world, fg_comm** out);
int fg_comm_set_trace(fg_comm* comm, int on);
int fg_comm_schedule(fg_comm* comm, char* buf, size_t len, int reset);

/* ---- step level (SURVEY.md 8(b) level (ii)): the two closures of the training loop as device-resident entries.
 *      fg_step_D = adversarial.lua:240-268 (batch assembly: B/2 real || B/2 fakes from G in TRAIN mode) + fevalD (:83-179:
 *                  D forward, BCECriterion, D backward, confusion counts) + penalty / clamp (:103-123) + the optimizer
 *                  (interruptable_optimizers.lua) on D's flat vectors;
 *      fg_step_G = adversarial.lua:275-288 + fevalG_on_D (:187-231): G forward on B noises, D forward, BCE against all
 *                  ones, D backward to its input only (MODEL_D.modules[1].gradInput, :210), G backward, optimizer on G.
 *      table_inputs = 1: adversarial_c2f.lua:40-187 -- G{noise[B,S,S,1], cond[B,S,S,C]} (JoinTable) -> diff image,
 *                  D{x, cond} (CAddTable); cond_* are device NHWC.
 *      The nets are fg_net objects bound to their flat vectors (fg_net_bind); their workspaces are the caller's
 *      (fg_gan_bind_workspaces: fg_net_workspace_bytes(net, max_batch) each) plus one workspace of the step object itself.
 *      noise / masks == NULL: drawn by the library, all of a closure in one Philox launch up to 12 segments (the noise and one
 *      per dropout layer of D; one more launch per further 12), keyed by fg_gan_set_seeds; otherwise
 *      noise = device [rows][noiseDim] (table mode [rows][S][S][1]), masks = fg_net_num_masks(D) device pointers.
 *      FG_STEP_NO_UPDATE: stop before the optimizer (gradients stay in the bound gradient vector, un-reduced);
 *      The second half of D's batch in a D-step is G's output: G's last stage writes it in place where (B/2) * C*H*W is a multiple
 *      of 4 (that half then starts on 16 bytes); at any other size G keeps its output and one copy places it.  Every even batch
 *      from 2 to max_batch is steppable at every image size.
 *      fg_gan_update applies it later -- the maxAccuracyD gate of adversarial.lua:124-178 reads the confusion counts in
 *      between (FG_GAN_CONFUSION: int[0..3] this rank, int[4..7] the global batch, both [pred*2 + target]); never calling
 *      fg_gan_update IS interruptableAdam's false,false path.
 *      fg_gan_set_comm: data parallelism -- gradients are sum-all-reduced over the communicator, scaled by 1/world inside
 *      the optimizer pass, clamp after the reduce; D's exchange overlaps the next generator forward (its update is deferred
 *      until D is next evaluated or fg_gan_finish_pending), G's is bucketed under its own backward; sync_bn = exact
 *      global-batch BatchNorm statistics (fp64 sums reduced at every BatchNorm).  overlap: 0 = blocking exchange, 1 =
 *      overlapped, 2 = overlapped even on a one-rank communicator (exercises the N > 1 path on one GPU). ---- */
/* CALL ORDER (fg_gan_*).  Steps may follow each other in any order and at any even batch from 2 to max_batch (an epoch's short last
 * batch), and the nets may be used between them by anything that leaves their vectors alone -- an fg_sampler on the same nets and
 * workspaces, fg_net_forward in either mode: the next step gives the bits it would have given without the visit.
 *   A FG_STEP_NO_UPDATE step holds its gradients for fg_gan_update until the next step of the SAME kind overwrites them; a step of the
 *   other kind in between does not disturb them (a G-step forms no gradients of D).  fg_gan_update with nothing held -- never stepped,
 *   already applied, or overwritten by a later step -- is refused (FG_ERR_INVALID).  The step count moves only when an update is
 *   applied.  FG_GAN_CONFUSION int[4..7] (the global batch) is written by FG_STEP_NO_UPDATE D-steps only: it is the gate's input and
 *   keeps the counts of the last gated step through plain ones.
 *   Library-drawn noise and masks: every draw of `count` floats advances its offset by ceil(count / 4), the noise of a closure being
 *   fg_rng_uniform(noise_seed, noise_offset, count, -1, 1); explicit noise / masks leave the offsets alone.  A step that is REFUSED
 *   (an odd batch, one above max_batch, a null input, a bound workspace that is too small, ...) leaves both offsets where they were,
 *   whether or not it had drawn already: the next accepted step gives the bits it would have given without the refused call.
 *   fg_gan_get_offsets reads them.
 *   Save / restore: both parameter vectors, the BatchNorm buffers, FG_GAN_OPT_STATE_D / _G and fg_gan_optimizer_steps, put back with
 *   copies, fg_gan_set_optimizer (first), fg_gan_set_optimizer_steps and fg_gan_set_seeds, continue a run bit for bit under every rule:
 *   fg_gan_set_optimizer_steps(n > 0) also tells SGD that its momentum buffer already holds a gradient.
 *   fg_gan_set_optimizer in mid-run: with the rule the net already has (method unchanged) only the hyper-parameters change -- state
 *   and step count stay; with ANOTHER rule the net's state buffer is zeroed, its step count returns to 0 and SGD's first-step rule
 *   (the momentum buffer starts as the first gradient) is armed again. */
enum { FG_STEP_NO_UPDATE = 1 };
enum fg_gan_buffer_id {
    FG_GAN_D_INPUT = 0,       /* D's batch, NHWC [B][H][W][C]: real || fake (D-step), G's samples (G-step)            */
    FG_GAN_NOISE = 1,         /* the noise the last closure used when the library drew it                              */
    FG_GAN_D_GRAD_INPUT = 2,  /* G-step: d loss / d samples                                                           */
    FG_GAN_LOSS = 3,          /* float[2]: BCE of the last D-step, of the last G-step (0 until that step has run)      */
    FG_GAN_CONFUSION = 4,     /* int[8] (same storage as floats): local counts, global counts (0 until a D-step ran)  */
    FG_GAN_OPT_STATE_D = 5,   /* 2 * nparams(D): Adam m | v   (SGD: momentum buffer; Adagrad: variance)                */
    FG_GAN_OPT_STATE_G = 6,
    FG_GAN_D_OUTPUT = 7,      /* D's probabilities [B] of the last closure (count = ITS batch, whichever kind it was); offset
                                 relative to D's OWN workspace                                                         */
    FG_GAN_D_MASKS = 8,       /* dropout masks the library drew (fg_gan_mask_offset per mask)                          */
    FG_GAN_SYNC_BUF = 9       /* sync-BN exchange buffer (doubles; count is in floats): what fg_gan_set_comm bound to both nets */
};
size_t fg_gan_workspace_bytes(const fg_net* G, const fg_net* D, int table_inputs, int max_batch);
int fg_gan_create(fg_ctx* ctx, fg_net* G, fg_net* D, int table_inputs, int max_batch, void* ws, size_t ws_bytes,
                  fg_gan** out);
int fg_gan_destroy(fg_gan* gan);
int fg_gan_bind_workspaces(fg_gan* gan, void* wsG, size_t wsG_bytes, void* wsD, size_t wsD_bytes);
int fg_gan_set_comm(fg_gan* gan, fg_comm* comm, int sync_bn, int overlap);
int fg_gan_set_seeds(fg_gan* gan, uint64_t noise_seed, uint64_t noise_offset, uint64_t mask_seed, uint64_t mask_offset);
int fg_gan_get_offsets(const fg_gan* gan, long long* noise_offset, long long* mask_offset);  /* where the next draws start */
int fg_gan_set_penalty(fg_gan* gan, int which, float l1, float l2, float clamp);             /* which: 0 = D, 1 = G */
/* method 0 adam / 1 sgd / 2 adagrad (OPT.*_optmethod); lr < 0: the rule's default (1e-3); dampening < 0: = momentum */
int fg_gan_set_optimizer(fg_gan* gan, int which, int method, double lr, double beta1, double beta2, double eps,
                         double momentum, double dampening, double weight_decay, double lr_decay, int nesterov);
int fg_gan_optimizer_steps(const fg_gan* gan, int which);          /* Adam's t / optim.sgd's evalCounter */
int fg_gan_set_optimizer_steps(fg_gan* gan, int which, int steps);
/* offset (in floats, relative to the step workspace unless noted) and length of a result / state buffer */
int fg_gan_buffer(const fg_gan* gan, int what, long long* offset_floats, long long* count);
long long fg_gan_mask_offset(const fg_gan* gan, int mask_index);
int fg_step_D(fg_gan* gan, int batch, const float* real, const float* cond_real, const float* cond_fake,
              const float* noise, const float* const* masks, int flags);
int fg_step_G(fg_gan* gan, int batch, const float* cond, const float* noise, const float* const* masks, int flags);
int fg_gan_update(fg_gan* gan, int which);
int fg_gan_finish_pending(fg_gan* gan);
int fg_gan_pending(const fg_gan* gan);   /* 1 while D's update is deferred behind its gradient all-reduce */
/* test hook: G's overlapped backward exchanges its gradient in buckets of about 900000 parameters, cut at stage boundaries from the
 * last stage to the first; this re-cuts them at `floats` each, so that a small G has more than one */
int fg_test_set_gan_bucket_target(fg_gan* gan, long long floats);

/* ---- sampler level: sample.lua:80-89 and NN_UTILS.visualizeProgress (nn_utils.lua:131-204) as device-resident entries ----
 * Two module-level operations, usable alone, and one object built from them.
 *
 * fg_rank_scores = the sort of NN_UTILS.sortImagesByPrediction (nn_utils.lua:99-106): order_out[r] (device int[n]) is the 0-based
 *   index of the score at rank r.  Lua's table.sort leaves the order of equal scores undefined and D's sigmoid saturates to exactly
 *   1.0f, so the order is FIXED here: descending = (score high -> low, index low -> high), ascending = (score low -> high, index
 *   low -> high); -0.0f ties with +0.0f; NaN scores come last in both directions, lowest index first.  No atomics: the result does
 *   not depend on scheduling.  1 <= n <= 1048576 (larger: FG_ERR_UNSUPPORTED, the message names n).  This implementation counts
 *   ranks instead of sorting and needs no scratch: fg_rank_scores_workspace_bytes is 0 and `scratch` may be NULL (the pair stays in
 *   the signature so that a sorting implementation can take its place).
 *
 * fg_image_grid = image.toDisplayTensor{input = images, nrow = nrow, padding = padding} of the Torch7 `image` package over the k
 *   images order[0..k-1] (order == NULL: 0..k-1) of images_nhwc [*][h][w][c].  The package is an un-vendored luarocks dependency
 *   of the reference, so this is a restatement of its documented behaviour -- PARITY UNPINNED, like fg_scale_bilinear:
 *   xmaps = min(nrow, k), ymaps = ceil(k / xmaps); grid_chw is [c][ymaps * (h + padding)][xmaps * (w + padding)] (CHW, what
 *   image.save takes); image j sits in cell (j / xmaps, j % xmaps) at offset padding / 2 (integer division) from the cell's corner;
 *   every element no image covers holds the maximum over the k selected images.  normalize = 1 maps the whole grid by
 *   (v - min) / (max - min), min / max over the k selected images (max == min: all 0); normalize = 0 keeps raw values.
 *   minmax_out: device float[2] = {min, max}, or NULL.  The reduction runs in a fixed order.
 *   Non-finite pixels: min and max are fmin / fmax reductions, which skip a NaN, so a NaN pixel stays NaN in the grid and changes
 *   no other element (all pixels NaN: min = +inf, max = -inf).  An infinite pixel IS an extremum: with normalize = 1 and max = +inf
 *   every finite pixel maps to 0 and the pixel itself and the padding (which holds the maximum) to NaN; min = -inf maps every
 *   finite pixel to NaN.
 *
 * fg_sampler: G and D are fg_net objects bound to their vectors; neither may be a table-input net (the c2f pair of fg_gan's
 *   table_inputs = 1 is refused, FG_ERR_UNSUPPORTED).  D may be any net that compiles to one plan, nn.ConcatTable ones included.
 *   ws: fg_sampler_workspace_bytes, 256-byte aligned; the nets' own workspaces hold `chunk` samples each
 *   (fg_sampler_bind_workspaces checks fg_net_workspace_bytes(net, chunk)).  Both nets run in EVALUATE mode (running BatchNorm
 *   statistics, dropout off): nothing they own changes.  Every entry stays on the context's stream and never synchronises.
 *   fg_sample_generate = createNoiseInputs + createImagesFromNoise (nn_utils.lua:35-69): noise == NULL draws n vectors with one
 *     Philox launch -- exactly fg_rng_uniform(seed, offset, n * noiseDim, -1, 1), the offset then advances by ceil(n * noiseDim / 4)
 *     -- else noise is a device [n][noiseDim] (16-byte aligned); G runs over chunks of `chunk` and a tail of n % chunk, each
 *     straight into its slice of FG_SAMPLER_IMAGES (NHWC [n][H][W][C]).
 *   fg_sample_score = the prediction loop of sortImagesByPrediction (nn_utils.lua:91-97) over the same chunks into
 *     FG_SAMPLER_PREDS; images != NULL scores a caller's device batch [n][H][W][C] instead (visualizeProgress plants a real face
 *     and a non-face among the samples).
 *   fg_sample = generate + score + both rankings (sample.lua:80-85): D runs ONCE per image -- the reference scores all images
 *     again for "worst", which in evaluate mode recomputes the same numbers -- and FG_SAMPLER_ORDER_DESC / _ASC hold both orders.
 *   chunk: the chunk's noise and image slices must start on 16 bytes (chunk * noiseDim and chunk * H * W * C multiples of 4; else
 *     fg_sampler_create refuses the chunk); a chunk that is not a multiple of 4 costs one small copy per chunk into PREDS. */
enum fg_sampler_buffer_id {
    FG_SAMPLER_NOISE = 0,       /* [max_images][noiseDim]: the noise the last fg_sample_generate drew                    */
    FG_SAMPLER_IMAGES = 1,      /* [max_images][H][W][C]                                                                 */
    FG_SAMPLER_PREDS = 2,       /* [max_images] D's probabilities                                                        */
    FG_SAMPLER_ORDER_DESC = 3,  /* int[max_images] (same storage as floats): best first                                  */
    FG_SAMPLER_ORDER_ASC = 4    /* int[max_images]: worst first                                                          */
};
size_t fg_rank_scores_workspace_bytes(int n);
int fg_rank_scores(fg_ctx* ctx, const float* scores, int n, int ascending, int* order_out, void* scratch, size_t scratch_bytes);
int fg_image_grid(fg_ctx* ctx, const float* images_nhwc, const int* order, int k, int c, int h, int w, int nrow, int padding,
                  int normalize, float* grid_chw, float* minmax_out);
size_t fg_sampler_workspace_bytes(const fg_net* G, const fg_net* D, int max_images);
int fg_sampler_create(fg_ctx* ctx, fg_net* G, fg_net* D, int max_images, int chunk, void* ws, size_t ws_bytes, fg_sampler** out);
int fg_sampler_destroy(fg_sampler* s);
int fg_sampler_bind_workspaces(fg_sampler* s, void* wsG, size_t wsG_bytes, void* wsD, size_t wsD_bytes);
int fg_sampler_set_seed(fg_sampler* s, uint64_t seed, uint64_t offset);
/* offset (in floats, relative to the sampler workspace) and length of a buffer */
int fg_sampler_buffer(const fg_sampler* s, int what, long long* offset_floats, long long* count);
int fg_sample_generate(fg_sampler* s, int n, const float* noise);
int fg_sample_score(fg_sampler* s, int n, const float* images);
int fg_sample(fg_sampler* s, int n, const float* noise);

/* ---- adversarial.approxParzen (adversarial_c2f.lua:305-344): dist[i] = || (gen[i] + cond) - fine ||_2 for the n
 *      generations of one example (torch.dist: squares accumulated in double), min_out[0] = min(1e10, min_i dist[i]).
 *      gen [n][elems]; cond, fine [elems]; all three in the same element order. ---- */
int fg_parzen_min_dist(fg_ctx* ctx, const float* gen, const float* cond, const float* fine, int n, long long elems,
                       float* dist, float* min_out);

/* ---- findClosestNeighboursOf (sample.lua:133-151): the nearest training image of each of q queries, as one streaming reduction
 *      over the training set.  The set is fed in chunks; the three result buffers are the state carried from chunk to chunk. ----
 * queries [q][elems] and rows [n][elems]: contiguous device floats in the same element order.  The rows of one call carry the global
 *   indices first_index .. first_index + n - 1.  best_d2 (device double[q]), best_index (device int[q]) and best_dist (device
 *   float[q]) hold the running result; first != 0 ignores what they hold and starts from (+inf, -1).
 * Distance: d2 = sum_e ((double)d_e)^2 with d_e = rows[i][e] - queries[j][e] rounded to fp32, the convention of THTensor_(dist)
 *   that the approxParzen entry above states.  torch.dist is a dependency of the reference that is not vendored -- PARITY UNPINNED,
 *   like the image grid entry.
 * Order rule: a row replaces the running best only with d2 < best_d2[j] (the strict `<` of sample.lua:142): the earliest row wins
 *   among equals, a later chunk never displaces an equal earlier one, and a NaN distance never wins.  After the call
 *   best_dist[j] = (float)sqrt(best_d2[j]), +inf while best_index[j] == -1.
 * Determinism: no atomics; the order in which the squares of one (query, row) pair are added depends on elems alone -- not on the
 *   row's place in the call, on n, on q or on alignment -- so equal rows give bit-equal d2, and best_d2 / best_index are
 *   bit-identical however the set is cut into calls.
 * Limits: any q >= 1 (the entry walks groups of up to 16 queries; every group reads the rows once); 1 <= n <= 1048576 per call
 *   (larger: FG_ERR_UNSUPPORTED, the message names n); first_index >= 0 and first_index + n <= 2^31 - 1; any elems >= 1.  Rows need
 *   4-byte alignment only: 16-byte loads are used where elems % 4 == 0 and both bases are 16-byte aligned, 4-byte loads of the same
 *   elements otherwise.  scratch (8-byte aligned) holds d2[q][n]: the workspace function's size; smaller is FG_ERR_WORKSPACE, and
 *   nothing outside that size is touched.  NULL or non-positive arguments: FG_ERR_INVALID.  The entry stays on the context's stream
 *   and never synchronises. */
size_t fg_nearest_workspace_bytes(int q, int n);
int fg_nearest_update(fg_ctx* ctx, const float* queries, int q, const float* rows, int n, long long elems, long long first_index,
                      int first, double* best_d2, int* best_index, float* best_dist, void* scratch, size_t scratch_bytes);

/* ---- dataset[i] for a set that lives in HBM (dataset.lua:66-69, dataset_c2f.lua:65-106; adversarial.lua:245 indexes the epoch's
 *      set once per sample): out[j] = set[idx[j]], j = 0 .. n-1, in one launch. ----
 * set: n_set images of c * h * w device floats, [n_set][c][h][w] (set_layout 1: the reference's tensors, and the order
 *   fg_nearest_update streams) or [n_set][h][w][c] (set_layout 0).  out: n images in out_layout, the convention of the `layout`
 *   argument of fg_scale_bilinear (0 is what fg_step_D's real / cond_* and the nets take).  All four combinations: two copy rows,
 *   two transpose through LDS (runs that are contiguous in the source are read, runs that are contiguous in the destination written).
 * idx: device int[n].  Repeated indices are legal (approxParzen's "one image nneighbors times" is one call).  An index outside
 *   [0, n_set) reads nothing and fills its image with quiet NaN (0x7fc00000): the device cannot refuse, and nothing outside `set`
 *   is ever read.  Nothing outside out[0 .. n * c * h * w) is written.
 * Sizes: n_set * c * h * w may exceed 2^31 floats (the image's base offset is 64-bit); c * h * w < 2^31.  Any c, h, w >= 1.
 * n == 0: FG_OK, nothing is launched.  NULL pointers, n_set / c / h / w < 1, n < 0, a layout other than 0 / 1 or an image of 2^31
 *   floats or more: FG_ERR_INVALID, nothing is launched.
 * Alignment: 4 bytes are enough.  16-byte accesses are used on a side whose base is 16-byte aligned and whose rows allow it
 *   (h * w % 4 == 0 on an NCHW side, c * h * w % 4 == 0 on an NHWC side and for a copy), 4-byte accesses of the same elements
 *   otherwise -- the rule fg_nearest_update states.  No scratch, no atomics, no synchronisation: one launch on the context's
 *   stream. */
int fg_gather_images(fg_ctx* ctx, const float* set, long long n_set, int c, int h, int w, int set_layout, const int* idx, int n,
                     float* out, int out_layout);

/* ---- dataset[i] under a fresh random transform: the augmentation of dataset/generate_dataset.py (19 warped copies of every face
 *      written to disk before training: flip, brightness, zoom, rotation, translation, bilinear warp with black fill, :43-48, :130)
 *      as a per-batch operation on a set that lives in HBM, gather + affine resample + gain + clamp + layout change in one launch:
 *        out[j][.][y][x] = clamp01( gains[j] * bilinear(set[idx[j]], sx, sy) ),  j = 0 .. n-1. ----
 * set, n_set, c, idx, n, set_layout, out_layout: as fg_gather_images; the set's images are hs x ws, the batch's ho x wo (they may
 *   differ: a set stored with a margin, 40x40, is cropped to 32x32 by the matrix alone).  All four layout pairs.
 * mats: device float [n][6], OUTPUT pixel (column x, row y, as fp32) -> SOURCE pixel coordinates:
 *     sx = (m0*x + m1*y) + m2        sy = (m3*x + m4*y) + m5
 *   All coordinate arithmetic is fp32, every operation rounded on its own in exactly this order (no fused multiply-add): the
 *   operation order of this comment is the contract, a numpy fp32 restatement matches bit for bit.  NULL: the identity for every
 *   image (ho == hs and wo == ws required).
 * fill 0, constant 0 (skimage warp(order=1, mode="constant", cval=0)): if !(sx > -1 && sx < ws && sy > -1 && sy < hs) -- tested in
 *   float before any conversion to int, so NaN, inf and huge coordinates land here -- the pixel is 0 and nothing is read.
 *   Otherwise x0 = floor(sx), fx = sx - x0, likewise y; the taps (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1) are a, b, c, d; a
 *   tap outside the image is 0.0f and is not read, a tap inside is read even at weight 0;
 *     top = a + (b - a)*fx,  bot = c + (d - c)*fx,  v = top + (bot - top)*fy.
 * fill 1, edge: sx = fminf(fmaxf(sx, 0), ws - 1), likewise sy, before the floor (a NaN coordinate becomes 0); the +1 taps that fall
 *   outside count as 0, at weight 0.
 * gains: device float [n]; the result is fminf(fmaxf(v * gains[j], 0), 1).  NULL: gain 1 and no clamp, so that an identity matrix
 *   reproduces fg_gather_images bit for bit (finite pixels; v = a + (b - a)*0).
 * An idx[j] outside [0, n_set) reads nothing and gives a quiet-NaN image (0x7fc00000), as fg_gather_images; repeated indices are
 *   legal.  Nothing outside out[0 .. n * c * ho * wo) is written; nothing outside set, idx[0 .. n), mats[0 .. 6n), gains[0 .. n) is
 *   read.  The image's base offset is 64-bit.  Any c, hs, ws, ho, wo >= 1.
 * n == 0: FG_OK, nothing is launched.  NULL set / idx / out, sizes < 1, n < 0, a layout or fill other than 0 / 1, mats == NULL with
 *   differing sizes, an output image of 2^31 floats or more: FG_ERR_INVALID, nothing is launched.  c * hs * ws > 16384 floats:
 *   FG_ERR_UNSUPPORTED, the message names the size -- a block keeps its source image in LDS, and 16384 floats are the 64 KB a launch
 *   gets without an attribute change (3 x 64 x 64 = 12288 is the largest image of the models here).
 * Alignment: 4 bytes are enough; the source image is read with 16-byte accesses when `set` is 16-byte aligned and c * hs * ws % 4
 *   == 0, the rule fg_gather_images states.  One launch on the context's stream (one block per output image), no scratch, no
 *   atomics, no synchronisation. */
int fg_warp_images(fg_ctx* ctx, const float* set, long long n_set, int c, int hs, int ws, int set_layout, const int* idx,
                   const float* mats, const float* gains, int n, float* out, int ho, int wo, int out_layout, int fill);

/* ---- the coarse-to-fine example under a fresh random transform (dataset_c2f.lua:49-61 applied to an augmented face): gather +
 *      warp + scale down + scale up + subtract in one launch.  With
 *        F = fg_warp_images(set, .., idx, mats, gains, n, F, s, s, out_layout, fill)
 *      the entry gives  fine = F,  coarse = image.scale(image.scale(F, cs, cs), s, s),  diff = F - coarse:  every written float equals,
 *      bit for bit, what fg_warp_images followed by fg_c2f_coarse_diff on its output gives (finite source pixels, indices inside
 *      the set). ----
 * set, n_set, c, hs, ws, set_layout, idx, mats, gains, n, out_layout, fill: as fg_warp_images; the batch's images are s x s, the
 *   coarse side is cs <= s.  mats == NULL is the identity (hs == ws == s required), gains == NULL gain 1 without the clamp.
 * fine, coarse, diff: each n images of c x s x s device floats in out_layout, or NULL: not wanted, nothing is written for it.  At
 *   least one is non-NULL.  All four layout pairs.
 * An idx[j] outside [0, n_set) reads nothing of `set` and fills image j of every requested output with quiet NaN (0x7fc00000) --
 *   a contract of its own: NaN - NaN has no pinned payload, so the composition does not define this case.
 * Nothing outside the requested outputs is written; nothing outside set, idx[0 .. n), mats[0 .. 6n), gains[0 .. n) is read.  The
 *   image's base offset is 64-bit.  No scratch argument, no atomics, no synchronisation: one launch on the context's stream, one
 *   block per image; the source image, the fine image and the cs x cs image live in LDS, the intermediate batches of the
 *   composition never reach HBM.
 * n == 0: FG_OK, nothing is launched.  NULL ctx / set / idx, all three outputs NULL, a size < 1, n < 0, a layout or fill other than
 *   0 / 1, cs > s, mats == NULL with differing sizes: FG_ERR_INVALID, nothing is launched.  c * hs * ws > 16384 or c * s * s > 16384
 *   floats: FG_ERR_UNSUPPORTED, the message names the size and the limit (two images of up to 64 KB -- the small one takes the
 *   source's place -- share the 160 KB of LDS of a compute unit).
 * Alignment: 4 bytes are enough; the source image is read with 16-byte accesses when `set` is 16-byte aligned and c * hs * ws % 4
 *   == 0, the rule fg_gather_images states; the outputs are written 4 bytes at a time. */
int fg_warp_c2f(fg_ctx* ctx, const float* set, long long n_set, int c, int hs, int ws, int set_layout, const int* idx,
                const float* mats, const float* gains, int n, int s, int cs, float* fine, float* coarse, float* diff, int out_layout,
                int fill);

/* ---- a face under a fresh random transform, cut from a photo of any size: the reference's whole pipeline per batch
 *      (dataset/generate_dataset.py:43-66 warps the 250 x 250 photo, cuts the 84 x 84 face window and resizes it; dataset.lua:95
 *      scales that with image.scale), so that rotations, shifts and zoom-out pull in real background and no fill.  Gather + warp in
 *      photo coordinates into a face window + image.scale to the face size + the coarse-to-fine fields, in one launch. ----
 * set, n_set, c, set_layout, idx, n, out_layout, fill, mats, gains: as fg_warp_images.  The only differences: the set's images (the
 *   photos) are hs x ws of ANY size -- a photo is never copied to LDS --, and the warp's output is the face window, hw x ww.
 * Stage 1, the warp:  W = fg_warp_images(set, .., idx, mats, gains, n, W, hw, ww, channel-major, fill).  The coordinate arithmetic
 *   and its operation order, the fp32 range test before any float-to-int conversion, the tap rules of both fills, the gain and the
 *   clamp are the ones fg_warp_images states.  mats == NULL is the identity (hw == hs and ww == ws required), gains == NULL gain 1
 *   without the clamp.  There is no window-origin argument: the matrix alone says where the window lies in the photo, as it does
 *   for a 40 x 40 set cropped to 32 x 32.  A tap outside the photo addresses nothing.
 * Stage 2, the scale:  F = image.scale(W, s, s) with the arithmetic of fg_scale_bilinear (the width pass nested in the height pass,
 *   per output element); hw == ww == s is the copy.  fine = F.
 * Stage 3, the coarse-to-fine fields, only with cs > 0:  coarse = image.scale(image.scale(F, cs, cs), s, s), diff = F - coarse, as
 *   fg_c2f_coarse_diff computes them.  cs == 0: no coarse-to-fine fields; coarse and diff must be NULL and fine non-NULL.
 * fine, coarse, diff: each n images of c x s x s device floats in out_layout, or NULL: not wanted, nothing is written for it.  With
 *   cs > 0 at least one is non-NULL.  All four layout pairs.
 * Bits: every written float equals, bit for bit, what fg_warp_images (to hw x ww), then fg_scale_bilinear (to s x s), then
 *   fg_c2f_coarse_diff give through HBM, wherever that composition exists; where fg_warp_images refuses the source size, the float
 *   the composition's stated arithmetic gives (every operation rounded on its own, no fused multiply-add).
 * An idx[j] outside [0, n_set) reads nothing of `set` and fills image j of every requested output with quiet NaN (0x7fc00000);
 *   repeated indices are legal.
 * Nothing outside the requested outputs is written; nothing outside set, idx[0 .. n), mats[0 .. 6n), gains[0 .. n) is read.  A
 *   photo's base offset is 64-bit, c * hs * ws < 2^31.  One launch on the context's stream, one block per face; no scratch
 *   argument, no atomics, no synchronisation, stateless.  The window, the face and the cs x cs image live in LDS (the cs x cs image
 *   takes the window's place), the intermediate batches of the composition never reach HBM.
 * n == 0: FG_OK, nothing is launched.  NULL ctx / set / idx, a size < 1 (cs < 0), cs > s, n < 0, a layout or fill other than 0 / 1,
 *   the NULL rules above broken, mats == NULL with differing sizes, a photo of 2^31 floats or more: FG_ERR_INVALID, nothing is
 *   launched.  FG_ERR_UNSUPPORTED, the message names the entry, the sizes and the limit, if the window, the face, the cs x cs image
 *   and the scale plans together do not fit the 160 KB of LDS of a compute unit:
 *     4 * (roundup4(max(c*hw*ww, c*cs*cs)) + c*s*s) + 28 * (3*s + cs), rounded up to 16  >  163840 bytes
 *   (roundup4: to a multiple of 4 floats; a scale plan is 28 bytes, one per coordinate of each of the four passes).
 *   3 x 84 x 84 -> 64 -> 32 takes 140096 bytes.
 * Alignment: 4 bytes are enough everywhere; photos and outputs are read and written 4 bytes at a time. */
int fg_warp_faces(fg_ctx* ctx, const float* set, long long n_set, int c, int hs, int ws, int set_layout, const int* idx,
                  const float* mats, const float* gains, int n, int hw, int ww, int s, int cs, float* fine, float* coarse, float* diff,
                  int out_layout, int fill);

/* ---- the three warps on a set held as 8-bit pixels: every pixel the reference loads is one byte of a JPEG divided by 255
 *      (image.load(.., "float"), dataset.lua:90 and :200), so a resident set kept as bytes takes a quarter of the HBM and loses
 *      nothing.  The bytes stay bytes in HBM and are decoded where they are read. ----
 * set: n_set images of c * hs * ws device bytes in set_layout.  The value of a byte b is
 *     p(b) = (float)b / 255.0f,
 *   the correctly rounded fp32 quotient (a true division: b * (1 / 255) is another float for 126 of the 256 bytes) -- what
 *   np.float32(b) / np.float32(255) gives, the float the host loaders produce.
 * Bits: every float an _u8 entry writes equals, bit for bit, what its fp32 sibling (the entry of the same name without the suffix)
 *   writes for the float set p(set) and the same other arguments: every layout pair, both fills, mats and gains NULL or given,
 *   every subset of fine / coarse / diff.  With mats == NULL and gains == NULL the entries decode: out[j] = p(set[idx[j]]).
 * Everything else is the sibling's contract: the meaning of every other argument, the refusals and their codes (a message names
 *   the _u8 entry), an idx[j] outside [0, n_set) reads nothing and gives a quiet-NaN image (0x7fc00000) in every requested output,
 *   the 64-bit base offset of an image, n == 0, nothing written outside the requested outputs, one launch on the context's stream
 *   with the sibling's grid, block and LDS size, no scratch, no atomics, no synchronisation.
 * Limits, unchanged and counted in pixels: c * hs * ws <= 16384 for fg_warp_images_u8 and fg_warp_c2f_u8 (the block's copy of the
 *   source image in LDS holds decoded floats), c * s * s <= 16384 for fg_warp_c2f_u8; fg_warp_faces_u8 takes photos of any size
 *   below 2^31 pixels under the LDS formula of fg_warp_faces.
 * Alignment: one byte is enough, for any base and any image size.  Nothing outside set[0 .. n_set * c * hs * ws) is read.  The copy
 *   of the source image (fg_warp_images_u8, fg_warp_c2f_u8) uses 16-byte loads only when `set` is 16-byte aligned and c * hs * ws
 *   % 16 == 0, 4-byte loads only when `set` is 4-byte aligned and c * hs * ws % 4 == 0, byte loads otherwise: no load reaches over
 *   the end of an image.  fg_warp_faces_u8 reads single bytes.  There is no fg_gather_images for bytes: the un-augmented pull of a
 *   byte set is the identity call (mats == NULL, gains == NULL) of fg_warp_images_u8 or fg_warp_faces_u8. */
int fg_warp_images_u8(fg_ctx* ctx, const uint8_t* set, long long n_set, int c, int hs, int ws, int set_layout, const int* idx,
                      const float* mats, const float* gains, int n, float* out, int ho, int wo, int out_layout, int fill);
int fg_warp_c2f_u8(fg_ctx* ctx, const uint8_t* set, long long n_set, int c, int hs, int ws, int set_layout, const int* idx,
                   const float* mats, const float* gains, int n, int s, int cs, float* fine, float* coarse, float* diff, int out_layout,
                   int fill);
int fg_warp_faces_u8(fg_ctx* ctx, const uint8_t* set, long long n_set, int c, int hs, int ws, int set_layout, const int* idx,
                     const float* mats, const float* gains, int n, int hw, int ww, int s, int cs, float* fine, float* coarse, float* diff,
                     int out_layout, int fill);

/* ---- grayscale from a resident byte set: the three warps on a set of R, G, B bytes read as luma.  The reference's grayscale mode
 *      (th train.lua --grayscale) loads every picture with image.load(path, 1, "float") (dataset.lua:90), the luma of the JPEG's RGB
 *      bytes, and scales that one channel (:95).  A luma pixel is no byte (for gray triples r = g = b it equals p(b) for only 191 of
 *      the 256 bytes), so the set stays the RGB bytes -- exact, and the one resident set serves colour and grayscale runs -- and the
 *      luma is formed where the bytes are read. ----
 * set: n_set images of 3 * hs * ws device bytes in set_layout: 0, pixel-major (the R, G, B of a pixel adjacent), or 1, three planes
 *   R, G, B of hs * ws bytes.  There is no c: three channels in, one out; the batch has one channel, its two layouts are one order,
 *   so there is no out_layout.  With p(b) = (float)b / 255.0f as above, the value of a pixel is
 *     Y(r, g, b) = ((0.299f * p(r)) + (0.587f * p(g))) + (0.114f * p(b))
 *   in fp32, every product and sum rounded on its own in this order (no FMA contraction); the three constants are the floats
 *   nearest to the decimals, 0x1.322d0ep-2, 0x1.2c8b44p-1, 0x1.d2f1aap-4.  This is Torch7's image.rgb2y on a float tensor
 *   (output:zero():add(0.299, R):add(0.587, G):add(0.114, B)); like the rest of the `image` package it is un-vendored: parity
 *   unpinned by the reference.  Y <= 1.0 for all 256^3 triples and white is exactly 1.0; the sum evaluated in double and rounded once
 *   is another float for 30 % of the triples.
 * Bits: every float a _u8_y entry writes equals, bit for bit, what its fp32 sibling (fg_warp_images, fg_warp_c2f, fg_warp_faces)
 *   writes with c = 1 for the float set Y(set) and the same other arguments: both fills, mats and gains NULL or given, every subset
 *   of fine / coarse / diff.  With mats == NULL and gains == NULL the entries decode: out[j] = Y(set[idx[j]]).
 * Everything else is the sibling's contract at c = 1: the refusals and their codes (a message names the _u8_y entry), an idx[j]
 *   outside [0, n_set) reads nothing and gives a quiet-NaN image (0x7fc00000) in every requested output, repeated indices, the
 *   64-bit base offset of an image, n == 0 (FG_OK without a launch), the NULL rules, cs <= s, a layout or fill other than 0 / 1 is
 *   FG_ERR_INVALID; nothing written outside the requested outputs; one launch on the context's stream, grid n, block 256, the LDS
 *   size of the sibling at c = 1, no scratch, no atomics, no synchronisation.
 * Limits, counted in luma floats: hs * ws <= 16384 for fg_warp_images_u8_y and fg_warp_c2f_u8_y (the block's copy in LDS holds the
 *   luma, a third of the image: sources up to 128 x 128, where three channels top out at 73 x 73), s * s <= 16384 for
 *   fg_warp_c2f_u8_y; fg_warp_faces_u8_y takes photos of any size below 2^31 bytes (3 * hs * ws) under the LDS formula of
 *   fg_warp_faces at c = 1.  Beyond these: FG_ERR_UNSUPPORTED with the size and the limit in the message; a photo of 2^31 bytes or
 *   more is FG_ERR_INVALID, as the sibling's is (offsets inside a photo are 32-bit).
 * Alignment: one byte is enough, for any base and any image size.  Nothing outside set[0 .. 3 * n_set * hs * ws) is read.  The copy
 *   of the source image (fg_warp_images_u8_y, fg_warp_c2f_u8_y) chooses its loads on the host, for either layout by one rule: with
 *   P = hs * ws, 16-byte loads only when `set` is 16-byte aligned and P % 16 == 0 (pixel-major: 3 P % 16 == 0, the same), 4-byte
 *   loads only when `set` is 4-byte aligned and P % 4 == 0, byte loads otherwise.  Planes: a lane takes 16 / 4 / 1 pixels from each
 *   of the three planes (the image's base 3 P i and the plane offsets P and 2 P are then aligned to the load); pixel-major: 16 / 4 /
 *   1 pixels as three loads of 48 / 12 / 3 contiguous bytes (the compiler may join the narrower ones: 12 bytes in one load, 3 as
 *   2 + 1).  No load reaches over the end of a plane or of an image.  fg_warp_faces_u8_y reads the twelve bytes of a window pixel
 *   (R, G, B of the four taps) as single bytes from planes, and from triples as the 2 bytes R, G (at any address) and the byte B;
 *   a tap outside the photo reads nothing. */
int fg_warp_images_u8_y(fg_ctx* ctx, const uint8_t* set, long long n_set, int hs, int ws, int set_layout, const int* idx,
                        const float* mats, const float* gains, int n, float* out, int ho, int wo, int fill);
int fg_warp_c2f_u8_y(fg_ctx* ctx, const uint8_t* set, long long n_set, int hs, int ws, int set_layout, const int* idx,
                     const float* mats, const float* gains, int n, int s, int cs, float* fine, float* coarse, float* diff, int fill);
int fg_warp_faces_u8_y(fg_ctx* ctx, const uint8_t* set, long long n_set, int hs, int ws, int set_layout, const int* idx,
                       const float* mats, const float* gains, int n, int hw, int ww, int s, int cs, float* fine, float* coarse, float* diff,
                       int fill);

/* ---- the random transforms of dataset/generate_dataset.py (:43-48 and its create_aug_matrices: flip, zoom, rotation, shear,
 *      translation, brightness) drawn, assembled into matrices and left on the device: the mats / gains of fg_warp_images and
 *      fg_warp_c2f for n images in one launch, no host arithmetic and no upload per batch. ----
 * spec: the ranges (host memory, read during the call only; it travels to the kernel by value).
 * mats: device float [n][6], output pixel -> source pixel, exactly the meaning fg_warp_images gives it.  gains: device float [n],
 *   or NULL: not wanted.  hs x ws: the images of the set; ho x wo: the images of the batch.
 * Stream: image j owns the quads offset + 3j, offset + 3j + 1 and offset + 3j + 2 of the Philox4x32-10 stream of fg_rng_uniform
 *   (counter = the quad's 64-bit number, modulo 2^64, in words 0 and 1, words 2 and 3 zero; key = seed lo / hi), twelve 32-bit
 *   words w0 .. w11 in the order the three quads give them.  The assignment is fixed whatever the spec enables: w0 horizontal
 *   flip, w1 vertical flip, w2 zoom x, w3 zoom y, w4 rotation, w5 shear, w6 tx, w7 ty, w8 gain, w9 .. w11 reserved.  The entry is
 *   stateless: n images at offset followed by m images at offset + 3n are the n + m images of one call at offset.
 * Picks: a flip iff its axis is enabled and w >> 31 == 1.  u(w) = (double)(w >> 8) * 2^-24.  zx = zoom_lo + u(w2) * (zoom_hi -
 *   zoom_lo); zy = zx if zoom_equal, else the same with w3; gain = (float)(gain_lo + u(w8) * (gain_hi - gain_lo)).  An integer
 *   pick (rotation and shear in whole degrees, tx and ty in whole output pixels) is
 *     lo + (int)(((uint64_t)w * (uint64_t)(hi - lo + 1)) >> 32):  no floating point is involved.
 * Angles: sin and cos of a whole number of degrees k are DEFINED here, not taken from a math library.  k is reduced to [0, 360);
 *   q = k / 90, r = k % 90.  For r <= 45: x = r * D, s0 = S(x), c0 = C(x); otherwise x = (90 - r) * D, s0 = C(x), c0 = S(x);
 *   D = 0x1.1df46a2529d39p-6 (pi / 180).  (sin, cos) = (s0, c0) for q = 0, (c0, 0.0 - s0) for 1, (0.0 - s0, 0.0 - c0) for 2,
 *   (0.0 - c0, s0) for 3.  S(x) = x * P, P the Horner evaluation in z = x*x of the coefficients (-1)^i / (2i+1)! for i = 8 .. 0,
 *   starting from the i = 8 term (P = c8; P = P*z + c7; ..); C(x) the Horner evaluation of (-1)^i / (2i)! for i = 9 .. 0.  Each
 *   coefficient is the double nearest to that quotient.
 * Matrix, runtime.Augmenter.matrix in fp64 with r the rotation and s the shear:
 *     a = zx*cos r,  b = 0.0 - zy*sin(r+s),  c = zx*sin r,  d = zy*cos(r+s),  det = a*d - b*c,
 *     ia = d/det,  ib = (0.0-b)/det,  ic = (0.0-c)/det,  id = a/det,
 *     cx = wo/2,  cy = ho/2 (integer division),  qx = cx+tx,  qy = cy+ty,
 *     m = [ia+0.0, ib+0.0, (cx-(ia*qx+ib*qy))+(ws-wo)/2.0, ic+0.0, id+0.0, (cy-(ic*qx+id*qy))+(hs-ho)/2.0];
 *   a horizontal flip then gives m[0:3] = [0.0-m0, 0.0-m1, (ws-1)-m2], a vertical one the same for m[3:6] with hs.  Each entry is
 *   rounded once to fp32.
 *   All of it is fp64 and every operation is rounded on its own, in the order written (no fused multiply-add: the kernel is
 *   compiled under `fp contract(off)`): a numpy float64 restatement equals the device bit for bit.  A neutral spec gives exactly
 *   [1, 0, (ws-wo)/2, 0, 1, (hs-ho)/2] and gain exactly 1.
 * Exactly mats[0 .. 6n) and gains[0 .. n) are written; nothing on the device is read.  4-byte alignment is enough.  One launch of
 *   one kernel on the context's stream, one thread per image; no LDS, no scratch, no atomics, no synchronisation.
 * n == 0: FG_OK, nothing is launched.  NULL ctx / spec / mats, n < 0, a size < 1, a flag other than 0 / 1, lo > hi anywhere, a
 *   non-finite or non-positive zoom, a negative or non-finite gain, a shear outside -89 .. 89, an integer range wider than 2^31
 *   values: FG_ERR_INVALID, the message names the entry, nothing is launched. */
typedef struct fg_augment_spec {
    int hflip, vflip;                   /* 0 / 1: that axis is mirrored with probability 1/2 */
    int zoom_equal;                     /* 1: zy = zx */
    double zoom_lo, zoom_hi;            /* finite, 0 < lo <= hi */
    int rot_lo, rot_hi;                 /* whole degrees, lo <= hi (the reference draws randint) */
    int shear_lo, shear_hi;             /* whole degrees, -89 <= lo <= hi <= 89 */
    int tx_lo, tx_hi, ty_lo, ty_hi;     /* whole output pixels, lo <= hi */
    double gain_lo, gain_hi;            /* finite, 0 <= lo <= hi */
} fg_augment_spec;
int fg_draw_transforms(fg_ctx* ctx, const fg_augment_spec* spec, uint64_t seed, uint64_t offset, int n, int hs, int ws, int ho,
                       int wo, float* mats, float* gains);

/* ---- the c2f data step in front of the train closure (dataset_c2f.lua:49-61, `dataset._toResult`) ----
 * fg_scale_bilinear = image.scale(src, width, height) of the Torch7 `image` package (default mode 'bilinear'; un-vendored luarocks
 * dependency, restated in oracle/image_scale.py): width pass then height pass; per axis up-scaling interpolates with
 * (src - 1) / (dst - 1) ("corners onto corners"), down-scaling is a box mean with fractional end coverage, equal sizes copy.
 * Bit-for-bit the C float loop.  src [n][hs][ws][c] (layout 0 = NHWC, the library's activation layout) or [n][c][hs][ws]
 * (layout 1 = NCHW, the reference's image tensors); dst likewise at hd x wd.
 * fg_c2f_coarse_diff = the whole step: coarse = scale(scale(fine, cs, cs), s, s), diff = fine - coarse, for n square images of
 * side s; tmp holds n * c * cs * cs floats. */
int fg_scale_bilinear(fg_ctx* ctx, const float* src, float* dst, int n, int c, int hs, int ws, int hd, int wd, int layout);
int fg_c2f_coarse_diff(fg_ctx* ctx, const float* fine, float* coarse, float* diff, float* tmp, int n, int c, int s, int cs,
                       int layout);

/* ---- module-level ops (nn.Module protocol: updateOutput / updateGradInput / accGradParameters), NHWC ----
 * conv / linear take REFERENCE-layout weights and pack them into `ws` on the fly. */
/* fg_conv2d_workspace_bytes / fg_linear_workspace_bytes: what ANY of the three passes needs at this shape, whatever fg_set_math,
 * fg_set_fusion and fg_test_set_wino_wgrad_thresholds say when the pass runs (the functions take no context: the bound covers every
 * setting).  ws: 256-byte aligned; the passes read nothing of it that they did not write in the same call and write nothing
 * outside [ws, ws + ws_bytes).
 * Geometries: fg_conv2d_* take odd k <= 7 with pad = (k - 1) / 2 ('same', stride 1) at ANY channel counts, and the three passes
 * accept exactly the same ones: a geometry either runs forward, data gradient and weight gradient or gets the same error code from
 * all three.  Refused (FG_ERR_UNSUPPORTED) are only, with upsample2x = 1 (the folded nearest-x2 upsample):
 *   - k = 7 (the folded window needs more tap groups than the kernels hold), and
 *   - a THIN layer: 1 or 3 channels on one side (also 4 at k = 3) against 64, 128 or a multiple of 256 on the other.  Those layers
 *     have kernels of their own (the image-side convolutions of the models), without a folded form;
 * and, with either value of upsample2x:
 *   - a THIN layer whose wide operand, batch * h * w * max(cin, cout), has 2^31 floats (8 GiB) or more: its kernels index that
 *     operand with 32 bits.  Nothing is launched; fg_net_forward refuses such a layer of a net at that batch, naming the layer.
 * Every other layer with few channels on one side (2 channels; 4 at 5x5 / 7x7; widths such as 192 or 320) is an ordinary
 * convolution on zero-padded channel rows.  fg_net_create classifies a FG_CONV layer the same way.
 * Linear(in_f -> 1) runs as a matrix-vector product at any batch. */
size_t fg_conv2d_workspace_bytes(int batch, int h, int w, int cin, int cout, int k, int upsample2x);
int fg_conv2d_forward(fg_ctx* ctx, const float* x, const float* w_oihw, const float* bias, float* y, int batch, int h,
                      int w, int cin, int cout, int k, int pad, int upsample2x, void* ws, size_t ws_bytes);
int fg_conv2d_backward_data(fg_ctx* ctx, const float* gy, const float* w_oihw, float* gx, int batch, int h, int w,
                            int cin, int cout, int k, int pad, int upsample2x, void* ws, size_t ws_bytes);
/* gw = beta*gw + dW, gb = beta*gb + db (beta = 1: Torch's accumulate semantics) */
int fg_conv2d_backward_weight(fg_ctx* ctx, const float* x, const float* gy, float* gw_oihw, float* gb, float beta,
                              int batch, int h, int w, int cin, int cout, int k, int pad, int upsample2x, void* ws,
                              size_t ws_bytes);
size_t fg_linear_workspace_bytes(int batch, int in_f, int out_f);
int fg_linear_forward(fg_ctx* ctx, const float* x, const float* w, const float* bias, float* y, int batch, int in_f,
                      int out_f, void* ws, size_t ws_bytes);
int fg_linear_backward_data(fg_ctx* ctx, const float* gy, const float* w, float* gx, int batch, int in_f, int out_f,
                            void* ws, size_t ws_bytes);
int fg_linear_backward_weight(fg_ctx* ctx, const float* x, const float* gy, float* gw, float* gb, float beta,
                              int batch, int in_f, int out_f, void* ws, size_t ws_bytes);
/* SpatialBatchNormalization; slope != NULL fuses the following PReLU.  scratch >= fg_bn_scratch_floats(c) floats.
 * Value domain of the batch statistics: one pass over d = x - pivot (pivot = row 0 of the channel) with sum d and sum d^2 in fp32
 * partials of at most ceil(rows / min(ceil(rows / 64), 256)) rows each, everything behind the partials in fp64.  A constant channel
 * has variance exactly 0 (invstd = 1 / sqrt(eps)); rows = 1 leaves the running variance's unbiased factor at 1.  A pivot k standard
 * deviations from the mean costs (1 + k^2) 2^-24 relative in the variance per fp32 addition of a partial.  d^2 overflows fp32 for
 * |x - pivot| above 1.8e19 (sqrt(FLT_MAX) = 1.8447e19), a partial once the root mean square of |x - pivot| over its rows passes
 * 1.8447e19 / sqrt(rows of the partial): the statistics are then inf / NaN.  Pinned at max |x - pivot| = 7e17 (2^59.3) with 64 rows
 * per partial (tests/test_gpu_value_domain.py). */
long long fg_bn_scratch_floats(int c);
int fg_batchnorm_forward(fg_ctx* ctx, const float* x, float* y, long long rows, int c, const float* gamma,
                         const float* beta, const float* slope, float* save_mean, float* save_invstd,
                         float* running_mean, float* running_var, float eps, float momentum, int train,
                         float* scratch);
int fg_batchnorm_backward(fg_ctx* ctx, const float* x, const float* gy, float* gx, long long rows, int c,
                          const float* gamma, const float* beta, const float* slope, const float* save_mean,
                          const float* save_invstd, float* ggamma, float* gbeta, float* gslope, float acc,
                          float* scratch);
/* PReLU with an optional same-shape keep mask (x mscale): nn.PReLU [+ nn.Dropout]; scratch >= 1024 floats.  gslope sums x * g over
 * the units with !(x > 0) and SKIPS the others: a non-finite gradient at a positive input does not reach it.  The forms fused into
 * the thin-layer, implicit-GEMM (single-pass and split-K) and Linear(-> 1) data gradients of fg_net do the same (the Winograd epilogue multiplies by a selected
 * zero instead; a non-finite gradient is already NaN across its tile there). */
int fg_prelu_forward(fg_ctx* ctx, const float* x, const float* slope, const float* mask, float mscale, float* y,
                     long long n);
int fg_prelu_backward(fg_ctx* ctx, const float* x, const float* gy, const float* slope, const float* mask,
                      float mscale, float* gx, float* gslope, float acc, long long n, float* scratch);
/* fused nn.PReLU -> nn.SpatialDropout(mask [batch][c]) -> nn.SpatialAveragePooling(2,2,2,2) (models.lua:386-388) */
int fg_actpool_forward(fg_ctx* ctx, const float* x, const float* slope, const float* mask, float mscale, float* y,
                       int batch, int h, int w, int c);
int fg_actpool_backward(fg_ctx* ctx, const float* x, const float* gy, const float* slope, const float* mask,
                        float mscale, float* gx, float* gslope, float acc, int batch, int h, int w, int c,
                        float* scratch);
int fg_spatial_dropout_apply(fg_ctx* ctx, const float* x, const float* mask, float mscale, float* y, int batch, int hw,
                             int c);
/* h and w even (FG_ERR_INVALID otherwise, nothing is launched) */
int fg_avgpool2x2_forward(fg_ctx* ctx, const float* x, float* y, int batch, int h, int w, int c);
int fg_avgpool2x2_backward(fg_ctx* ctx, const float* gy, float* gx, int batch, int h, int w, int c);
int fg_upsample_nearest2x_forward(fg_ctx* ctx, const float* x, float* y, int batch, int h, int w, int c);
int fg_upsample_nearest2x_backward(fg_ctx* ctx, const float* gy, float* gx, int batch, int h, int w, int c);
/* cudnn.SpatialConvolutionUpsample, factor f > 1 (layers/cudnnSpatialConvolutionUpsample.lua:19-58): the flat re-view of the
 * convolution's NCHW output [batch][c][h][w] (c = nOutputPlane * f * f) as [batch][c / f^2][h * f][w * f], on NHWC tensors.
 * forward: conv output -> viewed output; backward: gradient wrt the viewed output -> gradient wrt the conv output. */
int fg_conv_upsample_view_forward(fg_ctx* ctx, const float* conv_out, float* viewed, int batch, int h, int w, int c, int factor);
int fg_conv_upsample_view_backward(fg_ctx* ctx, const float* g_viewed, float* g_conv_out, int batch, int h, int w, int c, int factor);
/* nn.SpatialMaxPooling(2,2): backward recomputes the argmax from the saved input.  h and w even, and for the forward pass c % 4 == 0
 * (FG_ERR_INVALID otherwise, nothing is launched).  The slot of a window, for the forward and the backward pass and for the fused
 * PReLU + max-pool stages of fg_net alike (one shared scan): the window's first NaN in scan order (dy, dx) if it holds one,
 * otherwise its first maximum; a tie stays with the earlier slot, -0 against +0 included.  The forward value is that slot's bits
 * (behind a fused PReLU: of slope * x, so a NaN's payload need not survive); the backward pass writes gy to that slot and +0 to
 * the other three. */
int fg_maxpool2x2_forward(fg_ctx* ctx, const float* x, float* y, int batch, int h, int w, int c);
int fg_maxpool2x2_backward(fg_ctx* ctx, const float* x, const float* gy, float* gx, int batch, int h, int w, int c);
/* nn.Dropout on any shape: y = x * mask * scale (mask NULL: y = x * scale) */
int fg_dropout_apply(fg_ctx* ctx, const float* x, const float* mask, float scale, float* y, long long n);
/* nn.JoinTable(2,2) / its backward split, nn.CAddTable on NHWC tensors (models_c2f.lua:116, 240) */
int fg_concat_channels(fg_ctx* ctx, const float* a, const float* b, float* out, long long npix, int ca, int cb);
int fg_split_channels(fg_ctx* ctx, const float* g, float* ga, float* gb, long long npix, int ca, int cb);
int fg_add(fg_ctx* ctx, const float* a, const float* b, float* out, long long n);
/* The n-way forms a compiled nn.ConcatTable net uses (1 <= n <= 4; `parts` / `widths`: HOST arrays of n device pointers / row widths):
 * fg_join_rows: out[r][off_k + j] = parts[k][r][j] with off_k = widths[0] + ... + widths[k-1] (nn.JoinTable(2) on [rows][width] tensors);
 * fg_split_rows: the reverse, parts[k] = NULL skips that part; fg_sum_n: out = ((parts[0] + parts[1]) + parts[2]) + parts[3], fp32
 * additions in exactly that order.  16-byte accesses when every width is a multiple of 4 and every pointer 16-byte aligned. */
int fg_join_rows(fg_ctx* ctx, const float* const* parts, const int* widths, int n, float* out, int rows);
int fg_split_rows(fg_ctx* ctx, const float* g, float* const* parts, const int* widths, int n, int rows);
int fg_sum_n(fg_ctx* ctx, const float* const* parts, int n, float* out, long long count);
int fg_sigmoid_forward(fg_ctx* ctx, const float* x, float* y, long long n);
int fg_sigmoid_backward(fg_ctx* ctx, const float* y, const float* gy, float* gx, long long n);
/* LeakyReLU.lua:13-31's own formula, y = (|x| + x) / 2 + (|x| - x) * (-negslope / 2): as in the reference, x = +inf gives NaN
 * (inf - inf; -inf as well) and x > FLT_MAX / 2 gives +inf.  backward: x >= 0 ? gy : negslope * gy (a NaN x takes the second). */
int fg_leakyrelu_forward(fg_ctx* ctx, const float* x, float negslope, float* y, long long n);
int fg_leakyrelu_backward(fg_ctx* ctx, const float* x, const float* gy, float negslope, float* gx, long long n);

#ifdef __cplusplus
}
#endif
#endif /* FACEGEN_HIP_H */
