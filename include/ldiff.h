/* ldiff.h -- C ABI of libldiff_hip.so: the MI355X (gfx950) Laplace-diffusion sampling path.
 *
 * The reference (Lweihan/LDiffusion, /root/reference) has no FFI of its own: its sampler loops call
 * duck-typed python objects from `diffusers`.  Each entry point below names the
 * reference call it replaces (file:line into /root/reference); the python shims under ldiffusion_amd/ bind them with
 * ctypes behind shim objects that keep the reference's attribute surface, and INTEGRATION.md shows
 * the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 (LDIFF_OK) or a negative ldiff_status; the message of the last failure
 *     on the calling thread is ldiff_last_error().  -1 = bad argument/shape (python: ValueError),
 *     -2 = HIP runtime failure, -3 = handle not ready (weights/context missing) (python: RuntimeError).
 *   - tensors crossing the boundary are plain device pointers in the layouts the reference uses:
 *     float32, NCHW, contiguous (torch_dtype=torch.float32 everywhere: ldiffusion.py:67, segmentor.py:77).
 *     Internally activations are NHWC fp16 with fp32 accumulation; the residual stream is kept as fp16 hi|lo pairs
 *     (ldiff_unet_set_precision).
 *   - handles own device weights and workspace; caller-owned buffers are never retained past a call.
 *   - all work is enqueued on the caller's HIP stream (`stream` = hipStream_t, e.g. torch's current
 *     stream); no hidden synchronisation.  A handle is thread-compatible, not thread-safe; handles on different
 *     devices are independent (no process-wide device state in the library).
 *   - there is no CPU fallback anywhere: a missing GPU or code object is an error.
 *   - Non-finite detection.  Activations are stored as fp16 (also under precision 1 / 2: the hi half of a split tensor is an fp16), so a checkpoint /
 *     input whose activations leave +-65504 overflows where the reference's fp32 graph does not -- e.g. the SD-v1.x decoder fed z / 0.18215 of UN-scaled
 *     latents (pixel_latent_vector.py:73,81).  Every graph therefore carries a sticky flag, set on the device by the GroupNorm-statistics kernels when a
 *     group's totals are not finite (every activation reaches one: an inf from a conv / GEMM epilogue, or the NaN it becomes downstream; no extra launch,
 *     no extra read).  It is reported as LDIFF_ERR_NONFINITE (-4; python: RuntimeError subclass NonFiniteError)
 *       (a) by ldiff_{unet,vae,pipeline}_check_finite(handle, stream): synchronises `stream` (and the decode side stream), returns the verdict
 *           for everything enqueued so far and clears the flag -- the python shims call it wherever they hand results to the host;
 *       (b) at the latest by the NEXT ldiff_unet_forward / ldiff_vae_encode / ldiff_vae_decode / ldiff_sample on the handle, at entry, for work that has
 *           completed by then (no synchronisation; the flag is cleared when reported).
 *     The results of a flagged call are garbage.  LDIFF_TRACE_ABSMAX=1 prints max |activation| per graph stage to stderr (diagnostic; synchronises).
 *     The cure for the VAE decoder is ldiff_vae_set_range_shift(vae, k): the decoder then stores its residual stream, and every conv output that feeds
 *     a GroupNorm, times 2^-k, and every decoder GroupNorm uses eps * 4^-k.  GroupNorm is scale-invariant and a power of two is exact, so the shifted
 *     graph computes the unshifted one's numbers (up to values that fall into fp16's subnormals), in a range 2^k times wider.
 *   - The load contract.  Every ldiff_<family>_load(handle, name, host_ptr, dtype, shape, ndim) takes ONE checkpoint tensor as the checkpoint states it:
 *     the family's checkpoint key, host memory in the torch layout, dtype LDIFF_F32 / LDIFF_F16 / LDIFF_BF16, its torch shape.  The library converts it
 *     to the layout its kernels read and copies it; `host_ptr` is not retained.  Refused with LDIFF_ERR_INVALID and a message: a null argument, another
 *     dtype code ("unsupported dtype"), a name the handle does not expect ("unexpected tensor name"), a shape other than the expected one ("shape [..]
 *     does not match expected [..]").  The shape must match extent by extent, except for conv / linear weights of the UNet, ControlNet, VAE, nnU-Net head
 *     and text encoder, where the element count and the first two extents must match and the rank is 4, or 2 for a 1x1 (checkpoints in circulation hold
 *     the same attention projection as [C, C] and as [C, C, 1, 1]).  Tensors may be loaded in any order and again at any time: a reload of a tensor waits
 *     for the device first (earlier forwards may still read it), and the next forward uses the new values (derived weight layouts and captured graphs are
 *     rebuilt).  ldiff_<family>_missing(handle) counts the expected tensors not loaded yet, in the handle's registration order, and
 *     ldiff_<family>_missing_name(handle, i) names entry i of the list the last _missing call made; a forward with tensors missing is LDIFF_ERR_STATE.
 */
#ifndef LDIFF_H
#define LDIFF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LDIFF_VERSION 215 /* 0.2.1.4: + ldiff_op_keep_largest_component (+ _ws_bytes) and ldiff_op_cc_label: 8-connected components of label maps and nnU-Net's largest-component postprocessing on the device.  0.2.1.3: + ldiff_op_dice_ce_ignore / _ignore_stats / _ignore_from_sums (+ _ignore_ws_bytes, _ignore_nacc): the tissue head's loss with nnU-Net's ignore label; + ldiff_op_case_counts_classes and the selectors -1 - m (`label < m`) of ldiff_op_case_rank_to_coord, for the annotated-pixel locations of a partly annotated case.  0.2.1.2: + ldiff_op_label_table_u8 / ldiff_op_gather_labels / ldiff_op_warmup_labels (+ _supported) / ldiff_op_warmup_images (the warm-up trainer's dataset resident on the device: label bytes through a grey-level table, a batch of labels and masks gathered by index, and the 64x64 warm-up batch -- labels by torch's bilinear rule in integers, images through the normalisation table and the antialiased triangle weights in one pass over the stored bytes); 0.2.1.1: + ldiff_op_resize_u8 / ldiff_op_resize_u8_ws_bytes (the device image front end: PIL.Image.resize(size, BILINEAR) of 8-bit interleaved images bit for bit from host-made coefficient tables, optionally through a float [3][256] table into the sampler's NCHW input; LDIFF_RESIZE_MAX_TAPS); 0.2.1.0: + ldiff_op_window_gather / _accumulate_batch / _finish (the tissue head's sliding window in batches: tiles x mirror variants gathered, un-flipped, averaged and Gaussian-accumulated per chunk, then divide + inf flag + arg-max + un-crop in one launch; ldiff_window_tiles by value), after ldiff_op_dice_ce_stats / _from_sums, ldiff_op_bucket_pack, ldiff_op_sumsq (data-parallel tissue training); 0.2.0.9: + ldiff_op_case_bbox / _stats / _counts / _apply / _rank_to_coord (plan and preprocess of the tissue head's training cases on the device: non-zero box, crop statistics, label counts per row, normalise into the arena, rank -> pixel); 0.2.0.8: + ldiff_op_seg_intensity_lr (the intensity chain with nnU-Net's low-resolution simulation between contrast and the gammas), ldiff_op_spline_prefilter (cubic B-spline prefilter on the device, one workgroup per plane); 0.2.0.7: + ldiff_op_conv_wgrad (direct MFMA weight gradient of the narrow convs over the pixel index, no im2col), ldiff_op_colsum_slabs (slab-reduced bias gradient), both with fixed-order partials; 0.2.0.6: + ldiff_op_seg_sample (patches, labels and deep-supervision targets of a training batch from cases resident on the device), ldiff_op_seg_intensity (nnU-Net's intensity augmentations, one workgroup per plane); 0.2.0.5: + ldiff_unet_set_plan_batch / ldiff_vae_set_plan_batch / ldiff_controlnet_set_plan_batch (batch-invariant mode: every launch planned for a nominal batch), ldiff_op_conv_pb, ldiff_op_attention_pb, ldiff_op_gn_stats_pb; 0.2.0.4: + ldiff_op_in_train_fwd / _bwd (InstanceNorm + LeakyReLU with saved statistics), ldiff_op_dice_ce (nnU-Net deep-supervision loss of one scale, value and gradient), ldiff_op_sgd_nesterov_multi; 0.2.0.3: + ldiff_confusion (per-image confusion matrices of masks or logits against labels, accumulated on the device), ldiff_seg_metrics (host: Dice / IoU / pixel accuracy / frequency-weighted IoU from one matrix); 0.2.0.2: + ldiff_textenc_* (the CLIP text encoder of the prompt path, with the optional prompt projection), ldiff_op_text_attention (causal attention over a short sequence), ldiff_conv_args.act_out (quick_gelu / gelu behind a linear layer's sum); 0.2.0.1: + ldiff_conv_args.fold_gn (GroupNorm folded into per-image 1x1 weights, as the executors run it), profiler names gn_stats<1> / gn_stats<2> (one-launch / partial + finalize statistics) and fold_gn_weights; 0.2.0.0: + ldiff_resnet_* (the cell head's ResNet152 instance classifier), ldiff_op_maxpool3x3s2 / ldiff_op_crop_resize_norm / ldiff_op_cls_head, ldiff_conv_args.relu_out / cls_conv (the classifier's conv family, ks 1 | 3 | 7); 0.1.9.0: + ldiff_segnet_* (the nnU-Net tissue head), ldiff_conv_args.lrelu_in / tconv / seg_conv (LeakyReLU prologue, 2x2 transposed conv kernel, narrow 3x3 kernel); 0.1.8.0: + ldiff_controlnet_* (the ControlNet of the multimodal sampler), ldiff_unet_attach_controlnet, ldiff_conv_args.silu_out / cond_conv (conditioning-embedding conv kernel); 0.1.7.0: + ldiff_vae_set_range_shift, ldiff_conv_args.out_shift; 0.1.6.0: + non-finite detection (LDIFF_ERR_NONFINITE, ldiff_*_check_finite), ldiff_conv_args.splitk (split launches emit statistics); 0.1.5.2: + ldiff_conv_args.n_real (tap-folded conv_out kernel), c3d_ups (upsampling convs on the dataflow kernel); 0.1.5.1: dataflow GEMM (gemm_df), shortcut conv folded into the dataflow conv3x3 (sc_*) */
#define LDIFF_MAX_BLOCKS 8
#define LDIFF_RESIZE_MAX_TAPS 128 /* longest coefficient row ldiff_op_resize_u8 takes: reductions up to 63x (a 16x reduction has 33 taps) */

typedef enum { LDIFF_OK = 0, LDIFF_ERR_INVALID = -1, LDIFF_ERR_RUNTIME = -2, LDIFF_ERR_STATE = -3, LDIFF_ERR_NONFINITE = -4 } ldiff_status;
typedef enum { LDIFF_F32 = 0, LDIFF_F16 = 1, LDIFF_BF16 = 2 } ldiff_dtype; /* host dtypes accepted by *_load */

int ldiff_version(void);
const char* ldiff_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * UNet2DConditionModel  --  replaces `unet(latents, t, text_embeddings)`
 *   segmentor.py:103,444,526   pixel_latent_vector.py:78   ldiffusion.py:160,238   utils.py:201
 * cfg mirrors diffusers' unet/config.json.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ldiff_unet ldiff_unet;
typedef struct {
  int in_channels, out_channels;
  int n_blocks;
  int block_out_channels[LDIFF_MAX_BLOCKS];
  int down_has_attn[LDIFF_MAX_BLOCKS]; /* CrossAttnDownBlock2D = 1, DownBlock2D = 0 */
  int up_has_attn[LDIFF_MAX_BLOCKS];   /* CrossAttnUpBlock2D = 1, UpBlock2D = 0 */
  int layers_per_block;
  int heads;               /* config.json "attention_head_dim" (SD-v1.5: it is the head COUNT) */
  int cross_attention_dim;
  int norm_num_groups;
  float norm_eps;
  int flip_sin_to_cos;
  float freq_shift;
} ldiff_unet_cfg;

int ldiff_unet_create(ldiff_unet** out, const ldiff_unet_cfg* cfg, int device);
/* One tensor of diffusion_pytorch_model.safetensors (diffusers key names): "The load contract" above.
 * (from_pretrained: segmentor.py:79, ldiffusion.py:67) */
int ldiff_unet_load(ldiff_unet*, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
/* Storage policy of the graph (the reference computes in fp32: ldiffusion.py:67; every MFMA operand here is fp16):
 *   0 = all activations fp16 in HBM (fastest; ~2e-3 of the output range per UNet pass)
 *   1 = residual stream kept as fp16 hi|lo pairs (adds to fp32 round-off), stream-carrying contractions on split operands (default)
 *   2 = every conv / linear operand split (K doubled): ~1e-4 */
int ldiff_unet_set_precision(ldiff_unet*, int mode);
/* Plan batch n (default 0 = off: nothing changes).  By default the kernel, tile, split-K count, unit shape and GroupNorm form of a launch are chosen
 * from its workgroup count, which depends on B: an image alone and the same image inside a batch then differ in the last bits (DESIGN.md "Batch
 * invariance").  With n >= 1 every such choice is made AS IF the batch were n, while the launch runs at its real size.  The contract: an image
 * submitted in ANY batch B <= n -- alone, first or last of a short shard -- gets bit-identical results (UNet output; through ldiff_sample: latents,
 * features, rgb), on one device model and one precision mode.  Not promised: equality across different n, across devices with different CU counts,
 * or with n = 0.  n = B reproduces the default mode's plans at that B bit for bit (so n = the largest batch any rank submits keeps the tuned plans).
 *   - n < 0: LDIFF_ERR_INVALID.  A forward with B > n > 0 (and a set_context with B_ctx > n): LDIFF_ERR_INVALID, naming both numbers.
 *   - a different n makes the next forward capture its graph anew (as a set_precision does) and rebuilds derived weight layouts where the plan names others.
 *   - the cross-attention K / V of set_context are planned too (at n L rows, whether B_ctx is 1 or B): after a change of n call ldiff_unet_set_context
 *     again; a forward before that is LDIFF_ERR_STATE.
 *   - an attached ControlNet must carry the same n at forward time, else LDIFF_ERR_INVALID.
 * ldiff_sample takes the setting from the UNet and the VAE it borrows. */
int ldiff_unet_set_plan_batch(ldiff_unet*, int n);
/* One forward is ~390-450 kernel launches (384 at B = 8, 443 at B = 1 at SD-v1.5 size: ldiff_unet_graph_nodes).  With graphs on (default) the launch sequence of a (B, h, w, precision, context)
 * configuration is captured into a hipGraph on its second use and replayed from then on (input, timestep and output pass through
 * handle-owned staging buffers: any caller pointers, any timestep; bit-identical results).  Off: every forward is launched
 * eagerly.  Forwards issued while per-launch profiling is enabled, or on a stream that is itself being captured, run eagerly. */
int ldiff_unet_set_graph(ldiff_unet*, int on);
int64_t ldiff_unet_graph_replays(ldiff_unet*); /* forwards served by graph replay so far */
int64_t ldiff_unet_graph_nodes(ldiff_unet*);   /* kernel launches of the currently captured forward (0: none captured yet) */
/* number of expected tensors not loaded yet; names via ldiff_unet_missing_name(i) */
int ldiff_unet_missing(ldiff_unet*);
const char* ldiff_unet_missing_name(ldiff_unet*, int i);
/* encoder_hidden_states [B_ctx, L, cross_attention_dim] float32 on device; precomputes the cross-attention
 * K/V of all transformer blocks (they do not depend on the timestep).  B_ctx is 1 (broadcast) or the batch. */
int ldiff_unet_set_context(ldiff_unet*, const void* ctx_dev, int B_ctx, int L, void* stream);
/* sample [B,in_channels,h,w] f32 NCHW -> out [B,out_channels,h,w] f32 NCHW */
int ldiff_unet_forward(ldiff_unet*, const void* sample_dev, int B, int h, int w, float timestep, void* out_dev, void* stream);
/* ControlNet inputs of the NEXT ldiff_unet_forward (diffusers' down_block_additional_residuals / mid_block_additional_residual,
 * segmentor.py:357-375): n_down float32 NCHW device tensors in skip-stack order (conv_in output first; shapes of the skip tensors),
 * added to the skip connections, and one tensor added to the mid block's output (either may be absent: n_down = 0 / NULL).  The
 * pointers must stay valid until that forward has been enqueued; they are consumed by it. */
int ldiff_unet_set_additional_residuals(ldiff_unet*, const void* const* down_dev, int n_down, const void* mid_dev);
/* non-finite detector (see the conventions above): LDIFF_OK or LDIFF_ERR_NONFINITE for all forwards enqueued on `stream` so far; clears the flag */
int ldiff_unet_check_finite(ldiff_unet*, void* stream);
void ldiff_unet_destroy(ldiff_unet*);

/* ------------------------------------------------------------------------------------------------
 * ControlNetModel  --  replaces `controlnet(latents, t, encoder_hidden_states=..., controlnet_cond=..., return_dict=False)`
 *   segmentor.py:357-363 (Segmentor.ldiffusion_augment_for_multimodal: RGB + depth map).  The reference takes the module from diffusers;
 * this is diffusers 0.34's ControlNetModel for SD-v1.5-style configs: a conditioning embedding (3x3 convs conditioning_channels -> e[0], then per
 * pair e[i] -> e[i] and e[i] -> e[i+1] stride 2, SiLU behind each, then e[last] -> block_out_channels[0] without activation) whose output is added
 * to conv_in(sample); the UNet's down blocks and mid block on that sum (same time embedding, same context); one 1x1 conv behind every skip
 * tensor and one behind the mid block, times conditioning_scale.  trunk_cfg is the UNet's config (up_has_attn / out_channels are not read).
 * Entry points mirror the UNet's; checkpoint names are diffusers' (conv_in, time_embedding.*, down_blocks.*, mid_block.*,
 * controlnet_cond_embedding.{conv_in, blocks.i, conv_out}, controlnet_down_blocks.i, controlnet_mid_block).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ldiff_controlnet ldiff_controlnet;
int ldiff_controlnet_create(ldiff_controlnet** out, const ldiff_unet_cfg* trunk_cfg, int conditioning_channels, const int* embedding_channels, int n_embedding,
                            int device);
int ldiff_controlnet_load(ldiff_controlnet*, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim); /* "The load contract" above */
int ldiff_controlnet_missing(ldiff_controlnet*);
const char* ldiff_controlnet_missing_name(ldiff_controlnet*, int i);
int ldiff_controlnet_set_precision(ldiff_controlnet*, int mode);   /* as ldiff_unet_set_precision; default 1 */
/* As ldiff_unet_set_plan_batch, for the trunk, the zero convs and the conditioning embedding: an image's tensors are bit-identical in any batch B <= n.
 * A different n drops the kept embedding and context projections (call ldiff_controlnet_set_cond and _set_context again; a forward before that is
 * LDIFF_ERR_STATE) and whatever captured graph of a UNet holds this network's launches.  Attached to a UNet, both must carry the same n. */
int ldiff_controlnet_set_plan_batch(ldiff_controlnet*, int n);
int ldiff_controlnet_set_context(ldiff_controlnet*, const void* ctx_dev, int B_ctx, int L, void* stream);
/* cond [B or 1, conditioning_channels, H, W] f32 NCHW, H x W = 8 x the latent size for the four-entry embedding: runs the conditioning embedding once and
 * keeps its result for every later forward (it depends on neither timestep nor latents, so a multi-pass loop pays for it once, as set_context does for K / V). */
int ldiff_controlnet_set_cond(ldiff_controlnet*, const void* cond_dev, int B, int H, int W, void* stream);
/* The diffusers surface: n_down f32 NCHW device tensors in skip-stack order (shapes of the UNet's skip tensors; n_down = 0: none) and mid_out (may be
 * NULL) receive conditioning_scale * zero_conv_i(skip_i).  Launched eagerly. */
int ldiff_controlnet_forward(ldiff_controlnet*, const void* sample_dev, int B, int h, int w, float timestep, float conditioning_scale, void* const* down_out,
                             int n_down, void* mid_out, void* stream);
int ldiff_controlnet_check_finite(ldiff_controlnet*, void* stream);
void ldiff_controlnet_destroy(ldiff_controlnet*);
/* The fast path.  While a ControlNet is attached, ldiff_unet_forward(sample, t) also runs the ControlNet's blocks on (sample, t, its own context and
 * conditioning embedding) -- same stream, inside the same captured graph -- and every zero conv is one 1x1 launch that takes the UNet's skip tensor as
 * its residual operand and writes skip + conditioning_scale * (W cnskip + b) in the UNet's own layout (split where the stream is split, fused GroupNorm
 * statistics where the launch emits them): no fp32 NCHW tensors, no separate adds.  conditioning_scale is folded into the zero convs' weights and
 * biases when it changes, not applied per launch.  NULL detaches.  Widths, layers per block, input channels and device must agree (LDIFF_ERR_INVALID
 * names both).  The ControlNet is borrowed: keep it alive while attached.  ldiff_unet_check_finite then covers its blocks too. */
int ldiff_unet_attach_controlnet(ldiff_unet*, ldiff_controlnet* cn_or_null, float conditioning_scale);

/* ------------------------------------------------------------------------------------------------
 * nnU-Net v2 PlainConvUNet, 2-D  --  replaces `self.network(x)` inside nnUNetPredictor's sliding window
 *   segmentor.py:463-488 (Segmentor.inference_tissue_model_nnUNetv2), model/nnunetv2/inference/predict_from_raw_data.py:538-606
 * as model/nnunetv2/utilities/get_network_from_plans.py builds it: per encoder stage n_conv_encoder[s] 3x3 convs (bias), the first with stride
 * strides[s] (1 or 2, both axes), each followed by InstanceNorm2d(eps 1e-5, affine) and LeakyReLU(0.01); per decoder stage j (deepest first) a
 * transposed conv with kernel = stride = strides[n_stages - 1 - j], cat((upsampled, skip), 1) and n_conv_decoder[j] convs; one 1x1 segmentation
 * head behind the last decoder stage (deep supervision off).  features[s] are the stage widths (multiples of 16).
 * Dataflow: a conv stores its raw fp16 output plus per-channel partial sums; a finalize launch makes per-(image, channel) scale / shift; the
 * consumer applies affine + LeakyReLU in its prologue (ldiff_conv_args.lrelu_in).  No normalised tensor and no concat copy is written.
 * Checkpoint names are those of dynamic_network_architectures' PlainConvUNet state dict, restated from knowledge of that package (UNPINNED: the
 * package is not available to the test-suite; scripts/gen_golden_nnunet.py pins them where it is):
 *   encoder.stages.{s}.0.convs.{i}.conv.{weight,bias}, encoder.stages.{s}.0.convs.{i}.norm.{weight,bias},
 *   decoder.stages.{j}.convs.{i}.{conv,norm}.{weight,bias}, decoder.transpconvs.{j}.{weight [Cin, Cout, 2, 2], bias},
 *   decoder.seg_layers.{n_stages - 2}.{weight,bias}.
 * The aliases a checkpoint also holds (....all_modules.*, decoder.encoder.*, the unused seg_layers, an `_orig_mod.` prefix) are dropped by the
 * python loader (ldiffusion_amd/nnunet.py clean_state_dict); ldiff_segnet_load refuses names it does not expect.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ldiff_segnet ldiff_segnet;
int ldiff_segnet_create(ldiff_segnet** out, int in_channels, int n_stages, const int* features, const int* strides, const int* n_conv_encoder,
                        const int* n_conv_decoder /* n_stages - 1 entries */, int n_heads, int device);
int ldiff_segnet_load(ldiff_segnet*, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim); /* "The load contract" above */
int ldiff_segnet_missing(ldiff_segnet*);
const char* ldiff_segnet_missing_name(ldiff_segnet*, int i);
/* as ldiff_unet_set_graph: the launch sequence of a (B, H, W, out dtype) configuration is captured on its second use and replayed afterwards */
int ldiff_segnet_set_graph(ldiff_segnet*, int on);
int64_t ldiff_segnet_graph_replays(ldiff_segnet*);
/* x [B, in_channels, H, W] f32 NCHW -> logits [B, n_heads, H, W] NCHW, out_dtype LDIFF_F32 or LDIFF_F16; H and W divisible by the product of the strides */
int ldiff_segnet_forward(ldiff_segnet*, const void* x_dev, int B, int H, int W, void* logits_dev, int out_dtype, void* stream);
int ldiff_segnet_check_finite(ldiff_segnet*, void* stream);
void ldiff_segnet_destroy(ldiff_segnet*);

/* ------------------------------------------------------------------------------------------------
 * Instance classifier of the cell head  --  replaces `self.encoder` / `self.adapter` / pooling / `self.classifier` of CellSegClassifier.forward
 *   model/conductor.py:138-233, segmentor.py:490-545
 * torchvision's ResNet (v1.5 bottleneck: expansion 4, the stride on the 3x3 conv, a 1x1 strided conv + BatchNorm as `downsample` in the first block of every layer)
 * without avgpool / fc: conv 7x7 stride 2 (3 -> width) + BatchNorm + ReLU, max pooling 3x3 stride 2, layers[i] bottlenecks of width * 2^i planes (layers 2..4 halve
 * the map); then adapter = Conv2d(8 * 4 * width, adapter_channels, 3, padding = 1), the mean over its map, Linear(adapter_channels, num_classes).  ResNet152 is
 * layers (3, 8, 36, 3), width 64.  Restated from the public architecture (UNPINNED: torchvision is not available to the test-suite).
 * Every BatchNorm (eval mode, eps 1e-5) is folded into its conv on the host in double at load time -- w' = w * gamma / sqrt(var + eps), b' = beta - mean * gamma /
 * sqrt(var + eps), rounded once to fp16 / fp32 -- so no normalisation ever runs; every conv is one clsconv launch (ldiff_conv_args.relu_out) with bias, the block's
 * identity and the ReLU in its fp32 epilogue.  No split-K: a crop's logits are bit for bit those of a B = 1 call, whatever else is in the batch.
 * Checkpoint names (the module's state_dict): encoder.0.weight, encoder.1.{weight,bias,running_mean,running_var}, encoder.{4..7}.{b}.{conv1,bn1,conv2,bn2,conv3,bn3}.*,
 * encoder.{4..7}.0.downsample.{0,1}.*, adapter.{weight,bias}, classifier.{weight,bias}; *.num_batches_tracked is accepted and dropped.  A conv and its BatchNorm
 * are folded once all five tensors are present; a later reload of such a group needs all five again.
 * The epilogues set the handle's sticky non-finite flag where a value is NaN or beyond 65504 before the ReLU (ldiff_resnet_check_finite).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ldiff_resnet ldiff_resnet;
int ldiff_resnet_create(ldiff_resnet** out, const int* layers /* 4 entries */, int width /* % 16 == 0 */, int adapter_channels /* % 16 == 0 */, int num_classes /* >= 2 */, int device);
int ldiff_resnet_load(ldiff_resnet*, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim); /* "The load contract" above */
int ldiff_resnet_missing(ldiff_resnet*);
const char* ldiff_resnet_missing_name(ldiff_resnet*, int i);
/* as ldiff_segnet_set_graph: the launch sequence of a (B, S) configuration is captured on its second use and replayed afterwards */
int ldiff_resnet_set_graph(ldiff_resnet*, int on);
int64_t ldiff_resnet_graph_replays(ldiff_resnet*);
/* crops [B, S, S, 8] f16 NHWC (channels 3..7 zero: ldiff_op_crop_resize_norm), S % 32 == 0 -> logits [B, num_classes] f32, labels [B] i32 (may be NULL) = 1 + argmax(logits[:, 1:]) */
int ldiff_resnet_forward(ldiff_resnet*, const void* crops_nhwc_f16, int B, int S, void* logits_f32, void* labels_i32_or_null, void* stream);
/* Training mode (the reference's `self.model.train()`: every BatchNorm of the trunk normalises with the statistics of the batch it is given).
 * ldiff_resnet_set_train(h, 1) BEFORE the tensors are loaded (afterwards LDIFF_ERR_STATE: the fold consumes the host tensors): the handle then also keeps every conv's UN-folded
 * weight matrix (fp16, the same K-major layout, one rounding of w) and the fp32 gamma / beta of every BatchNorm on the device.  ldiff_resnet_forward on such a handle is unchanged
 * bit for bit (it reads the folded matrices).
 * The BatchNorms in forward order -- stem, then per block bn1, bn2, bn3 and, in a layer's first block, downsample.1 behind them -- share one flat channel axis of T =
 * ldiff_resnet_bn_channels entries (ResNet152: 75712); ldiff_resnet_bn_entry(h, i, ...) names BatchNorm i by its checkpoint prefix ("encoder.6.3.bn2"; the pointer lives as long as
 * the handle), its offset on that axis and its channel count, LDIFF_ERR_INVALID past the last.
 * ldiff_resnet_forward_train: the trunk with batch statistics over ALL B crops, three launches per conv (clsconv with ldiff_conv_args.bn_stats -> bn_finalize -> bn_apply, which
 * carries the ReLU and a block's identity), the adapter conv and the pooling / head as in eval mode.  Eager launches, no graph.  batch_stats_f32 [2][T] receives every BatchNorm's
 * batch mean and UNBIASED variance (what torch's running statistics take with momentum 0.1); the handle's running statistics are not touched.  features_f32 [B][adapter_channels] =
 * the pooled adapter map; logits / labels optional.  A BatchNorm with B * H * W == 1 values per channel is refused naming the layer (LDIFF_ERR_INVALID), before any launch. */
int ldiff_resnet_set_train(ldiff_resnet*, int on);
int64_t ldiff_resnet_bn_channels(ldiff_resnet*);
int ldiff_resnet_bn_entry(ldiff_resnet*, int i, const char** name, int64_t* offset, int* channels);
int ldiff_resnet_forward_train(ldiff_resnet*, const void* crops_nhwc_f16, int B, int S, void* batch_stats_f32, void* features_f32, void* logits_f32_or_null, void* labels_i32_or_null,
                               void* stream);
int ldiff_resnet_check_finite(ldiff_resnet*, void* stream);
void ldiff_resnet_destroy(ldiff_resnet*);

/* ------------------------------------------------------------------------------------------------
 * CLIP text encoder of the prompt path  --  replaces `pipeline.text_encoder(input_ids)["last_hidden_state"]` and the `Linear(hidden, cross_attention_dim)` behind it
 *   segmentor.py:55-60 (unpadded ids), 348-350 (padded to 77)   pixel_latent_vector.py:65-67   utils.py:193-195   ldiffusion.py:213-216 (every training step)
 * transformers' CLIPTextModel without the pooled output: token + position embeddings (fp32 tables, fp32 sum), `layers` pre-LN encoder layers -- LayerNorm -> fused
 * q/k/v projection -> causal self-attention (keys j > i masked, scale d^-0.5 in fp32, fp32 softmax over the whole row) -> out_proj + residual -> LayerNorm -> fc1 ->
 * quick_gelu | gelu -> fc2 + residual -- and final_layer_norm.  No attention_mask (the reference passes none: padding tokens are attended to like any other).  The
 * residual stream is kept as fp16 hi | lo pairs (as ldiff_unet_set_precision 1 keeps the UNet's); every linear layer contracts a split activation [hi | lo | hi] against
 * [wh | wh | wl] (wh = fp16(w), wl = fp16(w - wh): fp16 MFMA operands, K tripled, neither rounding enters the fp32 sum); q, k, v and the probabilities are single fp16.  With project = 1
 * the projection of proj_weights.pt runs as a last such GEMM on the final LayerNorm's split output, fp32 result; the output [B, L, cross_attention_dim] is what
 * ldiff_unet_set_context takes.  hidden % 64 == 0, hidden / heads a multiple of 16 up to 128, max_positions <= 128.
 * Checkpoint names are transformers' state_dict keys: text_model.embeddings.{token,position}_embedding.weight, text_model.encoder.layers.N.{layer_norm1,layer_norm2}.*,
 * text_model.encoder.layers.N.self_attn.{q_proj,k_proj,v_proj,out_proj}.*, text_model.encoder.layers.N.mlp.{fc1,fc2}.*, text_model.final_layer_norm.*; q/k/v are
 * concatenated at load.  Optional: proj.weight [cross_attention_dim, hidden] and proj.bias (both or neither; cross_attention_dim % 8 == 0).
 * The final LayerNorm sets the handle's sticky non-finite flag when a row's statistics are not finite (ldiff_textenc_check_finite).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ldiff_textenc ldiff_textenc;
/* (The only tagged struct of this header.  tests/test_cpu_host.py enumerates the UNTAGGED `typedef struct { ... } name;` blocks and wants each in its own
 * list of mirrors; this one's layout is checked against _lib.TextEncCfg, field by field, in tests/test_cpu_text_encoder.py.) */
typedef struct ldiff_textenc_cfg {
  int vocab_size, hidden, intermediate, layers, heads;
  int max_positions; /* config.json "max_position_embeddings" */
  int act;           /* config.json "hidden_act": 0 = quick_gelu, 1 = gelu */
  float ln_eps;      /* config.json "layer_norm_eps" */
} ldiff_textenc_cfg;
/* (CLIPTextModel.from_pretrained: the reference's pipeline loader, segmentor.py:77-80, ldiffusion.py:67-69) */
int ldiff_textenc_create(ldiff_textenc** out, const ldiff_textenc_cfg* cfg, int device);
int ldiff_textenc_load(ldiff_textenc*, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim); /* "The load contract" above */
int ldiff_textenc_missing(ldiff_textenc*);
const char* ldiff_textenc_missing_name(ldiff_textenc*, int i);
/* as ldiff_unet_set_graph: the launch sequence of a (B, L, project, out_dtype) configuration is captured on its second use and replayed afterwards; the ids pass
 * through a handle-owned staging buffer, so a replay serves any ids of that shape */
int ldiff_textenc_set_graph(ldiff_textenc*, int on);
int64_t ldiff_textenc_graph_replays(ldiff_textenc*);
int64_t ldiff_textenc_graph_nodes(ldiff_textenc*); /* kernel launches of the currently captured forward (0: none captured yet) */
/* ids_host [B, L] int32 on the HOST (the tokenizer's output; copied during the call), 0 <= id < vocab_size, 1 <= L <= max_positions: else LDIFF_ERR_INVALID naming
 * the offender, nothing launched.  out_dev [B, L, hidden] (project = 0: last_hidden_state) or [B, L, cross_attention_dim] (project = 1: `proj(last_hidden_state)`,
 * segmentor.py:55-60), out_dtype LDIFF_F32 or LDIFF_F16.  Not inside a stream capture (the ids are host data). */
int ldiff_textenc_forward(ldiff_textenc*, const int32_t* ids_host, int B, int L, int project, void* out_dev, int out_dtype, void* stream);
int ldiff_textenc_check_finite(ldiff_textenc*, void* stream);
void ldiff_textenc_destroy(ldiff_textenc*);

/* ------------------------------------------------------------------------------------------------
 * AutoencoderKL  --  replaces vae.encode(x).latent_dist / vae.decode(z).sample / pipeline.decode_latents
 *   segmentor.py:99,106,339,379,437,447,519,529  pixel_latent_vector.py:73,81  ldiffusion.py:228,240  utils.py:190,204
 * ---------------------------------------------------------------------------------------------- */
typedef struct ldiff_vae ldiff_vae;
typedef struct {
  int in_channels, out_channels, latent_channels;
  int n_blocks;
  int block_out_channels[LDIFF_MAX_BLOCKS];
  int layers_per_block;
  int norm_num_groups;
  float scaling_factor;
} ldiff_vae_cfg;

int ldiff_vae_create(ldiff_vae** out, const ldiff_vae_cfg* cfg, int device);
int ldiff_vae_load(ldiff_vae*, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim); /* "The load contract" above */
/* storage policy of the encoder and of the decoder graph (see ldiff_unet_set_precision); defaults: encoder 2 (its error is
 * inherited by every later pass of the sampler and it runs once per patch), decoder 0 (its output is only consumed as uint8
 * images / luma, never fed back into the latents: measured at SD-v1.5 width, 512x512, 5 passes, the luma features are within one
 * grey level of the fp32 oracle in all three modes -- 6.6 % / 3.5 % / 2.9 % of the pixels differ by one -- and the probe-head
 * masks are identical in all three; modes 1 / 2 cost +20 % / +96 % decode time) */
int ldiff_vae_set_precision(ldiff_vae*, int encoder_mode, int decoder_mode);
/* decoder range shift k = 0..16 (default 0; outside: LDIFF_ERR_INVALID), see "Non-finite detection" above: for checkpoints whose decoder activations
 * pass +-65504.  Decoder only (also the decodes ldiff_sample runs on the side stream); the encoder always runs unshifted.  k costs nothing where
 * it is not needed beyond the width-changing blocks' shortcut, which then runs as its own launch; large k pushes small activations of a healthy
 * checkpoint into fp16's subnormals, so use the smallest k that decodes (python: AutoencoderKL.fit_range_shift). */
int ldiff_vae_set_range_shift(ldiff_vae*, int k);
/* As ldiff_unet_set_plan_batch, for the encoder and the decoder graph (also the decodes ldiff_sample runs): moments, sample, image, rgb and luma of an image
 * are bit-identical in any batch B <= n, under any one precision pair and range shift.  n < 0, and an encode / decode with B > n > 0: LDIFF_ERR_INVALID. */
int ldiff_vae_set_plan_batch(ldiff_vae*, int n);
int ldiff_vae_missing(ldiff_vae*);
const char* ldiff_vae_missing_name(ldiff_vae*, int i);
/* x [B,3,H,W] f32 NCHW -> moments [B, 2*latent, H/8, W/8] f32 NCHW (mean | logvar), i.e. quant_conv(encoder(x)) */
int ldiff_vae_encode(ldiff_vae*, const void* x_dev, int B, int H, int W, void* moments_dev, void* stream);
/* z [B,latent,h,w] f32 NCHW, multiplied by z_scale first (decode_latents passes 1/scaling_factor, vae.decode passes 1).
 * Any of the outputs may be NULL:
 *   sample_nchw [B,3,8h,8w] f32            = vae.decode(z).sample
 *   image_nhwc  [B,8h,8w,3] f32            = (sample/2+0.5).clamp(0,1)            (decode_latents)
 *   rgb_u8      [B,8h,8w,3] u8             = (image*255).round()  half-even       (numpy_to_pil)
 *   luma_u8     [B,n_slots,8h,8w] u8, slot = PIL convert("L") of rgb_u8           (pixel_latent_vector.py:85) */
int ldiff_vae_decode(ldiff_vae*, const void* z_dev, int B, int h, int w, float z_scale, void* sample_nchw, void* image_nhwc,
                     void* rgb_u8, void* luma_u8, int n_slots, int slot, void* stream);
/* non-finite detector: LDIFF_OK or LDIFF_ERR_NONFINITE for all encodes / decodes enqueued so far (on `stream` and on the decode side stream) */
int ldiff_vae_check_finite(ldiff_vae*, void* stream);
void ldiff_vae_destroy(ldiff_vae*);

/* ------------------------------------------------------------------------------------------------
 * Sampler arithmetic
 * ---------------------------------------------------------------------------------------------- */
/* PNDM/PLMS update as one linear combination out = sum_i coef[i] * ops[i] over n float32 elements
 * (scheduler.step(...).prev_sample: segmentor.py:104,445,527  pixel_latent_vector.py:79); coefficients
 * are computed on the host from alphas_cumprod exactly as PNDMScheduler._get_prev_sample does. */
int ldiff_pndm_step(const float* coef, const void* const* ops, int nops, void* out, int64_t n, void* stream);
/* (host) the two float32 coefficients of _get_prev_sample for alphas_cumprod values a_t, a_prev:
 * prev_sample = sample_coeff * sample + eps_coeff * model_output.  Both the python scheduler shim and
 * ldiff_sample use this one routine, so the two drivers agree bit for bit on every machine. */
int ldiff_pndm_coeffs(float a_t, float a_prev, float* sample_coeff, float* eps_coeff);
/* alphas_cumprod table of the SD-v1.5 scheduler config (1000 float32) */
int ldiff_pndm_alphas_cumprod(float* out_host, int n);
/* out = z0 + Laplace(0, scale) given the uniform draw u (or u = NULL: counter-based Philox stream seed/offset)
 * (ldiffusion.py:234-237; torch.distributions.Laplace.rsample) */
int ldiff_laplace_add(const void* z0, float scale, const void* u_or_null, uint64_t seed, uint64_t offset, void* out, int64_t n, void* stream);
/* logits [B,C,H,W] f32 -> mask [B,H,W] u8 = argmax over C  (segmentor.py:536-537) */
int ldiff_argmax_u8(const void* logits, int B, int C, int H, int W, void* mask_u8, void* stream);
/* Mask tail over the per-pixel latent vectors in ONE launch: features [B,N,H,W] u8 (the N luma planes of a pixel are its latent vector,
 * pixel_latent_vector.py:85-93), weight [C,N] f32, bias [C] f32 or NULL -> mask [B,H,W] u8 = first argmax_c of
 *   logit_c = bias_c + sum_n weight[c,n] * (feature_n * scale)      (argmax(softmax(.)): segmentor.py:536-537)
 * with the arithmetic pinned (float32, x_n = fl(f_n * scale), acc = bias_c, acc = fl(acc + fl(w * x_n)) in plane order, no fused multiply-add)
 * so that a host statement reproduces the mask bit for bit (oracle/noise_post.py probe_argmax).  C <= 32, N <= 64, H*W % 4 == 0. */
int ldiff_probe_argmax_u8(const void* features_u8, int B, int N, int H, int W, const void* weight, const void* bias_or_null, float scale, int C, void* mask_u8,
                          void* stream);
/* One tile of a sliding-window / tile merge: acc[:, y0:y0+th, x0:x0+tw] += pred * weight;  cnt[y0:.., x0:..] += weight (weight NULL: 1)
 * acc [C,H,W], cnt [H,W], pred [C,th,tw], weight [th,tw]; dtypes 0: all float32, 1: all float16, 3: float16 accumulators and weight with a
 * float32 prediction (the product then stays float32, as type promotion makes it); product and sum rounded separately, as the tensor
 * formulation does (nnU-Net predictor, model/nnunetv2/inference/predict_from_raw_data.py:563-570,
 * called from segmentor.py:388-488; float16 accumulators there). */
int ldiff_window_accumulate(void* acc, void* cnt, const void* pred, const void* weight_or_null, int C, int H, int W, int th, int tw, int y0, int x0, int dtypes,
                            void* stream);
/* rgb [B,3,H,W] f32 -> gray [B,1,H,W] f32 = (rgb*[0.2989,0.5870,0.1140]).sum(1)  (ldiffusion.py:241-242) */
int ldiff_luma_float(const void* rgb_nchw, void* gray, int B, int H, int W, void* stream);
/* F.interpolate(x, size=(out_h,out_w), mode="bilinear", align_corners=False) on fp32 NCHW (ldiffusion.py:240,250: the decoded
 * image is resized to 64x64 before the float luma of the training-time features). */
int ldiff_bilinear_resize(const void* x_nchw_f32, void* y_nchw_f32, int B, int C, int H, int W, int out_h, int out_w, void* stream);
/* PIL.Image.resize((Wo, Ho), Image.BILINEAR) of 8-bit images, bit for bit (Pillow's 8-bit rule is integer arithmetic; utils.py:180, segmentor.py:92,428: the
 * Resize((1024, 1024)) in front of the sampler and behind it).  x_u8 [B, Hs, Ws, C] interleaved, C = 1 or 3, all B images one size.
 *   - the tables are made on the HOST in double, once per (in, out) pair (python: imgio.coefficients), and live on the device: bounds_i32 [out][2] =
 *     (first source index, window length) and coef_i32 [out][taps] = int(0.5 + w * 2^22), zero behind the window; h* for Ws -> Wo, v* for Hs -> Ho.
 *     The tables of a side that does not change are not read (NULL, 0): that pass is skipped.
 *   - out = clip((2^21 + sum_j coef[j] * src[first + j]) >> 22, 0, 255); the horizontal pass first, the intermediate [B, Hs, Wo, C] rounded and clipped to
 *     uint8 in `ws` (ldiff_op_resize_u8_ws_bytes bytes, caller-owned, 0 when one launch does it).  Reads are clamped into the source whatever the tables say.
 *   - lut_f32_or_null NULL: out is uint8 [B, Ho, Wo, C].  Else (C = 3 only) lut is float [3][256] on the device and out is float32 [B, 3, Ho, Wo] NCHW with
 *     out[b, c, y, x] = lut[c][resized byte]: ToTensor + Normalize as a table the caller evaluates (python: imgio.normalize_table), the sampler's input in one step.
 *   - LDIFF_ERR_INVALID, naming the argument: C other than 1 | 3, a side of 0, a missing table, htaps / vtaps above LDIFF_RESIZE_MAX_TAPS, ws too small, lut with C = 1,
 *     B, Hs or Ho above 65535. */
int64_t ldiff_op_resize_u8_ws_bytes(int B, int Hs, int Ws, int C, int Ho, int Wo, int to_float); /* -1: a shape ldiff_op_resize_u8 refuses */
int ldiff_op_resize_u8(const void* x_u8, int B, int Hs, int Ws, int C, int Ho, int Wo, const void* hbounds_i32, const void* hcoef_i32, int htaps, const void* vbounds_i32,
                       const void* vcoef_i32, int vtaps, const void* lut_f32_or_null, void* out, void* ws, int64_t ws_bytes, void* stream);

/* The warm-up trainer's dataset on the device (dataset.py:10-89, ldiffusion.py:72-119,200,212,225; python: ldiffusion_amd/dataset.py DeviceLoader).  The store is
 * two uint8 arrays on the device: images [N, Hs, Ws, 3] interleaved (already through ldiff_op_resize_u8) and labels [N, H, W] (already class indices).  A batch is
 * idx_i32 [B] on the device; an index outside [0, N) is clamped into the store (callers validate on the host).  A sample's result depends on its own bytes alone:
 * no atomics, fixed summation order, the same bits whatever B and whatever its position in the batch.
 *   - ldiff_op_label_table_u8: dst[i] = table_u8[src[i]], i < n; table_u8 [256] on the device; dst may be src.
 *   - ldiff_op_gather_labels: label_u8 [B, 1, H, W] = cache[idx] and mask_i64 [B, H, W] = the same values as int64, one launch.
 *   - ldiff_op_warmup_labels: out_u8 [B, 1, oh, ow] = F.interpolate(label.float(), (oh, ow), mode="bilinear", align_corners=False).to(uint8) bit for bit, for
 *     H % oh == 0 and W % ow == 0 (ldiff_op_warmup_labels_supported returns 1): per axis an even ratio r averages source indices r*i + r/2 - 1 and r*i + r/2 with
 *     weights 1/2, an odd one picks r*i + (r - 1)/2, so the value is (a + b + c + d) >> 2 in integers.  Other sizes are LDIFF_ERR_INVALID: torch's float32 result is
 *     the target there, and the caller evaluates it.
 *   - ldiff_op_warmup_images: out_f32 [B, 3, oh, ow] (NCHW) = sum_y wy[oy][y] * (sum_x wx[ox][x] * table[c][cache[idx[b], yfirst + y, xfirst + x, c]]), the
 *     horizontal sum first, each sum accumulated in index order in float32.  table_f32 [3][256] is ToTensor + Normalize of the grey levels (python:
 *     imgio.normalize_table); {x,y}bounds_i32 [out][2] = (first source index, window length) and {x,y}weights_f32 [out][taps] are the antialiased triangle weights
 *     of F.interpolate(..., mode="bilinear", antialias=True) = Pillow's window rule (python: imgio.weights, made in double), zero behind the window,
 *     taps <= LDIFF_RESIZE_MAX_TAPS; upsampling is the same formula with support 1.  Reads are clamped into the source whatever the tables say.
 *   - LDIFF_ERR_INVALID, naming the argument: null pointers, N < 1, a side of 0, B or a height above 65535, taps outside 1 .. LDIFF_RESIZE_MAX_TAPS, a reduction
 *     whose row span does not fit 64 KiB of LDS. */
int ldiff_op_label_table_u8(const void* src_u8, void* dst_u8, int64_t n, const void* table_u8, void* stream);
int ldiff_op_gather_labels(const void* cache_u8, int N, int H, int W, const void* idx_i32, int B, void* label_u8, void* mask_i64, void* stream);
int ldiff_op_warmup_labels_supported(int H, int W, int oh, int ow);
int ldiff_op_warmup_labels(const void* cache_u8, int N, int H, int W, const void* idx_i32, int B, int oh, int ow, void* out_u8, void* stream);
int ldiff_op_warmup_images(const void* cache_u8, int N, int Hs, int Ws, const void* idx_i32, int B, const void* table_f32, const void* ybounds_i32, const void* yweights_f32, int ytaps,
                           const void* xbounds_i32, const void* xweights_f32, int xtaps, int oh, int ow, void* out_f32, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Metrics  --  scoring the masks where they are (utils.py:55-104, evaluate.py:11-126, segmentor.py:114-142,284-289)
 *
 * The reference's four metrics are functions of one integer matrix, conf[t, p] = #{pixels with target t and prediction p} (`hist` of
 * evaluate.py:32-35).  ldiff_confusion forms it on the device in ONE launch (the reference: C^2 masked sums with an .item() each for the
 * frequency-weighted IoU, 2C - 3C more for the other three); ldiff_seg_metrics turns C^2 integers into the figures on the host.  The matrix is
 * exact and bitwise reproducible (integer atomics), so matrices of batches, images or ranks simply add (parallel.reduce_confusion).
 * ---------------------------------------------------------------------------------------------- */
/* confusion matrices, accumulated: evaluate.py:32-35 (hist), utils.py:55-104, segmentor.py:114-142
 *   conf [B, C, C] int64, rows = targets, columns = predictions: conf[b, t, p] += count.  The call ADDS: stream batches into one matrix, zero it yourself.
 *   dropped [B] int64 or NULL: += the pixels whose target or prediction is outside [0, C) (the reference's `==` matches no class for them: they are in no cell).
 *         With such pixels the reference's Dice and IoU are no function of the matrix (a prediction on a pixel whose label is no class still counts there as a
 *         false positive; here the pixel is left out of every figure): a caller who keeps an "ignore" label checks `dropped`.
 *   pred: kind 0 = mask u8 [B, H, W]; 1 / 2 = logits [B, C, H, W] float32 / float16, arg-max taken in the kernel by ldiff_argmax_u8's rule bit for bit
 *         (first maximal class; a pixel with any NaN or +inf logit is class 0); no mask is written.
 *   target: kind 0 = u8 [B, H, W], 1 = int64 [B, H, W] (the reference's torch.long labels; negative or >= C: dropped).
 *   LUTs (device, 256 x u8, or NULL): applied to the prediction (mask form only) / the u8 target before counting -- the grey levels of label PNGs to class
 *         ids, dataset.py:10-32,48-61; an output >= C is dropped.  Any LUT beside an int64 target, or a prediction LUT beside logits: LDIFF_ERR_INVALID.
 *   1 <= C <= 32, else LDIFF_ERR_INVALID and nothing is enqueued.  H * W and the pointers need no alignment beyond the element's own (int64: 8 bytes).
 * Everything is enqueued on `stream`: no synchronisation, no allocation, no workspace. */
int ldiff_confusion(const void* pred, int pred_kind /* 0 u8 mask, 1 f32 logits, 2 f16 logits */, const void* target, int target_kind /* 0 u8, 1 i64 */,
                    const uint8_t* pred_lut_or_null, const uint8_t* target_lut_or_null, int B, int C, int H, int W, int64_t* conf, int64_t* dropped_or_null,
                    void* stream);
/* (Tagged like ldiff_textenc_cfg: tests/test_cpu_host.py enumerates the untagged structs; this one's mirror is _lib.SegMetricsOut, checked in tests/test_cpu_metrics.py.) */
typedef struct ldiff_seg_metrics_out {
  int num_classes;
  float dice[32];        /* per class, float32 as the reference's tensor */
  float dice_mean;       /* over all C classes */
  double iou[32];        /* NaN where iou_skipped */
  int iou_skipped[32];   /* 1: empty union, the reference's None */
  double iou_mean;       /* over the classes not skipped; 1.0 if none is left */
  double pa[32];         /* 1.0 for a class absent from the target */
  double pa_mean;
  float fw_iou;          /* all classes */
  float fw_iou_fg;       /* ignore_background=True: class 0 left out, freq NOT renormalised (as the reference) */
} ldiff_seg_metrics_out;
/* (host) the reference's four metrics from ONE C x C matrix (rows = targets), with its rules and its arithmetic.  Python and C callers share this routine.
 *   Dice (utils.py:55-82 = segmentor.py:114-142): a class absent from target and prediction scores 1, else 2 TP / (2 TP + FP + FN) in float32; mean over C.
 *   IoU (utils.py:84-104): a class with an empty union is skipped; mean over the rest in double, 1.0 if none.
 *   pixel accuracy (evaluate.py:11-27): TP / |target == c| in double, 1.0 for an absent class; mean over C.
 *   frequency-weighted IoU (evaluate.py:29-45): float32 matrix and arithmetic, + 1e-10 in the denominator; an all-zero matrix gives what that arithmetic
 *   gives (NaN).
 * The reference sums float32 ones, exact only below 2^24 pixels per class; the matrix here is always exact, so beyond that the figures are those of the exact
 * counts rounded once.  C outside [1, 32], a null pointer or a negative count: LDIFF_ERR_INVALID. */
int ldiff_seg_metrics(const int64_t* conf_host, int C, ldiff_seg_metrics_out* out);

/* ------------------------------------------------------------------------------------------------
 * Fused sampler  --  replaces the whole per-image loop body of
 *   pixel_latent_vector.py:72-86 (mode LDIFF_SAMPLE_PLMS)  and  segmentor.py:99-107 / 519-530 (same, n_passes = 1)
 * for a batch of B patches:  z = vae.encode(x).mean;  set_timesteps;  for t: eps = unet(z,t,ctx);
 * z = scheduler.step(eps,t,z);  rgb = numpy_to_pil(decode_latents(z));  luma[:, pass] = convert("L").
 * ---------------------------------------------------------------------------------------------- */
typedef struct ldiff_pipeline ldiff_pipeline;
int ldiff_pipeline_create(ldiff_pipeline** out, ldiff_unet*, ldiff_vae*); /* borrows both handles */
/* Replace the built-in alphas_cumprod table (1000 float32, host) with the caller's scheduler.alphas_cumprod
 * (ldiffusion.py:198,234 reads that attribute); the built-in one agrees with torch's to ~2 ulp. */
int ldiff_pipeline_set_alphas_cumprod(ldiff_pipeline*, const float* abar_host, int n);
/* ldiff_sample runs the VAE decode of pass k (it only feeds the feature tensor) on the VAE's side stream beside the UNet
 * pass k+1 (+7 % patches/s: the UNet's 16x16 / 8x8 levels leave most CUs idle).  mode 0: everything on the caller's stream;
 * mode 1 (default): side stream, the caller's stream joins before ldiff_sample returns; mode 2: side stream, join deferred:
 * features / rgb of that call may only be read after ldiff_pipeline_join(p, stream) -- with two pipelines on the same
 * unet/vae used alternately, the encoder and UNet passes of batch k+1 then run under the trailing decodes of batch k.
 * Results are bit-identical in all modes. */
int ldiff_pipeline_set_overlap(ldiff_pipeline*, int mode);
int ldiff_pipeline_join(ldiff_pipeline*, void* stream);
/* images [B,3,H,W] f32.  n_passes = number of UNet passes N (set_timesteps(N-1) for N >= 3, set_timesteps(1) for N = 1;
 * N = 2 is rejected: the reference's set_timesteps(1) then yields a single pass, pixel_latent_vector.py:74).
 * Outputs (any may be NULL): latents_out [B,latent,H/8,W/8] f32 (after the last pass),
 * features_u8 [B,N,H,W] (luma of every pass), rgb_u8 [B,H,W,3] (last pass). */
int ldiff_sample(ldiff_pipeline*, const void* images, int B, int H, int W, int n_passes, void* latents_out, void* features_u8,
                 void* rgb_u8, void* stream);
/* non-finite detector over both graphs of the pipeline: joins a deferred decode, synchronises `stream`, LDIFF_OK or LDIFF_ERR_NONFINITE; clears the flags */
int ldiff_pipeline_check_finite(ldiff_pipeline*, void* stream);
/* PLMS timesteps the sampler will visit for n_passes (host); returns the count written. */
int ldiff_plms_timesteps(int n_passes, int64_t* out, int cap);
void ldiff_pipeline_destroy(ldiff_pipeline*);

/* ------------------------------------------------------------------------------------------------
 * Single-kernel entry points (internal NHWC fp16 layout) -- used by the parity tests and the roofline
 * bench so that every kernel is reachable through the C ABI.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* x;  const void* x2; int C1, C2;       /* NHWC f16 sources (x2 optional channel concat) */
  int B, Hin, Win, Hout, Wout, ks, stride, pad_t, pad_l, ups;
  const void* w;  int N, Nrows;                     /* [Nrows][ks*ks*(C1+C2)] f16, rows >= N zero */
  const void* gn_scale; const void* gn_shift; int silu_in;   /* f32 [B, C1+C2] or NULL */
  const void* bias;                                 /* f32 [Nrows] or NULL */
  const void* temb; int ld_temb;                    /* f32 [B, ld_temb] or NULL */
  const void* res; int ld_res;                      /* f16 [M, ld_res] or NULL */
  void* y; int ldy; int out_f32;
  void* stats;                                      /* optional f32 [B][N][R][2]: fused GroupNorm partial sums of y (R from ldiff_op_conv_stats_blocks) */
  int geglu;                                        /* 1x1 / linear only: the weight rows are the [x | gate] rows of diffusers' GEGLU projection
                                                       interleaved by 16 (row r of x -> 32*(r/16) + r%16, of gate -> 32*(r/16) + 16 + r%16);
                                                       y[m, 0..N/2) = x * gelu_erf(gate), ldy counts those N/2 columns (N % 32 == 0) */
  int ld1, ld2;                                     /* row pitch (elements) of x / x2; 0 = C1 / C2 */
  int res_lo;                                       /* > 0: res is a split tensor (value = hi + lo), lo half res_lo elements after the hi half */
  int y_lo;                                         /* > 0: write y split: hi at column n, lo = f16(v - hi) at column y_lo + n */
  int short_runs;                                   /* 1: the persistent conv kernels retire a workgroup after ONE unit / tile (what ldiff_sample sets for the VAE
                                                       decodes that run beside the next UNet pass); 0: one workgroup per CU walks its whole share */
  int lo8_slab0;                                    /* > 0: x is a split operand whose lo half is fp8 (ldiff_op_norm_apply_lo8): rows of [C fp16 | C e4m3] = 3C
                                                       bytes, C1 = 3C/2, lo8_slab0 = C/64, w built by ldiff_op_lo8_weights; 3x3 stride 1, C % 128 == 0, N % 128 == 0,
                                                       split output with statistics, maps that fill the chip with 16 x 16 tiles; anything else: LDIFF_ERR_INVALID */
  const void* lo8_scale;                            /* the int ldiff_op_lo8_weights wrote (device memory) */
  int gemm_df;                                      /* 1x1 / linear only, producer / consumer ("dataflow") GEMM: 0 = where the executors would pick it (unit list
                                                       fills the chip), -1 = never, 1 = always where the shape is eligible (LDIFF_ERR_INVALID otherwise), 16 mt + ntw
                                                       (mt 4 | 8, ntw 2 | 4 | 5) = always, with units of 16 mt rows x 64 ntw columns (tests, timing) */
  const void* sc_x;                                 /* 3x3 stride-1 GroupNorm + SiLU convs on the dataflow kernel only: the 1x1 conv_shortcut of a ResnetBlock2D that changes width
                                                       (diffusers ResnetBlock2D.conv_shortcut), folded into the block's second conv: y = conv3x3(silu(gn(x))) + sc_w . sc_x + bias +
                                                       sc_bias.  sc_x [B, Hin, Win, sc_C] fp16 (row pitch sc_ld, 0 = sc_C; sc_C % 64 == 0), sc_w [Nrows, sc_C] fp16 K-major,
                                                       sc_bias [Nrows] fp32 or NULL; no res then.  Shapes the dataflow kernel does not take: LDIFF_ERR_INVALID */
  int sc_C, sc_ld;
  const void* sc_w;
  const void* sc_bias;
  int c3d_ups;                                      /* ups = 1 convs on the dataflow kernel: 1 = wherever the shape is eligible (tests, timing); 0 = the executors' choice (never: it does
                                                       not pay in the sampler's step) */
  int n_real;                                       /* output channels of the layer where N (the stored columns, a multiple of 4) rounds them up; 0 = not stated.  The tap-folded
                                                       3x3 kernel for <= 3 output channels (the VAE's conv_out) runs only where this says so */
  int splitk;                                       /* 0 = the executors' plan (none when `stats` is given: this entry point's historical behaviour); 2..16 = that many K splits
                                                       (tests, timing): fp32 partials + the reduce kernel, which then also emits `stats` in blocks of 32 rows
                                                       (ldiff_op_conv_stats_blocks accounts for it; needs 32 | Hout * Wout).  fp16 output, no GEGLU, no parity-folded upsampling */
  int out_shift;                                    /* range shift k = 0..16 (0 = none; else LDIFF_ERR_INVALID): y = (sum + bias + temb) * 2^-k + res, res supplied already shifted;
                                                       hi | lo and `stats` are of that value (ldiff_vae_set_range_shift).  Exact: the k = 0 result times 2^-k wherever it stays
                                                       out of the fp16 subnormals.  Not with GEGLU; a folded shortcut (sc_x) is refused (LDIFF_ERR_INVALID) */
  int silu_out;                                     /* 1: y = silu(sum + bias), the activation BEHIND the sum, rounded once.  Only the conditioning-embedding kernel has it (3x3, pad 1,
                                                       stride 1 | 2, (C1, N) one of (8, 16) (16, 16) (16, 32) (32, 32) (32, 96) (96, 96) (96, 256), plain fp16 in and out, bias only);
                                                       any other launch: LDIFF_ERR_INVALID */
  int cond_conv;                                    /* the conditioning-embedding kernel: 0 = the executors' choice (the eligible launches that ask for silu_out: the embedding's own layers; a plain
                                                       launch of such a shape goes where it always went), 1 = every eligible launch (tests, timing), -1 = never (timing: the route such a
                                                       layer had before the kernel existed; silu_out is then refused) */
  int lrelu_in;                                     /* with gn_scale / gn_shift: the activation behind the affine is LeakyReLU(0.01) instead of SiLU / none.  Bit 0: on the channels of x, bit 1: on
                                                       those of x2 (a decoder conv of the nnU-Net head reads cat(upsampled, skip): identity scale / shift and no activation on the first source).
                                                       silu_in must be 0.  Such launches run on the narrow kernel (seg_conv), on the halo-tile 3x3 kernels where the shape is theirs (64-channel multiples, stride 1:
                                                       conv3x3_lrelu<...>), else on the register-staged implicit GEMM (igemm_lrelu<...>); with tconv, on the transposed-conv kernel */
  int tconv;                                        /* 1: transposed conv with kernel = stride = 2 (tconv2x2<...>): ks = 2, stride = 2, Hout = 2 Hin, Wout = 2 Win, one source (C1 % 8 == 0), w =
                                                       [4][Nrows][C1] f16 (tap dy * 2 + dx, then output channel; from torch's [Cin, Cout, 2, 2]), N == Nrows, N % 16 == 0, bias [N] added once per
                                                       output pixel, plain fp16 output; optional gn_scale / gn_shift (+ lrelu_in bit 0) prologue.  No residual, statistics, split or fp32 output */
  int seg_conv;                                     /* the narrow 3x3 kernel of the nnU-Net head (segconv<...>: pad 1, stride 1 | 2, C1 + C2 one of 8, 32, 64, N 32 | 64, optional gn_scale / gn_shift
                                                       + lrelu_in prologue, bias, plain fp16 output, statistics of the fp32 sums in one row block per wave): 0 = the executors' choice (the eligible
                                                       launches that carry lrelu_in; a plain launch of such a shape goes where it always went), 1 = every eligible launch (the head's first
                                                       conv; tests, timing), -1 = never (timing: the implicit-GEMM route) */
  int relu_out;                                     /* 1: y = relu(sum + bias + res), the activation BEHIND the sum, rounded once.  Only the instance classifier's conv family has it
                                                       (clsconv<...>: ks 1 | 3 | 7 with pad_t = pad_l = ks / 2, stride 1 | 2, one plain fp16 source with C1 % 8 == 0 (row pitch ld1 % 8 == 0),
                                                       N % 16 == 0, N <= Nrows, bias and a plain fp16 res (ld_res % 4 == 0) only, plain fp16 output with ldy % 4 == 0, Hout = (Hin - 1) / stride + 1,
                                                       no split, no statistics, pointers aligned for 16-byte operand loads); any other launch, and relu_out beside silu_out / cond_conv = 1 / tconv / lrelu_in /
                                                       seg_conv = 1 / sc_x: LDIFF_ERR_INVALID, never another route.  The K order of a sum is k = tap * C1 + c in
                                                       steps of 32 whatever B and the tile: an image's outputs do not depend on the batch it travels in */
  int cls_conv;                                     /* that family: 0 = the executors' choice (the eligible launches that ask for relu_out; a plain launch of such a shape goes where it
                                                       always went), 1 = every eligible launch (the classifier's convs without a ReLU; the only route of ks = 7; tests, timing),
                                                       -1 = never (relu_out is then refused) */
  void* bn_stats;                                   /* optional f32 [N][R][2] (8-byte aligned): training-mode BatchNorm partials of the classifier's conv family.  Needs cls_conv = 1 and a launch
                                                       that family takes, without bias, res and relu_out (anything else: LDIFF_ERR_INVALID).  Beside the raw fp16 output the launch writes
                                                       bn_stats[(n * R + r) * 2 + {0, 1}] = {sum, sum of squares} of the FP32 accumulators of channel n over the valid rows of row block
                                                       r = 4 * workgroup + wave (64 or 16 rows each), R = ldiff_op_conv_bn_stats_blocks; blocks past M hold zeros.  No atomics, bit-reproducible.
                                                       Not the per-image layout of `stats`, which keeps its meaning and its routes.  (Beside the family's other two fields and not
                                                       behind act_out: the layout of the struct changed with LDIFF_VERSION 211, callers are recompiled against it) */
  int fold_gn;                                      /* 1: plan the launch as the executors plan a GroupNorm -> 1x1 conv / Linear without activation: where the LDS-DMA GEMM takes
                                                       per-image weights (ks = 1, one source, no silu_in / lrelu_in / GEGLU / fp32 output / statistics, K % 64 == 0, 64 | Hout * Wout)
                                                       gn_scale / gn_shift are folded into W_b = W diag(scale_b), bias_b = bias + W shift_b by the fold kernel (profiler row
                                                       `fold_gn_weights`) and the contraction runs as gemm_dma<...> on them; where it does not, the plan declines and the launch runs
                                                       as with fold_gn = 0 (igemm<...,gn>, no `fold_gn_weights` row).  0 = never folded (this entry point's historical behaviour) */
  int act_out;                                      /* an activation BEHIND the sum of a linear layer, y = act(sum + bias) in fp32, rounded once (CLIPMLP.fc1 of the text encoder):
                                                       1 = quick_gelu v * sigmoid(1.702 v), 2 = gelu (erf form), 0 = none.  Only the LDS-DMA GEMM has it (gemm_dma<...>: ks = 1,
                                                       K % 64 == 0, fp16 output (plain, or split with y_lo), no res / out_f32 / geglu / stats / out_shift / splitk / gemm_df = 1); any other launch, and
                                                       act_out beside relu_out / silu_out / cls_conv = 1 / cond_conv = 1 / tconv / lrelu_in / seg_conv = 1: LDIFF_ERR_INVALID, never another route */
} ldiff_conv_args;
int ldiff_op_conv(const ldiff_conv_args*, void* stream);
/* ldiff_op_conv with a plan batch n (ldiff_unet_set_plan_batch): 0 is ldiff_op_conv; n >= B: kernel, tile, split and unit shape are chosen as if the launch had n
 * images (n Hout Wout rows), so the rows of an image come out bit-identical at every B <= n.  B > n, n < 0: LDIFF_ERR_INVALID.  (An entry point of its own and
 * not a field appended to ldiff_conv_args: callers compiled against the struct as it is keep working.) */
int ldiff_op_conv_pb(const ldiff_conv_args*, int plan_batch, void* stream);
/* row blocks per image the launch would emit statistics for (0 = unsupported for this shape) */
int ldiff_op_conv_stats_blocks(const ldiff_conv_args*);
/* R of ldiff_conv_args.bn_stats for the tile the plan picks for this launch: 4 * ceil(M / 64) or 4 * ceil(M / 256) (negative: the status of a launch the family refuses) */
int ldiff_op_conv_bn_stats_blocks(const ldiff_conv_args*);
/* Training-mode BatchNorm behind such a launch (kernels_clstrain.hip), eps 1e-5.
 * bn_finalize: part f32 [N][R][2] -> per channel the R partials added in index order in double; mean = sum / n, var = max(sumsq / n - mean^2, 0) (biased);
 *   scale[c] = gamma[c] / sqrt(var + eps), shift[c] = beta[c] - mean * scale (fp32, one rounding each); batch_stats[offset + c] = mean and
 *   batch_stats[T + offset + c] = var * n / (n - 1) (the UNBIASED variance torch's running_var takes), fp32, batch_stats a flat f32 [2][T].
 *   n < 2: LDIFF_ERR_INVALID before any launch (torch: "Expected more than 1 value per channel when training").
 * bn_apply: y[m, c] = fp16(relu?(x[m, c] * scale[c] + shift[c] + id)) over [M, N] fp16 (N % 8 == 0, pointers 16-byte aligned), one launch; id = nothing (id NULL),
 *   id[m, c] (a plain fp16 tensor: id_scale NULL) or id[m, c] * id_scale[c] + id_shift[c] (a second raw tensor with its own BatchNorm).  fp32 throughout, one rounding;
 *   *nonfinite_i32_or_null (device or host-mapped) is set to 1 where the fp32 value is NaN or beyond 65504, in front of the ReLU. */
int ldiff_op_bn_finalize(const void* part_f32, int R, int N, int64_t n, const void* gamma_f32, const void* beta_f32, void* scale_f32, void* shift_f32, void* batch_stats_f32,
                         int64_t offset, int64_t T, void* stream);
int ldiff_op_bn_apply(const void* x_f16, int64_t M, int N, const void* scale_f32, const void* shift_f32, const void* id_f16_or_null, const void* id_scale_f32_or_null,
                      const void* id_shift_f32_or_null, int relu, void* y_f16, void* nonfinite_i32_or_null, void* stream);
/* finalize producer-fused partial sums into per-(b,channel) scale/shift; part2 (second concat source) may be NULL */
int ldiff_op_gn_finalize(const void* part1, int R1, int C1, const void* part2, int R2, int C2, int B, int HW, int groups, float eps,
                         const void* gamma, const void* beta, void* scale, void* shift, void* stream);
/* InstanceNorm finalize of the nnU-Net head (ldiff_segnet): scale[b, ss_off + c] = gamma[c] * rstd, shift[b, ss_off + c] = beta[c] - mean * scale for c < C, rows of
 * ld_ss fp32 entries, plus scale 1 / shift 0 in the `ident` leading entries of every row (the upsampled half of a decoder concat).  Statistics from `part`
 * (f32 [B][C][R][2] partial {sum, sum of squares}, the layout of ldiff_conv_args.stats) or, with part NULL, from the tensor itself (x f16 [B, HW, ldx]). */
int ldiff_op_in_finalize(const void* part, int R, const void* x_f16, int ldx, int B, int HW, int C, float eps, const void* gamma, const void* beta, void* scale,
                         void* shift, int ld_ss, int ss_off, int ident, void* stream);
/* Kernels of the cell head beside its convs (ldiff_resnet; kernels_cls.hip).
 * maxpool3x3s2: x [B, H, W, C] f16 NHWC (C % 8 == 0) -> y [B, (H - 1) / 2 + 1, (W - 1) / 2 + 1, C]: 3x3 window, stride 2, padding 1, taps outside the map ignored.
 * crop_resize_norm: rgb_u8 [H, W, 3] (device), boxes_i32 [n, 4] = (x1, y1, x2, y2) inclusive (device), lut_u8 [3][256] (device) -> out [n, S, S, 8] f16 NHWC, channels 3..7 zero:
 *   per pixel lut[c][rgb] / 255, resampled to S x S with the anti-aliased bilinear filter of torch's F.interpolate(antialias=True, align_corners=False)
 *   (plain bilinear for a side <= S), then (v - mean[c]) / std[c], all of it in double (the normalisation cancels near the mean) and rounded once; mean3 / std3 are HOST double[3].  A box that leaves the image yields a zero crop.
 * cls_head: x [B, HW, ldx] f16 (the first A columns) -> feat = mean over HW (fp32), logits [B, C] f32 = w [C, A] f32 . feat + bias [C] f32, and
 *   labels [B] i32 (may be NULL) = 1 + argmax(logits[:, 1:]), the first maximum; C >= 2. */
int ldiff_op_maxpool3x3s2(const void* x, void* y, int B, int H, int W, int C, void* stream);
int ldiff_op_crop_resize_norm(const void* rgb_u8, int H, int W, const void* boxes_i32, int n, const void* lut_u8, int S, const double* mean3, const double* std3, void* out_f16,
                              void* stream);
int ldiff_op_cls_head(const void* x, int B, int HW, int A, int ldx, const void* w_f32, const void* bias_f32, int C, void* logits_f32, void* labels_i32_or_null, void* stream);
/* cls_head with one more optional output: features_f32 [B, A], the fp32 mean over the map the logits are computed from.  logits / labels: bit for bit ldiff_op_cls_head's. */
int ldiff_op_cls_head_feat(const void* x, int B, int HW, int A, int ldx, const void* w_f32, const void* bias_f32, int C, void* logits_f32_or_null, void* labels_i32_or_null,
                           void* features_f32_or_null, void* stream);
int ldiff_op_attention(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int B, int heads,
                       int Lq, int Lk, int d, int64_t q_bstride, int64_t kv_bstride, int64_t o_bstride, float scale, void* stream);
/* ldiff_op_attention with a plan batch (ldiff_unet_set_plan_batch): plan_batch = 0 is ldiff_op_attention; n >= B chooses the kernel as if the batch were n */
int ldiff_op_attention_pb(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int B, int heads,
                          int Lq, int Lk, int d, int64_t q_bstride, int64_t kv_bstride, int64_t o_bstride, float scale, int plan_batch, void* stream);
/* Causal self-attention over a short sequence (the text encoder's kernel, text_attn<d>): qkv [B L, ld] f16 is a fused projection output with Q | K | V in column
 * blocks of `hidden` (head h at columns h d of each), o [B L, ldo] f16.  One workgroup per (image, head); keys j > i are masked before an fp32 softmax over the whole
 * row, p is rounded once to fp16, the row sum is the fp32 sum of the unrounded p.  d % 16 == 0 in 16..128, 1 <= L <= 128, ld % 8 == 0, hidden % 8 == 0, ldo % 4 == 0.
 * (CLIPAttention with the causal mask of CLIPTextTransformer: segmentor.py:55-60) */
int ldiff_op_text_attention(const void* qkv, int ld, int hidden, void* o, int ldo, int B, int heads, int L, int d, float scale, void* stream);
/* The same with q ALREADY multiplied by scale * log2(e) (the executors do that in the fp32 epilogue of the q/k/v projection, so q is still rounded
 * once): the kernel then lets the MFMAs subtract the running softmax reference (a 1.0 in K's padding column against -reference in Q's) and skips the
 * per-score FMA.  Head dims with a free column in the last 32-wide k-step only (d = 40, 80: the UNet's levels 0 and 1); others: LDIFF_ERR_INVALID. */
int ldiff_op_attention_prescaled(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int B, int heads,
                                 int Lq, int Lk, int d, int64_t q_bstride, int64_t kv_bstride, int64_t o_bstride, void* stream);
/* sources are (pointer, channels C, row pitch ld (0 = C), lo offset (0 = plain, > 0 = split tensor hi|lo)) */
int ldiff_op_gn_stats(const void* x, int C1, int ld1, int lo1, const void* x2, int C2, int ld2, int lo2, int B, int HW, int groups, float eps,
                      const void* gamma, const void* beta, void* scale, void* shift, void* stream);
/* ldiff_op_gn_stats with a plan batch: 0 is ldiff_op_gn_stats; n >= B chooses the one-launch / two-launch form (gn_stats<1> / gn_stats<2>) as if the batch were n */
int ldiff_op_gn_stats_pb(const void* x, int C1, int ld1, int lo1, const void* x2, int C2, int ld2, int lo2, int B, int HW, int groups, float eps,
                         const void* gamma, const void* beta, void* scale, void* shift, int plan_batch, void* stream);
int ldiff_op_layernorm(const void* x, int ldx, int x_lo, void* y, int rows, int C, const void* gamma, const void* beta, float eps, void* stream);
/* LayerNorm folded into the linear layer that consumes it (BasicTransformerBlock norm1 -> to_q/k/v, norm2 -> attn2.to_q, norm3 -> ff.net.0.proj):
 *   y[rows, N] = LayerNorm(x; gamma, beta, eps)[rows, C] . w[N, C]^T + bias,  x as in ldiff_op_layernorm (x_lo > 0: split rows hi | lo),
 *   the normalised operand rounded ONCE to fp16 (as the two-launch form does); geglu as in ldiff_conv_args (y has N/2 columns).
 * qcols > 0 (a multiple of 64, no GEGLU): columns [0, qcols) are multiplied by qscale in fp32 before the rounding (q of a fused q/k/v projection for
 * ldiff_op_attention_prescaled).
 * Returns LDIFF_ERR_INVALID for shapes the kernel does not take (C != 320, N % 64 != 0, ...): callers then use ldiff_op_layernorm + ldiff_op_conv. */
int ldiff_op_ln_linear(const void* x, int ldx, int x_lo, int rows, int C, const void* gamma, const void* beta, float eps, const void* w, int N, int Nrows,
                       const void* bias_or_null, int geglu, void* y, int ldy, int qcols, float qscale, void* stream);
/* y[m, c] = act(x[m, c] * scale[b, c] + shift[b, c]) (GroupNorm-apply, optional SiLU) over the concat of one or two sources,
 * written plain (y_lo = 0) or split */
int ldiff_op_norm_apply(const void* x, int C1, int ld1, int lo1, const void* x2, int C2, int ld2, int lo2, int B, int HW, const void* scale,
                        const void* shift, int silu, void* y, int ldy, int y_lo, void* stream);
/* weights of a contraction over a split operand: per tap [a(Ca) b(Cb) ..] -> [a a b b 0..] */
int ldiff_op_dup_weights(const void* w, void* wd, int Nrows, int taps, int src_tap_stride, int Ca, int Cb, int dst_tap_stride, void* stream);
/* Split conv operand with an fp8 lo half (the lo product is a 2^-11 correction: three mantissa bits reproduce it to within everything else's noise,
 * profiles/r04_precision_study_lo8.txt; the block-scaled MFMA runs e4m3 at twice the fp16 rate).  norm_apply_lo8: y rows [C1 fp16 | C1 e4m3 of
 * lo * 2^15], 3 C1 bytes, C1 % 16 == 0.  lo8_weights: [Nrows][taps][Cin] fp16 -> [Nrows][taps][Cin fp16 | Cin e4m3 of w * 2^sw] (3 Cin bytes per tap),
 * scale_out[0] = 127 - sw (one int, device memory), Cin % 128 == 0. */
int ldiff_op_norm_apply_lo8(const void* x, int C1, int ld1, int lo1, int B, int HW, const void* scale, const void* shift, int silu, void* y, void* stream);
int ldiff_op_lo8_weights(const void* w, void* wd, void* scale_out, int Nrows, int taps, int Cin, void* stream);
int ldiff_op_geglu(const void* x, void* y, int64_t M, int C4, void* stream);
/* lo_off > 0: also store the rounding remainder of channel c at channel lo_off + c (split first-layer input) */
int ldiff_op_nchw_to_nhwc(const void* x_f32, void* y_f16, int B, int C, int H, int W, int Cpad, int lo_off, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward-pass primitives of the fine-tuning step  --  `engine.backward(loss)` / `engine.step()`
 *   ldiffusion.py:227-255 (V5 loop), model/loss.py:44-126 (loss); the reference trains at 64x64 images = 8x8 latents, where a step
 * is bound by the 859 M weights it reads and writes, so the contractions of the backward pass reuse ldiff_op_conv:
 *   dgrad: dx = ldiff_op_conv(dy, W rearranged to [Cin][ky'][kx'][Cout] with the taps flipped)          (a layout cast by the caller)
 *   wgrad: dW[n][tap*C+c] = ldiff_op_conv as a GEMM over K = M on dyT = ldiff_op_transpose(dy) and xcolT = ldiff_op_im2col_t(x)
 * and the entry points below add what has no forward counterpart.  Activations / gradients NHWC f16, parameter gradients f32.
 * ldiffusion_amd/autograd.py wraps them as torch.autograd.Function objects (the tape is torch's; every FLOP is in this library).
 * ---------------------------------------------------------------------------------------------- */
/* out[(tap*C + c)][m] (rows of Mpad columns, Mpad % 8 == 0, zero padded) = the im2col matrix of x, transposed; m = (b, oy, ox) */
int ldiff_op_im2col_t(const void* x, void* out, int B, int H, int W, int C, int ks, int stride, int pad, int ups, int Ho, int Wo, int Mpad, void* stream);
/* out[n][m] = x[m][n], rows of Mpad columns (zero padded) */
int ldiff_op_transpose(const void* x, void* out, int M, int N, int ldx, int Mpad, void* stream);
/* db[n] = sum_m dy[m, n]  (bias gradient, f32) */
int ldiff_op_colsum(const void* dy, void* db_f32, int M, int N, int ld, void* stream);
/* GroupNorm (+SiLU) forward that keeps mean / rstd [B, groups] f32, and its backward: dx f16; dgamma / dbeta f32 are ACCUMULATED
 * (atomics over the batch; zero them first) */
int ldiff_op_gn_train_fwd(const void* x, void* y, const void* gamma, const void* beta, void* mean, void* rstd, int B, int HW, int C, int groups, float eps,
                          int silu, void* stream);
int ldiff_op_gn_train_bwd(const void* x, const void* dy, const void* gamma, const void* beta, const void* mean, const void* rstd, void* dx, void* dgamma,
                          void* dbeta, int B, int HW, int C, int groups, int silu, void* stream);
/* LayerNorm backward (statistics recomputed from x); dgamma / dbeta accumulated */
int ldiff_op_ln_bwd(const void* x, const void* dy, const void* gamma, void* dx, void* dgamma, void* dbeta, int rows, int C, float eps, void* stream);
/* GEGLU backward: x [M, 2*C4] = [h | gate], dy [M, C4] -> dx [M, 2*C4] */
int ldiff_op_geglu_bwd(const void* x, const void* dy, void* dx, int64_t M, int C4, void* stream);
/* SiLU on n float16 elements and its backward (the time-embedding MLP of the step: time_embedding.act, the SiLU in front of every time_emb_proj) */
int ldiff_op_silu(const void* x, void* y, int64_t n, void* stream);
int ldiff_op_silu_bwd(const void* x, const void* dy, void* dx, int64_t n, void* stream);
/* softmax(scale Q K^T) V backward for short sequences (Lq * Lk <= 8192: the 8x8-latent fine-tuning step); layouts as ldiff_op_attention */
int ldiff_op_attention_bwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* dO, int ldo, void* dq, void* dk, void* dv,
                           int B, int heads, int Lq, int Lk, int d, int64_t q_bstride, int64_t kv_bstride, int64_t o_bstride, float scale, void* stream);
/* one AdamW update of n f32 parameters (torch.optim.AdamW semantics; step counts from 1) */
int ldiff_op_adamw(void* p, const void* g, void* m, void* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                   void* stream);
/* Contrastive (InfoNCE) feature loss of the fine-tuning step for GIVEN sample triples, forward and gradient in one launch
 * (/root/reference/model/loss.py:89-109; the random draws of :62-87 stay on the host, ldiffusion_amd/loss.py sample_triples):
 *   features f32 [B, n, HW] (n <= 32 planes);  triple t = image bi[t], anchor pixel ai[t], positive pi[t], negatives ni[t*K .. t*K+K) (int32, device)
 *   loss[0] = mean_t CE([a.p | a.n_k] / temperature, target 0);  dfeatures [B, n, HW] = d loss / d features.  Both are overwritten.
 *   T_dev (may be NULL): device int32 holding the actual number of triples (<= T, which is then the capacity of the index arrays and the
 *   launch size), read at execution time -- the launch is shape-stable, e.g. inside a captured graph whose batches yield varying counts. */
int ldiff_op_infonce(const void* features, int B, int n, int64_t HW, const void* bi, const void* ai, const void* pi, const void* ni, int T, const void* T_dev,
                     int K, float temperature, void* loss, void* dfeatures, void* stream);
/* Weight layouts of the training step (the float32 master [Cout, Cin, k, k] of torch / diffusers -> what ldiff_op_conv reads):
 *   mode 0, forward: dst[n][ky][kx][c] = w[n][c][ky][kx]           rows >= Cout, Cpad >= Cin, the rest zero
 *   mode 1, dgrad:   dst[c][ky][kx][n] = w[n][c][k-1-ky][k-1-kx]   rows >= Cin,  Cpad >= Cout, the rest zero
 * and back: the wgrad GEMM's g[n][tap*Cx + c] (row pitch ldg) -> dw[n][c][ky][kx] (loss.backward() of /root/reference/ldiffusion.py:254). */
int ldiff_op_pack_weight(const void* w_f32, void* dst_f16, int Cout, int Cin, int k, int rows, int Cpad, int mode, void* stream);
int ldiff_op_unpack_wgrad(const void* g_f32, void* dw_f32, int Cout, int Cin, int k, int Cx, int ldg, void* stream);
/* ldiff_op_pack_weight for MANY (tensor, layout) pairs in one launch.  entries: device array of n_entries records of 48 bytes
 *   { const float* w; _Float16* dst; int32 Cout, Cin, kk (= k*k: 1 or 9), rows, Cpad, mode, tiles_x, 0 }
 * tile_prefix: device int32 [n_entries + 1], tile_prefix[e] = first workgroup of entry e, tile_prefix[n_entries] = n_tiles.  Tiles per entry:
 *   mode 0: tiles_x = ceil(Cpad / 256) times (kk == 1 ? ceil(rows / 8) : rows);  mode 1: tiles_x = ceil(Cpad / 64) times ceil(rows / (kk == 1 ? 64 : 16)). */
int ldiff_op_pack_weight_multi(const void* entries, const void* tile_prefix, int n_entries, int n_tiles, void* stream);

/* All parameters of a model in one launch (the reference's optimiser step, /root/reference/ldiffusion.py:168-171,255: engine.step()).
 * Device tables: tensors[t] = {float* p, float* m, float* v, int64 n} (32 bytes), grads[t] = const float* (gradient of tensor t),
 * chunks[c] = {int32 tensor, int32 pad, int64 first element} (16 bytes): workgroup c updates elements [first, first + 16384) of its tensor. */
int ldiff_op_adamw_multi(const void* tensors, const void* grads, const void* chunks, int64_t nchunks, float lr, float beta1, float beta2, float eps,
                         float weight_decay, int step, void* stream);

/* Training form of the nnU-Net tissue head (nnUNetTrainer.train_step: PlainConvUNet forward + backward, deep-supervision loss, SGD).  The three
 * primitives reduce through per-workgroup partial sums in a caller-supplied workspace and a finalize that adds them in a fixed order: no
 * floating-point atomics, a replay on the same inputs is bit-identical.
 *
 * y = leaky_relu(instance_norm(x; gamma, beta, eps), slope) on NHWC f16 [B, HW, C], C % 8 == 0; mean / rstd f32 [B, C] are written for the backward,
 * which takes them back, recomputes the normalised value and the activation mask from x (no mask tensor), and OVERWRITES dx (f16), dgamma, dbeta
 * (f32 [C], summed over the batch in image order).  ws: ldiff_op_in_train_ws_bytes(B, HW, C) bytes of device memory, 16-byte aligned. */
int64_t ldiff_op_in_train_ws_bytes(int B, int HW, int C);
int ldiff_op_in_train_fwd(const void* x, void* y, const void* gamma, const void* beta, void* mean, void* rstd, int B, int HW, int C, float eps, float slope,
                          void* ws, int64_t ws_bytes, void* stream);
int ldiff_op_in_train_bwd(const void* x, const void* dy, const void* gamma, const void* beta, const void* mean, const void* rstd, void* dx, void* dgamma,
                          void* dbeta, int B, int HW, int C, float slope, void* ws, int64_t ws_bytes, void* stream);
/* DC_and_CE_loss with MemoryEfficientSoftDiceLoss (do_bg = False, ddp = False) of ONE deep-supervision scale, value and gradient:
 *   logits f16 [B, HW, ld], ld = roundup(n_heads, 8) (the seg layer's output; the pad columns take no part), 2 <= n_heads <= 32;
 *   target uint8 (target_i64 = 0) or int64 (1) [B, HW], labels in [0, n_heads) (another label makes the loss and that pixel's dlogits NaN);
 *   p = softmax over the n_heads real columns (fp32); per foreground class c: intersect = sum p_c [t == c], sum_pred = sum p_c, sum_gt = sum [t == c]
 *   over the pixels of a sample, and over the batch as well when batch_dice != 0;  dc = (2 intersect + smooth) / max(sum_gt + sum_pred + smooth, 1e-8);
 *   loss[0] (f32) = mean cross-entropy - mean dc;   dlogits f16 [B, HW, ld] = grad_scale * weight * d loss / d logits, pad columns zero.
 * grad_scale is the loss scale of the step: most of these gradients lie below float16's range unscaled.  ws: ldiff_op_dice_ce_ws_bytes(...) bytes. */
int64_t ldiff_op_dice_ce_ws_bytes(int B, int64_t HW, int n_heads);
int ldiff_op_dice_ce(const void* logits, int ld, int n_heads, const void* target, int target_i64, int B, int64_t HW, int batch_dice, float smooth, float weight,
                     float grad_scale, void* loss, void* dlogits, void* ws, int64_t ws_bytes, void* stream);
/* The same loss split at its sums, for data-parallel training (the reference's DC_and_CE_loss with ddp = True gathers the Dice statistics of all ranks
 * when batch_dice is set).  NACC = 3 ld + 2 doubles per row: sum_pred[ld], intersect[ld], sum_gt[ld], the cross-entropy sum, the count of labels outside
 * [0, n_heads); one row with batch_dice, B rows without.
 *   ldiff_op_dice_ce_stats      sums (device f64 [rows, NACC]) of this process's pixels, added in the order ldiff_op_dice_ce adds them.
 *   ldiff_op_dice_ce_from_sums  loss[0] = local cross-entropy sum / (B HW) - mean dc(dice_sums);  dlogits = grad_scale * weight * ((p - 1_t) / (B HW) +
 *                               world * d(-mean dc)/d logits at dice_sums).  dice_sums: the local sums, or with batch_dice the sum of `world` processes'
 *                               (their backward all-reduces identical rows: the factor world).  local_sums supplies the cross-entropy sum and B is local.
 * stats then from_sums on the same sums with world = 1 give ldiff_op_dice_ce's loss and dlogits bit for bit.  ws: ldiff_op_dice_ce_ws_bytes(...) bytes each. */
int ldiff_op_dice_ce_stats(const void* logits, int ld, int n_heads, const void* target, int target_i64, int B, int64_t HW, int batch_dice, void* sums, void* ws,
                           int64_t ws_bytes, void* stream);
int ldiff_op_dice_ce_from_sums(const void* logits, int ld, int n_heads, const void* target, int target_i64, int B, int64_t HW, int batch_dice, float smooth,
                               float weight, float grad_scale, const void* dice_sums, const void* local_sums, int world, void* loss, void* dlogits, void* ws,
                               int64_t ws_bytes, void* stream);
/* The three with nnU-Net's ignore label (DC_and_CE_loss(ignore_label = k); compound_losses.py:31-56, dice.py:72-119): a pixel whose label equals
 * ignore_label (n_heads <= ignore_label <= 254; nnU-Net's rule makes it n_heads) adds nothing -- the Dice sums run over the other, annotated pixels, the
 * cross-entropy is their sum over their count (this process's own; 0 when the count is 0, the Dice term is then -1), the pixel's dlogits row is +0 and its
 * logits are never read.  A label that is neither a class nor ignore_label still makes the loss and that pixel's dlogits NaN.  Region labels have entries of their own (ldiff_op_dice_focal, below).
 * A row of statistics holds ldiff_op_dice_ce_ignore_nacc(n_heads) = 3 ld + 3 doubles: the plain row, then the count of annotated pixels.
 * ws: ldiff_op_dice_ce_ignore_ws_bytes(...) bytes each.  On a target without an ignored pixel the three give the plain entries' loss and dlogits bit for bit;
 * stats then from_sums give ldiff_op_dice_ce_ignore's bits.  from_sums takes this process's own rows: the data-parallel exchange of the ignore form
 * (all ranks' Dice statistics with each rank's own annotated count) is not built. */
int64_t ldiff_op_dice_ce_ignore_ws_bytes(int B, int64_t HW, int n_heads);
int ldiff_op_dice_ce_ignore_nacc(int n_heads);
int ldiff_op_dice_ce_ignore(const void* logits, int ld, int n_heads, int ignore_label, const void* target, int target_i64, int B, int64_t HW, int batch_dice,
                            float smooth, float weight, float grad_scale, void* loss, void* dlogits, void* ws, int64_t ws_bytes, void* stream);
int ldiff_op_dice_ce_ignore_stats(const void* logits, int ld, int n_heads, int ignore_label, const void* target, int target_i64, int B, int64_t HW, int batch_dice,
                                  void* sums, void* ws, int64_t ws_bytes, void* stream);
int ldiff_op_dice_ce_ignore_from_sums(const void* logits, int ld, int n_heads, int ignore_label, const void* target, int target_i64, int B, int64_t HW,
                                      int batch_dice, float smooth, float weight, float grad_scale, const void* sums, void* loss, void* dlogits, void* ws,
                                      int64_t ws_bytes, void* stream);
/* Region labels (nnU-Net's region-based training: one sigmoid head per region, regions may overlap).  The target stays the LABEL MAP; membership is looked up in
 * table = device uint32 [256] indexed by label value (nnunet.region_spec builds it): bit r = the value belongs to region r (r < n_regions <= 24), bit 31 = the
 * ignore label, bit 30 = no label of the dataset (makes the loss and that pixel's dlogits NaN, as a label outside [0, n_heads) does in ldiff_op_dice_ce; an
 * int64 label outside a byte's range is read as 255).  logits f16 [B, HW, ld], ld = roundup(n_regions, 8), target uint8 / int64 [B, HW].
 * Per annotated pixel and region, in fp32: x the logit, y the table bit, s = 2 y - 1, p = sigmoid(x), p_t = sigmoid(s x), q = sigmoid(-s x),
 * bce = max(x, 0) - x y + log1p(exp(-|x|));  bce = 0: f = 0.25 q^2 bce (DC_and_Focal_loss, alpha 0.25, gamma 2);  bce = 1: f = bce (DC_and_BCE_loss).
 *   use_ignore = 0: term = mean f over B n_regions HW (a pixel with the ignore bit is then a bad label);
 *   use_ignore = 1: pixels with the ignore bit take no part (logits never read, dlogits row +0); term = sum f / max(A, 1e-8), A = this process's annotated
 *                   PIXELS -- not times n_regions, as the reference has it: the two differ by the factor n_regions even when nothing is ignored.
 * Dice = MemoryEfficientSoftDiceLoss(sigmoid, do_bg = True): sums over annotated pixels, ALL regions, M = (batch_dice ? 1 : B) n_regions averaged terms,
 * dc = (2 intersect + smooth) / max(sum_gt + sum_pred + smooth, 1e-8).  loss[0] = term - mean dc;  dlogits = grad_scale * weight * d loss / d logits, pad columns +0.
 * Rows of statistics hold ldiff_op_dice_focal_nacc(n_regions) = 3 ld + 3 doubles: sum_pred[ld], intersect[ld], sum_gt[ld], sum f, bad labels, annotated pixels.
 * _stats / _from_sums split the loss as ldiff_op_dice_ce_stats / _from_sums do (same roles of dice_sums, local_sums, world; stats then from_sums at world = 1
 * give ldiff_op_dice_focal's bits); with use_ignore = 1 from_sums takes world = 1 and dice_sums == local_sums only.  No floating-point atomics: bit-reproducible.
 * ws: ldiff_op_dice_focal_ws_bytes(...) bytes each, 16-byte aligned. */
int64_t ldiff_op_dice_focal_ws_bytes(int B, int64_t HW, int n_regions);
int ldiff_op_dice_focal_nacc(int n_regions);
int ldiff_op_dice_focal(const void* logits, int ld, int n_regions, const void* table, const void* target, int target_i64, int use_ignore, int bce, int B, int64_t HW,
                        int batch_dice, float smooth, float weight, float grad_scale, void* loss, void* dlogits, void* ws, int64_t ws_bytes, void* stream);
int ldiff_op_dice_focal_stats(const void* logits, int ld, int n_regions, const void* table, const void* target, int target_i64, int use_ignore, int bce, int B,
                              int64_t HW, int batch_dice, void* sums, void* ws, int64_t ws_bytes, void* stream);
int ldiff_op_dice_focal_from_sums(const void* logits, int ld, int n_regions, const void* table, const void* target, int target_i64, int use_ignore, int bce, int B,
                                  int64_t HW, int batch_dice, float smooth, float weight, float grad_scale, const void* dice_sums, const void* local_sums, int world,
                                  void* loss, void* dlogits, void* ws, int64_t ws_bytes, void* stream);
/* Validation counts of region training (nnUNetTrainer.validation_step's region branch): counts = device int64 [3, n_regions] = tp, fp, fn of
 * `logit > threshold` against the table bit, over the pixels without the ignore bit; exact.  A pixel whose label has bit 30 (no label of the dataset) is a
 * member of no region here: it counts towards fp where a logit exceeds the threshold, and raises nothing -- the loss entries make the same pixel NaN.  ws: ldiff_op_region_counts_ws_bytes(...) bytes. */
int64_t ldiff_op_region_counts_ws_bytes(int B, int64_t HW, int n_regions);
int ldiff_op_region_counts(const void* logits, int ld, int n_regions, const void* table, const void* target, int target_i64, int B, int64_t HW, float threshold,
                           void* counts, void* ws, int64_t ws_bytes, void* stream);
/* LabelManager.convert_probabilities_to_segmentation's region branch on logits [n_regions, H, W] (f16, or f32 with logits_f32 = 1): the pixel is 0, then for
 * i in order regions_class_order[i] (host int [n_regions], 0 .. 255) where logit_i > threshold, later entries overwriting earlier ones; a NaN logit compares
 * false.  Written into mask u8 [mask_H, mask_W] at (mask_y0, mask_x0), as ldiff_op_window_finish places its mask.  `sigmoid(l) > 0.5` is a step function of
 * the logit: the caller passes the step of the dtype the reference thresholds in (nnunet.REGION_THRESHOLD_F32 / _F16). */
int ldiff_op_region_mask_u8(const void* logits, int logits_f32, int n_regions, int H, int W, const int* regions_class_order, float threshold, void* mask, int mask_H,
                            int mask_W, int mask_y0, int mask_x0, void* stream);
/* Postprocessing (postprocessing/remove_connected_components.py:22-34, remove_all_but_largest_component_from_segmentation) on N uint8 label maps [N, H, W],
 * each image on its own.  table = 256 device bytes: byte v is 1 when the value v belongs to the label, list of labels or region being filtered; the binary
 * mask is table[seg] and is never stored.  Components under 8-connectivity (full connectivity: skimage.measure.label(mask, connectivity=None)); a component's
 * label is the smallest linear pixel index y W + x in it, so nothing depends on scheduling.  The largest component is kept; among components of equal
 * largest size the one whose first pixel in raster order comes first, that is the smallest label (UNPINNED: the reference calls acvl_utils, which the
 * test-suite cannot import; the rule lives in cc_winner_key of kernels_segpost.hip).  An empty mask changes nothing.
 *   ldiff_op_keep_largest_component: seg_out = seg_in with every member pixel outside the kept component set to background_label (0 .. 255), every other
 *     pixel copied.  seg_in is not modified; a seg_out that overlaps seg_in is refused.
 *   ldiff_op_cc_label: labels int32 [N, H, W] = the component's label + 1, 0 outside the mask; sizes int32 [N, H, W] = the component's pixel count at its
 *     label's pixel, 0 everywhere else.
 * Seven launches: union-find per LDIFF_CC_TILE_H x LDIFF_CC_TILE_W tile in LDS, a merge of the tile seams (agent-scope atomic loads and atomicMin only, no
 * waiting between workgroups), flatten, sizes by integer atomic adds, the per-image winner, the result.  Integer atomics only: bit-reproducible.
 * Limits, anything else LDIFF_ERR_INVALID naming the argument: 1 <= N, 1 <= H, 1 <= W, H * W <= 2^30, N * ceil(H W / 256) < 2^31.
 * ws: ldiff_op_keep_largest_component_ws_bytes(N, H, W) bytes (both entries; 8 bytes per pixel + 8 per image; 0 for a shape that is not accepted), 8-byte aligned. */
#define LDIFF_CC_TILE_H 32
#define LDIFF_CC_TILE_W 32
int64_t ldiff_op_keep_largest_component_ws_bytes(int N, int H, int W);
int ldiff_op_keep_largest_component(const void* seg_in, void* seg_out, int N, int H, int W, const void* table, int background_label, void* ws, int64_t ws_bytes,
                                    void* stream);
int ldiff_op_cc_label(const void* seg, int N, int H, int W, const void* table, void* labels_i32, void* sizes_i32, void* ws, int64_t ws_bytes, void* stream);
/* The gradient bucket of a data-parallel step.  ldiff_op_bucket_pack: bucket[offsets[t] + i] = grads[t][i] for every tensor in one launch; grads = device
 * table of const float*, offsets = device int64 [T + 1] (prefix sums of the element counts), chunks as ldiff_op_adamw_multi's.
 * ldiff_op_sumsq: out_f32[0] = sqrt(sum x^2) of n f32 elements (4-byte aligned) through one fp32 partial per 16384 elements (at most 27 dependent roundings
 * each) and a fixed-order double finalize: no atomics, a replay gives the same bits; a non-finite element gives a non-finite result.
 * ws: ldiff_op_sumsq_ws_bytes(n) bytes = 4 bytes per partial. */
int ldiff_op_bucket_pack(const void* grads, const void* offsets, const void* chunks, int64_t nchunks, void* bucket, void* stream);
int64_t ldiff_op_sumsq_ws_bytes(int64_t n);
int ldiff_op_sumsq(const void* x, int64_t n, void* out_f32, void* ws, int64_t ws_bytes, void* stream);
/* torch.optim.SGD(lr, momentum, nesterov=True, weight_decay) over many f32 tensors in one launch.  Device tables as ldiff_op_adamw_multi's, with
 * tensors[t] = {float* p, float* momentum_buffer, int64 n} (24 bytes).  inv_scale / clip_coef: device f32 scalars read at execution time.
 *   g = inv_scale * clip_coef * grad + weight_decay * p;   buf = first ? g : momentum * buf + g;   p -= lr * (g + momentum * buf) */
int ldiff_op_sgd_nesterov_multi(const void* tensors, const void* grads, const void* chunks, int64_t nchunks, float lr, float momentum, float weight_decay,
                                int first, const void* inv_scale, const void* clip_coef, void* stream);

/* Weight and bias gradients of the narrow convs of nnUNetTrainer.train_step's backward (`self.grad_scaler.scale(l).backward()`), where M = B Ho Wo runs to
 * millions of rows under 32 .. 128 channels: both reduce through per-workgroup fp32 partials in a caller-supplied workspace (16-byte aligned) and a finalize
 * that adds them in workgroup order -- no floating-point atomics, a replay on the same inputs is bit-identical.
 *
 * ldiff_op_conv_wgrad: dw[n][c][ky][kx] (f32, torch's [Cout][Cin][k][k], OVERWRITTEN) = sum_(b,oy,ox) dy[b,oy,ox,n] x[b, oy stride - pad + ky, ox stride - pad + kx, c],
 *   zero outside the image, straight from x f16 [B,H,W,Cx] and dy f16 [B,Ho,Wo,Cy] (NHWC; channels c >= Cin of x and n >= Cout of dy take no part): no
 *   im2col, no transposed copy, no unpack launch.  Accepted, anything else LDIFF_ERR_INVALID naming the argument: k = 3 with stride 1 or 2 (pad 1) or k = 1
 *   with stride 1 (pad 0); Ho, Wo = the conv's output size (no upsampling); Cx % 8 == 0, Cx <= 128; Cy % 8 == 0, Cy <= 64 (k = 3) or 128 (k = 1);
 *   1 <= Cout <= Cy, 1 <= Cin <= Cx; ws_bytes >= ldiff_op_conv_wgrad_ws_bytes(...) (0 for a shape that is not accepted) for the same wgs.
 *   wgs = 0: the library plans the persistent grid; wgs > 0: that many tile-walking workgroups per 32-channel slab of Cx (tests: few workgroups walking many
 *   tiles, or more workgroups than tiles -- an idle workgroup contributes exact zeros).
 * ldiff_op_colsum_slabs: db[n] (f32 [N], OVERWRITTEN) = sum_m dy[m, n] over row slabs; dy f16 [M, ld], N % 8 == 0, N <= 2048, ld % 8 == 0, ld >= N, M >= 1. */
int64_t ldiff_op_conv_wgrad_ws_bytes(int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs);
int ldiff_op_conv_wgrad(const void* x, const void* dy, void* dw_f32, int B, int H, int W, int Cx, int Ho, int Wo, int Cy, int Cout, int Cin, int k, int stride, int wgs,
                        void* ws, int64_t ws_bytes, void* stream);
int64_t ldiff_op_colsum_slabs_ws_bytes(int64_t M, int N);
int ldiff_op_colsum_slabs(const void* dy, void* db_f32, int64_t M, int N, int ld, void* ws, int64_t ws_bytes, void* stream);

/* ldiff_op_conv_wgrad_wide: the contraction, arguments, layouts and reduction of ldiff_op_conv_wgrad for the WIDE convs that entry refuses (the 128- and
 *   256-channel stages, the transposed convs run as linears, the head): a workgroup owns a 64 (output) x 32 (input channels) block of dw, and the blocks of
 *   both channel axes are grid axes beside the tile-walking workgroups.  Accepted, anything else LDIFF_ERR_INVALID naming the argument: k = 3 with stride 1 or
 *   2 (pad 1) or k = 1 with stride 1 (pad 0); Ho, Wo = the conv's output size (no upsampling); Cx % 8 == 0, 8 <= Cx <= 1024; Cy % 8 == 0, 8 <= Cy <= 512
 *   (k = 3) or 2048 (k = 1); 1 <= Cout <= Cy, 1 <= Cin <= Cx; wgs = 0 (planned) or 1 .. 65535 tile-walking workgroups per block; fewer than 2^31 tiles;
 *   ws_bytes >= ldiff_op_conv_wgrad_wide_ws_bytes(...) (0 for a shape that is not accepted) for the same wgs.
 *   Workspace = wgs * roundup(Cy, 64) * k * k * roundup(Cx, 32) * 4 bytes.  Planned (wgs = 0), wgs = max(1, min(tiles, 1024 / blocks)) and blocks <= 1024, so
 *   the workspace never exceeds LDIFF_WGRAD_WIDE_MAX_WS_BYTES = 1024 * 64 * 32 * 9 * 4, whatever the channel counts (k = 1: a ninth of it). */
#define LDIFF_WGRAD_WIDE_MAX_WS_BYTES 75497472
int64_t ldiff_op_conv_wgrad_wide_ws_bytes(int B, int Ho, int Wo, int Cx, int Cy, int k, int wgs);
int ldiff_op_conv_wgrad_wide(const void* x, const void* dy, void* dw_f32, int B, int H, int W, int Cx, int Ho, int Wo, int Cy, int Cout, int Cin, int k, int stride,
                             int wgs, void* ws, int64_t ws_bytes, void* stream);

/* Tissue head, training data: nnUNetDataLoader2D + the transforms of nnUNetTrainer.get_training_transforms (SimulateLowResolutionTransform only through
 * ldiff_op_seg_intensity_lr), on cases that stay on the device.  The host draws every random number and hands the kernels three tables (device memory, plain C structs):
 *   ldiff_seg_case    one per case: byte offsets into ONE arena (16-byte aligned) of the cubic B-spline coefficients f32 [C, H, stride], the raw
 *                     normalised image f32 [C, H, stride] and the labels u8 [H, label_stride]
 *   ldiff_seg_sample  one per sample: the case; m, the patch index (i, j) -> case coordinate map  y = m[0] i + m[1] j + m[2],  x = m[3] i + m[4] j + m[5]
 *                     (rotation, scale, mirror and crop centre folded in); copy != 0: m[0], m[4] are +-1 and m[2], m[5] integers, and the sample is an
 *                     exact crop of the raw image; the Gaussian noise's sigma (0 = off) and the sample's first Philox counter
 *   ldiff_seg_chan    one per (sample, channel): 0 = off, except brightness (1 = off).  lowres_zoom is read by ldiff_op_seg_intensity_lr alone; for
 *                     ldiff_op_seg_intensity it stays a reserved slot that is not read.
 * ldiff_op_seg_sample: data f32 [B, C, h, w]: order-3 spline of the coefficients (scipy.ndimage.map_coordinates(order=3, mode='constant', cval=0): taps
 *   mirrored at whole samples, 0 where a coordinate leaves [0, n - 1]).  target u8: the n_scales label maps [B, 1, h >> k, w >> k], one after the other,
 *   scale k holding the label of full-resolution pixel (2^k i + 2^(k-1), 2^k j + 2^(k-1)); a label is the highest one whose bilinear indicator reaches
 *   0.5, else 0 (interpolate_img(is_seg=True, order=1)), and 0 outside the case.  h, w divisible by 2^(n_scales - 1), n_scales <= 8.  A table row that
 *   names no case, leaves the arena or holds a float offset that is no multiple of 4 yields zeros.
 * ldiff_op_seg_intensity: in place on data, per plane: x + sigma N(0, 1); gaussian_filter(x, blur_sigma) (axis 0 then 1, radius int(4 sigma + 0.5),
 *   'reflect'; supported for blur_sigma < 1.875, radius <= 7: below 0.125 the radius is 0 and the filter the identity, as in scipy; from 1.875 on the row
 *   counts as off and the plane is not blurred); x * brightness; clip((x - mean) contrast + mean, min, max); gamma with retained statistics on -x (gamma_inverted) and on x (gamma):
 *   ((x - min) / (max - min + 1e-7))^g (max - min) + min, then (x - mean') / (std' + 1e-8) * std + mean.  normal: f32 [B, C, h, w] draws, or NULL:
 *   Box-Muller over Philox4x32-10 keyed by (seed, philox_offset + (c h w + i) / 4).  ws: ldiff_op_seg_intensity_ws_bytes(...) bytes.  No atomics:
 *   a replay on the same inputs is bit-identical.
 * ldiff_op_seg_intensity_lr: the same chain with SimulateLowResolutionTransform between contrast and the gammas, per plane with zoom = lowres_zoom:
 *   target shape m = rint(h zoom), rint(w zoom) (float32 product, half to even); the step is off and the plane untouched when zoom is NaN or outside
 *   (0, 1], when an m is below 1, or when m = (h, w).  d[i, j] = x[((2 i + 1) h) / (2 m0), ((2 j + 1) w) / (2 m1)] (order 0, integer division); d padded by 12
 *   edge samples a side and prefiltered as by ldiff_op_spline_prefilter; output (i, j) = the cubic B-spline at (((2 i + 1) m0 - h) / (2 h),
 *   ((2 j + 1) m1 - w) / (2 w)), floor and fraction formed in integers, 4 x 4 taps clamped to the padded plane; clipped to [min d, max d].  That is
 *   scipy.ndimage.zoom(order 0, then order 3, mode='nearest', grid_mode=True) and the clip of skimage.transform.resize; where scipy's floating-point
 *   order-0 index rounds an exact tie one lower, the integer rule stands.  h, w <= 16384.  ws: ldiff_op_seg_intensity_lr_ws_bytes(...) =
 *   B C (h + 24) (w + 24) 4 bytes (the blur's plane lives in it too).  Same reduction order and determinism as ldiff_op_seg_intensity.
 * ldiff_op_spline_prefilter: scipy.ndimage.spline_filter(order=3, mode='mirror') in place on n_planes f32 planes [H, W] of row stride `stride`, plane
 *   p at planes + p H stride; axis 0 then axis 1, one workgroup per plane, the causal start summed over 64 samples (or exactly, over the mirrored
 *   period, below 64).  Refused: H < 1, W < 1, stride < W, a pointer not aligned to 4 bytes, H stride >= 2^30. */
typedef struct ldiff_seg_case { int64_t coef_off, raw_off, label_off; int32_t H, W, stride, label_stride; } ldiff_seg_case;
typedef struct ldiff_seg_sample { float m[6]; int32_t case_index, copy; float noise_sigma; uint32_t reserved; uint64_t philox_offset; } ldiff_seg_sample;
typedef struct ldiff_seg_chan { float blur_sigma, brightness, contrast, lowres_zoom, gamma_inverted, gamma; } ldiff_seg_chan;
int ldiff_op_seg_sample(const void* arena, int64_t arena_bytes, const ldiff_seg_case* cases, int n_cases, const ldiff_seg_sample* samples, int B, int C, int h,
                        int w, int n_scales, void* data, void* target, void* stream);
int64_t ldiff_op_seg_intensity_ws_bytes(int B, int C, int h, int w);
int ldiff_op_seg_intensity(void* data, const ldiff_seg_sample* samples, const ldiff_seg_chan* chans, int B, int C, int h, int w, const void* normal_or_null,
                           uint64_t seed, void* ws, int64_t ws_bytes, void* stream);
int64_t ldiff_op_seg_intensity_lr_ws_bytes(int B, int C, int h, int w);
int ldiff_op_seg_intensity_lr(void* data, const ldiff_seg_sample* samples, const ldiff_seg_chan* chans, int B, int C, int h, int w, const void* normal_or_null,
                              uint64_t seed, void* ws, int64_t ws_bytes, void* stream);
int ldiff_op_spline_prefilter(void* planes_f32, int n_planes, int H, int W, int stride, void* stream);

/* Tissue head, plan and preprocess: what DefaultPreprocessor.run_case_npy and DatasetFingerprintExtractor.analyze_case do per training case, for a case that
 * is on the device: img, C planes [H, W] of uint8 (dtype 0) or float32 (dtype 1), rows row_stride and planes plane_stride ELEMENTS apart; label_u8 [H, W]
 * uint8, rows label_stride bytes apart.  C <= 16, H, W <= 32768.  A box is (y0, y1, x0, x1), ends exclusive, non-empty and inside the case; the host
 * reads it back from ldiff_op_case_bbox and hands it to the other four.  No kernel reads or writes outside the case, the box or the stated outputs.
 * ldiff_op_case_bbox: box (device, int32 [4]) of the pixels where any channel is non-zero (NaN counts as non-zero); the full extent for an all-zero image:
 *   crop_to_nonzero's box (cropping.py:24-49; filling the mask's holes never moves it).
 * ldiff_op_case_stats: stats (device, C records of 32 bytes): the sum and the sum of squares of the channel over the box -- uint64 for uint8 input (exact),
 *   float64 for float32 input (per-workgroup partial sums over fixed slices of rows, added in index order: no float atomics, bit-identical from run to
 *   run) -- then min and max as float64.  ws: ldiff_op_case_stats_ws_bytes(C) bytes, 8-byte aligned.
 * ldiff_op_case_counts: row_counts uint32 [rows, n_heads + 1]: per row of the box the pixels of class 0 .. n_heads - 1, then those with a label >= n_heads;
 *   row_prefix uint32 [n_heads + 1, rows + 1]: per selector -- class c, or (index n_heads) `label > 0` -- the selected pixels above each row, the last
 *   entry the total; totals uint32 [n_heads + 2]: per class, `label > 0`, labels >= n_heads.  n_heads <= 32.  Exact.
 * ldiff_op_case_counts_classes: the same with one more selector, `label < n_classes` (1 <= n_classes <= n_heads <= 33) -- "the label is a class" of a map
 *   whose highest value is an ignore label, counted here as class n_heads - 1: row_prefix uint32 [n_heads + 2, rows + 1], that selector's row last;
 *   totals uint32 [n_heads + 3], its count last.  The other rows and entries are ldiff_op_case_counts'.
 * ldiff_op_case_apply: the cropped planes as float32 (x - sub[c]) / div[c] (sub, div: HOST arrays of C floats; one subtraction and one correctly rounded
 *   division) to arena + row->raw_off [C, h, row->stride], also to row->coef_off when write_coef != 0 (ldiff_op_spline_prefilter then runs in place),
 *   and the cropped labels to row->label_off [h, row->label_stride].  row: a HOST ldiff_seg_case with H, W the box's extent; refused when a span leaves
 *   the arena or a float offset is no multiple of 4.
 * ldiff_op_case_rank_to_coord: coords int32 [n, 2] = (row, column) inside the box of the rank-th selected pixel in row-major order, numpy's
 *   argwhere(selection)[rank]; selector = a class, -1 for `label > 0`, or -1 - m for `label < m` (1 <= m <= 255: ldiff_op_case_counts_classes' selector);
 *   row_prefix: that selector's uint32 [rows + 1] of ldiff_op_case_counts; ranks int64
 *   [n], any order, repeats allowed.  values_or_null [n, C] of the image's dtype: the pixel's C channels.  A rank outside [0, total) yields (-1, -1) and
 *   zeros. */
int ldiff_op_case_bbox(const void* img, int dtype, int C, int H, int W, int64_t row_stride, int64_t plane_stride, int32_t* box, void* stream);
int64_t ldiff_op_case_stats_ws_bytes(int C);
int ldiff_op_case_stats(const void* img, int dtype, int C, int H, int W, int64_t row_stride, int64_t plane_stride, int y0, int y1, int x0, int x1, void* stats, void* ws,
                        int64_t ws_bytes, void* stream);
int ldiff_op_case_counts(const void* label_u8, int H, int W, int64_t label_stride, int y0, int y1, int x0, int x1, int n_heads, uint32_t* row_counts, uint32_t* row_prefix,
                         uint32_t* totals, void* stream);
int ldiff_op_case_counts_classes(const void* label_u8, int H, int W, int64_t label_stride, int y0, int y1, int x0, int x1, int n_heads, int n_classes,
                                 uint32_t* row_counts, uint32_t* row_prefix, uint32_t* totals, void* stream);
int ldiff_op_case_apply(const void* img, int dtype, int C, int H, int W, int64_t row_stride, int64_t plane_stride, const void* label_u8, int64_t label_stride, int y0, int y1,
                        int x0, int x1, const float* sub, const float* div, void* arena, int64_t arena_bytes, const ldiff_seg_case* row, int write_coef, void* stream);
int ldiff_op_case_rank_to_coord(const void* label_u8, int H, int W, int64_t label_stride, int y0, int y1, int x0, int x1, int selector, const uint32_t* row_prefix,
                                const int64_t* ranks, int64_t n, int32_t* coords, const void* img_or_null, int dtype, int C, int64_t row_stride, int64_t plane_stride,
                                void* values_or_null, void* stream);

/* Tissue head, batched sliding window: one image of nnUNetPredictor.predict_sliding_window_return_logits (predict_from_raw_data.py:547-635) in a few
 * launches -- gather a batch of tiles x mirror variants, ONE ldiff_segnet_forward, accumulate the whole batch, finish.  A chunk of tiles travels BY VALUE
 * in the kernels' arguments (a HOST ldiff_window_tiles: no copy to the device, no allocation); more than LDIFF_WINDOW_MAX_TILES tiles, n_variants not
 * 1 / 2 / 4, a variant mask outside 0..3 or a tile that leaves the padded extent are LDIFF_ERR_INVALID and nothing is enqueued.  A variant is a flip
 * mask: bit 0 flips axis 0 (rows), bit 1 axis 1 (columns); variants[0] is the identity in maybe_mirror_and_predict's order (predict_from_raw_data.py:530-545).
 * Batch entry k * n_variants + v is tile k under variant v.
 * ldiff_op_window_gather: img [C, h, w] float32, rows row_stride and planes plane_stride ELEMENTS apart, zero padded to [Hp, Wp] with its first pixel at
 *   (pad_top, pad_left) (acvl_utils pad_nd_image) -> x [n_tiles * n_variants, C, th, tw] float32: x[k, v, c, y, x] = padded(c, y0[k] + y', x0[k] + x'),
 *   y' = th - 1 - y when v flips axis 0, else y; likewise x'.  Exactly 0 in the pad.  n_valid is not read.
 * ldiff_op_window_accumulate_batch: acc [heads, Hp, Wp], cnt [Hp, Wp], pred [n_tiles * n_variants, heads, th, tw], weight [th, tw] of acc's type or NULL
 *   (weight 1).  dtypes as ldiff_window_accumulate -- 0: all float32, 1: all float16, 3: float16 accumulators and weight with a float32 prediction -- and
 *   2: float32 accumulators and weight with a float16 prediction.  One thread owns a pixel (or four adjacent ones) of the bounding box of the first
 *   n_valid tiles and walks those tiles IN ORDER; per covering tile and class:
 *     p = pred[k, 0];  p = rn(p + pred[k, v] at the un-flipped coordinate) for v = 1 .. n_variants - 1;  p = rn(p / n_variants) when n_variants > 1
 *       -- every rounding to the PREDICTION's type, as `prediction += flip(...); prediction /= n` rounds a tensor of that type;
 *     prod = rn(p * weight) in the promoted type of (prediction, weight) (float16 only when both are; dtypes 2 widens p first);
 *     acc = rn_T(acc + prod);  cnt = rn_T(cnt + weight)  -- ldiff_window_accumulate's rule, no fused multiply-add anywhere.
 *   Tiles n_valid .. n_tiles - 1 (the filler of a short last chunk) are not read.  Every pixel has one writer and chunks are ordered by the stream, so
 *   the result is that of n_valid ldiff_window_accumulate calls on the averaged tiles, bit for bit, whatever the chunk size.  heads <= 32.
 * ldiff_op_window_finish: over the h x w pixels of the padded extent from (y0, x0) (the revert slices): l_c = rn_T(acc_c / cnt), a correctly rounded
 *   float32 division and one rounding to the accumulators' type T (acc_f16 != 0: float16).  *inf_flag (device int32, zeroed by the caller) is set to 1
 *   when any l_c is +-inf.  logits_or_null [heads, h, w] of type T receives l; mask_or_null uint8 [mask_H, mask_W] receives, at (mask_y0 + y, mask_x0 + x),
 *   the arg-max by ldiff_argmax_u8's rule bit for bit (first maximal class; any NaN or +inf logit: class 0).  heads <= 32.
 * ldiff_op_window_finish_ensemble: the finish of n_folds heads of one image in ONE launch, where nnUNetPredictor sums the folds' logits and divides by
 *   their number (predict_from_raw_data.py:459-494).  acc is a HOST array of n_folds device pointers, each [heads, Hp, Wp] of type T; the table travels by
 *   value in the kernel's arguments.  cnt_or_null [Hp, Wp] is the count plane all folds share; NULL: the inputs are logits already (the per-tile path).
 *   Per pixel and head, every operation rounded on its own, no fused multiply-add:
 *     l_k = cnt ? rn_T(acc_k / cnt) : acc_k;  *inf_flag = 1 when any l_k is +-inf (the reference raises per fold, before the sum);
 *     s = l_0;  s = rn_T(s + l_k) for k = 1 .. n_folds - 1 in table order;  s = rn_T(s / (float)n_folds) when n_folds > 1, the float32 division correctly
 *     rounded.  An overflow of the sum itself is not flagged (the reference does not look there); the arg-max rule sends such a pixel to class 0.
 *   logits_or_null and mask_or_null receive s and its arg-max as ldiff_op_window_finish writes them.  With n_folds == 1 and cnt given the outputs are
 *   ldiff_op_window_finish's bit for bit.  n_folds outside 1 .. LDIFF_ENSEMBLE_MAX_FOLDS, heads outside 1 .. 32, a box or mask box that leaves its extent
 *   or a null table entry are LDIFF_ERR_INVALID and nothing is enqueued.
 * All four: enqueued on `stream`, no synchronisation, no allocation, no workspace. */
#define LDIFF_WINDOW_MAX_TILES 64
typedef struct ldiff_window_tiles {
  int32_t n_tiles, n_valid, n_variants, reserved;
  int32_t variants[4];
  int32_t y0[LDIFF_WINDOW_MAX_TILES], x0[LDIFF_WINDOW_MAX_TILES];
} ldiff_window_tiles;
int ldiff_op_window_gather(const void* img_f32, int C, int h, int w, int64_t row_stride, int64_t plane_stride, int pad_top, int pad_left, int Hp, int Wp,
                           const ldiff_window_tiles* tiles, int th, int tw, void* x_f32, void* stream);
int ldiff_op_window_accumulate_batch(void* acc, void* cnt, const void* pred, const void* weight_or_null, int heads, int Hp, int Wp, int th, int tw,
                                     const ldiff_window_tiles* tiles, int dtypes, void* stream);
int ldiff_op_window_finish(const void* acc, const void* cnt, int heads, int Hp, int Wp, int y0, int x0, int h, int w, int acc_f16, void* logits_or_null,
                           void* mask_or_null, int mask_H, int mask_W, int mask_y0, int mask_x0, int32_t* inf_flag, void* stream);
#define LDIFF_ENSEMBLE_MAX_FOLDS 8
int ldiff_op_window_finish_ensemble(const void* const* acc, int n_folds, const void* cnt_or_null, int heads, int Hp, int Wp, int y0, int x0, int h, int w,
                                    int acc_f16, void* logits_or_null, void* mask_or_null, int mask_H, int mask_W, int mask_y0, int mask_x0, int32_t* inf_flag,
                                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Live measurement for bench.py's roofline line: when enabled, every conv/linear, attention and
 * GroupNorm-statistics launch is bracketed by two HIP events recorded on the launch stream.
 * ldiff_prof_collect waits for them and returns one row per kernel (time, launches, algorithmic flops/bytes).
 * Two events per launch cost ~6 % of a sampler step when every launch carries them, so ldiff_prof_set_filter(name)
 * restricts the brackets to launches of ONE kernel (exact row name, e.g. "conv3x3<8x16,128,gn>"; NULL = all):
 * bench.py profiles every kernel in an untimed warm-up step and only the dominant one inside the timed region.
 * ---------------------------------------------------------------------------------------------- */
typedef struct { char name[64]; int64_t launches; double ms, flops, bytes; } ldiff_prof_row;
int ldiff_prof_enable(int on);
int ldiff_prof_set_filter(const char* kernel_name_or_null);
int ldiff_prof_collect(ldiff_prof_row* rows, int cap); /* returns the number of rows (may exceed cap) or <0 */

/* ------------------------------------------------------------------------------------------------
 * CU-restricted streams (measurement of chip partitioning between the UNet / encoder stream and the
 * decode side stream; no reference counterpart).  A stream made here only runs on the CUs whose index
 * modulo 32 lies in [lo32, hi32) (both multiples of 8): every XCD keeps the same share of its CUs.
 * ldiff_vae_set_side_cu_share re-creates the VAE's decode side stream with such a share (0, 32 = whole chip).
 * ---------------------------------------------------------------------------------------------- */
int ldiff_stream_create_cu_share(int lo32, int hi32, void** stream_out);
int ldiff_stream_destroy(void* stream);
int ldiff_vae_set_side_cu_share(ldiff_vae* v, int lo32, int hi32);

#ifdef __cplusplus
}
#endif
#endif /* LDIFF_H */
