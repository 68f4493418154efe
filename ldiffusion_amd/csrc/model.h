// Host-side executors: weight store, op helpers over the device arena, UNet / VAE graphs.
// Internal to libldiff_hip.so.
#pragma once
#include <array>
#include <cmath>
#include <functional>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ldiff.h"
#include "common.h"

static inline int roundup(int x, int m) { return (x + m - 1) / m * m; }

// NHWC fp16 activation (tokens [M, C] are B=1,H=1,W=M or keep the image shape).  A SPLIT activation stores every row as
// [hi(C) | lo(C)] with value = hi + lo (~22 significant bits): the residual stream is kept this way so that
// the reference's fp32 residual adds survive ~40 chained blocks; plain consumers read the hi half with row pitch 2C, split
// consumers (the contractions that carry the whole stream: shortcut / proj_in / proj_out / resampling convs) read all 2C
// channels against weights duplicated along K.
struct Act {
  f16* p = nullptr;
  int B = 0, H = 0, W = 0, C = 0;
  bool split = false;
  bool lo8 = false;      // split with an fp8 lo half: a row is [C fp16 | C e4m3 of lo * 2^LO8_SHIFT] = 3C bytes (ConvParams::lo8_slab0); conv operands only
  float* st = nullptr;   // producer-fused GroupNorm partial statistics [B][st_R][C][2] (nullptr: none)
  int st_R = 0;
  bool borrowed = false; // lives in ANOTHER executor's arena (a skip tensor written by an attached ControlNet's zero conv): Exec::release leaves it alone,
                         // that arena's next reset reclaims it
  long long rows() const { return (long long)B * H * W; }
  int ld() const { return lo8 ? C + C / 2 : (split ? 2 * C : C); }       // row pitch in elements
  int lo() const { return split ? C : 0; }           // offset of the lo half inside a row
  size_t bytes() const { return (size_t)rows() * ld() * sizeof(f16); }
  SrcView view() const { return SrcView{p, C, ld(), lo()}; }
};

// One lazily built buffer derived from a checkpoint matrix: the pointer, the checkpoint generation and the key it was last built with (Exec::derived).
struct Derived { void* p = nullptr; int gen = -1; int key = 0; };

struct MatW {   // [Nrows][K] fp16 K-major + fp32 bias
  f16* w = nullptr;
  float* b = nullptr;  // nullptr => no bias
  int N = 0, Nrows = 0, K = 0, ks = 1, Cin = 0;  // Cin = padded input channels (K = ks*ks*Cin)
  bool geglu = false;   // rows stored x/gate-interleaved by 16 so that the GEMM epilogue can apply x * gelu(gate) (ConvParams::geglu)
  int Cin_logical = 0;            // unpadded input channels of a first-layer conv (Cin padded to 8): the split form keeps hi | lo inside the pad
  // Derived weights: every one a slot of Exec::derived, built on first use by the Exec that needs it, rebuilt when the checkpoint is reloaded or its key
  // changes.  A copy built from another derived copy takes its source's key, so it is rebuilt whenever the source is.  Per slot: what it holds <- what it is
  // built from; key.  (The recipes of par, dup_par, frag, frag_par, frag_sc, bias_sc, gfrag and gfrag_dup are conv_route.hip's, shared with ldiff_op_conv.)
  mutable Derived dup;        // split operand [Nrows][taps][2*Cin], the same weights against the hi and the lo half <- w; key = C1 of a concat
  mutable Derived lo8;        // split operand with an fp8 lo half [Nrows][taps][Cin fp16 | Cin e4m3] + one int behind it (the E8M0 scale operand) <- w; no key
  mutable Derived tiled;      // panel-tiled copy for the LayerNorm-fused GEMM (kernels_gemm_ast.hip) <- w; no key
  mutable Derived b_shift;    // the bias times 2^-k for a launch whose input is the range-shifted stream <- b; key = k
  mutable Derived par;        // upsampler convs: parity weights [4][Nrows][4*Cin] <- w; no key
  mutable Derived dup_par;    // ... of the duplicated matrix <- dup; key = dup's
  mutable Derived frag;       // MFMA-fragment-packed copy for the dataflow conv3x3 kernel (kernels_conv3x3d.hip) <- the matrix the launch reads (w / dup); key = dup's or 0
  mutable Derived frag_par;   // ... of the parity weights (upsampling convs on the dataflow kernel) <- par / dup_par; key = theirs
  mutable Derived frag_sc;    // ... with a folded shortcut's weights behind the nine taps <- w and the shortcut's matrix; key = that matrix's address bits and width
  mutable Derived bias_sc;    // the bias plus that shortcut's <- b and the shortcut's bias; key = frag_sc's
  mutable Derived gfrag;      // MFMA-fragment-packed copy for the dataflow GEMM (kernels_gemm_df.hip) <- w; no key
  mutable Derived gfrag_dup;  // ... of the duplicated matrix <- dup; key = dup's
};
struct NormW { float* g = nullptr; float* b = nullptr; int C = 0; };
struct GNss { float* scale = nullptr; float* shift = nullptr; };

// ---- checkpoint loading (weight_store.hip) ---------------------------------------------------------------
// Every handle family owns one WeightStore.  At build() the owner registers each checkpoint tensor it expects as a LoadSpec: the torch shape, where the
// values land and in which layout.  *_load then is WeightStore::load: one name / alias lookup, the dtype check (LDIFF_F32 / F16 / BF16), the shape check,
// the repack on the host, the copy, `loaded` and ++generation (what derived weights and captured graphs are keyed by).
//
// Kinds:
//   MATRIX  fp16 rows [row][tap][Cin_pad] at a row offset of a K-major device matrix (a conv or linear weight; several checkpoint tensors may fill one
//           matrix: fused q / k / v).  Flags: geglu_half (GEGLU row interleave), tconv (transposed conv, [tap][Cout][Cin]), rows3 (the text encoder's
//           three-block rows [wh(K) | wh(K) | wl(K)], wh = f16(w), wl = f16(w - wh)).
//   TENSOR  fp32 tensor of any rank copied as is to the device (norms, biases, embedding tables, the classifier's linear head); geglu_half interleaves a bias.
//   HOST    fp32 tensor kept in a host vector of the spec until the owner takes it (fresh() / consume(): the classifier folds a conv with its BatchNorm).
// Two shape rules.  TENSOR and HOST: exact, extent by extent.  MATRIX: equal element count, equal first two extents, rank 4 or -- for a 1x1 -- rank 2:
// diffusers checkpoints store the same attention projection as [C, C] or as [C, C, 1, 1] depending on their age, and both must load.
// The wait rule: a load that overwrites a tensor that was loaded before waits for the device (hipDeviceSynchronize) before its device write, since a
// forward enqueued earlier may still read it; a first load does not wait, nothing can have read that memory.  (HOST tensors reach the device in the
// owner's own step, which waits itself.)
// missing() lists the tensors not loaded yet in registration order; missing_name(i) indexes the list of the last missing() call.
// Errors are reported under `who` ("unet_load"-style prefix of the messages), set by the owner at build().
struct LoadSpec {
  enum Kind { MATRIX, TENSOR, HOST } kind = TENSOR;
  std::vector<int64_t> shape;   // expected torch shape
  f16* mat = nullptr; int row_off = 0, K = 0, ks = 1, Cin_pad = 0;   // MATRIX
  float* vec = nullptr; int vec_off = 0;                             // TENSOR
  std::vector<float> host; bool fresh = false;                       // HOST: the values, and whether they were loaded since the owner last consumed them
  bool tconv = false;   // MATRIX of a transposed conv (torch [Cin, Cout, k, k]): element (c, n, tap) lands at row tap * Nrows_t + n, column c
  int tconv_rows = 0;
  bool rows3 = false;   // MATRIX of the text encoder: row r of [rows, K] lands as [wh | wh | wl] at row row_off + r of a matrix of pitch 3 K
  int geglu_half = 0;   // > 0: GEGLU projection of width 2*geglu_half: row r lands at geglu_row(r) (x / gate interleaved by 16 rows)
  bool loaded = false;
};

// The repacks: torch layout, dtype LDIFF_F32 / F16 / BF16 -> device layout, on the host, every element of dst written (pads zero).  No HIP call.
void repack_rows(const void* src, int dtype, int rows, int Cin, int taps, int Cin_pad, int K, int geglu_half, f16* dst);   // [rows, Cin, taps] -> [rows][K], K >= taps * Cin_pad
void repack_tconv(const void* src, int dtype, int Cin, int Cout, int taps, int rows_t, int K, f16* dst);                   // [Cin, Cout, taps] -> [taps][rows_t][K]
void repack_f32(const void* src, int dtype, size_t n, int geglu_half, float* dst);                                         // n values as they are
void repack_rows3(const void* src, int dtype, int rows, int K, f16* dst);                                                  // [rows, K] -> [rows][3 K]

class WeightStore {
 public:
  ~WeightStore();
  const char* who = "load";
  // allocation helpers (device memory owned by the store, zero-initialised)
  f16* alloc_mat(int Nrows, int K);
  float* alloc_vec(size_t n);
  // registration
  MatW add_conv(const std::string& prefix, int Cin, int Cout, int ks, bool bias = true, int Cin_pad = -1, int min_rows = 0, bool geglu = false);
  void add_rows(const std::string& wname, const std::string& bname, f16* mat, int K, int ks, int Cin, int Cin_pad, int row_off, int rows,
                float* bias_vec, bool has_bias);
  void add_rows3(const std::string& wname, const std::string& bname, f16* mat, int K, int row_off, int rows, float* bias_vec);   // three-block rows + their bias
  NormW add_norm(const std::string& prefix, int C);
  MatW add_tconv(const std::string& prefix, int Cin, int Cout, int k);   // ConvTranspose2d with kernel = stride = k: [k*k][Cout][Cin] fp16 + bias (kernels_seg.hip)
  void add_tensor(const std::string& name, std::vector<int64_t> shape, float* dst, int off = 0);
  void add_host(const std::string& name, std::vector<int64_t> shape);
  void alias(const std::string& alias_name, const std::string& name);
  // loading
  void check_tensor(const char* name, const void* host, int dtype, const int64_t* shape, int ndim) const;   // null arguments, dtype: load()'s first step
  void load(const char* name, const void* host, int dtype, const int64_t* shape, int ndim);
  int missing() const;
  const char* missing_name(int i) const;
  int generation = 0;   // bumped by every load(): derived weights are rebuilt when it changes
  // HOST tensors
  bool loaded(const std::string& name) const;
  const std::vector<float>* fresh(const std::string& name) const;   // the values if loaded since the last consume(), else nullptr
  void consume(const std::string& name);                            // the owner has taken them: the host copy goes
  int n_fresh() const { return n_fresh_; }

 private:
  void* alloc_zeroed(size_t bytes);
  LoadSpec& add(const std::string& name, LoadSpec::Kind kind, std::vector<int64_t> shape);
  std::unordered_map<std::string, LoadSpec> specs_;
  std::unordered_map<std::string, std::string> alias_;
  std::vector<std::string> order_;
  std::vector<void*> allocs_;
  mutable std::vector<std::string> missing_cache_;
  int n_fresh_ = 0;
};

// Sticky non-finite detector of a handle (include/ldiff.h "Non-finite detection").  One int per graph in host-mapped pinned memory: the device sets it
// (a plain store of 1 from a GroupNorm finalize workgroup whose totals are not finite), the host reads it without a device round trip.
struct NonFiniteFlag {
  int* words = nullptr;   // [4], host pointer == device pointer (hipHostMallocMapped under unified addressing)
  void create();
  void destroy();
  bool test_and_clear();  // true if any word was set (only meaningful for work that has completed)
};

struct ConvOpts {
  int stride = 1, pad_t = -1 /* -1 => (ks-1)/2 */, pad_l = -1, ups = 0;
  int Hout = -1, Wout = -1;     // override output size (asymmetric-pad downsample)
  const GNss* gn = nullptr; int silu = 0;
  bool splitk_per_image = false; // plan the K split from ONE image of the batch (the nnU-Net head: a batch then computes bit for bit what its images compute alone)
  int seg_conv = 0;              // ConvParams::seg_conv (the nnU-Net head's first conv asks for the narrow kernel without a prologue)
  int lrelu = 0;                 // with gn: LeakyReLU(0.01) behind the affine instead of SiLU, bit 0 = on x, bit 1 = on x2 (ConvParams::lrelu_in: the nnU-Net head)
  const float* temb = nullptr; int ld_temb = 0;
  const Act* res = nullptr;      // residual operand (plain or split)
  bool split_in = false;         // consume the (split) sources as a split operand: K doubled, duplicated weights
  bool split_out = false;        // write the output as a split activation
  void* out_f32 = nullptr; int ldy_f32 = 0;   // write fp32 [M, ldy] here instead of allocating an fp16 Act
  int N_override = 0;           // columns to store (multiple of 4), default = roundup4(w.N)
  int ldy = 0;                  // fp16 output channel stride (default N stored rounded up to 8)
  bool want_stats = false;      // also emit GroupNorm partial statistics of the output (consumed by Exec::gn)
  bool silu_out = false;        // SiLU behind the sum: ConvParams::silu_out where the conditioning-embedding kernel takes the launch (cond_conv_selected), else a SiLU launch of its own
  bool geglu = false;           // apply x * gelu(gate) in the epilogue (weights must be MatW::geglu); output has N/2 channels
  // decode_latents tail in the epilogue (VAE conv_out): applied iff the narrow-output kernel takes the launch; *post_done says whether it did
  float* post_img = nullptr; uint8_t* post_rgb = nullptr; uint8_t* post_luma = nullptr; int post_slots = 0, post_slot = 0; bool post_only = false;
  bool* post_done = nullptr;
  // the block's 1x1 conv_shortcut folded into this (its second) conv where the dataflow conv3x3 kernel takes the launch (ConvParams::xs): sc_x = the block's
  // input, sc_w = the shortcut's weights; *sc_done says whether the fold happened (else the caller runs the shortcut conv and passes its output as res)
  const Act* sc_x = nullptr; const struct MatW* sc_w = nullptr; bool* sc_done = nullptr;
  // range shift (ldiff_vae_set_range_shift, DESIGN.md section 3 "Range"): out_shift = k: y = (sum + bias) * 2^-k + res (ConvParams::out_shift), for a
  // launch whose output joins the shifted stream from a normalised / true-scale input; bias_shift = k: the bias times 2^-k, for a launch whose input IS
  // the shifted stream (its sum is shifted already)
  int out_shift = 0, bias_shift = 0;
  // under a plan batch (Exec::plan_batch): the rows of this launch ARE the batch (a [1, 1, rows, C] tensor: the time-embedding MLP has one row per image),
  // and plan_rows is their number at the plan batch.  0: an image-shaped tensor, whose nominal launch has plan_batch images of Hout x Wout rows
  int plan_rows = 0;
};

class Exec {
 public:
  Arena arena;
  hipStream_t s = nullptr;
  float* gn_partial = nullptr;
  size_t gn_partial_cap = 0;
  std::vector<void*> owned;   // the buffers of the derived-weight slots this Exec has built (Exec::derived), freed with it
  const int* weights_gen = nullptr;   // -> WeightStore::generation of the owning model
  bool short_runs = false;            // this graph runs beside another stream's (ConvParams::short_runs)
  int* nonfinite = nullptr;           // -> the owning handle's sticky non-finite flag (host-mapped; set by the GroupNorm finalize kernels, NonFiniteFlag below)
  const char* trace_tag = nullptr;    // LDIFF_TRACE_ABSMAX=1: name of the graph whose stages trace() reports (diagnostic, synchronises)
  int range_shift = 0;                // k: this graph's stream is stored times 2^-k (the VAE decoder's Exec only: ldiff_vae_set_range_shift; trace() reports true magnitudes)
  int plan_batch = 0;                 // n > 0: every launch of this graph is planned as if the batch were n (ldiff_*_set_plan_batch, ConvParams::plan_B); 0: from its own batch
  void check_plan_batch(const char* who, int B) const;   // refuses B > plan_batch > 0
  void trace(const char* stage, const Act& a);   // max |value| of a stage's output to stderr when LDIFF_TRACE_ABSMAX is set; otherwise nothing
  ~Exec();
  void ensure_gn_partial(size_t bytes);
  Act new_act(int B, int H, int W, int C, bool split = false, bool lo8 = false);
  // The rule of every derived-weight slot (MatW): `bytes` of device memory on first use (owned by this Exec; zeroed where `zero`),
  // build(d.p) when the checkpoint generation or `key` differs from what the slot was last built with.  Returns d.p.
  template <typename Build> void* derived(Derived& d, size_t bytes, int key, Build&& build, bool zero = false);
  const f16* derived_dup(const MatW& w, int C1_logical, int C2_logical);
  const f16* derived_tiled(const MatW& w, int N);
  const float* derived_bias_shift(const MatW& w, int k);   // w.b times 2^-k (nullptr without a bias), rebuilt when k or the checkpoint changes
  const f16* derived_lo8(const MatW& w, const int** scale);   // fp8-lo weights of a split operand + the device int holding their E8M0 scale operand
  bool lo8_conv_ok(const MatW& w, const Act& x, bool res, bool split_out) const;   // would conv(w, norm_apply(x) with an fp8 lo half) run on the ping-pong kernel?
  Act norm_apply(const Act& x, const Act* x2, const GNss& g, bool silu, bool split_out, bool lo8 = false);
  void release(Act& a);
  template <typename T> T* tmp(size_t n) { return reinterpret_cast<T*>(arena.alloc(n * sizeof(T))); }
  GNss gn(const Act& x, const Act* x2, const NormW& w, int groups, float eps);
  void release(GNss& g);
  Act conv(const MatW& w, const Act& x, const Act* x2, const ConvOpts& o);
  Act layernorm(const Act& x, const NormW& w);
  // LayerNorm + linear (+ GEGLU) in one launch where the activation-stationary kernel takes the shape (kernels_gemm_ast.hip), else the two launches
  // qcols > 0: ask for columns [0, qcols) multiplied by qscale before the rounding; *scaled says whether the fused kernel took the launch and did it
  Act ln_linear(const MatW& w, const Act& x, const NormW& ln, bool geglu, int qcols = 0, float qscale = 1.0f, bool* scaled = nullptr);
  Act geglu(const Act& x);
  // ResnetBlock2D (UNet: with time embedding and optional skip concat; VAE: neither) under storage policy `prec`
  Act resnet(const struct ResnetW& r, const Act& x, const Act* skip, const float* temb, int ld_temb, int groups, float eps, int prec);
};

// ---- hipGraph replay of an executor's forward -----------------------------------------------------
// Growable device buffer: the staging of a captured forward's inputs and outputs.
struct DeviceBuf {
  void* p = nullptr;
  size_t cap = 0;
  ~DeviceBuf();
  void ensure(size_t bytes);   // synchronises, frees and reallocates only when it grows
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// The replay cache of one executor (the UNet, the nnU-Net head, the instance classifier).  Lifecycle of a configuration, named by the key the
// executor supplies (shape, precision, checkpoint generation, workspace capacities: whatever the launch sequence reads through a fixed address or was planned with):
//   first use    the forward runs eagerly on the caller's pointers (builds lazily derived weights, sizes the workspaces); the key is then taken again
//                from the executor, so a workspace that this pass grew does not make the next use look like a new configuration;
//   second use   the same launch sequence is captured on handle-owned staging buffers into a hipGraph and instantiated; if the capture throws, the
//                cache turns itself off and the forward stays eager (same kernels, same results);
//   from then on copy-in, hipGraphLaunch on the caller's stream, copy-out: valid for any caller pointers.
// A different key drops the graph and starts over.  Bypassed (plain eager forward) while disabled, under LDIFF_NO_GRAPH, while per-launch profiling is on and
// on a stream that is itself being captured.  Whoever destroys a graph that may still be replaying synchronises first (set_enabled(false), the *_destroy entry points).
struct GraphCache {
  using Key = std::array<long long, 16>;   // unused entries stay 0
  struct Staging { DeviceBuf* buf; size_t bytes; };
  long long replays = 0, captures = 0, nodes = 0;   // nodes: kernel launches of the captured forward
  ~GraphCache();
  void set_enabled(bool on);            // off: waits for the device and drops the graph
  bool bypass(hipStream_t s) const;     // run this forward eagerly, without touching the cache?
  // one forward through the cache.  current_key: the executor's key now; staging: the buffers `staged` and the copies use, sized before the capture;
  // eager: the forward on the caller's pointers and stream; staged(cs): the forward on the staging buffers and stream cs; copy_in / copy_out: caller <-> staging on s
  void run(hipStream_t s, const std::function<Key()>& current_key, std::initializer_list<Staging> staging, const std::function<void()>& eager,
           const std::function<void(hipStream_t)>& staged, const std::function<void()>& copy_in, const std::function<void()>& copy_out);

 private:
  bool enabled = true;
  int uses = 0;   // forwards seen with the current key (0: none, 1: ran eagerly once, 2: graph ready)
  Key key{};
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipStream_t cap_stream = nullptr;
  void drop();
};

// ---- UNet -------------------------------------------------------------------------------------
struct ResnetW { NormW n1, n2; MatW c1, c2, sc; bool has_sc = false; int temb_off = 0; int Cin = 0, Cout = 0; };
struct TransformerW {
  NormW gn, ln1, ln2, ln3;
  MatW proj_in, qkv, out1, q2, kv2, out2, ff1, ff2, proj_out;
  int C = 0;
  f16* kv_ctx = nullptr;  // [Bctx*L, 2C] precomputed by set_context
};

// Storage policy of a graph (ldiff_*_set_precision):
//   0  everything fp16 in HBM (fastest; one UNet pass ~2e-3 of the output range from the fp32 reference)
//   1  split residual stream: stream tensors hi|lo, residual adds to fp32 round-off, stream-carrying contractions on split operands
//   2  every conv / linear operand split (K doubled everywhere): ~1e-4; used for the VAE encoder, whose error every later pass inherits
enum { PREC_FAST = 0, PREC_STREAM = 1, PREC_FULL = 2 };

struct ldiff_controlnet;
struct ldiff_unet {
  ldiff_unet_cfg cfg;
  bool encoder_only = false;   // the trunk of a ControlNet: conv_in, time embedding, down blocks and mid block only (no up path, no output head)
  int device = 0;
  int precision = PREC_STREAM;
  WeightStore ws;
  Exec ex;
  MatW conv_in, conv_out, t_lin1, t_lin2, temb_proj_all;
  NormW norm_out;
  int temb_total = 0;
  std::vector<std::vector<ResnetW>> down_res, up_res;
  std::vector<std::vector<TransformerW>> down_attn, up_attn;
  std::vector<MatW> down_sample, up_sample;
  std::vector<bool> has_down, has_up;
  ResnetW mid_res[2];
  TransformerW mid_attn;
  std::vector<TransformerW*> all_tf;
  NonFiniteFlag nf;
  int ctx_B = 0, ctx_L = 0, ctx_gen = 0;
  int ctx_plan = 0;            // the plan batch the cross-attention K / V were projected under (set_context): a forward under another one is refused
  void set_plan_batch(int n) { ex.plan_batch = n; }   // (captured graphs: the plan batch is part of the replay key)
  f16* ctx_buf = nullptr; size_t ctx_cap = 0;     // all kv_ctx live in one allocation
  void build();
  void set_context(const float* ctx, int Bc, int L, hipStream_t s);
  // forward = the ~390-450 launches of one pass (384 at B = 8, 443 at B = 1 at SD-v1.5 size), through the replay cache (GraphCache above): the timestep
  // is staged like the input and the output, so a replay is valid for any timestep.
  void forward(const float* x, int B, int h, int w, float t, float* out, hipStream_t s);
  void forward_impl(const float* x, int B, int h, int w, float t, const float* t_dev, float* out, hipStream_t s);
  // The stages of a pass that a UNet and a ControlNet's trunk share, and the state they hand on: begin_pass (argument checks, workspace), run_down
  // (time embedding, conv_in -- plus `emb`, a plain [B, h, w, C0] tensor added in conv_in's epilogue: the ControlNet's conditioning embedding -- and
  // the down blocks: fills pass.skips, pass.cur = the last of them) and run_mid (the mid block: pass.cur = its output, the skips stay alive).
  struct Pass {
    int B = 0, h = 0, w = 0;
    float* temb_all = nullptr;
    std::vector<Act> skips;
    Act cur;
    bool cur_is_skip = false;
    int stage_no = 0;
  } pass;
  void begin_pass(int B, int h, int w, hipStream_t s);
  void run_down(const float* x, float t, const float* t_dev, const Act* emb);
  void run_mid();
  void advance(Act nxt);
  Act resnet(const ResnetW& r, const Act& x, const Act* skip);
  // An attached ControlNet (ldiff_unet_attach_controlnet): its blocks run inside this UNet's forward and its zero convs write skip + scale * (W cnskip + b)
  // straight into the skip stack; borrowed, the caller keeps it alive while attached
  ldiff_controlnet* cn = nullptr;
  float cn_scale = 1.0f;
  long long cn_epoch = 0;   // bumped by every attach / detach (a new scale included): part of the graph key
  // ControlNet inputs of the next forward (down_block_additional_residuals, mid_block_additional_residual: segmentor.py:366-372);
  // float32 NCHW device pointers in skip-stack order, consumed (cleared) by that forward, which then runs eagerly
  std::vector<const float*> extra_down;
  const float* extra_mid = nullptr;
  int n_skips() const;
  GraphCache gc;
  DeviceBuf st_in, st_out, st_t;   // staging of a captured forward: sample, output, timestep
  ~ldiff_unet() { nf.destroy(); }
  Act transformer(const TransformerW& t, const Act& x);
};

// ---- VAE --------------------------------------------------------------------------------------
struct VaeAttnW { NormW gn; MatW qkv, out; int C = 0; };
struct ldiff_vae {
  ldiff_vae_cfg cfg;
  int device = 0;
  int prec_enc = PREC_FULL, prec_dec = PREC_FAST;   // the decoder feeds only uint8 images / luma (never the latents): see DESIGN.md section 3
  int prec() const { return cur == &ex_enc ? prec_enc : prec_dec; }
  WeightStore ws;
  // Two workspaces: the decoder's and the encoder's.  A pipelined sampler decodes batch k on the side stream while the encoder
  // of batch k+1 already runs on the caller's stream; ex() is the one the running graph builder uses.
  Exec ex_dec, ex_enc;
  NonFiniteFlag nf;   // word 0: encoder graph, word 1: decoder graph
  ~ldiff_vae() { nf.destroy(); }
  Exec* cur = &ex_dec;
  Exec& ex() { return *cur; }
  // side stream for decodes that only feed the feature tensor (ldiff_sample); ev_side = "everything queued on it so far is done"
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_side = nullptr;
  bool side_used = false;
  void wait_side(hipStream_t s);   // make s wait for the side stream's queued work (no-op if it was never used)
  // encoder
  MatW e_conv_in, e_conv_out, quant;
  std::vector<std::vector<ResnetW>> e_res;
  std::vector<MatW> e_down;
  ResnetW e_mid[2]; VaeAttnW e_attn; NormW e_norm_out;
  // decoder
  MatW post_quant, d_conv_in, d_conv_out;
  std::vector<std::vector<ResnetW>> d_res;
  std::vector<MatW> d_up;
  ResnetW d_mid[2]; VaeAttnW d_attn; NormW d_norm_out;
  void build();
  void encode(const float* x, int B, int H, int W, float* moments, hipStream_t s);
  // writes the fp32 NHWC decoder output [B*8h*8w, 4] into the arena and post-processes it
  void decode(const float* z, int B, int h, int w, float z_scale, float* sample_nchw, float* image_nhwc, uint8_t* rgb, uint8_t* luma,
              int n_slots, int slot, hipStream_t s);
  Act mid_attention(const VaeAttnW& a, const Act& x);
  // decoder range shift k (0..16): the decoder's residual stream and every conv output that feeds a GroupNorm are stored times 2^-k, its GroupNorms
  // use eps * 4^-k (DESIGN.md section 3 "Range").  No captured graph holds decoder launches, so nothing is invalidated; the pre-scaled biases are
  // rebuilt on their next use (Exec::derived_bias_shift)
  void set_range_shift(int k) { ex_dec.range_shift = k; }
  void set_plan_batch(int n) { ex_dec.plan_batch = ex_enc.plan_batch = n; }   // (no captured graph holds VAE launches)
  float dec_eps() const { return ldexpf(1e-6f, -2 * ex_dec.range_shift); }
};

// ---- ControlNet ---------------------------------------------------------------------------------
// diffusers ControlNetModel: a conditioning embedding (eight 3x3 convs, SiLU between them) whose output joins conv_in's, the UNet's down blocks and
// mid block on that (the trunk: an encoder-only ldiff_unet, same builders and executors), and a 1x1 "zero conv" behind every skip tensor and the mid block.
struct ldiff_controlnet {
  ldiff_unet trunk;
  int cond_channels = 3;
  std::vector<int> emb_ch;
  MatW e_conv_in, e_conv_out;
  std::vector<MatW> e_blocks;
  std::vector<MatW> zc;        // controlnet_down_blocks.i, then controlnet_mid_block: as loaded
  std::vector<MatW> zs;        // the same times conditioning_scale (weights and bias), what the launches read; rebuilt when the scale or the checkpoint changes
  float zs_scale = 0.f;
  int zs_gen = -1;
  long long state_gen = 0;     // bumped by whatever a captured graph that holds this network's launches must not outlive
  Exec ex_emb;                 // the embedding's executor (its own workspace: the map is eight times the latent size per side)
  f16* emb = nullptr;          // conditioning embedding [emb_B, emb_h, emb_w, C0] fp16, kept between set_cond calls
  size_t emb_cap = 0;
  int emb_B = 0, emb_h = 0, emb_w = 0;
  void build();
  void set_cond(const float* cond, int B, int H, int W, hipStream_t s);
  void ensure_scaled(float scale, hipStream_t s);
  void set_plan_batch(int n);   // trunk and embedding; a change drops the kept embedding (set_cond again) and whatever graph holds this network's launches
  // the trunk's pass: fills trunk.pass (skips, cur = the mid block's output); the tensors stay valid until the trunk's next pass
  void run_trunk(const float* x, int B, int h, int w, float t, const float* t_dev, hipStream_t s);
  void forward(const float* x, int B, int h, int w, float t, float scale, float* const* down_out, int n_down, float* mid_out, hipStream_t s);
  ~ldiff_controlnet();
};

// ---- nnU-Net tissue head ---------------------------------------------------------------------------
// PlainConvUNet (2-D) as get_network_from_plans builds it (include/ldiff.h).  Every conv's output is stored raw (before its InstanceNorm) with fused
// per-channel partial sums; in_finalize turns them into scale / shift; the consumer applies affine + LeakyReLU in its prologue.
struct SegConvW { MatW conv; NormW norm; };
struct ldiff_segnet {
  int device = 0;
  int in_ch = 0, n_stages = 0, n_heads = 0;
  std::vector<int> features, strides, nce, ncd;
  WeightStore ws;
  Exec ex;
  NonFiniteFlag nf;
  std::vector<std::vector<SegConvW>> enc, dec;
  std::vector<MatW> up;
  MatW head;
  void build();
  void forward(const float* x, int B, int H, int W, void* out, int out_dtype, hipStream_t s);
  void forward_impl(const float* x, int B, int H, int W, void* out, int out_dtype, hipStream_t s);
  // scale / shift [B, ident + a.C] of InstanceNorm over `a` (the leading `ident` channels: identity, for the upsampled half of a decoder concat)
  GNss in_ss(const Act& a, const NormW& w, int ident);
  GraphCache gc;
  DeviceBuf st_in, st_out;
  ~ldiff_segnet() { nf.destroy(); }
};

// ---- instance classifier of the cell head -------------------------------------------------------------
// torchvision's ResNet (v1.5 bottlenecks) + adapter conv + linear head (include/ldiff.h).  The checkpoint's conv and BatchNorm tensors stay on the host (LoadSpec::HOST); a conv and its
// BatchNorm are folded there in double (fold()) into one fp16 K-major matrix + fp32 bias, so every conv is one clsconv launch (kernels_cls.hip).
struct ClsConvW {
  std::string conv, bn;          // checkpoint prefixes; bn empty: the conv has its own bias (the adapter)
  int Cin = 0, Cout = 0, ks = 1, stride = 1;
  int Cin_pad = 0;               // stored input channels (the stem's 3 padded to 8 with zero weights)
  f16* w = nullptr;              // [Cout][ks ks Cin_pad]
  float* b = nullptr;            // [Cout]
  bool folded = false;
  // training mode (ldiff_resnet::set_train): the UN-folded matrix (one rounding of w, the layout of `w`), the BatchNorm's gamma / beta, its offset on the flat channel axis
  f16* w_raw = nullptr;
  float* gamma = nullptr; float* beta = nullptr;
  long long bn_off = -1;
};
struct ClsBnOut { Act raw; float* scale = nullptr; float* shift = nullptr; };   // a conv's raw sums and the scale / shift its batch statistics give (forward_train)
struct ClsBlockW { int c1 = -1, c2 = -1, c3 = -1, down = -1; };   // indices into ldiff_resnet::convs
struct ldiff_resnet {
  int device = 0;
  int layers[4] = {0, 0, 0, 0}, width = 0, adapter_ch = 0, n_classes = 0;
  std::vector<ClsConvW> convs;
  int stem = -1, adapter = -1;
  std::vector<ClsBlockW> blocks;
  float* fc_w = nullptr; float* fc_b = nullptr;   // [n_classes][adapter_ch], [n_classes] fp32
  WeightStore ws;   // the conv / BatchNorm tensors as HOST specs (fold() takes them), the linear head as TENSORs
  Exec ex;
  NonFiniteFlag nf;
  void build();
  void load(const char* name, const void* host, int dtype, const int64_t* shape, int ndim);
  void fold();                     // every group whose tensors are all freshly loaded -> device (synchronous copies: never inside a capture)
  Act conv(const ClsConvW& c, const Act& x, const Act* res, bool relu);
  void forward(const f16* crops, int B, int S, float* logits, int* labels, hipStream_t s);
  void forward_impl(const f16* crops, int B, int S, float* logits, int* labels, hipStream_t s);
  // training mode (include/ldiff.h ldiff_resnet_set_train / _forward_train): batch statistics, three launches per conv, eager
  bool train = false;
  long long bn_total = 0;          // T: channels of all BatchNorms
  std::vector<int> bn_order;       // convs with a BatchNorm, in forward order: BatchNorm i of ldiff_resnet_bn_entry
  void set_train(bool on);
  ClsBnOut conv_bn(const ClsConvW& c, const Act& x, float* batch_stats);
  Act bn_apply(ClsBnOut& a, const Act* id_plain, ClsBnOut* id_bn, bool relu);
  void forward_train(const f16* crops, int B, int S, float* batch_stats, float* features, float* logits, int* labels, hipStream_t s);
  GraphCache gc;
  DeviceBuf st_in, st_logits, st_labels;
  ~ldiff_resnet() { nf.destroy(); }
};

// ---- CLIP text encoder ---------------------------------------------------------------------------------
// transformers' CLIPTextModel without the pooled output (include/ldiff.h): embeddings, pre-LN encoder layers with causal self-attention, final LayerNorm,
// optionally the prompt projection Linear(hidden, cross_attention_dim) behind it.  The residual stream is split (hi | lo) throughout.
// A linear layer of the text encoder: the weight as a three-block operand [Nrows][wh(K) | wh(K) | wl(K)] (wh = fp16(w), wl = fp16(w - wh)) against a split
// activation read as [hi | lo | hi] -- the sum is x.w to ~22 bits of both factors (the lo.wl term is dropped) -- and an fp32 bias.
struct TextLinW { f16* w3 = nullptr; float* b = nullptr; int N = 0, Nrows = 0, K = 0; };
struct TextLayerW { NormW ln1, ln2; TextLinW qkv, out, fc1, fc2; };
struct ldiff_textenc {
  ldiff_textenc_cfg cfg;
  int device = 0;
  WeightStore ws;
  Exec ex;
  NonFiniteFlag nf;
  float* tok = nullptr;   // [vocab][hidden] fp32
  float* pos = nullptr;   // [max_positions][hidden] fp32
  std::vector<TextLayerW> layers;
  NormW final_ln;
  TextLinW proj;          // optional: registered by the first load of proj.weight / proj.bias, which states its width
  int proj_dim = 0;
  void build();
  TextLinW add_lin(const std::string& prefix, int K, int N);
  void add_part(TextLinW& l, const std::string& prefix, int row_off, int rows);
  void load(const char* name, const void* host, int dtype, const int64_t* shape, int ndim);
  void forward(const int32_t* ids_host, int B, int L, int project, void* out, int out_dtype, hipStream_t s);
  void forward_impl(const int* ids_dev, int B, int L, int project, void* out, int out_dtype, hipStream_t s);
  // y = act(x.w^T + b) [+ res]: x split [M, 2 K]; y a plain or split fp16 tensor, or fp32 rows at out_f32
  Act linear(const TextLinW& w, const Act& x, const Act* res, bool split_out, int act_out, float* out_f32);
  Act layernorm(const Act& x, const NormW& w);   // split in, split out
  GraphCache gc;
  DeviceBuf st_ids, st_out;
  ~ldiff_textenc() { nf.destroy(); }
};

struct ldiff_pipeline {
  ldiff_unet* unet;
  ldiff_vae* vae;
  Arena arena;   // latents / eps history
  float abar[1000];
  // decode side stream: the VAE decode of pass k (needed only for the features) runs beside the UNet pass k+1
  // 0: everything on the caller's stream; 1: decodes on the VAE's side stream, the caller's stream joins before ldiff_sample
  // returns (default); 2: as 1 but the join is deferred to ldiff_pipeline_join (lets the next batch start under the decodes)
  int overlap = 1;
  bool join_pending = false;
  hipEvent_t ev_latents = nullptr, ev_decoded = nullptr;
};

void pndm_alphas_cumprod(float* out1000);
int plms_timesteps(int n_passes, int64_t* out, int cap);
