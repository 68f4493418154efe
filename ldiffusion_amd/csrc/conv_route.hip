// Which kernel takes a conv / GEMM launch, with which split, statistics row blocks, tile and weight layout (common.h plan_conv).
// Each kernel file states its own limits (conv3x3_eligible, conv3x3{n,nt,d,p}_selected, gemm_dma_eligible, gemm_df_selected); this file
// cond_conv_selected comes first: its launches are ones no other family is made for.  This file
// is the one place that asks them, in one fixed order, and the only one that reads the routing switches LDIFF_GEMM_DF and LDIFF_LO8.
// Behind plan_conv: the recipe (byte count, pack launches) of each derived weight layout a plan names, for the executors and ldiff_op_conv alike.
#include "common.h"

namespace {

long long tiles(const ConvParams& p, int bm, int bn) { return (long long)((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn); }
bool n_small(const ConvParams& p) { return p.N <= 64 || (p.N % 128 != 0 && p.N % 128 <= 64 && p.N < 512); }
int splits(long long t, int nk) { int S = (int)(512 / t); S = S > nk / 16 ? nk / 16 : S; return S > 8 ? 8 : S; }

// Split count of a launch whose tiles do not fill the chip (round 6).  What bounds such a launch is not bytes: a workgroup takes its operand slices
// (16 KiB per K-step) at ~0.95 us per step whatever the ring depth or the slice layout, from HBM and L2 alike (scripts/micro/hbm_ring.hip,
// profiles/r06_hbm_ring.txt: the same 30 MB take 22 us on 80 workgroups, 13 on 160, 10.6 on 240, 8.9 on 480), so the lever is the NUMBER of workgroups --
// against the fp32 partials a finer cut writes and the reduce launch reads.  Returns the S in [s_old, s_cap] with the shortest modelled time
//     T(S) = 4 us + ceil(steps / S) * 0.95 us * max(1, tiles S / 330)  +  [S > 1] * (4 us + 2 * S * partial_bytes / 3 TB/s)
// and s_old (the rule of rounds 2-5, which the B = 8 shapes were tuned with) unless the model sees at least 15 % less.
int splitk_by_model(long long tiles, int steps, int min_steps, double partial_bytes, int s_old, int s_cap = 16) {
  auto T = [&](int S) {
    const double wgs = (double)tiles * S, per = (steps + S - 1) / S;
    return 4.0 + per * 0.95 * (wgs > 330.0 ? wgs / 330.0 : 1.0) + (S > 1 ? 4.0 + 2.0 * S * partial_bytes / 3.0e6 : 0.0);
  };
  if (s_old < 1) s_old = 1;
  int best = s_old;
  double tb = T(s_old);
  for (int S = s_old + 1; S <= s_cap && steps / S >= min_steps; ++S)
    if (T(S) < tb) { tb = T(S); best = S; }
  return tb <= 0.85 * T(s_old) ? best : s_old;
}

// ---- halo-tile 3x3 kernels (kernels_conv3x3.hip): 8 x 16 pixel tiles where the map is at least 16 wide, else 8 x 8 ----
void c3_tile(const ConvParams& p, ConvPlan& pl) {
  pl.bm = (p.w_par ? p.Win : p.Wout) >= 16 ? 128 : 64;
  pl.bn = (p.N % 128 != 0 && p.N % 160 == 0) ? 160 : (p.N <= 32 ? 32 : (p.N <= 64 ? 64 : 128));
}
int conv3x3_splitk_plan(const ConvParams& p) {
  if (p.w_par) return 1;
  // few workgroups and a long K loop (UNet 8x8 / 16x16 levels, K = 9*1280..9*2560): split the slabs so the grid fills the chip
  ConvPlan t;
  c3_tile(p, t);
  const int wgs = p.B * ((p.Hout + 7) / 8) * ((p.Wout + t.bm / 8 - 1) / (t.bm / 8)) * ((p.N + t.bn - 1) / t.bn);
  const int nslab = (p.C1 + p.C2) / 64;
  int S = 512 / (wgs > 0 ? wgs : 1);
  if (S > nslab / 4) S = nslab / 4;
  if (S > 8) S = 8;
  if (S < 1) S = 1;
  // small grids (batch 1 / 2, and the 8 x 8 level at any batch): a finer cut where the model sees it (whole slabs: a split starts at a slab)
  if (wgs > 0 && wgs * S < 256) {
    int Sm = splitk_by_model(wgs, nslab * 9, 9, (double)p.M * p.N * 4.0, S);
    while (Sm > S && nslab / Sm < 1) --Sm;
    S = Sm;
  }
  return S;
}

// ---- LDS-DMA GEMM (kernels_gemm.hip): 1x1 convs / linears ----
// Split-K only where the tiles leave most workgroup slots empty and K is long (1x1 shortcut convs over the concat input at the 8x8 level: M = 512,
// K = 2560 or 5120 on split operands): the largest tile whose splits fill the chip (128x128: 0.0156 operand bytes per flop, 128x64: 0.023, 64x64: 0.031)
int gemm_dma_splitk_plan(const ConvParams& p) {
  if (p.geglu || p.w_bstride != 0 || p.M <= 0) return 1;
  if (tiles(p, 128, 64) >= 384) return 1;
  const int nk = p.K / 64;
  const int S256 = n_small(p) ? 1 : splits(tiles(p, 128, 128), nk);
  if (S256 >= 2 && tiles(p, 128, 128) * S256 >= 384) return S256;
  const int S128 = splits(tiles(p, 128, 64), nk);
  if (S128 >= 2 && tiles(p, 128, 64) * S128 >= 384) return S128;
  int S64 = splits(tiles(p, 64, 64), nk);
  if (S64 < 1) S64 = 1;
  // small grids (batch 1 / 2; the 8 x 8 level): a finer cut where the model sees it
  if (tiles(p, 64, 64) * S64 < 256) S64 = splitk_by_model(tiles(p, 64, 64), nk, 4, (double)p.M * p.N * 4.0, S64);
  return S64;
}
// the tile: the largest whose workgroups (tiles x S) fill the chip
void gemm_dma_tile(const ConvParams& p, int S, ConvPlan& pl) {
  const bool bm128_ok = p.w_bstride == 0 || (p.Hout * p.Wout) % 128 == 0;   // per-image weights: 128-row tiles only if they divide an image
  if (!n_small(p) && bm128_ok && tiles(p, 128, 128) * S >= 384) pl.bm = 128, pl.bn = 128;
  else if (bm128_ok && tiles(p, 128, 64) * S >= 384) pl.bm = 128, pl.bn = 64;
  else pl.bm = 64, pl.bn = 64;
}

// ---- register-staged implicit GEMM (kernels_igemm.hip): everything else (stride-2 convs, GroupNorm prologues in front of 1x1 convs, ...) ----
// Split-K only where the 64x64 tiles leave most workgroup slots empty and the K loop is long (stride-2 3x3 convs of the UNet's 16x16 -> 8x8
// level: 160 tiles x 180-360 K-steps); 128x64 tiles (half the operand bytes per flop of 64x64) when their splits fill the chip
int igemm_splitk_plan(const ConvParams& p) {
  if (p.geglu || p.M <= 0) return 1;
  if (tiles(p, 128, 64) >= 384) return 1;
  const int nk = (p.K + 63) / 64;
  const int S128 = splits(tiles(p, 128, 64), nk);
  if (S128 >= 2 && tiles(p, 128, 64) * S128 >= 384) return S128;
  return splits(tiles(p, 64, 64), nk);
}
// the tile: the largest that still yields >= ~2 workgroups per CU worth of tiles (x S); narrow N gets BN = 64
void igemm_tile(const ConvParams& p, int S, ConvPlan& pl) {
  if (!n_small(p) && S == 1 && tiles(p, 128, 128) >= 384) pl.bm = 128, pl.bn = 128;
  else if (tiles(p, 128, 64) * S >= 384) pl.bm = 128, pl.bn = 64;
  else pl.bm = 64, pl.bn = 64;
}

float placeholder[1];   // stands in for a buffer the caller provides once the plan names it: the predicates read those as null / non-null only

}  // namespace

// LDIFF_LO8: 1 (default) = the lo half of a split conv operand travels as fp8 where the 16 x 16 ping-pong kernel takes it (Exec::lo8_conv_ok),
// 0 = fp16 lo halves everywhere
bool conv_lo8_enabled() {
  static const int mode = [] { const char* e = getenv("LDIFF_LO8"); return e ? atoi(e) : 1; }();
  return mode != 0;
}

ConvPlan plan_conv(ConvParams& p, const ConvAsk& ask) {
  ConvPlan pl;
  LDIFF_CHECK(p.out_shift >= 0 && p.out_shift <= 16, LDIFF_ERR_INVALID, "conv: range shift %d outside 0..16", p.out_shift);
  LDIFF_CHECK(p.plan_B >= 0 && (p.plan_B == 0 || (p.B <= p.plan_B && p.M <= p.plan_M)), LDIFF_ERR_INVALID,
              "conv: a launch of batch %d (%d rows) under a plan batch of %d (%d rows): the plan batch is the largest batch a handle takes", p.B, p.M, p.plan_B, p.plan_M);
  // the launch as the predicates see it: under a plan batch the nominal one, so that kernel, split, tile and layout do not depend on the batch the images travel in
  // (what comes back -- splitk, stats_R, the fold strides -- is per image or per K, never per batch)
  ConvParams q = nominal_launch(p);
  // LDIFF_GEMM_DF: 0 = no dataflow GEMM, 1 (default) = where its unit list fills the chip, 2 = every launch it takes (tests, A/B timing);
  // a launch's own ConvParams::df_force comes first
  static const int df_mode = [] { const char* e = getenv("LDIFF_GEMM_DF"); return e ? atoi(e) : 1; }();
  if (q.df_force == 0 && (df_mode == 0 || df_mode == 2)) q.df_force = df_mode == 0 ? -1 : 1;

  // A ReLU behind the sum exists in ONE family (0c below): asked for together with what selects another family it is refused here, before any of them can take the
  // launch and drop it
  LDIFF_CHECK(!q.relu_out || !(q.silu_out || q.cond_force > 0 || q.tconv || q.lrelu_in || q.seg_conv > 0), LDIFF_ERR_INVALID,
              "conv: relu_out cannot be combined with silu_out / cond_conv = 1 / tconv / lrelu_in / seg_conv = 1 (only the classifier's conv family has a ReLU epilogue)");
  // likewise quick_gelu / gelu behind the sum (act_out, 0d below): nothing that selects one of the families in front of it
  LDIFF_CHECK(!q.act_out || !(q.relu_out || q.cls_force > 0 || q.silu_out || q.cond_force > 0 || q.tconv || q.lrelu_in || q.seg_conv > 0), LDIFF_ERR_INVALID,
              "conv: act_out cannot be combined with relu_out / cls_conv = 1 / silu_out / cond_conv = 1 / tconv / lrelu_in / seg_conv = 1 (only the LDS-DMA GEMM has that epilogue)");
  // Training-mode BatchNorm partials (ConvParams::bn_stats) exist in the classifier's conv family alone, asked for by name: the launch is that family's raw form or it is refused
  if (q.bn_stats) {
    LDIFF_CHECK(ask.splitk < 2 && !ask.stats && cls_conv_bn_ok(q), LDIFF_ERR_INVALID,
                "conv: bn_stats needs cls_conv = 1 and a launch the classifier's conv family takes, without bias, residual, ReLU, split-K or `stats` (Cin=%d N=%d ks=%d stride=%d cls_conv=%d)",
                q.C1 + q.C2, q.N, q.ks, q.stride, q.cls_force);
    pl.kernel = ConvKernel::CLSCONV;
    p.splitk = 0;
    p.stats_R = 0;
    return pl;
  }
  // 0. the conditioning-embedding 3x3 (kernels_cond.hip): channel counts no other family is made for; no split, no fused statistics (the caller's
  //    separate statistics pass), plain weights.  It is the one kernel with an activation behind its sum
  if (ask.splitk < 2 && cond_conv_selected(q)) {
    pl.kernel = ConvKernel::COND;
    p.splitk = 0;
    p.stats_R = 0;
    return pl;
  }
  // 0b. the nnU-Net head's launches (ConvParams::lrelu_in / tconv): the 2x2 transposed conv has a kernel of its own (kernels_seg.hip); a conv with the
  //     LeakyReLU prologue runs on the halo-tile 3x3 kernels where the launch is theirs (64-channel multiples, stride 1: conv3x3_lrelu<...>), else on the
  //     register-staged implicit GEMM (igemm_lrelu<...>)
  LDIFF_CHECK(!q.lrelu_in || (q.gn_scale && q.gn_shift && !q.silu_in && (q.lrelu_in & ~3) == 0), LDIFF_ERR_INVALID, "conv: lrelu_in = %d needs gn_scale / gn_shift, silu_in = 0 and bits 0..1 only", q.lrelu_in);
  if (q.tconv) {
    LDIFF_CHECK(q.tconv == 1 && q.ks == 2 && q.stride == 2 && !q.ups && !q.x2 && q.C2 == 0 && q.C1 % 8 == 0 && q.Hout == 2 * q.Hin && q.Wout == 2 * q.Win && q.N == q.Nrows && q.N % 16 == 0 &&
                    q.K == q.C1 && !q.res && !q.temb && !q.out_f32 && !q.y_lo && !q.geglu && !q.silu_in && !q.silu_out && !q.out_shift && !q.xs && !q.lo8_slab0 && ask.splitk < 2 && !ask.stats &&
                    q.ldy >= q.N && q.ldy % 4 == 0 && (q.ld1 == 0 || (q.ld1 >= q.C1 && q.ld1 % 8 == 0)) && (long long)q.B * q.Hin * q.Win == q.M / 4 && q.M % 4 == 0,
                LDIFF_ERR_INVALID, "conv: tconv takes kernel = stride = 2, one source with C1 %% 8 == 0, N == Nrows, N %% 16 == 0, Hout = 2 Hin, a plain fp16 output and bias only (C1=%d N=%d Nrows=%d ks=%d stride=%d)",
                q.C1, q.N, q.Nrows, q.ks, q.stride);
    pl.kernel = ConvKernel::TCONV;
    p.splitk = 0;
    p.stats_R = 0;
    return pl;
  }
  if (ask.splitk < 2 && segconv_selected(q)) {   // the narrow 3x3 convs of the head's full- and half-resolution stages; statistics per wave (one row block each)
    pl.kernel = ConvKernel::SEGCONV;
    p.splitk = 0;
    p.stats_R = ask.stats ? segconv_stats_blocks(q) : 0;
    return pl;
  }
  // 0c. the instance classifier's convs (kernels_cls.hip): the one family with a ReLU behind its sum, and the only one with 7x7 taps; no split (the K order of a sum
  //     never depends on the batch), no fused statistics, plain weights
  if (ask.splitk < 2 && !ask.stats && cls_conv_selected(q)) {
    pl.kernel = ConvKernel::CLSCONV;
    p.splitk = 0;
    p.stats_R = 0;
    return pl;
  }
  LDIFF_CHECK(!q.relu_out && q.ks != 7, LDIFF_ERR_INVALID, "conv: a ReLU epilogue (relu_out) and 7x7 taps exist only in the classifier's conv family, which does not take this launch (Cin=%d N=%d ks=%d stride=%d pad=%d cls_conv=%d)",
              q.C1 + q.C2, q.N, q.ks, q.stride, q.pad_t, q.cls_force);
  LDIFF_CHECK(!q.silu_out, LDIFF_ERR_INVALID, "conv: a SiLU epilogue (silu_out) exists only in the conditioning-embedding kernel, which does not take this launch (Cin=%d N=%d ks=%d stride=%d)",
              q.C1 + q.C2, q.N, q.ks, q.stride);
  // 0d. quick_gelu / gelu behind the sum (ConvParams::act_out, the text encoder's FC1): the LDS-DMA GEMM has it, unsplit, with an fp16 output (plain or split: y_lo); the launch is
  //     that kernel's or it is refused -- the dataflow GEMM, the split reduce and the implicit GEMM have no such epilogue
  if (q.act_out) {
    LDIFF_CHECK((q.act_out == 1 || q.act_out == 2) && !q.geglu && !q.res && !q.out_f32 && !q.out_shift && !q.gn_scale && !q.temb && !ask.stats && ask.splitk < 2 && q.w_bstride == 0 &&
                    !q.xs && !q.lo8_slab0 && p.df_force <= 0 && gemm_dma_eligible(q),   // (p.df_force: what the launch itself asks for, not LDIFF_GEMM_DF)
                LDIFF_ERR_INVALID, "conv: act_out = %d (1 quick_gelu | 2 gelu) exists only in the LDS-DMA GEMM: a linear layer (ks = 1, K %% 64 == 0) with bias and an fp16 output (plain or split), no residual / "
                "fp32 output / GEGLU / statistics / range shift / split-K / gemm_df (C1=%d C2=%d N=%d ks=%d stride=%d)", q.act_out, q.C1, q.C2, q.N, q.ks, q.stride);
    pl.kernel = ConvKernel::GEMM_DMA;
    gemm_dma_tile(q, 1, pl);
    p.splitk = 0;
    p.stats_R = 0;
    return pl;
  }
  // 1. the kernel family.  GroupNorm -> 1x1 conv / Linear with no activation in between (VAE attention q/k/v; transformer proj_in under PREC_FAST):
  //    the normalisation folded into per-image weights and bias where the plain LDS-DMA GEMM takes that form, instead of the register-staged GN prologue
  if (ask.fold_gn && q.gn_scale && !q.silu_in && !q.lrelu_in && q.ks == 1 && !q.x2 && !q.out_f32 && !q.geglu) {
    ConvParams f = q;
    f.gn_scale = nullptr; f.gn_shift = nullptr;
    f.w_bstride = (long long)q.Nrows * q.K; f.bias_bstride = q.Nrows;
    if (gemm_dma_eligible(f)) { q = f; pl.fold_gn = true; }
  }
  const bool c3 = conv3x3_eligible(q) && !(q.lrelu_in && q.ups), gemm = !c3 && !q.lrelu_in && gemm_dma_eligible(q);   // (LeakyReLU prologue: the halo-tile 3x3 kernels and the implicit GEMM have it)
  // 2. nearest-2x upsample + conv3x3 folded algebraically: four 2x2 convs with pre-summed taps (ConvParams::w_par)
  pl.parity = q.ups && c3;
  if (pl.parity) q.w_par = reinterpret_cast<const f16*>(placeholder);
  // 3. split-K: blockIdx.y owns a range of K-steps, the reduce kernel (launch_splitk_reduce) applies the epilogue
  if (ask.splitk >= 2) {
    LDIFF_CHECK(ask.splitk <= (c3 ? (q.C1 + q.C2) / 64 : (q.K + 63) / 64), LDIFF_ERR_INVALID, "conv: more splits than K steps (%d)", ask.splitk);
    q.splitk = ask.splitk;
  } else if (ask.splitk == 0 && !q.out_f32) {
    q.splitk = c3 ? conv3x3_splitk_plan(q) : gemm ? gemm_dma_splitk_plan(q) : igemm_splitk_plan(q);
  }
  if (q.splitk < 2) q.splitk = 0;
  // 4. fused GroupNorm statistics (common.h).  A split launch's reduce kernel and the GEMM kernels emit them in 32-row blocks, which must not
  //    straddle two images; every 3x3 kernel that takes an unsplit launch emits them in its own tile rows (step 5)
  const int hw = q.Hout * q.Wout;
  const bool rows32 = q.splitk > 1 || !c3;
  q.stats = nullptr; q.stats_R = 0;
  if (ask.stats && !q.out_f32 && hw > 0 && (!rows32 || hw % 32 == 0)) {
    q.stats = placeholder;
    q.stats_R = rows32 ? hw / 32 : 0;
  }
  // 5. the kernel, with its tile where its launcher takes one
  if (c3) {
    const bool par = pl.parity;
    const int Ht = par ? q.Hin : q.Hout, Wt = par ? q.Win : q.Wout;
    if (q.lrelu_in) {   // the halo-tile kernels are the 3x3 family with the LeakyReLU prologue (conv3x3_lrelu<...>)
      pl.kernel = ConvKernel::C3_HALO;
      c3_tile(q, pl);
    } else if (q.lo8_slab0) pl.kernel = q.splitk <= 1 && conv3x3p_selected(q) ? ConvKernel::C3_PINGPONG : ConvKernel::NONE;   // the one kernel that reads an fp8 lo half
    else if (conv3x3n_selected(q)) pl.kernel = conv3x3nt_selected(q) ? ConvKernel::C3_NARROW_FOLD : ConvKernel::C3_NARROW;
    else if (conv3x3d_selected(q)) pl.kernel = ConvKernel::C3_DATAFLOW;
    else if (conv3x3p_selected(q)) pl.kernel = ConvKernel::C3_PINGPONG;
    else {
      pl.kernel = ConvKernel::C3_HALO;
      c3_tile(q, pl);
    }
    if (q.stats && !rows32) {
      if (q.lo8_slab0 || pl.kernel == ConvKernel::C3_PINGPONG) q.stats_R = conv3x3p_stats_blocks(q);
      else if (pl.kernel == ConvKernel::C3_DATAFLOW) q.stats_R = conv3x3d_stats_blocks(q);
      else {   // 8x16 tiles (wide kernel): one block per workgroup; 8x8 tiles: one per wave half
        const int TW = pl.bm / 8;
        q.stats_R = ((Ht + 7) / 8) * ((Wt + TW - 1) / TW) * (TW == 16 ? 1 : 2) * (par ? 4 : 1);
      }
    }
  } else if (gemm) {
    if (gemm_df_selected(q)) pl.kernel = ConvKernel::GEMM_DF;
    else {
      pl.kernel = ConvKernel::GEMM_DMA;
      gemm_dma_tile(q, q.splitk > 1 ? q.splitk : 1, pl);
    }
  } else {
    pl.kernel = ConvKernel::IGEMM;
    igemm_tile(q, q.splitk > 1 ? q.splitk : 1, pl);
  }
  // 6. the pre-packed weights that kernel reads
  if (pl.kernel == ConvKernel::C3_DATAFLOW) pl.weights = q.xs ? ConvWeights::FRAG_SC : pl.parity ? ConvWeights::FRAG_PAR : ConvWeights::FRAG;
  else if (pl.kernel == ConvKernel::GEMM_DF) pl.weights = ConvWeights::GEMM_FRAG;

  p.splitk = q.splitk;
  p.stats_R = q.stats_R;
  if (pl.fold_gn) {
    p.gn_scale = nullptr; p.gn_shift = nullptr;
    p.w_bstride = q.w_bstride; p.bias_bstride = q.bias_bstride;
  }
  return pl;
}

// ---- the derived weight layouts a plan names: one recipe each (common.h) ----
size_t parity_weights_bytes(const ConvParams& p) { return (size_t)4 * p.Nrows * 4 * (p.C1 + p.C2) * sizeof(f16); }
void pack_parity_weights(const ConvParams& p, f16* dst, hipStream_t s) { launch_make_parity_weights(p.w, dst, p.Nrows, p.C1 + p.C2, s); }
size_t packed_weights_bytes(ConvWeights layout, const ConvParams& p) {
  return layout == ConvWeights::PLAIN ? 0 : layout == ConvWeights::GEMM_FRAG ? gemm_df_frag_bytes(p) : conv3x3d_frag_bytes(p);
}
void pack_weights(ConvWeights layout, const ConvParams& p, const f16* sc_w, f16* dst, hipStream_t s) {
  switch (layout) {
    case ConvWeights::PLAIN: break;
    case ConvWeights::FRAG_PAR: launch_pack_frag_weights_par(p.w_par, dst, p.N, p.Nrows, p.C1, s); break;
    case ConvWeights::FRAG:
    case ConvWeights::FRAG_SC:   // the nine taps as in FRAG, the folded shortcut's weights behind them
      launch_pack_frag_weights(p.w, dst, p.N, p.C1, s);
      if (layout == ConvWeights::FRAG_SC) launch_pack_frag_weights_sc(sc_w, dst, p.N, p.C1, p.Cs, p.Cs, s);
      break;
    case ConvWeights::GEMM_FRAG: launch_pack_gemm_frag(p.w, dst, p.Nrows, p.K, s); break;
  }
}
void pack_shortcut_bias(const ConvParams& p, const float* sc_bias, float* dst, hipStream_t s) { launch_add_vectors(p.bias, sc_bias, dst, p.Nrows, s); }
