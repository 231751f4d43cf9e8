// Implicit-GEMM convolution for gfx950 (CDNA4):   out[m, n] = sum_{tap, c} in[pix(m) + tap, c] * w[n][tap, c]
//
//   M = N_img * Ho * Wo output pixels, N = Cout, K = kh*kw*Cin, NHWC activations with a zero halo (no bounds checks in
//   the loop), weights pre-packed in 64-row x 128-byte blocks (pack.h, block_rows).
//
// One workgroup (WM x WN waves) computes a BM x BN tile; each wave owns a (BM/WM) x (BN/WN) sub-tile of 16x16 MFMA
// accumulators (v_mfma_f32_16x16x32_{bf16,f16}; fp32 mode: v_mfma_f32_16x16x4_f32, exact fp32 fma chains = the parity
// mode).  Per K step both operands advance by one 128-byte row chunk (64 bf16 / 32 fp32 of one filter tap), staged
// global -> LDS by LDS-DMA (buffer_load ... lds, 16 B per lane) into an S-stage ring: one counted vmcnt + one raw
// s_barrier per K step, the DMA of tile kt+S-1 is issued after the barrier into the stage whose reads just retired.
// LDS rows are 128 B; the 16-byte chunk c of row r lives in slot c ^ ((r >> 1) & 7): the DMA writes linearly, so the
// permutation is applied on the per-lane *source* address and again on the ds_read_b128 side (conflict-free for the
// 16-lane groups of ds_read_b128).  The A operand is a row gather: row r of the tile is the Cin-chunk of input pixel
// pix(m0 + r) shifted by the tap, so the per-lane voffset is fixed for the whole K loop and the tap / chunk advance is
// a wave-uniform soffset.
// Epilogue: + bias, ReLU, optional relu(x + residual) (reverse-connection sum), optional pixel-shuffle addressing
// (2x2 stride-2 transposed conv), optional fused 2x2 max-pool, store as dtype or fp32.
//
// This file holds the configurations conv_pick_cfg() can select, nothing else.  The ablation / stamp / experimental forms of
// this kernel that rounds 1-3 measured (HISTORY.md) are not in the tree: tools/experiments/README.md says where they are.
#include "conv_igemm_tile.h"

namespace ron {
namespace detail {

// The four-wave assembly K loop takes the 256 x 256 launches of bf16 / f16 whose workgroups' K chains fit its step table
// (RON_IGEMM256_V1=1: the eight-wave loop instead, for side-by-side timing).
static bool asm_loop_ok(int steps_per_wg) {
  static const bool v1 = getenv("RON_IGEMM256_V1") != nullptr;
  return !v1 && steps_per_wg <= kAsmLoopMaxSteps;
}

template <class Tr>
int launch_cfg(int cfg, int bn, const ConvArgs& a, hipStream_t s) {
  switch (cfg) {
    case kCfgIgemm256: case kCfgIgemm256TapsInner:                                                      // (the K order: ConvArgs::taps_inner)
      if constexpr (AsmLoop<Tr>::value) {
        // four waves, assembly K loop (conv_mfma4w.hip); bn = 224: its 256 x 224 form (conv_takes_224)
        if (asm_loop_ok(a.kt_split)) return launch_igemm4w(DtypeOf<Tr>::value, bn == 224 ? 224 : 256, a, s);
      }
      return launch_t<Tr, 256, 256, 4, 2, 2, 1>(a, s);
    case kCfgIgemm128: return launch_t<Tr, 128, 128, 2, 2, 2, 1>(a, s);
    case kCfgIgemm128Early: case kCfgIgemm128EarlyTapsInner: return launch_t<Tr, 128, 128, 2, 2, 2, 2>(a, s);
    case kCfgIgemm128x64: return launch_t<Tr, 128, 64, 2, 2, 2, 2>(a, s);
    case kCfgIgemm256x128:
      if constexpr (AsmLoop<Tr>::value) {
        if (asm_loop_ok(a.kt_split)) return launch_igemm4w(DtypeOf<Tr>::value, 128, a, s);
      }
      ron::set_error("conv: the 256 x 128 tile is the four-wave assembly loop's (bf16 / f16 / f16x3, <= %d K steps per workgroup)", kAsmLoopMaxSteps);
      return RON_ERR_INVALID;
  }
  ron::set_error("conv: unknown tile config %d", cfg);
  return RON_ERR_INVALID;
}

template <class Tr>
int launch_finalize(const ConvArgs& a, hipStream_t s) {
  const long long total = (long long)a.M * (a.Npad / 4);
  const int grid = (int)std::min<long long>((total + 255) / 256, 2048);
  RON_LAUNCH(splitk_finalize_kernel<Tr>, dim3(grid), dim3(256), 0, s, a);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

}  // namespace detail
using namespace detail;

size_t dtype_size(int dtype) { return dtype_is_half(dtype) ? 2 : 4; }     // F16X3: a hi and a lo f16 per element
int conv_k_chunk(int dtype) { return kRowBytes / (int)dtype_size(dtype); }
int conv_n_tile(int cout) { return cout <= 64 ? 64 : 128; }
int conv_num_cfgs() { return kNumCfgs; }

int check_conv_desc(const ron_conv_desc* d) {
  RON_REQUIRE(d != nullptr, "NULL descriptor");
  RON_REQUIRE(d->n >= 1 && d->h >= 1 && d->w >= 1 && d->cin >= 1 && d->cout >= 1, "conv: empty tensor (n %d, map %d x %d, cin %d, cout %d)",
              d->n, d->h, d->w, d->cin, d->cout);
  RON_REQUIRE(d->kh >= 1 && d->kh <= kConvMaxFilter && d->kw >= 1 && d->kw <= kConvMaxFilter, "conv: filter %d x %d: 1 .. %d", d->kh, d->kw, kConvMaxFilter);
  RON_REQUIRE(d->stride >= 1 && d->stride <= kConvMaxStride, "conv: stride %d: 1 .. %d", d->stride, kConvMaxStride);
  RON_REQUIRE(d->dilation >= 1 && d->dilation <= kConvMaxDilation, "conv: dilation %d: 1 .. %d", d->dilation, kConvMaxDilation);
  RON_REQUIRE((d->relu == 0 || d->relu == 1) && (d->pool == 0 || d->pool == 1) && (d->transpose == 0 || d->transpose == 1),
              "conv: relu %d, pool %d, transpose %d: each 0 or 1", d->relu, d->pool, d->transpose);
  if (!d->transpose && d->stride == 1) {
    const int pad = (std::max(d->kh, d->kw) - 1) * d->dilation / 2;
    RON_REQUIRE(pad <= kConvMaxPad, "conv: %d x %d filter at dilation %d: SAME padding %d, at most %d", d->kh, d->kw, d->dilation, pad, kConvMaxPad);
  }
  return RON_OK;
}

// ---- the planner: everything the host decides about a row-gather launch, each rule in one place ------------------------------------
//   tile_of / ConvGeom   tile shapes (rows, columns, slots of the chip, K-step cost); M, K, KT, taps and tile counts of a ConvLaunch
//   conv_pick_cfg        the tile configuration of a launch of its own; single_splitk: its split factor (launching and sizing both ask)
//   taps_inner_rule      the K order
//   plan_member          ONE convolution on a given tile: checks, kernel arguments, tile counts, split, tile order, pos_major, K order,
//                        224-column form - for a launch of its own (plan_conv) and for each member of a group (launch_conv_group)
//   with_traits          dtype -> traits class of the kernels
static bool igemm_is256(int cfg) { return cfg == kCfgIgemm256 || cfg == kCfgIgemm256TapsInner; }

// Tile of a row-gather configuration: BM x BN, the workgroups of it the chip holds at once (256 CUs; 64 KB of LDS lets two share a
// CU) and what a K step of a workgroup costs with the slots full - the schedule model of a group (measured, tools/_tune in HISTORY.md;
// 0: no grouped form, never measured).  The configurations with kernels of their own, and numbers out of range until plan_conv refuses
// them, read as the 128 x 128 tile: conv_scratch_bytes has always sized kCfgC64Resident that way (the kernel never splits; no reason
// found, kept so that no allocation changes).
struct Tile { int bm, bn, slots; double step_us; };
static const Tile& tile_of(int cfg) {
  static const Tile t256 = {256, 256, 256, 1.4}, t128 = {128, 128, 512, 1.15}, t128x64 = {128, 64, 512, 0.75}, t256x128 = {256, 128, 256, 0.0};
  if (igemm_is256(cfg)) return t256;
  return cfg == kCfgIgemm128x64 ? t128x64 : (cfg == kCfgIgemm256x128 ? t256x128 : t128);
}

struct ConvGeom {
  int M, taps, K, KT, Npad, n_long;      // GEMM rows (un-pooled), filter taps, K in elements and in steps, columns, the long ones (center_from)
  explicit ConvGeom(const ConvLaunch& c)
      : M(c.in.N * c.Ho * c.Wo), taps(c.kh * c.kw), K(taps * c.in.C), KT(K / conv_k_chunk(c.dtype)), Npad(c.Npad),
        n_long(c.center_from > 0 ? c.center_from : c.Npad) {}
  int rows(const Tile& t) const { return (M + t.bm - 1) / t.bm; }
  int cols(const Tile& t) const { return Npad / t.bn; }
  int long_cols(const Tile& t) const { return n_long / t.bn; }      // centre-tap-only columns: the tiles that run every tap
  int tiles(const Tile& t) const { return rows(t) * cols(t); }
};
static int64_t slab_bytes(const ConvLaunch& c, int sk) { return (int64_t)sk * ConvGeom(c).M * c.Npad * 4; }      // fp32 slabs of sk K slices

// The 256 x 224 form of the four-wave 256 x 256 tile: a plain bf16 / f16 convolution of 193 .. 224 output channels in one column
// tile (the class-prediction heads: Cout = 210, 46 of 256 columns padding) runs 8 x 7 blocks per wave instead of 8 x 8: an eighth
// fewer MFMAs and B fragment reads per K step, evenly over the four waves.  Which columns a workgroup computes changes, the K order of
// an output element does not: the results are the 256-column tile's, bit for bit.  Not a tile configuration of its own - it is the
// width launch_conv / launch_conv_group run kCfgIgemm256[TapsInner] at for such a launch (conv_describe reports it as the N tile).
// `steps_per_wg`: the K steps of a workgroup (the assembly loop's step table).  ConvLaunch::n224 = 0: always 256 columns (what the
// single-operator entry points set under RON_IGEMM224=0, so that tests and sweeps can run both forms side by side).
static bool conv_takes_224(const ConvLaunch& c, int steps_per_wg) {
  return c.n224 != 0 && dtype_is_half(c.dtype) && c.Npad == 256 && c.Cout > 192 && c.Cout <= 224 && c.up == 0 && !c.pool && c.center_from == 0 &&
         c.split_n == 0 && c.out2.base == nullptr && asm_loop_ok(steps_per_wg);
}

// Split-K factor for grids that leave most CUs idle: such launches are a serial chain of KT dependent
// HBM round trips per workgroup, so the K loop is spread over enough workgroups to fill the chip (>= 8 steps each).
int conv_pick_splitk(int tiles, int KT, int slots, int tile_elems) {
  if (tiles < 1 || tiles * 2 > slots || KT < 16) return 1;
  int sk = slots / tiles, min_steps = 8;
  if (sk > KT / min_steps) sk = KT / min_steps;
  if (sk <= 1) return 1;
  // A split launch pays a second launch and writes, then reads, sk fp32 copies of its output: with many rows and a short K that
  // costs more than the chain it shortens (SSD-512 block8_conv1x1, 16 384 rows x 256 over 16 steps, kernel trace of round 5:
  // 20 us + a 16 us finalize pass for 33 MB of slabs).  Per K step of a workgroup ~1.1 us, ~5 us for the dependent launch,
  // ~4 TB/s for the slab traffic; the split stays where the model says it wins.  Same box, with / without (RON_SPLITK_NO_VETO=1):
  // SSD-512 batch 1 0.697 -> 0.685 ms, batch 4 1.157 -> 1.147, RON and the batch-16 / 32 / 64 benchmark configurations unchanged.
  static const bool veto = getenv("RON_SPLITK_NO_VETO") == nullptr;
  if (veto) {
    const double step_us = 1.1, launch_us = 5.0, bytes_per_us = 4e6;      // (a lone launch, slots not full: not Tile::step_us)
    const double tile_bytes = 4.0 * tile_elems;       // fp32 slab of one tile (BM x BN of the configuration: 256 x 128 is half of 256 x 256)
    const double t_split = ((KT + sk - 1) / sk) * step_us + launch_us + 2.0 * sk * tiles * tile_bytes / bytes_per_us;
    if (t_split >= KT * step_us) return 1;
  }
  return sk;
}

// The split factor of a launch of its own on `cfg`: the caller's, else by the grid.  plan_conv launches with it and conv_scratch_bytes
// sizes the slabs by it, so the two cannot disagree.  (A fused pool or transposed conv of its own never splits, whatever this says: plan_member.)
static int single_splitk(const ConvLaunch& c, int cfg) {
  const Tile& t = tile_of(cfg);
  const ConvGeom g(c);
  return c.splitk >= 0 ? c.splitk : conv_pick_splitk(g.tiles(t), g.KT, t.slots, t.bm * t.bn);
}

// Default tile of the row-gather kernel, from tools/sweep_conv.py on MI355X at batch 32 (profiles/r01/sweep_*.txt).
// The 256x256 tile wins once it yields >= ~160 workgroups; below that the grid is the problem and the 128x128 /
// 2-workgroups-per-CU form keeps more CUs busy.
constexpr int kTapsInnerMaxN = 2048;       // widest run of long columns the taps-innermost K order is chosen for
int conv_pick_igemm_cfg(int M, int Npad, int taps, int K, bool may_split) {
  const int tm256 = (M + 255) / 256;
  if (Npad % 128 != 0) return kCfgIgemm128x64;
  if (Npad % 256 == 0) {
    const int t256 = tm256 * (Npad / 256);
    // taps innermost: worth 1-6 % of the run time up to two column tiles, time-neutral on wider layers (trio3: six long column tiles,
    // 669 vs 660 us) where it still cuts the fabric reads by a fifth (profiles/r04/sweep_taps_inner_all.txt); conv_pick_cfg takes it
    // back where skipping halo filter rows is worth more (fc6: 514 us tap-major with skipping, 567 us taps-innermost)
    if (t256 >= 144) return (taps > 1 && Npad <= kTapsInnerMaxN) ? kCfgIgemm256TapsInner : kCfgIgemm256;      // (round 5: 160 -> 144, sweep_all_cfgs)
    // few fat tiles with a long K (in elements: the split-precision and fp32 forms take twice the steps for the same K): split-K
    // fills the chip with them too, at twice the arithmetic per staged byte of the 128 x 128 tiles (tools/sweep_conv.py, round 3:
    // block6_conv_left 26 tiles x 36 864 132 -> 126 us, fc6 at batch 8 214 -> 191, cls_pred / inception2 shapes of 50-100 tiles x 9 216
    // +3-10 %; with K = 4 608 or a handful of tiles the 128 x 128 form wins, in f16x3 as well: conv5_1 188 vs 202 us)
    if (may_split && t256 <= 128 && ((t256 >= 48 && K >= 9216) || (t256 >= 24 && K >= 32768))) return kCfgIgemm256;     // <= 128 tiles: K gets split
  }
  // the 128 x 128 tile with a stage's LDS-DMA pieces issued during its first k-step: level or 3-8 % ahead of the spread-out issue on
  // every layer and batch of the round-3 sweep (profiles/r03/sweep_conv_128_early.txt), not only on conv2_x's many rounds
  return kCfgIgemm128Early;
}

// Order of the tiles inside the run of workgroups that shares an XCD's L2 (1/8 of the launch): N fastest re-reads few activation
// tiles and every weight slice of those columns, M fastest the other way round.  Estimated bytes an XCD has to fetch once:
// activation tiles it touches x their size + weight slices it touches x theirs; M fastest when that is less (fc6: 13 row tiles x
// 16 column tiles of 12.8 MB of weights each - N fastest makes every XCD stream all 205 MB: 1.66 GB fetched per launch, 0.65 GB
// M fastest, 566 -> 541 us; fc7 113 -> 102 us).  Forced on every launch it costs the activation-heavy layers 2-4 %; walking the
// column tiles of an XCD's rows in blocks of 1-3 instead changed nothing (both measured, not kept).
// `tiles_m`: the row tiles of the launch (a fused pool's rows are not ConvGeom's).
constexpr int kPanelCols = 8;      // the panel width of wide and tall launches (plain GEMM shapes)
static int pick_m_fastest(const ConvLaunch& c, const Tile& t, int tiles_m, int splitk, int panel_steps) {
  const ConvGeom g(c);
  const int tiles_n = g.cols(t), cols = g.long_cols(t);      // (centre-tap-only columns: panels among the long ones)
  // split-K: the workgroups of one K slice are consecutive, an XCD's run then covers (nearly) every tile of its slices either way
  if (tiles_m < 2 || tiles_n < 2 || splitk > 1) return 0;
  const double esz = (double)dtype_size(c.dtype);
  const double a_tile = (double)t.bm * c.in.C * esz * (c.stride > 1 ? g.taps : (g.taps > 1 ? 2 : 1));   // unique input bytes of a row tile
  const double b_tile = (double)t.bn * g.K * esz;
  const int per_xcd = std::max(1, tiles_m * tiles_n / 8);
  const double cost_n = (per_xcd / tiles_n + 1) * a_tile + std::min(tiles_n, per_xcd) * b_tile;
  const double cost_m = std::min(tiles_m, per_xcd) * a_tile + (per_xcd / tiles_m + 1) * b_tile;
  // 2: panels of kPanelCols column tiles (wide AND tall launches: plain GEMM shapes, fc7 at large batches)
  // (not the transposed conv: its pixel-shuffle epilogue wants the four taps of a pixel block written close in time - measured at
  // batch 4: the groups that carry block4 / block5_deconv_right 8-10 us slower in panel order)
  // Only the four-wave tiles decode it (conv_igemm_tile): `panel_steps` = the K steps of a workgroup when the launch may go to
  // them, 0 when it may not (members of a grouped launch).
  const bool panels_ok = t.bm == 256 && c.dtype != RON_DTYPE_F32 && panel_steps > 0 && asm_loop_ok(panel_steps) && c.up == 0;
  // experiments (tools/experiments/r06_calls/r06_panels.sh): RON_PANEL_COLS = P forces panels of P column tiles on every launch that
  // can decode them (P = 1: row tiles fastest, 0: column tiles fastest)
  static const char* force = getenv("RON_PANEL_COLS");
  if (force != nullptr && panels_ok) {
    const int P = atoi(force);
    return P >= cols ? 0 : P;
  }
  int pick = cost_m < 0.95 * cost_n ? 1 : 0;
  if (panels_ok && tiles_n >= 2 * kPanelCols && tiles_m >= 8 && c.center_from == 0) {
    const double cost_p = std::min(tiles_m, per_xcd / kPanelCols + 1) * a_tile +
                          std::min(tiles_n, kPanelCols * (per_xcd / (tiles_m * kPanelCols) + 1)) * b_tile;
    if (cost_p < 0.9 * std::min(cost_n, cost_m)) pick = kPanelCols;
  }
  // Round 6: the width of the panel from what an XCD's CUs fetch PER ROUND.  Its 32 workgroups run in step through K; with panels of P
  // column tiles they are 32 / P row tiles x P column tiles, and a round streams those row tiles' input lines and those column tiles'
  // weights through a 4 MB L2 that keeps neither for the next round (the weights of ONE 256 x 4608 column tile are 2.4 MB).  Measured
  // (profiles/r06/panel_width_sweep.txt, FETCH_SIZE x 2 + WRITE_SIZE per launch at batch 32): block4 trio3 group 1482 MB with its six long
  // columns fastest, 1002 with P = 2, 1133 / 1166 with 3 / 4; block5 trio3 group 667 -> 547; fc7 group 606 (P = 8) -> 514 (P = 4);
  // 7.40 -> 6.71 GB per step with P = 2 everywhere.  The launches' TIMES did not move (560.4 vs 560.7 us, the step 4.291 vs 4.279 ms):
  // these launches are not short of fabric bandwidth, and the bytes saved did not come back as clock either - the choice is made for the
  // traffic alone, and only where the model sees a clear difference.  A row tile's unique input lines: ~1.3 x its own rows for a 3 x 3
  // filter on these maps (the halo rows), not the 2 x of the column / row estimate above.
  if (panels_ok && cols >= 3) {
    const double a_round = (double)t.bm * c.in.C * esz * (c.stride > 1 ? g.taps : (g.taps > 1 ? 1.3 : 1.0));
    const int resident = std::min(32, std::max(1, tiles_m * cols / 8));
    auto per_round = [&](int P) {
      P = std::max(1, std::min(P, cols));
      return ((resident + P - 1) / P) * a_round + P * b_tile;
    };
    const double now = per_round(pick == 0 ? cols : pick);
    int best = pick;
    double best_cost = now;
    for (int P : {2, 3, 4, 8}) {
      if (P >= cols) break;
      const double t_round = per_round(P);
      if (t_round < 0.95 * best_cost) { best = P; best_cost = t_round; }
    }
    if (best_cost < 0.95 * now) pick = best;
  }
  return pick;
}

// Position-major rows + per-tile skipping of filter rows that only see the zero halo (ConvArgs::pos_major): where the K steps a
// launch executes drop by >= 5 % (fc6 7x7 on 10 x 10: 91 -> 77 filter rows over its 13 row tiles; conv6 of SSD-512, rate 6).
// Only the tap-major K order (a skipped filter row is a contiguous K range), no fused pool / transposed conv; split-K slices
// share what is left of a tile's K range.
static int pick_pos_major(const ConvLaunch& c, int cfg) {
  if (!c.halo_skip || c.pool || c.up > 0 || c.kh < 2 || conv_cfg_taps_inner(cfg)) return 0;
  // at most (kh - 1) * dil of a map's H output rows can skip anything: below 5 % there is nothing to decide (and no per-tile walk
  // over the thousands of tiles of a large map on the launch path)
  if ((c.kh - 1) * c.dil * 20 < c.in.H) return 0;
  const int BM = tile_of(cfg).bm, M = ConvGeom(c).M, tiles_m = ConvGeom(c).rows(tile_of(cfg));
  long long rows_all = 0, rows_kept = 0;
  for (int t = 0; t < tiles_m; ++t) {
    const int oy_lo = (t * BM / c.in.N) / c.Wo, oy_hi = ((std::min(M, (t + 1) * BM) - 1) / c.in.N) / c.Wo;
    int lo = 0, hi = c.kh - 1;
    while (lo < hi && oy_hi * c.stride - c.cpad + lo * c.dil < 0) ++lo;
    while (hi > lo && oy_lo * c.stride - c.cpad + hi * c.dil > c.in.H - 1) --hi;
    rows_all += c.kh;
    rows_kept += hi - lo + 1;
  }
  return rows_kept * 100 <= rows_all * 95 ? 1 : 0;
}

// The K order: taps innermost (consecutive steps re-read almost the same input lines) for stride-1 filters that neither split K nor
// skip filter rows - only for the stride-1 convolutions it has been measured and tested on (the stride-2 3x3 convolutions of SSD-512's
// extra blocks keep the tap-major order); with split-K it loses (conv5_1 at batch 4 +10 %).  Centre-tap-only column tiles of such a
// launch keep the tap-major walk of their one tap.
// `splits` is an argument because the callers do not mean the same by it.  conv_pick_cfg chooses between a configuration and its
// taps-innermost twin before any split is applied: it passes the split the PLANNER would choose (none on the 256 x 256 tile, which is
// picked for grids that fill the chip) and a factor the caller forces does not count - a test or sweep that forces a factor on
// kCfgIgemm256TapsInner / kCfgIgemm128EarlyTapsInner runs that order split.  plan_member, for the tiles without a twin, passes the
// split it applied, forced or not.  No reason for the difference is recorded anywhere; both answers are kept as they were.
// (Both are callables: conv_pick_cfg runs for every launch ron_forward enqueues, and neither is worked out where the cheap clauses decide.)
template <class S, class R>
static bool taps_inner_rule(const ConvLaunch& c, S splits, R skips_rows) {
  return c.kh * c.kw > 1 && c.up == 0 && c.stride == 1 && !splits() && !skips_rows();
}

// The halo-patch kernel (conv_patch.hip) where it applies and wins (conv_patch_pick), else the row-gather kernel.
int conv_pick_cfg(const ConvLaunch& c) {
  const ConvGeom g(c);
  if (c.split_n == 0 && conv_c64_applicable(c)) return kCfgC64Resident;
  if (c.out2.base == nullptr && conv_patch_applicable(c)) {
    const int cfg = conv_patch_pick(c);
    if (cfg >= 0) return cfg;
  }
  // centre-tap-only columns are a ninth of a column's work: the grid that has to fill the chip is the long columns'
  // (split K: not with a fused pool / transposed conv, and a launch with centre-tap-only columns counts those tiles too)
  const bool may_split = c.center_from == 0 && !c.pool && c.up == 0 && c.splitk < 0;
  const int t256x128 = g.tiles(tile_of(kCfgIgemm256x128));
  // Cout = 128 (conv2_x) on maps large enough to fill the chip with 256 x 128 tiles: the four-wave assembly loop at 48 KB staged per
  // K step instead of two 128 x 128 workgroups per CU at 64 KB (sweep: profiles/r05/sweep_256x128.txt)
  if (c.dtype != RON_DTYPE_F32 && c.Npad % 256 == 128 && c.center_from == 0 && c.up == 0 && c.out2.base == nullptr && t256x128 >= 256 &&
      asm_loop_ok(g.KT))
    return kCfgIgemm256x128;
  const int cfg = conv_pick_igemm_cfg(g.M, g.n_long, g.taps, g.K, may_split);
  // (taps innermost on 256 x 256 is taken back where skipping halo filter rows is worth more: conv_pick_igemm_cfg)
  const auto skips_rows = [&](int on) { return [&c, on] { return pick_pos_major(c, on) != 0; }; };
  if (cfg == kCfgIgemm256TapsInner && !taps_inner_rule(c, [] { return false; }, skips_rows(kCfgIgemm256))) return kCfgIgemm256;
  if (cfg == kCfgIgemm128Early && c.dtype != RON_DTYPE_F32 && c.center_from == 0) {
    // Where 256 x 256 tiles would leave most CUs idle (and K is not long enough to split them, above) the fallback used to be the
    // 128-row tiles: two workgroups per CU, twice the staged bytes per MAC.  Every tile configuration against this function's choice,
    // every layer shape, batches 4 .. 64 (profiles/r05/sweep_256x128_all_layers_batches.txt, sweep_all_cfgs_all_layers_batches.txt):
    // the 256 x 128 four-wave tile where it makes the launch about ONE round of the chip (48 .. 287 tiles; below 129 with K split in
    //    two): conv5_x at batch 32 / conv4_x at 8 / conv3_x at 4 75 -> 55 us (200 tiles), fc7 at batch 16 65 -> 51 (224); from 288
    //    (= 144 tiles of 256 x 256) on that tile wins by 13-17 %, below ~48 the launch is latency either way;
    if (c.up == 0 && asm_loop_ok(g.KT) && t256x128 >= 48 && t256x128 < 288) return kCfgIgemm256x128;
    // (The 128 x 64 tile for the smallest launches - SSD-512's tail convolutions 13.5 -> 11.5 us stand-alone - was tried as a third
    // rule: SSD-512 batch 1 -0.8 %, RON batch 2 +0.6 %; not kept.)
  }
  if (cfg == kCfgIgemm128Early) {
    // taps innermost for the 128 x 128 tile too: 3-6 % on launches that do not split K, and where no filter rows can be skipped instead
    const auto splits = [&] { return may_split && single_splitk(c, kCfgIgemm128Early) > 1; };
    if (taps_inner_rule(c, splits, skips_rows(kCfgIgemm128Early))) return kCfgIgemm128EarlyTapsInner;
  }
  return cfg;
}

// ONE convolution on tile configuration `cfg` (a row-gather one): the requirement checks (`who` starts their messages; the caller has
// run check_conv_fields), the kernel arguments, tile counts, the split into `sk` K slices if `slab` (`slab_bytes`) holds their fp32
// sums, tile order, pos_major, K order, and *bn: the width of the column tile (the configuration's own, or 224: conv_takes_224).
// `four_wave`: the launch may go to the four-wave tiles (which decode panel tile orders and have the 224-column form) - a launch of its
// own always may, a group when every member's K chain fits their step table.
// `grouped`: a member of a group.  Two rules differ there, both because a group has one kernel per tile and not the twins a launch of
// its own chooses between: the K order of the 128 x 128 and 256 x 256 tiles comes from taps_inner_rule and not from the configuration;
// and a split factor the planner chose does not keep a member off the 224-column form.  As before, a transposed member is split when
// its factor says so (conv_group_scratch_bytes sizes that slab; group_splitks gives such members 1) and may have centre-tap-only columns.
static int plan_member(const char* who, const ConvLaunch& c, int cfg, int sk, void* slab, int64_t slab_size, bool four_wave, bool grouped,
                       ConvArgs& a, int* bn) {
  const Tile& t = tile_of(cfg);
  const ConvGeom g(c);
  const int chunk = conv_k_chunk(c.dtype);
  RON_REQUIRE(c.in.C % chunk == 0, "%s: Cin %d is not a multiple of the K chunk %d", who, c.in.C, chunk);
  RON_REQUIRE(c.in.pad >= c.cpad, "%s: input halo %d < conv padding %d", who, c.in.pad, c.cpad);
  RON_REQUIRE(c.in.bytes > 0 && c.in.bytes < (int64_t)1 << 32, "%s: input allocation must be < 4 GiB for buffer addressing", who);
  RON_REQUIRE(c.wgt_bytes > 0 && c.wgt_bytes < (int64_t)1 << 32, "%s: weight allocation must be < 4 GiB", who);
  RON_REQUIRE(c.out.pixels() * c.out.cstride < (int64_t)1 << 31, "%s: output too large for 32-bit offsets", who);
  RON_REQUIRE(c.Npad % t.bn == 0, "%s: Npad %d not a multiple of the N tile %d", who, c.Npad, t.bn);
  if (c.up > 0) RON_REQUIRE(c.up_cout % t.bn == 0, "transposed conv: channels per tap %d not a multiple of %d", c.up_cout, t.bn);
  if (c.center_from > 0)
    RON_REQUIRE(c.center_from % t.bn == 0 && (c.kh & 1) && (c.kw & 1) && (grouped || c.up == 0),
                "%s: centre-tap-only columns need an odd filter and a boundary on the N tile (%d)", who, t.bn);
  RON_REQUIRE((int64_t)c.Npad * g.K * (int)dtype_size(c.dtype) == c.wgt_bytes, "%s: packed weight size mismatch", who);
  fill_conv_args(c, &a);
  // SAME pool (plan_conv has checked the views): tile rows are the windows' four positions, ceil(Ho / 2) x ceil(Wo / 2) windows per
  // image (an odd map's last windows hold positions that are no pixel: conv_igemm_tile)
  if (c.pool) a.M = 4 * c.in.N * c.out.H * c.out.W;
  a.tiles_n = g.cols(t);
  a.tiles_total = ((a.M + t.bm - 1) / t.bm) * a.tiles_n;
  if (sk > 1 && (grouped || (c.up == 0 && !c.pool)) && slab != nullptr && slab_bytes(c, sk) <= slab_size) {
    a.kt_split = (a.KT + sk - 1) / sk;
    a.splitk = (a.KT + a.kt_split - 1) / a.kt_split;      // no empty split
    a.partial = static_cast<float*>(slab);
    if (a.splitk == 1) { a.kt_split = a.KT; a.partial = nullptr; }
  }
  const int tile_order = pick_m_fastest(c, t, a.tiles_total / a.tiles_n, a.splitk, four_wave ? a.kt_split : 0);
  RON_REQUIRE(tile_order >= 0 && tile_order <= kConvMaxTileOrder, "%s: tile order %d: 0 .. %d", who, tile_order, kConvMaxTileOrder);
  a.m_fastest = tile_order;
  a.pos_major = pick_pos_major(c, cfg);
  // K order: the configuration's where it names one; by the rule on the 256 x 128 tile and, in a group, on the 128 x 128 tile and on the
  // 256 x 256 tile where the long columns are at most two tiles wide (what conv_pick_igemm_cfg asks of a launch of its own)
  const bool by_rule = cfg == kCfgIgemm256x128 || (grouped && (cfg == kCfgIgemm128 || (cfg == kCfgIgemm256 && g.n_long <= kTapsInnerMaxN)));
  const bool by_rule_inner = by_rule && taps_inner_rule(c, [&] { return a.splitk > 1; }, [&] { return a.pos_major != 0; });
  a.taps_inner = (conv_cfg_taps_inner(cfg) || by_rule_inner) ? 1 : 0;
  // 193 .. 224 output channels on the four-wave 256 x 256 tile: its 224-column form.  A split factor plan_conv chose itself keeps the
  // 256 columns: those are the launches of fewer than 129 tiles (block4_cls_pred below batch 24), which nobody has measured on the
  // narrower tile; a factor the caller forces (single-operator entry points, the sweep) does not stand in the way.
  const bool split_allows = grouped || a.splitk == 1 || c.splitk >= 0;
  *bn = (four_wave && igemm_is256(cfg) && split_allows && conv_takes_224(c, a.kt_split)) ? 224 : t.bn;
  return RON_OK;
}

// Everything launch_conv decides before it launches: the tile configuration, the kernel arguments (plan_member) and the width of the
// row-gather kernel's column tile (0 for the other kernels).
static int plan_conv(const ConvLaunch& c, int* cfg_out, ConvArgs* a, int* bn) {
  *bn = 0;
  if (const int rc = check_conv_fields(c)) return rc;      // before the pickers divide by any of it
  const int cfg = c.cfg >= 0 ? c.cfg : conv_pick_cfg(c);
  *cfg_out = cfg;
  RON_REQUIRE(cfg >= 0 && cfg < kNumCfgs, "conv: tile config %d out of range [0, %d)", cfg, kNumCfgs);
  if (conv_cfg_is_patch(cfg) || cfg == kCfgC64Resident) return RON_OK;      // kernels of their own: nothing more to plan here
  RON_REQUIRE(!conv_cfg_taps_inner(cfg) || c.up == 0, "conv: the taps-innermost order is for plain convolutions");
  if (c.pool) {
    RON_REQUIRE(c.up == 0 && c.res == nullptr && !c.out_f32 && c.stride == 1, "conv + fused pool: plain stride-1 conv only");
    RON_REQUIRE(c.out.H == (c.Ho + 1) / 2 && c.out.W == (c.Wo + 1) / 2, "conv + fused pool: output view must be the pooled map");
  }
  if (const int rc = plan_member("conv", c, cfg, single_splitk(c, cfg), c.scratch, c.scratch_bytes, true, false, *a, bn)) return rc;
  if (c.split_n > 0) {
    RON_REQUIRE(c.out_f32 && !c.pool && c.up == 0 && c.res == nullptr && c.center_from == 0, "conv: two head outputs from a plain fp32-output convolution only");
    RON_REQUIRE(c.split_n % 8 == 0 && c.split_first > 0 && c.split_first <= c.split_n && c.split_n < c.Cout,
                "conv: bad output split (first %d, second from %d, %d columns)", c.split_first, c.split_n, c.Cout);
    RON_REQUIRE(c.out.pad == 0 && c.out.coff == 0 && c.out.cstride == c.out.C && c.out.C == c.split_first && c.out2.base != nullptr &&
                c.out2.pad == 0 && c.out2.coff == 0 && c.out2.cstride == c.out2.C && c.out2.C == c.Cout - c.split_n &&
                c.out2.H == c.Ho && c.out2.W == c.Wo && c.out2.N == c.in.N && c.out.H == c.Ho && c.out.W == c.Wo,
                "conv: the two head outputs must be dense [n][Ho][Wo][C] tensors of %d and %d channels", c.split_first, c.Cout - c.split_n);
    RON_REQUIRE(c.out2.pixels() * c.out2.cstride < (int64_t)1 << 31, "conv: second output too large for 32-bit offsets");
  } else if (c.out2.base != nullptr) {
    RON_REQUIRE(c.pool && c.out2.H == c.Ho && c.out2.W == c.Wo && c.out2.C >= c.Cout && c.out2.N == c.in.N,
                "conv: a second output is the un-pooled map of a fused-pool launch");
    RON_REQUIRE(c.out2.pixels() * c.out2.cstride < (int64_t)1 << 31, "conv: second output too large for 32-bit offsets");
  }
  return RON_OK;
}

int conv_describe(const ConvLaunch& c, int out[4], int* n_tile) {
  int cfg = -1, bn = 0;
  ConvArgs a = ConvArgs();
  if (const int rc = plan_conv(c, &cfg, &a, &bn)) return rc;
  if (n_tile != nullptr) *n_tile = bn;
  out[0] = cfg;
  const bool gather = !conv_cfg_is_patch(cfg) && cfg != kCfgC64Resident;
  out[1] = gather ? a.splitk : 1; out[2] = gather ? a.m_fastest : 0; out[3] = gather ? a.taps_inner : 0;
  return RON_OK;
}

// f(Tag<Traits>()) for the traits class of `dtype` (`who` starts the message when there is none)
template <class T> struct Tag { using type = T; };
template <class F>
static int with_traits(int dtype, const char* who, F f) {
  switch (dtype) {
    case RON_DTYPE_BF16: return f(Tag<TraitsBF16S>());
    case RON_DTYPE_F16: return f(Tag<TraitsF16S>());
    case RON_DTYPE_F32: return f(Tag<TraitsF32S>());
    case RON_DTYPE_F16X3: return f(Tag<TraitsF16X3S>());
  }
  ron::set_error("%s: unknown dtype %d", who, dtype);
  return RON_ERR_INVALID;
}

int launch_conv(const ConvLaunch& c, hipStream_t stream) {
  int cfg = -1, bn = 0;
  ConvArgs a = ConvArgs();
  if (const int rc = plan_conv(c, &cfg, &a, &bn)) return rc;
  if (conv_cfg_is_patch(cfg)) return launch_conv_patch(c, cfg, stream);
  if (cfg == kCfgC64Resident) return launch_conv_c64(c, stream);
  return with_traits(c.dtype, "conv", [&](auto tag) {
    using Tr = typename decltype(tag)::type;
    const int rc = launch_cfg<Tr>(cfg, bn, a, stream);
    return (rc != RON_OK || a.splitk == 1) ? rc : launch_finalize<Tr>(a, stream);
  });
}

// ---- grouped launches ---------------------------------------------------------------------------------------------
namespace detail {

template <class Tr>
int launch_group_cfg(int cfg, const ConvGroupArgs& g, bool any_split, hipStream_t s) {
  if (cfg == kGroupMixed) return launch_group_mixed<Tr>(g, any_split, s);
  if (cfg == kCfgIgemm128x64) return launch_group_t<Tr, 128, 64, 2, 2, 2, 2>(g, any_split, s);
  if (cfg == kCfgIgemm128) return launch_group_t<Tr, 128, 128, 2, 2, 2, 2>(g, any_split, s);      // pieces issued early, as kCfgIgemm128Early
  if (cfg == kCfgIgemm256) {                                                                       // two launches of < 1 round each as one
    if constexpr (AsmLoop<Tr>::value) {
      int longest = 0;
      for (int k = 0; k < g.n; ++k) longest = std::max(longest, g.op[k].kt_split);
      if (asm_loop_ok(longest)) return launch_igemm4w_group(DtypeOf<Tr>::value, g, any_split, s);
    }
    return launch_group_t<Tr, 256, 256, 4, 2, 2, 1>(g, any_split, s);
  }
  ron::set_error("conv group: tile config %d has no grouped form", cfg);
  return RON_ERR_INVALID;
}

// Split-K inside a group: the group as a whole fills the chip, so K is split only to bound the serial chain of K steps
// of one workgroup (the latency of the launch; <= ~24 steps each, >= 8) and only for convolutions with few tiles: the
// fp32 slabs of a many-tile convolution cost more HBM traffic than the shorter chain saves.
int group_pick_splitk(int KT, int tiles) {
  if (KT < 16 || tiles < 1) return 1;
  int sk = (KT + 23) / 24;
  if (sk > 512 / tiles) sk = 512 / tiles;
  if (sk > KT / 8) sk = KT / 8;
  return sk < 1 ? 1 : sk;
}

}  // namespace detail

// tile configuration member `c` of a group launched as `group_cfg` runs on
static int group_member_cfg(int group_cfg, const ConvLaunch& c) {
  return group_cfg == kGroupMixed ? (c.Npad % 128 == 0 ? kCfgIgemm128 : kCfgIgemm128x64) : group_cfg;
}

// Split-K factors of a mixed-width group (one dependency level of the heads: a large "carrier" member and latency-bound small
// ones) from a model of how the launch runs: workgroups are dispatched in blockIdx order onto the slots of the group's tile (512: two
// per CU for both 128-row tiles), a workgroup takes as long as its K steps.  For a common chunk length T (K steps per workgroup) every member
// is cut into ceil(KT / T) slices (>= 8 steps each; transposed convs, fused pools and forced factors stay as they are); the
// makespan of the resulting list schedule plus what the fp32 slabs cost (written and read once, in K-step units) is evaluated for
// a ladder of T, the cheapest wins.  What the fixed "<= 24 steps per workgroup" rule missed: {block7_conv_left, block6_conv_left}
// came to 808 workgroups of 116 / 24 steps = 1.6 rounds of the long ones; four slices of 144 steps are one round.
static long long group_makespan(const int* len, const int* cnt, int n, int slots) {
  // list scheduling in dispatch order (members as given, longest first is the caller's job); slot finish times in a min-heap
  std::vector<long long> heap(slots, 0);
  auto sift = [&](size_t i) {
    const size_t N = heap.size();
    for (;;) {
      size_t l = 2 * i + 1, r = l + 1, m = i;
      if (l < N && heap[l] < heap[m]) m = l;
      if (r < N && heap[r] < heap[m]) m = r;
      if (m == i) return;
      std::swap(heap[i], heap[m]);
      i = m;
    }
  };
  long long end = 0;
  for (int k = 0; k < n; ++k)
    for (int w = 0; w < cnt[k]; ++w) {
      heap[0] += len[k];
      end = std::max(end, heap[0]);
      sift(0);
    }
  return end;
}

static void group_splitks_scheduled(const ConvLaunch* ls, int n, int cfg, int* sk) {
  const double kSlabBytesPerUs = 2.0e6;      // slab bytes the memory side moves per us (slots and K-step costs: tile_of)
  int tiles[kMaxConvGroup], KT[kMaxConvGroup];
  double step_us[kMaxConvGroup];
  bool fixed[kMaxConvGroup];
  for (int k = 0; k < n; ++k) {
    const ConvLaunch& c = ls[k];
    const int mcfg = group_member_cfg(cfg, c);
    const Tile& t = tile_of(mcfg);
    const ConvGeom g(c);
    KT[k] = g.KT;
    // a member on the 256 x 224 tile: 7/8 of the MFMAs of a step (block4_cls_pred alone measured 0.83 x, profiles/r08).  The plans of
    // RON-320 full at batches 1 .. 64 are the same for any value from 1.15 to 1.4 here: the entry moves no split factor today.
    // (KT, not the slice the plan will give the member: a slice is never longer, so the step-table limit cannot turn out tighter.)
    step_us[k] = (mcfg == kCfgIgemm256 && conv_takes_224(c, KT[k])) ? t.step_us * 7 / 8 : t.step_us;
    // centre-tap-only column tiles are a ninth of a tile: count them as that
    tiles[k] = g.rows(t) * g.long_cols(t) + g.rows(t) * (g.cols(t) - g.long_cols(t)) / g.taps;
    fixed[k] = c.up > 0 || c.pool || c.splitk >= 0 || KT[k] < 16;
    sk[k] = c.splitk >= 0 ? std::max(c.splitk, 1) : 1;
  }
  static const int ladder[] = {8, 12, 16, 24, 32, 36, 48, 64, 72, 96, 128, 144, 192, 256, 288, 384, 576, 1 << 20};
  double best = 1e30;
  int best_sk[kMaxConvGroup];
  for (int T : ladder) {
    int cand[kMaxConvGroup], len[kMaxConvGroup], cnt[kMaxConvGroup], order[kMaxConvGroup];
    double slab_us = 0;
    bool any = false;
    for (int k = 0; k < n; ++k) {
      cand[k] = fixed[k] ? sk[k] : std::max(1, std::min((KT[k] + T - 1) / T, KT[k] / 8));
      len[k] = (int)(((KT[k] + cand[k] - 1) / cand[k]) * step_us[k] * 20.0 + 0.5);      // workgroup duration in ticks of 0.05 us
      cnt[k] = tiles[k] * cand[k];
      order[k] = k;
      if (cand[k] > 1) {
        slab_us += 2.0 * (double)slab_bytes(ls[k], cand[k]) / kSlabBytesPerUs;
        any = true;
      }
    }
    std::sort(order, order + n, [&](int a, int b) { return len[a] > len[b]; });
    int l2[kMaxConvGroup], c2[kMaxConvGroup];
    for (int k = 0; k < n; ++k) { l2[k] = len[order[k]]; c2[k] = cnt[order[k]]; }
    const double us = group_makespan(l2, c2, n, tile_of(cfg).slots) * 0.05 + slab_us + (any ? 6.0 : 0.0);      // + the finalize launch
    if (us < best) { best = us; for (int k = 0; k < n; ++k) best_sk[k] = cand[k]; }
  }
  for (int k = 0; k < n; ++k) sk[k] = best_sk[k];
}

// Split-K factors of the members of a group.  A member's own bound (group_pick_splitk) assumes the group fills the chip; when
// the whole group is short of that (small batches: every member is a few tiles), K is cut further so that the group's
// workgroups come to about the chip's slots, each with >= 8 K steps - what conv_pick_splitk does for a launch of its own.
static void group_splitks(const ConvLaunch* ls, int n, int cfg, int* sk) {
  const int slots = tile_of(cfg).slots;     // workgroups the chip holds (256 x 256: one per CU, the 128-row tiles: two)
  int tiles[kMaxConvGroup], KT[kMaxConvGroup];
  long long steps = 0, wgs = 0, wg1 = 0;
  for (int k = 0; k < n; ++k) {
    tiles[k] = ConvGeom(ls[k]).tiles(tile_of(group_member_cfg(cfg, ls[k])));
    KT[k] = ConvGeom(ls[k]).KT;
    wg1 += tiles[k];
  }
  // the schedule model assumes a launch that can fill the chip; below that (small batches: every member is a few tiles) the
  // per-member rule that follows measured better (batch 1, six levels: 271 vs 291 us)
  if ((cfg == kGroupMixed || cfg == kCfgIgemm256) && wg1 * 2 >= slots) return group_splitks_scheduled(ls, n, cfg, sk);
  for (int k = 0; k < n; ++k) {
    const ConvLaunch& c = ls[k];
    sk[k] = (c.up > 0 || c.pool) ? 1 : (c.splitk >= 0 ? std::max(c.splitk, 1) : group_pick_splitk(KT[k], tiles[k]));
    steps += (long long)tiles[k] * KT[k];
    wgs += (long long)tiles[k] * sk[k];
  }
  if (wgs * 4 > slots * 3) return;                       // the group (nearly) fills the chip as it is
  const int per_wg = (int)std::max<long long>(8, (steps + slots - 1) / slots);      // K steps per workgroup to aim for
  for (int k = 0; k < n; ++k) {
    const ConvLaunch& c = ls[k];
    if (c.up > 0 || c.pool || c.splitk >= 0 || KT[k] < 16) continue;
    const int want = std::min(KT[k] / 8, std::max(1, KT[k] / per_wg));
    if (want > sk[k]) sk[k] = want;
  }
}

static int64_t group_slab_bytes(const ConvLaunch& c, int sk) { return sk > 1 ? ron::align_up(slab_bytes(c, sk), 256) : 0; }

int64_t conv_group_scratch_bytes(const ConvLaunch* ls, int n, int cfg, const int* sk_plan) {
  int64_t total = 0;
  if (cfg == kCfgPatch64) {                      // a pair of the patch kernel, or each launch on its own
    for (int k = 0; k < n; ++k) total = std::max(total, conv_scratch_bytes(ls[k]));
    return total;
  }
  if (n < 1 || n > kMaxConvGroup) return 0;
  int sk[kMaxConvGroup];
  if (sk_plan != nullptr) for (int k = 0; k < n; ++k) sk[k] = sk_plan[k];
  else group_splitks(ls, n, cfg, sk);
  for (int k = 0; k < n; ++k) total += group_slab_bytes(ls[k], sk[k]);
  return total;
}

void conv_group_plan(const ConvLaunch* ls, int n, int cfg, int* sk) {
  if (cfg == kCfgPatch64 || n < 1 || n > kMaxConvGroup) { for (int k = 0; k < n && k < kMaxConvGroup; ++k) sk[k] = 1; return; }
  group_splitks(ls, n, cfg, sk);
}

// `n` mutually independent convolutions as one launch of tile configuration `cfg` (kCfgIgemm128x64, kCfgIgemm128, kCfgIgemm256, or
// kGroupMixed: each member on the 128-row tile of its own width);
// `scratch`: conv_group_scratch_bytes() for the split-K slabs (each conv gets its own part).
int launch_conv_group(const ConvLaunch* ls_in, int n, int cfg, void* scratch, int64_t scratch_bytes, hipStream_t stream, const int* sk_plan,
                      int* n_tiles) {
  RON_REQUIRE(n >= 1 && n <= kMaxGroup, "conv group: %d launches (1..%d)", n, kMaxGroup);
  for (int k = 0; k < n; ++k) RON_REQUIRE(ls_in[k].split_n == 0, "conv group: a two-output convolution is a launch of its own");
  if (cfg == kCfgPatch64) {
    // the two skinny heads of a scale: one launch of the patch kernel where it is the choice for both (dtype, map, batch),
    // otherwise each as the launch it would be on its own
    RON_REQUIRE(n == 2, "conv group: the patch-kernel form takes a pair");
    if (conv_patch_pair_applicable(ls_in[0], ls_in[1])) return launch_conv_patch_pair(ls_in[0], ls_in[1], stream);
    for (int k = 0; k < n; ++k)
      if (const int rc = launch_conv(ls_in[k], stream)) return rc;
    return RON_OK;
  }
  RON_REQUIRE(cfg == kCfgIgemm128x64 || cfg == kCfgIgemm128 || cfg == kGroupMixed || cfg == kCfgIgemm256,
              "conv group: tile config %d has no grouped form", cfg);
  ConvGroupArgs g = ConvGroupArgs();
  g.n = n;
  int64_t used = 0;
  bool any_split = false;
  int sks_in[kMaxConvGroup], order[kMaxConvGroup], chain[kMaxConvGroup];
  if (sk_plan != nullptr) for (int k = 0; k < n; ++k) sks_in[k] = sk_plan[k];
  else group_splitks(ls_in, n, cfg, sks_in);
  // workgroups are dispatched in blockIdx order: the members with the longest K chains per workgroup go first, the short ones fill
  // the slots the long ones leave (members are independent: their order is free); the 256 x 256 group runs on the four-wave tiles
  // (which decode panel tile orders) when every member's K chain fits their step table
  bool group_4w = cfg == kCfgIgemm256 && ls_in[0].dtype != RON_DTYPE_F32;
  for (int k = 0; k < n; ++k) {
    order[k] = k;
    chain[k] = (ConvGeom(ls_in[k]).KT + sks_in[k] - 1) / std::max(sks_in[k], 1);
    group_4w = group_4w && asm_loop_ok(chain[k]);
  }
  if (cfg == kGroupMixed || cfg == kCfgIgemm256) std::stable_sort(order, order + n, [&](int a, int b) { return chain[a] > chain[b]; });
  for (int k = 0; k < n; ++k) {
    const ConvLaunch& c = ls_in[order[k]];
    const int mcfg = group_member_cfg(cfg, c), sk = sks_in[order[k]];
    int bn = 0;
    RON_REQUIRE(c.dtype == ls_in[0].dtype, "conv group: mixed dtypes");
    RON_REQUIRE(c.Npad % tile_of(mcfg).bn == 0 && !c.pool, "conv group: Npad %d not a multiple of the N tile %d, or a fused pool", c.Npad,
                tile_of(mcfg).bn);
    if (const int rc = check_conv_fields(c)) return rc;
    const int64_t need = group_slab_bytes(c, sk);
    const bool fits = need > 0 && scratch != nullptr && used + need <= scratch_bytes;
    if (const int rc = plan_member("conv group", c, mcfg, sk, fits ? static_cast<char*>(scratch) + used : nullptr, fits ? need : 0, group_4w, true,
                                   g.op[k], &bn)) return rc;
    if (g.op[k].splitk > 1) { used += need; any_split = true; }
    // ConvGroupArgs::narrow, bit k: member k on the 128 x 64 tile (a mixed group), or on the 256 x 224 tile (a four-wave 256 x 256 group)
    if (mcfg == kCfgIgemm128x64 || bn == 224) g.narrow |= 1u << k;
    if (n_tiles != nullptr) n_tiles[order[k]] = bn;
  }
  // entries, longest K chain first (see ConvGroupArgs)
  struct Ent { int op, bid0, cnt, chain; };
  Ent ents[kMaxEntries];
  int ne = 0;
  for (int k = 0; k < n; ++k) {
    const ConvArgs& a = g.op[k];
    const int total = a.tiles_total * a.splitk;
    if (a.center_from_n > 0 && a.splitk == 1) {
      const int BN = tile_of(group_member_cfg(cfg, ls_in[order[k]])).bn;
      const int n_long = (a.tiles_total / a.tiles_n) * (a.center_from_n / BN);
      ents[ne++] = Ent{k, 0, n_long, a.KT};
      ents[ne++] = Ent{k, n_long, total - n_long, a.Cin / conv_k_chunk(ls_in[0].dtype)};
    } else {
      ents[ne++] = Ent{k, 0, total, a.kt_split};
    }
  }
  std::stable_sort(ents, ents + ne, [](const Ent& x, const Ent& y) { return x.chain > y.chain; });
  g.ne = ne;
  for (int e = 0; e < ne; ++e) {
    g.eop[e] = ents[e].op; g.ebid0[e] = ents[e].bid0; g.enwg[e] = g.op[ents[e].op].tiles_total * g.op[ents[e].op].splitk;
    g.first[e + 1] = g.first[e] + ents[e].cnt;
  }
  return with_traits(ls_in[0].dtype, "conv group",
                     [&](auto tag) { return launch_group_cfg<typename decltype(tag)::type>(cfg, g, any_split, stream); });
}

int64_t conv_scratch_bytes(const ConvLaunch& c) {
  const int cfg = c.cfg >= 0 ? c.cfg : conv_pick_cfg(c);
  if (conv_cfg_is_patch(cfg) || c.up > 0 || c.pool) return 0;      // the halo-patch kernel never splits K
  const int sk = single_splitk(c, cfg);
  return sk > 1 ? slab_bytes(c, sk) : 0;
}

}  // namespace ron
