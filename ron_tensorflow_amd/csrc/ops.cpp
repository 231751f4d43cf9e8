// Single-operator entry points (ron_conv2d_nhwc, ron_maxpool2x2_nhwc): the same kernels the
// graph launches, wrapped with dense-fp32 <-> halo-tensor conversion so that the parity tests
// can pin each kernel against the oracle.  They allocate scratch and synchronise: test/tool use.
// conv_launch_geometry (conv_mfma.h) is here too: the launch geometry of a descriptor, which the training forward shares.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pack.h"

void ron::conv_launch_geometry(const ron_conv_desc* d, ConvLaunch* c, int* ho, int* wo) {
  c->dtype = d->dtype;
  c->relu = d->relu;
  if (d->transpose) {
    *ho = d->h * d->stride; *wo = d->w * d->stride;
    c->Cout = c->Npad = d->kh * d->kw * d->cout;
    c->up = d->stride; c->up_cout = d->cout;
    c->kh = c->kw = 1; c->stride = 1; c->dil = 1; c->cpad = 0;
    c->Ho = d->h; c->Wo = d->w;
    return;
  }
  const bool stem = d->cin == 3 && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->dilation == 1;
  *ho = d->h / d->stride; *wo = d->w / d->stride;
  c->Cout = d->cout;
  c->Npad = round_up(d->cout, conv_n_tile(d->cout));
  c->kh = stem ? 1 : d->kh; c->kw = stem ? 1 : d->kw;
  c->stride = d->stride; c->dil = d->dilation;
  c->cpad = stem || d->stride != 1 ? 0 : (d->kh - 1) * d->dilation / 2;      // SAME
  c->Ho = *ho; c->Wo = *wo;
}

namespace {

using ron::DevBuf;

int alloc(DevBuf* b, int64_t bytes, bool zero) {
  RON_HIP_CHECK(ron::dev_malloc(b->put(), (size_t)bytes));
  if (zero) RON_HIP_CHECK(ron::dev_memset(b->p, 0, (size_t)bytes));
  return RON_OK;
}

ron::TensorView make_view(void* base, int n, int h, int w, int c, int pad, int esz) {
  ron::TensorView v;
  v.base = base; v.N = n; v.H = h; v.W = w; v.C = c; v.pad = pad; v.cstride = c; v.coff = 0;
  v.bytes = ron::TensorView::halo_pixels(n, h, w, pad) * c * esz;
  return v;
}

struct ConvSetup {
  ron::ConvLaunch c;
  DevBuf d_w, d_w_c64, d_b, d_in, d_out, d_res, d_scratch;
  int ho = 0, wo = 0;
  bool is_c3 = false;
};

// Packs weights like ron_finalize_weights does, uploads them and allocates the halo tensors.
int setup_conv(const ron_conv_desc* d, const float* w, const float* bias, bool with_residual, ConvSetup* S) {
  using namespace ron;
  // the descriptor itself, before any arithmetic on it (a stride of 0 used to reach the divisions below)
  {
    const int rc = check_conv_desc(d);
    if (rc != RON_OK) return rc;
  }
  RON_REQUIRE(d->dtype >= 0 && d->dtype <= RON_DTYPE_F16X3, "bad dtype");
  RON_REQUIRE(d->kh == d->kw, "conv: filter %d x %d: square filters only (one SAME padding for both axes)", d->kh, d->kw);
  // an even filter's SAME padding is one pixel wider behind than in front: the shared halo has one width, so it is refused
  RON_REQUIRE(d->transpose || d->stride > 1 || (d->kh & 1), "conv: %d x %d filter at stride 1: odd filters only", d->kh, d->kw);
  const int esz = (int)dtype_size(d->dtype);
  const int chunk = conv_k_chunk(d->dtype);
  S->is_c3 = (!d->transpose && d->cin == 3 && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->dilation == 1);
  RON_REQUIRE(S->is_c3 || d->cin % chunk == 0, "cin %d must be a multiple of %d (or the 3-channel 3x3 stem)", d->cin, chunk);
  ConvLaunch& c = S->c;
  c.cfg = d->tile_cfg;
  if (d->transpose) {
    RON_REQUIRE(d->kh == d->kw && d->kh == d->stride && d->dilation == 1, "transposed conv needs kernel == stride");
    RON_REQUIRE(d->cout % 128 == 0, "transposed conv: cout %d must be a multiple of 128", d->cout);
  } else {
    RON_REQUIRE(d->stride == 1 || (d->h % d->stride == 0 && d->w % d->stride == 0 && d->kh == d->stride),
                "strided conv: only kernel == stride on divisible maps");
  }
  conv_launch_geometry(d, &c, &S->ho, &S->wo);
  const int cpad = c.cpad;
  std::vector<float> rows;
  std::vector<float> bias_pad(c.Npad, 0.f);
  if (d->transpose) {
    // TF layout [kh,kw,cout,cin] -> rows[(t*cout + co)][ci]
    rows.assign((size_t)c.Npad * d->cin, 0.f);
    memcpy(rows.data(), w, rows.size() * sizeof(float));
    if (bias) for (int t = 0; t < d->kh * d->kw; ++t) for (int co = 0; co < d->cout; ++co) bias_pad[t * d->cout + co] = bias[co];
  } else {
    if (S->is_c3) {
      rows.assign((size_t)c.Npad * chunk, 0.f);
      for (int k = 0; k < 27; ++k) for (int n = 0; n < d->cout; ++n) rows[(size_t)n * chunk + k] = w[(size_t)k * d->cout + n];
    } else {
      hwio_to_rows(w, d->kh, d->kw, d->cin, d->cout, c.Npad, &rows);
    }
    if (bias) for (int n = 0; n < d->cout; ++n) bias_pad[n] = bias[n];
  }
  std::vector<uint8_t> wbytes = pack_conv_weights(rows, c.Npad, d->dtype, &c.oscale);
  int rc;
  RON_HIP_CHECK(dev_upload(&S->d_w, wbytes.data(), wbytes.size()));
  RON_HIP_CHECK(dev_upload(&S->d_b, bias_pad.data(), bias_pad.size() * 4));
  c.wgt = S->d_w.p; c.wgt_bytes = (int64_t)wbytes.size(); c.bias = (const float*)S->d_b.p;
  if (conv_c64_wants_images(d->dtype, d->kh, d->kw, d->cin, d->cout, c.Npad)) {      // (no transposed convolution: Npad = 9 cout there)
    // what ron_finalize_weights adds for such a layer: the weights once more as LDS images for the resident-weight kernel
    const std::vector<uint8_t> img = pack_conv_c64_weights(rows, c.Npad, d->dtype);
    RON_HIP_CHECK(dev_upload(&S->d_w_c64, img.data(), img.size()));
    c.wgt_c64 = S->d_w_c64.p;
  }
  if (S->is_c3) c.in = make_view(nullptr, d->n, d->h, d->w, chunk, 0, esz);
  else {
    const int cs = d->in_cstride > 0 ? d->in_cstride : d->cin;
    RON_REQUIRE(d->in_coff >= 0 && d->in_coff + d->cin <= cs, "bad channel slice");
    c.in = make_view(nullptr, d->n, d->h, d->w, cs, cpad, esz);     // allocation of the wide tensor
    c.in.C = d->cin;
    c.in.coff = d->in_coff;
  }
  if ((rc = alloc(&S->d_in, c.in.bytes, true))) return rc;
  c.in.base = S->d_in.p;
  c.pool = d->pool;
  if (d->pool) { S->ho = (S->ho + 1) / 2; S->wo = (S->wo + 1) / 2; }     // SAME pool: ceil
  // halo 1: exercises padded stores.  Split precision: pixels are whole 32-element (128-byte) chunks
  c.out = make_view(nullptr, d->n, S->ho, S->wo, d->dtype == RON_DTYPE_F16X3 ? round_up(d->cout, 32) : d->cout, 1, esz);
  c.out.C = d->cout;
  if ((rc = alloc(&S->d_out, c.out.bytes, true))) return rc;
  c.out.base = S->d_out.p;
  if (with_residual) {
    if ((rc = alloc(&S->d_res, c.out.bytes, true))) return rc;
    c.res = S->d_res.p;
  }
  c.splitk = d->splitk;
  // tests / sweeps: RON_IGEMM224=0 keeps 193 .. 224 output channels on 256-column tiles (ConvLaunch::n224), read per call so that
  // one process can run both forms; the graph does not read it
  if (const char* e = getenv("RON_IGEMM224")) { if (atoi(e) == 0) c.n224 = 0; }
  c.center_from = d->transpose ? 0 : d->center_from;
  const int64_t sb = conv_scratch_bytes(c);
  if (sb > 0) {
    if ((rc = alloc(&S->d_scratch, sb, false))) return rc;
    c.scratch = S->d_scratch.p;
    c.scratch_bytes = sb;
  }
  return RON_OK;
}

}  // namespace

extern "C" int ron_conv2d_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* bias,
                               const float* residual, float* y, void* stream) {
  using namespace ron;
  RON_REQUIRE(d && x && w && y, "NULL argument");
  hipStream_t s = (hipStream_t)stream;
  ConvSetup S;
  int rc;
  if ((rc = setup_conv(d, w, bias, residual != nullptr, &S))) return rc;
  // conv1_1 through the dedicated stem kernel (what the graph runs for bf16 / f16 / f16x3):
  //   * widths that are a multiple of 32 keep the routing they always had here: bf16 / f16 take the stem kernel, f16x3 im2col + GEMM
  //     (the comparison path of the tests);
  //   * a ragged width (which the stem kernel used to refuse, so it went to im2col + GEMM) takes the stem kernel in all three dtypes
  //     unless the caller forces a tile configuration, which selects im2col + GEMM;
  //   * with `pool` set the launch is im2col + GEMM with the fused pool (the stem kernel has no pool; this branch once ignored the flag).
  const bool stem_shape = S.is_c3 && d->cout == 64 && d->relu && !residual && !d->pool;
  const bool full_tiles = d->w % 32 == 0;
  const bool stem_dtype = full_tiles ? dtype_is_half(d->dtype) : (dtype_is_half(d->dtype) || d->dtype == RON_DTYPE_F16X3);
  const bool stem_forced_off = !full_tiles && d->tile_cfg >= 0;
  if (stem_shape && stem_dtype && !stem_forced_off) {
    std::vector<uint16_t> frags;
    float oscale = 1.f;
    if (d->dtype == RON_DTYPE_F16X3) oscale = stem_pack_weights_split(w, &frags);
    else stem_pack_weights(w, d->dtype, &frags);
    std::vector<float> b64(64, 0.f);
    if (bias) memcpy(b64.data(), bias, 64 * sizeof(float));
    DevBuf d_f, d_bb;
    RON_HIP_CHECK(dev_upload(&d_f, frags.data(), frags.size() * 2));
    RON_HIP_CHECK(dev_upload(&d_bb, b64.data(), 64 * 4));
    if ((rc = launch_stem_conv(x, d->n, d->h, d->w, d->dtype, d_f.p, (const float*)d_bb.p, S.c.out, s, oscale))) return rc;
    if ((rc = launch_unpack(S.c.out, d->dtype, 0, y, s))) return rc;
    RON_HIP_CHECK(dev_stream_sync(s));
    return RON_OK;
  }
  if (S.is_c3) {
    if ((rc = launch_im2col_c3(x, d->n, d->h, d->w, d->dtype, S.d_in.p, S.c.in.C, s))) return rc;
  } else {
    if ((rc = launch_pack_input(x, S.c.in, d->dtype, s))) return rc;
  }
  if (residual) {
    TensorView rv = S.c.out;
    rv.base = S.d_res.p;
    if ((rc = launch_pack_input(residual, rv, d->dtype, s))) return rc;
  }
  if ((rc = launch_conv(S.c, s))) return rc;
  if ((rc = launch_unpack(S.c.out, d->dtype, 0, y, s))) return rc;
  RON_HIP_CHECK(dev_stream_sync(s));
  return RON_OK;
}

// conv + fused SAME pool with the un-pooled map as the launch's second output (ConvLaunch::out2): what the graph does for conv4_3 /
// conv5_3 under RON_CFG_FUSE_POOLS, as a single operator for the parity tests.
extern "C" int ron_conv2d_pool2_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* bias, float* y_pooled,
                                     float* y_full, void* stream) {
  using namespace ron;
  RON_REQUIRE(d && x && w && y_pooled && y_full, "NULL argument");
  if (int rc0 = check_conv_desc(d)) return rc0;
  RON_REQUIRE(d->pool && !d->transpose && d->stride == 1 && d->cin % conv_k_chunk(d->dtype) == 0, "two-output pooled convolution: a plain stride-1 convolution with pool set");
  hipStream_t s = (hipStream_t)stream;
  ConvSetup S;
  int rc;
  if ((rc = setup_conv(d, w, bias, false, &S))) return rc;
  ConvLaunch& c = S.c;
  DevBuf d_full;
  c.out2 = make_view(nullptr, d->n, d->h, d->w, c.out.cstride, 1, (int)dtype_size(d->dtype));
  c.out2.C = d->cout;
  if ((rc = alloc(&d_full, c.out2.bytes, true))) return rc;
  c.out2.base = d_full.p;
  if ((rc = launch_pack_input(x, c.in, d->dtype, s))) return rc;
  if ((rc = launch_conv(c, s))) return rc;
  if ((rc = launch_unpack(c.out, d->dtype, 0, y_pooled, s))) return rc;
  if ((rc = launch_unpack(c.out2, d->dtype, 0, y_full, s))) return rc;
  RON_HIP_CHECK(dev_stream_sync(s));
  return RON_OK;
}

// How ron_conv2d_nhwc would launch `d` (no launch): the decisions of launch_conv for the same ConvLaunch.
static int plan_of_desc(const ron_conv_desc* d, int o[4], int* n_tile) {
  using namespace ron;
  RON_REQUIRE(!(d->cin == 3), "the 3-channel stem has a kernel of its own");
  if (int rc0 = check_conv_desc(d)) return rc0;       // (before the weights are sized from it)
  const size_t wn = (size_t)d->kh * d->kw * d->cin * d->cout;
  std::vector<float> w(wn, 0.f);
  ConvSetup S;
  int rc;
  if ((rc = setup_conv(d, w.data(), nullptr, false, &S))) return rc;
  return conv_describe(S.c, o, n_tile);
}

extern "C" int ron_conv_plan(const ron_conv_desc* d, int32_t out[4]) {
  RON_REQUIRE(d != nullptr && out != nullptr, "NULL argument");
  int o[4];
  if (int rc = plan_of_desc(d, o, nullptr)) return rc;
  for (int i = 0; i < 4; ++i) out[i] = o[i];
  return RON_OK;
}

// ... and the width of the row-gather kernel's column tile for the same launch (conv_describe)
extern "C" int ron_conv_plan_n_tile(const ron_conv_desc* d, int32_t* n_tile) {
  RON_REQUIRE(d != nullptr && n_tile != nullptr, "NULL argument");
  int o[4], bn = 0;
  if (int rc = plan_of_desc(d, o, &bn)) return rc;
  *n_tile = bn;
  return RON_OK;
}

// One or two head convolutions with the fp32 output the graph's head layers have (ConvLaunch::out_f32: the kernel's epilogue writes
// the dense fp32 tensor itself), each over its own input: as launches of their own, or as the two members of one grouped launch of
// 256 x 256 tiles (launch_conv_group, kCfgIgemm256: what the batch plan does with the class heads of the coarse scales).
extern "C" int ron_conv2d_f32out_nhwc(const ron_conv_desc* da, const float* xa, const float* wa, const float* ba, float* ya,
                                      const ron_conv_desc* db, const float* xb, const float* wb, const float* bb, float* yb,
                                      int grouped, int32_t* n_tiles, void* stream) {
  using namespace ron;
  RON_REQUIRE(da && xa && wa && ya, "NULL argument");
  RON_REQUIRE(db == nullptr || (xb && wb && yb), "NULL argument (second convolution)");
  RON_REQUIRE(!grouped || db != nullptr, "a grouped launch takes two convolutions");
  hipStream_t s = (hipStream_t)stream;
  const ron_conv_desc* ds[2] = {da, db};
  const float* xs[2] = {xa, xb};
  const float* ws[2] = {wa, wb};
  const float* bs[2] = {ba, bb};
  float* ys[2] = {ya, yb};
  const int n = db != nullptr ? 2 : 1;
  ConvSetup S[2];
  ConvLaunch L[2];
  int rc;
  for (int k = 0; k < n; ++k) {
    const ron_conv_desc* d = ds[k];
    if (int rc0 = check_conv_desc(d)) return rc0;
    RON_REQUIRE(!d->transpose && !d->pool && d->center_from == 0 && d->stride == 1 && d->cin % conv_k_chunk(d->dtype) == 0,
                "fp32-output convolution: a plain stride-1 convolution");
    // the grouped launch has one tile configuration, the 256 x 256 one: a descriptor that asks for another is refused, not ignored
    RON_REQUIRE(!grouped || d->tile_cfg < 0 || d->tile_cfg == kCfgIgemm256, "grouped fp32-output convolutions: tile_cfg %d (-1 or %d)", d->tile_cfg, kCfgIgemm256);
    if ((rc = setup_conv(d, ws[k], bs[k], false, &S[k]))) return rc;
    RON_REQUIRE(!grouped || S[k].c.Npad % 256 == 0, "grouped fp32-output convolutions: cout %d pads to %d, not a multiple of 256", d->cout, S[k].c.Npad);
    ConvLaunch& c = S[k].c;
    TensorView v;
    v.base = ys[k]; v.N = d->n; v.H = S[k].ho; v.W = S[k].wo; v.pad = 0; v.coff = 0; v.C = d->cout; v.cstride = d->cout;
    v.bytes = (int64_t)d->n * S[k].ho * S[k].wo * d->cout * 4;
    c.out = v;
    c.out_f32 = 1;
    if ((rc = launch_pack_input(xs[k], c.in, d->dtype, s))) return rc;
    L[k] = c;
  }
  // (after the first launch an error return waits for the stream first: the operands are freed on the way out)
  DevBuf scratch;
  int widths[2] = {0, 0};
  if (!grouped) {
    for (int k = 0; k < n; ++k) {
      int o[4];
      if ((rc = conv_describe(L[k], o, &widths[k])) || (rc = launch_conv(L[k], s))) { (void)dev_stream_sync(s); return rc; }
    }
  } else {
    // split factors: the descriptors' where both give one (>= 1), else the group's own plan
    int sk[2] = {da->splitk, db->splitk};
    const int* plan = (sk[0] >= 1 && sk[1] >= 1) ? sk : nullptr;
    for (int k = 0; k < 2; ++k) { L[k].scratch = nullptr; L[k].scratch_bytes = 0; L[k].splitk = plan ? sk[k] : -1; }
    const int64_t sb = conv_group_scratch_bytes(L, 2, kCfgIgemm256, plan);
    if (sb > 0 && (rc = alloc(&scratch, sb, false))) { (void)dev_stream_sync(s); return rc; }
    if ((rc = launch_conv_group(L, 2, kCfgIgemm256, scratch.p, sb, s, plan, widths))) { (void)dev_stream_sync(s); return rc; }
  }
  RON_HIP_CHECK(dev_stream_sync(s));
  if (n_tiles != nullptr) for (int k = 0; k < n; ++k) n_tiles[k] = widths[k];
  return RON_OK;
}

// The skinny heads of a scale as the graph launches them at large batches: two 3x3 convolutions of at most 64 output channels over
// channel slices of ONE tensor, one launch of the halo-patch pair kernel (64-column configuration, whatever the grid size), fp32 outputs.
extern "C" int ron_conv2d_patch_pair_nhwc(const ron_conv_desc* da, const ron_conv_desc* db, const float* x, const float* wa, const float* ba,
                                          const float* wb, const float* bb, float* ya, float* yb, int full_width, int32_t* columns,
                                          void* stream) {
  using namespace ron;
  RON_REQUIRE(da && db && x && wa && wb && ya && yb, "NULL argument");
  if (int rc0 = check_conv_desc(da)) return rc0;
  if (int rc0 = check_conv_desc(db)) return rc0;
  RON_REQUIRE(da->n == db->n && da->h == db->h && da->w == db->w && da->cin == db->cin && da->dtype == db->dtype &&
              da->in_cstride > 0 && da->in_cstride == db->in_cstride, "patch pair: the two convolutions read slices of one tensor");
  hipStream_t s = (hipStream_t)stream;
  const ron_conv_desc* ds[2] = {da, db};
  const float* ws[2] = {wa, wb};
  const float* bs[2] = {ba, bb};
  float* ys[2] = {ya, yb};
  ConvSetup S[2];
  int rc;
  for (int k = 0; k < 2; ++k) {
    const ron_conv_desc* d = ds[k];
    RON_REQUIRE(!d->transpose && !d->pool && d->center_from == 0 && d->stride == 1 && d->dilation == 1 && d->kh == 3 && d->kw == 3 &&
                d->cout <= 64 && d->cin % conv_k_chunk(d->dtype) == 0, "patch pair: plain 3x3 convolutions of at most 64 output channels");
    if ((rc = setup_conv(d, ws[k], bs[k], false, &S[k]))) return rc;
    ConvLaunch& c = S[k].c;
    TensorView v;
    v.base = ys[k]; v.N = d->n; v.H = S[k].ho; v.W = S[k].wo; v.pad = 0; v.coff = 0; v.C = d->cout; v.cstride = d->cout;
    v.bytes = (int64_t)d->n * S[k].ho * S[k].wo * d->cout * 4;
    c.out = v;
    c.out_f32 = 1;
    if (full_width) c.n224 = 0;
  }
  S[1].c.in.base = S[0].c.in.base;              // one tensor: the second convolution's own allocation stays unused
  TensorView wide = S[0].c.in;
  wide.C = da->in_cstride; wide.coff = 0;
  if ((rc = launch_pack_input(x, wide, da->dtype, s))) return rc;
  int cols[2];
  conv_patch_pair_columns(S[0].c, S[1].c, cols);
  if (columns != nullptr) { columns[0] = cols[0]; columns[1] = cols[1]; }
  rc = launch_conv_patch_pair(S[0].c, S[1].c, s, kCfgPatch64);
  RON_HIP_CHECK(dev_stream_sync(s));
  return rc;
}

// Two fp32 head tensors from ONE convolution over a shared input (ConvLaunch::split_n; the graph's pack_box_pair for the class and box
// convolutions of an SSD feature layer): the same packing - first head's columns, the second's from the next multiple of 8 - and
// the same launch, with the tile configuration and the split-K factor the caller's to force.
extern "C" int ron_conv2d_heads_nhwc(const ron_conv_desc* d, int split_first, const float* x, const float* w, const float* bias,
                                     float* y_first, float* y_second, void* stream) {
  using namespace ron;
  RON_REQUIRE(d && x && w && y_first && y_second, "NULL argument");
  if (int rc0 = check_conv_desc(d)) return rc0;
  RON_REQUIRE(!d->transpose && !d->pool && d->center_from == 0 && d->stride == 1 && d->cin % conv_k_chunk(d->dtype) == 0,
              "two-output convolution: a plain stride-1 convolution");
  RON_REQUIRE(split_first > 0 && split_first < d->cout, "two-output convolution: %d of %d channels in the first output", split_first, d->cout);
  hipStream_t s = (hipStream_t)stream;
  const int n_second = d->cout - split_first, split_n = round_up(split_first, 8);
  // the packed convolution: `split_n + n_second` columns, the ones between the two heads zero
  ron_conv_desc dp = *d;
  dp.cout = split_n + n_second;
  const int K = d->kh * d->kw * d->cin;
  std::vector<float> wp((size_t)K * dp.cout, 0.f), bp(dp.cout, 0.f);
  for (int k = 0; k < K; ++k) {
    for (int n = 0; n < split_first; ++n) wp[(size_t)k * dp.cout + n] = w[(size_t)k * d->cout + n];
    for (int n = 0; n < n_second; ++n) wp[(size_t)k * dp.cout + split_n + n] = w[(size_t)k * d->cout + split_first + n];
  }
  if (bias) {
    for (int n = 0; n < split_first; ++n) bp[n] = bias[n];
    for (int n = 0; n < n_second; ++n) bp[split_n + n] = bias[split_first + n];
  }
  ConvSetup S;
  int rc;
  if ((rc = setup_conv(&dp, wp.data(), bp.data(), false, &S))) return rc;
  ConvLaunch& c = S.c;
  TensorView v;
  v.base = y_first; v.N = d->n; v.H = S.ho; v.W = S.wo; v.pad = 0; v.coff = 0; v.C = split_first; v.cstride = split_first;
  v.bytes = (int64_t)d->n * S.ho * S.wo * split_first * 4;
  c.out = v;
  v.base = y_second; v.C = n_second; v.cstride = n_second;
  v.bytes = (int64_t)d->n * S.ho * S.wo * n_second * 4;
  c.out2 = v;
  c.out_f32 = 1;
  c.split_n = split_n; c.split_first = split_first;
  // (setup_conv sized the split-K scratch for a one-output launch, which may have gone to a kernel that never splits)
  DevBuf scratch2;
  const int64_t sb = conv_scratch_bytes(c);
  if (sb > c.scratch_bytes) {
    if ((rc = alloc(&scratch2, sb, false))) return rc;
    c.scratch = scratch2.p;
    c.scratch_bytes = sb;
  }
  if ((rc = launch_pack_input(x, c.in, d->dtype, s))) return rc;
  if ((rc = launch_conv(c, s))) return rc;
  RON_HIP_CHECK(dev_stream_sync(s));
  return RON_OK;
}

// Times the conv kernel alone on random data (tools/sweep_conv.py): ms per launch over `iters` launches.
extern "C" int ron_conv2d_bench(const ron_conv_desc* d, int warmup, int iters, float* ms_per_launch) {
  using namespace ron;
  RON_REQUIRE(d && ms_per_launch && iters > 0 && warmup >= 0, "bad argument");
  RON_REQUIRE(!(d->cin == 3), "the 3-channel stem is not benchmarked through this entry");
  if (int rc0 = check_conv_desc(d)) return rc0;
  const size_t wn = (size_t)d->kh * d->kw * d->cin * d->cout;
  std::vector<float> w(wn), b(d->cout);
  uint32_t st = 12345u;
  auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xFFFF) / 32768.f - 1.f; };
  const float scale = 1.f / sqrtf((float)(d->kh * d->kw * d->cin));
  // RON_BENCH_ZERO=1 (tools/sweep_conv.py --zeros): all-zero operands instead of random ones - the same instruction stream at the
  // clock the chip holds when the data paths do not toggle (MI355X_MICROARCH.md, DVFS): how much of a kernel's time is power
  const bool zeros = getenv("RON_BENCH_ZERO") != nullptr;
  for (auto& v : w) v = zeros ? 0.f : rnd() * scale;
  for (auto& v : b) v = zeros ? 0.f : rnd() * 0.1f;
  ConvSetup S;
  int rc;
  if ((rc = setup_conv(d, w.data(), b.data(), false, &S))) return rc;
  if (!zeros && (rc = launch_fill_random(S.c.in, d->dtype, 777u, nullptr))) return rc;
  Event e0, e1;
  RON_HIP_CHECK(hipEventCreate(e0.put()));
  RON_HIP_CHECK(hipEventCreate(e1.put()));
  for (int i = 0; i < warmup; ++i) if ((rc = launch_conv(S.c, nullptr))) return rc;
  RON_HIP_CHECK(hipEventRecord(e0, nullptr));
  for (int i = 0; i < iters; ++i) if ((rc = launch_conv(S.c, nullptr))) return rc;
  RON_HIP_CHECK(hipEventRecord(e1, nullptr));
  RON_HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  RON_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  *ms_per_launch = ms / iters;
  return RON_OK;
}

extern "C" int ron_maxpool2x2_nhwc(const float* x, int n, int h, int w, int c, int dtype, float* y, void* stream) {
  using namespace ron;
  RON_REQUIRE(x && y && n > 0 && h > 0 && w > 0 && c > 0, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int esz = (int)dtype_size(dtype);
  TensorView vin = make_view(nullptr, n, h, w, c, 1, esz);
  TensorView vout = make_view(nullptr, n, (h + 1) / 2, (w + 1) / 2, c, 3, esz);     // SAME: ceil
  DevBuf d_in, d_out;
  int rc;
  if ((rc = alloc(&d_in, vin.bytes, true))) return rc;
  if ((rc = alloc(&d_out, vout.bytes, true))) return rc;
  vin.base = d_in.p; vout.base = d_out.p;
  if ((rc = launch_pack_input(x, vin, dtype, s))) return rc;
  if ((rc = launch_maxpool2x2(vin, vout, dtype, s))) return rc;
  if ((rc = launch_unpack(vout, dtype, 0, y, s))) return rc;
  RON_HIP_CHECK(dev_stream_sync(s));
  return RON_OK;
}

// pool5 of SSD: the graph's launch_maxpool3x3s1 on packed tensors.  The kernel starts its maximum at 0 (the zero halo takes part), so
// it is slim.max_pool2d [3,3] stride 1 SAME for NON-NEGATIVE inputs only: what pool5 sees behind conv5_3's ReLU.
extern "C" int ron_maxpool3x3s1_nhwc(const float* x, int n, int h, int w, int c, int dtype, float* y, void* stream) {
  using namespace ron;
  RON_REQUIRE(x && y && n > 0 && h > 0 && w > 0 && c > 0, "bad argument");
  RON_REQUIRE(dtype >= 0 && dtype <= RON_DTYPE_F16X3, "bad dtype");
  hipStream_t s = (hipStream_t)stream;
  const int esz = (int)dtype_size(dtype);
  TensorView vin = make_view(nullptr, n, h, w, c, 1, esz);
  TensorView vout = make_view(nullptr, n, h, w, c, 1, esz);
  DevBuf d_in, d_out;
  int rc;
  if ((rc = alloc(&d_in, vin.bytes, true))) return rc;
  if ((rc = alloc(&d_out, vout.bytes, true))) return rc;
  vin.base = d_in.p; vout.base = d_out.p;
  if ((rc = launch_pack_input(x, vin, dtype, s))) return rc;
  if ((rc = launch_maxpool3x3s1(vin, vout, dtype, s))) return rc;
  if ((rc = launch_unpack(vout, dtype, 0, y, s))) return rc;
  RON_HIP_CHECK(dev_stream_sync(s));
  return RON_OK;
}

// block4 of SSD: the graph's launch_l2norm on packed tensors; gamma is a DEVICE fp32 vector [c], read as it stands
extern "C" int ron_l2norm_nhwc(const float* x, const float* gamma, int n, int h, int w, int c, int dtype, float* y, void* stream) {
  using namespace ron;
  RON_REQUIRE(x && gamma && y && n > 0 && h > 0 && w > 0 && c > 0, "bad argument");
  RON_REQUIRE(dtype >= 0 && dtype <= RON_DTYPE_F16X3, "bad dtype");
  hipStream_t s = (hipStream_t)stream;
  const int esz = (int)dtype_size(dtype);
  TensorView vin = make_view(nullptr, n, h, w, c, 1, esz);
  TensorView vout = make_view(nullptr, n, h, w, c, 1, esz);
  DevBuf d_in, d_out;
  int rc;
  if ((rc = alloc(&d_in, vin.bytes, true))) return rc;
  if ((rc = alloc(&d_out, vout.bytes, true))) return rc;
  vin.base = d_in.p; vout.base = d_out.p;
  if ((rc = launch_pack_input(x, vin, dtype, s))) return rc;
  if ((rc = launch_l2norm(vin, vout, gamma, dtype, s))) return rc;
  if ((rc = launch_unpack(vout, dtype, 0, y, s))) return rc;
  RON_HIP_CHECK(dev_stream_sync(s));
  return RON_OK;
}

extern "C" int ron_conv_num_tile_cfgs(void) { return ron::conv_num_cfgs(); }
