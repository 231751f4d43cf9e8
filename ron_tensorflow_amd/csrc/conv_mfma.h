// Host-side description of one implicit-GEMM convolution launch (see conv_mfma.hip).
#pragma once
#include <vector>

#include "common.h"

namespace ron {

// NHWC activation tensor in HBM with SHARED zero halos: rows are W + pad pixels long (the right halo of a row is the
// left halo of the next one), images are H + pad rows apart (the bottom halo of an image is the top halo of the next),
// one more band of `pad` rows + `pad` pixels closes the allocation.  Pixel (n, y, x) sits at row n*(H+pad) + pad + y,
// column pad + x; a tap that leaves the image lands in a halo pixel whichever side it leaves on, so the 3x3 / 7x7 /
// dilated taps never need a bounds check.  Kernels write interiors only; halos are zeroed once at allocation.
// The flat view matters to conv_patch.hip: positions that are consecutive in memory are consecutive pixels of the map
// with only `pad` halo pixels per row between them (4.8 % of a 40 x 40 map, not 9.3 %).
// Element type = the ctx dtype (bf16 / f16 / f32).  A view may address a channel slice [coff, coff + C) of a wider tensor.
struct TensorView {
  void* base = nullptr;      // start of the allocation (row 0, column 0, channel 0)
  int64_t bytes = 0;         // size of the allocation
  int N = 0, H = 0, W = 0, C = 0;
  int pad = 0;
  int cstride = 0;           // elements per pixel in memory
  int coff = 0;              // first channel of the view
  int Hp() const { return H + pad; }     // rows from one image to the next
  int Wp() const { return W + pad; }     // pixels per row
  int64_t pixels() const { return halo_pixels(N, H, W, pad); }
  static int64_t halo_pixels(int n, int h, int w, int pad) { return ((int64_t)n * (h + pad) + pad) * (w + pad) + pad; }
};

struct ConvLaunch {
  int dtype = RON_DTYPE_BF16;
  TensorView in, out;
  const void* res = nullptr;     // residual with the geometry of `out` (same dtype), or null
  const void* wgt = nullptr;     // packed [Npad][K] (K = kh*kw*Cin contiguous), dtype elements
  int64_t wgt_bytes = 0;
  const void* wgt_c64 = nullptr; // the same weights as LDS images for the resident-weight kernel (conv_c64.hip), or null
  const float* bias = nullptr;   // [Npad] fp32 (never null; zeros when the layer has none)
  float oscale = 1.f;            // out = acc * oscale + bias: 2^-k of the packed weights' scale (RON_DTYPE_F16X3), else 1
  int Cout = 0;                  // GEMM N that is stored (<= Npad)
  int Npad = 0;                  // rows of wgt, multiple of the N tile
  int kh = 1, kw = 1, stride = 1, dil = 1, cpad = 0;
  int relu = 0;
  int out_f32 = 0;               // store fp32 (head logits) instead of dtype
  // conv2d_transpose with kernel == stride == `up` (pixel shuffle epilogue); 0 = plain conv.
  int up = 0;
  int up_cout = 0;               // channels per tap of the transposed conv (Cout = up*up*up_cout)
  int Ho = 0, Wo = 0;            // GEMM rows = N*Ho*Wo (input grid for a transposed conv)
  int pool = 0;                  // fuse slim.max_pool2d [2,2] into the epilogue: `out` is the pooled map
  TensorView out2;               // with pool: the un-pooled map too (base == nullptr: none), same dtype, geometry Ho x Wo x Cout
  // Two fp32 outputs from one convolution (ConvArgs::split_n): packed columns [0, split_first) -> `out`, [split_n, Cout) -> `out2`,
  // both un-haloed fp32 views (out_f32 = 1).  Row-gather kernel only, a launch of its own; split-K allowed (the finalize pass routes the
  // columns the same way: block4 of SSD-512 at small batches splits).  0: one output.
  int split_n = 0, split_first = 0;
  int center_from = 0;           // > 0: output channels >= center_from have weights in the CENTRE tap only (a 1x1 branch packed beside
                                 // 3x3 ones: nets/ron_vgg_320.py:378-397); their column tiles run that tap's K steps alone
  int n224 = -1;                 // -1: 193 .. 224 output channels run the four-wave 256 x 256 configuration on 256 x 224 tiles where the rule
                                 // of conv_mfma.hip (conv_takes_224) says so, and a skinny pair of the patch kernel multiplies 32 + 48 columns
                                 // (conv_patch.hip); 0: never - full-width tiles (the single-operator entry points, for side-by-side runs)
  int halo_skip = 1;             // position-major rows + per-tile skipping of filter rows that only see the halo, where it pays (0: never)
  int cfg = -1;                  // tile configuration (kCfg* below); -1 = pick by shape
  int splitk = -1;               // split-K factor; -1 = pick by grid size, 1 = off
  void* scratch = nullptr;       // fp32 slabs for split-K (conv_scratch_bytes); null disables split-K
  int64_t scratch_bytes = 0;
};

constexpr int kWeightBlockRows = 64;     // packed weights: [Npad / 64][K steps][64 rows][128 B] (pack.h, block_rows)

// Tile configurations of the shipped library: exactly the ones conv_pick_cfg() can return (ron_conv_num_tile_cfgs()).
enum {
  kCfgIgemm256 = 0,        // row-gather kernel (conv_mfma.hip), 256 x 256 tile, 8 waves, 128 KB LDS
  kCfgIgemm128 = 1,        // 128 x 128, 4 waves, 2 workgroups / CU
  kCfgIgemm128Early = 2,   // ... with a stage's LDS-DMA pieces issued during its first k-step
  kCfgIgemm128x64 = 3,     // 128 x 64 (Cout <= 64 and the skinny heads)
  kCfgPatch256 = 4,        // halo-patch kernel (conv_patch.hip), 256 positions x 256 channels
  kCfgPatch128 = 5,        // ... x 128 channels, 3 weight stages
  kCfgPatch64 = 6,         // ... x 64 channels, 3 weight stages
  kCfgIgemm256TapsInner = 7,   // 256 x 256 with K ordered chunk-major, taps innermost (layers with <= 2 column tiles)
  kCfgC64Resident = 8,     // 3x3 on a 64-channel map with the weights resident in LDS (conv_c64.hip)
  kCfgIgemm128EarlyTapsInner = 9,   // 128 x 128, early issue, K ordered chunk-major with the taps innermost (launches that do not split K)
  kCfgIgemm256x128 = 10,   // 256 x 128 on four waves with the assembly K loop (bf16 / f16 / f16x3): layers with Cout = 128 (conv2_x)
  kNumCfgs = 11
};
inline bool conv_cfg_taps_inner(int cfg) { return cfg == kCfgIgemm256TapsInner || cfg == kCfgIgemm128EarlyTapsInner; }
inline bool conv_cfg_is_patch(int cfg) { return cfg >= kCfgPatch256 && cfg <= kCfgPatch64; }

// The envelope of the conv entry points: the largest value of each geometry field, which is what its bitfield in the kernel
// arguments holds (ConvArgs, conv_device.h: a static_assert there ties the two).  A value beyond it would wrap silently - dilation 32
// to 0, a 17 x 17 filter to 1 x 1 - so it is refused: by check_conv_desc at the descriptor, by check_conv_fields where a ConvLaunch
// is narrowed into ConvArgs.  The same numbers: ron_conv_desc in include/ron_hip.h, INTEGRATION.md, tests/conv_envelope_cases.py.
constexpr int kConvMaxFilter = 15;       // kh, kw
constexpr int kConvMaxStride = 7;        // stride, and kernel == stride of a transposed conv (`up`)
constexpr int kConvMaxDilation = 31;
constexpr int kConvMaxPad = 63;          // SAME padding (kh - 1) * dilation / 2
constexpr int kConvMaxInOrigin = 31;     // input halo beyond the conv's own padding (in.pad - cpad)
constexpr int kConvMaxOutPad = 15;       // halo of an output view
constexpr int kConvMaxTileOrder = 63;    // ConvArgs::m_fastest
// The descriptor of a single-operator entry point, before any arithmetic on it: sizes, filter, stride and dilation >= 1 and inside
// the envelope, the flags 0 or 1.  RON_OK, or RON_ERR_INVALID with the message set.
int check_conv_desc(const ron_conv_desc* d);
// The geometry of the launch that computes the convolution of a descriptor (ops.cpp), behind the caller's own checks (setup_conv and
// train_plan_forward accept different envelopes): dtype, relu, kh / kw / stride / dil / cpad, up / up_cout, Cout, Npad, Ho / Wo and
// *ho x *wo, the output map.  Plain: SAME at stride 1.  Strided: kernel == stride, no padding.  Transposed: kernel == stride, a 1x1
// launch on the input grid with the pixel-shuffle epilogue.  The 3-channel 3x3 stem: one K step of im2col rows, a 1x1 launch.
void conv_launch_geometry(const ron_conv_desc* d, ConvLaunch* c, int* ho, int* wo);

int launch_conv(const ConvLaunch& c, hipStream_t stream);
// what launch_conv would do with `c`: out = {tile configuration (kCfg*), split-K factor, tile order (ConvArgs::m_fastest), K order (taps_inner)};
// n_tile (may be null): columns of the row-gather kernel's tile - the configuration's own width, or 224 where a convolution of
// 193 .. 224 output channels runs the four-wave 256 x 256 configuration on its 256 x 224 form; 0 for the other kernels
int conv_describe(const ConvLaunch& c, int out[4], int* n_tile = nullptr);
// 3x3 / stride 1 / pad 1 on a 64-channel map, weights resident in LDS (conv_c64.hip); pack_conv_c64_weights builds wgt_c64
bool conv_c64_applicable(const ConvLaunch& c);
// a layer whose packed weights get those images beside the rows (graph.cpp, ops.cpp, conv_forward_train.hip): the launch decides later
inline bool conv_c64_wants_images(int dtype, int kh, int kw, int cin, int cout, int npad) {
  return (dtype == RON_DTYPE_BF16 || dtype == RON_DTYPE_F16) && kh == 3 && kw == 3 && cin == 64 && npad == cout && cout % 64 == 0;
}
int launch_conv_c64(const ConvLaunch& c, hipStream_t stream);
std::vector<uint8_t> pack_conv_c64_weights(const std::vector<float>& rows, int npad, int dtype);
// 3x3 / stride 1 / pad 1 with the input halo patch staged once per channel chunk (conv_patch.hip)
bool conv_patch_applicable(const ConvLaunch& c);
int conv_patch_pick(const ConvLaunch& c);          // kCfgPatch* when the patch kernel is the better choice for this launch, else -1
int launch_conv_patch(const ConvLaunch& c, int cfg, hipStream_t stream);
// two convolutions over channel slices of the same map as ONE launch of the patch kernel (the skinny heads of a scale)
bool conv_patch_pair_applicable(const ConvLaunch& a, const ConvLaunch& b);
// force_cfg >= 0 (tooling): that patch configuration whatever the grid size (the pair must still share its input tensor)
int launch_conv_patch_pair(const ConvLaunch& a, const ConvLaunch& b, hipStream_t stream, int force_cfg = -1);
// columns each member of such a pair multiplies on the 64-column tile: 32 / 48 / 64 (conv_patch.hip, patch_pair_widths)
int conv_patch_pair_columns(const ConvLaunch& a, const ConvLaunch& b, int out[2]);
// Elements along K one staging step covers for this dtype (Cin must be a multiple of it).
int conv_k_chunk(int dtype);
int conv_n_tile(int cout);       // granularity Cout is padded to (64 or 128)
int conv_num_cfgs();
int conv_pick_cfg(const ConvLaunch& c);
int conv_pick_splitk(int tiles, int KT, int slots, int tile_elems);      // tile_elems = BM x BN of the configuration (slab bytes of the cost model)
int64_t conv_scratch_bytes(const ConvLaunch& c);   // fp32 split-K slabs this launch can ask for (0: none)
// Several mutually independent convolutions as ONE launch of the row-gather kernel (tile kCfgIgemm128x64, kCfgIgemm128 or kGroupMixed)
// sk_plan: the members' split-K factors from conv_group_plan (depends on the members' geometry and the batch only: callers cache it;
// the mixed-width form models the launch's schedule, ~1 ms of host time), or null to compute them here
// n_tiles (may be null): the width of the column tile member k runs on (the configuration's own, or 224), in the order of `ls`
int launch_conv_group(const ConvLaunch* ls, int n, int cfg, void* scratch, int64_t scratch_bytes, hipStream_t stream, const int* sk_plan = nullptr,
                      int* n_tiles = nullptr);
void conv_group_plan(const ConvLaunch* ls, int n, int cfg, int* sk);
int64_t conv_group_scratch_bytes(const ConvLaunch* ls, int n, int cfg, const int* sk_plan = nullptr);   // sk_plan: from conv_group_plan, or null
constexpr int kMaxConvGroup = 8;
// launch_conv_group only: every member on the 128-row tile of its own width (128 x 128 when Npad % 128 == 0, else 128 x 64)
constexpr int kGroupMixed = 64;
size_t dtype_size(int dtype);
inline bool dtype_is_half(int dtype) { return dtype == RON_DTYPE_BF16 || dtype == RON_DTYPE_F16; }   // 2-byte elements

// Weight gradient of a stride-1 SAME convolution (conv_wgrad.hip): dw[ky,kx,ci,co] = sum over pixels of x[pixel + tap] * dz[pixel], fp32,
// not rounded.  x and dz are whole halo tensors of `dtype` (bf16 / f16) in ONE geometry (same N, H, W, pad = (kh - 1) * dil / 2,
// channels padded to 64: x.C = cin, dz.C >= Cout with zero pad channels).  The kernel walks the flat halo-pixel index without a bounds
// test, so the caller guarantees: dz's halo is zero; both tensors are zero from pixels() up to the next multiple of 32; x has `guard`
// >= pad * Wp + pad pixels of finite data (zeros) in front of base and behind its last padded pixel.  ron_conv2d_backward_nhwc packs
// its fp32 operands that way (conv_backward.hip); a network-level backward calls this on its own halo tensors without the fp32 boundary conversions.
struct WgradLaunch {
  int dtype = RON_DTYPE_BF16;
  TensorView x, dz;              // base = halo pixel 0
  int kh = 1, kw = 1, dil = 1;
  int Cout = 0;                  // columns of dw that are stored (<= dz.C)
  int64_t guard = 0;             // readable pixels of x on either side (see above)
  float* dw = nullptr;           // [kh,kw,cin,Cout] HWIO fp32: every element written
  int splitk = -1;               // pixel slices: -1 = by shape, 1 = off, S = forced (never more than there are 32-pixel steps, or than keeps the slabs below 2 GiB)
  void* scratch = nullptr;       // fp32 slabs of the slices (conv_wgrad_scratch_bytes), summed in slice order: bitwise reproducible
  int64_t scratch_bytes = 0;
};
int launch_conv_wgrad(const WgradLaunch& c, hipStream_t stream);
int conv_wgrad_slices(const WgradLaunch& c);                 // the pixel slices launch_conv_wgrad would use (-1: `c` is refused)
int64_t conv_wgrad_scratch_bytes(const WgradLaunch& c);      // 0 when it does not split, -1 when `c` is refused

// conv1_1 (stem.hip): 3 -> 64 channels straight from the fp32 image (bf16 / f16; f16x3: the split-precision form)
void stem_pack_weights(const float* hwio, int dtype, std::vector<uint16_t>* frags);
float stem_pack_weights_split(const float* hwio, std::vector<uint16_t>* frags);     // RON_DTYPE_F16X3: returns the epilogue's 2^-k
int launch_stem_conv(const float* x, int n, int h, int w, int dtype, const void* d_wfrag, const float* d_bias,
                     const TensorView& out, hipStream_t s, float oscale = 1.f);

// conv1_1 + conv1_2 + pool1 fused (stem.hip): image -> pool1, bf16 / f16 only
void stem2_pack_weights(const float* hwio, int dtype, std::vector<uint16_t>* lds_image);
void stem2_pack_w1(const float* hwio, int dtype, std::vector<uint16_t>* frags);
int launch_stem2(const float* x, int n, int h, int w, int dtype, const void* d_w1frag, const float* d_bias1,
                 const void* d_w2img, const float* d_bias2, const TensorView& out, hipStream_t s);

// helpers (elementwise.hip)
int launch_im2col_c3(const float* x, int n, int h, int w, int dtype, void* out, int kchunk, hipStream_t s);
int launch_maxpool2x2(const TensorView& in, const TensorView& out, int dtype, hipStream_t s);
int launch_maxpool3x3s1(const TensorView& in, const TensorView& out, int dtype, hipStream_t s);
int launch_l2norm(const TensorView& in, const TensorView& out, const float* d_gamma, int dtype, hipStream_t s);
int launch_pack_input(const float* x, const TensorView& out, int dtype, hipStream_t s);      // dense fp32 -> view
int launch_fill_random(const TensorView& out, int dtype, unsigned seed, hipStream_t s);       // interior <- U[-1,1)
int launch_unpack(const TensorView& in, int dtype, int in_is_f32, float* y, hipStream_t s);  // view -> dense fp32

}  // namespace ron
