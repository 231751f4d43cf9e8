// conv1_1: 3x3 SAME conv, 3 -> 64 channels, + bias + ReLU, straight from the caller's fp32 NHWC image into the
// halo bf16/f16 activation tensor (nets/ron_vgg_320.py:454 / :530, first slim.conv2d of conv1).
//
// K = 27 is too thin for the LDS-DMA implicit-GEMM kernel (its rows are 128-byte chunks), so this layer is its own
// kernel: HBM-bound on the 128 B/pixel output (13 MB/image), the 4 MFMAs per 32 pixels are noise.
//   * one wave = 32 consecutive pixels of one image row (fewer in the last tile of a row whose width is not a multiple of 32: the
//     staging is zero beyond the image and the stores of the pixels that do not exist are masked); it stages the 3 x 34 x 3 fp32 input patch in its private LDS
//     slice (zero outside the image), then every lane gathers its 16 A values (pixel r = lane & 31, k = 8h+j and
//     16+8h+j, k = ty*9 + tx*3 + c, zero for k >= 27) with stride-3 LDS reads (conflict free) and packs them to bf16;
//   * B (weights, [64][32] after padding K) lives in 4 registers per lane for the whole kernel;
//   * MFMA column r of accumulator t is output channel 2r + t, so a lane's two accumulators are adjacent channels:
//     one dword store per pixel row, 32 lanes = the pixel's full 128-byte channel vector.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <stdlib.h>

#include <vector>

#include "pack.h"

namespace ron {
namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 h16x8;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;

// cvt2: two fp32 -> one dword of two storage-type values (round to nearest even; bf16: ONE v_cvt_pk_bf16_f32), low half first
struct StemBF16 {
  static __device__ __forceinline__ unsigned short cvt(float v) { return __builtin_bit_cast(unsigned short, __float2bfloat16(v)); }
  static __device__ __forceinline__ unsigned cvt2(float a, float b) { return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2)); }
  static __device__ __forceinline__ float tof(unsigned v) { return __uint_as_float(v << 16); }
  static __device__ __forceinline__ void mma(const u32x4& a, const u32x4& b, f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(s16x8, a), __builtin_bit_cast(s16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ void mma16(const u32x4& a, const u32x4& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, a), __builtin_bit_cast(s16x8, b), c, 0, 0, 0);
  }
};
struct StemF16 {
  static __device__ __forceinline__ unsigned short cvt(float v) { return __builtin_bit_cast(unsigned short, (_Float16)v); }
  static __device__ __forceinline__ unsigned cvt2(float a, float b) { return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, f16x2)); }
  static __device__ __forceinline__ float tof(unsigned v) { return (float)__builtin_bit_cast(_Float16, (unsigned short)v); }
  static __device__ __forceinline__ void mma(const u32x4& a, const u32x4& b, f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ void mma16(const u32x4& a, const u32x4& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
  }
};

constexpr int kPatchW = 34 * 3;          // floats per staged row: pixels x0-1 .. x0+32, 3 channels
constexpr int kPatch = 3 * kPatchW;      // 306 floats per wave

template <class Tr>
__global__ __launch_bounds__(256) void stem_conv_kernel(const float* __restrict__ x, int n_img, int H, int W,
                                                        const u32x4* __restrict__ wfrag, const float* __restrict__ bias2,
                                                        unsigned* __restrict__ out, int out_Hp, int out_Wp, int out_pad) {
  __shared__ float s_in[4][kPatch + 14];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  // weights: [t][s][lane] 16-byte fragments; bias pairs (channel 2r, 2r+1)
  u32x4 wb[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s) wb[t][s] = wfrag[(t * 2 + s) * 64 + lane];
  const float b0 = bias2[2 * r], b1 = bias2[2 * r + 1];
  // LDS read offsets of this lane's 16 A values (floats, relative to the wave's patch)
  int a_off[2][8];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 16 * s + 8 * h + j;
      const int ty = k / 9, rem = k - ty * 9;
      a_off[s][j] = k < 27 ? ty * kPatchW + r * 3 + rem : -1;
    }
  float* patch = s_in[wave];
  const int tiles_per_row = (W + 31) / 32;      // the last tile of a row is ragged when W % 32 != 0 (SSD-300: 12 columns): masked stores
  const long long n_tiles = (long long)n_img * H * tiles_per_row;
  for (long long tile = (long long)blockIdx.x * 4 + wave; tile < n_tiles; tile += (long long)gridDim.x * 4) {
    const int tx = (int)(tile % tiles_per_row);
    const long long row = tile / tiles_per_row;
    const int y = (int)(row % H);
    const long long img = row / H;
    const int x0 = tx * 32;
    // stage rows y-1..y+1, pixels x0-1..x0+32 (zero outside the image)
    for (int i = lane; i < kPatch; i += 64) {
      const int ty = i / kPatchW, rem = i - ty * kPatchW;
      const int px = rem / 3, c = rem - px * 3;
      const int yy = y + ty - 1, xx = x0 + px - 1;
      float v = 0.f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = x[((img * H + yy) * (long long)W + xx) * 3 + c];
      patch[i] = v;
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);       // lgkmcnt(0): this wave's LDS writes are done (wave-private slice)
    __builtin_amdgcn_wave_barrier();
    u32x4 fa[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      unsigned short e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = Tr::cvt(a_off[s][j] >= 0 ? patch[a_off[s][j]] : 0.f);
      fa[s] = u32x4{(unsigned)e[0] | ((unsigned)e[1] << 16), (unsigned)e[2] | ((unsigned)e[3] << 16),
                    (unsigned)e[4] | ((unsigned)e[5] << 16), (unsigned)e[6] | ((unsigned)e[7] << 16)};
    }
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
      Tr::mma(fa[0], wb[t][0], acc[t]);
      Tr::mma(fa[1], wb[t][1], acc[t]);
    }
    // pixel row p = (e & 3) + 8 * (e >> 2) + 4 * h ; lanes r = 0..31 cover channels 0..63 as dwords
    const long long obase = ((img * out_Hp + y + out_pad) * (long long)out_Wp + x0 + out_pad) * 32;   // in dwords (64 ch * 2 B)
    const int n_px = min(32, W - x0);          // pixels of this tile that exist (the staged patch is zero beyond the image)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int p = (e & 3) + 8 * (e >> 2) + 4 * h;
      const unsigned lo = Tr::cvt(fmaxf(acc[0][e] + b0, 0.f)), hi = Tr::cvt(fmaxf(acc[1][e] + b1, 0.f));
      if (p < n_px) out[obase + (long long)p * 32 + r] = lo | (hi << 16);
    }
    __builtin_amdgcn_wave_barrier();          // patch is rewritten by the next iteration
  }
}


// conv1_1 in split precision (RON_DTYPE_F16X3, conv_device.h): the same tiling; A and B are two f16 planes each (hi = rnd(v),
// lo = rnd(v - hi); the weights times 2^k so that their lo plane is a normal f16, undone by `oscale`), a product is three MFMAs
// hi*hi + lo*hi + hi*lo into the fp32 accumulator, and a pixel's 64 outputs are stored as two 128-byte chunks [32 x hi][32 x lo].
// Replaces im2col (173 us at batch 32) + a K = 32 GEMM through the row-gather kernel (276 us): HBM-bound on its 838 MB of output.
__global__ __launch_bounds__(256) void stem_conv_split_kernel(const float* __restrict__ x, int n_img, int H, int W,
                                                              const u32x4* __restrict__ wfrag, const float* __restrict__ bias2, float oscale,
                                                              unsigned* __restrict__ out, int out_Hp, int out_Wp, int out_pad) {
  __shared__ float s_in[4][kPatch + 14];
  __builtin_amdgcn_s_setreg((0 << 11) | (23 << 6) | 1, 1);      // MODE.FP16_OVFL: overflowing f16 conversions saturate (conv_device.h)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  u32x4 wb[2][2][2];                    // [plane: hi, lo][t][s]
#pragma unroll
  for (int pl = 0; pl < 2; ++pl)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) wb[pl][t][s] = wfrag[((pl * 2 + t) * 2 + s) * 64 + lane];
  const float b0 = bias2[2 * r], b1 = bias2[2 * r + 1];
  int a_off[2][8];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 16 * s + 8 * h + j;
      const int ty = k / 9, rem = k - ty * 9;
      a_off[s][j] = k < 27 ? ty * kPatchW + r * 3 + rem : -1;
    }
  float* patch = s_in[wave];
  const int tiles_per_row = (W + 31) / 32;      // the last tile of a row is ragged when W % 32 != 0 (SSD-300: 12 columns): masked stores
  const long long n_tiles = (long long)n_img * H * tiles_per_row;
  for (long long tile = (long long)blockIdx.x * 4 + wave; tile < n_tiles; tile += (long long)gridDim.x * 4) {
    const int tx = (int)(tile % tiles_per_row);
    const long long row = tile / tiles_per_row;
    const int y = (int)(row % H);
    const long long img = row / H;
    const int x0 = tx * 32;
    for (int i = lane; i < kPatch; i += 64) {
      const int ty = i / kPatchW, rem = i - ty * kPatchW;
      const int px = rem / 3, c = rem - px * 3;
      const int yy = y + ty - 1, xx = x0 + px - 1;
      float v = 0.f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = x[((img * H + yy) * (long long)W + xx) * 3 + c];
      patch[i] = v;
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    u32x4 fa[2][2];                     // [plane][s]
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      unsigned short eh[8], el[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = a_off[s][j] >= 0 ? patch[a_off[s][j]] : 0.f;
        const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
        eh[j] = __builtin_bit_cast(unsigned short, hi);
        el[j] = __builtin_bit_cast(unsigned short, lo);
      }
      fa[0][s] = u32x4{(unsigned)eh[0] | ((unsigned)eh[1] << 16), (unsigned)eh[2] | ((unsigned)eh[3] << 16),
                       (unsigned)eh[4] | ((unsigned)eh[5] << 16), (unsigned)eh[6] | ((unsigned)eh[7] << 16)};
      fa[1][s] = u32x4{(unsigned)el[0] | ((unsigned)el[1] << 16), (unsigned)el[2] | ((unsigned)el[3] << 16),
                       (unsigned)el[4] | ((unsigned)el[5] << 16), (unsigned)el[6] | ((unsigned)el[7] << 16)};
    }
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        StemF16::mma(fa[0][s], wb[0][t][s], acc[t]);      // hi * hi
        StemF16::mma(fa[1][s], wb[0][t][s], acc[t]);      // lo * hi
        StemF16::mma(fa[0][s], wb[1][t][s], acc[t]);      // hi * lo
      }
    }
    // a pixel = 64 dwords: channel pair r (channels 2r, 2r + 1) -> chunk r / 16: hi dword at chunk * 32 + r % 16, lo dword 16 further
    const long long obase = ((img * out_Hp + y + out_pad) * (long long)out_Wp + x0 + out_pad) * 64;
    const int n_px = min(32, W - x0);
    const int od = (r >> 4) * 32 + (r & 15);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int p = (e & 3) + 8 * (e >> 2) + 4 * h;
      const float v0 = fmaxf(fmaf(acc[0][e], oscale, b0), 0.f), v1 = fmaxf(fmaf(acc[1][e], oscale, b1), 0.f);
      const _Float16 h0 = (_Float16)v0, h1 = (_Float16)v1;
      const _Float16 l0 = (_Float16)(v0 - (float)h0), l1 = (_Float16)(v1 - (float)h1);
      if (p >= n_px) continue;
      out[obase + (long long)p * 64 + od] = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
      out[obase + (long long)p * 64 + od + 16] = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
    }
    __builtin_amdgcn_wave_barrier();
  }
}


// ---------------------------------------------------------------------------------------------------------------
// conv1_1 + conv1_2 + pool1 in one kernel (RON_CFG_FUSE_POOLS, bf16 / f16).
//
// As separate launches the stem writes the 64-channel conv1_1 map (13 MB per image) and conv1_2 stages it back nine
// times: 9 % of the step at batch 32.  Here a workgroup of FOUR waves owns an 8 x 32 pixel tile of conv1_2's output, and TWO
// such workgroups share a CU, each on a tile of its own and out of phase with the other:
//   A. the 12 x 36 x 3 fp32 image patch goes to LDS (zero outside the image); the patch of the workgroup's next tile is fetched
//      into registers while this one computes;
//   B. conv1_1 (+bias, ReLU) of the 10 x 34 halo patch is computed with MFMAs (K = 27 -> 32, one 16x16x32 instruction per 16
//      pixels x 16 channels) and stored as rows of 64 channels in LDS, zero outside the image (= conv1_2's padding).  A row is 128
//      bytes of data in a stride of 144: sixteen lanes that read the same 16-byte chunk of sixteen consecutive rows hit sixteen
//      different bank quads, for any tap shift, and every address of phase C is ONE per-lane base + an immediate;
//   C. conv1_2 runs its 9 taps straight from that patch on 16x16x32 MFMAs.  Wave w owns output-channel blocks 2 (w & 1),
//      2 (w & 1) + 1 (of four blocks of 16) and tile rows 4 (w >> 1) .. + 3, as two passes of two rows.  Its share of the weights -
//      9 taps x 2 k-steps x 2 blocks = 36 fragments of 16 bytes per lane, 144 registers - is loaded ONCE, before the tile loop,
//      and stays in registers for the life of the (persistent) workgroup.  A pass walks its four patch rows once: a fragment of
//      patch row pr feeds output row 0 as filter row pr and output row 1 as filter row pr - 1, so phase C is 48 ds_read_b128
//      (fetched two steps ahead) + 144 MFMAs per pass and nothing else, and an output still sees its taps in the old order;
//   D. + bias, ReLU, 2x2 max-pool: horizontal pairs are adjacent accumulator registers, vertical pairs are the two rows of a pass
//      (same lane, same register index), so the pooled value is formed in registers with the operations, in the order, of the
//      form that met the vertical pair in LDS (round, then max, then round again: the same bits).  The 4 x 16 pooled tile is
//      collected in LDS (a wave holds two of a pixel's four channel quads' halves) and leaves in 16-byte stores.
// Two barriers per tile.  HBM traffic: image in (1.2 MB / image), pool1 out (3.3 MB / image).
//
// Why two workgroups per CU.  Phase C is matrix-pipe work (4 608 cycles per SIMD and tile), phases B and D are vector-ALU work of
// the same order (gather, convert, bias / ReLU / inside mask / pack of 340 pixels x 64 channels), and the barriers between them keep
// the waves of ONE workgroup in the same phase: with one workgroup on a CU the two pipes take turns.  A second, independent
// workgroup on the same SIMDs is in its vector phases while the first issues MFMAs.  What stood in the way was LDS: the form
// before this one kept all 72 KB of conv1_2 weights there (+ patch, image, pool staging: 137 KB, eight waves, one workgroup per CU,
// 275 us at batch 32); with the weights in registers a workgroup needs 72 KB.  Measured (profiles/r07): 275 -> 226 us at batch 32, the
// matrix pipe busy 41 % -> 50 % of the launch.  Starting the second workgroup of a CU half a tile late (s_sleep, by block index or by
// the hardware's wave slot) changed nothing: the two do not run in lockstep, and what is left is not a matter of their phase.
// Earlier forms that lost, and why:
//   * round 2, producer / consumer waves in one workgroup (waves 4-7: image fetch + conv1_1 of tile t+1 into a second patch buffer,
//     waves 0-3: conv1_2 of tile t): 335 us against 310.  Four producer waves, one per SIMD, had nothing to hide their own
//     latencies behind and took longer over a tile's 22 groups than the consumers' 4 600 MFMA cycles.
//   * round 6, two tile rows per wave inside the eight-wave form (tools/experiments/stem_two_rows_per_wave.patch): fewer weight
//     reads in phase C, the same lockstep, no gain; its variant with 336 bytes of scratch ran 451 us.  No build of this kernel may
//     use scratch (tests/test_stem2_resources.py reads the compiler's own figures).
constexpr int kS2TH = 8, kS2TW = 32;
constexpr int kS2PW = kS2TW + 2, kS2PH = kS2TH + 2, kS2Rows = kS2PW * kS2PH;       // 34 x 10 = 340 patch rows
constexpr int kS2IW = kS2TW + 4, kS2IH = kS2TH + 4;                                 // 36 x 12 image patch
constexpr int kS2Threads = 256, kS2Waves = kS2Threads / 64;
constexpr int kS2PerCU = 2, kS2MaxGrid = 256 * kS2PerCU;                            // workgroups per CU; the persistent grid
constexpr int kS2Groups = (kS2Rows + 15) / 16;                                      // 22 groups of 16 patch pixels (the last one: 4 + 12 spare rows)
constexpr int kS2GroupsPerWave = (kS2Groups + kS2Waves - 1) / kS2Waves;             // 6 = two trios
constexpr int kS2RowBytes = 128 + 16;
constexpr int kS2PatchBytes = kS2Groups * 16 * kS2RowBytes;                         // 352 rows: 49.5 KB
constexpr int kS2ImgFloats = kS2IH * kS2IW * 3;
constexpr int kS2PoolBytes = (kS2TH / 2) * (kS2TW / 2) * 128;                       // the pooled tile: 8 KB
constexpr int kS2TabBytes = kS2Groups * 16 * 4;                                     // one dword per patch row, four tables
constexpr int kS2W1Bytes = 4 * 64 * 16 + 64 * 4 + 4 * 8 * 4;                         // conv1_1: weight fragments, bias, gather offsets
constexpr int kS2Lds = kS2PatchBytes + kS2ImgFloats * 4 + kS2PoolBytes + 4 * kS2TabBytes + kS2W1Bytes;
static_assert(kS2GroupsPerWave == 6, "phase B runs a trio of groups twice");
static_assert(kS2Lds <= 80 * 1024, "two workgroups per CU: at most half of the CU's 160 KB of LDS each");
static_assert(kS2PatchBytes % 16 == 0 && (kS2ImgFloats * 4) % 16 == 0 && kS2PoolBytes % 16 == 0 && kS2TabBytes % 16 == 0, "16-byte LDS accesses");

template <class Tr>
__global__ __launch_bounds__(kS2Threads, kS2PerCU) void stem2_kernel(const float* __restrict__ x, int n_img, int H, int W,
                                                                     const u32x4* __restrict__ w1frag, const float* __restrict__ bias1,
                                                                     const u32x4* __restrict__ w2img, const float* __restrict__ bias2,
                                                                     unsigned short* __restrict__ out, int out_Hp, int out_Wp, int out_pad) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* s_p = smem;
  float* s_img = reinterpret_cast<float*>(s_p + kS2PatchBytes);
  char* s_pool = reinterpret_cast<char*>(s_img + kS2ImgFloats);
  unsigned* s_st = reinterpret_cast<unsigned*>(s_pool + kS2PoolBytes);
  int* s_gb = reinterpret_cast<int*>(s_st + kS2Groups * 16);
  u32x4* s_w1 = reinterpret_cast<u32x4*>(s_gb + kS2Groups * 16);
  float* s_b1 = reinterpret_cast<float*>(s_w1 + 4 * 64);
  int* s_aoff = reinterpret_cast<int*>(s_b1 + 64);
  unsigned* s_in = reinterpret_cast<unsigned*>(s_aoff + 32);
  unsigned* s_yx = s_in + kS2Groups * 16;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // in a scalar register: what depends on it alone branches uniformly
  const int c16 = lane & 15, kg = lane >> 4;                      // the 16x16x32 fragment and accumulator layout
  const int jw = 2 * (wave & 1), rw = 4 * (wave >> 1);            // this wave's first channel block and first tile row

  // conv1_2 weights.  The host packed the LDS image of the earlier form (tap, permuted output row j * 16 + c = channel 4 c + j,
  // 16-byte chunks swizzled by the row); the B fragment of (tap, k-step ks, block j) for lane (c16, kg) is one 16-byte element of it.
  u32x4 w2[9][2][2];
  {
    const int key_b = ((c16 >> 1) & 3) << 1;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) w2[tap][ks][jj] = w2img[tap * 512 + ((jw + jj) * 16 + c16) * 8 + ((4 * ks + kg) ^ key_b)];
  }
  float b2[2];                                   // conv1_2 bias of this lane's two adjacent output channels 4 c16 + jw, + 1
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) b2[jj] = bias2[4 * c16 + jw + jj];
  // conv1_1's constants wait in LDS and are read once per trio of groups (beside the 144 weight registers there is no room to hold
  // them): the weight fragments - n-tile t, lane (c = l & 15, kg = l >> 4) holds W[k = 8 kg + j][channel 4c + t], so a lane's four
  // accumulators are adjacent channels (one 8-byte LDS store per pixel) -, the bias, and per kg the image-patch offsets of the
  // lane's eight K elements k = 8 kg + j = (ty * 3 + tx) * 3 + c (k >= 27 is K padding: any address, the value is dropped).
  static_assert(kS2Threads == 4 * 64, "one conv1_1 weight fragment per thread");
  s_w1[tid] = w1frag[tid];
  if (tid < 64) s_b1[tid] = bias1[tid];
  if (tid < 32) {
    const int k = tid, ty = k / 9, rem = k - ty * 9;
    s_aoff[tid] = k < 27 ? ty * (kS2IW * 3) + rem : 0;
  }
  const bool k_pad = kg == 3;                                       // this lane's elements j >= 3 are K padding (k = 27 .. 31)
  // phase B bookkeeping is the same for every tile and lives in LDS, one dword per patch row q (a wave has six groups of 16 rows:
  // too many to keep per group in registers beside the weights): s_st[q] = byte offset of the row in the patch; s_gb[q] = where the
  // pixel's 3 x 3 x 3 window starts in the image patch (floats).  A third table changes with the tile and is written with the tile's
  // image patch: s_in[q] = all ones if pixel q of the patch lies inside the image, else zero (conv1_2 pads with zeros, not with
  // conv1_1 of zeros) - two entries per thread and tile instead of a coordinate test per accumulator register.
  // Rows 340 .. 351 exist in LDS, are computed like the others (a window clamped into the image patch) and are never read.
  for (int q = tid; q < kS2Groups * 16; q += kS2Threads) {
    s_st[q] = (unsigned)(q * kS2RowBytes);
    const int qc = min(q, kS2Rows - 1);
    s_gb[q] = ((qc / kS2PW) * kS2IW + qc % kS2PW) * 3;
  }
  static_assert(kS2Groups * 16 <= 2 * kS2Threads, "two adjacent patch rows per thread");
  const bool in_mine = 2 * tid < kS2Groups * 16;                  // this thread keeps s_in[2 tid], s_in[2 tid + 1] (one address for both tables)
  if (in_mine) {                                                  // patch row << 16 | patch column; read back by this thread only
    const int q = 2 * tid;
    *reinterpret_cast<u32x2*>(s_yx + q) = u32x2{(unsigned)(q / kS2PW) << 16 | (unsigned)(q % kS2PW), (unsigned)((q + 1) / kS2PW) << 16 | (unsigned)((q + 1) % kS2PW)};
  }
  const int tiles_x = W / kS2TW, tiles_y = H / kS2TH;
  const int n_tiles = n_img * tiles_y * tiles_x;
  // ---- A: image patch (rows y0-2 .. y0+9, columns x0-2 .. x0+33) of a tile: 12 rows of 108 floats.  Threads 0 .. 215 take one float
  // of every second row (thread = column + 108 * row parity), six each; the others fetch a clamped address and store nothing.  The
  // patch of tile t+1 is fetched into registers while tile t computes and dropped into LDS once phase B of tile t has read its own.
  constexpr int kImgRow = kS2IW * 3, kImgPer = kS2IH / 2;
  static_assert(2 * kImgRow <= kS2Threads, "two image rows per pass");
  const int i_par = tid / kImgRow, i_ix = tid - i_par * kImgRow;       // ix * 3 + c
  const bool i_store = tid < 2 * kImgRow;
  float pre[kImgPer];
#define RON_S2_FETCH(tile_)                                                                                   \
  do {                                                                                                        \
    const int t_ = min((tile_), n_tiles - 1);      /* past the last tile: fetched again, never used */        \
    const int fx = t_ % tiles_x, fy = (t_ / tiles_x) % tiles_y, fimg = t_ / (tiles_x * tiles_y);              \
    const int xc = (fx * kS2TW - 2) * 3 + i_ix, xcc = min(max(xc, 0), W * 3 - 1);                             \
    _Pragma("unroll") for (int k = 0; k < kImgPer; ++k) {                                                     \
      const int yy = fy * kS2TH - 2 + 2 * k + i_par;                                                          \
      const int yc = min(max(yy, 0), H - 1);                                      /* unconditional load */      \
      const float v_ = x[((long long)fimg * H + yc) * W * 3 + xcc];                                           \
      /* a bit mask, not a select: hipcc turns the select back into a branch around the load */               \
      pre[k] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v_) & (unsigned)-(int)(yy == yc && xc == xcc)); \
    }                                                                                                         \
  } while (0)
#define RON_S2_STORE()                                                                                        \
  do {                                                                                                        \
    if (i_store) {                                                                                            \
      _Pragma("unroll") for (int k = 0; k < kImgPer; ++k) s_img[(2 * k + i_par) * kImgRow + i_ix] = pre[k];   \
    }                                                                                                         \
  } while (0)
#define RON_S2_INSIDE(tile_)                                                                                  \
  do {                                                                                                        \
    const int t_ = min((tile_), n_tiles - 1);                                                                 \
    const int my = ((t_ / tiles_x) % tiles_y) * kS2TH - 1, mx = (t_ % tiles_x) * kS2TW - 1;                    \
    if (in_mine) {                                                                                            \
      const u32x2 yx = *reinterpret_cast<const u32x2*>(s_yx + 2 * tid);   /* from LDS, not from registers */    \
      u32x2 in_;                                                                                              \
      _Pragma("unroll") for (int k = 0; k < 2; ++k)                                                           \
        in_[k] = (unsigned)-(int)((unsigned)(my + (int)(yx[k] >> 16)) < (unsigned)H && (unsigned)(mx + (int)(yx[k] & 0xFFFFu)) < (unsigned)W); \
      *reinterpret_cast<u32x2*>(s_in + 2 * tid) = in_;                                                        \
    }                                                                                                         \
  } while (0)
  RON_S2_FETCH(blockIdx.x);
  RON_S2_STORE();
  RON_S2_INSIDE(blockIdx.x);
  __syncthreads();                                    // the image patch, the tables, conv1_1's constants
  const unsigned st_lane = (unsigned)c16 * 8u;        // the lane's four channels within a patch row
  const char* pa0 = s_p + (rw * kS2PW + c16) * kS2RowBytes + kg * 16;     // phase C: row rw, pixel c16, chunk kg
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int tx = tile % tiles_x;
    const int ty_ = (tile / tiles_x) % tiles_y;
    const int img = tile / (tiles_x * tiles_y);
    const int y0 = ty_ * kS2TH, x0 = tx * kS2TW;
    RON_S2_FETCH(tile + gridDim.x);                   // in flight during phase B
    // ---- B: conv1_1 of the 340 patch pixels, 16 at a time: groups wave, wave + 4, ... as two trios of straight-line code the
    // compiler interleaves (six unrolled would not fit beside the weights)
#pragma unroll 1
    for (int trio = 0; trio < 2; ++trio) {
      u32x4 wb[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) wb[t] = s_w1[t * 64 + lane];
      const f32x4 b1 = *reinterpret_cast<const f32x4*>(s_b1 + 4 * c16);
      int a_off[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a_off[j] = s_aoff[8 * kg + j];
#pragma unroll
      for (int gi = 0; gi < 3; ++gi) {
        const int g = wave + kS2Waves * (3 * trio + gi);
        if (gi == 2 && g >= kS2Groups) continue;      // groups 22, 23 do not exist (waves 2, 3, second trio): uniform branch
        const float* base = s_img + s_gb[g * 16 + c16];
        const u32x4 m4 = *reinterpret_cast<const u32x4*>(s_st + g * 16 + 4 * kg);
        const u32x4 in4 = *reinterpret_cast<const u32x4*>(s_in + g * 16 + 4 * kg);
        float gv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float gj = base[a_off[j]];
          gv[j] = j >= 3 && k_pad ? 0.f : gj;
        }
        const u32x4 fa = u32x4{Tr::cvt2(gv[0], gv[1]), Tr::cvt2(gv[2], gv[3]), Tr::cvt2(gv[4], gv[5]), Tr::cvt2(gv[6], gv[7])};
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
          Tr::mma16(fa, wb[t], acc[t]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {                 // accumulator register e: patch pixel g * 16 + 4 kg + e, channels 4 c16 .. + 3
          const unsigned inside = in4[e];                                   // a mask (no branch)
          float v[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] = fmaxf(acc[t][e] + b1[t], 0.f);
          *reinterpret_cast<u32x2*>(s_p + m4[e] + st_lane) = u32x2{Tr::cvt2(v[0], v[1]) & inside, Tr::cvt2(v[2], v[3]) & inside};
        }
      }
    }
    __syncthreads();
    RON_S2_STORE();                                   // s_img and s_in are free: the next tile's (read after one more barrier)
    RON_S2_INSIDE(tile + gridDim.x);
    // ---- C + D: conv1_2 of tile rows rw + 2 p, rw + 2 p + 1 (9 taps x 2 k-steps, each A fragment against the wave's two channel
    // blocks), then their pooled row.  Accumulator register e of [rr][a][jj] holds pixel 16 a + 4 kg + e of row rw + 2 p + rr,
    // channel 4 c16 + jw + jj.
#pragma unroll 1
    for (int p = 0; p < 2; ++p) {
      const char* pa = pa0 + p * (2 * kS2PW * kS2RowBytes);
      f32x4 acc2[2][2][2];
#pragma unroll
      for (int rr = 0; rr < 2; ++rr)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) acc2[rr][a][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
      // Patch row pr = 0 .. 3 of the pass serves output row rr = 0 as filter row pr and output row rr = 1 as filter row pr - 1: every
      // A fragment is read ONCE and used at once for both (nothing is held from one filter row to the next), and each accumulator
      // still sees its taps in order - filter row, column, k-step 0 then 1.  Fragments are fetched two steps ahead of their MFMAs.
      constexpr int kSteps = 4 * 3 * 2;                // (pr, tx, ks)
      u32x4 fa[3][2];
#define RON_S2_FRAGS(step_)                                                                                                  \
  _Pragma("unroll") for (int a = 0; a < 2; ++a) fa[(step_) % 3][a] = *reinterpret_cast<const u32x4*>(                         \
      pa + (((step_) / 6) * kS2PW + 16 * a + ((step_) / 2) % 3) * kS2RowBytes + ((step_) & 1) * 64)
      RON_S2_FRAGS(0);
      RON_S2_FRAGS(1);
#pragma unroll
      for (int step = 0; step < kSteps; ++step) {
        if (step + 2 < kSteps) RON_S2_FRAGS(step + 2);
        const int pr = step / 6, tx = (step / 2) % 3, ks = step & 1;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          const int ty = pr - rr;
          if (ty < 0 || ty > 2) continue;
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) Tr::mma16(fa[step % 3][a], w2[ty * 3 + tx][ks][jj], acc2[rr][a][jj]);
        }
      }
#undef RON_S2_FRAGS
      // bias, ReLU, pool.  Pooled column 8 a + 2 kg + hp comes from registers 2 hp, 2 hp + 1 of both rows: per row max, + bias,
      // ReLU, round to the storage type; then the larger of the two rounded values, rounded again (it is representable: no change)
      const int yp = (rw >> 1) + p;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int hp = 0; hp < 2; ++hp) {
          unsigned d[2];
#pragma unroll
          for (int rr = 0; rr < 2; ++rr) {
            const float m0 = fmaxf(fmaxf(acc2[rr][a][0][2 * hp], acc2[rr][a][0][2 * hp + 1]) + b2[0], 0.f);
            const float m1 = fmaxf(fmaxf(acc2[rr][a][1][2 * hp], acc2[rr][a][1][2 * hp + 1]) + b2[1], 0.f);
            d[rr] = Tr::cvt2(m0, m1);
          }
          const unsigned o = Tr::cvt2(fmaxf(Tr::tof(d[0] & 0xFFFFu), Tr::tof(d[1] & 0xFFFFu)), fmaxf(Tr::tof(d[0] >> 16), Tr::tof(d[1] >> 16)));
          const int mc = 8 * a + 2 * kg + hp;                             // pooled column 0..15
          *reinterpret_cast<unsigned*>(s_pool + (yp * 16 + mc) * 128 + c16 * 8 + jw * 2) = o;
        }
    }
    __syncthreads();
    // the pooled 4 x 16 x 64 tile leaves in 16-byte pieces: row yp, column m, 8 channels c8
#pragma unroll
    for (int k = 0; k < kS2PoolBytes / 16 / kS2Threads; ++k) {
      const int idx = tid + k * kS2Threads;
      const int yp = idx >> 7, m = (idx >> 3) & 15, c8 = idx & 7;
      const u32x4 o = *reinterpret_cast<const u32x4*>(s_pool + idx * 16);
      const long long opix = ((long long)img * out_Hp + (y0 >> 1) + yp + out_pad) * out_Wp + (x0 >> 1) + m + out_pad;
      *reinterpret_cast<u32x4*>(out + opix * 64 + c8 * 8) = o;
    }
    // the next tile's phase B writes the patch (all reads of this tile's are behind the barrier above); its phase D writes
    // s_pool one barrier from here, behind these reads
  }
#undef RON_S2_FETCH
#undef RON_S2_STORE
#undef RON_S2_INSIDE
}
}  // namespace

// Weight fragments for stem_conv_kernel from the HWIO [3,3,3,64] filter: fragment (t, s), lane (r, h), element j holds
// W[k = 16s + 8h + j][channel 2r + t] (zero for k >= 27), in the ctx dtype (bf16 / f16).
void stem_pack_weights(const float* hwio, int dtype, std::vector<uint16_t>* frags) {
  frags->assign(4 * 64 * 8, 0);
  for (int t = 0; t < 2; ++t)
    for (int s = 0; s < 2; ++s)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int r = lane & 31, h = lane >> 5;
          const int k = 16 * s + 8 * h + j, ch = 2 * r + t;
          const float v = k < 27 ? hwio[(size_t)k * 64 + ch] : 0.f;
          (*frags)[((size_t)(t * 2 + s) * 64 + lane) * 8 + j] = dtype == RON_DTYPE_BF16 ? f32_to_bf16_rne(v) : f32_to_f16_rne(v);
        }
}

// split precision: [plane hi / lo][t][s][lane] fragments of w * 2^k; returns 2^-k for the epilogue
float stem_pack_weights_split(const float* hwio, std::vector<uint16_t>* frags) {
  const int k = split_weight_exponent(std::vector<float>(hwio, hwio + 27 * 64));
  frags->assign(2 * 4 * 64 * 8, 0);
  for (int t = 0; t < 2; ++t)
    for (int s = 0; s < 2; ++s)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int r = lane & 31, h = lane >> 5;
          const int kk = 16 * s + 8 * h + j, ch = 2 * r + t;
          const float v = kk < 27 ? ldexpf(hwio[(size_t)kk * 64 + ch], k) : 0.f;
          const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
          (*frags)[((size_t)((0 * 2 + t) * 2 + s) * 64 + lane) * 8 + j] = f32_to_f16_rne((float)hi);
          (*frags)[((size_t)((1 * 2 + t) * 2 + s) * 64 + lane) * 8 + j] = f32_to_f16_rne((float)lo);
        }
  return ldexpf(1.f, -k);
}

int launch_stem_conv(const float* x, int n, int h, int w, int dtype, const void* d_wfrag, const float* d_bias,
                     const TensorView& out, hipStream_t s, float oscale) {
  RON_REQUIRE(dtype == RON_DTYPE_BF16 || dtype == RON_DTYPE_F16 || dtype == RON_DTYPE_F16X3, "stem kernel: bf16 / f16 / f16x3 only");
  RON_REQUIRE(w > 0 && out.C == 64 && out.cstride == 64 && out.coff == 0 && out.H == h && out.W == w, "stem kernel: bad shape");
  const long long tiles = (long long)n * h * ((w + 31) / 32);
  const int grid = (int)std::min<long long>((tiles + 3) / 4, 256 * 8);
  if (dtype == RON_DTYPE_F16X3)
    RON_LAUNCH(stem_conv_split_kernel, dim3(grid), dim3(256), 0, s, x, n, h, w, (const u32x4*)d_wfrag, d_bias, oscale,
                       (unsigned*)out.base, out.Hp(), out.Wp(), out.pad);
  else if (dtype == RON_DTYPE_BF16)
    RON_LAUNCH(stem_conv_kernel<StemBF16>, dim3(grid), dim3(256), 0, s, x, n, h, w, (const u32x4*)d_wfrag, d_bias,
                       (unsigned*)out.base, out.Hp(), out.Wp(), out.pad);
  else
    RON_LAUNCH(stem_conv_kernel<StemF16>, dim3(grid), dim3(256), 0, s, x, n, h, w, (const u32x4*)d_wfrag, d_bias,
                       (unsigned*)out.base, out.Hp(), out.Wp(), out.pad);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

}  // namespace ron

namespace ron {

// conv1_1 weight fragments for stem2_kernel (16x16x32 MFMA) from the HWIO [3,3,3,64] filter: n-tile t, lane (c, kg), element j
// holds W[k = 8 kg + j][channel 4c + t] (zero for k >= 27).
void stem2_pack_w1(const float* hwio, int dtype, std::vector<uint16_t>* frags) {
  frags->assign(4 * 64 * 8, 0);
  for (int t = 0; t < 4; ++t)
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 8; ++j) {
        const int c = lane & 15, kg = lane >> 4, k = 8 * kg + j, ch = 4 * c + t;
        const float v = k < 27 ? hwio[(size_t)k * 64 + ch] : 0.f;
        (*frags)[((size_t)t * 64 + lane) * 8 + j] = dtype == RON_DTYPE_BF16 ? f32_to_bf16_rne(v) : f32_to_f16_rne(v);
      }
}

// Image of the conv1_2 weights for stem2_kernel from the HWIO [3,3,64,64] filter: tap-major, row (j*16 + c) of a tap
// holds output channel 4c + j, 64 input channels = 8 chunks of 16 B, chunk k in slot k ^ (((row >> 1) & 3) << 1) (the layout the
// kernel once kept in LDS; every wave now picks its 36 B fragments per lane out of it, once, as 16-byte elements).
void stem2_pack_weights(const float* hwio, int dtype, std::vector<uint16_t>* img) {
  img->assign(9 * 64 * 64, 0);
  for (int tap = 0; tap < 9; ++tap)
    for (int row = 0; row < 64; ++row) {
      const int j = row / 16, c = row % 16, ch = 4 * c + j;
      for (int cin = 0; cin < 64; ++cin) {
        const float v = hwio[((size_t)tap * 64 + cin) * 64 + ch];
        const int chunk = cin / 8, slot = chunk ^ (((row >> 1) & 3) << 1);
        (*img)[((size_t)tap * 64 + row) * 64 + slot * 8 + cin % 8] = dtype == RON_DTYPE_BF16 ? f32_to_bf16_rne(v) : f32_to_f16_rne(v);
      }
    }
}

int launch_stem2(const float* x, int n, int h, int w, int dtype, const void* d_w1frag, const float* d_bias1,
                 const void* d_w2img, const float* d_bias2, const TensorView& out, hipStream_t s) {
  RON_REQUIRE(dtype == RON_DTYPE_BF16 || dtype == RON_DTYPE_F16, "stem2 kernel: bf16 / f16 only");
  RON_REQUIRE(w % kS2TW == 0 && h % kS2TH == 0 && out.C == 64 && out.cstride == 64 && out.coff == 0 && out.H == h / 2 && out.W == w / 2,
              "stem2 kernel: bad shape");
  const int tiles = n * (h / kS2TH) * (w / kS2TW);
  const int grid = std::min(tiles, kS2MaxGrid);
  const int which = dtype == RON_DTYPE_BF16 ? 0 : 1;
  const void* kernel = which == 0 ? reinterpret_cast<const void*>(&stem2_kernel<StemBF16>) : reinterpret_cast<const void*>(&stem2_kernel<StemF16>);
  static PerDeviceOnce attr_set[2];                // the attribute is per device (common.h)
  RON_HIP_CHECK(attr_set[which].max_dynamic_lds(kernel, kS2Lds));
  // The kernel is built for two workgroups on a CU (registers: __launch_bounds__, LDS: kS2Lds): with one, the matrix pipe idles
  // through every vector phase and half the persistent grid waits for the other half.  Asked of the runtime once per device; a
  // launch that would run that way is an error, not a slower launch.
  static PerDeviceOnce occupancy_checked[2];
  int per_cu = kS2PerCU;
  const hipError_t occ = occupancy_checked[which].once([&]() {
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kS2Threads, kS2Lds);
    return e != hipSuccess ? e : per_cu == kS2PerCU ? hipSuccess : hipErrorLaunchOutOfResources;
  });
  RON_REQUIRE(per_cu == kS2PerCU, "stem2 kernel: %d workgroup(s) of %d threads and %d bytes of LDS fit a CU, it is built for %d", per_cu,
              kS2Threads, kS2Lds, kS2PerCU);
  RON_HIP_CHECK(occ);
  if (which == 0)
    RON_LAUNCH(stem2_kernel<StemBF16>, dim3(grid), dim3(kS2Threads), kS2Lds, s, x, n, h, w, (const u32x4*)d_w1frag, d_bias1,
                       (const u32x4*)d_w2img, d_bias2, (unsigned short*)out.base, out.Hp(), out.Wp(), out.pad);
  else
    RON_LAUNCH(stem2_kernel<StemF16>, dim3(grid), dim3(kS2Threads), kS2Lds, s, x, n, h, w, (const u32x4*)d_w1frag, d_bias1,
                       (const u32x4*)d_w2img, d_bias2, (unsigned short*)out.base, out.Hp(), out.Wp(), out.pad);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

}  // namespace ron

// Tooling / tests: how many workgroups of the fused stem kernel (conv1_1 + conv1_2 + pool1) the runtime places on one CU of the
// current device, at the launch's own block size and LDS size.  The launch requires 2 (launch_stem2).
extern "C" int ron_stem2_workgroups_per_cu(int dtype, int32_t* per_cu) {
  using namespace ron;
  RON_REQUIRE(per_cu != nullptr && (dtype == RON_DTYPE_BF16 || dtype == RON_DTYPE_F16), "stem2 kernel: bf16 / f16 only");
  *per_cu = kS2PerCU;
  if (plan_only()) return RON_OK;
  const void* kernel = dtype == RON_DTYPE_BF16 ? reinterpret_cast<const void*>(&stem2_kernel<StemBF16>) : reinterpret_cast<const void*>(&stem2_kernel<StemF16>);
  RON_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kS2Lds));
  int n = 0;
  RON_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, kS2Threads, kS2Lds));
  *per_cu = n;
  return RON_OK;
}
