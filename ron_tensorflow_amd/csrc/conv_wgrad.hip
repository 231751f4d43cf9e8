// Backward of the stride-1 SAME convolution (ron_conv2d_backward_nhwc): data, weight and bias gradients.  The padded 3x3 convolutions
// of the SSD extra blocks (ron_conv2d_padded_backward_nhwc) reuse it behind a scattering pack of dz, the 2x2 stride-2 convolution and
// transposed convolution (ron_conv2d_k2s2_backward_nhwc) reuse its kernels on space-to-depth views: the last two sections of this file.
//
//   dz    = round(dy * (y > 0))                              pack_halo_kernel (ReLU mask fused), a halo tensor of the storage type
//   dx    = round(conv_SAME(dz, flipped / swapped weights))  launch_conv on dz (the forward's kernels), weights packed ON THE DEVICE
//   dw[t] = X_t^T . dZ  per tap                              conv_wgrad_tile_kernel: the new GEMM, K = the pixel axis
//   dbias = column sums of dz                                colsum kernels, two passes, fixed order
//
// The weight gradient.  x and dz live in the SAME halo geometry (TensorView: shared halos, pad = (k - 1) * dilation / 2) and dz's
// halo is zero, so K is simply the flat halo-pixel index q: dz row q meets x row q + (ky * dil - pad) * Wp + (kx * dil - pad), the
// addressing of the forward's row gather.  A product whose dz pixel is a halo pixel is 0 * (a finite x value), one whose x pixel left
// the map reads a zero halo pixel: no 2-D index math and no bounds test in the loop.  The price is that EVERY row the loop can touch
// holds finite data: x carries `guard` = pad * Wp + pad zero pixels in front of pixel 0 and behind the last one, and both tensors
// are zero up to the next multiple of 32 pixels (the K step).  ron_conv2d_backward_nhwc writes all of that itself.
//
// One workgroup = four waves = one 128 (cin) x 128 (cout) tile of one tap over one slice of the pixel range; each wave owns 64 x 64
// of it as 4 x 4 v_mfma_f32_16x16x32 accumulators (64 fp32 registers per lane).  An axis of exactly 64 channels gets a 64-wide tile
// (2 blocks per wave along it) instead of multiplying zeros in half of a 128-wide one.  Per K step of 32 pixels both operands are staged
// as [32 pixels][128 channels] images: plain 16-byte global loads -> registers -> ds_write_b128, double buffered, one barrier per step
// (no LDS-DMA, no counted vmcnt: nothing for tools/check_dma_counts.py here).  Both MFMA operands want K (pixels) along the lane's
// registers while the images have channels along the row, so both are read with ds_read_b64_tr_b16: per 16 channels two reads per
// lane group g, pixel rows 8g .. 8g+3 and 8g+4 .. 8g+7.  The images use the XOR swizzle of 256-byte rows that is documented as
// conflict free for these reads on a full 128-channel image (not measured here: no LDS bank-conflict counter was collected):  off(row, ch) = 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))),  ch = the 16-byte chunk of the row.
// The transposed read needs EXEC all ones: the workgroup is 256 lanes, every branch around the reads is workgroup-uniform, and
// channel tiles that overhang the tensor are staged as zeros (pad, do not mask).
//
// Pixel slices: when tiles x taps leave CUs idle the pixel range is split over S workgroups per tile (conv1_2: 64 x 64 channels,
// 3.3 M pixels -> 9 tiles, S > 100).  Slices write fp32 slabs with plain stores, conv_wgrad_reduce_kernel adds them in slice order:
// no float atomics, the same bits on every run.  The taps of one (slice, tile) are adjacent workgroup ids: the nine read the same
// pixel rows, shifted, while those are in L2.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "conv_mfma.h"
#include "conv_train.h"
#include "wgrad_device.h"

namespace ron {
namespace {

constexpr int kWgTile = 128;       // channels per tile side
constexpr int kWgStep = 32;         // pixels per K step
constexpr int kWgImage = kWgStep * kWgTile * 2;     // bytes of one staged operand image
constexpr int kWgLds = 4 * kWgImage;                // two operands, double buffered: 32 KB, inside the default limit

using namespace wgrad;      // wgrad_device.h: the roundings, the MFMA and its transposed operand read (shared with stem_wgrad.hip)

// byte offset of 16-byte chunk `ch` (0..15) of pixel row `row` (0..31) in a staged image
__device__ __forceinline__ int image_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

// ---- pack: dense fp32 [N,H,W,Csrc] -> halo tensor of the storage type, EVERY pixel of the buffer written ---------------------------
// The buffer holds `rows` pixels of Cdst channels; pixel `guard` is halo pixel 0 of the view.  Interior pixels get the rounded
// value (zero where mask <= 0, and in channels >= Csrc), everything else - halos, guards, the tail - zero.
struct PackArgs {
  const float* src;
  const float* mask;        // null: no mask
  unsigned short* out;
  long long rows, guard;
  int N, H, W, pad, Csrc, Cdst;
  // SCATTER only (ron_conv2d_padded_backward_nhwc): src and mask are [N,Hs,Ws,Csrc] and source pixel (sy, sx) lands on pixel
  // (soff + sstep * sy, soff + sstep * sx) of the H x W map; every other pixel of the map is zero
  int Hs, Ws, sstep, soff;
};

template <bool BF16, bool SCATTER = false>
__global__ void conv_bwd_pack_halo_kernel(PackArgs a) {
  // (every buffer of the entry point is below 2 GiB, plan_backward: the 16-byte pieces and the pixels fit 32-bit arithmetic)
  const unsigned vecs = a.Cdst / 8;
  const unsigned total = (unsigned)a.rows * vecs;
  const unsigned Wp = a.W + a.pad, Hp = a.H + a.pad;
  const bool vec_ok = a.Csrc % 4 == 0;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned b = i / vecs;
    const int v = (int)(i - b * vecs);
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (b >= (unsigned)a.guard) {
      const unsigned q = b - (unsigned)a.guard;
      const unsigned r = q / Wp;
      const int col = (int)(q - r * Wp);
      const unsigned img = r / Hp;
      const int row = (int)(r - img * Hp);
      bool inside = col >= a.pad && row >= a.pad && img < (unsigned)a.N;
      int sy = row - a.pad, sx = col - a.pad, sh = a.H, sw = a.W;
      if (SCATTER && inside) {
        sy -= a.soff; sx -= a.soff;
        inside = sy >= 0 && sx >= 0 && sy % a.sstep == 0 && sx % a.sstep == 0;
        sy /= a.sstep; sx /= a.sstep; sh = a.Hs; sw = a.Ws;
        inside = inside && sy < sh && sx < sw;
      }
      if (inside) {
        const long long s0 = (((long long)img * sh + sy) * sw + sx) * a.Csrc + v * 8;
        if (vec_ok && v * 8 + 8 <= a.Csrc) {
          const float4 lo = *reinterpret_cast<const float4*>(a.src + s0), hi = *reinterpret_cast<const float4*>(a.src + s0 + 4);
          f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w; f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
          if (a.mask != nullptr) {
            const float4 ml = *reinterpret_cast<const float4*>(a.mask + s0), mh = *reinterpret_cast<const float4*>(a.mask + s0 + 4);
            const float m[8] = {ml.x, ml.y, ml.z, ml.w, mh.x, mh.y, mh.z, mh.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = m[e] > 0.f ? f[e] : 0.f;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if (v * 8 + e < a.Csrc) {
              const float val = a.src[s0 + e];
              f[e] = (a.mask == nullptr || a.mask[s0 + e] > 0.f) ? val : 0.f;
            }
          }
        }
      }
    }
    uint4 o;
    o.x = round_bits<BF16>(f[0]) | ((unsigned)round_bits<BF16>(f[1]) << 16);
    o.y = round_bits<BF16>(f[2]) | ((unsigned)round_bits<BF16>(f[3]) << 16);
    o.z = round_bits<BF16>(f[4]) | ((unsigned)round_bits<BF16>(f[5]) << 16);
    o.w = round_bits<BF16>(f[6]) | ((unsigned)round_bits<BF16>(f[7]) << 16);
    *reinterpret_cast<uint4*>(a.out + (long long)i * 8) = o;
  }
}

// ---- weights for the data gradient: fp32 HWIO on the device -> the blocked rows of pack.h, taps flipped, cin / cout swapped ----------
// rows[n = ci][k = t * CoP + co] = round(w[kh-1-ky, kw-1-kx, ci, co])  (zero for co >= cout and n >= cin), stored as
// [Npad / 64][K / 64][64 rows][64 elements]: hwio_to_rows + cast_rows + block_rows of the transposed filter.
struct WpackArgs {
  const float* w;
  unsigned short* out;
  int taps, cin, cout, cop, npad;
};

template <bool BF16>
__global__ void conv_bwd_pack_weights_kernel(WpackArgs a) {
  const int K = a.taps * a.cop, steps = K / 64;
  const long long total = (long long)a.npad * (K / 8);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    // i counts 16-byte pieces of the blocked image: [n / 64][kt][n % 64][piece of 8]
    const int piece = (int)(i & 7);
    const int nl = (int)((i >> 3) & 63);
    const long long blk = i >> 9;
    const int kt = (int)(blk % steps), nb = (int)(blk / steps);
    const int n = nb * 64 + nl, k = kt * 64 + piece * 8;
    const int t = k / a.cop, co = k - t * a.cop;
    const int ts = a.taps - 1 - t;                 // flipped tap (ky, kx both reversed = the flat tap index reversed)
    unsigned short h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = 0.f;
      if (n < a.cin && co + e < a.cout) v = a.w[((long long)ts * a.cin + n) * a.cout + co + e];
      h[e] = round_bits<BF16>(v);
    }
    uint4 o;
    o.x = h[0] | ((unsigned)h[1] << 16); o.y = h[2] | ((unsigned)h[3] << 16);
    o.z = h[4] | ((unsigned)h[5] << 16); o.w = h[6] | ((unsigned)h[7] << 16);
    *reinterpret_cast<uint4*>(a.out + i * 8) = o;
  }
}

// ---- bias gradient: column sums of the packed dz, two passes in a fixed order ----------------------------------------------------------
// pass 1: block (chunk, 64-channel group): 32 row lanes x 8 vectors of 8 channels; a row lane adds rows r, r + 32, ... of its chunk,
// then 64 threads add the 32 lane sums in lane order.  pass 2: one wave per channel adds the chunk sums, lanes strided, then a fixed tree.
template <bool BF16>
__global__ __launch_bounds__(256) void conv_bwd_colsum_kernel(const unsigned short* dz, long long rows, int cop, long long chunk_rows, float* partial) {
  __shared__ float sums[32][64];
  const int tid = threadIdx.x, v = tid & 7, rl = tid >> 3;
  const int c0 = blockIdx.y * 64;
  const long long r0 = (long long)blockIdx.x * chunk_rows, r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (long long r = r0 + rl; r < r1; r += 32) {
    const uint4 d = *reinterpret_cast<const uint4*>(dz + r * cop + c0 + v * 8);
    const unsigned u[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[2 * e] += bits_to_f<BF16>((unsigned short)(u[e] & 0xFFFFu));
      acc[2 * e + 1] += bits_to_f<BF16>((unsigned short)(u[e] >> 16));
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) sums[rl][v * 8 + e] = acc[e];
  __syncthreads();
  if (tid < 64) {
    float s = 0.f;
    for (int l = 0; l < 32; ++l) s += sums[l][tid];
    partial[(long long)blockIdx.x * cop + c0 + tid] = s;
  }
}

// one wave per channel: lane l adds chunks l, l + 64, ... in that order, then the 64 lane sums are added in a fixed tree
__global__ __launch_bounds__(64) void conv_bwd_colsum_final_kernel(const float* partial, int chunks, int cop, float* dbias) {
  const int c = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int k = lane; k < chunks; k += 64) s += partial[(long long)k * cop + c];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) dbias[c] = s;
}

// ---- the weight-gradient tile ----------------------------------------------------------------------------------------------------------
struct WgradArgs {
  const char* x;            // halo pixel 0 of x (guard pixels in front)
  const char* dz;           // halo pixel 0 of dz
  float* out;               // dw [taps][cin][cout], or the slabs [slices][taps][cin][cout]
  long long slab_elems;     // taps * cin * cout
  int cin, cop, cout;
  int Wp, pad, dil, kw, taps;
  int tiles_m, tiles_n;
  int steps, steps_per;     // K steps in all / per slice (no empty slice)
};

// WBM, WBN: 16-channel MFMA blocks per wave along cin / cout (4 or 2): the workgroup's tile is 32 WBM x 32 WBN channels.  The 64-wide
// forms are for tensors of 64 channels (conv1_2; heads of <= 64 outputs), where a 128-wide tile would multiply zeros half the time.
// They keep the 256-byte image rows and their swizzle and fill half of each row: whether the transposed reads stay conflict free on
// the half-filled image has not been measured.  The epilogue stores 4 bytes per lane, 16 lanes side by side (64-byte segments at
// stride cout): not measured either; it runs once per workgroup behind the whole K loop.
template <bool BF16, int WBM, int WBN>
__global__ __launch_bounds__(256) void conv_wgrad_tile_kernel(WgradArgs a) {
  constexpr int TM = 32 * WBM, TN = 32 * WBN;
  constexpr int XCH = TM / 8, ZCH = TN / 8;            // 16-byte chunks per image row
  constexpr int XN = XCH * kWgStep / 256, ZN = ZCH * kWgStep / 256;      // chunks a lane stages per step (2 or 1)
  extern __shared__ __attribute__((aligned(16))) char smem[];      // [buffer][x image | dz image]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  unsigned id = blockIdx.x;
  const int tap = id % a.taps; id /= a.taps;
  const int tn = id % a.tiles_n; id /= a.tiles_n;
  const int tm = id % a.tiles_m;
  const int slice = id / a.tiles_m;
  const int m0 = tm * TM, n0 = tn * TN;
  const int ky = tap / a.kw, kx = tap - ky * a.kw;
  const long long tap_off = (long long)(ky * a.dil - a.pad) * a.Wp + (kx * a.dil - a.pad);

  // staging: lane -> 16-byte chunk xch of pixel row xrow (and, 128-wide, of row xrow + 16) of the x image; the same for dz
  const int xrow = tid / XCH, xch = tid % XCH, zrow = tid / ZCH, zch = tid % ZCH;
  const bool xv = m0 + xch * 8 < a.cin, zv = n0 + zch * 8 < a.cop;        // a tile that overhangs the channels stages zeros
  const int s_begin = slice * a.steps_per;
  const int n_steps = (a.steps - s_begin < a.steps_per ? a.steps - s_begin : a.steps_per);
  const long long q0 = (long long)s_begin * kWgStep;
  const long long x_row_bytes = (long long)a.cin * 2, z_row_bytes = (long long)a.cop * 2;
  const char* xp = a.x + (q0 + xrow + tap_off) * x_row_bytes + (long long)(m0 + xch * 8) * 2;
  const char* zp = a.dz + (q0 + zrow) * z_row_bytes + (long long)(n0 + zch * 8) * 2;
  const int xst = image_off(xrow, xch), zst = image_off(zrow, zch);        // (row + 16: the same swizzle, 4096 bytes on)
  const uint4 zero4 = {0u, 0u, 0u, 0u};
  // (plain variables, not arrays: indexed through the lambdas' references they ended up in scratch memory, the loads waited for at once)
  uint4 rx0 = zero4, rx1 = zero4, rz0 = zero4, rz1 = zero4;
  auto fetch = [&]() {
    rx0 = xv ? *reinterpret_cast<const uint4*>(xp) : zero4;
    if constexpr (XN == 2) rx1 = xv ? *reinterpret_cast<const uint4*>(xp + 16 * x_row_bytes) : zero4;
    rz0 = zv ? *reinterpret_cast<const uint4*>(zp) : zero4;
    if constexpr (ZN == 2) rz1 = zv ? *reinterpret_cast<const uint4*>(zp + 16 * z_row_bytes) : zero4;
    xp += kWgStep * x_row_bytes;
    zp += kWgStep * z_row_bytes;
  };
  auto stage = [&](int buf) {
    char* xi = smem + buf * 2 * kWgImage;
    char* zi = xi + kWgImage;
    *reinterpret_cast<uint4*>(xi + xst) = rx0;
    if constexpr (XN == 2) *reinterpret_cast<uint4*>(xi + xst + 4096) = rx1;
    *reinterpret_cast<uint4*>(zi + zst) = rz0;
    if constexpr (ZN == 2) *reinterpret_cast<uint4*>(zi + zst + 4096) = rz1;
  };

  // transposed reads: lane 16g + 4q + p supplies row 8g + 4h + q, channels 16 * blk + 4p .. + 3 (h = 0, 1)
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  int aoff[WBM][2], boff[WBN][2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int row = 8 * g + 4 * h + q;
#pragma unroll
    for (int i = 0; i < WBM; ++i) aoff[i][h] = image_off(row, 2 * (wm * WBM + i) + (p >> 1)) + 8 * (p & 1);
#pragma unroll
    for (int j = 0; j < WBN; ++j) boff[j][h] = image_off(row, 2 * (wn * WBN + j) + (p >> 1)) + 8 * (p & 1);
  }

  v4f32 acc[WBM][WBN];
#pragma unroll
  for (int i = 0; i < WBM; ++i)
#pragma unroll
    for (int j = 0; j < WBN; ++j) acc[i][j] = v4f32{0.f, 0.f, 0.f, 0.f};

  fetch();
  stage(0);
  __syncthreads();
  for (int k = 0; k < n_steps; ++k) {                 // every branch here is workgroup-uniform: EXEC stays all ones at the reads
    const bool more = k + 1 < n_steps;
    if (more) fetch();
    const char* xi = smem + (k & 1) * 2 * kWgImage;
    const char* zi = xi + kWgImage;
    v8i16 A[WBM], B[WBN];
#pragma unroll
    for (int i = 0; i < WBM; ++i) A[i] = wgrad_operand(xi, aoff[i][0], aoff[i][1]);
#pragma unroll
    for (int j = 0; j < WBN; ++j) B[j] = wgrad_operand(zi, boff[j][0], boff[j][1]);
#pragma unroll
    for (int i = 0; i < WBM; ++i)
#pragma unroll
      for (int j = 0; j < WBN; ++j) acc[i][j] = wgrad_mfma<BF16>(A[i], B[j], acc[i][j]);
    if (more) stage((k + 1) & 1);
    __syncthreads();
  }

  // accumulator (i, j), register r of lane l: cin = 16 i + 4 (l / 16) + r, cout = 16 j + l % 16 of the wave's blocks
  float* out = a.out + (long long)slice * a.slab_elems + (long long)tap * a.cin * a.cout;
#pragma unroll
  for (int i = 0; i < WBM; ++i)
#pragma unroll
    for (int j = 0; j < WBN; ++j) {
      const int n = n0 + (wn * WBN + j) * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + (wm * WBM + i) * 16 + 4 * g + r;
        if (m < a.cin && n < a.cout) out[(long long)m * a.cout + n] = acc[i][j][r];
      }
    }
}

// dw = slab 0 + slab 1 + ... in slice order
__global__ void conv_wgrad_reduce_kernel(const float* slabs, int slices, long long elems, float* dw) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < elems; i += (long long)gridDim.x * blockDim.x) {
    float s = slabs[i];
    for (int k = 1; k < slices; ++k) s += slabs[(long long)k * elems + i];
    dw[i] = s;
  }
}

int grid_for(long long total) { return (int)std::max<long long>(1, std::min<long long>((total + 255) / 256, 256 * 16)); }

// ---- planner ---------------------------------------------------------------------------------------------------------------------------
struct WgradPlan {
  int tm, tn;               // tile sides (128 or 64 channels)
  int taps, tiles_m, tiles_n, steps, steps_per, slices;
  int64_t slab_elems;
};

int plan_wgrad(const WgradLaunch& c, WgradPlan* p) {
  RON_REQUIRE(dtype_is_half(c.dtype), "conv wgrad: bf16 / f16 only (dtype %d)", c.dtype);
  RON_REQUIRE(c.kh >= 1 && c.kh == c.kw && (c.kh & 1) && c.dil >= 1, "conv wgrad: square odd filters (%d x %d, dilation %d)", c.kh, c.kw, c.dil);
  const int pad = (c.kh - 1) * c.dil / 2;
  RON_REQUIRE(c.x.N == c.dz.N && c.x.H == c.dz.H && c.x.W == c.dz.W && c.x.pad == pad && c.dz.pad == pad && c.x.N > 0 && c.x.H > 0 && c.x.W > 0,
              "conv wgrad: x and dz must share one halo geometry with pad %d", pad);
  RON_REQUIRE(c.x.coff == 0 && c.dz.coff == 0 && c.x.cstride == c.x.C && c.dz.cstride == c.dz.C && c.x.C % 64 == 0 && c.x.C > 0 &&
              c.dz.C % 64 == 0 && c.Cout >= 1 && c.Cout <= c.dz.C, "conv wgrad: whole tensors with channels padded to 64 (cin %d, dz %d, cout %d)",
              c.x.C, c.dz.C, c.Cout);
  RON_REQUIRE(c.guard >= (int64_t)pad * c.x.Wp() + pad, "conv wgrad: x needs %lld guard pixels, has %lld", (long long)pad * c.x.Wp() + pad, (long long)c.guard);
  const int64_t pixels = c.x.pixels();
  RON_REQUIRE(pixels + kWgStep < ((int64_t)1 << 31), "conv wgrad: too many pixels");
  p->taps = c.kh * c.kw;
  p->tm = c.x.C == 64 ? 64 : kWgTile;
  p->tn = c.dz.C == 64 ? 64 : kWgTile;
  p->tiles_m = (c.x.C + p->tm - 1) / p->tm;
  p->tiles_n = (c.dz.C + p->tn - 1) / p->tn;
  p->steps = (int)((pixels + kWgStep - 1) / kWgStep);
  p->slab_elems = (int64_t)p->taps * c.x.C * c.Cout;
  // by shape: about four workgroups per CU (256 CUs; 32 KB of LDS each), slices of >= 8 steps
  const int64_t base = (int64_t)p->taps * p->tiles_m * p->tiles_n;
  int want = c.splitk;
  if (want < 0) want = (int)std::min<int64_t>(std::max<int64_t>(1, 1024 / base), std::max(1, p->steps / 8));
  RON_REQUIRE(want >= 1, "conv wgrad: pixel split %d", c.splitk);
  want = std::min(want, p->steps);
  // a forced split is capped where the slabs would reach 2 GiB (the sum kernel walks them serially per element)
  want = (int)std::min<int64_t>(want, std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / (p->slab_elems * 4)));
  p->steps_per = (p->steps + want - 1) / want;
  p->slices = (p->steps + p->steps_per - 1) / p->steps_per;       // no empty slice
  RON_REQUIRE(base * p->slices < ((int64_t)1 << 31), "conv wgrad: grid too large");
  return RON_OK;
}

template <bool BF16, int WBM, int WBN>
int launch_wgrad_t(const WgradLaunch& c, const WgradPlan& p, hipStream_t s) {
  WgradArgs a = WgradArgs();
  a.x = static_cast<const char*>(c.x.base); a.dz = static_cast<const char*>(c.dz.base);
  a.out = p.slices > 1 ? static_cast<float*>(c.scratch) : c.dw;
  a.slab_elems = p.slab_elems;
  a.cin = c.x.C; a.cop = c.dz.C; a.cout = c.Cout;
  a.Wp = c.x.Wp(); a.pad = c.x.pad; a.dil = c.dil; a.kw = c.kw; a.taps = p.taps;
  a.tiles_m = p.tiles_m; a.tiles_n = p.tiles_n; a.steps = p.steps; a.steps_per = p.steps_per;
  const unsigned grid = (unsigned)((int64_t)p.taps * p.tiles_m * p.tiles_n * p.slices);
  RON_LAUNCH((conv_wgrad_tile_kernel<BF16, WBM, WBN>), dim3(grid), dim3(256), kWgLds, s, a);
  RON_HIP_CHECK(ron::launch_error());
  if (p.slices > 1) {
    RON_LAUNCH(conv_wgrad_reduce_kernel, dim3(grid_for(p.slab_elems)), dim3(256), 0, s, static_cast<const float*>(c.scratch), p.slices, (long long)p.slab_elems, c.dw);
    RON_HIP_CHECK(ron::launch_error());
  }
  return RON_OK;
}

template <bool BF16>
int launch_wgrad_dtype(const WgradLaunch& c, const WgradPlan& p, hipStream_t s) {
  if (p.tm == 64) return p.tn == 64 ? launch_wgrad_t<BF16, 2, 2>(c, p, s) : launch_wgrad_t<BF16, 2, 4>(c, p, s);
  return p.tn == 64 ? launch_wgrad_t<BF16, 4, 2>(c, p, s) : launch_wgrad_t<BF16, 4, 4>(c, p, s);
}

}  // namespace

int conv_wgrad_slices(const WgradLaunch& c) {
  WgradPlan p;
  return plan_wgrad(c, &p) == RON_OK ? p.slices : -1;
}

int64_t conv_wgrad_scratch_bytes(const WgradLaunch& c) {
  WgradPlan p;
  if (plan_wgrad(c, &p) != RON_OK) return -1;
  return p.slices > 1 ? (int64_t)p.slices * p.slab_elems * 4 : 0;
}

int launch_conv_wgrad(const WgradLaunch& c, hipStream_t stream) {
  WgradPlan p;
  int rc = plan_wgrad(c, &p);
  if (rc != RON_OK) return rc;
  RON_REQUIRE(c.x.base != nullptr && c.dz.base != nullptr && c.dw != nullptr, "conv wgrad: NULL tensor");
  RON_REQUIRE(p.slices == 1 || (c.scratch != nullptr && c.scratch_bytes >= (int64_t)p.slices * p.slab_elems * 4),
              "conv wgrad: %d pixel slices need %lld bytes of scratch", p.slices, (long long)p.slices * p.slab_elems * 4);
  return c.dtype == RON_DTYPE_BF16 ? launch_wgrad_dtype<true>(c, p, stream) : launch_wgrad_dtype<false>(c, p, stream);
}

// ---- what the two backward entry points share: the tail of the plan, the checks of a call, the three launch steps ----------------------
namespace {

// (BackwardCore, what both operators decide on the host behind their own descriptor checks: conv_train.h)
int64_t carve(BackwardCore* P, int64_t bytes) {
  const int64_t o = P->total;
  P->total += align_up(bytes, 256);
  return o;
}

int finish_plan(BackwardCore* P) {
  P->conv.out.bytes = P->dx_bytes;
  P->conv.wgt_bytes = P->w_bytes;
  P->sk_bytes = conv_scratch_bytes(P->conv);
  P->slab_bytes = conv_wgrad_scratch_bytes(P->wg);
  if (P->slab_bytes < 0) return RON_ERR_INVALID;
  // bias gradient: at most 512 chunks of >= 32 rows
  P->chunk_rows = std::max<int64_t>(32, (P->rows + 511) / 512);
  P->chunks = (int)((P->rows + P->chunk_rows - 1) / P->chunk_rows);
  P->off_w = carve(P, P->w_bytes);
  P->off_bias = carve(P, (int64_t)P->conv.Npad * 4);
  P->off_dx = carve(P, P->dx_bytes);
  P->off_sk = carve(P, P->sk_bytes);
  P->off_slab = carve(P, P->slab_bytes);
  P->off_part = carve(P, (int64_t)P->chunks * P->sum_cols * 4);
  return RON_OK;
}

// the checks of a call behind its plan; `what` starts every message, `sizer` is the entry that gives the workspace's size
int check_backward_call(const char* what, const char* sizer, const ron_conv_desc* d, const BackwardCore& P, const float* x,
                        const float* w, const float* y, const float* dy, const float* dx, const float* dw, void* workspace,
                        int64_t workspace_bytes) {
  RON_REQUIRE(dy != nullptr, "%s: dy is NULL", what);
  RON_REQUIRE(!d->relu || y != nullptr, "%s: relu is set and y is NULL (the mask is y > 0)", what);
  RON_REQUIRE(dx == nullptr || w != nullptr, "%s: dx needs w", what);
  RON_REQUIRE(dw == nullptr || x != nullptr, "%s: dw needs x", what);
  RON_REQUIRE(workspace != nullptr && workspace_bytes >= P.total, "%s: workspace of %lld bytes, %lld needed (%s)", what,
              (long long)workspace_bytes, (long long)P.total, sizer);
  RON_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: the workspace must be 256-byte aligned", what);
  RON_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)dy) & 15) == 0, "%s: x, y and dy must be 16-byte aligned (they are read 16 bytes at a time)", what);
  if (dx != nullptr) {
    // what launch_conv would refuse is refused here, before anything is enqueued
    ConvLaunch c = P.conv;
    c.in.base = workspace; c.out.base = workspace; c.wgt = workspace; c.bias = static_cast<const float*>(workspace);
    if (P.sk_bytes > 0) { c.scratch = workspace; c.scratch_bytes = P.sk_bytes; }
    int o[4];
    if (int rc = conv_describe(c, o)) return rc;
  }
  return RON_OK;
}

// dense fp32 [n,h,w,csrc] -> `rows` + 2 `guard` pixels of cdst channels in the halo geometry of `pad` (0: a dense tensor)
template <bool BF16>
int launch_pack_halo(const float* src, const float* mask, void* out, int64_t rows, int n, int h, int w, int pad, int csrc, int cdst,
                     int64_t guard, hipStream_t s) {
  PackArgs a = PackArgs();
  a.src = src; a.mask = mask; a.out = static_cast<unsigned short*>(out);
  a.rows = rows + 2 * guard; a.guard = guard;
  a.N = n; a.H = h; a.W = w; a.pad = pad; a.Csrc = csrc; a.Cdst = cdst;
  a.Hs = h; a.Ws = w; a.sstep = 1; a.soff = 0;
  RON_LAUNCH(conv_bwd_pack_halo_kernel<BF16>, dim3(grid_for(a.rows * (cdst / 8))), dim3(256), 0, s, a);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

// the same buffer from a COARSER source: dense fp32 [n,hs,ws,csrc] scattered to pixels (soff + sstep * sy, soff + sstep * sx) of the
// h x w map (the caller guarantees that they all exist), zero at every other pixel
template <bool BF16>
int launch_pack_halo_scatter(const float* src, const float* mask, void* out, int64_t rows, int n, int h, int w, int pad, int csrc,
                             int cdst, int hs, int ws, int sstep, int soff, hipStream_t s) {
  PackArgs a = PackArgs();
  a.src = src; a.mask = mask; a.out = static_cast<unsigned short*>(out);
  a.rows = rows; a.guard = 0;
  a.N = n; a.H = h; a.W = w; a.pad = pad; a.Csrc = csrc; a.Cdst = cdst;
  a.Hs = hs; a.Ws = ws; a.sstep = sstep; a.soff = soff;
  RON_LAUNCH((conv_bwd_pack_halo_kernel<BF16, true>), dim3(grid_for(a.rows * (cdst / 8))), dim3(256), 0, s, a);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

// the data gradient behind the weights' pack: zero bias, the forward launch over dz; *out is the halo tensor it wrote
int launch_data_grad(const BackwardCore& P, void* dzbuf, char* ws, hipStream_t s, TensorView* out) {
  RON_HIP_CHECK(dev_memset_async(ws + P.off_bias, 0, (size_t)P.conv.Npad * 4, s));
  ConvLaunch c = P.conv;
  c.in.base = dzbuf; c.out.base = ws + P.off_dx;
  c.wgt = ws + P.off_w; c.bias = reinterpret_cast<const float*>(ws + P.off_bias);
  if (P.sk_bytes > 0) { c.scratch = ws + P.off_sk; c.scratch_bytes = P.sk_bytes; }
  *out = c.out;
  return launch_conv(c, s);
}

// the weight gradient of the packed operands
int launch_weight_grad(const BackwardCore& P, void* xbase, void* dzbase, float* dw, char* ws, hipStream_t s) {
  WgradLaunch g = P.wg;
  g.x.base = xbase;
  g.dz.base = dzbase;
  g.dw = dw;
  if (P.slab_bytes > 0) { g.scratch = ws + P.off_slab; g.scratch_bytes = P.slab_bytes; }
  return launch_conv_wgrad(g, s);
}

// pass 1 of the bias gradient: the chunks' column sums of dz; returns them ([chunks][sum_cols]) for the operator's second pass
template <bool BF16>
int launch_colsum(const BackwardCore& P, const void* dzbuf, char* ws, hipStream_t s, const float** part) {
  *part = reinterpret_cast<const float*>(ws + P.off_part);
  RON_LAUNCH(conv_bwd_colsum_kernel<BF16>, dim3(P.chunks, P.sum_cols / 64), dim3(256), 0, s, static_cast<const unsigned short*>(dzbuf),
             (long long)P.rows, P.sum_cols, (long long)P.chunk_rows, reinterpret_cast<float*>(ws + P.off_part));
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

// ---- ron_conv2d_backward_nhwc ------------------------------------------------------------------------------------------------------------
// Everything the entry point decides on the host: the descriptor's checks and the carving of the workspace (BackwardPlan, conv_train.h).
int plan_backward(const ron_conv_desc* d, BackwardPlan* P) {
  if (int rc0 = check_conv_desc(d)) return rc0;       // sizes, filter, stride, dilation inside the envelope of the forward; flags 0 or 1
  RON_REQUIRE(d->dtype == RON_DTYPE_BF16 || d->dtype == RON_DTYPE_F16, "conv backward: dtype %d: bf16 or fp16 only (fp32 and f16x3 have no backward)", d->dtype);
  RON_REQUIRE(d->transpose == 0 && d->pool == 0 && d->center_from == 0 && d->in_cstride == 0 && d->in_coff == 0 && d->tile_cfg == -1,
              "conv backward: a plain convolution (transpose, pool, center_from, in_cstride, in_coff = 0, tile_cfg = -1)");
  RON_REQUIRE(d->stride == 1, "conv backward: stride %d: stride-1 SAME convolutions only", d->stride);
  // 7 x 7 is fc6 of the `full` variant (dilation 1 there; nothing runs a dilated one, so none is accepted untested); 5 x 5 has no user
  RON_REQUIRE(d->kh == d->kw && (d->kh == 1 || d->kh == 3 || (d->kh == 7 && d->dilation == 1)),
              "conv backward: filter %d x %d at dilation %d: 1 x 1, 3 x 3, or 7 x 7 at dilation 1 only", d->kh, d->kw, d->dilation);
  RON_REQUIRE(d->dilation >= 1 && d->dilation <= kConvMaxDilation, "conv backward: dilation %d: 1 .. %d (the data gradient is a forward launch)",
              d->dilation, kConvMaxDilation);
  RON_REQUIRE(d->n > 0 && d->h > 0 && d->w > 0 && d->cout >= 1, "conv backward: empty tensor");
  RON_REQUIRE(d->cin > 0 && d->cin % 64 == 0, "conv backward: cin %d must be a multiple of 64 (the 3-channel stem is out of scope)", d->cin);
  RON_REQUIRE(d->splitk == -1 || d->splitk >= 1, "conv backward: pixel split %d (-1 = by shape, 1 = off, S = forced)", d->splitk);
  const int esz = 2;
  P->pad = (d->kh - 1) * d->dilation / 2;
  P->cop = (int)align_up(d->cout, 64);
  P->sum_cols = P->cop;
  P->taps = d->kh * d->kw;
  P->npad = (int)align_up(d->cin, conv_n_tile(d->cin));
  P->pixels = TensorView::halo_pixels(d->n, d->h, d->w, P->pad);
  P->rows = align_up(P->pixels, kWgStep);
  P->guard = (int64_t)P->pad * (d->w + P->pad) + P->pad;
  const int64_t dz_bytes = P->rows * P->cop * esz;
  const int64_t x_bytes = (P->rows + 2 * P->guard) * d->cin * esz;
  P->w_bytes = (int64_t)P->npad * P->taps * P->cop * esz;
  P->dx_bytes = TensorView::halo_pixels(d->n, d->h, d->w, 1) * d->cin * esz;
  const int64_t lim = (int64_t)1 << 31;
  RON_REQUIRE(dz_bytes < lim && x_bytes < lim && P->w_bytes < lim && P->dx_bytes < lim, "conv backward: a packed tensor would reach 2 GiB");
  // the data gradient as a forward launch over dz
  ConvLaunch& c = P->conv;
  c.dtype = d->dtype;
  c.in.N = d->n; c.in.H = d->h; c.in.W = d->w; c.in.C = P->cop; c.in.cstride = P->cop; c.in.pad = P->pad;
  c.in.bytes = P->pixels * P->cop * esz;
  c.out.N = d->n; c.out.H = d->h; c.out.W = d->w; c.out.C = d->cin; c.out.cstride = d->cin; c.out.pad = 1;
  c.Cout = d->cin; c.Npad = P->npad;
  c.kh = d->kh; c.kw = d->kw; c.stride = 1; c.dil = d->dilation; c.cpad = P->pad;
  c.relu = 0; c.Ho = d->h; c.Wo = d->w;
  c.splitk = -1;
  // the weight gradient
  WgradLaunch& g = P->wg;
  g.dtype = d->dtype;
  g.x = c.in; g.x.C = d->cin; g.x.cstride = d->cin; g.x.bytes = P->pixels * d->cin * esz;
  g.dz = c.in;
  g.kh = d->kh; g.kw = d->kw; g.dil = d->dilation; g.Cout = d->cout; g.guard = P->guard; g.splitk = d->splitk;
  P->off_dz = carve(P, dz_bytes);
  P->off_x = carve(P, x_bytes);
  return finish_plan(P);
}

// the data gradient's weights: w (device fp32 HWIO) -> the blocked rows at ws + P.off_w.  The launch run_backward makes in line, as a
// step of its own for conv_train.h (run_backward keeps its text: the dry run's launch trace of the entry point is pinned).
template <bool BF16>
int backward_pack_w(const ron_conv_desc* d, const BackwardPlan& P, const float* w, char* ws, hipStream_t s) {
  WpackArgs wa = WpackArgs();
  wa.w = w; wa.out = reinterpret_cast<unsigned short*>(ws + P.off_w);
  wa.taps = P.taps; wa.cin = d->cin; wa.cout = d->cout; wa.cop = P.cop; wa.npad = P.npad;
  RON_LAUNCH(conv_bwd_pack_weights_kernel<BF16>, dim3(grid_for(P.w_bytes / 16)), dim3(256), 0, s, wa);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

// sstep = 0: y and dy are [n,h,w,cout] (ron_conv2d_backward_nhwc); else they are [n,hs,ws,cout] and dz is their scatter to pixels
// (soff + sstep * oy, soff + sstep * ox) of a zero h x w map (ron_conv2d_padded_backward_nhwc) - everything behind the pack is the same
template <bool BF16>
int run_backward(const ron_conv_desc* d, const BackwardPlan& P, const float* x, const float* w, const float* y, const float* dy,
                 float* dx, float* dw, float* dbias, char* ws, hipStream_t s, int hs = 0, int wsrc = 0, int sstep = 0, int soff = 0) {
  int rc;
  void* dzbuf = ws + P.off_dz;
  if (sstep == 0) rc = launch_pack_halo<BF16>(dy, d->relu ? y : nullptr, dzbuf, P.rows, d->n, d->h, d->w, P.pad, d->cout, P.cop, 0, s);
  else rc = launch_pack_halo_scatter<BF16>(dy, d->relu ? y : nullptr, dzbuf, P.rows, d->n, d->h, d->w, P.pad, d->cout, P.cop, hs, wsrc, sstep, soff, s);
  if (rc) return rc;
  if (dx != nullptr) {
    WpackArgs wa = WpackArgs();
    wa.w = w; wa.out = reinterpret_cast<unsigned short*>(ws + P.off_w);
    wa.taps = P.taps; wa.cin = d->cin; wa.cout = d->cout; wa.cop = P.cop; wa.npad = P.npad;
    RON_LAUNCH(conv_bwd_pack_weights_kernel<BF16>, dim3(grid_for(P.w_bytes / 16)), dim3(256), 0, s, wa);
    RON_HIP_CHECK(ron::launch_error());
    TensorView out;
    if ((rc = launch_data_grad(P, dzbuf, ws, s, &out))) return rc;
    if ((rc = launch_unpack(out, d->dtype, 0, dx, s))) return rc;
  }
  if (dw != nullptr) {
    char* xbuf = ws + P.off_x;
    if ((rc = launch_pack_halo<BF16>(x, nullptr, xbuf, P.rows, d->n, d->h, d->w, P.pad, d->cin, d->cin, P.guard, s))) return rc;
    if ((rc = launch_weight_grad(P, xbuf + P.guard * d->cin * 2, dzbuf, dw, ws, s))) return rc;
  }
  if (dbias != nullptr) {
    const float* part;
    if ((rc = launch_colsum<BF16>(P, dzbuf, ws, s, &part))) return rc;
    RON_LAUNCH(conv_bwd_colsum_final_kernel, dim3(d->cout), dim3(64), 0, s, part, P.chunks, P.cop, dbias);
    RON_HIP_CHECK(ron::launch_error());
  }
  return RON_OK;
}

}  // namespace
}  // namespace ron

extern "C" int64_t ron_conv2d_backward_workspace_bytes(const ron_conv_desc* d) {
  ron::BackwardPlan P;
  if (ron::plan_backward(d, &P) != RON_OK) return -1;
  return P.total;
}

extern "C" int ron_conv2d_backward_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* y, const float* dy,
                                        float* dx, float* dw, float* dbias, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ron;
  BackwardPlan P;
  if (int rc = plan_backward(d, &P)) return rc;
  if (int rc = check_backward_call("conv backward", "ron_conv2d_backward_workspace_bytes", d, P, x, w, y, dy, dx, dw, workspace,
                                   workspace_bytes))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  return d->dtype == RON_DTYPE_BF16 ? run_backward<true>(d, P, x, w, y, dy, dx, dw, dbias, ws, s)
                                    : run_backward<false>(d, P, x, w, y, dy, dx, dw, dbias, ws, s);
}

// ---- ron_conv2d_padded_backward_nhwc: the 3x3 convolutions of the SSD extra blocks ----------------------------------------------------
// pad2d(cpad) + 3x3 VALID at stride s is the stride-1 SAME convolution sampled at (o + s oy, o + s ox), o = 1 - cpad.  So its
// backward is the stride-1 SAME backward of dz scattered to those pixels of a zero map of the input's size: dx, dw and dbias are the
// same sums with zero terms added.  The only new device code is the scatter in the pack (conv_bwd_pack_halo_kernel<.., true>); the
// plan, the data gradient, the weight gradient and the column sums run unchanged on the full-resolution geometry.  At stride 2 that
// is four times the MFMA work of a strided gather, on maps of 32 x 32 and smaller.
namespace ron {
namespace {

struct PaddedPlan : BackwardPlan {
  int ho = 0, wo = 0, soff = 0;
};

int plan_padded(const ron_conv_desc* d, int cpad, PaddedPlan* P) {
  RON_REQUIRE(d != nullptr, "conv padded backward: NULL descriptor");
  if (int rc0 = check_conv_desc(d)) return rc0;
  RON_REQUIRE(d->kh == 3 && d->kw == 3 && d->dilation == 1, "conv padded backward: filter %d x %d, dilation %d: 3 x 3, dilation 1 only (the 4 x 4 of block12 is ron_conv2d_k2s2_backward_nhwc on its inner taps)",
              d->kh, d->kw, d->dilation);
  RON_REQUIRE((d->stride == 2 && cpad == 1) || (d->stride == 1 && cpad == 0),
              "conv padded backward: stride %d with padding %d: (2, 1) = pad2d(1) + stride-2 VALID or (1, 0) = plain VALID only", d->stride, cpad);
  RON_REQUIRE(cpad == 1 || (d->h >= 3 && d->w >= 3), "conv padded backward: map %d x %d: a VALID 3 x 3 convolution needs h, w >= 3", d->h, d->w);
  ron_conv_desc full = *d;          // the stride-1 SAME convolution on the same map
  full.stride = 1;
  if (int rc = plan_backward(&full, P)) return rc;
  P->ho = (d->h + 2 * cpad - 3) / d->stride + 1;
  P->wo = (d->w + 2 * cpad - 3) / d->stride + 1;
  P->soff = 1 - cpad;
  return RON_OK;
}

}  // namespace
}  // namespace ron

extern "C" int64_t ron_conv2d_padded_backward_workspace_bytes(const ron_conv_desc* d, int cpad) {
  ron::PaddedPlan P;
  if (ron::plan_padded(d, cpad, &P) != RON_OK) return -1;
  return P.total;
}

extern "C" int ron_conv2d_padded_backward_nhwc(const ron_conv_desc* d, int cpad, const float* x, const float* w, const float* y, const float* dy,
                                               float* dx, float* dw, float* dbias, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ron;
  PaddedPlan P;
  if (int rc = plan_padded(d, cpad, &P)) return rc;
  if (int rc = check_backward_call("conv padded backward", "ron_conv2d_padded_backward_workspace_bytes", d, P, x, w, y, dy, dx, dw, workspace,
                                   workspace_bytes))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  return d->dtype == RON_DTYPE_BF16 ? run_backward<true>(d, P, x, w, y, dy, dx, dw, dbias, ws, s, P.ho, P.wo, d->stride, P.soff)
                                    : run_backward<false>(d, P, x, w, y, dy, dx, dw, dbias, ws, s, P.ho, P.wo, d->stride, P.soff);
}

// ---- ron_conv2d_k2s2_backward_nhwc: the 2x2 stride-2 convolution and the 2x2 stride-2 transposed convolution ----------------------------
// Kernel == stride: every input pixel meets every output pixel through exactly one tap, so with s2d = space-to-depth
// ([n,2H,2W,C] -> [n,H,W,(ky,kx,C)]) and d2s its inverse both operators are 1x1 convolutions on the coarse H x W grid:
//
//   convolution (x [n,2H,2W,cin], w [2,2,cin,cout], dz [n,H,W,cout])
//     dw.reshape(4 cin, cout) = s2d(xs)^T dz          launch_conv_wgrad, kh = 1: x := s2d(xs), dz := dz
//     dx = d2s(dz @ ws.reshape(4 cin, cout)^T)        launch_conv, 1x1, 4 cin outputs; the depth-to-space happens in the unpack
//     dbias = column sums of dz
//   transposed (x [n,H,W,cin], w [2,2,cout,cin], dz [n,2H,2W,cout]), Dz = s2d(dz) [n,H,W,4 cout]
//     dw.reshape(4 cout, cin) = Dz^T xs               launch_conv_wgrad with the operands' roles swapped: x := Dz, dz := xs
//     dx = Dz @ ws.reshape(4 cout, cin)               launch_conv, 1x1, K = 4 cout
//     dbias[co] = the four taps' column sums of Dz, added in tap order
//
// No new MFMA kernel.  New here: the pack that gathers space-to-depth while it masks, rounds and packs (no fp32 shuffle pass), the
// weights pack for [4 cout] x [cin] (the transposed layout is already K-major per output row: no flip, no swap), the depth-to-space
// unpack and the tap fold of the bias gradient.  The coarse grid has no halo (pad 0, no guard pixels): the only zeros the weight
// gradient relies on are the rows from n H W up to the next multiple of 32, which both packs write.
namespace ron {
namespace {

// dense fp32 [N,2H,2W,C] -> [rows][4 C] of the storage type: row = coarse pixel, column (ky * 2 + kx) * C + c; rows >= N H W zero
struct S2dArgs {
  const float* src;
  const float* mask;        // null: no mask
  unsigned short* out;
  long long rows;
  int N, H, W, C;           // the COARSE grid; C % 8 == 0
};

template <bool BF16>
__global__ void k2s2_pack_s2d_kernel(S2dArgs a) {
  // (every packed tensor is below 2 GiB, plan_k2s2: the 16-byte pieces and the pixels fit 32-bit arithmetic)
  const unsigned vecs = a.C / 2;                    // 4 C / 8
  const unsigned total = (unsigned)a.rows * vecs;
  const unsigned pixels = (unsigned)a.N * a.H * a.W;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned b = i / vecs;
    const int k = (int)(i - b * vecs) * 8;
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (b < pixels) {
      const int t = k / a.C, c = k - t * a.C;
      const unsigned r = b / a.W;
      const int col = (int)(b - r * a.W);
      const unsigned img = r / a.H;
      const int row = (int)(r - img * a.H);
      const long long s0 = (((long long)img * 2 * a.H + 2 * row + (t >> 1)) * 2 * a.W + 2 * col + (t & 1)) * a.C + c;
      const float4 lo = *reinterpret_cast<const float4*>(a.src + s0), hi = *reinterpret_cast<const float4*>(a.src + s0 + 4);
      f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w; f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
      if (a.mask != nullptr) {
        const float4 ml = *reinterpret_cast<const float4*>(a.mask + s0), mh = *reinterpret_cast<const float4*>(a.mask + s0 + 4);
        const float m[8] = {ml.x, ml.y, ml.z, ml.w, mh.x, mh.y, mh.z, mh.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = m[e] > 0.f ? f[e] : 0.f;
      }
    }
    uint4 o;
    o.x = round_bits<BF16>(f[0]) | ((unsigned)round_bits<BF16>(f[1]) << 16);
    o.y = round_bits<BF16>(f[2]) | ((unsigned)round_bits<BF16>(f[3]) << 16);
    o.z = round_bits<BF16>(f[4]) | ((unsigned)round_bits<BF16>(f[5]) << 16);
    o.w = round_bits<BF16>(f[6]) | ((unsigned)round_bits<BF16>(f[7]) << 16);
    *reinterpret_cast<uint4*>(a.out + (long long)i * 8) = o;
  }
}

// weights of the transposed convolution for its data gradient: fp32 [2,2,cout,cin] = [K = 4 cout][cin] on the device -> the blocked rows
// of pack.h, rows[n = ci][k] = round(w[k, ci]) (zero for n >= cin): [Npad / 64][K / 64][64 rows][64 elements]
template <bool BF16>
__global__ void k2s2_pack_weights_kn_kernel(const float* w, unsigned short* out, int K, int cin, int npad) {
  const int steps = K / 64;
  const long long total = (long long)npad * (K / 8);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int piece = (int)(i & 7);
    const int nl = (int)((i >> 3) & 63);
    const long long blk = i >> 9;
    const int kt = (int)(blk % steps), nb = (int)(blk / steps);
    const int n = nb * 64 + nl, k = kt * 64 + piece * 8;
    unsigned short h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = round_bits<BF16>(n < cin ? w[(long long)(k + e) * cin + n] : 0.f);
    uint4 o;
    o.x = h[0] | ((unsigned)h[1] << 16); o.y = h[2] | ((unsigned)h[3] << 16);
    o.z = h[4] | ((unsigned)h[5] << 16); o.w = h[6] | ((unsigned)h[7] << 16);
    *reinterpret_cast<uint4*>(out + i * 8) = o;
  }
}

// dx of the convolution: the 1x1 launch's output, a halo tensor [N,H,W,4 C] (pad 1) of the storage type -> dense fp32 [N,2H,2W,C]
struct D2sArgs {
  const unsigned short* in;
  float* dx;
  int N, H, W, C;           // the coarse grid; C = cin
  int vec_store;            // dx is 16-byte aligned
};

template <bool BF16>
__global__ void k2s2_unpack_d2s_kernel(D2sArgs a) {
  const int groups = a.C / 8;
  const long long total = (long long)a.N * 2 * a.H * 2 * a.W * groups;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(i % groups);
    const long long pix = i / groups;
    const int ox = (int)(pix % (2 * a.W));
    const int oy = (int)((pix / (2 * a.W)) % (2 * a.H));
    const long long img = pix / ((long long)4 * a.W * a.H);
    const long long q = (img * (a.H + 1) + 1 + (oy >> 1)) * (a.W + 1) + 1 + (ox >> 1);
    const uint4 d = *reinterpret_cast<const uint4*>(a.in + q * 4 * a.C + ((oy & 1) * 2 + (ox & 1)) * a.C + g * 8);
    const unsigned u[4] = {d.x, d.y, d.z, d.w};
    float f[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f[2 * e] = bits_to_f<BF16>((unsigned short)(u[e] & 0xFFFFu));
      f[2 * e + 1] = bits_to_f<BF16>((unsigned short)(u[e] >> 16));
    }
    float* o = a.dx + i * 8;
    if (a.vec_store) {
      *reinterpret_cast<float4*>(o) = make_float4(f[0], f[1], f[2], f[3]);
      *reinterpret_cast<float4*>(o + 4) = make_float4(f[4], f[5], f[6], f[7]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f[e];
    }
  }
}

// bias gradient of the transposed convolution: per channel the four taps' column sums of Dz, each summed like
// conv_bwd_colsum_final_kernel does (lanes strided over the chunks, a fixed tree), then added in tap order
__global__ __launch_bounds__(64) void k2s2_colsum_fold_kernel(const float* partial, int chunks, int cols, int cout, float* dbias) {
  const int c = blockIdx.x, lane = threadIdx.x;
  float total = 0.f;
  for (int t = 0; t < 4; ++t) {
    float s = 0.f;
    for (int k = lane; k < chunks; k += 64) s += partial[(long long)k * cols + t * cout + c];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    total = t == 0 ? s : total + s;
  }
  if (lane == 0) dbias[c] = total;
}

struct K2Plan : BackwardCore {
  int H = 0, W = 0;             // the coarse grid
  int ca = 0, cz = 0;           // channels of the two packed operands: A (s2d gathered) and Z (dense)
  int npad = 0, nout = 0;       // rows of the packed weights; outputs of the data-gradient launch
  int kconv = 0;                // K of the data-gradient launch = channels of its input
  int64_t pixels = 0;
  int64_t off_a = 0, off_z = 0;
};

int plan_k2s2(const ron_conv_desc* d, K2Plan* P) {
  if (int rc0 = check_conv_desc(d)) return rc0;       // flags 0 or 1, sizes >= 1
  RON_REQUIRE(d->dtype == RON_DTYPE_BF16 || d->dtype == RON_DTYPE_F16, "conv k2s2 backward: dtype %d: bf16 or fp16 only (fp32 and f16x3 have no backward)", d->dtype);
  RON_REQUIRE(d->pool == 0 && d->center_from == 0 && d->in_cstride == 0 && d->in_coff == 0 && d->tile_cfg == -1,
              "conv k2s2 backward: a plain operator (pool, center_from, in_cstride, in_coff = 0, tile_cfg = -1)");
  RON_REQUIRE(d->kh == 2 && d->kw == 2 && d->stride == 2, "conv k2s2 backward: filter %d x %d, stride %d: 2 x 2 stride 2 only", d->kh, d->kw, d->stride);
  RON_REQUIRE(d->dilation == 1, "conv k2s2 backward: dilation %d: 1 only", d->dilation);
  RON_REQUIRE(d->n > 0 && d->h > 0 && d->w > 0 && d->cout >= 1, "conv k2s2 backward: empty tensor");
  RON_REQUIRE(d->cin > 0 && d->cin % 64 == 0, "conv k2s2 backward: cin %d must be a multiple of 64", d->cin);
  RON_REQUIRE(d->splitk == -1 || d->splitk >= 1, "conv k2s2 backward: pixel split %d (-1 = by shape, 1 = off, S = forced)", d->splitk);
  const bool tr = d->transpose != 0;
  if (tr) RON_REQUIRE(d->cout % 64 == 0, "conv k2s2 backward: transposed: cout %d must be a multiple of 64", d->cout);
  else RON_REQUIRE(d->h % 2 == 0 && d->w % 2 == 0, "conv k2s2 backward: map %d x %d: the strided convolution needs even sides", d->h, d->w);
  const int esz = 2;
  const int64_t lim = (int64_t)1 << 31;
  P->H = tr ? d->h : d->h / 2;
  P->W = tr ? d->w : d->w / 2;
  RON_REQUIRE((int64_t)d->n * P->H * P->W + kWgStep < lim, "conv k2s2 backward: too many pixels");
  const int cop = (int)align_up(d->cout, 64);
  P->ca = tr ? 4 * d->cout : 4 * d->cin;
  P->cz = tr ? d->cin : cop;
  P->kconv = tr ? P->ca : P->cz;
  P->nout = tr ? d->cin : 4 * d->cin;
  P->npad = (int)align_up(P->nout, conv_n_tile(P->nout));
  P->sum_cols = tr ? P->ca : P->cz;
  P->pixels = (int64_t)d->n * P->H * P->W;
  P->rows = align_up(P->pixels, kWgStep);
  const int64_t a_bytes = P->rows * P->ca * esz, z_bytes = P->rows * P->cz * esz;
  P->w_bytes = (int64_t)P->npad * P->kconv * esz;
  P->dx_bytes = TensorView::halo_pixels(d->n, P->H, P->W, 1) * P->nout * esz;
  RON_REQUIRE(a_bytes < lim && z_bytes < lim && P->w_bytes < lim && P->dx_bytes < lim, "conv k2s2 backward: a packed tensor would reach 2 GiB");
  // the data gradient: a 1x1 forward launch on the coarse grid
  ConvLaunch& c = P->conv;
  c.dtype = d->dtype;
  c.in.N = d->n; c.in.H = P->H; c.in.W = P->W; c.in.C = P->kconv; c.in.cstride = P->kconv; c.in.pad = 0;
  c.in.bytes = P->pixels * P->kconv * esz;
  c.out.N = d->n; c.out.H = P->H; c.out.W = P->W; c.out.C = P->nout; c.out.cstride = P->nout; c.out.pad = 1;
  c.Cout = P->nout; c.Npad = P->npad;
  c.kh = 1; c.kw = 1; c.stride = 1; c.dil = 1; c.cpad = 0;
  c.relu = 0; c.Ho = P->H; c.Wo = P->W;
  c.splitk = -1;
  // the weight gradient: x := A, dz := Z
  WgradLaunch& g = P->wg;
  g.dtype = d->dtype;
  g.x = c.in; g.x.C = P->ca; g.x.cstride = P->ca; g.x.bytes = P->pixels * P->ca * esz;
  g.dz = c.in; g.dz.C = P->cz; g.dz.cstride = P->cz; g.dz.bytes = P->pixels * P->cz * esz;
  g.kh = 1; g.kw = 1; g.dil = 1; g.Cout = tr ? d->cin : d->cout; g.guard = 0; g.splitk = d->splitk;
  P->off_a = carve(P, a_bytes);
  P->off_z = carve(P, z_bytes);
  return finish_plan(P);
}

template <bool BF16>
int k2s2_pack_s2d(const float* src, const float* mask, void* out, const K2Plan& P, int n, int c, hipStream_t s) {
  S2dArgs a = S2dArgs();
  a.src = src; a.mask = mask; a.out = static_cast<unsigned short*>(out);
  a.rows = P.rows; a.N = n; a.H = P.H; a.W = P.W; a.C = c;
  RON_LAUNCH(k2s2_pack_s2d_kernel<BF16>, dim3(grid_for(a.rows * (c / 2))), dim3(256), 0, s, a);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

template <bool BF16>
int run_k2s2(const ron_conv_desc* d, const K2Plan& P, const float* x, const float* w, const float* y, const float* dy,
             float* dx, float* dw, float* dbias, char* ws, hipStream_t s) {
  int rc;
  const bool tr = d->transpose != 0;
  const float* mask = d->relu ? y : nullptr;
  void* abuf = ws + P.off_a;
  void* zbuf = ws + P.off_z;
  // dz: the dense operand of the convolution, the gathered one of the transposed convolution
  void* dzbuf = tr ? abuf : zbuf;
  if (tr) rc = k2s2_pack_s2d<BF16>(dy, mask, abuf, P, d->n, d->cout, s);
  else rc = launch_pack_halo<BF16>(dy, mask, zbuf, P.rows, d->n, P.H, P.W, 0, d->cout, P.cz, 0, s);
  if (rc) return rc;
  if (dx != nullptr) {
    unsigned short* wout = reinterpret_cast<unsigned short*>(ws + P.off_w);
    if (tr) {
      RON_LAUNCH(k2s2_pack_weights_kn_kernel<BF16>, dim3(grid_for(P.w_bytes / 16)), dim3(256), 0, s, w, wout, P.kconv, d->cin, P.npad);
    } else {
      // HWIO [2,2,cin,cout] = [4 cin][cout]: the rows of the launch as they stand (conv_bwd_pack_weights_kernel with a single tap)
      WpackArgs wa = WpackArgs();
      wa.w = w; wa.out = wout;
      wa.taps = 1; wa.cin = 4 * d->cin; wa.cout = d->cout; wa.cop = P.cz; wa.npad = P.npad;
      RON_LAUNCH(conv_bwd_pack_weights_kernel<BF16>, dim3(grid_for(P.w_bytes / 16)), dim3(256), 0, s, wa);
    }
    RON_HIP_CHECK(ron::launch_error());
    TensorView out;
    if ((rc = launch_data_grad(P, dzbuf, ws, s, &out))) return rc;
    if (tr) {
      if ((rc = launch_unpack(out, d->dtype, 0, dx, s))) return rc;
    } else {
      D2sArgs u = D2sArgs();
      u.in = reinterpret_cast<const unsigned short*>(ws + P.off_dx); u.dx = dx;
      u.N = d->n; u.H = P.H; u.W = P.W; u.C = d->cin; u.vec_store = ((uintptr_t)dx & 15) == 0;
      RON_LAUNCH(k2s2_unpack_d2s_kernel<BF16>, dim3(grid_for((long long)d->n * d->h * d->w * (d->cin / 8))), dim3(256), 0, s, u);
      RON_HIP_CHECK(ron::launch_error());
    }
  }
  if (dw != nullptr) {
    if (tr) rc = launch_pack_halo<BF16>(x, nullptr, zbuf, P.rows, d->n, P.H, P.W, 0, d->cin, d->cin, 0, s);
    else rc = k2s2_pack_s2d<BF16>(x, nullptr, abuf, P, d->n, d->cin, s);
    if (rc) return rc;
    if ((rc = launch_weight_grad(P, abuf, zbuf, dw, ws, s))) return rc;
  }
  if (dbias != nullptr) {
    const float* part;
    if ((rc = launch_colsum<BF16>(P, dzbuf, ws, s, &part))) return rc;
    if (tr) RON_LAUNCH(k2s2_colsum_fold_kernel, dim3(d->cout), dim3(64), 0, s, part, P.chunks, P.sum_cols, d->cout, dbias);
    else RON_LAUNCH(conv_bwd_colsum_final_kernel, dim3(d->cout), dim3(64), 0, s, part, P.chunks, P.sum_cols, dbias);
    RON_HIP_CHECK(ron::launch_error());
  }
  return RON_OK;
}

}  // namespace
}  // namespace ron

extern "C" int64_t ron_conv2d_k2s2_backward_workspace_bytes(const ron_conv_desc* d) {
  ron::K2Plan P;
  if (ron::plan_k2s2(d, &P) != RON_OK) return -1;
  return P.total;
}

extern "C" int ron_conv2d_k2s2_backward_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* y, const float* dy,
                                             float* dx, float* dw, float* dbias, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ron;
  K2Plan P;
  if (int rc = plan_k2s2(d, &P)) return rc;
  if (int rc = check_backward_call("conv k2s2 backward", "ron_conv2d_k2s2_backward_workspace_bytes", d, P, x, w, y, dy, dx, dw,
                                   workspace, workspace_bytes))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  return d->dtype == RON_DTYPE_BF16 ? run_k2s2<true>(d, P, x, w, y, dy, dx, dw, dbias, ws, s)
                                    : run_k2s2<false>(d, P, x, w, y, dy, dx, dw, dbias, ws, s);
}

// ---- ron_conv2d_forward_nhwc: the forward the entry points above differentiate, fed from DEVICE weights ---------------------------------
// ron_conv2d_nhwc (ops.cpp) is the same launch behind a host pack: it reads w and bias on the host, allocates its operands and
// synchronises.  Here everything that pack does happens on the stream: x goes through the halo pack of the backward (every pixel of the
// buffer written, so nothing is assumed about the workspace), w through conv_fwd_pack_weights_kernel below, the bias through a pad
// kernel, then launch_conv with the by-shape plan and launch_unpack.  The packed operands are byte for byte what setup_conv uploads
// (hwio_to_rows + cast_rows + block_rows, pack_conv_c64_weights, stem_pack_weights), the ConvLaunch is field for field the one it
// builds: for the same inputs y has the same bytes.  Nothing is cached between calls: the optimizer changes w every step.
//
// The weight pack.  HWIO flattened is [K = taps * cin][cout] with cout fastest; the kernels read rows[n = co][k], k fastest, in
// 64 x 64 blocks of 8 KB ([Npad / 64][K / 64][64][64], pack.h block_rows): a blocked 2-D transpose.  One workgroup moves one block through
// LDS.  In: a lane loads 16 bytes (four co) of two adjacent k rows, 8 lanes side by side (128 contiguous bytes per row), rounds and
// writes four dwords {k even | k odd << 16} into tile[co][k / 2].  Out: a lane reads four dwords of one co row and stores 16 bytes, the
// 256 lanes of a pass covering 4 KB of contiguous memory.  Rows are 33 dwords apart: with the 32-bank rule of ds_write_b32 / ds_read_b32
// (lane groups of 32) a write group touches banks 4 ql + (p & 3) + const - ql 0..7, four consecutive p - and a read group
// r + 4 j + const - four consecutive r, j 0..7: all distinct, no conflict in either direction (computed from the bank rule; no
// conflict counter was collected).  cout that is no multiple of 4, or a w that is not 16-byte aligned, takes 4-byte loads behind the
// same staging.
namespace ron {
namespace {

struct FwdWpackArgs {
  const float* w;
  unsigned short* out;
  int K, cout, npad;        // K = taps * cin, a multiple of 64
  int vec;                  // cout % 4 == 0 and w 16-byte aligned: 16-byte loads
};

constexpr int kFwdTileStride = 33;      // dwords between the co rows of the staged block

template <bool BF16>
__global__ __launch_bounds__(256) void conv_fwd_pack_weights_kernel(FwdWpackArgs a) {
  __shared__ unsigned tile[64 * kFwdTileStride];
  const int tid = threadIdx.x;
  const int nbs = a.npad / 64, steps = a.K / 64;
  const long long blocks = (long long)nbs * steps;
  for (long long b = blockIdx.x; b < blocks; b += gridDim.x) {
    // column blocks fastest: neighbouring workgroups read neighbouring 256-byte pieces of the same k rows
    const int nb = (int)(b % nbs);
    const int kt = (int)(b / nbs);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = tid + 256 * it;
      const int p = (i >> 3) & 31, q = (i >> 8) * 8 + (i & 7);      // k pair, co quad of the block
      const int co = nb * 64 + 4 * q;
      const float* r0 = a.w + ((long long)kt * 64 + 2 * p) * a.cout + co;
      const float* r1 = r0 + a.cout;
      float lo[4] = {0.f, 0.f, 0.f, 0.f}, hi[4] = {0.f, 0.f, 0.f, 0.f};
      if (a.vec) {
        if (co < a.cout) {      // (cout % 4 == 0: the whole quad is inside)
          const float4 l = *reinterpret_cast<const float4*>(r0), h = *reinterpret_cast<const float4*>(r1);
          lo[0] = l.x; lo[1] = l.y; lo[2] = l.z; lo[3] = l.w; hi[0] = h.x; hi[1] = h.y; hi[2] = h.z; hi[3] = h.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (co + e < a.cout) { lo[e] = r0[e]; hi[e] = r1[e]; }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) tile[(4 * q + e) * kFwdTileStride + p] = round_bits<BF16>(lo[e]) | ((unsigned)round_bits<BF16>(hi[e]) << 16);
    }
    __syncthreads();
    unsigned short* blk = a.out + ((long long)nb * steps + kt) * 4096;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int i = tid + 256 * it;
      const int j = i & 7, r = i >> 3;
      const unsigned* t = tile + r * kFwdTileStride + 4 * j;
      uint4 o;
      o.x = t[0]; o.y = t[1]; o.z = t[2]; o.w = t[3];
      *reinterpret_cast<uint4*>(blk + r * 64 + j * 8) = o;
    }
    __syncthreads();
  }
}

// the transposed convolution's weights [2,2,cout,cin] = rows[n = t * cout + co][k = ci] as they stand: a cast and the blocking
template <bool BF16>
__global__ void conv_fwd_pack_rows_kernel(const float* w, unsigned short* out, int K, int npad, int vec) {
  const int steps = K / 64;
  const long long total = (long long)npad * (K / 8);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int piece = (int)(i & 7);
    const int nl = (int)((i >> 3) & 63);
    const long long blk = i >> 9;
    const int kt = (int)(blk % steps), nb = (int)(blk / steps);
    const float* src = w + ((long long)nb * 64 + nl) * K + kt * 64 + piece * 8;
    float f[8];
    if (vec) {
      const float4 lo = *reinterpret_cast<const float4*>(src), hi = *reinterpret_cast<const float4*>(src + 4);
      f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w; f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = src[e];
    }
    uint4 o;
    o.x = round_bits<BF16>(f[0]) | ((unsigned)round_bits<BF16>(f[1]) << 16);
    o.y = round_bits<BF16>(f[2]) | ((unsigned)round_bits<BF16>(f[3]) << 16);
    o.z = round_bits<BF16>(f[4]) | ((unsigned)round_bits<BF16>(f[5]) << 16);
    o.w = round_bits<BF16>(f[6]) | ((unsigned)round_bits<BF16>(f[7]) << 16);
    *reinterpret_cast<uint4*>(out + i * 8) = o;
  }
}

// The small images, one element per lane (a few KB each).  `what`:
//   0  the stem's im2col rows [64][64]: rows[n][k] = w[k][n] for k < 27, else 0 (one K step: blocked = plain)
//   1  the stem kernel's fragments (stem.hip, stem_pack_weights): fragment (t, s), lane (r, h), element j = w[k = 16 s + 8 h + j][2 r + t]
//   2  the resident-weight kernel's LDS images (conv_c64.hip, pack_conv_c64_weights) of a 3x3 filter over 64 channels
template <bool BF16>
__global__ void conv_fwd_pack_small_kernel(const float* w, unsigned short* out, int what, int cout, int total) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    float v = 0.f;
    if (what == 0) {
      const int n = i >> 6, k = i & 63;
      if (k < 27 && n < cout) v = w[k * cout + n];
    } else if (what == 1) {
      const int j = i & 7, lane = (i >> 3) & 63, ts = i >> 9;
      const int k = 16 * (ts & 1) + 8 * (lane >> 5) + j, ch = 2 * (lane & 31) + (ts >> 1);
      if (k < 27) v = w[k * 64 + ch];
    } else {
      const int e = i & 7, slot = (i >> 3) & 7, row = (i >> 6) & 63, rest = i >> 12;
      const int tap = rest % 9, hf = rest / 9;
      const int cin = (slot ^ (((row >> 1) & 3) << 1)) * 8 + e, ch = 64 * hf + 4 * (row % 16) + row / 16;
      v = w[((long long)tap * 64 + cin) * cout + ch];
    }
    out[i] = round_bits<BF16>(v);
  }
}

// bias [cout] (or none) -> [total] floats: `live` values bias[i % cout], then zeros (the transposed form repeats it per tap)
__global__ void conv_fwd_pad_bias_kernel(const float* bias, float* out, int cout, int live, int total) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x)
    out[i] = (bias != nullptr && i < live) ? bias[i % cout] : 0.f;
}

enum { kFwdPlain = 0, kFwdStrided, kFwdTransposed, kFwdStem, kFwdStemIm2col };

// Everything the entry point decides on the host: the descriptor's checks, the ConvLaunch of setup_conv, the carving of the workspace
// (ForwardPlan, conv_train.h)
static_assert(kFwdPlain == 0, "ForwardPlan::kind defaults to the plain convolution");

TensorView dense_view(int n, int h, int w, int c, int pad) {
  TensorView v;
  v.N = n; v.H = h; v.W = w; v.C = c; v.cstride = c; v.coff = 0; v.pad = pad;
  v.bytes = TensorView::halo_pixels(n, h, w, pad) * c * 2;
  return v;
}

int plan_forward(const ron_conv_desc* d, ForwardPlan* P) {
  if (int rc0 = check_conv_desc(d)) return rc0;       // sizes, filter, stride, dilation inside the envelope; flags 0 or 1
  RON_REQUIRE(d->dtype == RON_DTYPE_BF16 || d->dtype == RON_DTYPE_F16, "conv forward: dtype %d: bf16 or fp16 only (fp32 and f16x3 run through ron_conv2d_nhwc)", d->dtype);
  RON_REQUIRE(d->pool == 0 && d->center_from == 0 && d->in_cstride == 0 && d->in_coff == 0 && d->tile_cfg == -1 && d->splitk == -1,
              "conv forward: a plain operator planned by shape (pool, center_from, in_cstride, in_coff = 0, tile_cfg = -1, splitk = -1)");
  RON_REQUIRE(d->kh == d->kw, "conv forward: filter %d x %d: square filters only", d->kh, d->kw);
  const bool k2s2 = d->kh == 2 && d->stride == 2 && d->dilation == 1;
  int ho = d->h, wo = d->w;
  ConvLaunch& c = P->conv;
  if (d->transpose) {
    RON_REQUIRE(k2s2, "conv forward: transposed: filter %d x %d, stride %d, dilation %d: 2 x 2 stride 2 only", d->kh, d->kw, d->stride, d->dilation);
    RON_REQUIRE(d->cin % 64 == 0, "conv forward: cin %d must be a multiple of 64", d->cin);
    RON_REQUIRE(d->cout % 128 == 0, "conv forward: transposed: cout %d must be a multiple of 128", d->cout);
    P->kind = kFwdTransposed;
    ho = 2 * d->h; wo = 2 * d->w;
    c.Cout = c.Npad = 4 * d->cout;
    c.up = 2; c.up_cout = d->cout;
    c.kh = c.kw = 1; c.stride = 1; c.dil = 1; c.cpad = 0;
    c.Ho = d->h; c.Wo = d->w;
    P->K = d->cin;
  } else if (d->stride != 1) {
    RON_REQUIRE(k2s2, "conv forward: stride %d with a %d x %d filter at dilation %d: the only strided convolution is 2 x 2 at stride 2", d->stride, d->kh,
                d->kw, d->dilation);
    RON_REQUIRE(d->h % 2 == 0 && d->w % 2 == 0, "conv forward: map %d x %d: the strided convolution needs even sides", d->h, d->w);
    RON_REQUIRE(d->cin % 64 == 0, "conv forward: cin %d must be a multiple of 64", d->cin);
    P->kind = kFwdStrided;
    ho = d->h / 2; wo = d->w / 2;
    c.kh = c.kw = 2; c.stride = 2; c.dil = 1; c.cpad = 0;
    P->K = 4 * d->cin;
  } else if (d->cin == 3) {
    RON_REQUIRE(d->kh == 3 && d->dilation == 1 && d->cout == 64, "conv forward: a 3-channel input: the 3 x 3, 3 -> 64 stem at dilation 1 only (%d x %d, cout %d, dilation %d)",
                d->kh, d->kw, d->cout, d->dilation);
    // the routes of ron_conv2d_nhwc: with the ReLU the stem kernel, without it (the kernel has it built in) im2col + one GEMM step
    P->kind = d->relu ? kFwdStem : kFwdStemIm2col;
    c.kh = c.kw = 1; c.stride = 1; c.dil = 1; c.cpad = 0;
    P->K = 64;
  } else {
    RON_REQUIRE(d->kh == 1 || d->kh == 3 || (d->kh == 7 && d->dilation == 1),
                "conv forward: filter %d x %d at dilation %d: 1 x 1, 3 x 3, or 7 x 7 at dilation 1 only", d->kh, d->kw, d->dilation);
    RON_REQUIRE(d->cin % 64 == 0, "conv forward: cin %d must be a multiple of 64 (or the 3-channel stem)", d->cin);
    P->pad = (d->kh - 1) * d->dilation / 2;
    c.kh = d->kh; c.kw = d->kw; c.stride = 1; c.dil = d->dilation; c.cpad = P->pad;
    P->K = d->kh * d->kw * d->cin;
  }
  if (P->kind != kFwdTransposed) {
    c.Cout = d->cout;
    c.Npad = (int)align_up(d->cout, conv_n_tile(d->cout));
    c.Ho = ho; c.Wo = wo;
  }
  c.dtype = d->dtype;
  c.relu = d->relu;
  c.cfg = -1; c.splitk = -1;
  const bool stem = P->kind == kFwdStem || P->kind == kFwdStemIm2col;
  c.in = dense_view(d->n, d->h, d->w, stem ? 64 : d->cin, P->pad);
  c.out = dense_view(d->n, ho, wo, d->cout, 1);
  const int64_t lim = (int64_t)1 << 31;
  P->x_bytes = P->kind == kFwdStem ? 0 : c.in.bytes;       // the stem kernel reads the fp32 image itself
  P->w_bytes = P->kind == kFwdStem ? 4 * 64 * 8 * 2 : (int64_t)c.Npad * P->K * 2;
  P->out_bytes = c.out.bytes;
  RON_REQUIRE(P->x_bytes < lim && P->w_bytes < lim && P->out_bytes < lim, "conv forward: a packed tensor would reach 2 GiB");
  c.wgt_bytes = P->w_bytes;
  P->c64 = P->kind == kFwdPlain && d->kh == 3 && d->cin == 64 && c.Npad == d->cout;
  if (P->c64) P->c64_bytes = (int64_t)(c.Npad / 64) * 9 * 64 * 64 * 2;
  P->bias_total = P->kind == kFwdStem ? 64 : c.Npad;
  P->bias_live = P->kind == kFwdTransposed ? c.Npad : d->cout;
  if (P->kind != kFwdStem) {
    static const char present = 0;      // conv_c64_applicable asks whether the images exist, not where
    ConvLaunch probe = c;
    if (P->c64) probe.wgt_c64 = &present;
    P->sk_bytes = conv_scratch_bytes(probe);
  }
  auto carve_fwd = [P](int64_t bytes) {
    const int64_t o = P->total;
    P->total += align_up(bytes, 256);
    return o;
  };
  P->off_x = carve_fwd(P->x_bytes);
  P->off_w = carve_fwd(P->w_bytes);
  P->off_c64 = carve_fwd(P->c64_bytes);
  P->off_bias = carve_fwd((int64_t)P->bias_total * 4);
  P->off_out = carve_fwd(P->out_bytes);
  P->off_sk = carve_fwd(P->sk_bytes);
  return RON_OK;
}

// the launch of a plan over a workspace
ConvLaunch forward_launch(const ForwardPlan& P, char* ws) {
  ConvLaunch c = P.conv;
  c.in.base = ws + P.off_x; c.out.base = ws + P.off_out;
  c.wgt = ws + P.off_w; c.bias = reinterpret_cast<const float*>(ws + P.off_bias);
  if (P.c64) c.wgt_c64 = ws + P.off_c64;
  if (P.sk_bytes > 0) { c.scratch = ws + P.off_sk; c.scratch_bytes = P.sk_bytes; }
  return c;
}

// step 1: x -> the launch's input tensor (the stem kernel reads the fp32 image itself)
template <bool BF16>
int forward_pack_x(const ron_conv_desc* d, const ForwardPlan& P, const ConvLaunch& c, const float* x, hipStream_t s) {
  if (P.kind == kFwdStem) return RON_OK;
  if (P.kind == kFwdStemIm2col) return launch_im2col_c3(x, d->n, d->h, d->w, d->dtype, c.in.base, 64, s);
  return launch_pack_halo<BF16>(x, nullptr, c.in.base, c.in.pixels(), d->n, d->h, d->w, P.pad, d->cin, d->cin, 0, s);
}

// step 2: w and bias -> what the launch reads
template <bool BF16>
int forward_pack_w(const ron_conv_desc* d, const ForwardPlan& P, const ConvLaunch& c, const float* w, const float* bias, char* ws, hipStream_t s) {
  unsigned short* wout = reinterpret_cast<unsigned short*>(ws + P.off_w);
  const int w_vec16 = ((uintptr_t)w & 15) == 0;
  if (P.kind == kFwdStem || P.kind == kFwdStemIm2col) {
    const int total = (int)(P.w_bytes / 2);
    RON_LAUNCH(conv_fwd_pack_small_kernel<BF16>, dim3(grid_for(total)), dim3(256), 0, s, w, wout, P.kind == kFwdStem ? 1 : 0, d->cout, total);
  } else if (P.kind == kFwdTransposed) {
    RON_LAUNCH(conv_fwd_pack_rows_kernel<BF16>, dim3(grid_for(P.w_bytes / 16)), dim3(256), 0, s, w, wout, P.K, c.Npad, w_vec16);
  } else {
    FwdWpackArgs a = FwdWpackArgs();
    a.w = w; a.out = wout; a.K = P.K; a.cout = d->cout; a.npad = c.Npad;
    a.vec = w_vec16 && d->cout % 4 == 0;
    const long long blocks = (long long)(c.Npad / 64) * (P.K / 64);
    RON_LAUNCH(conv_fwd_pack_weights_kernel<BF16>, dim3((unsigned)std::min<long long>(blocks, 1 << 20)), dim3(256), 0, s, a);
  }
  RON_HIP_CHECK(ron::launch_error());
  if (P.c64) {
    const int total = (int)(P.c64_bytes / 2);
    RON_LAUNCH(conv_fwd_pack_small_kernel<BF16>, dim3(grid_for(total)), dim3(256), 0, s, w, reinterpret_cast<unsigned short*>(ws + P.off_c64), 2, d->cout, total);
    RON_HIP_CHECK(ron::launch_error());
  }
  RON_LAUNCH(conv_fwd_pad_bias_kernel, dim3(grid_for(P.bias_total)), dim3(256), 0, s, bias, reinterpret_cast<float*>(ws + P.off_bias), d->cout, P.bias_live,
             P.bias_total);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

// the steps of `parts` (RON_FWD_PART_*) in order; step 3 is the launch of ron_conv2d_nhwc on the packed operands, step 4 delivers y
template <bool BF16>
int run_forward(const ron_conv_desc* d, const ForwardPlan& P, const float* x, const float* w, const float* bias, float* y, char* ws, hipStream_t s,
                int parts) {
  int rc;
  const ConvLaunch c = forward_launch(P, ws);
  if ((parts & RON_FWD_PART_X) && (rc = forward_pack_x<BF16>(d, P, c, x, s))) return rc;
  if ((parts & RON_FWD_PART_W) && (rc = forward_pack_w<BF16>(d, P, c, w, bias, ws, s))) return rc;
  if (parts & RON_FWD_PART_LAUNCH) {
    rc = P.kind == kFwdStem ? launch_stem_conv(x, d->n, d->h, d->w, d->dtype, c.wgt, c.bias, c.out, s) : launch_conv(c, s);
    if (rc) return rc;
  }
  return (parts & RON_FWD_PART_UNPACK) ? launch_unpack(c.out, d->dtype, 0, y, s) : RON_OK;
}

}  // namespace

// ---- conv_train.h: the plans and steps above, for the network-level chain (conv_chain.hip) ---------------------------------------------
int train_plan_forward(const ron_conv_desc* d, ForwardPlan* P) { return plan_forward(d, P); }
int train_plan_backward(const ron_conv_desc* d, BackwardPlan* P) { return plan_backward(d, P); }
ConvLaunch train_forward_launch(const ForwardPlan& P, char* ws) { return forward_launch(P, ws); }

int train_pack_halo(int dtype, const float* src, const float* mask, void* out, int64_t rows, int n, int h, int w, int pad, int csrc,
                    int cdst, int64_t guard, hipStream_t s) {
  return dtype == RON_DTYPE_BF16 ? launch_pack_halo<true>(src, mask, out, rows, n, h, w, pad, csrc, cdst, guard, s)
                                 : launch_pack_halo<false>(src, mask, out, rows, n, h, w, pad, csrc, cdst, guard, s);
}

int train_forward_pack_w(const ron_conv_desc* d, const ForwardPlan& P, const ConvLaunch& c, const float* w, const float* bias, char* ws,
                         hipStream_t s) {
  return d->dtype == RON_DTYPE_BF16 ? forward_pack_w<true>(d, P, c, w, bias, ws, s) : forward_pack_w<false>(d, P, c, w, bias, ws, s);
}

int train_backward_pack_w(const ron_conv_desc* d, const BackwardPlan& P, const float* w, char* ws, hipStream_t s) {
  return d->dtype == RON_DTYPE_BF16 ? backward_pack_w<true>(d, P, w, ws, s) : backward_pack_w<false>(d, P, w, ws, s);
}

int train_data_grad(const BackwardCore& P, void* dzbuf, char* ws, hipStream_t s, TensorView* out) { return launch_data_grad(P, dzbuf, ws, s, out); }

int train_weight_grad(const BackwardCore& P, void* xbase, void* dzbase, float* dw, char* ws, hipStream_t s) {
  return launch_weight_grad(P, xbase, dzbase, dw, ws, s);
}

int train_bias_grad(int dtype, const BackwardPlan& P, const void* dzbuf, char* ws, int cout, float* dbias, hipStream_t s) {
  const float* part;
  if (int rc = dtype == RON_DTYPE_BF16 ? launch_colsum<true>(P, dzbuf, ws, s, &part) : launch_colsum<false>(P, dzbuf, ws, s, &part)) return rc;
  RON_LAUNCH(conv_bwd_colsum_final_kernel, dim3(cout), dim3(64), 0, s, part, P.chunks, P.cop, dbias);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

}  // namespace ron

extern "C" int64_t ron_conv2d_forward_workspace_bytes(const ron_conv_desc* d) {
  ron::ForwardPlan P;
  if (ron::plan_forward(d, &P) != RON_OK) return -1;
  return P.total;
}

extern "C" int ron_conv2d_forward_parts_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* bias, float* y, void* workspace,
                                             int64_t workspace_bytes, int parts, void* stream) {
  using namespace ron;
  RON_REQUIRE(parts >= 1 && parts <= RON_FWD_PART_ALL, "conv forward: parts %d: a non-empty set of RON_FWD_PART_*", parts);
  ForwardPlan P;
  if (int rc = plan_forward(d, &P)) return rc;
  RON_REQUIRE(x != nullptr && w != nullptr && y != nullptr, "conv forward: x, w or y is NULL");
  RON_REQUIRE(workspace != nullptr && workspace_bytes >= P.total, "conv forward: workspace of %lld bytes, %lld needed (ron_conv2d_forward_workspace_bytes)",
              (long long)workspace_bytes, (long long)P.total);
  RON_REQUIRE(((uintptr_t)workspace & 255) == 0, "conv forward: the workspace must be 256-byte aligned");
  const bool stem = P.kind == kFwdStem || P.kind == kFwdStemIm2col;
  RON_REQUIRE(((uintptr_t)x & (stem ? 3 : 15)) == 0 && ((uintptr_t)y & 15) == 0,
              "conv forward: x and y must be 16-byte aligned (x of the 3-channel stem: 4-byte)");
  RON_REQUIRE((((uintptr_t)w | (uintptr_t)bias) & 3) == 0, "conv forward: w and bias must be 4-byte aligned");
  char* ws = static_cast<char*>(workspace);
  if (P.kind != kFwdStem) {
    // what launch_conv would refuse is refused here, before anything is enqueued
    int o[4];
    if (int rc = conv_describe(forward_launch(P, ws), o)) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  return d->dtype == RON_DTYPE_BF16 ? run_forward<true>(d, P, x, w, bias, y, ws, s, parts) : run_forward<false>(d, P, x, w, bias, y, ws, s, parts);
}

extern "C" int ron_conv2d_forward_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* bias, float* y, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  return ron_conv2d_forward_parts_nhwc(d, x, w, bias, y, workspace, workspace_bytes, RON_FWD_PART_ALL, stream);
}
