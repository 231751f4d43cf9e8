// Training-mode batch normalisation, forward and backward (ron_batchnorm_train_nhwc, ron_batchnorm_backward_nhwc): the twenty
// slim.batch_norm layers of the RON heads under ron_arg_scope(is_training=True) (nets/ron_vgg_320.py:616-624), each followed by ReLU.
//
//   M = n h w, xs = round(x) to the storage type (a convolution's output as this library stores it)
//   forward   mean = sum(xs) / M, var = sum((xs - mean)^2) / M (biased: the one that normalises), rstd = 1 / sqrt(var + eps)
//             y = round(act(gamma (xs - mean) rstd + beta))
//             moving_mean = decay moving_mean + (1 - decay) mean,  moving_var likewise with var M / max(M - 1, 1)
//   backward  dz = round(dy (y > 0)) with relu, else round(dy);  xhat = (xs - mean) rstd
//             dbeta = sum(dz), dgamma = sum(dz xhat), dx = round(gamma rstd (dz - dbeta / M - xhat dgamma / M))
//
// Bandwidth bound, so the fewest passes over the fp32 tensors: the forward reads x twice and writes y, the backward reads x, dy (and
// y) twice and writes dx.  Every pass has the same geometry, a function of the shape alone (plan):
//
//   a lane owns 4 adjacent channels (one 16-byte access); `lpr` lanes side by side cover a row's channel tile, 64 / lpr rows share a
//   wave, a workgroup of 4 waves covers `rpb` rows at a time; the rows are cut into `slices` slices of `slice_rows` rows (a power of
//   two, a multiple of rpb), blockIdx.x = slice, blockIdx.y = channel tile; inside a slice row lane rl takes rows rl, rl + rpb, ...
//
// Statistics in ONE read of x, never as E[x^2] - mean^2: a lane shifts by the first value it meets (K), adds d = xs - K and d^2,
// and ends with (count, mean = K + s1 / count, M2 = s2 - s1^2 / count); the row lanes of a workgroup, then a channel's slices, are
// merged with Chan's formula behind a fixed binary tree (lane i with lane i + stride, the stride halving).  All counts follow
// from the shape, so the same inputs give the same bytes; with M and hence every count a power of two each merge joins equal counts
// and small-integer inputs come out exact.  The gradient sums take the same route with plain additions.  No atomics anywhere.
//
// Every kernel that touches a [M][c] tensor takes its PLACE as a template parameter (DensePlace: the entry points' fp32 dense tensors;
// HaloPlace: a storage-type halo view of the head chain, batchnorm.h / conv_chain.hip).  The geometry, the lane that owns a value and
// the order of every sum do not depend on the place, so the chain's statistics and gradient sums have the operators' bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "batchnorm.h"
#include "common.h"
#include "storage_device.h"      // round_storage, bits_to_f, round_bits, halo_off

namespace ron {
namespace {

constexpr int kBnThreads = 256;
constexpr int kBnMaxSlices = 1024;      // 4 per thread of the merge kernels
constexpr int64_t kBnMaxRows = (int64_t)1 << 24;      // counts stay exact in fp32

// the geometry every kernel of an operator call shares
RON_KERNEL_ARGS_BEGIN
struct BnGeom {
  long long rows;           // M
  long long slice_rows;
  int c, cg;                // channels, groups of 4 channels
  int lpr, lpr_log2;        // lanes per row of a channel tile (a power of two <= 64)
  int rpb;                  // rows a workgroup covers at a time: 256 / lpr
  int slices, tiles;
  int fill_ = 0;
};
RON_KERNEL_ARGS_END(BnGeom)

struct BnPlan : BnGeom {
  int64_t off_part = 0, off_fin = 0, total = 0;
};

struct Stat4 { float v[4]; };

__device__ __forceinline__ void load4(const float* p, float* o) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
}
__device__ __forceinline__ void store4(float* p, const float* o) { *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]); }

// ---- the place of a [rows][c] tensor: where row r, channels ch .. ch + 3 of the walk lie ------------------------------------------------
// DensePlace: fp32 dense NHWC, the operators' boundary (one 16-byte access).  HaloPlace: a storage-type halo tensor of the chain
// (conv_chain.hip), possibly a channel slice of a wider one: row r of the dense walk is pixel (img, y, x) = halo_off, so every lane
// meets the same values in the same order as in the dense walk and the sums have the same bytes.  4 channels are 8 bytes there; the
// lanes of a row are adjacent, so a wave still reads or writes whole 128-byte pieces of a pixel's channels.
RON_KERNEL_ARGS_BEGIN
struct DensePlace {
  float* p;
};
RON_KERNEL_ARGS_END(DensePlace)
RON_KERNEL_ARGS_BEGIN
struct HaloPlace {
  unsigned short* p;        // halo pixel 0, channel 0 of the allocation
  int H, W, pad, cs, coff;  // the map, its halo, elements per pixel, first channel of the slice
  int fill_ = 0;
};
RON_KERNEL_ARGS_END(HaloPlace)

__device__ __forceinline__ long long place_off(const DensePlace&, const BnGeom& g, long long row, long long ch) { return row * g.c + ch; }
__device__ __forceinline__ long long place_off(const HaloPlace& t, const BnGeom&, long long row, long long ch) {
  // (rows <= 2^24: 32-bit divisions)
  const unsigned r = (unsigned)row, hw = (unsigned)(t.H * t.W);
  const unsigned img = r / hw, rem = r - img * hw;
  const unsigned y = rem / (unsigned)t.W, x = rem - y * (unsigned)t.W;
  return halo_off(img, (int)y, (int)x, t.H, t.W, t.pad, t.cs) + t.coff + ch;
}
template <bool BF16> __device__ __forceinline__ void place_load(const DensePlace& t, const BnGeom& g, long long row, long long ch, float* o) {
  load4(t.p + place_off(t, g, row, ch), o);
}
template <bool BF16> __device__ __forceinline__ void place_load(const HaloPlace& t, const BnGeom& g, long long row, long long ch, float* o) {
  const uint2 v = *reinterpret_cast<const uint2*>(t.p + place_off(t, g, row, ch));
  o[0] = bits_to_f<BF16>((unsigned short)(v.x & 0xFFFFu)); o[1] = bits_to_f<BF16>((unsigned short)(v.x >> 16));
  o[2] = bits_to_f<BF16>((unsigned short)(v.y & 0xFFFFu)); o[3] = bits_to_f<BF16>((unsigned short)(v.y >> 16));
}
// o holds storage-type values (every caller rounds first): the halo place stores their bits
template <bool BF16> __device__ __forceinline__ void place_store(const DensePlace& t, const BnGeom& g, long long row, long long ch, const float* o) {
  store4(t.p + place_off(t, g, row, ch), o);
}
template <bool BF16> __device__ __forceinline__ void place_store(const HaloPlace& t, const BnGeom& g, long long row, long long ch, const float* o) {
  uint2 v;
  v.x = round_bits<BF16>(o[0]) | ((unsigned)round_bits<BF16>(o[1]) << 16);
  v.y = round_bits<BF16>(o[2]) | ((unsigned)round_bits<BF16>(o[3]) << 16);
  *reinterpret_cast<uint2*>(t.p + place_off(t, g, row, ch)) = v;
}

// Chan's merge of (nb, mb, Mb) into (na, ma, Ma); an empty side changes nothing, equal counts give f = 1/2 exactly
__device__ __forceinline__ void chan_merge(float& na, float* ma, float* Ma, float nb, const float* mb, const float* Mb) {
  if (nb == 0.f) return;
  if (na == 0.f) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { ma[e] = mb[e]; Ma[e] = Mb[e]; }
    na = nb;
    return;
  }
  const float n = na + nb, f = nb / n, w = na * f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float delta = mb[e] - ma[e];
    ma[e] = ma[e] + delta * f;
    Ma[e] = (Ma[e] + Mb[e]) + (delta * delta) * w;
  }
  na = n;
}

// rows of slice s, and of them those of row lane rl
__device__ __forceinline__ long long slice_count(const BnGeom& g, long long s) {
  const long long left = g.rows - s * g.slice_rows;
  return left < g.slice_rows ? left : g.slice_rows;
}

// ---- forward, pass 1: per slice (mean, M2) of every channel -> part [slices][2][c] ---------------------------------------------------
template <bool BF16, class PL>
__global__ __launch_bounds__(kBnThreads) void bn_stats_kernel(BnGeom g, PL x, float* __restrict__ part) {
  __shared__ float sh_n[kBnThreads];
  __shared__ Stat4 sh_mean[kBnThreads], sh_m2[kBnThreads];
  const int tid = threadIdx.x, gl = tid & (g.lpr - 1), rl = tid >> g.lpr_log2;
  const int cgi = blockIdx.y * g.lpr + gl;
  const bool active = cgi < g.cg;
  const long long r0 = (long long)blockIdx.x * g.slice_rows, cnt = slice_count(g, blockIdx.x);
  float n = 0.f, mean[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
  if (active && rl < cnt) {
    const long long row = r0 + rl, ch = (long long)cgi * 4;
    const int mine = (int)((cnt - rl + g.rpb - 1) / g.rpb);
    float k[4], s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    place_load<BF16>(x, g, row, ch, k);
#pragma unroll
    for (int e = 0; e < 4; ++e) k[e] = round_storage<BF16>(k[e]);
#pragma unroll 4
    for (int i = 1; i < mine; ++i) {
      float v[4];
      place_load<BF16>(x, g, row + (long long)i * g.rpb, ch, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = round_storage<BF16>(v[e]) - k[e];
        s1[e] += d;
        s2[e] += d * d;
      }
    }
    n = (float)mine;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float q = s1[e] / n, v = s2[e] - s1[e] * q;
      mean[e] = k[e] + q;
      m2[e] = v < 0.f ? 0.f : v;          // (a NaN stays a NaN)
    }
  }
  sh_n[tid] = n;
#pragma unroll
  for (int e = 0; e < 4; ++e) { sh_mean[tid].v[e] = mean[e]; sh_m2[tid].v[e] = m2[e]; }
  __syncthreads();
  for (int off = kBnThreads / 2; off >= g.lpr; off >>= 1) {
    if (tid < off) {
      chan_merge(n, mean, m2, sh_n[tid + off], sh_mean[tid + off].v, sh_m2[tid + off].v);
      sh_n[tid] = n;
#pragma unroll
      for (int e = 0; e < 4; ++e) { sh_mean[tid].v[e] = mean[e]; sh_m2[tid].v[e] = m2[e]; }
    }
    __syncthreads();
  }
  if (rl == 0 && active) {
    float* o = part + (long long)blockIdx.x * 2 * g.c + (long long)cgi * 4;
    store4(o, mean);
    store4(o + g.c, m2);
  }
}

// ---- forward, pass 2: one workgroup per 4 channels merges the slices: thread t its slices 4t .. 4t + 3 as a tree, then the threads ----
// writes mean and var (and the moving statistics, in place)
__global__ __launch_bounds__(kBnThreads) void bn_stats_final_kernel(BnGeom g, const float* __restrict__ part, float* __restrict__ mean_out,
                                                                    float* __restrict__ var_out, float* moving_mean, float* moving_var,
                                                                    float decay) {
  __shared__ float sh_n[kBnThreads];
  __shared__ Stat4 sh_mean[kBnThreads], sh_m2[kBnThreads];
  const int tid = threadIdx.x;
  const long long ch = (long long)blockIdx.x * 4;
  float n[4], mean[4][4], m2[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int s = tid * 4 + j;
    n[j] = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { mean[j][e] = 0.f; m2[j][e] = 0.f; }
    if (s < g.slices) {
      n[j] = (float)slice_count(g, s);
      load4(part + (long long)s * 2 * g.c + ch, mean[j]);
      load4(part + (long long)s * 2 * g.c + g.c + ch, m2[j]);
    }
  }
  chan_merge(n[0], mean[0], m2[0], n[1], mean[1], m2[1]);
  chan_merge(n[2], mean[2], m2[2], n[3], mean[3], m2[3]);
  chan_merge(n[0], mean[0], m2[0], n[2], mean[2], m2[2]);
  sh_n[tid] = n[0];
#pragma unroll
  for (int e = 0; e < 4; ++e) { sh_mean[tid].v[e] = mean[0][e]; sh_m2[tid].v[e] = m2[0][e]; }
  __syncthreads();
  for (int off = kBnThreads / 2; off >= 1; off >>= 1) {
    if (tid < off) {
      chan_merge(n[0], mean[0], m2[0], sh_n[tid + off], sh_mean[tid + off].v, sh_m2[tid + off].v);
      sh_n[tid] = n[0];
#pragma unroll
      for (int e = 0; e < 4; ++e) { sh_mean[tid].v[e] = mean[0][e]; sh_m2[tid].v[e] = m2[0][e]; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float rows = (float)g.rows, bessel = g.rows > 1 ? (float)(g.rows - 1) : 1.f;
    float var[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) var[e] = m2[0][e] / rows;
    store4(mean_out + ch, mean[0]);
    store4(var_out + ch, var);
    if (moving_mean != nullptr) {
      const float keep = decay, take = 1.f - decay;
      float mm[4], mv[4];
      load4(moving_mean + ch, mm);
      load4(moving_var + ch, mv);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        mm[e] = keep * mm[e] + take * mean[0][e];
        mv[e] = keep * mv[e] + take * (m2[0][e] / bessel);
      }
      store4(moving_mean + ch, mm);
      store4(moving_var + ch, mv);
    }
  }
}

// the chain keeps mean and var in its workspace and delivers them too: [c] floats each, 4 per lane
__global__ __launch_bounds__(kBnThreads) void bn_copy_stats_kernel(int groups, const float* __restrict__ mean, const float* __restrict__ var,
                                                                   float* mean_out, float* var_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= groups) return;
  float v[4];
  if (mean_out != nullptr) { load4(mean + 4 * i, v); store4(mean_out + 4 * i, v); }
  if (var_out != nullptr) { load4(var + 4 * i, v); store4(var_out + 4 * i, v); }
}

// ---- forward, pass 3: y = round(act(gamma (xs - mean) rstd + beta)) -------------------------------------------------------------------
template <bool BF16, bool RELU, class PL>
__global__ __launch_bounds__(kBnThreads) void bn_apply_kernel(BnGeom g, PL x, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float* __restrict__ mean,
                                                              const float* __restrict__ var, float eps, PL y) {
  const int tid = threadIdx.x, gl = tid & (g.lpr - 1), rl = tid >> g.lpr_log2;
  const int cgi = blockIdx.y * g.lpr + gl;
  const long long cnt = slice_count(g, blockIdx.x);
  if (cgi >= g.cg || rl >= cnt) return;
  const long long ch = (long long)cgi * 4;
  float ga[4], be[4], mu[4], rstd[4];
  load4(gamma + ch, ga);
  load4(beta + ch, be);
  load4(mean + ch, mu);
  load4(var + ch, rstd);
#pragma unroll
  for (int e = 0; e < 4; ++e) rstd[e] = 1.f / sqrtf(rstd[e] + eps);
  const long long row0 = (long long)blockIdx.x * g.slice_rows + rl;
  const int mine = (int)((cnt - rl + g.rpb - 1) / g.rpb);
#pragma unroll 4
  for (int i = 0; i < mine; ++i) {
    const long long row = row0 + (long long)i * g.rpb;
    float v[4], o[4];
    place_load<BF16>(x, g, row, ch, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xhat = (round_storage<BF16>(v[e]) - mu[e]) * rstd[e];
      float t = ga[e] * xhat + be[e];
      if (RELU) t = t > 0.f ? t : (t == t ? 0.f : t);          // NaN stays NaN
      o[e] = round_storage<BF16>(t);
    }
    place_store<BF16>(y, g, row, ch, o);
  }
}

// ---- backward, pass 1: per slice sum(dz) and sum(dz xhat) -> part [slices][2][c] -------------------------------------------------------
template <bool BF16, bool RELU, class PL>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_sums_kernel(BnGeom g, PL x, PL y, PL dy, const float* __restrict__ mean,
                                                                 const float* __restrict__ var, float eps, float* __restrict__ part) {
  __shared__ Stat4 sh_b[kBnThreads], sh_g[kBnThreads];
  const int tid = threadIdx.x, gl = tid & (g.lpr - 1), rl = tid >> g.lpr_log2;
  const int cgi = blockIdx.y * g.lpr + gl;
  const bool active = cgi < g.cg;
  const long long cnt = slice_count(g, blockIdx.x);
  float sb[4] = {0.f, 0.f, 0.f, 0.f}, sg[4] = {0.f, 0.f, 0.f, 0.f};
  if (active && rl < cnt) {
    const long long ch = (long long)cgi * 4;
    float mu[4], rstd[4];
    load4(mean + ch, mu);
    load4(var + ch, rstd);
#pragma unroll
    for (int e = 0; e < 4; ++e) rstd[e] = 1.f / sqrtf(rstd[e] + eps);
    const long long row0 = (long long)blockIdx.x * g.slice_rows + rl;
    const int mine = (int)((cnt - rl + g.rpb - 1) / g.rpb);
#pragma unroll 4
    for (int i = 0; i < mine; ++i) {
      const long long row = row0 + (long long)i * g.rpb;
      float v[4], d[4], m[4] = {1.f, 1.f, 1.f, 1.f};
      place_load<BF16>(x, g, row, ch, v);
      place_load<BF16>(dy, g, row, ch, d);
      if (RELU) place_load<BF16>(y, g, row, ch, m);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dz = round_storage<BF16>(RELU ? (m[e] > 0.f ? d[e] : 0.f) : d[e]);
        const float xhat = (round_storage<BF16>(v[e]) - mu[e]) * rstd[e];
        sb[e] += dz;
        sg[e] += dz * xhat;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) { sh_b[tid].v[e] = sb[e]; sh_g[tid].v[e] = sg[e]; }
  __syncthreads();
  for (int off = kBnThreads / 2; off >= g.lpr; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sb[e] += sh_b[tid + off].v[e];
        sg[e] += sh_g[tid + off].v[e];
        sh_b[tid].v[e] = sb[e];
        sh_g[tid].v[e] = sg[e];
      }
    }
    __syncthreads();
  }
  if (rl == 0 && active) {
    float* o = part + (long long)blockIdx.x * 2 * g.c + (long long)cgi * 4;
    store4(o, sb);
    store4(o + g.c, sg);
  }
}

// ---- backward, pass 2: the slices' sums behind the tree of bn_stats_final_kernel -> fin [2][c] (what pass 3 reads), dbeta, dgamma -----
__global__ __launch_bounds__(kBnThreads) void bn_bwd_final_kernel(BnGeom g, const float* __restrict__ part, float* __restrict__ fin,
                                                                  float* dbeta, float* dgamma) {
  __shared__ Stat4 sh_b[kBnThreads], sh_g[kBnThreads];
  const int tid = threadIdx.x;
  const long long ch = (long long)blockIdx.x * 4;
  float b[4][4], q[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int s = tid * 4 + j;
#pragma unroll
    for (int e = 0; e < 4; ++e) { b[j][e] = 0.f; q[j][e] = 0.f; }
    if (s < g.slices) {
      load4(part + (long long)s * 2 * g.c + ch, b[j]);
      load4(part + (long long)s * 2 * g.c + g.c + ch, q[j]);
    }
  }
  float sb[4], sg[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sb[e] = (b[0][e] + b[1][e]) + (b[2][e] + b[3][e]);
    sg[e] = (q[0][e] + q[1][e]) + (q[2][e] + q[3][e]);
    sh_b[tid].v[e] = sb[e];
    sh_g[tid].v[e] = sg[e];
  }
  __syncthreads();
  for (int off = kBnThreads / 2; off >= 1; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sb[e] += sh_b[tid + off].v[e];
        sg[e] += sh_g[tid + off].v[e];
        sh_b[tid].v[e] = sb[e];
        sh_g[tid].v[e] = sg[e];
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    store4(fin + ch, sb);
    store4(fin + g.c + ch, sg);
    if (dbeta != nullptr) store4(dbeta + ch, sb);
    if (dgamma != nullptr) store4(dgamma + ch, sg);
  }
}

// ---- backward, pass 3: dx = round(gamma rstd (dz - dbeta / M - xhat dgamma / M)) -------------------------------------------------------
template <bool BF16, bool RELU, class PL>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_dx_kernel(BnGeom g, PL x, PL y, PL dy, const float* __restrict__ gamma,
                                                               const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                                               const float* __restrict__ fin, PL dx) {
  const int tid = threadIdx.x, gl = tid & (g.lpr - 1), rl = tid >> g.lpr_log2;
  const int cgi = blockIdx.y * g.lpr + gl;
  const long long cnt = slice_count(g, blockIdx.x);
  if (cgi >= g.cg || rl >= cnt) return;
  const long long ch = (long long)cgi * 4;
  float scale[4], mu[4], rstd[4], mb[4], mg[4];
  load4(gamma + ch, scale);
  load4(mean + ch, mu);
  load4(var + ch, rstd);
  load4(fin + ch, mb);
  load4(fin + g.c + ch, mg);
  const float rows = (float)g.rows;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    rstd[e] = 1.f / sqrtf(rstd[e] + eps);
    scale[e] = scale[e] * rstd[e];
    mb[e] = mb[e] / rows;
    mg[e] = mg[e] / rows;
  }
  const long long row0 = (long long)blockIdx.x * g.slice_rows + rl;
  const int mine = (int)((cnt - rl + g.rpb - 1) / g.rpb);
#pragma unroll 4
  for (int i = 0; i < mine; ++i) {
    const long long row = row0 + (long long)i * g.rpb;
    float v[4], d[4], m[4] = {1.f, 1.f, 1.f, 1.f}, o[4];
    place_load<BF16>(x, g, row, ch, v);
    place_load<BF16>(dy, g, row, ch, d);
    if (RELU) place_load<BF16>(y, g, row, ch, m);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float dz = round_storage<BF16>(RELU ? (m[e] > 0.f ? d[e] : 0.f) : d[e]);
      const float xhat = (round_storage<BF16>(v[e]) - mu[e]) * rstd[e];
      o[e] = round_storage<BF16>(scale[e] * ((dz - mb[e]) - xhat * mg[e]));
    }
    place_store<BF16>(dx, g, row, ch, o);
  }
}

int pow2_ceil_log2(int64_t v) {
  int l = 0;
  while (((int64_t)1 << l) < v) ++l;
  return l;
}

// descriptor checks + the geometry + the workspace layout; `what` starts every message
int plan_bn(const char* what, const ron_bn_desc* d, BnPlan* P) {
  RON_REQUIRE(d != nullptr, "%s: NULL descriptor", what);
  RON_REQUIRE(d->dtype == RON_DTYPE_BF16 || d->dtype == RON_DTYPE_F16, "%s: dtype %d: bf16 or fp16 only", what, d->dtype);
  RON_REQUIRE(d->n >= 1 && d->h >= 1 && d->w >= 1, "%s: empty tensor (n %d, h %d, w %d)", what, d->n, d->h, d->w);
  RON_REQUIRE(d->c >= 8 && d->c % 8 == 0, "%s: c %d must be a multiple of 8", what, d->c);
  RON_REQUIRE(d->relu == 0 || d->relu == 1, "%s: relu %d must be 0 or 1", what, d->relu);
  RON_REQUIRE(std::isfinite(d->eps) && d->eps >= 0.f, "%s: eps %g must be finite and >= 0", what, (double)d->eps);
  RON_REQUIRE(d->decay >= 0.f && d->decay <= 1.f, "%s: decay %g must lie in [0, 1]", what, (double)d->decay);
  const int64_t rows = (int64_t)d->n * d->h * d->w;
  RON_REQUIRE(rows <= kBnMaxRows, "%s: n h w = %lld rows, at most 2^24 (the count must be exact in fp32)", what, (long long)rows);
  P->rows = rows;
  P->c = d->c;
  P->cg = d->c / 4;
  P->lpr_log2 = std::min(6, pow2_ceil_log2(P->cg));
  P->lpr = 1 << P->lpr_log2;
  P->rpb = kBnThreads / P->lpr;
  P->tiles = (P->cg + P->lpr - 1) / P->lpr;
  RON_REQUIRE(P->tiles <= 65535, "%s: c %d is beyond the grid", what, d->c);
  const int64_t per = (rows + kBnMaxSlices - 1) / kBnMaxSlices;
  P->slice_rows = std::max<int64_t>((int64_t)P->rpb * 4, (int64_t)1 << pow2_ceil_log2(per));
  P->slices = (int)((rows + P->slice_rows - 1) / P->slice_rows);
  P->off_part = 0;
  P->off_fin = align_up((int64_t)P->slices * 2 * d->c * 4, 256);
  P->total = P->off_fin + align_up((int64_t)2 * d->c * 4, 256);
  return RON_OK;
}


template <bool BF16, bool RELU, class PL>
int run_forward(const ron_bn_desc* d, const BnPlan& P, PL x, const float* gamma, const float* beta, PL y, float* mean, float* var,
                float* moving_mean, float* moving_var, char* ws, hipStream_t s) {
  // (the kernels are spelled as the operators' launch trace has them since before the place: PL is deduced from the arguments)
  const BnGeom& g = P;
  float* part = reinterpret_cast<float*>(ws + P.off_part);
  const dim3 grid(P.slices, P.tiles);
  RON_LAUNCH(bn_stats_kernel<BF16>, grid, dim3(kBnThreads), 0, s, g, x, part);
  RON_LAUNCH(bn_stats_final_kernel, dim3(P.cg), dim3(kBnThreads), 0, s, g, part, mean, var, moving_mean, moving_var, d->decay);
  RON_LAUNCH((bn_apply_kernel<BF16, RELU>), grid, dim3(kBnThreads), 0, s, g, x, gamma, beta, mean, var, d->eps, y);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

template <bool BF16, bool RELU, class PL>
int run_backward(const ron_bn_desc* d, const BnPlan& P, PL x, PL y, PL dy, const float* gamma, const float* mean, const float* var,
                 bool want_dx, PL dx, float* dgamma, float* dbeta, char* ws, hipStream_t s) {
  const BnGeom& g = P;
  float* part = reinterpret_cast<float*>(ws + P.off_part);
  float* fin = reinterpret_cast<float*>(ws + P.off_fin);
  const dim3 grid(P.slices, P.tiles);
  RON_LAUNCH((bn_bwd_sums_kernel<BF16, RELU>), grid, dim3(kBnThreads), 0, s, g, x, y, dy, mean, var, d->eps, part);
  RON_LAUNCH(bn_bwd_final_kernel, dim3(P.cg), dim3(kBnThreads), 0, s, g, part, fin, dbeta, dgamma);
  if (want_dx) RON_LAUNCH((bn_bwd_dx_kernel<BF16, RELU>), grid, dim3(kBnThreads), 0, s, g, x, y, dy, gamma, mean, var, d->eps, fin, dx);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

// the four (storage type, activation) instantiations behind one call
template <class PL, class... A>
int forward_by_type(const ron_bn_desc* d, A... a) {
  if (d->dtype == RON_DTYPE_BF16) return d->relu ? run_forward<true, true, PL>(d, a...) : run_forward<true, false, PL>(d, a...);
  return d->relu ? run_forward<false, true, PL>(d, a...) : run_forward<false, false, PL>(d, a...);
}
template <class PL, class... A>
int backward_by_type(const ron_bn_desc* d, A... a) {
  if (d->dtype == RON_DTYPE_BF16) return d->relu ? run_backward<true, true, PL>(d, a...) : run_backward<true, false, PL>(d, a...);
  return d->relu ? run_backward<false, true, PL>(d, a...) : run_backward<false, false, PL>(d, a...);
}

DensePlace dense(const float* p) { return DensePlace{const_cast<float*>(p)}; }
HaloPlace halo(const TensorView& v) {
  HaloPlace t = HaloPlace();
  t.p = static_cast<unsigned short*>(v.base);
  t.H = v.H; t.W = v.W; t.pad = v.pad; t.cs = v.cstride; t.coff = v.coff;
  return t;
}

}  // namespace

int bn_view_plan(const char* what, const ron_bn_desc* d, int64_t* scratch_bytes) {
  BnPlan P = BnPlan();
  if (int rc = plan_bn(what, d, &P)) return rc;
  *scratch_bytes = P.total;
  return RON_OK;
}

int bn_view_forward(const ron_bn_desc* d, const TensorView& x, const TensorView& y, const float* gamma, const float* beta, float* mean,
                    float* var, float* mean_copy, float* var_copy, float* moving_mean, float* moving_var, char* scratch, hipStream_t s) {
  BnPlan P = BnPlan();
  if (int rc = plan_bn("batchnorm on views", d, &P)) return rc;
  if (int rc = forward_by_type<HaloPlace>(d, P, halo(x), gamma, beta, halo(y), mean, var, moving_mean, moving_var, scratch, s)) return rc;
  if (mean_copy != nullptr || var_copy != nullptr) {
    RON_LAUNCH(bn_copy_stats_kernel, dim3((d->c / 4 + kBnThreads - 1) / kBnThreads), dim3(kBnThreads), 0, s, d->c / 4, mean, var, mean_copy, var_copy);
    RON_HIP_CHECK(ron::launch_error());
  }
  return RON_OK;
}

int bn_view_backward(const ron_bn_desc* d, const TensorView& x, const TensorView& y, const TensorView& dy, const float* gamma,
                     const float* mean, const float* var, const TensorView* dx, float* dgamma, float* dbeta, char* scratch, hipStream_t s) {
  BnPlan P = BnPlan();
  if (int rc = plan_bn("batchnorm on views", d, &P)) return rc;
  return backward_by_type<HaloPlace>(d, P, halo(x), halo(y), halo(dy), gamma, mean, var, dx != nullptr, dx != nullptr ? halo(*dx) : HaloPlace(),
                                     dgamma, dbeta, scratch, s);
}

}  // namespace ron

extern "C" int64_t ron_batchnorm_workspace_bytes(const ron_bn_desc* d) {
  ron::BnPlan P = ron::BnPlan();
  if (ron::plan_bn("batchnorm", d, &P) != RON_OK) return -1;
  return P.total;
}

extern "C" int ron_batchnorm_train_nhwc(const ron_bn_desc* d, const float* x, const float* gamma, const float* beta, float* y, float* mean,
                                        float* var, float* moving_mean, float* moving_var, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
  using namespace ron;
  const char* what = "batchnorm forward";
  BnPlan P = BnPlan();
  if (int rc = plan_bn(what, d, &P)) return rc;
  RON_REQUIRE(x != nullptr && gamma != nullptr && beta != nullptr && y != nullptr && mean != nullptr && var != nullptr,
              "%s: x, gamma, beta, y, mean and var must not be NULL", what);
  RON_REQUIRE((moving_mean == nullptr) == (moving_var == nullptr), "%s: moving_mean and moving_var come together (both, or both NULL)", what);
  RON_REQUIRE((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y | (uintptr_t)mean | (uintptr_t)var |
                (uintptr_t)moving_mean | (uintptr_t)moving_var) & 15) == 0,
              "%s: every tensor must be 16-byte aligned (16 bytes per access)", what);
  if (int rc = check_workspace(what, "ron_batchnorm_workspace_bytes", workspace, workspace_bytes, P.total)) return rc;
  return forward_by_type<DensePlace>(d, P, dense(x), gamma, beta, dense(y), mean, var, moving_mean, moving_var,
                                     static_cast<char*>(workspace), (hipStream_t)stream);
}

extern "C" int ron_batchnorm_backward_nhwc(const ron_bn_desc* d, const float* x, const float* y, const float* dy, const float* gamma,
                                           const float* mean, const float* var, float* dx, float* dgamma, float* dbeta, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
  using namespace ron;
  const char* what = "batchnorm backward";
  BnPlan P = BnPlan();
  if (int rc = plan_bn(what, d, &P)) return rc;
  RON_REQUIRE(x != nullptr && dy != nullptr && gamma != nullptr && mean != nullptr && var != nullptr,
              "%s: x, dy, gamma, mean and var must not be NULL", what);
  RON_REQUIRE(!d->relu || y != nullptr, "%s: relu is set and y is NULL (the mask is y > 0)", what);
  RON_REQUIRE((((uintptr_t)x | (uintptr_t)(d->relu ? y : nullptr) | (uintptr_t)dy | (uintptr_t)gamma | (uintptr_t)mean | (uintptr_t)var |
                (uintptr_t)dx | (uintptr_t)dgamma | (uintptr_t)dbeta) & 15) == 0,
              "%s: every tensor must be 16-byte aligned (16 bytes per access)", what);
  if (int rc = check_workspace(what, "ron_batchnorm_workspace_bytes", workspace, workspace_bytes, P.total)) return rc;
  return backward_by_type<DensePlace>(d, P, dense(x), dense(y), dense(dy), gamma, mean, var, dx != nullptr, dense(dx), dgamma, dbeta,
                                      static_cast<char*>(workspace), (hipStream_t)stream);
}
