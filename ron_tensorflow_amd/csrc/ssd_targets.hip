// The SSD losses (ssd_vgg_300.ssd_losses, nets/ssd_vgg_300.py:580-659; ssd_vgg_512.ssd_losses, nets/ssd_vgg_512.py:516-607) and their
// gradient with respect to the head tensors: cross-entropy of the positives, cross-entropy of the hard negatives, abs_smooth
// (nets/custom_layers.py:51-63) of the positives' localisations.
//
// Hard negative mining: a row's value v is its background probability p0 when the row is a candidate (not positive, not ignored)
// and 1 otherwise; the k-th smallest v of a segment (the whole batch, or one feature layer) is the threshold t, the candidates
// strictly below t are mined.  k runs to 1e5 and a segment to 4e5 rows spread over all workgroups, so t is found by an exact radix
// select on the bit pattern of v (v >= 0: the pattern orders as an unsigned): four 8-bit digits, high to low.  Every digit is one
// launch that histograms, per segment, the keys that agree with the digits chosen so far (LDS histogram per workgroup, one integer
// atomic per non-empty bin and workgroup into a [4][segments][256] table); a workgroup re-derives the chosen digits from the finished
// tables in its prologue (a 256-wide scan per digit), so nothing goes through the host and no tiny launch sits in between.
//   rows    per row: v, the row's cross-entropy against label 0, the segment's n_pos / n_cand, the first digit's histogram
//   hist    digits 2, 3, 4 (three launches)
//   sum     t, k and n_mined (the number of keys below t: read off the tables) re-derived; the three terms per row in float32, added
//           per workgroup and segment in double; with kGrad the gradient rows, already scaled, in the same pass
//   final   one workgroup adds the partial sums in a fixed order and forms the four losses and the counts
// Counts are integer atomics (exact); no floating-point atomics; every loop's trip count is fixed by the shapes.
//
// Compiled with -ffp-contract=off, like targets.hip: the comparisons decide sets.
#include <hip/hip_runtime.h>

#include <math.h>

#include "loss_device.h"

namespace ron {
namespace {

constexpr int kHistRows = 1024;            // rows of one workgroup of a digit pass (4 per thread)
constexpr int kSegs = RON_MAX_LAYERS;      // most segments of a call
constexpr int kDigits = 4;

// workspace: counters, the digit tables (both cleared per call), the keys, the label-0 cross-entropies, the partial sums
constexpr int64_t kCountBytes = 128;       // int32 n_pos[kSegs], n_cand[kSegs]
constexpr int64_t kHistBytes = (int64_t)kDigits * kSegs * 256 * (int64_t)sizeof(unsigned);
constexpr int64_t kZeroBytes = kCountBytes + kHistBytes;

RON_KERNEL_ARGS_BEGIN
struct SsdDev {
  int num_layers, num_classes, num_segs, batch, mining;
  float match_threshold, negative_ratio, alpha;
  long long row_off[RON_MAX_LAYERS + 1];   // first flattened row of a layer (batch included)
  long long seg_off[RON_MAX_LAYERS + 1];   // first flattened row of a segment
  const float* cls[RON_MAX_LAYERS];
  const float* loc[RON_MAX_LAYERS];
  const int64_t* gclasses[RON_MAX_LAYERS];
  const float* gloc[RON_MAX_LAYERS];
  const float* gscores[RON_MAX_LAYERS];
};
RON_KERNEL_ARGS_END(SsdDev)

RON_KERNEL_ARGS_BEGIN
struct SsdGradDev {
  float* d_cls[RON_MAX_LAYERS];
  float* d_loc[RON_MAX_LAYERS];
};
RON_KERNEL_ARGS_END(SsdGradDev)

__device__ inline int segment_of(const SsdDev& p, long long r) {
  int s = 0;
  while (s + 1 < p.num_segs && r >= p.seg_off[s + 1]) ++s;
  return s;
}

// custom_layers.abs_smooth, one coordinate
__device__ inline float abs_smooth(float d) {
  const float a = fabsf(d);
  return 0.5f * ((a - 1.f) * fminf(a, 1.f) + a);
}

// the number of rows whose k-th smallest value is the threshold: nets/ssd_vgg_300.py:630-632 (BATCH), nets/ssd_vgg_512.py:563-567
// (LAYER); the cast truncates like tf.cast; clamped to [0, R] (TF's top_k raises beyond R, val[-1] raises at 0)
__device__ inline int segment_k(const SsdDev& p, int n_pos, int n_cand, int s) {
  const long long R = p.seg_off[s + 1] - p.seg_off[s];
  const float f = p.negative_ratio * (float)n_pos;
  long long k = (long long)(int)fminf(fmaxf(f, -1.0e9f), 1.0e9f);
  if (p.mining == RON_SSD_MINING_BATCH) {
    k += p.batch;
    if (k > n_cand) k = n_cand;
  } else {
    if (k < R / 8) k = R / 8;
    if (k < 4ll * p.batch) k = 4ll * p.batch;
    if (k > 1ll + n_cand) k = 1ll + n_cand;
  }
  if (k > R) k = R;
  if (k < 0) k = 0;
  return (int)k;
}

struct SelectLds {
  unsigned prefix[kSegs];                  // the digits chosen so far, in place: after four digits the bit pattern of t
  int k[kSegs];                            // the segment's k
  int kres[kSegs];                         // rank of t among the keys that share the prefix
  int less[kSegs];                         // keys below the prefix: after four digits the number of mined rows
  int wave_total[kThreads / 64];
};

// Re-derives, for the segments s_lo .. s_hi, the first `digits` digits of t from the finished tables.  The whole workgroup calls
// it; L is valid for every thread on return.
__device__ inline void derive_select(const SsdDev& p, const int32_t* __restrict__ cnt, const unsigned* __restrict__ hist, int digits,
                                     int s_lo, int s_hi, SelectLds& L) {
  const int t = threadIdx.x;
  for (int s = s_lo; s <= s_hi; ++s) {
    if (t == 0) {
      const int k = segment_k(p, cnt[s], cnt[kSegs + s], s);
      L.k[s] = k;
      L.kres[s] = k;
      L.prefix[s] = 0u;
      L.less[s] = 0;
    }
    __syncthreads();
    for (int d = 0; d < digits; ++d) {
      const int c = (int)hist[((size_t)d * kSegs + s) * 256 + t];
      int incl = c;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if ((t & 63) >= off) incl += o;
      }
      if ((t & 63) == 63) L.wave_total[t >> 6] = incl;
      __syncthreads();
      for (int w = 0; w < (t >> 6); ++w) incl += L.wave_total[w];
      const int kres = L.kres[s];
      __syncthreads();                                                   // kres and the wave totals are read
      if (kres > 0 && incl - c < kres && kres <= incl) {                 // one bin holds the kres-th key
        L.prefix[s] |= (unsigned)t << (24 - 8 * d);
        L.kres[s] = kres - (incl - c);
        L.less[s] += incl - c;
      }
      __syncthreads();
    }
  }
}

// a workgroup's LDS histograms of the segments s_lo .. s_hi into one table of the workspace
__device__ inline void flush_histograms(unsigned (*h)[256], unsigned* __restrict__ table, int s_lo, int s_hi) {
  for (int s = s_lo; s <= s_hi; ++s) {
    const unsigned c = h[s][threadIdx.x];
    if (c) atomicAdd(&table[(size_t)s * 256 + threadIdx.x], c);
  }
}

// Thread per row: the row's sets, v and the cross-entropy against label 0; n_pos / n_cand and the first digit's histogram.
__global__ __launch_bounds__(kThreads) void ssd_rows_kernel(SsdDev p, int32_t* __restrict__ cnt, unsigned* __restrict__ hist,
                                                            unsigned* __restrict__ keys, float* __restrict__ ce0,
                                                            float* __restrict__ nvalues) {
  __shared__ unsigned h[kSegs][256];
  __shared__ int c[2][kSegs];
  const int t = threadIdx.x;
  for (int s = 0; s < kSegs; ++s) h[s][t] = 0u;
  if (t < 2 * kSegs) (&c[0][0])[t] = 0;
  __syncthreads();
  const long long total = p.row_off[p.num_layers];
  const long long first = (long long)blockIdx.x * kThreads;
  const long long last = first + kThreads - 1 < total - 1 ? first + kThreads - 1 : total - 1;
  const int s_lo = segment_of(p, first), s_hi = segment_of(p, last);
  const long long r = first + t;
  if (r < total) {
    int l; long long j;
    locate_row(p, r, &l, &j);
    const int seg = p.mining == RON_SSD_MINING_BATCH ? 0 : l;
    const float score = p.gscores[l][j];
    const bool pos = score > p.match_threshold;
    const bool cand = !pos && score > -0.5f;
    float v = 1.f, e0 = 0.f;
    if (cand) {
      const float* x = p.cls[l] + j * p.num_classes;
      float mx = x[0];
      for (int i = 1; i < p.num_classes; ++i) mx = fmaxf(mx, x[i]);
      float sum = 0.f;
      for (int i = 0; i < p.num_classes; ++i) sum += expf(x[i] - mx);
      v = expf(x[0] - mx) / sum;
      e0 = (logf(sum) + mx) - x[0];
    }
    const unsigned key = __float_as_uint(v);
    keys[r] = key;
    ce0[r] = e0;
    if (nvalues != nullptr) nvalues[r] = v;
    atomicAdd(&h[seg][key >> 24], 1u);
    if (pos) atomicAdd(&c[0][seg], 1);
    if (cand) atomicAdd(&c[1][seg], 1);
  }
  __syncthreads();
  flush_histograms(h, hist, s_lo, s_hi);
  if (t < 2)
    for (int s = s_lo; s <= s_hi; ++s)
      if (c[t][s]) atomicAdd(&cnt[t * kSegs + s], c[t][s]);
}

// Digit `digit` (1 .. 3): the keys that share the digits chosen so far, by their next eight bits.
__global__ __launch_bounds__(kThreads) void ssd_hist_kernel(SsdDev p, const int32_t* __restrict__ cnt, unsigned* __restrict__ hist,
                                                            const unsigned* __restrict__ keys, int digit) {
  __shared__ unsigned h[kSegs][256];
  __shared__ SelectLds L;
  const int t = threadIdx.x;
  for (int s = 0; s < kSegs; ++s) h[s][t] = 0u;
  const long long total = p.row_off[p.num_layers];
  const long long first = (long long)blockIdx.x * kHistRows;
  const long long last = first + kHistRows - 1 < total - 1 ? first + kHistRows - 1 : total - 1;
  const int s_lo = segment_of(p, first), s_hi = segment_of(p, last);
  derive_select(p, cnt, hist, digit, s_lo, s_hi, L);                     // synchronises: h[] is cleared
  const int shift = 32 - 8 * digit;
  for (int i = 0; i < kHistRows / kThreads; ++i) {
    const long long r = first + i * kThreads + t;
    if (r < total) {
      const int seg = segment_of(p, r);
      const unsigned key = keys[r];
      if (L.k[seg] > 0 && (key >> shift) == (L.prefix[seg] >> shift)) atomicAdd(&h[seg][(key >> (shift - 8)) & 255u], 1u);
    }
  }
  __syncthreads();
  flush_histograms(h, hist + (size_t)digit * kSegs * 256, s_lo, s_hi);
}

// the per-segment divisors of the three terms (0 where the term is 0)
struct Scales { float pos, neg, loc; };
__device__ inline Scales segment_scales(const SsdDev& p, int n_pos, int n_mined) {
  Scales s;
  if (p.mining == RON_SSD_MINING_BATCH) {
    s.pos = s.neg = 1.f / (float)p.batch;
    s.loc = p.alpha / (float)p.batch;
  } else {
    s.pos = n_pos > 0 ? 1.f / (float)n_pos : 0.f;
    s.neg = n_mined > 0 ? 1.f / (float)n_mined : 0.f;
    s.loc = (n_pos > 0 && p.alpha != 0.f) ? p.alpha / (float)(4ll * n_pos) : 0.f;
  }
  return s;
}

// One workgroup owns the 256 rows it owned in ssd_rows_kernel.  A thread forms its row's three terms; they are added per segment in
// double and stored as the workgroup's partial sums.  With kGrad the thread also writes the row's localisation gradient (16 bytes
// per lane), and the rows of the positive and the mined set go through LDS (class_grad_pass), each with its segment's scale.
template <bool kGrad>
__global__ __launch_bounds__(kThreads) void ssd_sum_kernel(SsdDev p, SsdGradDev q, const int32_t* __restrict__ cnt,
                                                           const unsigned* __restrict__ hist, const unsigned* __restrict__ keys,
                                                           const float* __restrict__ ce0, double* __restrict__ partials) {
  __shared__ SelectLds L;
  __shared__ double red[3][kThreads];
  __shared__ float seg_pos[kSegs], seg_neg[kSegs], seg_loc[kSegs];
  const int t = threadIdx.x;
  const int C = p.num_classes;
  const long long total = p.row_off[p.num_layers];
  const long long first = (long long)blockIdx.x * kThreads;
  const long long last = first + kThreads - 1 < total - 1 ? first + kThreads - 1 : total - 1;
  const int s_lo = segment_of(p, first), s_hi = segment_of(p, last);
  derive_select(p, cnt, hist, kDigits, s_lo, s_hi, L);
  if (kGrad && t >= s_lo && t <= s_hi) {
    const Scales sc = segment_scales(p, cnt[t], L.less[t]);
    seg_pos[t] = sc.pos; seg_neg[t] = sc.neg; seg_loc[t] = sc.loc;
  }
  __syncthreads();
  const long long r = first + t;
  int seg = -1, lab = -1;
  double v_pos = 0.0, v_neg = 0.0, v_loc = 0.0;
  const float* src = nullptr;
  float* dst = nullptr;
  float scale = 0.f;
  if (r < total) {
    int l; long long j;
    locate_row(p, r, &l, &j);
    seg = p.mining == RON_SSD_MINING_BATCH ? 0 : l;
    const float score = p.gscores[l][j];
    const bool pos = score > p.match_threshold;
    const bool cand = !pos && score > -0.5f;
    const bool mined = cand && L.k[seg] > 0 && keys[r] < L.prefix[seg];
    src = p.cls[l] + j * C;
    float4 gl = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pos) {
      const long long g = p.gclasses[l][j];
      lab = clip_label(g, C);
      v_pos = (double)cross_entropy(src, C, lab);
      const float4 a = *(reinterpret_cast<const float4*>(p.loc[l]) + j);
      const float4 b = *(reinterpret_cast<const float4*>(p.gloc[l]) + j);
      const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z, dw = a.w - b.w;
      v_loc = (double)(((abs_smooth(dx) + abs_smooth(dy)) + abs_smooth(dz)) + abs_smooth(dw));
      if (kGrad) {
        const float s = seg_loc[seg];
        gl = make_float4(fminf(fmaxf(dx, -1.f), 1.f) * s, fminf(fmaxf(dy, -1.f), 1.f) * s, fminf(fmaxf(dz, -1.f), 1.f) * s,
                         fminf(fmaxf(dw, -1.f), 1.f) * s);
        scale = seg_pos[seg];
      }
    } else if (mined) {
      lab = 0;
      v_neg = (double)ce0[r];
      if (kGrad) scale = seg_neg[seg];
    }
    if (kGrad) {
      dst = q.d_cls[l] + j * C;
      *(reinterpret_cast<float4*>(q.d_loc[l]) + j) = gl;
    }
  }
  // the three terms, per segment, in double: a tree over the workgroup, the same order in every call
  for (int s = s_lo; s <= s_hi; ++s) {
    red[0][t] = seg == s ? v_pos : 0.0;
    red[1][t] = seg == s ? v_neg : 0.0;
    red[2][t] = seg == s ? v_loc : 0.0;
    __syncthreads();
    reduce3(red);
    if (t < 3) partials[((size_t)blockIdx.x * p.num_segs + s) * 3 + t] = red[t][0];
    __syncthreads();
  }
  if (!kGrad) return;

  __shared__ ClassGradLds lds;                     // (row_lab: clipped label of a positive row, 0 of a mined row, -1 outside both)
  __shared__ float row_scale[kThreads];
  row_scale[t] = scale;
  class_grad_pass(lds, C, src, dst, lab, [](int row) { return row_scale[row]; });
}

// One workgroup: per segment the partial sums of its workgroups in a fixed order, then the four losses and the counts.
__global__ __launch_bounds__(kThreads) void ssd_final_kernel(SsdDev p, const int32_t* __restrict__ cnt, const unsigned* __restrict__ hist,
                                                             const double* __restrict__ partials, float* __restrict__ losses,
                                                             int32_t* __restrict__ counts) {
  __shared__ SelectLds L;
  __shared__ double red[3][kThreads];
  __shared__ double seg_sum[kSegs][3];
  const int t = threadIdx.x;
  derive_select(p, cnt, hist, kDigits, 0, p.num_segs - 1, L);
  for (int s = 0; s < p.num_segs; ++s) {
    const long long w_lo = p.seg_off[s] / kThreads, w_hi = (p.seg_off[s + 1] - 1) / kThreads;
    double acc[3] = {0.0, 0.0, 0.0};
    for (long long w = w_lo + t; w <= w_hi; w += kThreads)
      for (int k = 0; k < 3; ++k) acc[k] += partials[((size_t)w * p.num_segs + s) * 3 + k];
    for (int k = 0; k < 3; ++k) red[k][t] = acc[k];
    __syncthreads();
    reduce3(red);
    if (t < 3) seg_sum[s][t] = red[t][0];
    __syncthreads();
  }
  if (t != 0) return;
  float l_pos = 0.f, l_neg = 0.f, l_loc = 0.f;
  for (int s = 0; s < p.num_segs; ++s) {
    const int n_pos = cnt[s], n_cand = cnt[kSegs + s], n_mined = L.less[s];
    const float s_pos = (float)seg_sum[s][0], s_neg = (float)seg_sum[s][1], s_loc = (float)seg_sum[s][2];
    float a, b, c;
    if (p.mining == RON_SSD_MINING_BATCH) {                               // tf.div(tf.reduce_sum(...), batch_size)
      a = s_pos / (float)p.batch;
      b = s_neg / (float)p.batch;
      c = p.alpha * (s_loc / (float)p.batch);
    } else {                                                              // compute_weighted_loss: the sum by the non-zero weights
      a = n_pos > 0 ? s_pos / (float)n_pos : 0.f;
      b = n_mined > 0 ? s_neg / (float)n_mined : 0.f;
      c = (n_pos > 0 && p.alpha != 0.f) ? p.alpha * (s_loc / (float)(4ll * n_pos)) : 0.f;
    }
    l_pos = s == 0 ? a : l_pos + a;                                       // tf.add_n: the layers in order
    l_neg = s == 0 ? b : l_neg + b;
    l_loc = s == 0 ? c : l_loc + c;
    counts[4 * s + 0] = n_pos;
    counts[4 * s + 1] = n_cand;
    counts[4 * s + 2] = L.k[s];
    counts[4 * s + 3] = n_mined;
  }
  losses[0] = l_pos;
  losses[1] = l_neg;
  losses[2] = l_loc;
  losses[3] = (l_pos + l_neg) + l_loc;
}

struct Layout {
  int64_t rows, wgs, keys, ce0, partials, bytes;
};

Layout workspace_layout(const ron_heads* heads, int n) {
  Layout w;
  w.rows = count_rows(heads, n);
  w.wgs = (w.rows + kThreads - 1) / kThreads;
  w.keys = kZeroBytes;
  w.ce0 = w.keys + align_up(w.rows * 4, 16);
  w.partials = w.ce0 + align_up(w.rows * 4, 16);
  w.bytes = w.partials + w.wgs * heads->num_layers * 3 * (int64_t)sizeof(double);      // one segment per layer at the most
  return w;
}

int64_t workspace_bytes(const char* what, const ron_heads* heads, int n) {
  if (check_layers(heads, what) != RON_OK) return -1;
  if (n <= 0) {
    set_error("%s: bad batch %d", what, n);
    return -1;
  }
  return workspace_layout(heads, n).bytes;
}

// what ron_ssd_losses and ron_ssd_losses_grad share: the arguments checked (before any HIP call), the parameter block filled
int setup(const char* what, const ron_heads* heads, const ron_targets* targets, int n, const ron_ssd_loss_cfg* cfg, void* workspace,
          int64_t workspace_bytes, float* losses, int32_t* counts, SsdDev* out, Layout* layout) {
  if (int rc = check_layers(heads, what)) return rc;
  RON_REQUIRE(n > 0, "%s: bad batch %d", what, n);
  RON_REQUIRE(targets != nullptr && cfg != nullptr && losses != nullptr && counts != nullptr, "%s: null argument", what);
  RON_REQUIRE(cfg->mining == RON_SSD_MINING_BATCH || cfg->mining == RON_SSD_MINING_LAYER, "%s: unknown mining mode %d", what,
              cfg->mining);
  RON_REQUIRE(heads->num_classes >= 2 && heads->num_classes <= RON_MAX_CLASSES, "%s: %d classes not in [2, %d]", what,
              heads->num_classes, RON_MAX_CLASSES);
  SsdDev p = {};
  p.num_layers = heads->num_layers;
  p.num_classes = heads->num_classes;
  p.batch = n;
  p.mining = cfg->mining;
  p.match_threshold = cfg->match_threshold;
  p.negative_ratio = cfg->negative_ratio;
  p.alpha = cfg->alpha;
  int64_t rows = 0;
  for (int l = 0; l < p.num_layers; ++l) {
    RON_REQUIRE(heads->cls[l] && heads->loc[l], "%s: null head pointer of layer %d", what, l);
    RON_REQUIRE(targets->gclasses[l] && targets->glocalisations[l] && targets->gscores[l], "%s: null target pointer of layer %d", what, l);
    // a localisation row moves as one 16-byte access
    RON_REQUIRE((((uintptr_t)heads->loc[l] | (uintptr_t)targets->glocalisations[l]) & 15) == 0,
                "%s: loc / glocalisations of layer %d must be 16-byte aligned", what, l);
    p.row_off[l] = rows;
    rows += (int64_t)n * heads->feat_h[l] * heads->feat_w[l] * heads->num_anchors[l];
    p.cls[l] = heads->cls[l]; p.loc[l] = heads->loc[l];
    p.gclasses[l] = targets->gclasses[l]; p.gloc[l] = targets->glocalisations[l]; p.gscores[l] = targets->gscores[l];
  }
  p.row_off[p.num_layers] = rows;
  RON_REQUIRE(rows < (1ll << 30), "%s: too many rows", what);
  if (p.mining == RON_SSD_MINING_BATCH) {
    p.num_segs = 1;
    p.seg_off[0] = 0;
    p.seg_off[1] = rows;
  } else {
    p.num_segs = p.num_layers;
    for (int l = 0; l <= p.num_layers; ++l) p.seg_off[l] = p.row_off[l];
  }
  const Layout w = workspace_layout(heads, n);
  RON_REQUIRE(workspace != nullptr && workspace_bytes >= w.bytes, "%s: workspace of %lld bytes, %lld needed", what,
              (long long)workspace_bytes, (long long)w.bytes);
  RON_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", what);
  *out = p;
  *layout = w;
  return RON_OK;
}

template <bool kGrad>
int run(const SsdDev& p, const SsdGradDev& q, const Layout& w, void* workspace, float* losses, int32_t* counts, float* nvalues,
        hipStream_t s) {
  char* base = (char*)workspace;
  int32_t* cnt = (int32_t*)base;
  unsigned* hist = (unsigned*)(base + kCountBytes);
  unsigned* keys = (unsigned*)(base + w.keys);
  float* ce0 = (float*)(base + w.ce0);
  double* partials = (double*)(base + w.partials);
  const dim3 rows_grid((unsigned)w.wgs), hist_grid((unsigned)((w.rows + kHistRows - 1) / kHistRows));
  RON_HIP_CHECK(dev_memset_async(workspace, 0, (size_t)kZeroBytes, s));
  RON_LAUNCH(ssd_rows_kernel, rows_grid, dim3(kThreads), 0, s, p, cnt, hist, keys, ce0, nvalues);
  for (int digit = 1; digit < kDigits; ++digit)
    RON_LAUNCH(ssd_hist_kernel, hist_grid, dim3(kThreads), 0, s, p, (const int32_t*)cnt, hist, (const unsigned*)keys, digit);
  RON_LAUNCH(ssd_sum_kernel<kGrad>, rows_grid, dim3(kThreads), 0, s, p, q, (const int32_t*)cnt, (const unsigned*)hist,
             (const unsigned*)keys, (const float*)ce0, partials);
  RON_LAUNCH(ssd_final_kernel, dim3(1), dim3(kThreads), 0, s, p, (const int32_t*)cnt, (const unsigned*)hist, (const double*)partials,
             losses, counts);
  RON_HIP_CHECK(launch_error());
  return RON_OK;
}

}  // namespace
}  // namespace ron

extern "C" int64_t ron_ssd_losses_workspace_bytes(const ron_heads* heads, int n) {
  return ron::workspace_bytes("ron_ssd_losses_workspace_bytes", heads, n);
}

extern "C" int64_t ron_ssd_losses_grad_workspace_bytes(const ron_heads* heads, int n) {
  return ron::workspace_bytes("ron_ssd_losses_grad_workspace_bytes", heads, n);
}

extern "C" int ron_ssd_losses(const ron_heads* heads, const ron_targets* targets, int n, const ron_ssd_loss_cfg* cfg, void* workspace,
                              int64_t workspace_bytes, float* losses, int32_t* counts, float* nvalues, void* stream) {
  ron::SsdDev p;
  ron::Layout w;
  if (int rc = ron::setup("ron_ssd_losses", heads, targets, n, cfg, workspace, workspace_bytes, losses, counts, &p, &w)) return rc;
  return ron::run<false>(p, ron::SsdGradDev{}, w, workspace, losses, counts, nvalues, (hipStream_t)stream);
}

extern "C" int ron_ssd_losses_grad(const ron_heads* heads, const ron_targets* targets, int n, const ron_ssd_loss_cfg* cfg,
                                   void* workspace, int64_t workspace_bytes, float* losses, int32_t* counts, float* nvalues,
                                   const ron_head_grads* grads, void* stream) {
  ron::SsdDev p;
  ron::Layout w;
  if (int rc = ron::setup("ron_ssd_losses_grad", heads, targets, n, cfg, workspace, workspace_bytes, losses, counts, &p, &w)) return rc;
  RON_REQUIRE(grads != nullptr, "ron_ssd_losses_grad: null argument");
  ron::SsdGradDev q = {};
  for (int l = 0; l < p.num_layers; ++l) {
    RON_REQUIRE(grads->d_cls[l] && grads->d_loc[l], "ron_ssd_losses_grad: null gradient pointer of layer %d", l);
    RON_REQUIRE(((uintptr_t)grads->d_loc[l] & 15) == 0, "ron_ssd_losses_grad: d_loc of layer %d must be 16-byte aligned", l);
    q.d_cls[l] = grads->d_cls[l]; q.d_loc[l] = grads->d_loc[l];
  }
  return ron::run<true>(p, q, w, workspace, losses, counts, nvalues, (hipStream_t)stream);
}
