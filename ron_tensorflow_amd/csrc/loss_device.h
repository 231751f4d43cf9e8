// What the two loss sources (targets.hip: the RON losses; ssd_targets.hip: the SSD losses) share, on the device and on the host:
// the row's cross-entropy, the row -> (layer, local row) lookup, the clipped label, the three-term tree reduction, the pass that
// writes the class gradient through LDS, and the host's shape check and row count.  Both sources are compiled with
// -ffp-contract=off and so is everything here: one rounding per operation.
#ifndef RON_LOSS_DEVICE_H_
#define RON_LOSS_DEVICE_H_

#include <hip/hip_runtime.h>

#include <math.h>

#include "common.h"

namespace ron {

constexpr int kThreads = 256;             // lanes of every loss workgroup: one per row
constexpr int kGradTileFloats = 8192;     // LDS tile of class logits: rows x (C | 1) floats, 32 KiB

// the layer of flattened row r and the row inside the layer; P holds num_layers and row_off[]
template <typename P>
__device__ inline void locate_row(const P& p, long long r, int* layer, long long* j) {
  int l = 0;
  while (l + 1 < p.num_layers && r >= p.row_off[l + 1]) ++l;
  *layer = l;
  *j = r - p.row_off[l];
}

// a ground-truth class as a label of the C logits: clipped to [0, C]; C itself is out of range and makes the row NaN
__device__ inline int clip_label(long long g, int C) { return (int)(g < 0 ? 0 : (g > C ? C : g)); }

// sparse softmax cross-entropy of one row, log-sum-exp with the maximum subtracted
__device__ inline float cross_entropy(const float* x, int c, int label) {
  float mx = x[0];
  for (int i = 1; i < c; ++i) mx = fmaxf(mx, x[i]);
  float sum = 0.f;
  for (int i = 0; i < c; ++i) sum += expf(x[i] - mx);
  return label < c ? (logf(sum) + mx) - x[label] : __uint_as_float(0x7fc00000u);
}

// Three sums over the workgroup in double: red[k][t] holds thread t's term k (written and synchronised), red[k][0] the sum on
// return.  A tree, the same order in every call.
__device__ inline void reduce3(double (&red)[3][kThreads]) {
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off)
      for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
    __syncthreads();
  }
}

// LDS of class_grad_pass; the kernel declares it __shared__
struct ClassGradLds {
  float tile[kGradTileFloats];
  const float* row_src[kThreads];         // the row's logits (null: the row does not exist)
  float* row_dst[kThreads];
  int row_lab[kThreads];                  // clipped label of a row that has a gradient, -1 of one that has none (its row is zero)
  float row_mx[kThreads], row_sum[kThreads];
};

// The class gradient of a workgroup's 256 rows, (softmax - onehot) * scale(row).  The whole workgroup calls it, thread t with its
// own row's logits, destination and label.  The rows go through LDS: those with a label are loaded with consecutive lanes on
// consecutive floats, a thread takes its own row's maximum and sum (in index order, like cross_entropy) from LDS at an odd row
// stride, and every element of the gradient leaves with consecutive lanes on consecutive floats again.  Rows x (C | 1) floats that
// do not fit the tile are taken in several chunks of rows.  scale(row) is read after the pass's first barrier.
template <typename Scale>
__device__ __forceinline__ void class_grad_pass(ClassGradLds& s, int C, const float* src, float* dst, int lab, Scale scale) {
  const int t = threadIdx.x;
  s.row_src[t] = src;
  s.row_dst[t] = dst;
  s.row_lab[t] = lab;
  const int stride = C | 1;                                               // odd: a thread per row walks the banks without conflict
  const int chunk = kGradTileFloats / stride < kThreads ? kGradTileFloats / stride : kThreads;      // >= 63 rows (C <= 128)
  const int dq = kThreads / C, dr = kThreads - dq * C;
  for (int r0 = 0; r0 < kThreads; r0 += chunk) {
    const int nrows = kThreads - r0 < chunk ? kThreads - r0 : chunk;
    const int nelem = nrows * C;
    __syncthreads();                                                      // row_*[] written; the previous chunk's tile consumed
    for (int e = t, row = t / C, k = t - (t / C) * C; e < nelem; e += kThreads) {
      if (s.row_lab[r0 + row] >= 0) s.tile[row * stride + k] = s.row_src[r0 + row][k];
      row += dq; k += dr;
      if (k >= C) { k -= C; ++row; }
    }
    __syncthreads();
    if (t >= r0 && t < r0 + nrows && lab >= 0) {
      const float* x = s.tile + (t - r0) * stride;
      float mx = x[0];
      for (int i = 1; i < C; ++i) mx = fmaxf(mx, x[i]);
      float sum = 0.f;
      for (int i = 0; i < C; ++i) sum += expf(x[i] - mx);
      s.row_mx[t] = mx;
      s.row_sum[t] = sum;
    }
    __syncthreads();
    for (int e = t, row = t / C, k = t - (t / C) * C; e < nelem; e += kThreads) {
      float* out = s.row_dst[r0 + row];
      if (out != nullptr) {
        const int rl = s.row_lab[r0 + row];
        float v = 0.f;
        if (rl >= C) {
          v = __uint_as_float(0x7fc00000u);                               // label out of range: the forward's row is NaN
        } else if (rl >= 0) {
          const float pk = expf(s.tile[row * stride + k] - s.row_mx[r0 + row]) / s.row_sum[r0 + row];
          v = (pk - (k == rl ? 1.f : 0.f)) * scale(r0 + row);
        }
        out[k] = v;
      }
      row += dq; k += dr;
      if (k >= C) { k -= C; ++row; }
    }
  }
}

inline int check_layers(const ron_heads* h, const char* what) {
  RON_REQUIRE(h != nullptr, "%s: null argument", what);
  RON_REQUIRE(h->num_layers >= 1 && h->num_layers <= RON_MAX_LAYERS, "%s: %d layers not in [1, %d]", what, h->num_layers,
              RON_MAX_LAYERS);
  for (int l = 0; l < h->num_layers; ++l)
    RON_REQUIRE(h->feat_h[l] > 0 && h->feat_w[l] > 0 && h->num_anchors[l] > 0 && h->num_anchors[l] <= RON_MAX_ANCHORS_PER_CELL,
                "%s: bad shape of layer %d", what, l);
  return RON_OK;
}

// rows of all layers, the batch included
inline int64_t count_rows(const ron_heads* heads, int n) {
  int64_t rows = 0;
  for (int l = 0; l < heads->num_layers; ++l) rows += (int64_t)n * heads->feat_h[l] * heads->feat_w[l] * heads->num_anchors[l];
  return rows;
}

}  // namespace ron

#endif  // RON_LOSS_DEVICE_H_
