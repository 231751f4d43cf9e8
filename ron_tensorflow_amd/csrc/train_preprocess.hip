// Training preprocessing: ron_preprocess_for_train (preprocessing/ssd_vgg_preprocessing.py:297-356), the only training chain the
// reference reaches (preprocess_image(is_training=True), :454-457).  Its colour distortion is computed and discarded (:343-348), so
// the output is: convert_image_dtype (uint8 * (1/255)) -> ssd_random_expand with probability 1/2 (tf_image.py:440-467) ->
// ssd_random_sample_patch (:310-438) -> random_flip_left_right (:284-308) -> TF1 bilinear resize -> * 255 -> minus the means.
//
// Three kernels:
//   train_geometry_kernel      every random decision of one image and what it does to the boxes: one wave per image, the ground-truth
//                              boxes across its lanes (RON_MAX_GT / 64 per lane), the loops' conditions through ballots - no LDS, no
//                              barrier, wave-uniform control flow.  TensorFlow's random streams cannot be reproduced: the draws are
//                              an input, a table of RON_TRAIN_DRAWS uniform floats per image at FIXED slots (include/ron_hip.h).
//   train_channel_sums_kernel  exact 64-bit integer sums of the uint8 channels of the expanded images: the canvas fill is the image's
//                              mean colour, taken here as the correctly rounded quotient, independent of any reduction order.
//   preprocess_train_kernel    one pass over the output: bilinear taps of the flipped crop window, read straight from the uint8 image
//                              where the canvas holds it and from the fill elsewhere; the canvas is never materialised.
// -ffp-contract=off: every float operation rounds once, like the TF kernels and the numpy references of tests/train_pre_ref.py.
#include <hip/hip_runtime.h>

#include "common.h"

namespace ron {
namespace {

constexpr int kDraws = RON_TRAIN_DRAWS;
constexpr int kGeom = RON_TRAIN_GEOM;
constexpr int kWave = 64;
constexpr int kSlabs = RON_MAX_GT / kWave;        // boxes per lane
static_assert(RON_MAX_GT % kWave == 0, "the geometry kernel spreads RON_MAX_GT boxes over one wave");
static_assert(RON_TRAIN_DRAWS == 5 + 10 * 10 * 12, "draw slots: 5 + outer x inner x 12");

RON_KERNEL_ARGS_BEGIN
struct Means { float m[3]; };
RON_KERNEL_ARGS_END(Means)

// tf.random_uniform([1], minval=0, maxval=m, dtype=tf.int32) from a uniform float in [0, 1)
__device__ inline int int_draw(float u, int m) { return min((int)(u * (float)m), m - 1); }
// tf.random_uniform([1], minval=0.1, maxval=0.999)[0] * size (tf_image.py:320-321)
__device__ inline float size_draw(float u, float size) { return (u * (0.999f - 0.1f) + 0.1f) * size; }

__device__ inline int wave_count(bool p) { return __popcll(__ballot(p)); }

__global__ __launch_bounds__(kWave) void train_geometry_kernel(const int32_t* __restrict__ hw, const int32_t* __restrict__ glabels,
                                                               const float* __restrict__ gbboxes, int g, const float* __restrict__ draws,
                                                               int32_t* __restrict__ geom, int32_t* __restrict__ glabels_out,
                                                               float* __restrict__ gbboxes_out, int32_t* __restrict__ counts) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const float* d = draws + (long long)img * kDraws;
  const long long row0 = (long long)img * g;
  const int h0 = hw[2 * img], w0 = hw[2 * img + 1];

  // the present rows are a prefix: everything from the first label 0 on is padding and takes no part in anything below
  int lab[kSlabs];
  float b[kSlabs][4];
  int present_rows = g;
#pragma unroll
  for (int k = 0; k < kSlabs; ++k) {
    const int i = k * kWave + lane;
    lab[k] = i < g ? glabels[row0 + i] : 0;
    const unsigned long long zero = __ballot(i < g && lab[k] == 0);
    if (zero != 0 && present_rows == g) present_rows = k * kWave + __ffsll((long long)zero) - 1;
  }
  bool present[kSlabs];
#pragma unroll
  for (int k = 0; k < kSlabs; ++k) {
    const int i = k * kWave + lane;
    present[k] = i < present_rows;
#pragma unroll
    for (int j = 0; j < 4; ++j) b[k][j] = present[k] ? gbboxes[(row0 + i) * 4 + j] : 0.f;
  }

  // ssd_random_expand (tf_image.py:440-467) unless d[0] < 0.5 (ssd_vgg_preprocessing.py:326)
  const bool expanded = !(d[0] < 0.5f);
  int H = h0, W = w0, img_y = 0, img_x = 0;
  if (expanded) {
    img_x = int_draw(d[1], w0);
    img_y = int_draw(d[2], h0);
    H = 2 * h0;
    W = 2 * w0;
    const float fh = (float)h0, fw = (float)w0, fy = (float)img_y, fx = (float)img_x, ch = (float)H, cw = (float)W;
#pragma unroll
    for (int k = 0; k < kSlabs; ++k) {
      b[k][0] = (b[k][0] * fh + fy) / ch;
      b[k][1] = (b[k][1] * fw + fx) / cw;
      b[k][2] = (b[k][2] * fh + fy) / ch;
      b[k][3] = (b[k][3] * fw + fx) / cw;
    }
  }
  const float fH = (float)H, fW = (float)W;

  // ssd_random_sample_patch (tf_image.py:310-438): six logits, so min_iou 1.0 is never drawn and the patch branch always runs
  const int iou_index = min((int)(d[3] * 6.0f), 5);
  const float min_iou = iou_index == 0 ? 0.4f : iou_index == 1 ? 0.5f : iou_index == 2 ? 0.6f : iou_index == 3 ? 0.7f
                        : iou_index == 4 ? 0.8f : 0.9f;
  float cen_y[kSlabs], cen_x[kSlabs];
  bool kept[kSlabs];
#pragma unroll
  for (int k = 0; k < kSlabs; ++k) {
    cen_y[k] = (b[k][0] + b[k][2]) / 2.0f;
    cen_x[k] = (b[k][1] + b[k][3]) / 2.0f;
    kept[k] = present[k];
  }
  float roi0 = 0.f, roi1 = 0.f, roi2 = 1.f, roi3 = 1.f;
  int n_kept = present_rows;
  int outer = 0;
  for (;;) {                                                     // check_roi_overlap (:379-399)
    bool again = outer < 1;                                      // "or index < 1": the body runs at least once
    if (!again && outer < 10) {
      bool low = false;
#pragma unroll
      for (int k = 0; k < kSlabs; ++k) {                         // jaccard_with_anchors (:332-343) on the kept boxes
        const float ih = fmaxf(fminf(roi2, b[k][2]) - fmaxf(roi0, b[k][0]), 0.f);
        const float iw = fmaxf(fminf(roi3, b[k][3]) - fmaxf(roi1, b[k][1]), 0.f);
        const float inter = ih * iw;
        const float uni = (roi3 - roi1) * (roi2 - roi0) + ((b[k][2] - b[k][0]) * (b[k][3] - b[k][1]) - inter);
        low = low || (kept[k] && inter / uni < min_iou);
      }
      again = __any(low) != 0;
    }
    if (!again) break;
    int inner = 0;
    do {                                                         // check_roi_center (:345-378)
      const float* a = d + 5 + (outer * 10 + inner) * 12;        // this attempt's own twelve slots
      float sw = 0.f, sh = 0.f;
      for (int t = 0; t < 5; ++t) {                              // sample_width_height (:311-330): the fifth try is taken as it is
        sw = size_draw(a[2 * t], fW);
        sh = size_draw(a[2 * t + 1], fH);
        if (!(sw > sh * 2.0f || sh > sw * 2.0f)) break;
      }
      const int isw = (int)sw, ish = (int)sh;
      const int x = int_draw(a[10], W - isw), y = int_draw(a[11], H - ish);
      roi0 = (float)y / fH;
      roi1 = (float)x / fW;
      roi2 = (float)(y + ish) / fH;
      roi3 = (float)(x + isw) / fW;
      n_kept = 0;
#pragma unroll
      for (int k = 0; k < kSlabs; ++k) {
        kept[k] = present[k] && cen_y[k] > roi0 && cen_x[k] > roi1 && cen_y[k] < roi2 && cen_x[k] < roi3;
        n_kept += wave_count(kept[k]);
      }
      ++inner;
    } while (n_kept < 1 && inner < 10);
    ++outer;
  }

  // the crop window (:399): the products truncated, not (y, x, sh, sw); without a kept box the whole image and every box
  int crop_y = 0, crop_x = 0, crop_h = H, crop_w = W;
  if (n_kept > 0) {
    crop_y = (int)(roi0 * fH);
    crop_x = (int)(roi1 * fW);
    crop_h = (int)((roi2 - roi0) * fH);
    crop_w = (int)((roi3 - roi1) * fW);
  } else {
#pragma unroll
    for (int k = 0; k < kSlabs; ++k) kept[k] = present[k];
  }
  if (crop_h < 1 || crop_w < 1) {                                // :427: image, labels and boxes pass unchanged
    crop_y = 0; crop_x = 0; crop_h = H; crop_w = W;
#pragma unroll
    for (int k = 0; k < kSlabs; ++k) kept[k] = present[k];
  } else {
    const float oy = (float)crop_y, ox = (float)crop_x, sh = (float)crop_h, sw = (float)crop_w;
#pragma unroll
    for (int k = 0; k < kSlabs; ++k) {                           // :409-427
      b[k][0] = fmaxf(0.f, b[k][0] * fH - oy) / sh;
      b[k][1] = fmaxf(0.f, b[k][1] * fW - ox) / sw;
      b[k][2] = fminf(sh, b[k][2] * fH - oy) / sh;
      b[k][3] = fminf(sw, b[k][3] * fW - ox) / sw;
    }
  }

  // random_flip_left_right (:284-308)
  const bool flip = d[4] < 0.5f;
  if (flip) {
#pragma unroll
    for (int k = 0; k < kSlabs; ++k) {
      const float x0 = 1.0f - b[k][3], x1 = 1.0f - b[k][1];
      b[k][1] = x0;
      b[k][3] = x1;
    }
  }

  // kept rows to the front in their order, zeros behind: a row is written by exactly one lane
  int total = 0;
  int dst[kSlabs];
#pragma unroll
  for (int k = 0; k < kSlabs; ++k) {
    const unsigned long long m = __ballot(kept[k]);
    dst[k] = total + __popcll(m & ((1ull << lane) - 1ull));
    total += __popcll(m);
  }
#pragma unroll
  for (int k = 0; k < kSlabs; ++k) {
    const int i = k * kWave + lane;
    if (kept[k]) {
      glabels_out[row0 + dst[k]] = lab[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) gbboxes_out[(row0 + dst[k]) * 4 + j] = b[k][j];
    }
    if (i < g && i >= total) {
      glabels_out[row0 + i] = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) gbboxes_out[(row0 + i) * 4 + j] = 0.f;
    }
  }
  if (lane == 0) {
    int32_t* o = geom + (long long)img * kGeom;
    o[0] = expanded; o[1] = H; o[2] = W; o[3] = img_y; o[4] = img_x;
    o[5] = crop_y; o[6] = crop_x; o[7] = crop_h; o[8] = crop_w; o[9] = flip;
    o[10] = iou_index; o[11] = outer;
    counts[img] = total;
  }
}

constexpr int kSumBlocks = 64;                    // workgroups per image of the channel sums

__global__ __launch_bounds__(256) void train_channel_sums_kernel(const uint8_t* __restrict__ packed, const int64_t* __restrict__ offsets,
                                                                 const int32_t* __restrict__ hw, const int32_t* __restrict__ geom,
                                                                 unsigned long long* __restrict__ sums) {
  const int img = blockIdx.y;
  if (geom[(long long)img * kGeom] == 0) return;                 // only an expanded image has a fill
  const long long px = (long long)hw[2 * img] * hw[2 * img + 1];
  const uint8_t* src = packed + offsets[img];
  unsigned long long s[3] = {0, 0, 0};
  for (long long p = blockIdx.x * 256 + threadIdx.x; p < px; p += (long long)gridDim.x * 256) {
    const uint8_t* q = src + p * 3;
    s[0] += q[0]; s[1] += q[1]; s[2] += q[2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    for (int off = kWave / 2; off > 0; off >>= 1) s[c] += __shfl_down(s[c], off);
    if ((threadIdx.x & (kWave - 1)) == 0 && s[c] != 0) atomicAdd(&sums[img * 3 + c], s[c]);
  }
}

__global__ __launch_bounds__(256) void preprocess_train_kernel(const uint8_t* __restrict__ packed, const int64_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ hw, const int32_t* __restrict__ geom,
                                                               const unsigned long long* __restrict__ sums, int out_h, int out_w,
                                                               Means mean, float* __restrict__ out) {
  const int img = blockIdx.y;
  const int32_t* g = geom + (long long)img * kGeom;              // uniform per workgroup: scalar loads, scalar registers
  const int expanded = g[0], img_y = g[3], img_x = g[4], cy = g[5], cx = g[6], ch = g[7], cw = g[8], flip = g[9];
  const int h0 = hw[2 * img], w0 = hw[2 * img + 1];
  __shared__ float fill[3];
  if (threadIdx.x < 3)                                           // the mean colour of the image, correctly rounded
    fill[threadIdx.x] = expanded ? (float)((double)sums[img * 3 + threadIdx.x] / (255.0 * (double)h0 * (double)w0)) : 0.f;
  __syncthreads();
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= out_h * out_w) return;
  const int oy = p / out_w, ox = p - oy * out_w;
  const float sy = (float)ch / (float)out_h, sx = (float)cw / (float)out_w;
  const float in_y = (float)oy * sy, in_x = (float)ox * sx;
  const int y0 = (int)floorf(in_y), x0 = (int)floorf(in_x);
  const int y1 = min(y0 + 1, ch - 1), x1 = min(x0 + 1, cw - 1);
  const float ly = in_y - (float)y0, lx = in_x - (float)x0;
  // patch -> canvas (the flip comes before the resize) -> image; a tap the image does not cover reads the fill, so no geometry row can
  // make this kernel read outside the image
  const int r0 = cy + y0 - img_y, r1 = cy + y1 - img_y;
  const int c0 = cx + (flip ? cw - 1 - x0 : x0) - img_x, c1 = cx + (flip ? cw - 1 - x1 : x1) - img_x;
  const bool r0_in = (unsigned)r0 < (unsigned)h0, r1_in = (unsigned)r1 < (unsigned)h0;
  const bool c0_in = (unsigned)c0 < (unsigned)w0, c1_in = (unsigned)c1 < (unsigned)w0;
  const uint8_t* src = packed + offsets[img];
  const uint8_t* p00 = src + ((long long)r0 * w0 + c0) * 3;
  const uint8_t* p01 = src + ((long long)r0 * w0 + c1) * 3;
  const uint8_t* p10 = src + ((long long)r1 * w0 + c0) * 3;
  const uint8_t* p11 = src + ((long long)r1 * w0 + c1) * 3;
  const float k = 1.0f / 255.0f;                                 // convert_image_dtype
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float tl = r0_in && c0_in ? (float)p00[c] * k : fill[c];
    const float tr = r0_in && c1_in ? (float)p01[c] * k : fill[c];
    const float bl = r1_in && c0_in ? (float)p10[c] * k : fill[c];
    const float br = r1_in && c1_in ? (float)p11[c] * k : fill[c];
    const float top = tl + (tr - tl) * lx;
    const float bot = bl + (br - bl) * lx;
    v[c] = (top + (bot - top) * ly) * 255.0f - mean.m[c];
  }
  float* o = out + ((long long)img * out_h * out_w + p) * 3;     // 12 contiguous bytes per lane
  o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

}  // namespace
}  // namespace ron

extern "C" int ron_train_geometry(const int32_t* hw, const int32_t* glabels, const float* gbboxes, int n, int g, const float* draws,
                                  int32_t* geom, int32_t* glabels_out, float* gbboxes_out, int32_t* counts, void* stream) {
  RON_REQUIRE(hw != nullptr && glabels != nullptr && gbboxes != nullptr && draws != nullptr, "ron_train_geometry: null input");
  RON_REQUIRE(geom != nullptr && glabels_out != nullptr && gbboxes_out != nullptr && counts != nullptr, "ron_train_geometry: null output");
  RON_REQUIRE(n > 0, "ron_train_geometry: batch %d", n);
  RON_REQUIRE(g >= 1 && g <= RON_MAX_GT, "ron_train_geometry: %d ground-truth rows not in [1, %d]", g, RON_MAX_GT);
  RON_LAUNCH(ron::train_geometry_kernel, dim3(n), dim3(ron::kWave), 0, (hipStream_t)stream, hw, glabels, gbboxes, g, draws, geom,
             glabels_out, gbboxes_out, counts);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

extern "C" int64_t ron_preprocess_train_workspace_bytes(int n) {
  if (n <= 0) {
    ron::set_error("ron_preprocess_train_workspace_bytes: batch %d", n);
    return -1;
  }
  return ron::align_up((int64_t)n * 3 * (int64_t)sizeof(unsigned long long), 256);
}

extern "C" int ron_preprocess_train(const uint8_t* packed, const int64_t* offsets, const int32_t* hw, const int32_t* geom, int n,
                                    int out_h, int out_w, const float* means, void* workspace, float* out, void* stream) {
  RON_REQUIRE(packed != nullptr && offsets != nullptr && hw != nullptr && geom != nullptr, "ron_preprocess_train: null input");
  RON_REQUIRE(means != nullptr && workspace != nullptr && out != nullptr, "ron_preprocess_train: null means, workspace or output");
  RON_REQUIRE(n > 0 && out_h > 0 && out_w > 0, "ron_preprocess_train: batch %d, output %d x %d", n, out_h, out_w);
  RON_REQUIRE((long long)out_h * out_w <= 0x7fffffffLL, "ron_preprocess_train: output %d x %d too large", out_h, out_w);
  ron::Means m;
  for (int c = 0; c < 3; ++c) m.m[c] = means[c];
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* sums = static_cast<unsigned long long*>(workspace);
  RON_HIP_CHECK(ron::dev_memset_async(sums, 0, (size_t)n * 3 * sizeof(unsigned long long), s));
  RON_LAUNCH(ron::train_channel_sums_kernel, dim3(ron::kSumBlocks, n), dim3(256), 0, s, packed, offsets, hw, geom, sums);
  RON_HIP_CHECK(ron::launch_error());
  const int px = out_h * out_w;
  RON_LAUNCH(ron::preprocess_train_kernel, dim3((px + 255) / 256, n), dim3(256), 0, s, packed, offsets, hw, geom, sums, out_h, out_w, m,
             out);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}
