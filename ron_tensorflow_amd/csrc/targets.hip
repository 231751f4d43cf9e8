// The label side: per-anchor targets (RONNet.bboxes_encode) and the held-out loss (RONNet.losses).
//
// Encode restates tf_ssd_bboxes_encode / tf_ssd_bboxes_encode_layer / do_dual_max_match / iou_matrix (nets/ssd_common.py:337-414,
// :77-147, :49-75, :27-47) for a batch.  Two launches over (image, anchor), the image's boxes in LDS:
//   pass 1  every anchor's best box (first maximum) in registers; every box's best anchor by a wave reduction and one 64-bit
//           atomicMax of the key (overlap bits, ~anchor index) per wave and box: the lowest anchor of maximal overlap wins whatever
//           the arrival order;
//   pass 2  resolves the claims (the lowest box that claims an anchor gets it) and writes the four outputs.
// Losses restate ron_losses (nets/ron_vgg_320.py:635-778): a counting pass (the selection probabilities need the four counts), a
// pass that forms the per-row terms in float32 and adds them per workgroup, and a one-workgroup pass that adds the partial sums in a
// fixed order.  The counts are integer atomics (exact); no floating-point atomics anywhere, so a call is reproducible bit for bit.
// The gradient of the three terms with respect to the head tensors (ron_losses_grad) is one more pass behind those three: the set
// sizes are known by then, so every element is written once, already scaled.
//
// Compiled with -ffp-contract=off: every comparison here decides an index or a set, it has to round once per operation like the
// float32 numpy / TF arithmetic it restates.
#include <hip/hip_runtime.h>

#include <math.h>

#include "loss_device.h"

namespace ron {
namespace {

typedef unsigned long long u64;

RON_KERNEL_ARGS_BEGIN
struct EncodeDev {
  int num_layers;
  int total;                              // anchors per image
  int off[RON_MAX_LAYERS + 1];            // first flat anchor index of a layer
  int na[RON_MAX_LAYERS];                 // anchors per cell
  int fill_ = 0;
  const float* ay[RON_MAX_LAYERS];
  const float* ax[RON_MAX_LAYERS];
  const float* ah[RON_MAX_LAYERS];
  const float* aw[RON_MAX_LAYERS];
  float lo_y[RON_MAX_LAYERS], lo_x[RON_MAX_LAYERS], hi_y[RON_MAX_LAYERS], hi_x[RON_MAX_LAYERS];      // inside bounds
  int64_t* gclasses[RON_MAX_LAYERS];
  float* gloc[RON_MAX_LAYERS];
  float* gscores[RON_MAX_LAYERS];
  float* gbboxes[RON_MAX_LAYERS];
  float low, high;
  float ps[4];
};
RON_KERNEL_ARGS_END(EncodeDev)

struct Anchor {
  int layer, local;                       // layer and index inside the layer's [H, W, A]
  float yc, xc, h, w;                     // centre and size as the wrapper re-derives them (ssd_common.py:375-381)
  float ymin, xmin, ymax, xmax;           // corners as the layer function forms them (:105-108)
  float inside;
};

__device__ inline Anchor load_anchor(const EncodeDev& p, int t) {
  Anchor a;
  int l = 0;
  while (l + 1 < p.num_layers && t >= p.off[l + 1]) ++l;
  a.layer = l;
  a.local = t - p.off[l];
  const int cell = a.local / p.na[l], k = a.local - cell * p.na[l];
  const float y = p.ay[l][cell], x = p.ax[l][cell], h = p.ah[l][k], w = p.aw[l][k];
  const float ymin_ = y - h / 2.f, xmin_ = x - w / 2.f, ymax_ = y + h / 2.f, xmax_ = x + w / 2.f;
  a.yc = (ymin_ + ymax_) / 2.f;
  a.xc = (xmin_ + xmax_) / 2.f;
  a.h = ymax_ - ymin_;
  a.w = xmax_ - xmin_;
  a.ymin = a.yc - a.h / 2.f;
  a.xmin = a.xc - a.w / 2.f;
  a.ymax = a.yc + a.h / 2.f;
  a.xmax = a.xc + a.w / 2.f;
  a.inside = (a.ymin >= p.lo_y[l] && a.xmin >= p.lo_x[l] && a.ymax < p.hi_y[l] && a.xmax < p.hi_x[l]) ? 1.f : 0.f;
  return a;
}

struct BoxesLds {
  float b[RON_MAX_GT][4];
  float area[RON_MAX_GT];
  int present;                            // rows in front of the first padding row
};

// the image's boxes into LDS; returns the number of present rows
__device__ inline int load_boxes(BoxesLds& s, const int32_t* glabels, const float* gbboxes, int img, int G) {
  if (threadIdx.x == 0) s.present = G;
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    const float* bb = gbboxes + ((size_t)img * G + g) * 4;
    const float y0 = bb[0], x0 = bb[1], y1 = bb[2], x1 = bb[3];
    s.b[g][0] = y0; s.b[g][1] = x0; s.b[g][2] = y1; s.b[g][3] = x1;
    s.area[g] = (x1 - x0) * (y1 - y0);
    if (glabels[(size_t)img * G + g] == 0) atomicMin(&s.present, g);
  }
  __syncthreads();
  return s.present;
}

// iou_matrix (ssd_common.py:27-47) times the inside mask (:118); "+ 0.f" folds a -0 quotient into +0
__device__ inline float overlap(const BoxesLds& s, int g, const Anchor& a, float area_a) {
  const float ih = fmaxf(fminf(s.b[g][2], a.ymax) - fmaxf(s.b[g][0], a.ymin), 0.f);
  const float iw = fmaxf(fminf(s.b[g][3], a.xmax) - fmaxf(s.b[g][1], a.xmin), 0.f);
  const float inter = ih * iw;
  const float uni = (s.area[g] + area_a) - inter;
  return (uni == 0.f ? 0.f : inter / uni) * a.inside + 0.f;
}

// float -> unsigned that orders like the float
__device__ inline unsigned ordered_bits(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(kThreads) void encode_match_kernel(EncodeDev p, const int32_t* __restrict__ glabels,
                                                                const float* __restrict__ gbboxes, int G, u64* __restrict__ keys) {
  __shared__ BoxesLds s;
  const int img = blockIdx.y;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  const int present = load_boxes(s, glabels, gbboxes, img, G);
  const bool live = t < p.total;
  Anchor a = load_anchor(p, live ? t : 0);
  const float area_a = (a.xmax - a.xmin) * (a.ymax - a.ymin);
  float best = 0.f;
  int best_g = 0;
  for (int g = 0; g < present; ++g) {
    const float ov = overlap(s, g, a, area_a);
    if (g == 0 || ov > best) { best = ov; best_g = g; }                  // tf.argmax: the first maximum
    // the box's best anchor: the largest (overlap, ~anchor) of the wave, then of the image
    u64 key = live ? ((u64)ordered_bits(ov) << 32) | (u64)(~(unsigned)t) : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const u64 o = __shfl_xor(key, off);
      key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(&keys[(size_t)img * G + g], key);
  }
  if (live) {
    const size_t o = (size_t)img * (p.off[a.layer + 1] - p.off[a.layer]) + a.local;
    p.gscores[a.layer][o] = best;
    p.gclasses[a.layer][o] = best_g;                                     // pass 2 turns the box index into the label
  }
}

__global__ __launch_bounds__(kThreads) void encode_write_kernel(EncodeDev p, const int32_t* __restrict__ glabels,
                                                                const float* __restrict__ gbboxes, int G, const u64* __restrict__ keys) {
  __shared__ BoxesLds s;
  __shared__ int claimed[RON_MAX_GT];                                    // the anchor every box claims
  const int img = blockIdx.y;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  const int present = load_boxes(s, glabels, gbboxes, img, G);
  for (int g = threadIdx.x; g < present; g += kThreads) claimed[g] = (int)~(unsigned)(keys[(size_t)img * G + g] & 0xffffffffull);
  __syncthreads();
  if (t >= p.total) return;
  const Anchor a = load_anchor(p, t);
  const size_t o = (size_t)img * (p.off[a.layer + 1] - p.off[a.layer]) + a.local;
  float score = p.gscores[a.layer][o];
  long long m = p.gclasses[a.layer][o];
  if (present == 0) {
    m = -1;                                                              // no box at all: every anchor is negative
  } else {
    int claim = -1;
    for (int g = 0; g < present; ++g)
      if (claimed[g] == t) { claim = g; break; }                         // tf.argmax over the one-hot rows: the lowest box
    if (claim >= 0) {
      m = claim;
      score = overlap(s, claim, a, (a.xmax - a.xmin) * (a.ymax - a.ymin));
    } else if (score < p.low) {
      m = -1;
    } else if (score < p.high) {                                         // low <= match < high; match == high stays matched
      m = -2;
    }
  }
  const float mask = m > -1 ? 1.f : 0.f;
  const int row = m > 0 ? (int)m : 0;
  float loc[4] = {0.f, 0.f, 0.f, 0.f};
  long long cls = 0;
  if (present > 0) {
    const float gy0 = s.b[row][0], gx0 = s.b[row][1], gy1 = s.b[row][2], gx1 = s.b[row][3];
    const float cy = (((gy1 + gy0) / 2.f - a.yc) / a.h) / p.ps[0];
    const float cx = (((gx1 + gx0) / 2.f - a.xc) / a.w) / p.ps[1];
    const float lh = logf((gy1 - gy0) / a.h) / p.ps[2];
    const float lw = logf((gx1 - gx0) / a.w) / p.ps[3];
    loc[0] = mask * cx; loc[1] = mask * cy; loc[2] = mask * lw; loc[3] = mask * lh;      // a real product: 0 * -inf is NaN (:147)
    cls = (long long)glabels[(size_t)img * G + row] * (m > -1 ? 1 : 0) + (m < -1 ? -1 : 0);
  }
  p.gclasses[a.layer][o] = cls;
  p.gscores[a.layer][o] = present > 0 ? score : 0.f;
  float4* gl = reinterpret_cast<float4*>(p.gloc[a.layer]) + o;
  float4* gb = reinterpret_cast<float4*>(p.gbboxes[a.layer]) + o;
  *gl = make_float4(loc[0], loc[1], loc[2], loc[3]);
  *gb = make_float4(a.ymin, a.xmin, a.ymax, a.xmax);
}

// ----------------------------------------------------------------------------------------------------------------- losses
RON_KERNEL_ARGS_BEGIN
struct LossDev {
  int num_layers, num_classes;
  long long row_off[RON_MAX_LAYERS + 1];  // first flattened row of a layer (batch included)
  const float* cls[RON_MAX_LAYERS];
  const float* obj[RON_MAX_LAYERS];
  const float* loc[RON_MAX_LAYERS];
  const float* objp[RON_MAX_LAYERS];
  const int64_t* gclasses[RON_MAX_LAYERS];
  const float* gloc[RON_MAX_LAYERS];
  float objness_threshold, negative_ratio;
};
RON_KERNEL_ARGS_END(LossDev)

// counters of the workspace (int32): 0 n_pos, 1 n_neg, 2 n_cls_pos, 3 n_cls_neg, 4 objectness set, 5 class set
constexpr int kNumCounts = 6;
constexpr int64_t kPartialsOffset = 64;   // bytes: the double partial sums [workgroups][3] start here

// adds a 0 / 1 flag over the workgroup and lets one thread add the sum to a global counter
__device__ inline void count_flag(bool flag, int* lds_slot, int32_t* counter) {
  const int c = __popcll(__ballot(flag));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(lds_slot, c);
  __syncthreads();
  if (threadIdx.x == 0 && *lds_slot) atomicAdd(counter, *lds_slot);
}

__global__ __launch_bounds__(kThreads) void loss_count_kernel(LossDev p, int32_t* __restrict__ counts) {
  __shared__ int c[4];
  if (threadIdx.x < 4) c[threadIdx.x] = 0;
  __syncthreads();
  const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
  bool pos = false, neg = false, om = false;
  if (r < p.row_off[p.num_layers]) {
    int l; long long j;
    locate_row(p, r, &l, &j);
    const long long g = p.gclasses[l][j];
    pos = g > 0;
    neg = g == 0;
    om = p.objp[l][j] > p.objness_threshold;
  }
  count_flag(pos, &c[0], &counts[0]);
  count_flag(neg, &c[1], &counts[1]);
  count_flag(pos && om, &c[2], &counts[2]);
  count_flag(neg && om, &c[3], &counts[3]);
}

// tfe.safe_divide(min((int)(ratio * n_pos), n_neg), n_neg) (ron_vgg_320.py:700-703), float32
__device__ inline float select_probability(float ratio, int n_pos, int n_neg) {
  const int want = (int)(ratio * (float)n_pos);
  const int sel = want < n_neg ? want : n_neg;
  return n_neg > 0 ? (float)sel / (float)n_neg : 0.f;
}

// custom_layers.modified_smooth_l1, sigma 3 (custom_layers.py:31-49), one coordinate
__device__ inline float smooth_l1(float pred, float target) {
  const float d = pred - target;
  const float sign = fabsf(d) < 1.0f / 9.0f ? 1.f : 0.f;
  const float opt1 = (d * d) * 4.5f;
  const float opt2 = fabsf(d) - 0.5f / 9.0f;
  return opt1 * sign + opt2 * fabsf(sign - 1.f);
}

__global__ __launch_bounds__(kThreads) void loss_rows_kernel(LossDev p, const float* __restrict__ rand_obj,
                                                             const float* __restrict__ rand_cls, int32_t* __restrict__ counts,
                                                             double* __restrict__ partials) {
  __shared__ int c[2];
  __shared__ double red[3][kThreads];
  if (threadIdx.x < 2) c[threadIdx.x] = 0;
  __syncthreads();
  const float p_obj = select_probability(p.negative_ratio, counts[0], counts[1]);
  const float p_cls = select_probability(p.negative_ratio, counts[2], counts[3]);
  const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
  bool in_obj = false, in_cls = false;
  double v_cls = 0.0, v_obj = 0.0, v_loc = 0.0;
  if (r < p.row_off[p.num_layers]) {
    int l; long long j;
    locate_row(p, r, &l, &j);
    const long long g = p.gclasses[l][j];
    const bool pos = g > 0, neg = g == 0;
    const bool om = p.objp[l][j] > p.objness_threshold;
    in_obj = (neg && rand_obj[r] < p_obj) || pos;
    in_cls = (neg && om && rand_cls[r] < p_cls) || (pos && om);
    if (in_cls) v_cls = (double)cross_entropy(p.cls[l] + j * p.num_classes, p.num_classes, clip_label(g, p.num_classes));
    if (in_obj) v_obj = (double)cross_entropy(p.obj[l] + j * 2, 2, pos ? 1 : 0);
    if (pos && om) {
      const float* a = p.loc[l] + j * 4;
      const float* b = p.gloc[l] + j * 4;
      v_loc = (double)(((smooth_l1(a[0], b[0]) + smooth_l1(a[1], b[1])) + smooth_l1(a[2], b[2])) + smooth_l1(a[3], b[3]));
    }
  }
  red[0][threadIdx.x] = v_cls;
  red[1][threadIdx.x] = v_obj;
  red[2][threadIdx.x] = v_loc;
  count_flag(in_obj, &c[0], &counts[4]);
  count_flag(in_cls, &c[1], &counts[5]);           // (both calls synchronise the workgroup: red[] is complete)
  reduce3(red);
  if (threadIdx.x < 3) partials[(size_t)blockIdx.x * 3 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(kThreads) void loss_final_kernel(const double* __restrict__ partials, int num_partials,
                                                              const int32_t* __restrict__ counts, float w_cls, float w_obj,
                                                              float w_loc, float* __restrict__ losses, int32_t* __restrict__ out_counts) {
  __shared__ double red[3][kThreads];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < num_partials; i += kThreads)
    for (int k = 0; k < 3; ++k) acc[k] += partials[(size_t)i * 3 + k];
  for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = acc[k];
  __syncthreads();
  reduce3(red);
  if (threadIdx.x == 0) {
    const int n_pos = counts[0], n_cls_pos = counts[2], n_obj_set = counts[4], n_cls_set = counts[5];
    // tf.reduce_mean over tf.boolean_mask: an empty set is 0 / 0 = NaN (:750, :759, :772)
    const float l_cls = n_pos > 0 ? w_cls * ((float)red[0][0] / (float)n_cls_set) : 0.f;
    const float l_obj = n_pos > 0 ? w_obj * ((float)red[1][0] / (float)n_obj_set) : 0.f;
    const float l_loc = n_cls_pos > 0 ? w_loc * ((float)red[2][0] / (float)n_cls_pos) : 0.f;
    losses[0] = l_cls;
    losses[1] = l_obj;
    losses[2] = l_loc;
    losses[3] = (l_cls + l_obj) + l_loc;
    for (int k = 0; k < kNumCounts; ++k) out_counts[k] = counts[k];
  }
}

// ----------------------------------------------------------------------------------------------------------------- loss gradients
RON_KERNEL_ARGS_BEGIN
struct GradDev {
  float* d_cls[RON_MAX_LAYERS];
  float* d_obj[RON_MAX_LAYERS];
  float* d_loc[RON_MAX_LAYERS];
};
RON_KERNEL_ARGS_END(GradDev)

// d modified_smooth_l1 / d pred, one coordinate: 9 d in the square branch, sign(d) in the linear one; the branch test is the forward's
__device__ inline float smooth_l1_grad(float pred, float target, float s) {
  const float d = pred - target;
  return fabsf(d) < 1.0f / 9.0f ? (9.0f * d) * s : copysignf(1.f, d) * s;
}

// One workgroup owns the same 256 rows as in loss_rows_kernel.  A thread forms its row's sets and writes the row's objectness and
// localisation gradients (8 and 16 bytes per lane: contiguous across lanes).  The rows of the class set go through LDS
// (class_grad_pass); their scale is the same for every row and stays in a register.
__global__ __launch_bounds__(kThreads) void loss_grad_kernel(LossDev p, GradDev q, const float* __restrict__ rand_obj,
                                                             const float* __restrict__ rand_cls, const int32_t* __restrict__ counts,
                                                             float w_cls, float w_obj, float w_loc) {
  __shared__ ClassGradLds lds;
  const int t = threadIdx.x;
  const int C = p.num_classes;
  const int n_pos = counts[0], n_cls_pos = counts[2];
  const float p_obj = select_probability(p.negative_ratio, n_pos, counts[1]);
  const float p_cls = select_probability(p.negative_ratio, n_cls_pos, counts[3]);
  const float s_cls = n_pos > 0 ? w_cls / (float)counts[5] : 0.f;
  const float s_obj = n_pos > 0 ? w_obj / (float)counts[4] : 0.f;
  const float s_loc = n_cls_pos > 0 ? w_loc / (float)n_cls_pos : 0.f;
  const long long r = (long long)blockIdx.x * kThreads + t;
  const long long total = p.row_off[p.num_layers];
  const float* src = nullptr;
  float* dst = nullptr;
  int lab = -1;
  if (r < total) {
    int l; long long j;
    locate_row(p, r, &l, &j);
    const long long g = p.gclasses[l][j];
    const bool pos = g > 0, neg = g == 0;
    const bool om = p.objp[l][j] > p.objness_threshold;
    const bool in_obj = (neg && rand_obj[r] < p_obj) || pos;
    const bool in_cls = (neg && om && rand_cls[r] < p_cls) || (pos && om);
    src = p.cls[l] + j * C;
    dst = q.d_cls[l] + j * C;
    if (in_cls) lab = clip_label(g, C);
    float2 go = make_float2(0.f, 0.f);
    if (in_obj) {
      const float2 x = *(reinterpret_cast<const float2*>(p.obj[l]) + j);
      const float mx = fmaxf(x.x, x.y);
      const float e0 = expf(x.x - mx), e1 = expf(x.y - mx);
      const float sum = e0 + e1;
      go.x = (e0 / sum - (pos ? 0.f : 1.f)) * s_obj;
      go.y = (e1 / sum - (pos ? 1.f : 0.f)) * s_obj;
    }
    *(reinterpret_cast<float2*>(q.d_obj[l]) + j) = go;
    float4 gl = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pos && om) {
      const float4 a = *(reinterpret_cast<const float4*>(p.loc[l]) + j);
      const float4 b = *(reinterpret_cast<const float4*>(p.gloc[l]) + j);
      gl = make_float4(smooth_l1_grad(a.x, b.x, s_loc), smooth_l1_grad(a.y, b.y, s_loc), smooth_l1_grad(a.z, b.z, s_loc),
                       smooth_l1_grad(a.w, b.w, s_loc));
    }
    *(reinterpret_cast<float4*>(q.d_loc[l]) + j) = gl;
  }
  class_grad_pass(lds, C, src, dst, lab, [s_cls](int) { return s_cls; });
}

// workspace: the counters, then the partial sums of every workgroup
struct Layout {
  int64_t rows, wgs, bytes;
};

Layout workspace_layout(const ron_heads* heads, int n) {
  Layout w;
  w.rows = count_rows(heads, n);
  w.wgs = (w.rows + kThreads - 1) / kThreads;
  w.bytes = kPartialsOffset + w.wgs * 3 * (int64_t)sizeof(double);
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

}  // namespace
}  // namespace ron

extern "C" int64_t ron_bboxes_encode_workspace_bytes(int n, int g) {
  if (n <= 0 || g < 1 || g > RON_MAX_GT) {
    ron::set_error("ron_bboxes_encode_workspace_bytes: n %d, ground-truth boxes per image %d not in [1, %d]", n, g, RON_MAX_GT);
    return -1;
  }
  return (int64_t)n * g * (int64_t)sizeof(ron::u64);
}

extern "C" int ron_bboxes_encode(const ron_heads* anchors, int n, const int32_t* glabels, const float* gbboxes, int g, int img_h,
                                 int img_w, const int32_t* allowed_borders, float positive_threshold, float ignore_threshold,
                                 const float prior_scaling[4], void* workspace, int64_t workspace_bytes, ron_targets* out,
                                 void* stream) {
  if (int rc = ron::check_layers(anchors, "ron_bboxes_encode")) return rc;
  RON_REQUIRE(n > 0 && img_h > 0 && img_w > 0, "ron_bboxes_encode: bad batch / image shape");
  RON_REQUIRE(g >= 1 && g <= RON_MAX_GT, "ron_bboxes_encode: ground-truth boxes per image %d not in [1, %d]", g, RON_MAX_GT);
  RON_REQUIRE(glabels != nullptr && gbboxes != nullptr && allowed_borders != nullptr && prior_scaling != nullptr && out != nullptr,
              "ron_bboxes_encode: null argument");
  const int64_t need = (int64_t)n * g * (int64_t)sizeof(ron::u64);
  RON_REQUIRE(workspace != nullptr && workspace_bytes >= need, "ron_bboxes_encode: workspace of %lld bytes, %lld needed",
              (long long)workspace_bytes, (long long)need);
  ron::EncodeDev p = {};
  p.num_layers = anchors->num_layers;
  int64_t total = 0;
  for (int l = 0; l < p.num_layers; ++l) {
    RON_REQUIRE(anchors->anchor_y[l] && anchors->anchor_x[l] && anchors->anchor_h[l] && anchors->anchor_w[l],
                "ron_bboxes_encode: null anchor pointer of layer %d", l);
    RON_REQUIRE(out->gclasses[l] && out->glocalisations[l] && out->gscores[l] && out->gbboxes[l],
                "ron_bboxes_encode: null target pointer of layer %d", l);
    p.off[l] = (int)total;
    p.na[l] = anchors->num_anchors[l];
    total += (int64_t)anchors->feat_h[l] * anchors->feat_w[l] * anchors->num_anchors[l];
    RON_REQUIRE(total < (1ll << 30), "ron_bboxes_encode: too many anchors");
    p.ay[l] = anchors->anchor_y[l]; p.ax[l] = anchors->anchor_x[l]; p.ah[l] = anchors->anchor_h[l]; p.aw[l] = anchors->anchor_w[l];
    // the bounds are formed in double and rounded to float32 (ssd_common.py:112-115)
    const double b = (double)allowed_borders[l];
    p.lo_y[l] = (float)(-b * 1. / img_h);
    p.lo_x[l] = (float)(-b * 1. / img_w);
    p.hi_y[l] = (float)((img_h + b) * 1. / img_h);
    p.hi_x[l] = (float)((img_w + b) * 1. / img_w);
    p.gclasses[l] = out->gclasses[l]; p.gloc[l] = out->glocalisations[l]; p.gscores[l] = out->gscores[l]; p.gbboxes[l] = out->gbboxes[l];
  }
  p.off[p.num_layers] = (int)total;
  p.total = (int)total;
  p.low = ignore_threshold;
  p.high = positive_threshold;
  for (int i = 0; i < 4; ++i) p.ps[i] = prior_scaling[i];
  hipStream_t s = (hipStream_t)stream;
  RON_HIP_CHECK(ron::dev_memset_async(workspace, 0, (size_t)need, s));
  const dim3 grid((unsigned)((total + ron::kThreads - 1) / ron::kThreads), (unsigned)n);
  RON_LAUNCH(ron::encode_match_kernel, grid, dim3(ron::kThreads), 0, s, p, glabels, gbboxes, g, (ron::u64*)workspace);
  RON_LAUNCH(ron::encode_write_kernel, grid, dim3(ron::kThreads), 0, s, p, glabels, gbboxes, g, (const ron::u64*)workspace);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

extern "C" int64_t ron_losses_workspace_bytes(const ron_heads* heads, int n) {
  return ron::workspace_bytes("ron_losses_workspace_bytes", heads, n);
}

extern "C" int64_t ron_losses_grad_workspace_bytes(const ron_heads* heads, int n) {
  return ron::workspace_bytes("ron_losses_grad_workspace_bytes", heads, n);
}

// what ron_losses and ron_losses_grad share: the arguments checked, the kernels' parameter block filled
static int loss_setup(const char* what, const ron_heads* heads, const float* const* objness_pred, const ron_targets* targets, int n,
                      const float* rand_objness, const float* rand_cls, const ron_loss_cfg* cfg, void* workspace,
                      int64_t workspace_bytes, float* losses, int32_t* counts, ron::LossDev* out, int64_t* out_wgs) {
  if (int rc = ron::check_layers(heads, what)) return rc;
  RON_REQUIRE(n > 0, "%s: bad batch %d", what, n);
  RON_REQUIRE(objness_pred != nullptr && targets != nullptr && rand_objness != nullptr && rand_cls != nullptr && cfg != nullptr &&
              losses != nullptr && counts != nullptr, "%s: null argument", what);
  RON_REQUIRE(heads->num_classes >= 2 && heads->num_classes <= RON_MAX_CLASSES, "%s: %d classes not in [2, %d]", what,
              heads->num_classes, RON_MAX_CLASSES);
  ron::LossDev p = {};
  p.num_layers = heads->num_layers;
  p.num_classes = heads->num_classes;
  int64_t rows = 0;
  for (int l = 0; l < p.num_layers; ++l) {
    RON_REQUIRE(heads->cls[l] && heads->obj[l] && heads->loc[l] && objness_pred[l], "%s: null head pointer of layer %d", what, l);
    RON_REQUIRE(targets->gclasses[l] && targets->glocalisations[l], "%s: null target pointer of layer %d", what, l);
    p.row_off[l] = rows;
    rows += (int64_t)n * heads->feat_h[l] * heads->feat_w[l] * heads->num_anchors[l];
    p.cls[l] = heads->cls[l]; p.obj[l] = heads->obj[l]; p.loc[l] = heads->loc[l]; p.objp[l] = objness_pred[l];
    p.gclasses[l] = targets->gclasses[l]; p.gloc[l] = targets->glocalisations[l];
  }
  p.row_off[p.num_layers] = rows;
  RON_REQUIRE(rows < (1ll << 24) * 64, "%s: too many rows", what);
  p.objness_threshold = cfg->objness_threshold;
  p.negative_ratio = cfg->negative_ratio;
  const ron::Layout w = ron::workspace_layout(heads, n);
  RON_REQUIRE(workspace != nullptr && workspace_bytes >= w.bytes, "%s: workspace of %lld bytes, %lld needed", what,
              (long long)workspace_bytes, (long long)w.bytes);
  RON_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", what);
  *out = p;
  *out_wgs = w.wgs;
  return RON_OK;
}

// the class term's weight: 1 - alpha - beta, formed once in double (:750)
static float class_weight(const ron_loss_cfg* cfg) { return (float)(1.0 - (double)cfg->alpha - (double)cfg->beta); }

// the three forward launches; the counters and the partial sums stay in the workspace
static int loss_forward(const ron::LossDev& p, int64_t wgs, const float* rand_objness, const float* rand_cls, const ron_loss_cfg* cfg,
                        void* workspace, float* losses, int32_t* counts, hipStream_t s) {
  int32_t* d_counts = (int32_t*)workspace;
  double* partials = (double*)((char*)workspace + ron::kPartialsOffset);
  RON_HIP_CHECK(ron::dev_memset_async(workspace, 0, (size_t)ron::kPartialsOffset, s));
  RON_LAUNCH(ron::loss_count_kernel, dim3((unsigned)wgs), dim3(ron::kThreads), 0, s, p, d_counts);
  RON_LAUNCH(ron::loss_rows_kernel, dim3((unsigned)wgs), dim3(ron::kThreads), 0, s, p, rand_objness, rand_cls, d_counts, partials);
  RON_LAUNCH(ron::loss_final_kernel, dim3(1), dim3(ron::kThreads), 0, s, (const double*)partials, (int)wgs, (const int32_t*)d_counts,
             class_weight(cfg), cfg->alpha, cfg->beta, losses, counts);
  return RON_OK;
}

extern "C" int ron_losses(const ron_heads* heads, const float* const* objness_pred, const ron_targets* targets, int n,
                          const float* rand_objness, const float* rand_cls, const ron_loss_cfg* cfg, void* workspace,
                          int64_t workspace_bytes, float* losses, int32_t* counts, void* stream) {
  ron::LossDev p;
  int64_t wgs;
  if (int rc = loss_setup("ron_losses", heads, objness_pred, targets, n, rand_objness, rand_cls, cfg, workspace, workspace_bytes,
                          losses, counts, &p, &wgs))
    return rc;
  if (int rc = loss_forward(p, wgs, rand_objness, rand_cls, cfg, workspace, losses, counts, (hipStream_t)stream)) return rc;
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

extern "C" int ron_losses_grad(const ron_heads* heads, const float* const* objness_pred, const ron_targets* targets, int n,
                               const float* rand_objness, const float* rand_cls, const ron_loss_cfg* cfg, void* workspace,
                               int64_t workspace_bytes, float* losses, int32_t* counts, const ron_head_grads* grads, void* stream) {
  ron::LossDev p;
  int64_t wgs;
  if (int rc = loss_setup("ron_losses_grad", heads, objness_pred, targets, n, rand_objness, rand_cls, cfg, workspace,
                          workspace_bytes, losses, counts, &p, &wgs))
    return rc;
  RON_REQUIRE(grads != nullptr, "ron_losses_grad: null argument");
  ron::GradDev q = {};
  for (int l = 0; l < p.num_layers; ++l) {
    RON_REQUIRE(grads->d_cls[l] && grads->d_obj[l] && grads->d_loc[l], "ron_losses_grad: null gradient pointer of layer %d", l);
    // the kernel moves an objectness row as one 8-byte and a localisation row as one 16-byte access
    RON_REQUIRE((((uintptr_t)p.obj[l] | (uintptr_t)grads->d_obj[l]) & 7) == 0 &&
                (((uintptr_t)p.loc[l] | (uintptr_t)p.gloc[l] | (uintptr_t)grads->d_loc[l]) & 15) == 0,
                "ron_losses_grad: obj / d_obj of layer %d must be 8-byte, loc / glocalisations / d_loc 16-byte aligned", l);
    q.d_cls[l] = grads->d_cls[l]; q.d_obj[l] = grads->d_obj[l]; q.d_loc[l] = grads->d_loc[l];
  }
  hipStream_t s = (hipStream_t)stream;
  if (int rc = loss_forward(p, wgs, rand_objness, rand_cls, cfg, workspace, losses, counts, s)) return rc;
  RON_LAUNCH(ron::loss_grad_kernel, dim3((unsigned)wgs), dim3(ron::kThreads), 0, s, p, q, rand_objness, rand_cls,
             (const int32_t*)workspace, class_weight(cfg), cfg->alpha, cfg->beta);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}
