// ron_ctx: the RON-320 conv stack as a fixed launch plan over pre-allocated HBM tensors.
//
// Restates the graph of nets/ron_vgg_320.py (ron_net :434-508, ron_net_reducedfc :510-580,
// reverse_connection_module_with_pred :418-432, pred_cls_module :378-404, reg_bbox_module
// :406-415) with the slim layer semantics of ron_arg_scope (:595-629), re-planned for the
// MFMA implicit-GEMM kernel:
//   * inference BatchNorm (eps 1e-5) is folded into the preceding conv at load time;
//   * per scale, everything that reads the reference map (objectness hidden layer, box hidden layer,
//     both inception-1 branches) runs as ONE conv with 2048 output channels, the 1x1 branch in the centre
//     tap of its rows (those column tiles run that tap's K steps only); inception-2 likewise; the
//     BatchNorm after each concat is split per branch and folded; consumers read channel slices;
//   * the 2x2 stride-2 transposed conv is a GEMM with a pixel-shuffle epilogue; the left conv of a
//     reverse connection writes its half of relu(left + up) first and the transposed conv adds its
//     half in place, so only the (small) transposed convs sit on the coarse -> fine chain;
//   * head logits are written as fp32 straight into the caller's buffers.
// Every activation lives in HBM as NHWC with a zero halo (conv_mfma.h); all buffers are
// allocated once for max_batch images (activations of the full variant: ~150 MB / image).
//
// The four networks (RON-320 reducedfc / full, SSD-512, SSD-300) are one VGG-16 body (VggBody) and one of two tails: the reverse
// connections of RON, or the extra blocks + multibox heads of SSD (SsdSpec).  Variables, tensors and ops of each are declared by
// the same three steps, body first.
#include <math.h>

#include <array>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "pack.h"

using namespace ron;

namespace {

constexpr float kBnEps = 1e-5f;
constexpr int kCarrierPlanMinBatch = 24;   // contexts from this max_batch on pack the small head convolutions into the partial rounds of 256 x 256 launches
constexpr int kLevelPlanMaxBatch = 12;      // contexts up to this max_batch run the heads one launch per dependency level (plan_groups)
const char* kFeatLayers[4] = {"block7", "block6", "block5", "block4"};

struct Var {
  std::string name;
  std::vector<int64_t> shape;
  std::vector<float> data;
  bool loaded = false;
  int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

struct Tensor {
  std::string name;
  int H, W, C, pad;
  int cstride = 0;           // elements per pixel in memory (>= C): wide tensors get +64 so that the pixel stride
                             // is not a power of two (4 KiB strides serialise on a few L2 channels)
  DevBuf d;
  int64_t bytes = 0;
};

struct PackedConv {
  DevBuf w;
  int64_t w_bytes = 0;
  DevBuf w_c64;               // 3x3 on 64 input channels (conv2_1): the weights once more as LDS images for conv_c64.hip
  DevBuf bias;
  float oscale = 1.f;         // accumulator scale of the epilogue (split-precision weights are stored times a power of two)
  int Npad = 0, Cout = 0;
  int split_n = 0, split_first = 0;   // two head convolutions packed side by side (pack_box_pair): ConvLaunch::split_n
};

// What ron_finalize_weights puts on the device.  The context that packed it owns it; an execution slot (ron_clone) points at its
// owner's, so nothing here is ever listed buffer by buffer.
struct Weights {
  std::vector<PackedConv> packed;
  DevBuf l2_gamma;            // SSD block4 L2Normalization scale
  DevBuf stem_w, stem_b;      // conv1_1 fragments + bias for the dedicated stem kernel (bf16 / f16)
  float stem_oscale = 1.f;    // split precision: 2^-k of the stem weights' scale
  DevBuf stem2_w;             // conv1_2 weights as the LDS image of stem2_kernel (conv1_1 + conv1_2 + pool1 fused)
  DevBuf stem2_w1;            // conv1_1 weights as 16x16x32 fragments for stem2_kernel
  DevBuf stem2_b;
};

enum OpKind { OP_IM2COL, OP_CONV, OP_POOL, OP_STEM, OP_POOL3, OP_L2NORM, OP_STEM2 };

struct Op {
  OpKind kind;
  std::string name;
  int in = -1, out = -1, res = -1;      // tensor indices; out == -2: caller head buffer
  int in_coff = 0, in_C = 0;            // channel slice of the input
  int packed = -1;
  int kh = 1, kw = 1, stride = 1, dil = 1, cpad = 0, relu = 0;
  int up = 0, up_cout = 0, pool = 0;
  int center_from = 0;                  // output channels >= this hold a 1x1 branch in the centre tap of the 3x3 filter (0: none)
  int fuse_next_pool = 0;               // the next op is this conv's 2x2 pool and both maps are needed (conv4_3, conv5_3): one launch
                                        // with two outputs whenever the conv would not split K (decided per batch by slot_resources)
  int head_kind = -1, head_layer = -1;  // 0 cls, 1 obj, 2 loc
  int head_kind2 = -1;                  // a second head output of the same layer from the same launch (pack_box_pair), or -1
  int Ho = 0, Wo = 0;
  int lane = 0;                         // 0 = the caller's stream; 1..3 = side streams (independent head branches)
  int group = -1;                       // >= 0: launched together with the neighbouring ops of the same group (launch_conv_group)
  int group_cfg = 0;                    // tile configuration of that grouped launch
  double flops = 0;                     // algorithmic 2*MAC per image of this launch
  double act_bytes = 0;                 // algorithmic HBM bytes per image: input read once + output written once
  double wgt_bytes = 0;                 // ... plus the packed weights, once per launch
};

struct OpTiming {
  double ms = 0;
  int launches = 0;
};

// What a profiling stamp marks (ron_ctx::pending_ops): an op index >= 0 (the op's start), or one of these.  The end of side lane l is
// kStampLaneEnd - 10 * l.
constexpr int kStampLaneEnd = -1, kStampPostStart = -2, kStampPostEnd = -3;

}  // namespace

struct ron_ctx {
  ron_config cfg;
  int c6 = 0;                 // fc6 / fc7 channels
  int num_anchors = 10;                 // RON: anchors per cell on every scale
  // head layers, generic (RON: 4 scales x 10 anchors + objectness; SSD-512 / SSD-300: 7 / 6 scales, 4/6 anchors, no objectness)
  int n_feat = 0;
  int feat_h[RON_MAX_LAYERS] = {}, feat_w[RON_MAX_LAYERS] = {}, feat_A[RON_MAX_LAYERS] = {};
  bool has_obj = true;
  bool is_ssd() const { return cfg.variant == RON_VARIANT_SSD512 || cfg.variant == RON_VARIANT_SSD300; }
  const char* scope() const { return cfg.variant == RON_VARIANT_SSD512 ? "ssd_512_vgg" : (cfg.variant == RON_VARIANT_SSD300 ? "ssd_300_vgg" : "ron_320_vgg"); }
  std::vector<Var> vars;
  std::map<std::string, int> var_index;
  std::vector<Tensor> tensors;
  std::map<std::string, int> tensor_index;
  Weights own;                          // filled by ron_finalize_weights; empty in an execution slot
  const Weights* wts = &own;            // ron_clone: the owner's
  std::vector<Op> ops;
  bool finalized = false;
  double flops_per_image = 0;
  // anchors (device) + head buffers / workspace for ron_detect
  DevBuf anchor[RON_MAX_LAYERS][4];
  DevBuf head[3][RON_MAX_LAYERS];
  DevBuf post_ws;
  int64_t post_ws_bytes = 0;
  bool post_ws_dirty = false;     // a ron_detect / ron_detect_tfe call failed after its select pass may have run: the self-cleaning counters are re-zeroed on the next call
  bool tfe_counters_stale = false;  // ron_detect ran since the last ron_detect_tfe: its keys may sit on the TF counters (postproc.hip, post_tfe_ctx)
  DevBuf splitk[4];                     // fp32 slabs of the split-K launches, one set per stream lane
  int64_t splitk_bytes[4] = {};
  // RON_CFG_MULTI_STREAM: the heads of the three coarse scales run on side streams beside the main chain
  Stream side[4];
  Event lane_ready[4], lane_done[4];
  // optional per-launch timing (ron_profile_*): event pairs recorded on the caller's stream
  int profiling = 0;                    // calls still to be recorded (ron_profile_enable)
  std::vector<OpTiming> timing;                       // ops.size() + 1 (last = post-processing)
  std::vector<std::string> labels;                    // ron_profile_get names, one per op, built once (stable until ron_destroy)
  int grouped_launches = 0;                           // grouped launches in the plan (0: one launch per convolution)
  // What each conv launch does at each batch size, [batch 1 .. max_batch][first op of the launch]: decided once by slot_resources (a
  // clone copies its owner's) and only read by ron_forward - conv_group_plan models a launch's schedule, ~1 ms: too slow to enqueue with.
  struct LaunchPlan {
    std::array<int, kMaxConvGroup> sk{};      // a grouped launch: the members' split-K factors
    bool fuse_pool = false;                   // conv4_3 / conv5_3 (Op::fuse_next_pool): the conv takes its pool along at this batch
  };
  std::vector<std::vector<LaunchPlan>> launch_plans;
  std::vector<std::vector<Event>> pending;            // per recorded call: one event per stamp ...
  std::vector<std::vector<int>> pending_ops;          // ... and what it marks: op index or kStamp*
  std::vector<Event> event_pool;
  // ron_clone: an execution slot that borrows the packed weights of `weights_owner` (its own activations, scratch, streams)
  ron_ctx* weights_owner = nullptr;
  int clones = 0;                       // live slots that borrow this context's weights

  int esz() const { return (int)dtype_size(cfg.dtype); }
  int add_tensor(const std::string& name, int H, int W, int C, int pad) {
    Tensor t;
    t.name = name; t.H = H; t.W = W; t.C = C; t.pad = pad;
    t.cstride = C >= 1024 ? C + 64 : C;
    tensors.push_back(std::move(t));
    tensor_index[name] = (int)tensors.size() - 1;
    return (int)tensors.size() - 1;
  }
  int T(const std::string& name) const { return tensor_index.at(name); }
  void add_var(const std::string& rel, std::vector<int64_t> shape) {
    Var v;
    v.name = std::string(scope()) + "/" + rel;
    v.shape = shape;
    var_index[v.name] = (int)vars.size();
    vars.push_back(v);
  }
  void add_conv_vars(const std::string& rel, int k, int cin, int cout) {      // a convolution with a bias
    add_var(rel + "/weights", {k, k, cin, cout});
    add_var(rel + "/biases", {cout});
  }
  void add_feat(int h, int w, int A) { feat_h[n_feat] = h; feat_w[n_feat] = w; feat_A[n_feat] = A; ++n_feat; }
  const Var& var(const std::string& rel) const { return vars[var_index.at(std::string(scope()) + "/" + rel)]; }
  TensorView view(int t, int n, int coff = 0, int C = -1) const {
    const Tensor& T = tensors[t];
    TensorView v;
    v.base = T.d; v.bytes = T.bytes; v.N = n; v.H = T.H; v.W = T.W; v.pad = T.pad; v.cstride = T.cstride;
    v.coff = coff; v.C = C < 0 ? T.C : C;
    return v;
  }
};

namespace {

// ---------------------------------------------------------------------------------------------------------
// The VGG-16 body, conv1_1 ... pool5: the same thirteen convolutions in all four networks.  What differs per family is below
// (VggBody); how conv1_1 / conv1_2 / the pools are launched depends on the dtype and the RON_CFG_* flags alone (stem_kernel,
// pool_fused, stem2_fused).
// ---------------------------------------------------------------------------------------------------------
struct BodyConv {
  int block;                 // 0 .. 4
  bool last;                 // the block's last convolution: its pool follows
  int cin, cout;
  std::string name, scope;   // "conv4_3", "conv4/conv4_3"
};
std::vector<BodyConv> vgg_body_convs() {
  const int widths[5] = {64, 128, 256, 512, 512};
  const int reps[5] = {2, 2, 3, 3, 3};
  std::vector<BodyConv> v;
  int cin = 3;
  for (int b = 0; b < 5; ++b)
    for (int r = 0; r < reps[b]; ++r) {
      const std::string blk = "conv" + std::to_string(b + 1), nm = blk + "_" + std::to_string(r + 1);
      v.push_back({b, r == reps[b] - 1, cin, widths[b], nm, blk + "/" + nm});
      cin = widths[b];
    }
  return v;
}
struct VggBody {
  int early_last_pad;        // halo of conv1_2 / conv2_2 / conv3_3, which feed nothing but their pool (RON: none)
  OpKind pool5;              // OP_POOL: 2x2 stride 2 like pool1-4 (RON); OP_POOL3: 3x3 stride 1 (SSD, nets/ssd_vgg_512.py:391)
  int pool5_pad;             // halo of pool5 = the reach of what reads it: fc6 (7x7, or 3x3 at rate 3), conv6 (3x3 at rate 6)
};
const VggBody kRonBody = {0, OP_POOL, 3}, kSsdBody = {1, OP_POOL3, 6};
const VggBody& vgg_body(const ron_ctx* c) { return c->is_ssd() ? kSsdBody : kRonBody; }

// slim.max_pool2d [2, 2] stride 2 SAME; a k x k convolution with stride s over a map zero-padded by p
int pool2_out(int h) { return (h + 1) / 2; }
int conv_out(int h, int k, int stride, int p) { return (h + 2 * p - k) / stride + 1; }

bool stem_kernel(const ron_config& cfg) { return cfg.dtype != RON_DTYPE_F32; }      // bf16 / f16 / f16x3; fp32: conv1_1 as im2col + GEMM
// blocks 1..3 feed nothing but their pool: with RON_CFG_FUSE_POOLS the h x w map of the block's last conv is never written
bool pool_fused(const ron_config& cfg, int h, int w) {
  return (cfg.flags & RON_CFG_FUSE_POOLS) && !((cfg.flags & RON_CFG_NO_ODD_POOL_FUSE) && ((h | w) & 1));
}
// conv1_1 + conv1_2 + pool1 as one kernel (stem.hip): neither full-resolution 64-channel map touches HBM
bool stem2_fused(const ron_config& cfg) {
  return (cfg.flags & RON_CFG_FUSE_POOLS) && !(cfg.flags & RON_CFG_NO_STEM2) && dtype_is_half(cfg.dtype) && cfg.img_h % 8 == 0 &&
         cfg.img_w % 32 == 0;
}

// ---------------------------------------------------------------------------------------------------------
// SSD (nets/ssd_vgg_512.py:364-460, nets/ssd_vgg_300.py:434-523; multibox heads nets/ssd_vgg_300.py:403-431): one description per
// variant, read by declare_ssd_variables, declare_ssd_tensors, make_anchors, build_ssd_tail and head_plan.
// ---------------------------------------------------------------------------------------------------------
constexpr int kSsdMaxFeat = 7, kSsdMaxExtra = 5;
struct SsdExtra { int mid, outc, k, stride, cpad; };      // block8 ...: 1x1 to `mid` channels, then k x k (stride, zero padding cpad) to `outc`
struct SsdSpec {
  const char* scope;
  int img;                                // the one input size of the variant (square)
  int n_feat;
  const char* feat[kSsdMaxFeat];          // feature layers: block4 (L2-normalised), block7 (= conv7), then the extra blocks
  int anchors[kSsdMaxFeat];               // per cell: len(sizes) + len(ratios); 4 = ratios {2, 1/2}, 6 = {2, 1/2, 3, 1/3}
  int feat_c[kSsdMaxFeat];
  int n_extra;
  SsdExtra extra[kSsdMaxExtra];           // pad2d(1) + VALID of the reference = cpad 1; plain VALID = cpad 0
  double sizes[kSsdMaxFeat][2], steps[kSsdMaxFeat];      // SSDNet.default_params
};
// nets/ssd_vgg_512.py:79-102, :395-458: blocks 8-11 are 1x1 then pad 1 + 3x3 stride 2, block12 1x1 then pad 1 + 4x4
const SsdSpec kSsd512 = {
    "ssd_512_vgg", 512, 7,
    {"block4", "block7", "block8", "block9", "block10", "block11", "block12"},
    {4, 6, 6, 6, 6, 4, 4},
    {512, 1024, 512, 256, 256, 256, 256},
    5, {{256, 512, 3, 2, 1}, {128, 256, 3, 2, 1}, {128, 256, 3, 2, 1}, {128, 256, 3, 2, 1}, {128, 256, 4, 1, 1}},
    {{20.48, 51.2}, {51.2, 133.12}, {133.12, 215.04}, {215.04, 296.96}, {296.96, 378.88}, {378.88, 460.8}, {460.8, 542.72}},
    {8, 16, 32, 64, 128, 256, 512}};
// nets/ssd_vgg_300.py:94-124, :466-503: blocks 8 / 9 are 1x1 then pad 1 + 3x3 stride 2 (19 -> 10 -> 5), blocks 10 / 11 1x1 then 3x3
// VALID (5 -> 3 -> 1); 8732 anchors
const SsdSpec kSsd300 = {
    "ssd_300_vgg", 300, 6,
    {"block4", "block7", "block8", "block9", "block10", "block11"},
    {4, 6, 6, 6, 4, 4},
    {512, 1024, 512, 256, 256, 256},
    4, {{256, 512, 3, 2, 1}, {128, 256, 3, 2, 1}, {128, 256, 3, 1, 0}, {128, 256, 3, 1, 0}},
    {{21., 45.}, {45., 99.}, {99., 153.}, {153., 207.}, {207., 261.}, {261., 315.}},
    {8, 16, 32, 64, 100, 300}};
// SSDNet.default_params anchors with ssd_anchor_one_layer (nets/ssd_vgg_512.py:286-338): anchors per cell are [s0 square,
// sqrt(s0*s1) square, s0 at each of the first A - 2 ratios]
const double kSsdRatios[4] = {2, .5, 3, 1. / 3};
// RONNet.default_params (nets/ron_vgg_320.py:97-124), coarse -> fine like kFeatLayers: every size at every ratio
const struct { double sizes[4][2], ratios[5], steps[4]; } kRonAnchors = {
    {{224., 256.}, {160., 192.}, {96., 128.}, {32., 64.}}, {1., 2., 3., 1. / 2, 1. / 3}, {64, 32, 16, 8}};
const SsdSpec* ssd_spec(int variant) {
  return variant == RON_VARIANT_SSD512 ? &kSsd512 : (variant == RON_VARIANT_SSD300 ? &kSsd300 : nullptr);
}
std::string ssd_block(int b) { return "block" + std::to_string(8 + b); }
std::string ssd_extra_conv(const SsdExtra& e) { return "conv" + std::to_string(e.k) + "x" + std::to_string(e.k); }
// Feature layers whose loc + cls convolutions run as one two-output launch (block4: 64 x 64 / 38 x 38, block7: 32 x 32 / 19 x 19).
// The small maps' heads stay two members of a grouped launch with the next block's 1x1 (head_plan).
const int kSsdPairedHeads = 2;

// ---- step 1: the variable list (names/shapes as TensorFlow stores them; SURVEY.md 8b weight contract) ----------------------
void add_bn_vars(ron_ctx* c, const std::string& scope, int ch) {
  for (const char* n : {"beta", "gamma", "moving_mean", "moving_variance"}) c->add_var(scope + "/BatchNorm/" + n, {ch});
}

void declare_ron_variables(ron_ctx* c) {
  const int nc = c->cfg.num_classes, A = c->num_anchors, c6 = c->c6;
  c->add_conv_vars("fc6", c->cfg.variant == RON_VARIANT_FULL ? 7 : 3, 512, c6);
  c->add_conv_vars("fc7", 1, c6, c6);
  for (int i = 0; i < 4; ++i) {
    const std::string L = std::string("reverse_module/") + kFeatLayers[i] + "_reverse";
    const int left_c = i < 2 ? c6 : 512;
    const int k = i == 0 ? 2 : 3;
    c->add_var(L + "_conv_left/weights", {k, k, left_c, 512});
    add_bn_vars(c, L + "_conv_left", 512);
    if (i > 0) c->add_conv_vars(L + "_deconv_right", 2, 512, 512);
    c->add_var(L + "_objectness/weights", {3, 3, 512, 512});
    add_bn_vars(c, L + "_objectness", 512);
    c->add_conv_vars(L + "_objectness_score", 3, 512, 2 * A);
    for (int blk = 1; blk <= 2; ++blk) {
      const std::string I = L + "_inception" + std::to_string(blk);
      const int ic = blk == 1 ? 512 : 1024;
      c->add_conv_vars(I + "/Branch_0/Conv2d_3x3", 3, ic, 512);
      c->add_conv_vars(I + "/Branch_1/Conv2d_1x1", 1, ic, 512);
      add_bn_vars(c, I, 1024);
    }
    c->add_conv_vars(L + "_inception2/Conv2d_pred_3x3", 3, 1024, A * nc);
    c->add_var(L + "/Conv2d_0_3x3/weights", {3, 3, 512, 512});
    add_bn_vars(c, L + "/Conv2d_0_3x3", 512);
    c->add_conv_vars(L + "/Conv2d_1_3x3", 3, 512, 4 * A);
  }
}

void declare_ssd_variables(ron_ctx* c, const SsdSpec& S) {
  c->add_conv_vars("conv6", 3, 512, 1024);
  c->add_conv_vars("conv7", 1, 1024, 1024);
  int inc = 1024;
  for (int b = 0; b < S.n_extra; ++b) {
    const SsdExtra& e = S.extra[b];
    c->add_conv_vars(ssd_block(b) + "/conv1x1", 1, inc, e.mid);
    c->add_conv_vars(ssd_block(b) + "/" + ssd_extra_conv(e), e.k, e.mid, e.outc);
    inc = e.outc;
  }
  for (int i = 0; i < S.n_feat; ++i) {
    const std::string L = std::string(S.feat[i]) + "_box";
    if (i == 0) c->add_var(L + "/L2Normalization/gamma", {512});
    c->add_conv_vars(L + "/conv_loc", 3, S.feat_c[i], S.anchors[i] * 4);
    c->add_conv_vars(L + "/conv_cls", 3, S.feat_c[i], S.anchors[i] * c->cfg.num_classes);
  }
}

void declare_variables(ron_ctx* c) {
  for (const BodyConv& bc : vgg_body_convs()) c->add_conv_vars(bc.scope, 3, bc.cin, bc.cout);
  if (const SsdSpec* S = ssd_spec(c->cfg.variant)) declare_ssd_variables(c, *S);
  else declare_ron_variables(c);
}

// ---- step 2: the tensors, and with them the head layers' maps (feat_h / feat_w / feat_A) ------------------------------------
void declare_body_tensors(ron_ctx* c, const VggBody& body) {
  int h = c->cfg.img_h, w = c->cfg.img_w;
  c->add_tensor("im2col", h, w, conv_k_chunk(c->cfg.dtype), 0);
  for (const BodyConv& bc : vgg_body_convs()) {
    c->add_tensor(bc.name, h, w, bc.cout, bc.last && bc.block < 3 ? body.early_last_pad : 1);
    if (!bc.last) continue;
    const bool pool5 = bc.block == 4;
    if (!pool5 || body.pool5 == OP_POOL) { h = pool2_out(h); w = pool2_out(w); }
    c->add_tensor("pool" + std::to_string(bc.block + 1), h, w, bc.cout, pool5 ? body.pool5_pad : 1);
  }
}

void declare_ron_tensors(ron_ctx* c) {
  const int H = c->cfg.img_h, W = c->cfg.img_w, p5 = c->T("pool5"), h = c->tensors[p5].H, w = c->tensors[p5].W;
  c->add_tensor("fc6", h, w, c->c6, 1);
  c->add_tensor("fc7", h, w, c->c6, 0);
  for (int i = 0; i < 4; ++i) {
    const int s_h = (H / 64) << i, s_w = (W / 64) << i;
    c->add_feat(s_h, s_w, c->num_anchors);
    const std::string L = kFeatLayers[i];
    c->add_tensor(L + "_ref", s_h, s_w, 512, 1);
    c->add_tensor(L + "_hcat", s_h, s_w, 2048, 1);
    c->add_tensor(L + "_inc2", s_h, s_w, 1024, 1);
  }
}

void declare_ssd_tensors(ron_ctx* c, const SsdSpec& S) {
  const int b4 = c->T("conv4_3"), p5 = c->T("pool5");
  int h = c->tensors[p5].H, w = c->tensors[p5].W;
  c->has_obj = false;
  c->add_feat(c->tensors[b4].H, c->tensors[b4].W, S.anchors[0]);                              // block4 = conv4_3
  c->add_tensor("block4_norm", c->tensors[b4].H, c->tensors[b4].W, 512, 1);
  c->add_tensor("conv6", h, w, 1024, 0);
  c->add_tensor("conv7", h, w, 1024, 1);
  c->add_feat(h, w, S.anchors[1]);
  for (int b = 0; b < S.n_extra; ++b) {
    const SsdExtra& e = S.extra[b];
    c->add_tensor(ssd_block(b) + "_mid", h, w, e.mid, 1);             // pad2d(1) of the reference = the halo (unused by the VALID blocks)
    h = conv_out(h, e.k, e.stride, e.cpad); w = conv_out(w, e.k, e.stride, e.cpad);
    c->add_tensor(ssd_block(b), h, w, e.outc, 1);
    c->add_feat(h, w, S.anchors[2 + b]);
  }
}

void declare_tensors(ron_ctx* c) {
  declare_body_tensors(c, vgg_body(c));
  if (const SsdSpec* S = ssd_spec(c->cfg.variant)) declare_ssd_tensors(c, *S);
  else declare_ron_tensors(c);
}

// ---- step 3: device memory of the tensors a launch plan of this configuration touches ---------------------------------------
int allocate_tensors(ron_ctx* c) {
  const ron_config& cfg = c->cfg;
  for (auto& t : c->tensors) {
    if (t.name == "im2col" && stem_kernel(cfg)) continue;
    if ((t.name == "conv1_2" || t.name == "conv2_2" || t.name == "conv3_3") && pool_fused(cfg, t.H, t.W)) continue;
    if (t.name == "conv1_1" && stem2_fused(cfg)) continue;
    t.bytes = TensorView::halo_pixels(cfg.max_batch, t.H, t.W, t.pad) * t.cstride * c->esz();     // shared halos, conv_mfma.h
    if (t.bytes >= ((int64_t)1 << 32)) {
      ron::set_error("tensor %s needs %lld bytes for max_batch %d: above the 4 GiB buffer-addressing limit; lower max_batch",
                     t.name.c_str(), (long long)t.bytes, cfg.max_batch);
      return RON_ERR_INVALID;
    }
    RON_HIP_CHECK(ron::dev_malloc(t.d.put(), (size_t)t.bytes));
    RON_HIP_CHECK(ron::dev_memset(t.d, 0, (size_t)t.bytes));     // halos stay zero forever: kernels write interiors only
  }
  return RON_OK;
}

// ---- step 4: anchors of the head layers, on the device ---------------------------------------------------------------------
int make_anchors(ron_ctx* c) {
  const SsdSpec* S = ssd_spec(c->cfg.variant);
  const int H = c->cfg.img_h, W = c->cfg.img_w;
  for (int i = 0; i < c->n_feat; ++i) {
    const int fh = c->feat_h[i], fw = c->feat_w[i], A = c->feat_A[i];
    std::vector<float> y(fh * fw), x(fh * fw), hh(A), ww(A);
    const int rc = S ? ron_ssd_anchor_one_layer(H, W, fh, fw, S->sizes[i], 2, kSsdRatios, A - 2, S->steps[i], 0.5, y.data(), x.data(),
                                                hh.data(), ww.data())
                     : ron_anchor_one_layer(H, W, fh, fw, kRonAnchors.sizes[i], 2, kRonAnchors.ratios, 5, kRonAnchors.steps[i], 0.5,
                                            y.data(), x.data(), hh.data(), ww.data());
    if (rc) return rc;
    const std::vector<float>* src[4] = {&y, &x, &hh, &ww};
    for (int k = 0; k < 4; ++k) RON_HIP_CHECK(ron::dev_upload(&c->anchor[i][k], src[k]->data(), src[k]->size() * sizeof(float)));
  }
  return RON_OK;
}

// ---- weight assembly: fp32 rows [npad][K] + bias [npad] -----------------------------------
struct Rows {
  int K = 0, npad = 0, kh = 0, kw = 0, cin = 0;
  int cout = 0;                         // rows that are stored (<= npad)
  int split_n = 0, split_first = 0;     // pack_box_pair
  int64_t placed = 0;                   // weights of the variables placed here: the convolution's MACs per output pixel
  std::vector<float> w, b;
  Rows(int kh_, int kw_, int cin_, int n_real, int ntile) {
    kh = kh_; kw = kw_; cin = cin_; K = kh * kw * cin; cout = n_real; npad = round_up(n_real, ntile);
    w.assign((size_t)npad * K, 0.f);
    b.assign(npad, 0.f);
  }
  // place an HWIO filter (fh x fw, centred) at output rows [n_off, n_off + cout)
  void place(const Var& wv, int n_off) {
    const int fh = (int)wv.shape[0], fw = (int)wv.shape[1], ci = (int)wv.shape[2], co = (int)wv.shape[3];
    const int oy = (kh - fh) / 2, ox = (kw - fw) / 2;
    for (int y = 0; y < fh; ++y)
      for (int x = 0; x < fw; ++x)
        for (int c = 0; c < ci; ++c) {
          const float* src = &wv.data[(((size_t)y * fw + x) * ci + c) * co];
          const size_t k = ((size_t)(y + oy) * kw + (x + ox)) * cin + c;
          for (int n = 0; n < co; ++n) w[(size_t)(n_off + n) * K + k] = src[n];
        }
    placed += wv.numel();
  }
  void add_bias(const Var& bv, int n_off) { for (size_t n = 0; n < bv.data.size(); ++n) b[n_off + n] += bv.data[n]; }
  // y = gamma * (x - mean) / sqrt(var + eps) + beta  folded into rows [n_off, n_off + ch)
  void fold_bn(const ron_ctx* c, const std::string& scope, int n_off, int ch, int bn_off = 0) {
    const Var& be = c->var(scope + "/BatchNorm/beta"); const Var& ga = c->var(scope + "/BatchNorm/gamma");
    const Var& mu = c->var(scope + "/BatchNorm/moving_mean"); const Var& va = c->var(scope + "/BatchNorm/moving_variance");
    for (int n = 0; n < ch; ++n) {
      const int q = bn_off + n;
      const float s = ga.data[q] / sqrtf(va.data[q] + kBnEps);
      float* row = &w[(size_t)(n_off + n) * K];
      for (int k = 0; k < K; ++k) row[k] *= s;
      b[n_off + n] = (b[n_off + n] - mu.data[q]) * s + be.data[q];
    }
  }
  // a 512-channel branch of an inception block at rows [n_off, n_off + 512): conv + bias, then its channels [bn_off, bn_off + 512) of
  // the BatchNorm that follows the concat
  void place_branch(const ron_ctx* c, const std::string& conv, const std::string& bn, int n_off, int bn_off) {
    place(c->var(conv + "/weights"), n_off);
    add_bias(c->var(conv + "/biases"), n_off);
    fold_bn(c, bn, n_off, 512, bn_off);
  }
};

Rows pack_plain(const ron_ctx* c, const std::string& scope, bool bn) {
  const Var& w = c->var(scope + "/weights");
  const int cout = (int)w.shape[3];
  Rows r((int)w.shape[0], (int)w.shape[1], (int)w.shape[2], cout, conv_n_tile(cout));
  r.place(w, 0);
  if (bn) r.fold_bn(c, scope, 0, cout); else r.add_bias(c->var(scope + "/biases"), 0);
  return r;
}

// The class and box convolutions of an SSD feature layer (nets/ssd_vgg_300.py:403-431: both 3x3 over the same map) as ONE
// convolution: rows [0, A*classes) conv_cls, rows [split_n, split_n + 4A) conv_loc, split_n = A*classes rounded up to 8 (a lane's
// vector of adjacent channels then never straddles the two outputs).  The input is staged once instead of twice and the box
// columns ride in what would be padding of the class convolution's last column tile (block4: 84 + 16 -> 104 of 128 columns).
Rows pack_box_pair(const ron_ctx* c, const std::string& L) {
  const Var& wc = c->var(L + "/conv_cls/weights");
  const Var& wl = c->var(L + "/conv_loc/weights");
  const int n_cls = (int)wc.shape[3], n_loc = (int)wl.shape[3], split_n = round_up(n_cls, 8);
  Rows r((int)wc.shape[0], (int)wc.shape[1], (int)wc.shape[2], split_n + n_loc, conv_n_tile(split_n + n_loc));
  r.place(wc, 0);
  r.add_bias(c->var(L + "/conv_cls/biases"), 0);
  r.place(wl, split_n);
  r.add_bias(c->var(L + "/conv_loc/biases"), split_n);
  r.split_n = split_n; r.split_first = n_cls;
  return r;
}

// conv1_1 for the GEMM kernel (fp32 contexts): its 27 taps as the first elements of one K chunk of the im2col tensor
Rows pack_stem(const ron_ctx* c, const std::string& scope) {
  const Var& w = c->var(scope + "/weights");
  const int cout = (int)w.shape[3], chunk = conv_k_chunk(c->cfg.dtype);
  Rows r(1, 1, chunk, cout, conv_n_tile(cout));
  for (int k = 0; k < 27; ++k) for (int n = 0; n < cout; ++n) r.w[(size_t)n * chunk + k] = w.data[(size_t)k * cout + n];
  r.placed = w.numel();
  r.add_bias(c->var(scope + "/biases"), 0);
  return r;
}

Rows pack_deconv(const ron_ctx* c, const std::string& scope) {
  const Var& w = c->var(scope + "/weights");     // [kh, kw, Cout, Cin]
  const Var& bv = c->var(scope + "/biases");
  const int taps = (int)(w.shape[0] * w.shape[1]), co = (int)w.shape[2], ci = (int)w.shape[3];
  Rows r(1, 1, ci, taps * co, conv_n_tile(taps * co));
  memcpy(r.w.data(), w.data.data(), w.data.size() * sizeof(float));
  r.placed = w.numel();
  for (int t = 0; t < taps; ++t) for (int n = 0; n < co; ++n) r.b[t * co + n] = bv.data[n];
  return r;
}

// Everything that reads the reference map of a scale, as ONE convolution with 2048 outputs = the per-scale "hcat" tensor:
// rows 0..511 objectness hidden (3x3 conv + BN), 512..1023 box hidden (3x3 conv + BN), 1024..1535 inception-1 branch 0 (3x3 + bias,
// BN channels 0..511 of the concat), 1536..2047 inception-1 branch 1 (1x1 + bias, BN channels 512..1023) -- the 1x1 filter sits in
// the CENTRE tap of its rows and those column tiles run that tap's K steps only (ConvLaunch::center_from = 1536), so it costs
// its own MACs, not nine times them.
Rows pack_trio3(const ron_ctx* c, const std::string& L) {
  Rows r(3, 3, 512, 2048, 256);
  r.place(c->var(L + "_objectness/weights"), 0);
  r.fold_bn(c, L + "_objectness", 0, 512);
  r.place(c->var(L + "/Conv2d_0_3x3/weights"), 512);
  r.fold_bn(c, L + "/Conv2d_0_3x3", 512, 512);
  r.place_branch(c, L + "_inception1/Branch_0/Conv2d_3x3", L + "_inception1", 1024, 0);
  r.place_branch(c, L + "_inception1/Branch_1/Conv2d_1x1", L + "_inception1", 1536, 512);
  return r;
}

// Both branches of an "inception" block (nets/ron_vgg_320.py:378-397) as one convolution over the block's input: rows 0..511 the 3x3
// branch, 512..1023 the 1x1 branch in the centre tap (center_from = 512); each conv + bias, then its half of the BatchNorm that
// follows the concat, ReLU in the kernel epilogue.
Rows pack_inception(const ron_ctx* c, const std::string& I) {
  const Var& w3 = c->var(I + "/Branch_0/Conv2d_3x3/weights");
  Rows r(3, 3, (int)w3.shape[2], 1024, 256);
  r.place_branch(c, I + "/Branch_0/Conv2d_3x3", I, 0, 0);
  r.place_branch(c, I + "/Branch_1/Conv2d_1x1", I, 512, 512);
  return r;
}

// ---- the op list ------------------------------------------------------------------------------------------------------------
double conv_flops(int64_t weights, int out_pixels) { return 2.0 * (double)weights * out_pixels; }

Op conv_op(const std::string& name, int in, int out, int k, int cpad, int relu, int Ho, int Wo) {
  Op o;
  o.kind = OP_CONV; o.name = name; o.in = in; o.out = out;
  o.kh = o.kw = k; o.cpad = cpad; o.relu = relu; o.Ho = Ho; o.Wo = Wo;
  return o;
}
Op head_op(const std::string& name, int in, int layer, int kind, const ron_ctx* c) {      // 3x3 logits into the caller's buffer
  Op o = conv_op(name, in, -2, 3, 1, 0, c->feat_h[layer], c->feat_w[layer]);
  o.head_kind = kind; o.head_layer = layer;
  return o;
}

// Packs `r` for the kernels, uploads it and appends `o` as the convolution that runs it, credited with the MACs of the weights
// that were placed into `r`.
int add_conv(ron_ctx* c, Op o, const Rows& r) {
  PackedConv p;
  const std::vector<uint8_t> bytes = pack_conv_weights(r.w, r.npad, c->cfg.dtype, &p.oscale);
  p.w_bytes = (int64_t)bytes.size();
  p.Npad = r.npad; p.Cout = r.cout; p.split_n = r.split_n; p.split_first = r.split_first;
  RON_HIP_CHECK(ron::dev_upload(&p.w, bytes.data(), bytes.size()));
  if (conv_c64_wants_images(c->cfg.dtype, r.kh, r.kw, r.cin, r.cout, r.npad)) {
    const std::vector<uint8_t> img = pack_conv_c64_weights(r.w, r.npad, c->cfg.dtype);
    RON_HIP_CHECK(ron::dev_upload(&p.w_c64, img.data(), img.size()));
  }
  RON_HIP_CHECK(ron::dev_upload(&p.bias, r.b.data(), r.b.size() * sizeof(float)));
  c->own.packed.push_back(std::move(p));
  o.packed = (int)c->own.packed.size() - 1;
  o.flops = conv_flops(r.placed, o.Ho * o.Wo);
  c->ops.push_back(o);
  return RON_OK;
}

int upload_u16(DevBuf* b, const std::vector<uint16_t>& v) { RON_HIP_CHECK(ron::dev_upload(b, v.data(), v.size() * 2)); return RON_OK; }
int upload_bias64(DevBuf* b, const Var& v) { RON_HIP_CHECK(ron::dev_upload(b, v.data.data(), 64 * sizeof(float))); return RON_OK; }

int build_body(ron_ctx* c, const VggBody& body) {
  const ron_config& cfg = c->cfg;
  Weights& W = c->own;
  int rc, h = cfg.img_h, w = cfg.img_w, prev = c->T("im2col");
  if (!stem_kernel(cfg)) {
    Op o; o.kind = OP_IM2COL; o.name = "im2col"; o.out = prev;
    c->ops.push_back(o);
  }
  for (const BodyConv& bc : vgg_body_convs()) {
    const bool first = bc.cin == 3;
    if (first && stem_kernel(cfg)) {
      const Var& w1 = c->var(bc.scope + "/weights");
      std::vector<uint16_t> frags;
      if (cfg.dtype == RON_DTYPE_F16X3) W.stem_oscale = stem_pack_weights_split(w1.data.data(), &frags);
      else stem_pack_weights(w1.data.data(), cfg.dtype, &frags);
      if ((rc = upload_u16(&W.stem_w, frags)) || (rc = upload_bias64(&W.stem_b, c->var(bc.scope + "/biases")))) return rc;
      Op o; o.kind = OP_STEM; o.name = bc.name; o.out = c->T(bc.name);
      o.flops = conv_flops(w1.numel(), h * w);
      c->ops.push_back(o);
    } else if (first) {
      if ((rc = add_conv(c, conv_op(bc.name, prev, c->T(bc.name), 1, 0, 1, h, w), pack_stem(c, bc.scope)))) return rc;
    } else {
      if ((rc = add_conv(c, conv_op(bc.name, prev, c->T(bc.name), 3, 1, 1, h, w), pack_plain(c, bc.scope, false)))) return rc;
    }
    prev = c->T(bc.name);
    if (!bc.last) continue;
    const std::string pname = "pool" + std::to_string(bc.block + 1);
    const int pooled = c->T(pname);
    if (bc.block == 4 && body.pool5 == OP_POOL3) {
      Op p; p.kind = OP_POOL3; p.name = pname; p.in = prev; p.out = pooled;
      c->ops.push_back(p);
      continue;
    }
    if (bc.block < 3 && pool_fused(cfg, h, w)) {
      Op& conv = c->ops.back();
      conv.pool = 1;
      conv.out = pooled;
      conv.name += "+" + pname;
      if (bc.block == 0 && stem2_fused(cfg)) {
        // (the stand-alone stem kernel keeps its 32x32 fragments in stem_w; the fused kernel reads conv1_1 as 16x16x32 fragments)
        std::vector<uint16_t> img, w1;
        stem2_pack_weights(c->var("conv1/conv1_2/weights").data.data(), cfg.dtype, &img);
        stem2_pack_w1(c->var("conv1/conv1_1/weights").data.data(), cfg.dtype, &w1);
        if ((rc = upload_u16(&W.stem2_w, img)) || (rc = upload_bias64(&W.stem2_b, c->var("conv1/conv1_2/biases"))) ||
            (rc = upload_u16(&W.stem2_w1, w1))) return rc;
        Op f; f.kind = OP_STEM2; f.name = "conv1_1+conv1_2+pool1"; f.out = pooled;
        const size_t n_ops = c->ops.size();
        f.flops = c->ops[n_ops - 2].flops + c->ops[n_ops - 1].flops;
        c->ops.erase(c->ops.end() - 2, c->ops.end());
        c->ops.push_back(f);
      }
    } else {
      if ((cfg.flags & RON_CFG_FUSE_POOLS) && bc.block >= 3) c->ops.back().fuse_next_pool = 1;
      Op p; p.kind = OP_POOL; p.name = pname; p.in = prev; p.out = pooled;
      c->ops.push_back(p);
    }
    prev = pooled;
    h = pool2_out(h); w = pool2_out(w);
  }
  return RON_OK;
}

// fc6 / fc7, then the reverse connections + heads, coarse -> fine
int build_ron_tail(ron_ctx* c) {
  auto T = [&](const std::string& n) { return c->T(n); };
  const bool full = c->cfg.variant == RON_VARIANT_FULL;
  const int h = c->tensors[T("pool5")].H, w = c->tensors[T("pool5")].W;
  int rc;
  Op fc6 = conv_op("fc6", T("pool5"), T("fc6"), full ? 7 : 3, 3, 1, h, w);
  if (!full) fc6.dil = 3;
  if ((rc = add_conv(c, fc6, pack_plain(c, "fc6", false)))) return rc;
  if ((rc = add_conv(c, conv_op("fc7", T("fc6"), T("fc7"), 1, 0, 1, h, w), pack_plain(c, "fc7", false)))) return rc;
  const char* left_src[4] = {"fc7", "fc6", "conv5_3", "conv4_3"};
  for (int i = 0; i < 4; ++i) {
    const std::string Ln = kFeatLayers[i];
    const std::string L = "reverse_module/" + Ln + "_reverse";
    const int sh = c->feat_h[i], sw = c->feat_w[i], ref = T(Ln + "_ref"), hcat = T(Ln + "_hcat");
    // relu(relu(BN(conv_left(backbone map))) + relu(deconv_right(coarser reference map) + b))  (nets/ron_vgg_320.py:420-425).
    // The LEFT conv writes its half into the reference map's tensor first - it reads a backbone map only, so it is OFF the
    // coarse -> fine chain and free to be launched early / beside anything - and the transposed conv, the cheap one that IS on the
    // chain, adds its half in place (pixel-shuffle epilogue with the residual at the same address).  block7 has a left conv only
    // (2x2 stride 2 over fc7).
    Op left = conv_op(Ln + "_conv_left", T(left_src[i]), ref, i == 0 ? 2 : 3, i == 0 ? 0 : 1, 1, sh, sw);
    if (i == 0) left.stride = 2;
    if ((rc = add_conv(c, left, pack_plain(c, L + "_conv_left", true)))) return rc;
    if (i > 0) {
      Op d = conv_op(Ln + "_deconv_right", T(std::string(kFeatLayers[i - 1]) + "_ref"), ref, 1, 0, 1, sh / 2, sw / 2);
      d.up = 2; d.up_cout = 512;
      d.res = ref;                            // in place: ref = relu(left + up)
      if ((rc = add_conv(c, d, pack_deconv(c, L + "_deconv_right")))) return rc;
    }
    // hcat channels: [0,512) objectness hidden | [512,1024) box hidden | [1024,1536) inception-1 3x3 | [1536,2048) inception-1 1x1
    Op trio = conv_op(Ln + "_trio3", ref, hcat, 3, 1, 1, sh, sw);
    trio.center_from = 1536;
    if ((rc = add_conv(c, trio, pack_trio3(c, L)))) return rc;
    Op obj = head_op(Ln + "_objectness_score", hcat, i, 1, c);
    obj.in_coff = 0; obj.in_C = 512;
    if ((rc = add_conv(c, obj, pack_plain(c, L + "_objectness_score", false)))) return rc;
    Op inc2 = conv_op(Ln + "_inception2", hcat, T(Ln + "_inc2"), 3, 1, 1, sh, sw);
    inc2.in_coff = 1024; inc2.in_C = 1024; inc2.center_from = 512;
    if ((rc = add_conv(c, inc2, pack_inception(c, L + "_inception2")))) return rc;
    if ((rc = add_conv(c, head_op(Ln + "_cls_pred", T(Ln + "_inc2"), i, 0, c), pack_plain(c, L + "_inception2/Conv2d_pred_3x3", false)))) return rc;
    Op loc = head_op(Ln + "_loc_pred", hcat, i, 2, c);
    loc.in_coff = 512; loc.in_C = 512;
    if ((rc = add_conv(c, loc, pack_plain(c, L + "/Conv2d_1_3x3", false)))) return rc;
  }
  return RON_OK;
}

// conv6 (3x3 rate 6), conv7 (1x1), the extra blocks (1x1, then SsdExtra: pad 1 + 3x3 stride 2 / pad 1 + 4x4 / 3x3 VALID), then the
// multibox heads (nets/ssd_vgg_300.py:403-431)
int build_ssd_tail(ron_ctx* c, const SsdSpec& S) {
  auto T = [&](const std::string& n) { return c->T(n); };
  int h = c->tensors[T("pool5")].H, w = c->tensors[T("pool5")].W, rc;
  Op conv6 = conv_op("conv6", T("pool5"), T("conv6"), 3, 6, 1, h, w);
  conv6.dil = 6;
  if ((rc = add_conv(c, conv6, pack_plain(c, "conv6", false)))) return rc;
  if ((rc = add_conv(c, conv_op("conv7", T("conv6"), T("conv7"), 1, 0, 1, h, w), pack_plain(c, "conv7", false)))) return rc;
  int src = T("conv7");
  for (int b = 0; b < S.n_extra; ++b) {
    const SsdExtra& e = S.extra[b];
    const std::string B = ssd_block(b), kxk = ssd_extra_conv(e);
    if ((rc = add_conv(c, conv_op(B + "_conv1x1", src, T(B + "_mid"), 1, 0, 1, h, w), pack_plain(c, B + "/conv1x1", false)))) return rc;
    h = conv_out(h, e.k, e.stride, e.cpad); w = conv_out(w, e.k, e.stride, e.cpad);
    Op o = conv_op(B + "_" + kxk, T(B + "_mid"), T(B), e.k, e.cpad, 1, h, w);
    o.stride = e.stride;
    if ((rc = add_conv(c, o, pack_plain(c, B + "/" + kxk, false)))) return rc;
    src = T(B);
  }
  const Var& g = c->var("block4_box/L2Normalization/gamma");
  RON_HIP_CHECK(ron::dev_upload(&c->own.l2_gamma, g.data.data(), g.data.size() * sizeof(float)));
  Op norm; norm.kind = OP_L2NORM; norm.name = "block4_l2norm"; norm.in = T("conv4_3"); norm.out = T("block4_norm");
  c->ops.push_back(norm);
  for (int i = 0; i < S.n_feat; ++i) {
    const std::string L = std::string(S.feat[i]) + "_box";
    const int feat = T(i == 0 ? "block4_norm" : (i == 1 ? "conv7" : S.feat[i]));
    if (i < kSsdPairedHeads) {
      // the two large maps: loc and cls as one launch with two outputs (pack_box_pair)
      Op o = head_op(L + "_conv_cls_loc", feat, i, 0, c);
      o.head_kind2 = 2;
      if ((rc = add_conv(c, o, pack_box_pair(c, L)))) return rc;
      continue;
    }
    if ((rc = add_conv(c, head_op(L + "_conv_loc", feat, i, 2, c), pack_plain(c, L + "/conv_loc", false)))) return rc;
    if ((rc = add_conv(c, head_op(L + "_conv_cls", feat, i, 0, c), pack_plain(c, L + "/conv_cls", false)))) return rc;
  }
  return RON_OK;
}

// Launch order of the heads with the small convolutions grouped (launch_conv_group).  The reference builds the scales one after the
// other (nets/ron_vgg_320.py:495-506); the true dependencies are listed at the RON tables below.  Every braced set only reads what
// earlier entries wrote, and its members write disjoint tensors / channel slices.  History of the measurements behind the plans:
// HISTORY.md (rounds 2-3: T64 / T128 groups by dependency level) and DESIGN.md 3.2 (round 4: mixed-width groups with carriers).
struct Slot { int cfg; std::vector<std::string> names; };     // cfg < 0: launches of their own

// The plan of this context: the SSD table built from the variant's description, or one of the three RON tables.
std::vector<Slot> head_plan(const ron_ctx* c) {
  const int T64 = kCfgIgemm128x64;     // tiny convolutions (Npad = 64)
  // SSD-512 (nets/ssd_vgg_512.py:395-458): blocks 8-12 are a chain of 1x1 -> 3x3 stride-2 convolutions on 16x16 ... 1x1 maps,
  // each a 13-20 us launch at batch 16; the two box convolutions of a block only need that block's output, so they share a
  // launch with the next block's 1x1 (20 small launches -> 11).  The block4 / block7 heads are real work and stay alone (round 4:
  // as carriers of the chain's small launches in mixed-width groups they measured -0.8 % images/s - block4_box_conv_loc then leaves
  // the halo-patch kernel: 114 us for {block8_conv1x1, block4_box_conv_loc} where the two take 40 + 45 us on their own).
  // SSD-300 has the same chain on 19x19 ... 1x1 maps, one block shorter (16 small launches -> 9).
  if (const SsdSpec* S = ssd_spec(c->cfg.variant)) {
    std::vector<Slot> ssd_order = {{-1, {"conv6"}}, {-1, {"conv7"}}, {-1, {"block8_conv1x1"}}};
    for (int b = 0; b < S->n_extra; ++b) {
      const std::string B = ssd_block(b);
      ssd_order.push_back({-1, {B + "_" + ssd_extra_conv(S->extra[b])}});
      Slot g{T64, {B + "_box_conv_loc", B + "_box_conv_cls"}};
      if (b + 1 < S->n_extra) g.names.push_back(ssd_block(b + 1) + "_conv1x1");
      ssd_order.push_back(g);
    }
    ssd_order.push_back({-1, {"block4_l2norm"}});
    for (int i = 0; i < kSsdPairedHeads; ++i) ssd_order.push_back({-1, {std::string(S->feat[i]) + "_box_conv_cls_loc"}});
    return ssd_order;
  }
  // RON heads.  Dependencies after the round-4 re-formulation of the reverse connection (the LEFT conv of a scale reads a backbone
  // map only; the transposed conv adds its half in place, build_ron_tail):
  //   conv_left(i)                       <- backbone (fc7 / fc6 / conv5_3 / conv4_3)        i = block7, 6, 5, 4
  //   deconv_right(i) -> ref(i)          <- ref(i-1), conv_left(i)
  //   trio3(i) -> hcat(i)                <- ref(i)
  //   {objectness_score, inception2, loc_pred}(i) <- hcat(i);   cls_pred(i) <- inception2(i)
  // so the coarse -> fine chain is ref7 -> deconv6 -> deconv5 -> deconv4 (three small GEMMs), and a dependency LEVEL is
  // {cls_pred(i-2), obj / inc2 / loc(i-1), trio3(i), deconv_right(i+1)}.  MIX = one launch of the row-gather kernel with the tile width
  // chosen per member (kGroupMixed): the latency-bound launches of the 5x5 / 10x10 scales (M = 800 / 3200 rows at batch 32: 18-50 us
  // apiece, mostly pipeline fill and split-K hand-off) ride in the partial rounds of the level's large member.  The members that are
  // several full rounds of 256 x 256 tiles on their own (block4: conv_left, trio3, inception2, cls_pred) keep launches of their own.
  const int MIX = kGroupMixed;
  // Batch plan.  G256 = one launch of 256 x 256 tiles (launch_conv_group, kCfgIgemm256): a member that is several rounds of the chip
  // on its own ends with a partial round (400 tiles = 1.56 rounds, 1200 = 4.69), and the members beside it - whose tiles have the same
  // or twice the K length - are dispatched into it (longest chains first); everything here has Npad % 256 == 0.  The skinny heads
  // (Npad = 64) cannot ride on 256-wide tiles: the ones of the three coarse scales share one mixed-width launch.
  const int G256 = kCfgIgemm256;
  const std::vector<Slot> ron_order = {
      // the left conv of block4 reads conv4_3 only: its 400 tiles (1.56 rounds) carry conv5_1's 100 (0.39 of a round on its own)
      {G256, {"conv5_1", "block4_conv_left"}},
      {-1, {"conv5_2"}}, {-1, {"conv5_3"}}, {-1, {"pool5"}}, {-1, {"fc6"}},
      // fc7 (208 tiles) and the left conv of block6 (26 tiles x 576 K steps: split-K) both read fc6 and are each short of one round.
      // (The left conv of block5 on the 48 CUs fc6 leaves idle - {fc6, block5_conv_left} - measured 531 us for the pair where fc6 alone
      // takes 513: -42 us per step with one batch in flight, but -0.85 % images/s with two, where the other batch uses those CUs.)
      {G256, {"fc7", "block6_conv_left"}},
      {MIX, {"block7_conv_left", "block5_conv_left"}},
      {MIX, {"block7_trio3", "block6_deconv_right"}},
      {MIX, {"block6_trio3", "block7_inception2", "block5_deconv_right"}},
      {G256, {"block5_trio3", "block6_inception2", "block7_cls_pred", "block4_deconv_right"}},
      {MIX, {"block7_objectness_score", "block7_loc_pred", "block6_objectness_score", "block6_loc_pred", "block5_objectness_score",
             "block5_loc_pred"}},
      {G256, {"block4_trio3", "block5_inception2", "block6_cls_pred"}},
      // Cout = 20 / 40 over channel slices of the same tensor: one launch of the halo-patch kernel (400 workgroups; 200 each alone)
      {kCfgPatch64, {"block4_objectness_score", "block4_loc_pred"}},
      {G256, {"block4_inception2", "block5_cls_pred"}},
      {-1, {"block4_cls_pred"}},
  };
  // Medium batches (max_batch kLevelPlanMaxBatch + 1 .. kCarrierPlanMinBatch - 1): the large members are not several rounds of 256 x 256 tiles there, so a
  // dependency level is one mixed-width launch (128-row tiles), the free left convs being the carriers of the first levels
  // (batch 8 / 16, one in flight: 2.02 -> 1.94 ms, 3.18 -> 3.08 ms; the 256 x 256 groups above measured 2.08 / 3.23 there).
  const std::vector<Slot> ron_mid = {
      {G256, {"fc7", "block6_conv_left"}},
      {MIX, {"block7_conv_left", "block5_conv_left"}},
      {MIX, {"block7_trio3", "block6_deconv_right"}},
      {MIX, {"block7_objectness_score", "block7_inception2", "block7_loc_pred", "block6_trio3", "block5_deconv_right"}},
      {-1, {"block4_conv_left"}},
      {MIX, {"block7_cls_pred", "block6_objectness_score", "block6_inception2", "block6_loc_pred", "block5_trio3", "block4_deconv_right"}},
      {MIX, {"block6_cls_pred", "block5_objectness_score", "block5_loc_pred", "block5_inception2"}},
      {-1, {"block4_trio3"}},
      {-1, {"block5_cls_pred"}},
      {kCfgPatch64, {"block4_objectness_score", "block4_loc_pred"}},
      {-1, {"block4_inception2"}},
      {-1, {"block4_cls_pred"}},
  };
  // Small batches (RON_CFG_LEVEL_GROUPS, the default when max_batch <= kLevelPlanMaxBatch): every head convolution is a
  // latency-bound launch of a few hundred workgroups (25-40 us each with its split-K finalize, whatever its size), so
  // the heads go out one launch per dependency level, the large convolutions included: 16 head launches -> 7.  Since the left
  // convs left the chain (round 4) this wins up to batch 12 with one or two batches in flight (batch 8: 1.76 vs 1.91 ms, batch 12:
  // 2.44 vs 2.64 ms); from 16 on two batches in flight prefer the plans above (2.47 vs 2.56 ms), one in flight still this one.
  const std::vector<Slot> ron_levels = {
      {MIX, {"block7_conv_left", "block6_conv_left", "block5_conv_left", "block4_conv_left"}},
      {MIX, {"block7_trio3", "block6_deconv_right"}},
      {MIX, {"block7_objectness_score", "block7_inception2", "block7_loc_pred", "block6_trio3", "block5_deconv_right"}},
      {MIX, {"block7_cls_pred", "block6_objectness_score", "block6_inception2", "block6_loc_pred", "block5_trio3", "block4_deconv_right"}},
      {MIX, {"block6_cls_pred", "block5_objectness_score", "block5_inception2", "block5_loc_pred", "block4_trio3"}},
      {MIX, {"block5_cls_pred", "block4_objectness_score", "block4_inception2", "block4_loc_pred"}},
      {-1, {"block4_cls_pred"}},
  };
  const bool levels = !(c->cfg.flags & RON_CFG_BATCH_GROUPS) &&
                      ((c->cfg.flags & RON_CFG_LEVEL_GROUPS) || c->cfg.max_batch <= kLevelPlanMaxBatch);
  return levels ? ron_levels : (c->cfg.max_batch >= kCarrierPlanMinBatch ? ron_order : ron_mid);
}

// Reorders the tail of the op list as `order` says and marks the grouped launches.
void plan_groups(ron_ctx* c, const std::vector<Slot>& order) {
  std::map<std::string, int> at;
  for (size_t i = 0; i < c->ops.size(); ++i) at[c->ops[i].name] = (int)i;
  size_t first_head = c->ops.size(), n_named = 0;
  for (const Slot& s : order)
    for (const std::string& nm : s.names) {
      auto it = at.find(nm);
      if (it == at.end()) {                               // not the graph this plan was written for: keep the plain order, loudly
        fprintf(stderr, "libron_hip: grouped launch plan names op '%s' which the graph does not have: one launch per convolution\n", nm.c_str());
        return;
      }
      first_head = std::min(first_head, (size_t)it->second);
      ++n_named;
    }
  if (first_head + n_named != c->ops.size()) {            // the heads must be exactly the tail of the op list
    fprintf(stderr, "libron_hip: grouped launch plan covers %zu ops, the graph has %zu after '%s': one launch per convolution\n",
            n_named, c->ops.size() - first_head, c->ops[first_head].name.c_str());
    return;
  }
  std::vector<Op> planned(c->ops.begin(), c->ops.begin() + first_head);
  int gid = 0;
  for (const Slot& s : order) {
    for (const std::string& nm : s.names) {
      Op o = c->ops[at[nm]];
      if (s.cfg >= 0) { o.group = gid; o.group_cfg = s.cfg; }
      planned.push_back(o);
    }
    if (s.cfg >= 0) ++gid;
  }
  c->grouped_launches = gid;
  c->ops.swap(planned);
}

}  // namespace

// ------------------------------------------------------------------------------------------
extern "C" int ron_create(ron_ctx** out, const ron_config* cfg) {
  RON_REQUIRE(out && cfg, "NULL argument");
  RON_REQUIRE(cfg->variant >= RON_VARIANT_REDUCEDFC && cfg->variant <= RON_VARIANT_SSD300, "unknown variant %d", cfg->variant);
  RON_REQUIRE(cfg->dtype >= 0 && cfg->dtype <= RON_DTYPE_F16X3, "unknown dtype %d", cfg->dtype);
  if (const SsdSpec* S = ssd_spec(cfg->variant))
    RON_REQUIRE(cfg->img_h == S->img && cfg->img_w == S->img, "SSD-%d runs on %d x %d inputs", S->img, S->img, S->img);
  else
    RON_REQUIRE(cfg->img_h > 0 && cfg->img_h % 64 == 0 && cfg->img_w > 0 && cfg->img_w % 64 == 0, "image size must be a multiple of 64");
  RON_REQUIRE(cfg->num_classes >= 2 && cfg->num_classes <= RON_MAX_CLASSES, "num_classes %d out of range [2, %d]", cfg->num_classes, RON_MAX_CLASSES);
  RON_REQUIRE(cfg->max_batch >= 1, "max_batch must be >= 1");
  RON_HIP_CHECK(ron::dev_set_device(cfg->device));
  std::unique_ptr<ron_ctx> c(new ron_ctx());     // (a failure below frees what was allocated so far: every buffer has an owner)
  c->cfg = *cfg;
  c->c6 = cfg->variant == RON_VARIANT_FULL ? 4096 : 1024;
  declare_variables(c.get());
  declare_tensors(c.get());
  int rc = allocate_tensors(c.get());
  if (rc == RON_OK) rc = make_anchors(c.get());
  if (rc == RON_OK) *out = c.release();
  return rc;
}

extern "C" int ron_destroy(ron_ctx* c) {
  if (!c) return RON_OK;
  if (c->clones > 0) { ron::set_error("ron_destroy: %d execution slot(s) still borrow this context's weights", c->clones); return RON_ERR_STATE; }
  if (c->weights_owner != nullptr) --c->weights_owner->clones;
  delete c;
  return RON_OK;
}

extern "C" int ron_num_variables(const ron_ctx* c) { return c ? (int)c->vars.size() : RON_ERR_INVALID; }

extern "C" int ron_variable_info(const ron_ctx* c, int i, const char** name, int64_t shape[4], int* ndim) {
  RON_REQUIRE(c && i >= 0 && i < (int)c->vars.size(), "variable index out of range");
  if (name) *name = c->vars[i].name.c_str();
  if (ndim) *ndim = (int)c->vars[i].shape.size();
  if (shape) for (size_t k = 0; k < c->vars[i].shape.size(); ++k) shape[k] = c->vars[i].shape[k];
  return RON_OK;
}

extern "C" int ron_load_weight(ron_ctx* c, const char* tf_name, const float* host_ptr, const int64_t* shape, int ndim) {
  RON_REQUIRE(c && tf_name && host_ptr && shape, "NULL argument");
  if (c->finalized) { ron::set_error("weights are already finalized"); return RON_ERR_STATE; }
  auto it = c->var_index.find(tf_name);
  if (it == c->var_index.end()) { ron::set_error("unknown variable '%s'", tf_name); return RON_ERR_UNKNOWN_NAME; }
  Var& v = c->vars[it->second];
  bool same = ndim == (int)v.shape.size();
  for (int k = 0; same && k < ndim; ++k) same = shape[k] == v.shape[k];
  if (!same) { ron::set_error("variable '%s': shape mismatch", tf_name); return RON_ERR_INVALID; }
  v.data.assign(host_ptr, host_ptr + v.numel());
  v.loaded = true;
  return RON_OK;
}

static int slot_resources(ron_ctx* c);

extern "C" int ron_finalize_weights(ron_ctx* c) {
  RON_REQUIRE(c, "NULL ctx");
  if (c->finalized) { ron::set_error("weights are already finalized"); return RON_ERR_STATE; }
  for (auto& v : c->vars)
    if (!v.loaded) { ron::set_error("variable '%s' was not loaded", v.name.c_str()); return RON_ERR_STATE; }
  RON_HIP_CHECK(ron::dev_set_device(c->cfg.device));
  const SsdSpec* ssd = ssd_spec(c->cfg.variant);
  int rc = build_body(c, vgg_body(c));
  if (rc == RON_OK) rc = ssd ? build_ssd_tail(c, *ssd) : build_ron_tail(c);
  if (rc) return rc;
  for (const Op& o : c->ops) c->flops_per_image += o.flops;
  if (!(c->cfg.flags & (RON_CFG_MULTI_STREAM | RON_CFG_NO_GROUPS))) plan_groups(c, head_plan(c));
  // stream lanes: heads of block7 / block6 / block5 are independent of the main chain once their reference map exists
  if ((c->cfg.flags & RON_CFG_MULTI_STREAM) && !ssd) {
    for (Op& o : c->ops)
      for (int i = 0; i < 3; ++i) {
        const std::string pre = std::string(kFeatLayers[i]) + "_";
        if (o.name.compare(0, pre.size(), pre) == 0 && o.name.find("_conv_left") == std::string::npos &&
            o.name.find("_deconv_right") == std::string::npos)
          o.lane = i + 1;
      }
  }
  for (Op& o : c->ops) {
    if (o.kind != OP_CONV) continue;
    const PackedConv& pk = c->own.packed[o.packed];
    const Tensor& ti = c->tensors[o.in];
    const int cin = o.in_C > 0 ? o.in_C : ti.C;
    const double out_esz = o.out == -2 ? 4.0 : (double)c->esz();
    const int os = o.up > 0 ? o.up * o.up : 1;
    const double out_px = o.pool ? (double)pool2_out(o.Ho) * pool2_out(o.Wo) : (double)o.Ho * o.Wo * os;
    const double out_ch = o.up > 0 ? (double)o.up_cout : (double)(pk.Cout - (pk.split_n - pk.split_first));
    o.act_bytes = (double)ti.H * ti.W * cin * c->esz() + out_px * out_ch * out_esz + (o.res >= 0 ? out_px * out_ch * c->esz() : 0.0);
    o.wgt_bytes = (double)pk.w_bytes;
  }
  for (auto& v : c->vars) { v.data.clear(); v.data.shrink_to_fit(); }
  if ((rc = slot_resources(c))) return rc;
  c->finalized = true;
  return RON_OK;
}

// The dense fp32 tensor of one head output (kind 0 cls, 1 obj, 2 loc) of `o`'s layer in the caller's buffers (heads == nullptr:
// geometry only, base null).
static int head_view(const ron_ctx* c, const Op& o, int kind, int n, const ron_heads* heads, TensorView* out_v) {
  float* dst = nullptr;
  if (heads != nullptr) {
    const float* const* arr = kind == 0 ? heads->cls : (kind == 1 ? heads->obj : heads->loc);
    dst = const_cast<float*>(arr[o.head_layer]);
    RON_REQUIRE(dst != nullptr, "ron_forward: head buffer (kind %d, layer %d) is NULL", kind, o.head_layer);
  }
  TensorView v;
  const int A = c->feat_A[o.head_layer];
  v.base = dst; v.N = n; v.H = o.Ho; v.W = o.Wo; v.pad = 0; v.coff = 0;
  v.C = kind == 0 ? A * c->cfg.num_classes : (kind == 1 ? 2 * A : 4 * A);
  v.cstride = v.C;
  v.bytes = (int64_t)n * v.H * v.W * v.C * 4;
  *out_v = v;
  return RON_OK;
}

// The launch description of conv op `o` at batch n (heads == nullptr: geometry only, for sizing).
static int describe_conv(const ron_ctx* c, const Op& o, int n, const ron_heads* heads, ConvLaunch* out_l) {
  const PackedConv& p = c->wts->packed[o.packed];
  ConvLaunch L;
  int rc;
  L.dtype = c->cfg.dtype;
  L.in = c->view(o.in, n, o.in_coff, o.in_C > 0 ? o.in_C : -1);
  if (o.out == -2) {
    if ((rc = head_view(c, o, o.head_kind, n, heads, &L.out))) return rc;
    L.out_f32 = 1;
    if (o.head_kind2 >= 0) {
      // second head output of the launch (pack_box_pair): dense like the first
      if ((rc = head_view(c, o, o.head_kind2, n, heads, &L.out2))) return rc;
      if (L.out2.base == nullptr) L.out2.base = reinterpret_cast<float*>(16);        // (geometry only: any non-null address)
      L.split_n = p.split_n; L.split_first = p.split_first;
    }
  } else {
    L.out = c->view(o.out, n);
  }
  L.res = o.res >= 0 ? c->tensors[o.res].d.p : nullptr;
  L.wgt = p.w; L.wgt_bytes = p.w_bytes; L.wgt_c64 = p.w_c64; L.bias = p.bias.as<float>(); L.oscale = p.oscale; L.Cout = p.Cout; L.Npad = p.Npad;
  L.kh = o.kh; L.kw = o.kw; L.stride = o.stride; L.dil = o.dil; L.cpad = o.cpad; L.relu = o.relu;
  L.up = o.up; L.up_cout = o.up_cout; L.Ho = o.Ho; L.Wo = o.Wo; L.pool = o.pool;
  L.center_from = o.center_from;
  L.scratch = c->splitk[o.lane]; L.scratch_bytes = c->splitk_bytes[o.lane];
  L.halo_skip = (c->cfg.flags & RON_CFG_NO_HALO_SKIP) ? 0 : 1;
  *out_l = L;
  return RON_OK;
}

// The members of the launch that starts at op `oi`, at batch n: the op itself, or it and the following ops of its group.
static int gather_launch(const ron_ctx* c, size_t oi, int n, const ron_heads* heads, ConvLaunch* L, int* members) {
  const Op& o = c->ops[oi];
  int m = 0;
  do {
    RON_REQUIRE(m < kMaxConvGroup, "conv group %d has more than %d members", o.group, kMaxConvGroup);
    if (const int rc = describe_conv(c, c->ops[oi + m], n, heads, &L[m])) return rc;
    ++m;
  } while (o.group >= 0 && oi + m < c->ops.size() && c->ops[oi + m].group == o.group);
  *members = m;
  return RON_OK;
}

// the context's own head buffers, as ron_detect hands them to the forward pass and the post-processing
static void own_heads(const ron_ctx* c, ron_heads* hd) {
  for (int i = 0; i < c->n_feat; ++i) {
    hd->cls[i] = c->head[0][i].as<float>(); hd->obj[i] = c->head[1][i].as<float>(); hd->loc[i] = c->head[2][i].as<float>();
  }
}

// Streams, events, split-K scratch and timing slots of one execution slot (after c->ops / c->wts are in place).
static int slot_resources(ron_ctx* c) {
  if ((c->cfg.flags & RON_CFG_MULTI_STREAM) && !c->is_ssd()) {
    for (int l = 1; l < 4; ++l) {
      RON_HIP_CHECK(hipStreamCreateWithFlags(c->side[l].put(), hipStreamNonBlocking));
      RON_HIP_CHECK(hipEventCreateWithFlags(c->lane_ready[l].put(), hipEventDisableTiming));
      RON_HIP_CHECK(hipEventCreateWithFlags(c->lane_done[l].put(), hipEventDisableTiming));
    }
  }
  // The launch plans of every batch size, and with them the split-K scratch: the largest slab set any launch (or grouped launch) of
  // a lane can ask for.  A clone takes both from the slot it was cloned from (the schedule model costs ~1 ms per (group, batch)).
  if (const ron_ctx* from = c->weights_owner) {
    c->launch_plans = from->launch_plans;
    for (int l = 0; l < 4; ++l) c->splitk_bytes[l] = from->splitk_bytes[l];
  } else {
    c->launch_plans.assign(c->cfg.max_batch + 1, std::vector<ron_ctx::LaunchPlan>(c->ops.size()));
    int members = 1;
    for (size_t i = 0; i < c->ops.size(); i += members) {
      const Op& o = c->ops[i];
      members = 1;
      if (o.kind != OP_CONV || (o.group < 0 && o.up > 0)) continue;
      const bool pool_follows = o.fuse_next_pool && i + 1 < c->ops.size() && c->ops[i + 1].kind == OP_POOL;
      for (int nb = 1; nb <= c->cfg.max_batch; ++nb) {
        ConvLaunch L[kMaxConvGroup];
        if (const int rc = gather_launch(c, i, nb, nullptr, L, &members)) return rc;
        ron_ctx::LaunchPlan& plan = c->launch_plans[nb][i];
        int64_t b;
        if (o.group >= 0) {
          // the plan ron_forward will launch with, and its scratch, from ONE run of the model
          conv_group_plan(L, members, o.group_cfg, plan.sk.data());
          b = conv_group_scratch_bytes(L, members, o.group_cfg, plan.sk.data());
        } else {
          b = conv_scratch_bytes(L[0]);
          if (pool_follows) {
            // conv4_3 / conv5_3: both the map and its pool are read later.  When the launch does not split K (it does at small
            // batches: the pool epilogue needs whole sums) the pool comes out of the same accumulators and the pool launch is skipped.
            // (The pool inside the split-K finalize pass instead was measured at batch 1: conv4_3 30.9 + pool4 8.7 us -> 40.9 us, no gain.)
            ConvLaunch F = L[0];
            F.out2 = L[0].out;                           // the kernel choice of a two-output launch (row-gather kernel only) ...
            plan.fuse_pool = conv_scratch_bytes(F) == 0;      // ... would not split K at this batch
          }
        }
        if (b > c->splitk_bytes[o.lane]) c->splitk_bytes[o.lane] = b;
      }
    }
  }
  for (int l = 0; l < 4; ++l)
    if (c->splitk_bytes[l] > 0) RON_HIP_CHECK(ron::dev_malloc(c->splitk[l].put(), (size_t)c->splitk_bytes[l]));
  // ron_detect's head buffers and post-processing workspace, for max_batch: allocated (and the workspace zeroed) here, so that the
  // first ron_detect is as free of host synchronisation as every later one (include/ron_hip.h, Ownership)
  const int mb = c->cfg.max_batch;
  for (int i = 0; i < c->n_feat; ++i) {
    const int A = c->feat_A[i];
    const size_t cells = (size_t)mb * c->feat_h[i] * c->feat_w[i];
    RON_HIP_CHECK(ron::dev_malloc(c->head[0][i].put(), cells * A * c->cfg.num_classes * sizeof(float)));
    if (c->has_obj) RON_HIP_CHECK(ron::dev_malloc(c->head[1][i].put(), cells * A * 2 * sizeof(float)));
    RON_HIP_CHECK(ron::dev_malloc(c->head[2][i].put(), cells * A * 4 * sizeof(float)));
  }
  ron_heads hd;
  memset(&hd, 0, sizeof(hd));
  int rc = ron_heads_describe(c, &hd);
  if (rc) return rc;
  own_heads(c, &hd);
  c->post_ws_bytes = ron_post_np_workspace_bytes(&hd, mb);
  if (c->post_ws_bytes <= 0) return RON_ERR_INVALID;      // (ron_last_error says why)
  RON_HIP_CHECK(ron::dev_malloc(c->post_ws.put(), (size_t)c->post_ws_bytes));
  RON_HIP_CHECK(ron::dev_memset(c->post_ws, 0, (size_t)c->post_ws_bytes));      // once: the kernels keep the counters clean
  c->timing.assign(c->ops.size() + 1, OpTiming());
  // names ron_profile_get hands out: a grouped launch is reported on its first member as "group[first+N]", the other members as
  // "(name)"; built once so that the pointers stay valid until ron_destroy
  c->labels.assign(c->ops.size() + 1, std::string());
  for (size_t i = 0; i < c->ops.size(); ++i) {
    const Op& o = c->ops[i];
    const bool member = o.group >= 0 && i > 0 && c->ops[i - 1].group == o.group;
    if (member) { c->labels[i] = "(" + o.name + ")"; continue; }
    int extra = 0;
    for (size_t j = i + 1; o.group >= 0 && j < c->ops.size() && c->ops[j].group == o.group; ++j) ++extra;
    c->labels[i] = extra > 0 ? "group[" + o.name + "+" + std::to_string(extra) + "]" : o.name;
  }
  c->labels[c->ops.size()] = "post_np";
  return RON_OK;
}

// A second execution slot over the same weights: own activations, head buffers, scratch and streams, so that two
// (or more) batches can be in flight on different streams; the packed weights stay with `src`.
extern "C" int ron_clone(ron_ctx* src, ron_ctx** out) {
  RON_REQUIRE(src && out, "NULL argument");
  if (!src->finalized) { ron::set_error("ron_clone before ron_finalize_weights"); return RON_ERR_STATE; }
  ron_ctx* owner = src->weights_owner ? src->weights_owner : src;
  ron_ctx* c = nullptr;
  int rc = ron_create(&c, &src->cfg);
  if (rc) return rc;
  c->wts = &owner->own;
  c->ops = owner->ops;
  c->flops_per_image = owner->flops_per_image;
  c->grouped_launches = owner->grouped_launches;
  c->weights_owner = owner;
  ++owner->clones;
  for (auto& v : c->vars) v.loaded = true;
  if ((rc = slot_resources(c))) { (void)ron_destroy(c); return rc; }
  c->finalized = true;
  *out = c;
  return RON_OK;
}

extern "C" double ron_flops_per_image(const ron_ctx* c) { return c ? c->flops_per_image : -1.0; }

extern "C" int ron_heads_describe(const ron_ctx* c, ron_heads* hd) {
  RON_REQUIRE(c && hd, "NULL argument");
  hd->num_layers = c->n_feat;
  hd->num_classes = c->cfg.num_classes;
  for (int i = 0; i < c->n_feat; ++i) {
    hd->feat_h[i] = c->feat_h[i];
    hd->feat_w[i] = c->feat_w[i];
    hd->num_anchors[i] = c->feat_A[i];
    hd->anchor_y[i] = c->anchor[i][0].as<float>(); hd->anchor_x[i] = c->anchor[i][1].as<float>();
    hd->anchor_h[i] = c->anchor[i][2].as<float>(); hd->anchor_w[i] = c->anchor[i][3].as<float>();
    if (!c->has_obj) hd->obj[i] = nullptr;
  }
  return RON_OK;
}

// One event on `st` for the call being recorded (the last of c->pending): an op's start on the op's stream, or a kStamp* mark.  An
// op ends where the next op of its lane starts (or at the lane's end stamp).
static int stamp(ron_ctx* c, hipStream_t st, int what) {
  Event e;
  if (!c->event_pool.empty()) { e = std::move(c->event_pool.back()); c->event_pool.pop_back(); }
  else RON_HIP_CHECK(hipEventCreate(e.put()));
  RON_HIP_CHECK(hipEventRecord(e, st));
  c->pending.back().push_back(std::move(e));
  c->pending_ops.back().push_back(what);
  return RON_OK;
}
// the stream lane a stamp was recorded on
static int stamp_lane(const ron_ctx* c, int what) {
  if (what >= 0) return c->ops[what].lane;
  return what >= kStampPostEnd ? 0 : (kStampLaneEnd - what) / 10;
}

// ron_forward; *recorded: the call was picked for per-launch timing (ron_profile_enable) and has opened c->pending.back()
static int forward(ron_ctx* c, const float* d_images, int n, ron_heads* out, void* stream, bool* recorded) {
  *recorded = false;
  RON_REQUIRE(c && d_images && out, "NULL argument");
  if (!c->finalized) { ron::set_error("ron_forward before ron_finalize_weights"); return RON_ERR_STATE; }
  RON_REQUIRE(n >= 1 && n <= c->cfg.max_batch, "batch %d outside [1, max_batch=%d]", n, c->cfg.max_batch);
  // launches go to the context's device whatever the caller's current device is (the stream must belong to it)
  DeviceGuard on_device(c->cfg.device);
  RON_HIP_CHECK(on_device.err);
  int rc = ron_heads_describe(c, out);
  if (rc) return rc;
  if (c->profiling > 0 && c->pending.size() < 256) {
    --c->profiling;
    c->pending.emplace_back();
    c->pending_ops.emplace_back();
    *recorded = true;
  }
  const bool rec = *recorded;
  const Weights& W = *c->wts;
  const hipStream_t main_stream = (hipStream_t)stream;
  bool lane_started[4] = {false, false, false, false};
  ConvLaunch L[kMaxConvGroup];      // the members of the launch being enqueued
  for (size_t oi = 0; oi < c->ops.size(); ++oi) {
    const Op& o = c->ops[oi];
    hipStream_t s = main_stream;
    if (o.lane > 0) {
      s = c->side[o.lane];
      if (!lane_started[o.lane]) {          // everything enqueued on the main stream so far (incl. this scale's reference map)
        RON_HIP_CHECK(hipEventRecord(c->lane_ready[o.lane], main_stream));
        RON_HIP_CHECK(hipStreamWaitEvent(s, c->lane_ready[o.lane], 0));
        lane_started[o.lane] = true;
      }
    }
    if (rec && (rc = stamp(c, s, (int)oi))) return rc;
    if (o.kind == OP_IM2COL) {
      const Tensor& t = c->tensors[o.out];
      if ((rc = launch_im2col_c3(d_images, n, t.H, t.W, c->cfg.dtype, t.d, t.C, s))) return rc;
    } else if (o.kind == OP_STEM) {
      const Tensor& t = c->tensors[o.out];
      if ((rc = launch_stem_conv(d_images, n, t.H, t.W, c->cfg.dtype, W.stem_w, W.stem_b.as<float>(), c->view(o.out, n), s, W.stem_oscale))) return rc;
    } else if (o.kind == OP_STEM2) {
      const Tensor& t = c->tensors[o.out];
      if ((rc = launch_stem2(d_images, n, 2 * t.H, 2 * t.W, c->cfg.dtype, W.stem2_w1, W.stem_b.as<float>(), W.stem2_w, W.stem2_b.as<float>(),
                             c->view(o.out, n), s))) return rc;
    } else if (o.kind == OP_POOL) {
      if ((rc = launch_maxpool2x2(c->view(o.in, n), c->view(o.out, n), c->cfg.dtype, s))) return rc;
    } else if (o.kind == OP_POOL3) {
      if ((rc = launch_maxpool3x3s1(c->view(o.in, n), c->view(o.out, n), c->cfg.dtype, s))) return rc;
    } else if (o.kind == OP_L2NORM) {
      if ((rc = launch_l2norm(c->view(o.in, n), c->view(o.out, n), W.l2_gamma.as<float>(), c->cfg.dtype, s))) return rc;
    } else {
      // a convolution, or this op and the rest of its group as one launch (one stamp for it), as slot_resources planned it for this batch
      int members = 1;
      if ((rc = gather_launch(c, oi, n, out, L, &members))) return rc;
      const ron_ctx::LaunchPlan& plan = c->launch_plans[n][oi];
      if (o.group >= 0) {
        rc = launch_conv_group(L, members, o.group_cfg, c->splitk[o.lane], c->splitk_bytes[o.lane], s, plan.sk.data());
      } else {
        if (plan.fuse_pool) {                     // the pooled map from the same launch; the pool op that follows is skipped
          L[0].out2 = L[0].out; L[0].out = c->view(c->ops[oi + 1].out, n); L[0].pool = 1;
          ++members;
        }
        rc = launch_conv(L[0], s);
      }
      if (rc) {
        std::string msg = ron_last_error();
        ron::set_error(o.group >= 0 ? "group of %s: %s" : "%s: %s", o.name.c_str(), msg.c_str());
        return rc;
      }
      oi += members - 1;
    }
  }
  if (rec) {
    if ((rc = stamp(c, main_stream, kStampLaneEnd))) return rc;
    for (int l = 1; l < 4; ++l) if (lane_started[l] && (rc = stamp(c, c->side[l], kStampLaneEnd - 10 * l))) return rc;
  }
  for (int l = 1; l < 4; ++l)
    if (lane_started[l]) {                  // join: the caller's stream continues after every side branch
      RON_HIP_CHECK(hipEventRecord(c->lane_done[l], c->side[l]));
      RON_HIP_CHECK(hipStreamWaitEvent(main_stream, c->lane_done[l], 0));
    }
  return RON_OK;
}

extern "C" int ron_forward(ron_ctx* c, const float* d_images, int n, ron_heads* out, void* stream) {
  bool recorded;
  return forward(c, d_images, n, out, stream, &recorded);
}

// ---- per-launch timing -----------------------------------------------------------------------
extern "C" int ron_profile_enable(ron_ctx* c, int enable) {
  RON_REQUIRE(c, "NULL ctx");
  c->profiling = enable > 0 ? enable : 0;
  return RON_OK;
}

static int profile_collect(ron_ctx* c) {
  for (size_t k = 0; k < c->pending.size(); ++k) {
    auto& call = c->pending[k];
    const auto& what = c->pending_ops[k];
    if (call.empty()) continue;
    for (const Event& e : call) RON_HIP_CHECK(hipEventSynchronize(e));
    // the end of op i = the next stamp recorded on the same lane
    for (size_t i = 0; i < call.size(); ++i) {
      int slot;
      if (what[i] >= 0) slot = what[i];
      else if (what[i] == kStampPostStart) slot = (int)c->ops.size();
      else continue;
      const int lane = stamp_lane(c, what[i]);
      size_t j = i + 1;
      while (j < call.size() && stamp_lane(c, what[j]) != lane) ++j;
      if (j == call.size()) continue;
      float ms = 0.f;
      RON_HIP_CHECK(hipEventElapsedTime(&ms, call[i], call[j]));
      c->timing[slot].ms += ms;
      c->timing[slot].launches += 1;
    }
    for (Event& e : call) c->event_pool.push_back(std::move(e));
  }
  c->pending.clear();
  c->pending_ops.clear();
  return RON_OK;
}

extern "C" int ron_profile_num_ops(const ron_ctx* c) { return c ? (int)c->ops.size() + 1 : RON_ERR_INVALID; }
extern "C" int ron_num_grouped_launches(const ron_ctx* c) { return c ? c->grouped_launches : RON_ERR_INVALID; }

extern "C" int ron_profile_get(ron_ctx* c, int i, const char** name, int* is_conv, double* flops_per_image,
                               double* total_ms, int* launches, double* act_bytes_per_image, double* weight_bytes) {
  RON_REQUIRE(c && i >= 0 && i <= (int)c->ops.size(), "op index out of range");
  int rc = profile_collect(c);
  if (rc) return rc;
  const bool post = i == (int)c->ops.size();
  // a grouped launch is reported on its first member (FLOPs / bytes of the whole group, name "first+N"); the other members
  // report nothing, so sums over the rows stay right
  double fl = 0, ab = 0, wb = 0;
  if (!post) {
    const Op& o = c->ops[i];
    const bool member = o.group >= 0 && i > 0 && c->ops[i - 1].group == o.group;
    if (!member)
      for (size_t j = i; j < c->ops.size() && (j == (size_t)i || (o.group >= 0 && c->ops[j].group == o.group)); ++j) {
        fl += c->ops[j].flops; ab += c->ops[j].act_bytes; wb += c->ops[j].wgt_bytes;
      }
  }
  if (name) *name = c->labels[i].c_str();
  if (is_conv) *is_conv = !post && c->ops[i].kind == OP_CONV;
  if (flops_per_image) *flops_per_image = fl;
  if (total_ms) *total_ms = c->timing[i].ms;
  if (launches) *launches = c->timing[i].launches;
  if (act_bytes_per_image) *act_bytes_per_image = ab;
  if (weight_bytes) *weight_bytes = wb;
  return RON_OK;
}

extern "C" int ron_profile_reset(ron_ctx* c) {
  RON_REQUIRE(c, "NULL ctx");
  int rc = profile_collect(c);
  if (rc) return rc;
  for (auto& t : c->timing) t = OpTiming();
  return RON_OK;
}

extern "C" int ron_end_point_shape(const ron_ctx* c, const char* name, int n, int64_t nhwc[4]) {
  RON_REQUIRE(c && name && nhwc, "NULL argument");
  std::string key = name;
  // end_points of the reference: block1..5 = last conv of the VGG block, block6 = fc6, block7 = fc7
  static const std::map<std::string, std::string> alias = {{"block1", "conv1_2"}, {"block2", "conv2_2"}, {"block3", "conv3_3"},
                                                           {"block4", "conv4_3"}, {"block5", "conv5_3"}, {"block6", "fc6"},
                                                           {"block7", "fc7"}};
  auto a = alias.find(key);
  if (a != alias.end()) key = a->second;
  if (c->is_ssd()) { if (key == "fc6") key = "conv6"; else if (key == "fc7") key = "conv7"; }
  auto it = c->tensor_index.find(key);
  if (it == c->tensor_index.end()) { ron::set_error("unknown end point '%s'", name); return RON_ERR_UNKNOWN_NAME; }
  const Tensor& t = c->tensors[it->second];
  nhwc[0] = n; nhwc[1] = t.H; nhwc[2] = t.W; nhwc[3] = t.C;
  return it->second + 1;     // > 0: tensor index + 1 (internal use), callers test for < 0
}

extern "C" int ron_end_point_copy(ron_ctx* c, const char* name, int n, float* d_out, void* stream) {
  RON_REQUIRE(c && name && d_out, "NULL argument");
  RON_REQUIRE(n >= 1 && n <= c->cfg.max_batch, "bad batch");
  int64_t shp[4];
  const int idx = ron_end_point_shape(c, name, n, shp);
  if (idx < 0) return idx;
  if (c->tensors[idx - 1].d.p == nullptr) { ron::set_error("end point '%s' is not materialised in this configuration", name); return RON_ERR_UNKNOWN_NAME; }
  return launch_unpack(c->view(idx - 1, n), c->cfg.dtype, 0, d_out, (hipStream_t)stream);
}

// forward + one post-processing stage on the context's head buffers and workspace, the stage timed as the last ron_profile_get
// index when this call is profiled.  `post` enqueues the stage on the heads; a stage that fails leaves the workspace dirty.
template <class Post>
static int detect_with(ron_ctx* c, const float* d_images, int n, void* stream, Post post) {
  DeviceGuard on_device(c->cfg.device);
  RON_HIP_CHECK(on_device.err);
  if (!c->finalized) { ron::set_error("ron_detect before ron_finalize_weights"); return RON_ERR_STATE; }
  ron_heads hd;
  memset(&hd, 0, sizeof(hd));
  own_heads(c, &hd);      // (head buffers and workspace: slot_resources, at ron_finalize_weights / ron_clone)
  if (c->post_ws_dirty) {
    // an earlier call failed between its select pass and the pass that zeroes the counters again: start from a clean workspace
    RON_HIP_CHECK(ron::dev_memset_async(c->post_ws, 0, (size_t)c->post_ws_bytes, (hipStream_t)stream));
    c->post_ws_dirty = false;
    c->tfe_counters_stale = false;
  }
  bool prof;
  int rc = forward(c, d_images, n, &hd, stream, &prof);
  if (rc) return rc;
  if (prof && (rc = stamp(c, (hipStream_t)stream, kStampPostStart))) return rc;
  rc = post(hd);
  if (rc != RON_OK) c->post_ws_dirty = true;
  if (rc == RON_OK && prof) rc = stamp(c, (hipStream_t)stream, kStampPostEnd);
  return rc;
}

extern "C" int ron_detect(ron_ctx* c, const float* d_images, int n, const ron_post_cfg* cfg, ron_detections* out, void* stream) {
  RON_REQUIRE(c && cfg && out, "NULL argument");
  RON_REQUIRE(n >= 1 && n <= c->cfg.max_batch, "batch %d outside [1, max_batch=%d]", n, c->cfg.max_batch);
  return detect_with(c, d_images, n, stream, [&](ron_heads& hd) {
    ron_post_cfg pc = *cfg;
    pc.input_flags = ron::kPostWsClean;      // logits + raw offsets straight from the conv stack; self-cleaning workspace (common.h)
    c->tfe_counters_stale = true;
    return ron_post_np(&hd, n, &pc, c->post_ws, c->post_ws_bytes, out, nullptr, nullptr, stream);
  });
}

extern "C" int ron_detect_tfe(ron_ctx* c, const float* d_images, int n, const ron_tfe_cfg* cfg, float* scores, float* bboxes,
                              void* stream) {
  RON_REQUIRE(c && cfg && scores && bboxes, "NULL argument");
  RON_REQUIRE(n >= 1 && n <= c->cfg.max_batch, "batch %d outside [1, max_batch=%d]", n, c->cfg.max_batch);
  int rc = ron::tfe_cfg_check(cfg);         // before anything is enqueued: a rejected cfg leaves the context as it was
  if (rc != RON_OK) return rc;
  if (!c->finalized) { ron::set_error("ron_detect_tfe before ron_finalize_weights"); return RON_ERR_STATE; }
  return detect_with(c, d_images, n, stream, [&](ron_heads& hd) {
    const int r = ron::post_tfe_ctx(&hd, n, c->cfg.max_batch, cfg, c->post_ws, c->post_ws_bytes, c->tfe_counters_stale, scores,
                                    bboxes, (hipStream_t)stream);
    if (r == RON_OK) c->tfe_counters_stale = false;
    return r;
  });
}
