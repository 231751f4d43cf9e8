// Dry-run sweep of the host planners of libron_hip under AddressSanitizer / UBSan (make -C ron_tensorflow_amd/csrc asan).
//
// With RON_PLAN_ONLY=1 (csrc/common.h) the library makes every host-side decision and no HIP call.  For every
// (variant, dtype, head plan, max_batch) below: ron_create -> ron_load_weight (constant weights) -> ron_finalize_weights, which builds
// the graph (describe_conv geometry), the grouped launch plans (plan_groups) and, for EVERY batch 1..max_batch, the split-K plans and
// scratch sizes (conv_pick_cfg, pick_pos_major, conv_group_plan -> group_splitks_scheduled); then ron_detect at a few batch sizes,
// which walks launch_conv / launch_conv_group up to the launch itself (tile counts, split-K slices, tile order, entry lists, the
// post-processing's workspace layout) and ron_clone (a second slot taking over the plans).  Index tables overrun or integer
// overflow in any of it ends the run with a sanitizer report and a non-zero exit code.  Then the argument passes of the single-operator
// entry points.  With RON_PLAN_TRACE=<file> the library writes a line per skipped launch and this program a heading per context and
// pass: the trace two trees must agree on when a change is meant to leave every plan alone (tests/test_plan_trace_cpu.py).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <string>
#include <vector>

#include "../include/ron_hip.h"

// The objects of this binary are compiled host-only: the registration hooks hipcc emits per translation unit must not reach the HIP
// runtime (there is no device code to register, and no GPU where this runs).  Defined here, they take precedence over libamdhip64's.
extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle = nullptr; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
void __hipRegisterManagedVar(void*, void**, void*, const char*, size_t, unsigned) {}
}

#define CHECK(expr)                                                                        \
  do {                                                                                     \
    const int rc_ = (expr);                                                                \
    if (rc_ != 0) {                                                                        \
      fprintf(stderr, "%s -> %d: %s\n", #expr, rc_, ron_last_error());                     \
      return 1;                                                                            \
    }                                                                                      \
  } while (0)

// RON_PLAN_TRACE=<file>: the library appends one line per launch it skips (csrc/common.h); the headings of this program go to the same
// file, so that every context and argument pass is a section of its own (tests/test_plan_trace_cpu.py digests them one by one).
static FILE* g_trace = nullptr;
static void trace_note(const char* fmt, ...) {
  if (g_trace == nullptr) return;
  va_list ap;
  va_start(ap, fmt);
  vfprintf(g_trace, fmt, ap);
  va_end(ap);
  fputc('\n', g_trace);
  fflush(g_trace);
}

static int run(int variant, int dtype, uint32_t flags, int max_batch, bool detect) {
  trace_note("context %d %d 0x%x %d", variant, dtype, flags, max_batch);
  ron_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.variant = variant; cfg.dtype = dtype;
  cfg.img_h = cfg.img_w = variant == RON_VARIANT_SSD512 ? 512 : (variant == RON_VARIANT_SSD300 ? 300 : 320);
  cfg.num_classes = 21; cfg.max_batch = max_batch; cfg.device = 0; cfg.flags = flags;
  ron_ctx* c = nullptr;
  CHECK(ron_create(&c, &cfg));
  const int nv = ron_num_variables(c);
  std::vector<float> buf;
  for (int i = 0; i < nv; ++i) {
    const char* name = nullptr;
    int64_t shape[4] = {0, 0, 0, 0};
    int nd = 0;
    CHECK(ron_variable_info(c, i, &name, shape, &nd));
    size_t n = 1;
    for (int k = 0; k < nd; ++k) n *= (size_t)shape[k];
    if (buf.size() < n) buf.resize(n);
    const std::string s = name;
    const float v = s.find("moving_variance") != std::string::npos || s.find("gamma") != std::string::npos ? 1.f : 0.01f;
    for (size_t k = 0; k < n; ++k) buf[k] = v;
    CHECK(ron_load_weight(c, name, buf.data(), shape, nd));
  }
  CHECK(ron_finalize_weights(c));
  if (detect) {
    ron_post_cfg pc;
    memset(&pc, 0, sizeof(pc));
    pc.objectness_thres = 0.03f; pc.select_threshold = 0.01f; pc.nms_threshold = 0.45f; pc.top_k = 400;
    pc.bbox_img[2] = pc.bbox_img[3] = 1.f;
    pc.prior_scaling[0] = pc.prior_scaling[1] = 0.1f; pc.prior_scaling[2] = pc.prior_scaling[3] = 0.2f;
    // fake device addresses (never dereferenced in a dry run), sized like the real buffers
    ron_detections det;
    memset(&det, 0, sizeof(det));
    det.capacity = 400;
    det.classes = (int32_t*)0x7000000000ull; det.scores = (float*)0x7100000000ull; det.bboxes = (float*)0x7200000000ull;
    det.anchor_index = (int32_t*)0x7300000000ull; det.count = (int32_t*)0x7400000000ull;
    const float* images = (const float*)0x7500000000ull;
    const int batches[4] = {1, (max_batch + 1) / 2, max_batch > 1 ? max_batch - 1 : 1, max_batch};
    for (int b : batches) CHECK(ron_detect(c, images, b, &pc, &det, nullptr));
    ron_ctx* slot = nullptr;
    CHECK(ron_clone(c, &slot));
    CHECK(ron_detect(slot, images, max_batch, &pc, &det, nullptr));
    CHECK(ron_destroy(slot));
  }
  CHECK(ron_destroy(c));
  return 0;
}

// The argument handling of ron_losses / ron_losses_grad in the dry run (no launch): the per-layer tables filled for 1 .. RON_MAX_LAYERS
// layers from pointers nobody dereferences, and every refusal the header promises as a status code.
static int loss_arguments() {
  float* const f = reinterpret_cast<float*>(uintptr_t(1) << 20);          // fake device addresses, 16-byte aligned
  int64_t* const g = reinterpret_cast<int64_t*>(uintptr_t(2) << 20);
  const ron_loss_cfg cfg = {0.03f, 3.f, 1.f / 3, 1.f / 3};
  for (int layers = 1; layers <= RON_MAX_LAYERS; ++layers) {
    ron_heads h;
    ron_targets t;
    ron_head_grads d;
    const float* objp[RON_MAX_LAYERS];
    memset(&h, 0, sizeof h);
    memset(&t, 0, sizeof t);
    memset(&d, 0, sizeof d);
    h.num_layers = layers;
    h.num_classes = layers == 1 ? 2 : (layers == RON_MAX_LAYERS ? RON_MAX_CLASSES : 21);
    for (int l = 0; l < layers; ++l) {
      h.feat_h[l] = l + 1; h.feat_w[l] = 2 * l + 1; h.num_anchors[l] = l % RON_MAX_ANCHORS_PER_CELL + 1;
      h.cls[l] = f; h.obj[l] = f; h.loc[l] = f; objp[l] = f;
      t.gclasses[l] = g; t.glocalisations[l] = f;
      d.d_cls[l] = f; d.d_obj[l] = f; d.d_loc[l] = f;
    }
    for (int n : {1, 2, 32}) {
      const int64_t ws = ron_losses_grad_workspace_bytes(&h, n);
      if (ws <= 0 || ws != ron_losses_workspace_bytes(&h, n)) return 1;
      int32_t* counts = reinterpret_cast<int32_t*>(g);
      CHECK(ron_losses(&h, objp, &t, n, f, f, &cfg, f, ws, f, counts, nullptr));
      CHECK(ron_losses_grad(&h, objp, &t, n, f, f, &cfg, f, ws, f, counts, &d, nullptr));
      // refusals: a short workspace, a missing gradient table, a missing and a misaligned gradient pointer, a bad batch
      if (ron_losses_grad(&h, objp, &t, n, f, f, &cfg, f, ws - 1, f, counts, &d, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_losses_grad(&h, objp, &t, n, f, f, &cfg, f, ws, f, counts, nullptr, nullptr) != RON_ERR_INVALID) return 1;
      ron_head_grads bad = d;
      bad.d_obj[layers - 1] = nullptr;
      if (ron_losses_grad(&h, objp, &t, n, f, f, &cfg, f, ws, f, counts, &bad, nullptr) != RON_ERR_INVALID) return 1;
      bad = d;
      bad.d_loc[layers - 1] = f + 1;
      if (ron_losses_grad(&h, objp, &t, n, f, f, &cfg, f, ws, f, counts, &bad, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_losses_grad(&h, objp, &t, 0, f, f, &cfg, f, ws, f, counts, &d, nullptr) != RON_ERR_INVALID) return 1;
    }
    h.num_layers = RON_MAX_LAYERS + 1;
    if (ron_losses_grad_workspace_bytes(&h, 1) != -1) return 1;
  }
  return 0;
}

// ron_conv2d_backward_nhwc in the dry run: the descriptor checks, the planner of the weight gradient (tiles, pixel slices), the data
// gradient's forward plan and the carving of the workspace, over the case table of tests/conv_grad_cases.py plus the layer
// shapes of tools/conv_backward_time.py, every dtype and pixel split; the workspace pointer is used for arithmetic only.
static int conv_backward_arguments() {
  struct Case { int n, h, w, cin, cout, k, dil; };
  const Case cases[] = {{1, 1, 1, 64, 64, 3, 1},     {2, 5, 7, 64, 24, 3, 1},      {3, 3, 3, 128, 126, 3, 1},  {1, 10, 10, 64, 192, 3, 6},
                        {2, 19, 19, 192, 64, 1, 1},  {1, 38, 38, 320, 256, 3, 1},  {2, 40, 40, 64, 64, 3, 1},
                        {32, 320, 320, 64, 64, 3, 1}, {32, 160, 160, 128, 128, 3, 1}, {32, 80, 80, 256, 256, 3, 1}, {32, 40, 40, 512, 512, 3, 1},
                        {32, 20, 20, 512, 512, 3, 1}, {32, 10, 10, 1024, 1024, 1, 1}, {32, 40, 40, 512, 210, 3, 1}};
  float* const f = reinterpret_cast<float*>(uintptr_t(1) << 30);          // fake device addresses, 256-byte aligned
  void* const ws = reinterpret_cast<void*>(uintptr_t(1) << 40);
  for (const Case& c : cases) {
    for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F16}) {
      for (int splitk : {-1, 1, 2, 7, 1000000}) {
        for (int relu : {0, 1}) {
          ron_conv_desc d;
          memset(&d, 0, sizeof d);
          d.n = c.n; d.h = c.h; d.w = c.w; d.cin = c.cin; d.cout = c.cout; d.kh = d.kw = c.k; d.stride = 1; d.dilation = c.dil;
          d.relu = relu; d.dtype = dtype; d.tile_cfg = -1; d.splitk = splitk;
          const int64_t bytes = ron_conv2d_backward_workspace_bytes(&d);
          if (bytes <= 0 || bytes % 256 != 0) return 1;
          CHECK(ron_conv2d_backward_nhwc(&d, f, f, relu ? f : nullptr, f, f, f, f, ws, bytes, nullptr));
          CHECK(ron_conv2d_backward_nhwc(&d, nullptr, f, relu ? f : nullptr, f, f, nullptr, nullptr, ws, bytes, nullptr));
          CHECK(ron_conv2d_backward_nhwc(&d, f, nullptr, relu ? f : nullptr, f, nullptr, f, f, ws, bytes, nullptr));
          if (ron_conv2d_backward_nhwc(&d, f, f, relu ? f : nullptr, f, f, f, f, ws, bytes - 1, nullptr) != RON_ERR_INVALID) return 1;
          if (relu && ron_conv2d_backward_nhwc(&d, f, f, nullptr, f, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
          ron_conv_desc bad = d;
          bad.stride = 2;
          if (ron_conv2d_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d; bad.cin = 96;
          if (ron_conv2d_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d; bad.dtype = RON_DTYPE_F16X3;
          if (ron_conv2d_backward_nhwc(&bad, f, f, f, f, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        }
      }
    }
  }
  return 0;
}

// ron_conv_chain_forward / ron_conv_chain_backward in the dry run: the descriptor checks, every layer's plans, the carving of the
// workspace and the refusals, over the chains of tests/conv_chain_cases.py and the VGG body of both RON-320 variants at batch 1 and
// 32, with full and with NULL output sets.
static int conv_chain_arguments() {
  struct Layer { int kind, k, dil, cout, relu, tap; };
  struct Chain { int n, h, w, cin; std::vector<Layer> layers; };
  const Layer P = {RON_CHAIN_POOL2, 0, 0, 0, 0, 0};
  auto c3 = [](int cout, int tap = 0) { return Layer{RON_CHAIN_CONV, 3, 1, cout, 1, tap}; };
  auto body = [&](int n, bool full) {
    const int c6 = full ? 4096 : 1024;
    return Chain{n, 320, 320, 64, {c3(64), P, c3(128), c3(128), P, c3(256), c3(256), c3(256), P, c3(512), c3(512), c3(512, 1), P, c3(512), c3(512),
                                   c3(512, 1), P, full ? Layer{RON_CHAIN_CONV, 7, 1, c6, 1, 1} : Layer{RON_CHAIN_CONV, 3, 3, c6, 1, 1},
                                   Layer{RON_CHAIN_CONV, 1, 1, c6, 1, 0}}};
  };
  const std::vector<Chain> chains = {
      {2, 12, 20, 64, {c3(64), c3(64, 1), P, c3(128), P, Layer{RON_CHAIN_CONV, 3, 3, 192, 1, 1}, Layer{RON_CHAIN_CONV, 1, 1, 65, 0, 0}}},
      {3, 5, 7, 64, {c3(64), P, Layer{RON_CHAIN_CONV, 7, 1, 64, 1, 1}, P, Layer{RON_CHAIN_CONV, 1, 1, 24, 1, 0}}},
      {2, 9, 6, 128, {P, P, Layer{RON_CHAIN_CONV, 3, 1, 64, 0, 0}, P}},
      {1, 1, 1, 64, {c3(64)}},
      {1, 38, 38, 320, {c3(256, 1)}},
      body(1, false), body(32, false), body(1, true), body(32, true)};
  float* const f = reinterpret_cast<float*>(uintptr_t(1) << 30);          // fake device addresses, 256-byte aligned
  void* const ws = reinterpret_cast<void*>(uintptr_t(1) << 40);
  for (const Chain& c : chains) {
    for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F16}) {
      ron_chain_desc d;
      memset(&d, 0, sizeof d);
      d.n = c.n; d.h = c.h; d.w = c.w; d.cin = c.cin; d.dtype = dtype; d.num_layers = (int)c.layers.size();
      const float* in[RON_CHAIN_MAX_LAYERS];
      float* out[RON_CHAIN_MAX_LAYERS];
      float* none[RON_CHAIN_MAX_LAYERS];
      int first_conv = -1, tapped = -1;
      for (int i = 0; i < d.num_layers; ++i) {
        const Layer& l = c.layers[i];
        d.layers[i].kind = l.kind; d.layers[i].k = l.k; d.layers[i].dilation = l.dil; d.layers[i].cout = l.cout;
        d.layers[i].relu = l.relu; d.layers[i].has_bias = l.kind == RON_CHAIN_CONV; d.layers[i].tap = l.tap;
        in[i] = f + 64 * i; out[i] = f + 64 * i; none[i] = nullptr;
        if (l.kind == RON_CHAIN_CONV && first_conv < 0) first_conv = i;
        if (l.tap && tapped < 0) tapped = i;
      }
      const int64_t bytes = ron_conv_chain_workspace_bytes(&d);
      if (bytes <= 0 || bytes % 256 != 0) return 1;
      int64_t shape[4];
      CHECK(ron_conv_chain_shape(&d, d.num_layers - 1, shape));
      if (shape[0] != c.n || ron_conv_chain_shape(&d, d.num_layers, shape) != RON_ERR_INVALID) return 1;
      CHECK(ron_conv_chain_forward(&d, f, in, in, out, f, ws, bytes, nullptr));
      CHECK(ron_conv_chain_backward(&d, f, in, in, f, out, out, ws, bytes, nullptr));
      CHECK(ron_conv_chain_backward(&d, f, nullptr, in, nullptr, out, nullptr, ws, bytes, nullptr));
      CHECK(ron_conv_chain_backward(&d, f, in, in, f, nullptr, nullptr, ws, bytes, nullptr));
      CHECK(ron_conv_chain_backward(&d, f, in, in, nullptr, none, none, ws, bytes, nullptr));
      if (ron_conv_chain_forward(&d, nullptr, in, in, out, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_conv_chain_forward(&d, f, in, in, out, nullptr, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_conv_chain_forward(&d, f + 1, in, in, out, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_conv_chain_forward(&d, f, in, in, out, f, ws, bytes - 1, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_conv_chain_forward(&d, f, in, in, out, f, static_cast<char*>(ws) + 128, bytes, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_conv_chain_backward(&d, nullptr, in, in, f, out, out, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_conv_chain_backward(&d, f, in, in, f, out, out, ws, bytes - 1, nullptr) != RON_ERR_INVALID) return 1;
      if (first_conv >= 0) {
        in[first_conv] = nullptr;
        if (ron_conv_chain_forward(&d, f, in, in, out, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_conv_chain_backward(&d, f, in, in, f, out, out, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        in[first_conv] = f;
      }
      if (tapped >= 0) {
        out[tapped] = nullptr;
        if (ron_conv_chain_forward(&d, f, in, in, out, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        out[tapped] = f;
      }
      ron_chain_desc bad = d;
      bad.num_layers = 0;
      if (ron_conv_chain_workspace_bytes(&bad) != -1) return 1;
      bad.num_layers = RON_CHAIN_MAX_LAYERS + 1;
      if (ron_conv_chain_workspace_bytes(&bad) != -1) return 1;
      bad = d; bad.dtype = RON_DTYPE_F32;
      if (ron_conv_chain_workspace_bytes(&bad) != -1) return 1;
      bad = d; bad.dtype = RON_DTYPE_F16X3;
      if (ron_conv_chain_workspace_bytes(&bad) != -1) return 1;
      bad = d; bad.cin = 96;
      if (ron_conv_chain_workspace_bytes(&bad) != -1) return 1;
      bad = d; bad.layers[0].kind = 2;
      if (ron_conv_chain_workspace_bytes(&bad) != -1) return 1;
      bad = d; bad.n = 1 << 26;          // an activation of 2 GiB or more
      if (ron_conv_chain_workspace_bytes(&bad) != -1) return 1;
      if (first_conv >= 0) {
        bad = d; bad.layers[first_conv].k = 5;
        if (ron_conv_chain_workspace_bytes(&bad) != -1) return 1;
        bad = d; bad.layers[first_conv].k = 7; bad.layers[first_conv].dilation = 2;
        if (ron_conv_chain_workspace_bytes(&bad) != -1) return 1;
        if (first_conv < d.num_layers - 1) {
          bad = d; bad.layers[first_conv].cout = 24;
          if (ron_conv_chain_workspace_bytes(&bad) != -1) return 1;
        }
      }
    }
  }
  return 0;
}

// ron_head_chain_forward / ron_head_chain_backward in the dry run: the cases of tests/head_chain_cases.py and the four chains of each
// RON-320 scale (nets.ron_vgg_320.head_chains: 40^2, 20^2, 10^2, 5^2; 21 classes) at batch 1 and 32, with full and with NULL output
// sets, and the refusals the two new layer kinds add.
static int head_chain_arguments() {
  struct Layer { int kind, k, cout, cout2, relu, bias; };
  struct Chain { int n, h, w, cin; std::vector<Layer> layers; };
  const Layer P = {RON_CHAIN_POOL2, 0, 0, 0, 0, 0};
  auto cv = [](int k, int cout, int relu = 1, int bias = 1) { return Layer{RON_CHAIN_CONV, k, cout, 0, relu, bias}; };
  auto bn = [](int relu = 1) { return Layer{RON_CHAIN_BN, 0, 0, 0, relu, 0}; };
  auto pr = [](int cout, int cout2, int relu = 0) { return Layer{RON_CHAIN_CONV_PAIR, 0, cout, cout2, relu, 1}; };
  std::vector<Chain> chains = {
      {2, 6, 10, 64, {cv(3, 64, 0, 0), bn(), cv(3, 12, 0)}},
      {2, 6, 10, 64, {pr(64, 64), bn(), pr(128, 64), bn(), cv(3, 18, 0)}},
      {3, 5, 7, 64, {cv(3, 64, 0, 0), bn()}},
      {2, 4, 4, 128, {bn(0), cv(1, 64)}},
      {2, 9, 6, 64, {cv(3, 64), P, bn(), P, bn(0)}},
      {1, 4, 4, 64, {cv(3, 64), pr(64, 64, 1)}},
      {1, 3, 3, 64, {cv(1, 512, 0, 0), bn(), cv(1, 8)}},
      {1, 1, 1, 8, {bn()}},
      {1, 1, 1027, 8, {bn()}},
      {2, 40, 40, 512, {bn()}}};
  const int anchors = 10, classes = 21;
  for (int n : {1, 32}) {
    for (int s = 0; s < 4; ++s) {
      const int hw = 5 << s, left_c = s < 2 ? 1024 : 512;
      if (s == 0) chains.push_back({n, hw, hw, 512, {bn()}});                               // the top scale: the 2x2 convolution is in front
      else chains.push_back({n, hw, hw, left_c, {cv(3, 512, 0, 0), bn()}});
      chains.push_back({n, hw, hw, 512, {cv(3, 512, 0, 0), bn(), cv(3, 2 * anchors, 0)}});
      chains.push_back({n, hw, hw, 512, {pr(512, 512), bn(), pr(512, 512), bn(), cv(3, anchors * classes, 0)}});
      chains.push_back({n, hw, hw, 512, {cv(3, 512, 0, 0), bn(), cv(3, 4 * anchors, 0)}});
    }
  }
  float* const f = reinterpret_cast<float*>(uintptr_t(1) << 30);          // fake device addresses, 256-byte aligned
  void* const ws = reinterpret_cast<void*>(uintptr_t(1) << 40);
  for (const Chain& c : chains) {
    for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F16}) {
      ron_head_chain_desc d;
      memset(&d, 0, sizeof d);
      d.n = c.n; d.h = c.h; d.w = c.w; d.cin = c.cin; d.dtype = dtype; d.num_layers = (int)c.layers.size();
      ron_head_chain_ptrs all[RON_CHAIN_MAX_LAYERS], some[RON_CHAIN_MAX_LAYERS];
      int first_bn = -1, first_pair = -1;
      for (int i = 0; i < d.num_layers; ++i) {
        const Layer& l = c.layers[i];
        ron_head_chain_layer& t = d.layers[i];
        t.kind = l.kind; t.k = l.k; t.dilation = 1; t.cout = l.cout; t.cout2 = l.cout2; t.relu = l.relu; t.has_bias = l.bias;
        t.eps = 1e-5f; t.decay = 0.997f;
        float* const p = f + 64 * i;
        all[i] = ron_head_chain_ptrs{p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p};
        some[i] = ron_head_chain_ptrs{p, p, p, p, p, p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr};
        if (l.kind == RON_CHAIN_BN && first_bn < 0) first_bn = i;
        if (l.kind == RON_CHAIN_CONV_PAIR && first_pair < 0) first_pair = i;
      }
      const int64_t bytes = ron_head_chain_workspace_bytes(&d);
      if (bytes <= 0 || bytes % 256 != 0) return 1;
      int64_t shape[4];
      CHECK(ron_head_chain_shape(&d, d.num_layers - 1, shape));
      if (shape[0] != c.n || ron_head_chain_shape(&d, d.num_layers, shape) != RON_ERR_INVALID) return 1;
      CHECK(ron_head_chain_forward(&d, f, all, f, ws, bytes, nullptr));
      CHECK(ron_head_chain_forward(&d, f, some, f, ws, bytes, nullptr));          // no moving statistics, no mean / var outputs
      CHECK(ron_head_chain_backward(&d, f, all, f, ws, bytes, nullptr));
      CHECK(ron_head_chain_backward(&d, f, all, nullptr, ws, bytes, nullptr));
      CHECK(ron_head_chain_backward(&d, f, some, f, ws, bytes, nullptr));          // dx alone
      CHECK(ron_head_chain_backward(&d, f, some, nullptr, ws, bytes, nullptr));    // nothing asked for: nothing runs
      if (ron_head_chain_forward(&d, nullptr, all, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_head_chain_forward(&d, f, nullptr, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_head_chain_forward(&d, f, all, f, ws, bytes - 1, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_head_chain_backward(&d, f + 1, all, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_head_chain_backward(&d, f, all, f, ws, bytes - 1, nullptr) != RON_ERR_INVALID) return 1;
      if (first_bn >= 0) {
        ron_head_chain_ptrs keep = all[first_bn];
        all[first_bn].moving_var = nullptr;
        if (ron_head_chain_forward(&d, f, all, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        all[first_bn] = keep; all[first_bn].gamma = f + 1;
        if (ron_head_chain_forward(&d, f, all, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_head_chain_backward(&d, f, all, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        all[first_bn] = keep;
        ron_head_chain_desc bad = d;
        bad.layers[first_bn].tap = 1;
        if (ron_head_chain_workspace_bytes(&bad) != -1) return 1;
        bad = d; bad.layers[first_bn].eps = -1.f;
        if (ron_head_chain_workspace_bytes(&bad) != -1) return 1;
        bad = d; bad.layers[first_bn].decay = 1.5f;
        if (ron_head_chain_workspace_bytes(&bad) != -1) return 1;
      }
      if (first_pair >= 0) {
        ron_head_chain_ptrs keep = all[first_pair];
        all[first_pair].w2 = nullptr;
        if (ron_head_chain_forward(&d, f, all, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_head_chain_backward(&d, f, all, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        all[first_pair] = keep;
        ron_head_chain_desc bad = d;
        bad.layers[first_pair].tap = 1;
        if (ron_head_chain_workspace_bytes(&bad) != -1) return 1;
        bad = d; bad.layers[first_pair].cout2 = 96;
        if (ron_head_chain_workspace_bytes(&bad) != -1) return 1;
        if (first_pair > 0 && c.layers[first_pair - 1].kind == RON_CHAIN_CONV) {
          bad = d; bad.layers[first_pair - 1].tap = 1;
          if (ron_head_chain_workspace_bytes(&bad) != -1) return 1;
        }
      }
      ron_head_chain_desc bad = d;
      bad.num_layers = 0;
      if (ron_head_chain_workspace_bytes(&bad) != -1) return 1;
      bad = d; bad.layers[0].kind = 4;
      if (ron_head_chain_workspace_bytes(&bad) != -1) return 1;
      bad = d; bad.cin = 12;
      if (ron_head_chain_workspace_bytes(&bad) != -1) return 1;
      bad = d; bad.n = 1 << 26;          // an activation of 2 GiB or more, or a batch normalisation over more than 2^24 rows
      if (ron_head_chain_workspace_bytes(&bad) != -1) return 1;
    }
  }
  return 0;
}

// ron_conv2d_forward_nhwc in the dry run: the descriptor checks, the ConvLaunch of every route (plain, 7 x 7, the stem with and without
// its kernel, 2 x 2 stride 2, transposed, the resident-weight images), the workspace and the refusals, over the case table of
// tests/conv_fwd_cases.py plus the layer shapes of tools/conv_forward_time.py; and the 7 x 7 filter through ron_conv2d_backward_nhwc.
static int conv_forward_arguments() {
  struct Case { int n, h, w, cin, cout, k, dil, stride, tr; };
  const Case cases[] = {{1, 1, 1, 64, 64, 3, 1, 1, 0},     {2, 5, 7, 64, 24, 3, 1, 1, 0},      {3, 3, 3, 128, 126, 3, 1, 1, 0},   {1, 10, 10, 64, 192, 3, 6, 1, 0},
                        {2, 19, 19, 192, 64, 1, 1, 1, 0},  {1, 38, 38, 320, 256, 3, 1, 1, 0},  {2, 40, 40, 64, 64, 3, 1, 1, 0},   {2, 5, 7, 64, 24, 7, 1, 1, 0},
                        {1, 10, 10, 128, 192, 7, 1, 1, 0}, {1, 10, 10, 64, 64, 3, 3, 1, 0},    {2, 3, 5, 64, 1, 3, 1, 1, 0},      {2, 4, 6, 128, 65, 1, 1, 1, 0},
                        {2, 8, 32, 3, 64, 3, 1, 1, 0},     {2, 9, 37, 3, 64, 3, 1, 1, 0},      {2, 6, 8, 64, 24, 2, 1, 2, 0},     {1, 2, 2, 128, 128, 2, 1, 2, 0},
                        {2, 3, 5, 64, 128, 2, 1, 2, 1},    {1, 1, 1, 128, 256, 2, 1, 2, 1},    {1, 8, 32, 64, 64, 3, 1, 1, 0},
                        {32, 320, 320, 3, 64, 3, 1, 1, 0}, {32, 320, 320, 64, 64, 3, 1, 1, 0}, {32, 160, 160, 64, 128, 3, 1, 1, 0}, {32, 80, 80, 256, 256, 3, 1, 1, 0},
                        {32, 40, 40, 512, 512, 3, 1, 1, 0}, {32, 10, 10, 512, 1024, 3, 3, 1, 0}, {32, 10, 10, 512, 4096, 7, 1, 1, 0}, {32, 10, 10, 4096, 4096, 1, 1, 1, 0},
                        {32, 10, 10, 4096, 512, 2, 1, 2, 0}, {32, 20, 20, 512, 512, 2, 1, 2, 1}, {32, 40, 40, 512, 210, 3, 1, 1, 0}};
  float* const f = reinterpret_cast<float*>(uintptr_t(1) << 30);          // fake device addresses, 256-byte aligned
  void* const ws = reinterpret_cast<void*>(uintptr_t(1) << 40);
  for (const Case& c : cases) {
    for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F16}) {
      for (int relu : {0, 1}) {
        ron_conv_desc d;
        memset(&d, 0, sizeof d);
        d.n = c.n; d.h = c.h; d.w = c.w; d.cin = c.cin; d.cout = c.cout; d.kh = d.kw = c.k; d.stride = c.stride; d.dilation = c.dil;
        d.relu = relu; d.transpose = c.tr; d.dtype = dtype; d.tile_cfg = -1; d.splitk = -1;
        const int64_t bytes = ron_conv2d_forward_workspace_bytes(&d);
        if (bytes <= 0 || bytes % 256 != 0) return 1;
        CHECK(ron_conv2d_forward_nhwc(&d, f, f, f, f, ws, bytes, nullptr));
        CHECK(ron_conv2d_forward_nhwc(&d, f, f + 1, nullptr, f, ws, bytes, nullptr));      // no bias; a w that is only 4-byte aligned
        CHECK(ron_conv2d_forward_parts_nhwc(&d, f, f, f, f, ws, bytes, RON_FWD_PART_W | RON_FWD_PART_UNPACK, nullptr));
        if (c.cin == 3) CHECK(ron_conv2d_forward_nhwc(&d, f + 1, f, f, f, ws, bytes, nullptr));
        else if (ron_conv2d_forward_nhwc(&d, f + 1, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_conv2d_forward_nhwc(&d, f, f, f, f + 1, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_conv2d_forward_nhwc(&d, f, f, f, f, ws, bytes - 1, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_conv2d_forward_nhwc(&d, f, f, f, f, static_cast<char*>(ws) + 128, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_conv2d_forward_nhwc(&d, nullptr, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_conv2d_forward_nhwc(&d, f, nullptr, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_conv2d_forward_nhwc(&d, f, f, f, nullptr, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_conv2d_forward_parts_nhwc(&d, f, f, f, f, ws, bytes, 0, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_conv2d_forward_parts_nhwc(&d, f, f, f, f, ws, bytes, 16, nullptr) != RON_ERR_INVALID) return 1;
        ron_conv_desc bad = d;
        bad.dtype = RON_DTYPE_F16X3;
        if (ron_conv2d_forward_workspace_bytes(&bad) != -1) return 1;
        bad = d; bad.dtype = RON_DTYPE_F32;
        if (ron_conv2d_forward_workspace_bytes(&bad) != -1) return 1;
        bad = d; bad.cin = 96;
        if (ron_conv2d_forward_workspace_bytes(&bad) != -1) return 1;
        bad = d; bad.kh = bad.kw = 5;
        if (ron_conv2d_forward_workspace_bytes(&bad) != -1) return 1;
        bad = d; bad.pool = 1;
        if (ron_conv2d_forward_workspace_bytes(&bad) != -1) return 1;
        bad = d; bad.tile_cfg = 1;
        if (ron_conv2d_forward_workspace_bytes(&bad) != -1) return 1;
        bad = d; bad.splitk = 2;
        if (ron_conv2d_forward_workspace_bytes(&bad) != -1) return 1;
        bad = d; bad.center_from = 8;
        if (ron_conv2d_forward_nhwc(&bad, f, f, f, f, ws, (int64_t)1 << 40, nullptr) != RON_ERR_INVALID) return 1;
        if (c.k == 7 && c.stride == 1) {
          bad = d; bad.dilation = 2;
          if (ron_conv2d_forward_workspace_bytes(&bad) != -1 || ron_conv2d_backward_workspace_bytes(&bad) != -1) return 1;
          for (int splitk : {-1, 1, 3, 1000000}) {
            ron_conv_desc g = d;
            g.splitk = splitk;
            const int64_t gb = ron_conv2d_backward_workspace_bytes(&g);
            if (gb <= 0 || gb % 256 != 0) return 1;
            CHECK(ron_conv2d_backward_nhwc(&g, f, f, relu ? f : nullptr, f, f, f, f, ws, gb, nullptr));
            if (ron_conv2d_backward_nhwc(&g, f, f, relu ? f : nullptr, f, f, f, f, ws, gb - 1, nullptr) != RON_ERR_INVALID) return 1;
          }
        }
      }
    }
  }
  // a packed tensor of 2 GiB: conv1_2 at batch 256 (x: 256 * 321 * 321 * 64 * 2 bytes)
  ron_conv_desc big;
  memset(&big, 0, sizeof big);
  big.n = 256; big.h = big.w = 320; big.cin = big.cout = 64; big.kh = big.kw = 3; big.stride = 1; big.dilation = 1; big.relu = 1;
  big.dtype = RON_DTYPE_BF16; big.tile_cfg = -1; big.splitk = -1;
  if (ron_conv2d_forward_workspace_bytes(&big) != -1) return 1;
  return 0;
}

// ron_conv2d_stem_backward_nhwc in the dry run: the descriptor checks, the pixel slices and the workspace, over the case table of
// tests/stem_grad_cases.py plus the layer itself (tools/stem_backward_time.py) and the last accepted pixel count, every dtype and pixel
// split, and the refusals; pointers are used for arithmetic only.
static int stem_backward_arguments() {
  struct Case { int n, h, w; };
  const Case cases[] = {{1, 1, 1}, {2, 5, 7}, {3, 3, 3}, {1, 1, 33}, {1, 33, 1}, {1, 8, 32}, {2, 40, 40}, {1, 320, 320}, {32, 320, 320},
                        {64, 512, 512}, {1, 1, (int)RON_STEM_BACKWARD_MAX_PIXELS}, {32768, 1, 65535}};
  float* const f = reinterpret_cast<float*>(uintptr_t(1) << 30);          // fake device addresses, 256-byte aligned
  void* const ws = reinterpret_cast<void*>(uintptr_t(1) << 40);
  for (const Case& c : cases) {
    for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F16}) {
      for (int splitk : {-1, 1, 2, 7, 1000000, 0x7FFFFFFF}) {
        for (int relu : {0, 1}) {
          ron_conv_desc d;
          memset(&d, 0, sizeof d);
          d.n = c.n; d.h = c.h; d.w = c.w; d.cin = 3; d.cout = 64; d.kh = d.kw = 3; d.stride = 1; d.dilation = 1;
          d.relu = relu; d.dtype = dtype; d.tile_cfg = -1; d.splitk = splitk;
          const int64_t bytes = ron_conv2d_stem_backward_workspace_bytes(&d);
          if (bytes <= 0 || bytes % 256 != 0 || bytes >= ((int64_t)1 << 32)) return 1;
          float* const y = relu ? f : nullptr;
          CHECK(ron_conv2d_stem_backward_nhwc(&d, f, y, f, f, f, ws, bytes, nullptr));
          CHECK(ron_conv2d_stem_backward_nhwc(&d, nullptr, y, f, nullptr, f, ws, bytes, nullptr));
          CHECK(ron_conv2d_stem_backward_nhwc(&d, f + 1, y, f, f, nullptr, ws, bytes, nullptr));      // an x that is only 4-byte aligned
          CHECK(ron_conv2d_stem_backward_nhwc(&d, nullptr, y, f, nullptr, nullptr, ws, bytes, nullptr));
          if (ron_conv2d_stem_backward_nhwc(&d, f, y, f, f, f, ws, bytes - 1, nullptr) != RON_ERR_INVALID) return 1;
          if (relu && ron_conv2d_stem_backward_nhwc(&d, f, nullptr, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
          if (ron_conv2d_stem_backward_nhwc(&d, f, y, f + 1, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
          if (ron_conv2d_stem_backward_nhwc(&d, nullptr, y, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
          ron_conv_desc bad = d;
          bad.cin = 64;
          if (ron_conv2d_stem_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d; bad.cout = 24;
          if (ron_conv2d_stem_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d; bad.kh = bad.kw = 5;
          if (ron_conv2d_stem_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d; bad.dilation = 2;
          if (ron_conv2d_stem_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d; bad.splitk = 0;
          if (ron_conv2d_stem_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d; bad.dtype = RON_DTYPE_F16X3;
          if (ron_conv2d_stem_backward_nhwc(&bad, f, f, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        }
      }
    }
  }
  // one pixel more than the kernel's 32-bit pixel arithmetic holds, and products that leave 32 and 64 bits
  const Case big[] = {{1, 1, (int)RON_STEM_BACKWARD_MAX_PIXELS + 1}, {32768, 256, 256}, {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, {65536, 65536, 1}};
  for (const Case& c : big) {
    ron_conv_desc d;
    memset(&d, 0, sizeof d);
    d.n = c.n; d.h = c.h; d.w = c.w; d.cin = 3; d.cout = 64; d.kh = d.kw = 3; d.stride = 1; d.dilation = 1;
    d.relu = 1; d.dtype = RON_DTYPE_BF16; d.tile_cfg = -1; d.splitk = -1;
    if (ron_conv2d_stem_backward_workspace_bytes(&d) != -1) return 1;
    if (ron_conv2d_stem_backward_nhwc(&d, f, f, f, f, f, ws, (int64_t)1 << 40, nullptr) != RON_ERR_INVALID) return 1;
  }
  return 0;
}

// ron_maxpool2x2_backward_nhwc and ron_conv2d_k2s2_backward_nhwc in the dry run: the case tables of tests/op_grad_cases.py plus the
// shapes of tools/op_backward_time.py, every dtype and pixel split, and the refusals; pointers are used for arithmetic only.
static int op_backward_arguments() {
  float* const f = reinterpret_cast<float*>(uintptr_t(1) << 30);          // fake device addresses, 256-byte aligned
  void* const ws = reinterpret_cast<void*>(uintptr_t(1) << 40);
  struct Pool { int n, h, w, c; };
  const Pool pools[] = {{1, 1, 1, 8}, {1, 2, 2, 8}, {2, 5, 7, 8}, {1, 4, 6, 72}, {2, 9, 8, 64}, {1, 38, 38, 512},
                        {32, 320, 320, 64}, {32, 160, 160, 128}, {32, 80, 80, 256}, {32, 40, 40, 512}, {32, 20, 20, 512}, {64, 75, 75, 256}};
  for (const Pool& p : pools) {
    for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F16}) {
      CHECK(ron_maxpool2x2_backward_nhwc(f, f, p.n, p.h, p.w, p.c, dtype, f, nullptr));
      if (ron_maxpool2x2_backward_nhwc(f, f, p.n, p.h, p.w, p.c + 4, dtype, f, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_maxpool2x2_backward_nhwc(f, f, p.n, 0, p.w, p.c, dtype, f, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_maxpool2x2_backward_nhwc(f, f + 1, p.n, p.h, p.w, p.c, dtype, f, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_maxpool2x2_backward_nhwc(f, f, p.n, p.h, p.w, p.c, dtype, nullptr, nullptr) != RON_ERR_INVALID) return 1;
    }
    if (ron_maxpool2x2_backward_nhwc(f, f, p.n, p.h, p.w, p.c, RON_DTYPE_F32, f, nullptr) != RON_ERR_INVALID) return 1;
    if (ron_maxpool2x2_backward_nhwc(f, f, p.n, p.h, p.w, p.c, RON_DTYPE_F16X3, f, nullptr) != RON_ERR_INVALID) return 1;
  }
  struct Case { int n, h, w, cin, cout, transpose; };
  const Case cases[] = {{1, 2, 2, 64, 64, 0},   {2, 6, 10, 64, 24, 0},  {3, 4, 4, 128, 126, 0},  {1, 10, 10, 320, 192, 0}, {2, 40, 40, 64, 64, 0},
                        {1, 1, 1, 64, 64, 1},   {2, 3, 5, 64, 128, 1},  {3, 2, 2, 192, 64, 1},   {1, 20, 20, 512, 512, 1}, {2, 19, 19, 128, 64, 1},
                        {32, 10, 10, 1024, 512, 0}, {32, 10, 10, 4096, 512, 0}, {32, 5, 5, 512, 512, 1}, {32, 10, 10, 512, 512, 1},
                        {32, 20, 20, 512, 512, 1}, {32, 2, 2, 64, 1, 0}};
  for (const Case& c : cases) {
    for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F16}) {
      for (int splitk : {-1, 1, 2, 7, 1000000}) {
        for (int relu : {0, 1}) {
          ron_conv_desc d;
          memset(&d, 0, sizeof d);
          d.n = c.n; d.h = c.h; d.w = c.w; d.cin = c.cin; d.cout = c.cout; d.kh = d.kw = 2; d.stride = 2; d.dilation = 1;
          d.relu = relu; d.transpose = c.transpose; d.dtype = dtype; d.tile_cfg = -1; d.splitk = splitk;
          const int64_t bytes = ron_conv2d_k2s2_backward_workspace_bytes(&d);
          if (bytes <= 0 || bytes % 256 != 0) return 1;
          CHECK(ron_conv2d_k2s2_backward_nhwc(&d, f, f, relu ? f : nullptr, f, f, f, f, ws, bytes, nullptr));
          CHECK(ron_conv2d_k2s2_backward_nhwc(&d, nullptr, f, relu ? f : nullptr, f, f, nullptr, nullptr, ws, bytes, nullptr));
          CHECK(ron_conv2d_k2s2_backward_nhwc(&d, f, nullptr, relu ? f : nullptr, f, nullptr, f, f, ws, bytes, nullptr));
          CHECK(ron_conv2d_k2s2_backward_nhwc(&d, f, f, relu ? f : nullptr, f, f + 1, f, f, ws, bytes, nullptr));      // a dx that is only 4-byte aligned
          if (ron_conv2d_k2s2_backward_nhwc(&d, f, f, relu ? f : nullptr, f, f, f, f, ws, bytes - 1, nullptr) != RON_ERR_INVALID) return 1;
          if (relu && ron_conv2d_k2s2_backward_nhwc(&d, f, f, nullptr, f, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
          if (ron_conv2d_k2s2_backward_nhwc(&d, f, f, f, f + 1, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
          ron_conv_desc bad = d;
          bad.stride = 1;
          if (ron_conv2d_k2s2_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d; bad.kh = bad.kw = 3;
          if (ron_conv2d_k2s2_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d; bad.dilation = 2;
          if (ron_conv2d_k2s2_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d; bad.cin = 96;
          if (ron_conv2d_k2s2_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d; bad.pool = 1;
          if (ron_conv2d_k2s2_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d; bad.splitk = 0;
          if (ron_conv2d_k2s2_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d;
          if (c.transpose) bad.cout = 24; else bad.h += 1;
          if (ron_conv2d_k2s2_backward_workspace_bytes(&bad) != -1) return 1;
          bad = d; bad.dtype = RON_DTYPE_F16X3;
          if (ron_conv2d_k2s2_backward_nhwc(&bad, f, f, f, f, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        }
      }
    }
  }
  return 0;
}

// ron_batchnorm_train_nhwc and ron_batchnorm_backward_nhwc in the dry run: the shapes of tests/bn_cases.py (M around the rows of a wave,
// of a workgroup and of a slice for 2, 18-of-32 and 64 lanes per row), the shapes tools/batchnorm_time.py times, the last accepted
// row count, and every refusal; pointers are used for arithmetic only.
static int batchnorm_arguments() {
  float* const f = reinterpret_cast<float*>(uintptr_t(1) << 30);          // fake device addresses, 256-byte aligned
  void* const ws = reinterpret_cast<void*>(uintptr_t(1) << 40);
  auto desc = [](int n, int h, int w, int c, int dtype, int relu) {
    ron_bn_desc d;
    memset(&d, 0, sizeof d);
    d.n = n; d.h = h; d.w = w; d.c = c; d.dtype = dtype; d.relu = relu; d.eps = 1e-5f; d.decay = 0.997f;
    return d;
  };
  struct Shape { int n, h, w, c; };
  std::vector<Shape> shapes = {{1, 1, 1, 8}, {1, 1, 2, 8}, {2, 5, 5, 512}, {2, 40, 40, 512}, {1, 64, 64, 8}, {1, 32, 32, 8}, {1, 8, 8, 72},
                               {2, 4, 4, 1024}, {1, 4096, 4096, 8}, {4096, 64, 64, 8}, {1, 1, 1, 262144}};
  for (int m : {31, 32, 33, 127, 128, 129, 511, 512, 513, 1027}) shapes.push_back({1, 1, m, 8});
  for (int m : {1, 2, 3, 7, 8, 9, 31, 32, 33, 67}) shapes.push_back({1, 1, m, 72});
  for (int m : {1, 2, 3, 4, 5, 15, 16, 17, 35}) shapes.push_back({1, 1, m, 1024});
  for (int s : {40, 20, 10, 5})
    for (int c : {512, 1024}) shapes.push_back({32, s, s, c});
  for (const Shape& p : shapes) {
    for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F16}) {
      for (int relu : {0, 1}) {
        const ron_bn_desc d = desc(p.n, p.h, p.w, p.c, dtype, relu);
        const int64_t bytes = ron_batchnorm_workspace_bytes(&d);
        if (bytes <= 0 || bytes % 256 != 0) return 1;
        float* const y = relu ? f : nullptr;
        CHECK(ron_batchnorm_train_nhwc(&d, f, f, f, f, f, f, f, f, ws, bytes, nullptr));
        CHECK(ron_batchnorm_train_nhwc(&d, f, f, f, f, f, f, nullptr, nullptr, ws, bytes, nullptr));
        CHECK(ron_batchnorm_backward_nhwc(&d, f, y, f, f, f, f, f, f, f, ws, bytes, nullptr));
        CHECK(ron_batchnorm_backward_nhwc(&d, f, y, f, f, f, f, nullptr, f, f, ws, bytes, nullptr));
        CHECK(ron_batchnorm_backward_nhwc(&d, f, y, f, f, f, f, f, nullptr, nullptr, ws, bytes, nullptr));
        CHECK(ron_batchnorm_backward_nhwc(&d, f, y, f, f, f, f, nullptr, nullptr, nullptr, ws, bytes, nullptr));
        // the calls it refuses: a short, misaligned or missing workspace, a misaligned or missing tensor, half of the moving pair
        if (ron_batchnorm_train_nhwc(&d, f, f, f, f, f, f, f, f, ws, bytes - 1, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_batchnorm_train_nhwc(&d, f, f, f, f, f, f, f, f, static_cast<char*>(ws) + 16, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_batchnorm_train_nhwc(&d, f, f, f, f, f, f, f, f, nullptr, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_batchnorm_train_nhwc(&d, f + 1, f, f, f, f, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_batchnorm_train_nhwc(&d, f, f, f, f, f, f + 2, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_batchnorm_train_nhwc(&d, f, f, f, nullptr, f, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_batchnorm_train_nhwc(&d, f, f, f, f, f, f, f, nullptr, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_batchnorm_train_nhwc(&d, f, f, f, f, f, f, nullptr, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_batchnorm_backward_nhwc(&d, f, y, f, f, f, f, f, f, f, ws, bytes - 1, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_batchnorm_backward_nhwc(&d, f, y, f + 1, f, f, f, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_batchnorm_backward_nhwc(&d, f, y, f, f, f, f, f + 1, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (ron_batchnorm_backward_nhwc(&d, nullptr, y, f, f, f, f, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
        if (relu && ron_batchnorm_backward_nhwc(&d, f, nullptr, f, f, f, f, f, f, f, ws, bytes, nullptr) != RON_ERR_INVALID) return 1;
      }
    }
    // the descriptors it refuses, through all three entries
    ron_bn_desc bad[16];
    for (ron_bn_desc& b : bad) b = desc(p.n, p.h, p.w, p.c, RON_DTYPE_BF16, 1);
    bad[0].dtype = RON_DTYPE_F32; bad[1].dtype = RON_DTYPE_F16X3; bad[2].c += 4; bad[3].c = 0; bad[4].n = 0; bad[5].h = -1; bad[6].w = 0;
    bad[7].relu = 2; bad[8].relu = -1; bad[9].eps = -1e-5f; bad[10].eps = NAN; bad[11].eps = INFINITY; bad[12].decay = -0.5f;
    bad[13].decay = 1.5f; bad[14].decay = NAN; bad[15].n = 65536; bad[15].h = 65536;
    for (const ron_bn_desc& b : bad) {
      if (ron_batchnorm_workspace_bytes(&b) != -1) return 1;
      if (ron_batchnorm_train_nhwc(&b, f, f, f, f, f, f, f, f, ws, (int64_t)1 << 40, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_batchnorm_backward_nhwc(&b, f, f, f, f, f, f, f, f, f, ws, (int64_t)1 << 40, nullptr) != RON_ERR_INVALID) return 1;
    }
  }
  const ron_bn_desc over = desc(4097, 64, 64, 8, RON_DTYPE_BF16, 1);          // 2^24 + 4096 rows: the count would not be exact in fp32
  if (ron_batchnorm_workspace_bytes(&over) != -1 || ron_batchnorm_workspace_bytes(nullptr) != -1) return 1;
  return 0;
}

// ron_optimizer_step in the dry run: the lists of tests/optim_cases.py (single tensors around the work unit, lists around the launch
// table), the lists tools/optimizer_time.py times (the trainable variables of both RON-320 variants, from ron_variable_info), the
// largest accepted list and every refusal; pointers are used for arithmetic only.
static int optimizer_arguments() {
  void* const ws = reinterpret_cast<void*>(uintptr_t(1) << 40);
  float* const reg = reinterpret_cast<float*>(uintptr_t(1) << 41);
  auto table = [](const std::vector<int64_t>& counts) {
    std::vector<ron_opt_tensor> t(counts.size());
    for (size_t i = 0; i < counts.size(); ++i) {
      float* const base = reinterpret_cast<float*>((uintptr_t(i) + 1) << 42);          // fake device addresses, 16-byte aligned, all distinct
      t[i].var = base; t[i].grad = base + 4; t[i].slot0 = base + 8; t[i].slot1 = base + 12;
      t[i].count = counts[i];
      t[i].weight_decay = i % 2 == 0 ? 0.0005f : 0.f;
    }
    return t;
  };
  auto cfg_of = [](int rule) {
    ron_opt_cfg c;
    memset(&c, 0, sizeof c);
    c.rule = rule; c.momentum = 0.9f; c.decay = 0.9f; c.beta1 = 0.9f; c.beta2 = 0.999f; c.epsilon = 1.f;
    return c;
  };
  int64_t plan[4] = {0, 0, 0, 0};
  {
    ron_opt_tensor one;
    memset(&one, 0, sizeof one);
    one.count = 1;
    CHECK(ron_optimizer_plan(&one, 1, plan));
  }
  const int64_t E = plan[2], U = plan[3];
  if (E < 1 || U < 4 || U % 4 != 0 || E * 48 + 64 > 4096) return 1;
  std::vector<std::vector<int64_t>> lists;
  for (int64_t c : {(int64_t)1, (int64_t)3, (int64_t)4, (int64_t)5, U - 1, U, U + 1, 2 * U + 7, (int64_t)1 << 34}) lists.push_back({c});
  for (int64_t n : {(int64_t)1, E - 1, E, E + 1, 2 * E + 1, (int64_t)4096}) {
    std::vector<int64_t> l;
    for (int64_t i = 0; i < n; ++i) l.push_back(1 + (5 * i + 3) % 9);
    lists.push_back(l);
  }
  for (int variant : {(int)RON_VARIANT_REDUCEDFC, (int)RON_VARIANT_FULL}) {
    ron_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.variant = variant; cfg.dtype = RON_DTYPE_BF16; cfg.img_h = cfg.img_w = 320; cfg.num_classes = 21; cfg.max_batch = 1;
    ron_ctx* c = nullptr;
    CHECK(ron_create(&c, &cfg));
    std::vector<int64_t> l;
    for (int i = 0; i < ron_num_variables(c); ++i) {
      const char* name = nullptr;
      int64_t shape[4] = {0, 0, 0, 0};
      int nd = 0;
      CHECK(ron_variable_info(c, i, &name, shape, &nd));
      if (strstr(name, "/moving_") != nullptr) continue;
      int64_t n = 1;
      for (int k = 0; k < nd; ++k) n *= shape[k];
      l.push_back(n);
    }
    CHECK(ron_destroy(c));
    if (l.size() < 100) return 1;
    lists.push_back(l);
  }
  for (const std::vector<int64_t>& counts : lists) {
    std::vector<ron_opt_tensor> t = table(counts);
    const int n = (int)t.size();
    CHECK(ron_optimizer_plan(t.data(), n, plan));
    int64_t units = 0;
    for (int64_t c : counts) units += (c + U - 1) / U;
    if (plan[0] != (n + E - 1) / E || plan[1] != units) return 1;
    const int64_t bytes = ron_optimizer_workspace_bytes(t.data(), n);
    if (bytes < units * 4 || bytes % 256 != 0) return 1;
    for (int rule : {(int)RON_OPT_SGD, (int)RON_OPT_MOMENTUM, (int)RON_OPT_RMSPROP, (int)RON_OPT_ADAM}) {
      const ron_opt_cfg c = cfg_of(rule);
      CHECK(ron_optimizer_step(&c, t.data(), n, 0.001f, 1, reg, ws, bytes, nullptr));
      CHECK(ron_optimizer_step(&c, t.data(), n, 0.001f, 90001, nullptr, nullptr, 0, nullptr));
      // the calls it refuses: a short, misaligned or missing workspace with reg_loss, a missing, misaligned or aliased tensor
      if (ron_optimizer_step(&c, t.data(), n, 0.001f, 1, reg, ws, bytes - 1, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_optimizer_step(&c, t.data(), n, 0.001f, 1, reg, static_cast<char*>(ws) + 16, bytes, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_optimizer_step(&c, t.data(), n, 0.001f, 1, reg, nullptr, bytes, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_optimizer_step(&c, t.data(), n, NAN, 1, nullptr, nullptr, 0, nullptr) != RON_ERR_INVALID) return 1;
      if (ron_optimizer_step(&c, t.data(), n, INFINITY, 1, nullptr, nullptr, 0, nullptr) != RON_ERR_INVALID) return 1;
      if (rule == RON_OPT_ADAM && ron_optimizer_step(&c, t.data(), n, 0.001f, 0, nullptr, nullptr, 0, nullptr) != RON_ERR_INVALID) return 1;
      const int last = n - 1;
      std::vector<ron_opt_tensor> bad[10];
      for (std::vector<ron_opt_tensor>& b : bad) b = t;
      bad[0][last].var = nullptr; bad[1][last].grad = nullptr; bad[2][last].var += 1; bad[3][last].grad += 2;
      bad[4][last].grad = bad[4][last].var; bad[5][last].weight_decay = -1.f; bad[6][last].weight_decay = NAN; bad[7][last].weight_decay = INFINITY;
      bad[8][last].count = 0; bad[9][last].var = bad[9][0].var;          // (a list of one tensor: the entry itself, accepted)
      for (int i = 0; i < 10; ++i) {
        if (i == 9 && n == 1) continue;
        if (ron_optimizer_step(&c, bad[i].data(), n, 0.001f, 1, nullptr, nullptr, 0, nullptr) != RON_ERR_INVALID) {
          fprintf(stderr, "optimizer: rule %d, %d tensors: bad table %d accepted\n", rule, n, i);
          return 1;
        }
      }
      std::vector<ron_opt_tensor> slots[4];
      for (std::vector<ron_opt_tensor>& b : slots) b = t;
      slots[0][last].slot0 = nullptr; slots[1][last].slot1 = nullptr; slots[2][last].slot0 = slots[2][last].var; slots[3][last].slot1 += 1;
      const bool uses[4] = {rule != RON_OPT_SGD, rule >= RON_OPT_RMSPROP, rule != RON_OPT_SGD, rule >= RON_OPT_RMSPROP};
      for (int i = 0; i < 4; ++i)          // a slot the rule does not use is ignored
        if (ron_optimizer_step(&c, slots[i].data(), n, 0.001f, 1, nullptr, nullptr, 0, nullptr) != (uses[i] ? RON_ERR_INVALID : RON_OK)) return 1;
    }
    // the configurations it refuses
    ron_opt_cfg bad[14];
    for (ron_opt_cfg& b : bad) b = cfg_of(RON_OPT_ADAM);
    bad[0].rule = -1; bad[1].rule = 4; bad[2].momentum = -0.1f; bad[3].momentum = 1.5f; bad[4].decay = NAN; bad[5].decay = 2.f; bad[6].beta1 = 1.f;
    bad[7].beta2 = 1.f; bad[8].beta1 = -0.5f; bad[9].beta2 = NAN; bad[10].epsilon = -1.f; bad[11].epsilon = NAN; bad[12].epsilon = INFINITY;
    bad[13].rule = INT32_MAX;
    for (const ron_opt_cfg& b : bad)
      if (ron_optimizer_step(&b, t.data(), n, 0.001f, 1, nullptr, nullptr, 0, nullptr) != RON_ERR_INVALID) return 1;
    if (ron_optimizer_step(nullptr, t.data(), n, 0.001f, 1, nullptr, nullptr, 0, nullptr) != RON_ERR_INVALID) return 1;
  }
  // the lists it refuses, through all three entries
  const ron_opt_cfg c = cfg_of(RON_OPT_MOMENTUM);
  std::vector<ron_opt_tensor> big = table(std::vector<int64_t>(4097, 1));
  std::vector<ron_opt_tensor> wide = table({(int64_t)1 << 34, 1}), huge = table({((int64_t)1 << 40) + 1}), neg = table({-5});
  struct Refused { const ron_opt_tensor* t; int n; };
  const Refused refused[] = {{big.data(), 4097}, {big.data(), 0}, {big.data(), -1}, {nullptr, 1}, {wide.data(), 2}, {huge.data(), 1}, {neg.data(), 1}};
  for (const Refused& r : refused) {
    if (ron_optimizer_plan(r.t, r.n, plan) != RON_ERR_INVALID || ron_optimizer_workspace_bytes(r.t, r.n) != -1) return 1;
    if (ron_optimizer_step(&c, r.t, r.n, 0.001f, 1, nullptr, nullptr, 0, nullptr) != RON_ERR_INVALID) return 1;
  }
  if (ron_optimizer_plan(big.data(), 1, nullptr) != RON_ERR_INVALID) return 1;
  return 0;
}

// The argument envelope of ron_conv_desc (include/ron_hip.h): for every field limit - 1 and limit plan, limit + 1 is refused, through
// ron_conv_plan and the backward's workspace query; zeros, negatives and flags other than 0 / 1 are refused before any arithmetic on
// them (a stride of 0 used to reach a division).  The shapes are those of tests/conv_envelope_cases.py.
static int conv_envelope() {
  auto desc = [](int n, int h, int w, int cin, int cout, int k, int stride, int dil, int transpose, int dtype) {
    ron_conv_desc d;
    memset(&d, 0, sizeof d);
    d.n = n; d.h = h; d.w = w; d.cin = cin; d.cout = cout; d.kh = d.kw = k; d.stride = stride; d.dilation = dil;
    d.relu = 1; d.transpose = transpose; d.dtype = dtype; d.tile_cfg = -1; d.splitk = -1;
    return d;
  };
  int32_t plan[4];
  for (int dtype : {(int)RON_DTYPE_F32, (int)RON_DTYPE_BF16, (int)RON_DTYPE_F16, (int)RON_DTYPE_F16X3}) {
    struct Row { ron_conv_desc d; bool ok; };
    const Row rows[] = {
        {desc(1, 32, 32, 64, 64, 3, 1, 30, 0, dtype), true},   {desc(1, 32, 32, 64, 64, 3, 1, 31, 0, dtype), true},   {desc(1, 40, 40, 64, 64, 3, 1, 32, 0, dtype), false},
        {desc(1, 8, 9, 64, 64, 13, 1, 1, 0, dtype), true},     {desc(1, 8, 9, 64, 64, 15, 1, 1, 0, dtype), true},     {desc(1, 18, 18, 64, 64, 17, 1, 1, 0, dtype), false},
        {desc(1, 16, 16, 64, 64, 16, 1, 1, 0, dtype), false},  {desc(1, 16, 16, 64, 64, 16, 16, 1, 0, dtype), false},
        {desc(2, 12, 18, 64, 64, 6, 6, 1, 0, dtype), true},    {desc(2, 14, 21, 64, 64, 7, 7, 1, 0, dtype), true},    {desc(2, 16, 16, 64, 64, 8, 8, 1, 0, dtype), false},
        {desc(1, 2, 3, 64, 128, 6, 6, 1, 1, dtype), true},     {desc(1, 2, 3, 64, 128, 7, 7, 1, 1, dtype), true},     {desc(1, 2, 2, 64, 128, 8, 8, 1, 1, dtype), false},
        {desc(1, 3, 64, 64, 64, 5, 1, 31, 0, dtype), true},    {desc(1, 3, 64, 64, 64, 7, 1, 21, 0, dtype), true},    {desc(1, 3, 72, 64, 64, 7, 1, 22, 0, dtype), false},
        {desc(1, 3, 72, 64, 64, 5, 1, 32, 0, dtype), false},   {desc(2, 28, 28, 64, 128, 7, 1, 9, 0, dtype), true},   {desc(1, 30, 16, 64, 64, 15, 1, 4, 0, dtype), true},
        {desc(1, 8, 8, 64, 64, 2, 1, 1, 0, dtype), false},     {desc(1, 8, 8, 64, 64, 4, 1, 1, 0, dtype), false},
    };
    for (const Row& r : rows) {
      const int rc = ron_conv_plan(&r.d, plan);
      if (rc != (r.ok ? RON_OK : RON_ERR_INVALID)) {
        fprintf(stderr, "conv envelope: %d x %d stride %d dilation %d transpose %d dtype %d: status %d\n", r.d.kh, r.d.kw, r.d.stride, r.d.dilation, r.d.transpose, dtype, rc);
        return 1;
      }
      if (r.ok && !(plan[2] >= 0 && plan[2] <= 63)) return 1;
      for (int pool : {0, 1}) {                     // the fused pool where it applies: plain stride-1 convolutions
        if (r.d.transpose || r.d.stride != 1) continue;
        ron_conv_desc dp = r.d;
        dp.pool = pool;
        if (ron_conv_plan(&dp, plan) != (r.ok ? RON_OK : RON_ERR_INVALID)) return 1;
      }
    }
    // zeros, negatives, flags: one field at a time on a plain 3x3
    const ron_conv_desc base = desc(1, 8, 8, 64, 64, 3, 1, 1, 0, dtype);
    for (int v : {0, -1, -64, 2, INT32_MIN}) {
      ron_conv_desc bad[12];
      for (ron_conv_desc& b : bad) b = base;
      bad[0].n = v; bad[1].h = v; bad[2].w = v; bad[3].cin = v; bad[4].cout = v; bad[5].kh = bad[5].kw = v; bad[6].stride = v; bad[7].dilation = v;
      bad[8].relu = v; bad[9].pool = v; bad[10].transpose = v; bad[11].kh = v;
      for (int i = 0; i < 12; ++i) {
        if (v == 2 && i <= 4) continue;                                    // (a size of 2 is a size)
        if (v == 2 && i == 7) continue;                                    // (... and a dilation of 2 a dilation)
        if (v == 0 && i >= 8 && i <= 10) continue;                         // (a flag of 0 is a flag)
        if (ron_conv_plan(&bad[i], plan) != RON_ERR_INVALID) { fprintf(stderr, "conv envelope: field %d = %d accepted\n", i, v); return 1; }
        if (ron_conv2d_backward_workspace_bytes(&bad[i]) != -1) { fprintf(stderr, "conv envelope: backward: field %d = %d accepted\n", i, v); return 1; }
        if (ron_conv2d_k2s2_backward_workspace_bytes(&bad[i]) != -1) return 1;
      }
    }
  }
  // the backward's workspace query and plan at the last dilation, 3x3 and 1x1, and one beyond
  float* const f = reinterpret_cast<float*>(uintptr_t(1) << 30);
  void* const ws = reinterpret_cast<void*>(uintptr_t(1) << 40);
  for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F16}) {
    for (int k : {1, 3}) {
      for (int dil : {30, 31, 32}) {
        ron_conv_desc d = desc(k == 1 ? 2 : 1, k == 1 ? 5 : 40, k == 1 ? 7 : 40, 64, k == 1 ? 24 : 64, k, 1, dil, 0, dtype);
        const int64_t bytes = ron_conv2d_backward_workspace_bytes(&d);
        if (dil > 31) {
          if (bytes != -1 || ron_conv2d_backward_nhwc(&d, f, f, f, f, f, f, f, ws, (int64_t)1 << 40, nullptr) != RON_ERR_INVALID) return 1;
          continue;
        }
        if (bytes <= 0 || bytes % 256 != 0) return 1;
        CHECK(ron_conv2d_backward_nhwc(&d, f, f, f, f, f, f, f, ws, bytes, nullptr));
      }
    }
  }
  return 0;
}

// plan_conv and launch_conv_group through the single-operator entry points, with what the graphs never set: every tile configuration
// forced (refusals included: their status and message go into the trace), forced split factors, centre-tap-only columns, the transposed
// convolution, the fused pool with and without its second output, the two-output heads, the grouped pair and RON_IGEMM224=0.  The
// weights are host memory (the entry points pack them); activations are fake device addresses nobody dereferences in a dry run.
static int conv_planner_arguments() {
  struct Case { int n, h, w, cin, cout, k, stride, dil, transpose, pool, center_from; bool all_cfgs; };
  const Case cases[] = {
      {32, 40, 40, 256, 512, 3, 1, 1, 0, 0, 0, true},    // two column tiles of 256, taps innermost
      {4, 40, 40, 256, 512, 3, 1, 1, 0, 0, 0, true},     // about one round of 256 x 128 tiles
      {32, 40, 40, 256, 210, 3, 1, 1, 0, 0, 0, true},    // 193 .. 224 output channels: the 256 x 224 form
      {8, 40, 40, 128, 128, 3, 1, 1, 0, 0, 0, true},     // Cout = 128
      {32, 160, 160, 128, 128, 3, 1, 1, 0, 0, 0, false}, // ... on a map that fills the chip (conv2_x)
      {4, 80, 80, 64, 64, 3, 1, 1, 0, 0, 0, true},       // 64 channels: the resident-weight and patch kernels
      {2, 5, 7, 64, 24, 3, 1, 1, 0, 0, 0, true},         // one tile of 128 x 64
      {32, 10, 10, 512, 1024, 3, 1, 6, 0, 0, 0, false},  // few fat tiles, long K, dilation 6 on a 10 x 10 map (filter rows to skip)
      {8, 10, 10, 128, 256, 7, 1, 1, 0, 0, 0, true},     // 7 x 7 on 10 x 10: position-major rows
      {32, 10, 10, 1024, 1024, 1, 1, 1, 0, 0, 0, false}, // a plain GEMM
      {32, 40, 40, 128, 768, 3, 1, 1, 0, 0, 512, true},  // centre-tap-only columns behind two long column tiles
      {8, 20, 20, 128, 384, 3, 1, 1, 0, 0, 128, false},  // ... behind one of 128
      {32, 10, 10, 256, 256, 2, 2, 1, 1, 0, 0, true},    // transposed, kernel == stride
      {8, 20, 20, 256, 256, 2, 2, 1, 0, 0, 0, true},     // stride 2
      {32, 40, 40, 256, 512, 3, 1, 1, 0, 1, 0, true},    // fused pool
      {3, 19, 19, 128, 256, 3, 1, 1, 0, 1, 0, false},    // ... on an odd map
  };
  float* const x = reinterpret_cast<float*>(uintptr_t(1) << 40);          // fake device addresses
  float* const y = reinterpret_cast<float*>(uintptr_t(2) << 40);
  float* const y2 = reinterpret_cast<float*>(uintptr_t(3) << 40);
  const int ncfg = ron_conv_num_tile_cfgs();
  std::vector<float> w, bias(4096, 0.5f);
  auto desc = [&](const Case& c, int dtype, int cfg, int splitk) {
    ron_conv_desc d;
    memset(&d, 0, sizeof d);
    d.n = c.n; d.h = c.h; d.w = c.w; d.cin = c.cin; d.cout = c.cout; d.kh = d.kw = c.k; d.stride = c.stride; d.dilation = c.dil;
    d.relu = 1; d.transpose = c.transpose; d.dtype = dtype; d.tile_cfg = cfg; d.pool = c.pool; d.splitk = splitk; d.center_from = c.center_from;
    w.assign((size_t)c.k * c.k * c.cin * c.cout, 0.01f);
    return d;
  };
  auto note_rc = [](int rc) { trace_note("-> %d %s", rc, rc != 0 ? ron_last_error() : ""); };
  int launched = 0;
  for (const Case& c : cases) {
    for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F16X3, (int)RON_DTYPE_F32}) {
      if (dtype != RON_DTYPE_BF16 && !c.all_cfgs) continue;
      for (int cfg = -1; cfg < (c.all_cfgs ? ncfg + 1 : 0); ++cfg) {         // (ncfg itself: out of range)
        for (int splitk : {-1, 1, 2, 7}) {
          // (every call packs the weights again: the other dtypes take the forced configurations with the library's own split factor only)
          if (cfg >= 0 && (splitk == 1 || (dtype != RON_DTYPE_BF16 && splitk != -1))) continue;
          if (cfg < 0 && dtype != RON_DTYPE_BF16 && (splitk == 1 || splitk == 7)) continue;
          const ron_conv_desc d = desc(c, dtype, cfg, splitk);
          trace_note("conv %d %d %d %d %d k %d stride %d dil %d transpose %d pool %d center_from %d dtype %d cfg %d splitk %d", c.n, c.h, c.w, c.cin,
                     c.cout, c.k, c.stride, c.dil, c.transpose, c.pool, c.center_from, dtype, cfg, splitk);
          const int rc = ron_conv2d_nhwc(&d, x, w.data(), bias.data(), c.pool || c.transpose ? nullptr : y2, y, nullptr);
          note_rc(rc);
          if (rc != RON_OK && rc != RON_ERR_INVALID) return 1;
          if (cfg < 0 && rc != RON_OK) return 1;                              // the library's own choice is never refused
          launched += rc == RON_OK;
          if (cfg < 0 && splitk < 0) {
            int32_t plan[4] = {0, 0, 0, 0}, n_tile = 0;
            CHECK(ron_conv_plan(&d, plan));
            CHECK(ron_conv_plan_n_tile(&d, &n_tile));
            trace_note("plan %d %d %d %d n_tile %d", plan[0], plan[1], plan[2], plan[3], n_tile);
          }
          if (c.pool && (cfg < 0 || splitk < 0)) {
            trace_note("... with the un-pooled map as a second output");
            note_rc(ron_conv2d_pool2_nhwc(&d, x, w.data(), bias.data(), y, y2, nullptr));
          }
        }
      }
    }
  }
  if (launched < 100) return 1;
  // RON_IGEMM224=0 (read per call): the 256-column tile for 193 .. 224 output channels, chosen and forced, with split factors
  setenv("RON_IGEMM224", "0", 1);
  for (int cfg : {-1, 0, 7}) {
    for (int splitk : {-1, 2}) {
      const ron_conv_desc d = desc(cases[2], RON_DTYPE_BF16, cfg, splitk);
      int32_t n_tile = 0;
      trace_note("RON_IGEMM224=0 cfg %d splitk %d", cfg, splitk);
      note_rc(ron_conv2d_nhwc(&d, x, w.data(), bias.data(), nullptr, y, nullptr));
      CHECK(ron_conv_plan_n_tile(&d, &n_tile));
      trace_note("n_tile %d", n_tile);
      if (n_tile == 224) return 1;
    }
  }
  unsetenv("RON_IGEMM224");
  // the two-output heads (an SSD feature layer's class and box convolutions as one launch)
  const Case heads[] = {{16, 64, 64, 256, 100, 3, 1, 1, 0, 0, 0, true}, {1, 8, 8, 256, 150, 3, 1, 1, 0, 0, 0, true}, {32, 32, 32, 256, 210, 3, 1, 1, 0, 0, 0, true}};
  for (const Case& c : heads) {
    for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F32}) {
      for (int cfg = -1; cfg < ncfg; ++cfg) {
        for (int splitk : {-1, 2, 7}) {
          if (cfg >= 0 && splitk == 7) continue;
          const ron_conv_desc d = desc(c, dtype, cfg, splitk);
          trace_note("heads %d %d %d %d %d first %d dtype %d cfg %d splitk %d", c.n, c.h, c.w, c.cin, c.cout, c.cout * 4 / 5 + 4, dtype, cfg, splitk);
          const int rc = ron_conv2d_heads_nhwc(&d, c.cout * 4 / 5 + 4, x, w.data(), bias.data(), y, y2, nullptr);
          note_rc(rc);
          if (cfg < 0 && rc != RON_OK) return 1;
        }
      }
    }
  }
  // fp32-output heads: one, two on their own, and the grouped pair of 256 x 256 tiles with its own and with forced split factors
  const Case pairs[][2] = {{{32, 10, 10, 256, 210, 3, 1, 1, 0, 0, 0, true}, {32, 5, 5, 256, 210, 3, 1, 1, 0, 0, 0, true}},
                           {{4, 20, 20, 512, 210, 3, 1, 1, 0, 0, 0, true}, {4, 10, 10, 512, 256, 3, 1, 1, 0, 0, 0, true}},
                           {{32, 40, 40, 128, 210, 3, 1, 1, 0, 0, 0, true}, {32, 20, 20, 128, 512, 1, 1, 1, 0, 0, 0, true}}};
  std::vector<float> wb;
  for (const auto& p : pairs) {
    for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F16, (int)RON_DTYPE_F16X3, (int)RON_DTYPE_F32}) {
      for (int n224 : {1, 0}) {
        if (n224) unsetenv("RON_IGEMM224"); else setenv("RON_IGEMM224", "0", 1);
        const int sks[][2] = {{-1, -1}, {1, 1}, {2, 7}, {7, 2}, {2, -1}};
        for (const auto& sk : sks) {
          const ron_conv_desc db = desc(p[1], dtype, -1, sk[1]);
          wb = w;
          const ron_conv_desc da = desc(p[0], dtype, -1, sk[0]);
          for (int grouped : {0, 1}) {
            int32_t widths[2] = {0, 0};
            trace_note("f32out pair %d x %d x %d + %d x %d x %d dtype %d n224 %d splitk %d %d grouped %d", p[0].n, p[0].h, p[0].cout, p[1].n, p[1].h,
                       p[1].cout, dtype, n224, sk[0], sk[1], grouped);
            CHECK(ron_conv2d_f32out_nhwc(&da, x, w.data(), bias.data(), y, &db, x, wb.data(), bias.data(), y2, grouped, widths, nullptr));
            trace_note("widths %d %d", widths[0], widths[1]);
          }
        }
      }
    }
  }
  unsetenv("RON_IGEMM224");
  return 0;
}

int main(int argc, char** argv) {
  if (getenv("RON_PLAN_ONLY") == nullptr) {
    fprintf(stderr, "plan_sweep: run with RON_PLAN_ONLY=1 (a dry run: this binary holds no device code)\n");
    return 2;
  }
  const bool quick = argc > 1 && strcmp(argv[1], "--quick") == 0;
  // --head-chain: the head chain's pass alone (it is part of the full sweep; --quick leaves it out, its sections being pinned one by one)
  if (argc > 1 && strcmp(argv[1], "--head-chain") == 0) {
    if (head_chain_arguments()) {
      fprintf(stderr, "plan_sweep: ron_head_chain_forward / ron_head_chain_backward planning / argument handling: %s\n", ron_last_error());
      return 1;
    }
    printf("plan_sweep: 0 contexts planned, no sanitizer report\n");
    return 0;
  }
  if (const char* path = getenv("RON_PLAN_TRACE")) {
    FILE* f = fopen(path, "w");           // a fresh file; the library appends to it from its first skipped launch on
    if (f != nullptr) fclose(f);
    g_trace = fopen(path, "a");
    if (g_trace == nullptr) { fprintf(stderr, "plan_sweep: cannot write %s\n", path); return 2; }
  }
  const int batches_all[] = {1, 2, 3, 4, 6, 8, 12, 13, 16, 23, 24, 32, 48, 64};
  const uint32_t plans[] = {0u, RON_CFG_LEVEL_GROUPS, RON_CFG_BATCH_GROUPS, RON_CFG_NO_GROUPS, RON_CFG_NO_HALO_SKIP};
  int runs = 0;
  timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  // reducedfc and SSD-512: every head plan x every batch size of the ladder (the plan tables change at 12 / 13 and 23 / 24)
  for (int variant : {(int)RON_VARIANT_REDUCEDFC, (int)RON_VARIANT_SSD512}) {
    for (uint32_t plan : plans) {
      if (variant == RON_VARIANT_SSD512 && (plan == RON_CFG_LEVEL_GROUPS || plan == RON_CFG_BATCH_GROUPS)) continue;
      for (int mb : batches_all) {
        if (quick && mb != 1 && mb != 13 && mb != 32) continue;
        if (variant == RON_VARIANT_SSD512 && mb > 32) continue;       // (conv1_x of 64 images at 512 x 512 is beyond 4 GiB)
        for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F16X3}) {
          if (dtype == RON_DTYPE_F16X3 && (plan != 0u || (mb != 1 && mb != 32))) continue;
          if (run(variant, dtype, RON_CFG_FUSE_POOLS | plan, mb, true)) return 1;
          ++runs;
        }
      }
    }
  }
  // the full VGG-16 variant (229 M parameters to fold and pack per context): the three plan regimes, fp32 once
  for (int mb : {1, 13, 32}) {
    if (quick && mb != 32) continue;
    if (run(RON_VARIANT_FULL, RON_DTYPE_BF16, RON_CFG_FUSE_POOLS, mb, true)) return 1;
    ++runs;
  }
  // SSD-300 (odd maps: SAME pools 75 -> 38, the ragged stem tile, VALID 3x3 blocks): with and without the fused pools and the grouped
  // tail; --quick keeps three contexts (the sweep's time limit)
  for (uint32_t flags : {(uint32_t)RON_CFG_FUSE_POOLS, 0u, (uint32_t)(RON_CFG_FUSE_POOLS | RON_CFG_NO_GROUPS), (uint32_t)RON_CFG_NO_HALO_SKIP}) {
    for (int mb : {1, 4, 13, 16, 32}) {
      for (int dtype : {(int)RON_DTYPE_BF16, (int)RON_DTYPE_F16X3, (int)RON_DTYPE_F32}) {
        if (dtype != RON_DTYPE_BF16 && (flags & ~(uint32_t)RON_CFG_FUSE_POOLS) != 0u) continue;
        if (dtype == RON_DTYPE_F32 && mb > 4) continue;
        if (quick && !((dtype == RON_DTYPE_BF16 && flags == RON_CFG_FUSE_POOLS && (mb == 1 || mb == 32)) ||
                       (dtype == RON_DTYPE_F32 && flags == 0u && mb == 1))) continue;
        if (run(RON_VARIANT_SSD300, dtype, flags, mb, true)) return 1;
        ++runs;
      }
    }
  }
  if (!quick) {
    if (run(RON_VARIANT_REDUCEDFC, RON_DTYPE_F32, 0u, 4, true)) return 1;
    if (run(RON_VARIANT_REDUCEDFC, RON_DTYPE_F16, RON_CFG_FUSE_POOLS | RON_CFG_NO_STEM2, 32, true)) return 1;
    runs += 2;
  }
  clock_gettime(CLOCK_MONOTONIC, &t1);
  printf("plan_sweep: %d contexts created, planned and run dry in %.1f s\n", runs, (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec));
  trace_note("pass loss_arguments");
  if (loss_arguments()) {
    fprintf(stderr, "plan_sweep: ron_losses / ron_losses_grad argument handling: %s\n", ron_last_error());
    return 1;
  }
  trace_note("pass conv_backward_arguments");
  if (conv_backward_arguments()) {
    fprintf(stderr, "plan_sweep: ron_conv2d_backward_nhwc planning / argument handling: %s\n", ron_last_error());
    return 1;
  }
  trace_note("pass stem_backward_arguments");
  if (stem_backward_arguments()) {
    fprintf(stderr, "plan_sweep: ron_conv2d_stem_backward_nhwc planning / argument handling: %s\n", ron_last_error());
    return 1;
  }
  trace_note("pass op_backward_arguments");
  if (op_backward_arguments()) {
    fprintf(stderr, "plan_sweep: ron_maxpool2x2_backward_nhwc / ron_conv2d_k2s2_backward_nhwc planning / argument handling: %s\n", ron_last_error());
    return 1;
  }
  trace_note("pass batchnorm_arguments");
  if (batchnorm_arguments()) {
    fprintf(stderr, "plan_sweep: ron_batchnorm_train_nhwc / ron_batchnorm_backward_nhwc planning / argument handling: %s\n", ron_last_error());
    return 1;
  }
  trace_note("pass optimizer_arguments");
  if (optimizer_arguments()) {
    fprintf(stderr, "plan_sweep: ron_optimizer_step planning / argument handling: %s\n", ron_last_error());
    return 1;
  }
  trace_note("pass conv_envelope");
  if (conv_envelope()) {
    fprintf(stderr, "plan_sweep: the argument envelope of ron_conv_desc: %s\n", ron_last_error());
    return 1;
  }
  trace_note("pass conv_planner_arguments");
  if (conv_planner_arguments()) {
    fprintf(stderr, "plan_sweep: plan_conv / launch_conv_group through the single-operator entry points: %s\n", ron_last_error());
    return 1;
  }
  trace_note("pass conv_forward_arguments");
  if (conv_forward_arguments()) {
    fprintf(stderr, "plan_sweep: ron_conv2d_forward_nhwc planning / argument handling (and the 7 x 7 backward): %s\n", ron_last_error());
    return 1;
  }
  trace_note("pass conv_chain_arguments");
  if (conv_chain_arguments()) {
    fprintf(stderr, "plan_sweep: ron_conv_chain_forward / ron_conv_chain_backward planning / argument handling: %s\n", ron_last_error());
    return 1;
  }
  if (!quick) {
    trace_note("pass head_chain_arguments");
    if (head_chain_arguments()) {
      fprintf(stderr, "plan_sweep: ron_head_chain_forward / ron_head_chain_backward planning / argument handling: %s\n", ron_last_error());
      return 1;
    }
  }
  if (g_trace != nullptr) fclose(g_trace);
  printf("plan_sweep: %d contexts planned, no sanitizer report\n", runs);
  return 0;
}
