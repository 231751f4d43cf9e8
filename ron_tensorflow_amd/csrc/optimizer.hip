// The training update (ron_optimizer_step): TensorFlow 1.x's dense apply kernels for the four rules tf_utils.configure_optimizer can
// give the RON training step (tf_utils.py:126-171) - GradientDescent, Momentum (use_nesterov=False), RMSProp, Adam - with the gradient
// of slim's l2_regularizer folded into the gradient, and that regulariser's value (the part of total_loss the losses do not hold).
//
//   g' = g + weight_decay w      (tensors with weight_decay != 0 only; otherwise the bits of g)
//   SGD       w = w - lr g'
//   MOMENTUM  m = momentum m + g';  w = w - lr m
//   RMSPROP   ms = ms + (1 - decay) (g' g' - ms);  mom = momentum mom + (lr g') / sqrt(ms + epsilon);  w = w - mom
//   ADAM      m = m + (1 - beta1) (g' - m);  v = v + (1 - beta2) (g' g' - v);  w = w - (lr_t m) / (sqrt(v) + epsilon)
//
// all fp32, one rounding per arithmetic sign in the order written (this file is compiled with -ffp-contract=off; the division and
// the square root are the correctly rounded ones), so that numpy reproduces every bit (tests/optim_ref.py).
//
// Bandwidth bound with many small tensors (most variables of a RON-320 context are 512-element vectors), so: every byte once, in as
// few launches as the list allows.  The list is cut into work units of kOptUnit elements that never straddle two tensors; a
// workgroup takes ONE unit (measured against a capped, striding grid: DESIGN.md 4.10).  The tensor table - pointers, counts, decay,
// first unit - travels BY VALUE in the kernel arguments, kOptEntries entries per launch (under 4 KiB with the scalars); a longer list
// is cut into consecutive launches of the same kernel.  Nothing is uploaded and nothing allocated; the pointers may change from call
// to call.  A workgroup finds its entry by a binary search over the first-unit column: uniform, so it stays in scalar registers.
//
// A lane moves 16 bytes per access while a whole float4 lies inside the tensor; the last count % 4 elements go one at a time, so no
// access touches a byte outside [ptr, ptr + count) and a neighbouring tensor may start 16 bytes behind the last whole vector.
//
// reg_loss: a unit leaves (0.5 weight_decay) sum(w^2) of its elements (the weights BEFORE the update; 0 without reading for an
// undecayed tensor) in the workspace: each lane adds its elements in order, the lanes of a wave meet in a shuffle tree, the four
// waves in LDS; one workgroup then adds the units' values (thread t those of units t, t + 256, ... in order, then the same tree).
// Every order is a function of the counts alone: the same inputs give the same bytes.  No atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "common.h"

namespace ron {
namespace {

constexpr int kOptThreads = 256;
constexpr int kOptVecs = 4;                                   // float4 accesses per lane and tensor kind
constexpr int kOptUnit = kOptThreads * 4 * kOptVecs;          // elements per work unit
constexpr int kOptEntries = 64;                               // table entries per launch
// Workgroups per launch: 0 = one per work unit (the default: the faster of the two on the RON-320 lists); N = at
// most N, striding over the units (the guide's rule for memory-bound kernels is 8 per CU = 2048; what -DRON_OPT_GRID_CAP=2048 builds)
#ifndef RON_OPT_GRID_CAP
#define RON_OPT_GRID_CAP 0
#endif
constexpr unsigned kOptGridCap = RON_OPT_GRID_CAP;
constexpr int kOptMaxTensors = 4096;
constexpr int64_t kOptMaxCount = (int64_t)1 << 40;
constexpr int64_t kOptMaxUnits = (int64_t)1 << 22;            // per list: 2^34 elements, and a grid far inside every limit

RON_KERNEL_ARGS_BEGIN      // (a member of OptArgs)
struct OptEntry {
  float* var;
  const float* grad;
  float* slot0;
  float* slot1;
  long long count;
  float weight_decay;
  unsigned first_unit;          // of this entry, within the launch
};
RON_KERNEL_ARGS_END(OptEntry)
static_assert(sizeof(OptEntry) == 48, "the table is laid out for 48-byte entries");

RON_KERNEL_ARGS_BEGIN
struct OptArgs {
  OptEntry t[kOptEntries];
  float* partial;               // workspace: one float per unit of the whole list (WANT_REG only)
  float lr;                     // Adam: lr_t
  float momentum;
  float om0, om1;               // 1 - decay (RMSProp); 1 - beta1, 1 - beta2 (Adam)
  float epsilon;
  int n;                        // entries in use
  unsigned unit_base;           // the launch's first unit within the list
  unsigned units;               // of the launch
};
RON_KERNEL_ARGS_END(OptArgs)
static_assert(sizeof(OptArgs) <= 4096 - 256, "the kernel arguments must stay under 4 KiB with the hidden ones");

// the rule on one element; g is g'
template <int RULE>
__device__ __forceinline__ void opt_rule(const OptArgs& a, float& w, float g, float& s0, float& s1) {
  if (RULE == RON_OPT_SGD) {
    w = w - a.lr * g;
  } else if (RULE == RON_OPT_MOMENTUM) {
    s0 = a.momentum * s0 + g;
    w = w - a.lr * s0;
  } else if (RULE == RON_OPT_RMSPROP) {
    s0 = s0 + a.om0 * (g * g - s0);
    s1 = a.momentum * s1 + (a.lr * g) / sqrtf(s0 + a.epsilon);
    w = w - s1;
  } else {
    s0 = s0 + a.om0 * (g - s0);
    s1 = s1 + a.om1 * (g * g - s1);
    w = w - (a.lr * s0) / (sqrtf(s1) + a.epsilon);
  }
}

template <int RULE, bool WANT_REG>
__device__ __forceinline__ void opt_element(const OptArgs& a, bool decay, float wd, float& w, float g, float& s0, float& s1, float& sq) {
  if (WANT_REG && decay) sq = sq + w * w;
  if (decay) g = g + wd * w;
  opt_rule<RULE>(a, w, g, s0, s1);
}

__device__ __forceinline__ float opt_block_sum(float v, float* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const float sum = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();          // sh is free again: a workgroup may take another unit
  return sum;
}

// one work unit of the launch
template <int RULE, bool WANT_REG>
__device__ __forceinline__ void opt_unit(const OptArgs& a, unsigned unit, float* sh) {
  constexpr bool S0 = RULE != RON_OPT_SGD, S1 = RULE == RON_OPT_RMSPROP || RULE == RON_OPT_ADAM;
  int lo = 0, hi = a.n;                          // t[lo].first_unit <= unit < t[hi].first_unit (t[n]: the launch's unit count)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.t[mid].first_unit <= unit) lo = mid; else hi = mid;
  }
  const long long base = (long long)(unit - a.t[lo].first_unit) * kOptUnit;
  const long long left = a.t[lo].count - base;
  const int len = left < kOptUnit ? (int)left : kOptUnit;
  const float wd = a.t[lo].weight_decay;
  const bool decay = wd != 0.f;
  float* const w = a.t[lo].var + base;
  const float* const g = a.t[lo].grad + base;
  float* const s0 = S0 ? a.t[lo].slot0 + base : nullptr;
  float* const s1 = S1 ? a.t[lo].slot1 + base : nullptr;
  const int tid = threadIdx.x;
  float sq = 0.f;
  if (len == kOptUnit) {
    float4 vw[kOptVecs], vg[kOptVecs], v0[kOptVecs], v1[kOptVecs];
#pragma unroll
    for (int v = 0; v < kOptVecs; ++v) {
      const int i = (v * kOptThreads + tid) * 4;
      vw[v] = *reinterpret_cast<const float4*>(w + i);
      vg[v] = *reinterpret_cast<const float4*>(g + i);
      v0[v] = S0 ? *reinterpret_cast<const float4*>(s0 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
      v1[v] = S1 ? *reinterpret_cast<const float4*>(s1 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int v = 0; v < kOptVecs; ++v) {
      const int i = (v * kOptThreads + tid) * 4;
      opt_element<RULE, WANT_REG>(a, decay, wd, vw[v].x, vg[v].x, v0[v].x, v1[v].x, sq);
      opt_element<RULE, WANT_REG>(a, decay, wd, vw[v].y, vg[v].y, v0[v].y, v1[v].y, sq);
      opt_element<RULE, WANT_REG>(a, decay, wd, vw[v].z, vg[v].z, v0[v].z, v1[v].z, sq);
      opt_element<RULE, WANT_REG>(a, decay, wd, vw[v].w, vg[v].w, v0[v].w, v1[v].w, sq);
      *reinterpret_cast<float4*>(w + i) = vw[v];
      if (S0) *reinterpret_cast<float4*>(s0 + i) = v0[v];
      if (S1) *reinterpret_cast<float4*>(s1 + i) = v1[v];
    }
  } else {
    for (int v = 0; v < kOptVecs; ++v) {
      const int i = (v * kOptThreads + tid) * 4;
      if (i + 4 <= len) {
        float4 vw = *reinterpret_cast<const float4*>(w + i);
        const float4 vg = *reinterpret_cast<const float4*>(g + i);
        float4 v0 = S0 ? *reinterpret_cast<const float4*>(s0 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 v1 = S1 ? *reinterpret_cast<const float4*>(s1 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        opt_element<RULE, WANT_REG>(a, decay, wd, vw.x, vg.x, v0.x, v1.x, sq);
        opt_element<RULE, WANT_REG>(a, decay, wd, vw.y, vg.y, v0.y, v1.y, sq);
        opt_element<RULE, WANT_REG>(a, decay, wd, vw.z, vg.z, v0.z, v1.z, sq);
        opt_element<RULE, WANT_REG>(a, decay, wd, vw.w, vg.w, v0.w, v1.w, sq);
        *reinterpret_cast<float4*>(w + i) = vw;
        if (S0) *reinterpret_cast<float4*>(s0 + i) = v0;
        if (S1) *reinterpret_cast<float4*>(s1 + i) = v1;
      } else {
        for (int j = i; j < len; ++j) {          // the last count % 4 elements (nothing when i >= len)
          float ew = w[j], e0 = S0 ? s0[j] : 0.f, e1 = S1 ? s1[j] : 0.f;
          opt_element<RULE, WANT_REG>(a, decay, wd, ew, g[j], e0, e1, sq);
          w[j] = ew;
          if (S0) s0[j] = e0;
          if (S1) s1[j] = e1;
        }
      }
    }
  }
  if (WANT_REG) {
    const float sum = opt_block_sum(sq, sh);
    if (tid == 0) a.partial[(long long)a.unit_base + unit] = (0.5f * wd) * sum;
  }
}

// a workgroup takes units blockIdx.x, blockIdx.x + gridDim.x, ...: ONE each with the grid run_opt launches (kOptGridCap)
template <int RULE, bool WANT_REG>
__global__ __launch_bounds__(kOptThreads) void opt_apply_kernel(const OptArgs a) {
  __shared__ float sh[4];
  for (unsigned unit = blockIdx.x; unit < a.units; unit += gridDim.x) opt_unit<RULE, WANT_REG>(a, unit, sh);
}

// one workgroup: reg_loss = the units' values, thread t adding those of units t, t + 256, ... in order, then the tree of a unit
__global__ __launch_bounds__(kOptThreads) void opt_reg_final_kernel(const float* __restrict__ partial, long long units, float* __restrict__ reg_loss) {
  __shared__ float sh[4];
  float acc = 0.f;
  for (long long u = threadIdx.x; u < units; u += kOptThreads) acc = acc + partial[u];
  const float sum = opt_block_sum(acc, sh);
  if (threadIdx.x == 0) *reg_loss = sum;
}

struct OptPlan {
  int launches = 0;
  int64_t units = 0;
  int64_t workspace = 0;
};

// what depends on the counts alone: the units, the cut into launches, the workspace
int plan_opt(const char* what, const ron_opt_tensor* t, int n, OptPlan* P) {
  RON_REQUIRE(n >= 1 && n <= kOptMaxTensors, "%s: %d tensors, 1 to %d are accepted", what, n, kOptMaxTensors);
  RON_REQUIRE(t != nullptr, "%s: NULL tensor table", what);
  int64_t units = 0;
  for (int i = 0; i < n; ++i) {
    RON_REQUIRE(t[i].count >= 1, "%s: tensor %d: count %lld must be at least 1", what, i, (long long)t[i].count);
    RON_REQUIRE(t[i].count <= kOptMaxCount, "%s: tensor %d: count %lld is beyond 2^40", what, i, (long long)t[i].count);
    units += (t[i].count + kOptUnit - 1) / kOptUnit;
  }
  RON_REQUIRE(units <= kOptMaxUnits, "%s: %lld work units of %d elements, at most %lld per list", what, (long long)units, kOptUnit,
              (long long)kOptMaxUnits);
  P->launches = (n + kOptEntries - 1) / kOptEntries;
  P->units = units;
  P->workspace = align_up(units * 4, 256);
  return RON_OK;
}

int need_slots(int rule) { return rule == RON_OPT_SGD ? 0 : (rule == RON_OPT_MOMENTUM ? 1 : 2); }

int check_cfg(const char* what, const ron_opt_cfg* c, float learning_rate, int64_t step) {
  RON_REQUIRE(c != nullptr, "%s: NULL configuration", what);
  RON_REQUIRE(c->rule >= RON_OPT_SGD && c->rule <= RON_OPT_ADAM, "%s: unknown rule %d (sgd 0, momentum 1, rmsprop 2, adam 3)", what, c->rule);
  RON_REQUIRE(std::isfinite(learning_rate), "%s: the learning rate %g must be finite", what, (double)learning_rate);
  RON_REQUIRE(c->momentum >= 0.f && c->momentum <= 1.f, "%s: momentum %g must lie in [0, 1]", what, (double)c->momentum);
  RON_REQUIRE(c->decay >= 0.f && c->decay <= 1.f, "%s: decay %g must lie in [0, 1]", what, (double)c->decay);
  RON_REQUIRE(c->beta1 >= 0.f && c->beta1 <= 1.f, "%s: beta1 %g must lie in [0, 1]", what, (double)c->beta1);
  RON_REQUIRE(c->beta2 >= 0.f && c->beta2 <= 1.f, "%s: beta2 %g must lie in [0, 1]", what, (double)c->beta2);
  RON_REQUIRE(std::isfinite(c->epsilon) && c->epsilon >= 0.f, "%s: epsilon %g must be finite and >= 0", what, (double)c->epsilon);
  if (c->rule == RON_OPT_ADAM) {
    RON_REQUIRE(c->beta1 < 1.f && c->beta2 < 1.f, "%s: adam: beta1 %g and beta2 %g must be below 1 (the bias correction divides by 1 - beta1^step)",
                what, (double)c->beta1, (double)c->beta2);
    RON_REQUIRE(step >= 1, "%s: adam: step %lld must be at least 1", what, (long long)step);
  }
  return RON_OK;
}

int check_tensors(const char* what, int rule, const ron_opt_tensor* t, int n) {
  const int slots = need_slots(rule);
  uintptr_t vars[kOptMaxTensors];
  for (int i = 0; i < n; ++i) {
    const ron_opt_tensor& e = t[i];
    RON_REQUIRE(e.var != nullptr && e.grad != nullptr, "%s: tensor %d: var and grad must not be NULL", what, i);
    RON_REQUIRE(slots < 1 || e.slot0 != nullptr, "%s: tensor %d: the rule needs slot0 and it is NULL", what, i);
    RON_REQUIRE(slots < 2 || e.slot1 != nullptr, "%s: tensor %d: the rule needs slot1 and it is NULL", what, i);
    const uintptr_t s0 = slots >= 1 ? (uintptr_t)e.slot0 : 0, s1 = slots >= 2 ? (uintptr_t)e.slot1 : 0;
    RON_REQUIRE((((uintptr_t)e.var | (uintptr_t)e.grad | s0 | s1) & 15) == 0,
                "%s: tensor %d: var, grad and the slots must be 16-byte aligned (16 bytes per access)", what, i);
    RON_REQUIRE(std::isfinite(e.weight_decay) && e.weight_decay >= 0.f, "%s: tensor %d: weight_decay %g must be finite and >= 0", what, i,
                (double)e.weight_decay);
    RON_REQUIRE((uintptr_t)e.var != (uintptr_t)e.grad, "%s: tensor %d: var is its own grad", what, i);
    RON_REQUIRE((uintptr_t)e.var != s0 && (uintptr_t)e.var != s1, "%s: tensor %d: var is its own slot", what, i);
    vars[i] = (uintptr_t)e.var;
  }
  std::sort(vars, vars + n);
  RON_REQUIRE(std::adjacent_find(vars, vars + n) == vars + n, "%s: a var appears twice in the list (it would be updated twice)", what);
  return RON_OK;
}

template <int RULE, bool WANT_REG>
int run_opt(const OptArgs& scalars, const ron_opt_tensor* t, int n, const OptPlan& P, float* reg_loss, hipStream_t s) {
  OptArgs a = scalars;
  unsigned unit_base = 0;
  for (int first = 0; first < n; first += kOptEntries) {
    const int m = std::min(kOptEntries, n - first);
    unsigned units = 0;
    for (int i = 0; i < kOptEntries; ++i) {
      const ron_opt_tensor& e = t[first + std::min(i, m - 1)];          // (the unused entries repeat the last one: never indexed)
      a.t[i] = OptEntry{e.var, e.grad, RULE != RON_OPT_SGD ? e.slot0 : nullptr,
                        RULE == RON_OPT_RMSPROP || RULE == RON_OPT_ADAM ? e.slot1 : nullptr, (long long)e.count, e.weight_decay, units};
      if (i < m) units += (unsigned)((e.count + kOptUnit - 1) / kOptUnit);
    }
    a.n = m;
    a.unit_base = unit_base;
    a.units = units;
    const unsigned grid = kOptGridCap != 0 && units > kOptGridCap ? kOptGridCap : units;
    RON_LAUNCH((opt_apply_kernel<RULE, WANT_REG>), dim3(grid), dim3(kOptThreads), 0, s, a);
    unit_base += units;
  }
  if (WANT_REG) RON_LAUNCH(opt_reg_final_kernel, dim3(1), dim3(kOptThreads), 0, s, a.partial, (long long)P.units, reg_loss);
  RON_HIP_CHECK(ron::launch_error());
  return RON_OK;
}

template <int RULE>
int run_opt_rule(const OptArgs& a, const ron_opt_tensor* t, int n, const OptPlan& P, float* reg_loss, hipStream_t s) {
  return reg_loss != nullptr ? run_opt<RULE, true>(a, t, n, P, reg_loss, s) : run_opt<RULE, false>(a, t, n, P, nullptr, s);
}

}  // namespace
}  // namespace ron

extern "C" int ron_optimizer_plan(const ron_opt_tensor* t, int n, int64_t out[4]) {
  using namespace ron;
  OptPlan P;
  if (int rc = plan_opt("optimizer plan", t, n, &P)) return rc;
  RON_REQUIRE(out != nullptr, "optimizer plan: NULL output");
  out[0] = P.launches;
  out[1] = P.units;
  out[2] = kOptEntries;
  out[3] = kOptUnit;
  return RON_OK;
}

extern "C" int64_t ron_optimizer_workspace_bytes(const ron_opt_tensor* t, int n) {
  ron::OptPlan P;
  if (ron::plan_opt("optimizer", t, n, &P) != RON_OK) return -1;
  return P.workspace;
}

extern "C" int ron_optimizer_step(const ron_opt_cfg* cfg, const ron_opt_tensor* t, int n, float learning_rate, int64_t step, float* reg_loss,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace ron;
  const char* what = "optimizer step";
  if (int rc = check_cfg(what, cfg, learning_rate, step)) return rc;
  OptPlan P;
  if (int rc = plan_opt(what, t, n, &P)) return rc;
  if (int rc = check_tensors(what, cfg->rule, t, n)) return rc;
  OptArgs a = {};
  if (reg_loss != nullptr) {
    RON_REQUIRE(((uintptr_t)reg_loss & 3) == 0, "%s: reg_loss must be 4-byte aligned", what);
    RON_REQUIRE(workspace != nullptr && workspace_bytes >= P.workspace,
                "%s: workspace of %lld bytes, %lld needed with reg_loss (ron_optimizer_workspace_bytes)", what, (long long)workspace_bytes,
                (long long)P.workspace);
    RON_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: the workspace must be 256-byte aligned", what);
    a.partial = static_cast<float*>(workspace);
  }
  a.lr = learning_rate;
  a.momentum = cfg->momentum;
  a.epsilon = cfg->epsilon;
  hipStream_t s = (hipStream_t)stream;
  switch (cfg->rule) {
    case RON_OPT_SGD: return run_opt_rule<RON_OPT_SGD>(a, t, n, P, reg_loss, s);
    case RON_OPT_MOMENTUM: return run_opt_rule<RON_OPT_MOMENTUM>(a, t, n, P, reg_loss, s);
    case RON_OPT_RMSPROP:
      a.om0 = 1.0f - cfg->decay;
      return run_opt_rule<RON_OPT_RMSPROP>(a, t, n, P, reg_loss, s);
    default: {
      a.om0 = 1.0f - cfg->beta1;
      a.om1 = 1.0f - cfg->beta2;
      // lr_t in double, rounded to fp32 once (TensorFlow forms it from fp32 pieces on the host; here the whole factor is exact first)
      const double b1 = cfg->beta1, b2 = cfg->beta2, k = (double)step;
      a.lr = (float)((double)learning_rate * std::sqrt(1.0 - std::pow(b2, k)) / (1.0 - std::pow(b1, k)));
      return run_opt_rule<RON_OPT_ADAM>(a, t, n, P, reg_loss, s);
    }
  }
}
