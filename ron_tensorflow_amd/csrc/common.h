// Shared host-side helpers of libron_hip.so (error reporting, HIP checks, the grid of a striding kernel, the workspace check).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <type_traits>

#include "../../include/ron_hip.h"

namespace ron {

// Thread-local message behind ron_last_error().
void set_error(const char* fmt, ...);

#define RON_HIP_CHECK(expr)                                                              \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      ron::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,    \
                     __LINE__);                                                          \
      return RON_ERR_HIP;                                                                \
    }                                                                                    \
  } while (0)

#define RON_REQUIRE(cond, ...)            \
  do {                                    \
    if (!(cond)) {                        \
      ron::set_error(__VA_ARGS__);        \
      return RON_ERR_INVALID;             \
    }                                     \
  } while (0)

static inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
// workgroups of 256 lanes for a kernel that strides over `total` items: at least one, at most `cap` (the training side's packs, sums
// and elementwise backwards: 4096; the forward boundary of elementwise.hip: 2048)
inline int grid_for(long long total, int cap = 256 * 16) { return (int)std::max<long long>(1, std::min<long long>((total + 255) / 256, cap)); }
// The workspace of a call: there, as large as `sizer` (the entry point that gives its size) says, 256-byte aligned.  `what` starts
// the messages.
inline int check_workspace(const char* what, const char* sizer, const void* workspace, int64_t bytes, int64_t needed) {
  RON_REQUIRE(workspace != nullptr && bytes >= needed, "%s: workspace of %lld bytes, %lld needed (%s)", what, (long long)bytes, (long long)needed, sizer);
  RON_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: the workspace must be 256-byte aligned", what);
  return RON_OK;
}

// Dry run (RON_PLAN_ONLY=1 in the environment, read once): every host-side decision of the library is made - launch plans, tile
// choices, split-K factors, kernel arguments, workspace sizes - but no HIP call: device "allocations" are distinct fake addresses
// nobody dereferences, copies, events and kernel launches are skipped.  What `make asan` (csrc/Makefile) runs the host planners
// under AddressSanitizer / UBSan with, on a machine without a GPU (tools/plan_sweep.cpp, tests/test_asan_plan_sweep.py).
bool plan_only();
hipError_t dev_malloc(void** p, size_t bytes);
hipError_t dev_free(void* p);
hipError_t dev_memset(void* p, int v, size_t bytes);                              // complete when it returns (waits for the null stream)
hipError_t dev_memset_async(void* p, int v, size_t bytes, hipStream_t s);
hipError_t dev_memcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
hipError_t dev_set_device(int device);
hipError_t launch_error();                     // hipGetLastError(), hipSuccess in a dry run
template <class T> hipError_t dev_malloc(T** p, size_t bytes) { return dev_malloc(reinterpret_cast<void**>(p), bytes); }

// Owner of one HIP object - a device allocation, a stream, an event: move-only, released by the destructor, so that an early return
// (RON_HIP_CHECK) or a destroyed context cannot leak it and nothing is released twice.
template <class T, hipError_t (*Release)(T)>
struct Owned {
  T p = nullptr;
  Owned() = default;
  Owned(Owned&& o) noexcept : p(o.p) { o.p = nullptr; }
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) { reset(); p = o.p; o.p = nullptr; }
    return *this;
  }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { reset(); }
  void reset() { if (p) (void)Release(p); p = nullptr; }
  T* put() { reset(); return &p; }      // for the call that creates the object: dev_malloc(b.put(), bytes), hipEventCreate(e.put())
  operator T() const { return p; }
  template <class U> U* as() const { return static_cast<U*>(p); }
};
using DevBuf = Owned<void*, dev_free>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
hipError_t dev_upload(DevBuf* b, const void* host, size_t bytes);      // a new allocation of `bytes` bytes holding the host data
hipError_t dev_stream_sync(hipStream_t s);

// A struct that reaches a kernel by value is defined between these two:
//
//   RON_KERNEL_ARGS_BEGIN
//   struct FooArgs { const float* p; int n; int fill_ = 0; };
//   RON_KERNEL_ARGS_END(FooArgs)
//
// In between, implicit padding - a hole or the tail - is a compile error (-Wpadded, raised where the struct's layout is first used,
// in the host and the device pass): what the compiler would pad becomes a named filler member where the padding was, so sizeof and
// every offset stay as they are.  A filler is 0: by its initialiser, or - ConvArgs and PatchArgs, which device code declares and
// which hold a bit-field filler - because every host object starts as T().  END declares the struct to trace_launch, which takes no
// other class type (found by argument-dependent lookup, so it works in any namespace; one BEGIN / END pair per struct).
#define RON_KERNEL_ARGS_BEGIN _Pragma("clang diagnostic push") _Pragma("clang diagnostic error \"-Wpadded\"")
#define RON_KERNEL_ARGS_END(T) \
  _Pragma("clang diagnostic pop") [[maybe_unused]] constexpr bool ron_kernel_args_declared(const T*) { return true; }
constexpr bool ron_kernel_args_declared(const volatile void*) { return false; }

// Launch trace of the dry run (RON_PLAN_TRACE=<file> beside RON_PLAN_ONLY=1): one line per skipped launch - the kernel as spelled at
// the RON_LAUNCH site, grid, block, dynamic LDS bytes and, per by-value argument, its size and the CRC32C of its sizeof bytes - and
// one per dev_memset_async.  Every hashed byte is the value of a member: scalars and pointers have no padding, and a class type has
// none because it was declared with RON_KERNEL_ARGS (anything else does not compile).  So the digest is a function of the argument
// VALUES alone - not of the compiler, its flags, or the copies and returns an argument went through on the way to the launch - and
// two trees whose traces are equal launch the same kernels with the same arguments wherever a launch is written
// (tools/plan_sweep.cpp, tests/test_plan_trace_cpu.py).  Nothing is evaluated outside the dry run.
FILE* plan_trace();      // the open trace file (appended to, line-buffered), or null
void trace_launch(const char* kernel, dim3 grid, dim3 block, size_t lds, int nargs, const size_t* sizes, const uint32_t* crcs);
template <class... A>
void trace_launch(const char* kernel, dim3 grid, dim3 block, size_t lds, hipStream_t, const A&... args) {
  static_assert(((!std::is_class<A>::value || ron_kernel_args_declared(static_cast<const A*>(nullptr))) && ...),
                "a struct passed to a kernel by value is defined between RON_KERNEL_ARGS_BEGIN and RON_KERNEL_ARGS_END (no padding)");
  const size_t sizes[] = {sizeof(A)..., 0};
  const uint32_t crcs[] = {ron_crc32c(&args, sizeof(A), 0)..., 0};
  trace_launch(kernel, grid, block, lds, (int)sizeof...(A), sizes, crcs);
}
#define RON_LAUNCH(kernel, ...)                                                  \
  do {                                                                           \
    if (!ron::plan_only()) hipLaunchKernelGGL(kernel, __VA_ARGS__);              \
    else if (ron::plan_trace()) ron::trace_launch(#kernel, __VA_ARGS__);         \
  } while (0)

// hipFuncSetAttribute applies to the current device only: one of these per kernel instantiation remembers on which
// devices (id < 64) the dynamic-LDS limit has been raised (or another per-device step, `once`, has been taken).  Safe from several host threads: nobody returns before the
// attribute is set on his device.
struct PerDeviceOnce {
  std::atomic<uint64_t> done{0};
  std::mutex mu;
  // f() once per device, again at the next call for as long as it fails; nothing is called in a dry run
  template <class F> hipError_t once(F f) {
    if (plan_only()) return hipSuccess;
    int dev = 0;
    const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev <= 63;     // unknown device: just do it again
    const uint64_t bit = known ? 1ull << dev : 0;
    if (known && (done.load(std::memory_order_acquire) & bit)) return hipSuccess;
    std::lock_guard<std::mutex> lock(mu);
    if (known && (done.load(std::memory_order_relaxed) & bit)) return hipSuccess;
    const hipError_t e = f();
    if (e == hipSuccess && known) done.fetch_or(bit, std::memory_order_release);
    return e;
  }
  hipError_t max_dynamic_lds(const void* kernel, int bytes) {
    return once([&]() { return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); });
  }
};

// ron_post_cfg::input_flags, internal bit (not in include/ron_hip.h; reserved there): the workspace's counters are zero on entry and
// ron_post_np leaves them zero (topk_nms_kernel cleans up after itself) - set by ron_detect for its context-owned workspace only
constexpr unsigned kPostWsClean = 0x40000000u;

// ron_tfe_cfg checks of ron_post_tfe (postproc.hip): RON_OK or RON_ERR_INVALID with the message set
int tfe_cfg_check(const ron_tfe_cfg* cfg);
// ron_detect_tfe's post stage (postproc.hip): the TF-evaluation lists of the context's raw heads (`heads`, n images) in the
// context's ron_post_np workspace (sized for max_batch), behind the np counters, its own counters laid out for max_batch and
// self-cleaning; zero_counters: they may hold something else (ron_detect wrote keys there since) and are zeroed first.
int post_tfe_ctx(const ron_heads* heads, int n, int max_batch, const ron_tfe_cfg* cfg, void* workspace, int64_t workspace_bytes,
                 bool zero_counters, float* scores, float* bboxes, hipStream_t stream);

// class ids the post-processing kernels group and encode (a power of two: label masks, anchor * kMaxClasses + label keys)
constexpr int kMaxClasses = RON_MAX_CLASSES;
static_assert((kMaxClasses & (kMaxClasses - 1)) == 0, "kMaxClasses must be a power of two");

// Makes `device` current for the lifetime of the guard and restores the caller's device afterwards.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int device) {
    if (plan_only()) return;
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != device) { err = hipSetDevice(device); switched = err == hipSuccess; }
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

}  // namespace ron
