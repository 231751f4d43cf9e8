#include <stdlib.h>
#include <string.h>
#include "common.h"

namespace ron {
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const char* get_error() { return g_err; }

bool plan_only() {
  static const bool on = getenv("RON_PLAN_ONLY") != nullptr;
  return on;
}
// dry run: addresses from a counter (4 KB apart at least, never handed to HIP, never dereferenced on the host)
static std::atomic<uint64_t> g_fake_next{0x100000000ull};
hipError_t dev_malloc(void** p, size_t bytes) {
  if (!plan_only()) return hipMalloc(p, bytes);
  *p = reinterpret_cast<void*>(g_fake_next.fetch_add((uint64_t)align_up((int64_t)bytes + 1, 4096)));
  return hipSuccess;
}
hipError_t dev_free(void* p) { return plan_only() ? hipSuccess : hipFree(p); }
// hipMemset on device memory only ENQUEUES on the null stream (measured: with the null stream busy it returns at once, the memory
// still unset; tests/test_gpu_stream_order.py).  Callers of this one zero memory at set-up and hand it to streams that do not wait
// for the null stream (ron_clone: a slot used at once on a non-blocking stream), so it returns when the memory is zero.
hipError_t dev_memset(void* p, int v, size_t bytes) {
  if (plan_only()) return hipSuccess;
  const hipError_t e = hipMemset(p, v, bytes);
  return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}
FILE* plan_trace() {
  static FILE* const f = [] {
    const char* path = plan_only() ? getenv("RON_PLAN_TRACE") : nullptr;
    FILE* t = path != nullptr ? fopen(path, "a") : nullptr;
    if (t != nullptr) setvbuf(t, nullptr, _IOLBF, 0);      // whole lines: the sweep appends its headings to the same file
    return t;
  }();
  return f;
}
void trace_launch(const char* kernel, dim3 grid, dim3 block, size_t lds, int nargs, const size_t* sizes, const uint32_t* crcs) {
  std::string line = kernel;
  char buf[96];
  snprintf(buf, sizeof buf, " grid %u %u %u block %u %u %u lds %zu args", grid.x, grid.y, grid.z, block.x, block.y, block.z, lds);
  line += buf;
  for (int i = 0; i < nargs; ++i) { snprintf(buf, sizeof buf, " %zu:%08x", sizes[i], crcs[i]); line += buf; }
  fprintf(plan_trace(), "%s\n", line.c_str());
}
hipError_t dev_memset_async(void* p, int v, size_t bytes, hipStream_t s) {
  if (!plan_only()) return hipMemsetAsync(p, v, bytes, s);
  if (plan_trace()) fprintf(plan_trace(), "memset %p value %d bytes %zu\n", p, v, bytes);
  return hipSuccess;
}
hipError_t dev_stream_sync(hipStream_t s) { return plan_only() ? hipSuccess : hipStreamSynchronize(s); }
hipError_t dev_memcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  return plan_only() ? hipSuccess : hipMemcpy(dst, src, bytes, kind);
}
hipError_t dev_upload(DevBuf* b, const void* host, size_t bytes) {
  const hipError_t e = dev_malloc(b->put(), bytes);
  return e != hipSuccess ? e : dev_memcpy(b->p, host, bytes, hipMemcpyHostToDevice);
}
hipError_t dev_set_device(int device) { return plan_only() ? hipSuccess : hipSetDevice(device); }
hipError_t launch_error() { return plan_only() ? hipSuccess : hipGetLastError(); }
}  // namespace ron

extern "C" const char* ron_last_error(void) { return ron::get_error(); }
extern "C" int ron_abi_version(void) { return 2; }   // 2: ron_conv_desc.center_from, RON_DTYPE_F16X3, ron_num_grouped_launches

// CRC32C (Castagnoli, reflected 0x82F63B78), slicing-by-8 on the host: the checksum of TensorFlow's tensor-bundle files
// (ron_tensorflow_amd/checkpoint.py); `crc` chains calls (0 for the first).
extern "C" uint32_t ron_crc32c(const void* data, uint64_t nbytes, uint32_t crc) {
  static uint32_t tab[8][256];
  static bool ready = false;
  if (!ready) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
      tab[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int t = 1; t < 8; ++t) tab[t][i] = (tab[t - 1][i] >> 8) ^ tab[0][tab[t - 1][i] & 0xFF];
    ready = true;
  }
  const unsigned char* p = static_cast<const unsigned char*>(data);
  crc = ~crc;
  while (nbytes >= 8) {
    uint32_t lo, hi;
    memcpy(&lo, p, 4);
    memcpy(&hi, p + 4, 4);
    lo ^= crc;
    crc = tab[7][lo & 0xFF] ^ tab[6][(lo >> 8) & 0xFF] ^ tab[5][(lo >> 16) & 0xFF] ^ tab[4][lo >> 24] ^
          tab[3][hi & 0xFF] ^ tab[2][(hi >> 8) & 0xFF] ^ tab[1][(hi >> 16) & 0xFF] ^ tab[0][hi >> 24];
    p += 8;
    nbytes -= 8;
  }
  while (nbytes--) crc = tab[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8);
  return ~crc;
}
