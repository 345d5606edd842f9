// Process-wide error string + ABI version of libpfst_hip.so.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include "../../include/pfst_hip.h"

static char g_err[512] = "no error";

void pfst_set_error(const char* file, int line, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s:%d: %s", file, line, msg);
}

// Deterministic mode (pfst_set_deterministic): every sum that is normally completed by fp32 / fp64 atomic adds of several workgroups -- the
// split-K slices of the weight gradients, the BatchNorm-backward reductions, the depthwise and bias gradients, PFGSTLoss's source statistics --
// goes through per-workgroup (per grid slice) partials in a scratch and is added up by a second kernel in index order (det.h, bn.hip,
// dwconv.hip): same launch shapes, no sum depends on which workgroup finishes first.  +3 % on the b = 8 x 1024^2 step; the gradient of a step is
// bit-identical run to run and for any stream schedule (tests/test_deterministic_gpu.py, tools/det_repro_fullsize.py).
static int g_deterministic = 0;
int pfst_deterministic(void) { return g_deterministic; }
extern "C" int pfst_set_deterministic(int on) {
  g_deterministic = on != 0;
  return 0;
}
extern "C" int pfst_get_deterministic(void) { return g_deterministic; }

// Scratch of the deterministic mode's partial sums (the only memory the library allocates itself; nothing outside that mode touches it): one
// grow-only buffer per (device, stream) -- a launcher fills it, a second kernel of the same launcher reduces it, both queued on that stream.
// The table has a fixed number of slots; a launch on a stream beyond them takes the least recently used slot over.  On failure the message
// names this scratch (pfst_last_error) and the launcher returns PFST_ERR_LAUNCH without a message of its own (PFST_CHECK_DET).
static void* det_scratch_fail(int line, const char* what, size_t bytes, hipError_t e) {
  char msg[256];
  snprintf(msg, sizeof(msg), "deterministic-mode scratch of %zu bytes: %s failed (%s)", bytes, what, hipGetErrorString(e));
  pfst_set_error(__FILE__, line, msg);
  return nullptr;
}

void* pfst_det_scratch(size_t bytes, void* stream) {
  constexpr int kSlots = 8;
  struct Slot { int dev; void* stream; void* buf; size_t cap; unsigned long long used; };
  static Slot slots[kSlots];
  static unsigned long long clock = 0;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  // The key holds the device as well as the stream: the default stream's handle (NULL) is the same number on every device.  (A one-GPU test
  // box cannot tell the two halves of the key apart; tests/test_deterministic_kernels_gpu.py covers the stream half.)
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return det_scratch_fail(__LINE__, "hipGetDevice", bytes, e);
  int at = -1;
  for (int i = 0; i < kSlots && at < 0; ++i)
    if (slots[i].buf && slots[i].dev == dev && slots[i].stream == stream) at = i;
  for (int i = 0; i < kSlots && at < 0; ++i)
    if (!slots[i].buf) at = i;
  if (at < 0) {
    // every slot is held: evict the least recently used one.  Its stream may have been destroyed since, so wait for all work of its device
    // (which may still read the buffer) rather than for that stream.
    at = 0;
    for (int i = 1; i < kSlots; ++i)
      if (slots[i].used < slots[at].used) at = i;
    if (slots[at].dev != dev && (e = hipSetDevice(slots[at].dev)) != hipSuccess) return det_scratch_fail(__LINE__, "hipSetDevice", bytes, e);
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipFree(slots[at].buf);
    const hipError_t e_back = slots[at].dev != dev ? hipSetDevice(dev) : hipSuccess;
    if (e != hipSuccess) return det_scratch_fail(__LINE__, "eviction (hipDeviceSynchronize / hipFree)", bytes, e);
    if (e_back != hipSuccess) return det_scratch_fail(__LINE__, "hipSetDevice", bytes, e_back);
    slots[at] = Slot{};
  }
  Slot& sl = slots[at];
  if (sl.cap < bytes) {
    if (sl.buf) {
      if ((e = hipDeviceSynchronize()) != hipSuccess)                 // earlier launches may still read the old buffer
        return det_scratch_fail(__LINE__, "hipDeviceSynchronize before regrowth", bytes, e);
      (void)hipFree(sl.buf);
      sl = Slot{};
    }
    const size_t cap = bytes < (size_t(8) << 20) ? (size_t(8) << 20) : bytes + bytes / 2;
    if ((e = hipMalloc(&sl.buf, cap)) != hipSuccess) {
      sl = Slot{};
      return det_scratch_fail(__LINE__, "hipMalloc", bytes, e);
    }
    sl.cap = cap;
  }
  sl.dev = dev;
  sl.stream = stream;
  sl.used = ++clock;
  return sl.buf;
}

extern "C" const char* pfst_last_error(void) { return g_err; }
extern "C" int pfst_abi_version(void) { return 1; }
