// A device scratch buffer that grows on demand and never shrinks (ym_embed's chunk partials, the scratch of ym_masks,
// ym_annotate, ym_mask_contours and ym_mask_rle).  Plain C++, no HIP: it reaches the device through the three functions
// below, which ym_runtime.cpp defines over hipMalloc, hipFree and hipDeviceSynchronize (tests/devbuf_check.cpp builds
// this header alone with a host compiler and defines them over malloc and free).
#pragma once
#include <cstddef>

// Each returns 0, or the status its definition already reported (the runtime's: ym_last_error names the failure).
// ym_dev_alloc's out-of-memory message opens with `what`, a printf format with exactly one "%zu", for the count `n`
// (a non-literal format: the compiler cannot check that, every caller of grow must).
__attribute__((visibility("hidden"))) int ym_dev_alloc(void** p, size_t bytes, const char* what, size_t n);
__attribute__((visibility("hidden"))) int ym_dev_free(void* p);
__attribute__((visibility("hidden"))) int ym_dev_sync();

struct __attribute__((visibility("hidden"))) DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)ym_dev_free(p); }
  // At least `need` bytes.  A buffer that has to grow is replaced, its contents dropped: an earlier launch on any
  // stream may still use the old one, so the device drains first.  On a failure the buffer is left empty, {nullptr, 0}
  // (never a freed pointer beside its old size), so the next call allocates again whatever it asks for.
  int grow(size_t need, const char* what, size_t n) {
    if (need <= bytes) return 0;
    if (p) {
      if (int rc = ym_dev_sync()) return rc;
      void* old = p;
      p = nullptr; bytes = 0;
      if (int rc = ym_dev_free(old)) return rc;
    }
    if (int rc = ym_dev_alloc(&p, need, what, n)) {
      p = nullptr;
      return rc;
    }
    bytes = need;
    return 0;
  }
};
