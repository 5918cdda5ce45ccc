// devbuf_check: the grow-on-demand device buffer (csrc/ym_devbuf.h DevBuf) over a fake device — malloc / free, every
// call logged, an allocation failure on request.  Checks, in this order: a grow to a smaller or equal size neither
// syncs nor reallocates; a larger grow syncs, then frees, then allocates; after a failed allocation the buffer is
// {nullptr, 0} and the status is YM_ENOMEM; a following SMALLER request allocates again (a buffer that kept its old
// size beside the freed pointer would hand that pointer out: what ym_masks' scratch once did); the destructor frees
// exactly once, and an empty buffer's not at all.  Prints "OK" (exit 0) or the failed check (exit 1).  Host-only;
// tests/test_devbuf_host.py builds it with the sanitizers, so a double free or a use of the freed block fails too.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../include/yolomi.h"
#include "../yolo-infer_amd/csrc/ym_devbuf.h"

static std::string g_log;       // 's' sync, 'f' free, 'a' allocation, 'x' failed allocation
static bool g_fail_next = false;
static std::string g_what;      // the message opening the last failed allocation was given
static int g_live = 0;          // blocks allocated and not freed

int ym_dev_alloc(void** p, size_t bytes, const char* what, size_t n) {
  if (g_fail_next) {
    g_fail_next = false;
    g_log += 'x';
    g_what = what + std::to_string(n);
    *p = reinterpret_cast<void*>(0x10);  // what a failed allocation may leave behind: never to be kept
    return YM_ENOMEM;
  }
  g_log += 'a';
  *p = malloc(bytes);
  ++g_live;
  return 0;
}
int ym_dev_free(void* p) {
  g_log += 'f';
  free(p);
  --g_live;
  return 0;
}
int ym_dev_sync() {
  g_log += 's';
  return 0;
}

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      printf("line %d: %s (log \"%s\")\n", __LINE__, #cond, g_log.c_str()); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

static int run() {
  {
    DevBuf b;
    CHECK(b.p == nullptr && b.bytes == 0);
    CHECK(b.grow(0, "zero", 0) == 0 && g_log == "");  // nothing asked for, nothing done
    CHECK(b.grow(100, "first", 100) == 0 && g_log == "a");  // no old buffer: nothing to drain or free
    CHECK(b.p && b.bytes == 100 && g_live == 1);
    memset(b.p, 0xab, 100);
    void* const first = b.p;
    CHECK(b.grow(100, "equal", 100) == 0 && b.grow(7, "smaller", 7) == 0 && g_log == "a");
    CHECK(b.p == first && b.bytes == 100);
    CHECK(b.grow(1000, "larger", 1000) == 0 && g_log == "asfa");  // sync, then free, then allocate
    CHECK(b.p && b.bytes == 1000 && g_live == 1);
    memset(b.p, 0xcd, 1000);
    g_fail_next = true;
    CHECK(b.grow(5000, "too large", 5000) == YM_ENOMEM && g_log == "asfasfx" && g_what == "too large5000");
    CHECK(b.p == nullptr && b.bytes == 0 && g_live == 0);
    CHECK(b.grow(10, "small again", 10) == 0 && g_log == "asfasfxa");  // allocates: no stale size to succeed on
    CHECK(b.p && b.bytes == 10 && g_live == 1);
    memset(b.p, 0xef, 10);
  }
  CHECK(g_log == "asfasfxaf" && g_live == 0);  // the destructor: one free, no sync
  {
    DevBuf empty;
    g_fail_next = true;
    CHECK(empty.grow(1, "never", 1) == YM_ENOMEM && empty.p == nullptr && empty.bytes == 0);
  }
  CHECK(g_log == "asfasfxafx" && g_live == 0);  // an empty buffer frees nothing
  return 0;
}

int main() {
  if (run()) return 1;
  printf("OK\n");
  return 0;
}
