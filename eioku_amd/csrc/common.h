// Shared host-side plumbing for libeioku_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/eioku_hip.h"

namespace eioku {

void set_error(const char* fmt, ...);
bool initialised();
int num_cus();

// Scratch device buffer owned by the library, grown on demand (EIOKU_MEM_HOST staging and
// per-call workspaces).  Slot ids keep independent users from aliasing each other.
enum ScratchSlot { kSlotIn = 0, kSlotPrev, kSlotOut, kSlotWork0, kSlotWork1, kSlotWork2, kNumSlots };
void* scratch(ScratchSlot slot, size_t bytes);  // nullptr + error set on failure

// hipEvent brackets around tagged kernel launches (no-ops unless eioku_prof_enable(1)).
void prof_start(int tag, hipStream_t stream);
void prof_stop(int tag, hipStream_t stream);
bool prof_enabled();

// Environment switches ("r3 — switches").  env_off(X): X is set to a value atoi() reads as 0 -- the one form
// of an off switch; env_num(X, d): X as a number, d when unset.  Callers keep the result in a function-local static:
// every switch is read once per process.
bool env_off(const char* name);
double env_num(const char* name, double dflt);

}  // namespace eioku

#define EIOKU_HIP_CHECK(expr)                                                                  \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      ::eioku::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,      \
                         __LINE__);                                                            \
      return EIOKU_EHIP;                                                                       \
    }                                                                                          \
  } while (0)

#define EIOKU_REQUIRE(cond, ...)          \
  do {                                    \
    if (!(cond)) {                        \
      ::eioku::set_error(__VA_ARGS__);    \
      return EIOKU_EINVAL;                \
    }                                     \
  } while (0)

#define EIOKU_REQUIRE_INIT()                                                \
  do {                                                                      \
    if (!::eioku::initialised()) {                                          \
      ::eioku::set_error("eioku_init() has not been called");               \
      return EIOKU_ENODEV;                                                  \
    }                                                                       \
  } while (0)

// Launch-error check that does not synchronise.
#define EIOKU_LAUNCH_CHECK() EIOKU_HIP_CHECK(hipGetLastError())

// Pass a callee's error code up unchanged.
#define EIOKU_TRY(expr)                \
  do {                                 \
    const int _rc = (expr);            \
    if (_rc != EIOKU_OK) return _rc;   \
  } while (0)

namespace eioku {

// An owning device buffer of `cap` elements: freed by its destructor, moved but never copied.  grow(n) reallocates (and
// drops the contents) only when n exceeds the capacity; it does not synchronise.  A failed allocation leaves the buffer
// empty (p == nullptr, cap == 0), so the handle that holds it can be used again or destroyed.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    return *this;
  }
  ~DevBuf() { reset(); }
  operator T*() const { return p; }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr, cap = 0;
  }
  int grow(size_t n) {
    if (p && n <= cap) return EIOKU_OK;
    reset();
    if (hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)) != hipSuccess) {
      p = nullptr;
      set_error("hipMalloc of %zu bytes failed", n * sizeof(T));
      return EIOKU_ENOMEM;
    }
    cap = n;
    return EIOKU_OK;
  }
  // allocate on first use, then a synchronous copy of n host elements
  int upload(const T* host, size_t n) {
    EIOKU_TRY(grow(n));
    if (n) EIOKU_HIP_CHECK(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
    return EIOKU_OK;
  }
};

// For handles whose launches may still be in flight when a call regrows a buffer: wait for the device before the old
// memory is freed.  No-op, and no wait, while the buffer is large enough.
template <typename T>
int grow_synced(DevBuf<T>& b, size_t n) {
  if (b.p && b.cap < n) (void)hipDeviceSynchronize();
  return b.grow(n);
}

static_assert(!std::is_copy_constructible<DevBuf<int>>::value, "DevBuf owns its memory");
static_assert(std::is_nothrow_move_constructible<DevBuf<int>>::value, "DevBuf lives in std::vector");

// An owning set of timing events: ensure(n) creates what is missing of the first n, the destructor destroys them all, and
// the set is never copied.  The handle that holds it synchronises before it is deleted, as for its buffers.
struct DevEvents {
  std::vector<hipEvent_t> ev;
  DevEvents() = default;
  DevEvents(const DevEvents&) = delete;
  DevEvents& operator=(const DevEvents&) = delete;
  ~DevEvents() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  int ensure(size_t n) {
    while (ev.size() < n) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) {
        set_error("hipEventCreate failed");
        return EIOKU_EHIP;
      }
      ev.push_back(e);
    }
    return EIOKU_OK;
  }
  int record(size_t i, hipStream_t stream) const {
    EIOKU_HIP_CHECK(hipEventRecord(ev[i], stream));
    return EIOKU_OK;
  }
  // device milliseconds from event a to event b; waits for b
  int ms(size_t a, size_t b, double* out) const {
    float v = 0.f;
    EIOKU_HIP_CHECK(hipEventSynchronize(ev[b]));
    EIOKU_HIP_CHECK(hipEventElapsedTime(&v, ev[a], ev[b]));
    *out = v;
    return EIOKU_OK;
  }
};

// The N consecutive stages of a model's call between N + 1 events: stage i runs from mark(i) to mark(i + 1).  begin(mask)
// says which stages this call runs (bit i = stage i); last_ms reports 0 for the others and waits for the rest.
template <int N>
struct StageClock {
  DevEvents ev;
  bool ran[N] = {};
  int create() { return ev.ensure(N + 1); }
  void begin(unsigned mask) {
    for (int i = 0; i < N; ++i) ran[i] = (mask >> i & 1u) != 0;
  }
  int mark(int i, hipStream_t stream) const { return ev.record((size_t)i, stream); }
  int last_ms(double* const out[N]) const {
    for (int i = 0; i < N; ++i) {
      *out[i] = 0.0;
      if (ran[i]) EIOKU_TRY(ev.ms((size_t)i, (size_t)i + 1, out[i]));
    }
    return EIOKU_OK;
  }
};

__device__ __forceinline__ unsigned long long splitmix64_at(unsigned long long seed,
                                                            unsigned long long i) {
  unsigned long long z = seed + (i + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

template <typename T>
__device__ __forceinline__ T wave_reduce_add(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Sum of a 32-bit value over the wave on the DPP crossbar: six v_add_u32_dpp and one v_readlane_b32, against ~25
// instructions (ds_bpermute + address + bounds select per step) for the __shfl_down form -- the per-frame reductions
// of the VALU-bound scene kernels.  The result is wave-uniform (an SGPR).
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);  // row_half_mirror
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);  // row_mirror: every lane = its row's sum
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, true);  // row_bcast:15 into rows 1 and 3
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, true);  // row_bcast:31 into rows 2 and 3
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

}  // namespace eioku
