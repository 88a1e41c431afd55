// The order of the search family (flat kNN and IVF-PQ), written once: results are the k best by (distance, id)
// ascending, ties to the smaller id, (FLT_MAX, -1) padding.  Device-only helpers; every selection kernel of knn.hip and
// ivfpq.hip that compares ids goes through them, so "bit-identical D and I across routes" is a property of this file.
//
// "No entry" is (FLT_MAX, none<Id>()) - the largest id, so the plain order puts it last - while it travels through a
// reduction, and a negative id where it is stored: the padding of a result or partial list, an empty SmallTop slot.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>

namespace eioku {

typedef unsigned u32x4k __attribute__((ext_vector_type(4)));
typedef unsigned u32x2k __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_cvoid_t;

__device__ __forceinline__ unsigned bf16_rne_bits(float f) {  // finite inputs
  unsigned u = __float_as_uint(f);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return u >> 16;
}

template <typename Id>
__device__ __forceinline__ constexpr Id none() {  // Id = int or long long
  return sizeof(Id) == 8 ? (Id)0x7FFFFFFFFFFFFFFFll : (Id)0x7FFFFFFF;
}

// (v, i) comes strictly before (w, j)
template <typename Id>
__device__ __forceinline__ bool better(float v, Id i, float w, Id j) {
  return v < w || (v == w && i < j);
}

// Every lane leaves with the wave's smallest (v, i).
template <typename Id>
__device__ __forceinline__ void wave_argmin(float& v, Id& i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const Id oi = __shfl_xor(i, off, 64);
    if (better(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
}

// The same with the owning lane as a third key (in: the caller's lane, out: the winner's): among lanes that hold the same
// (v, i) - "no entry" included - the lowest one wins, and it is the one that pops its list.
template <typename Id>
__device__ __forceinline__ void wave_argmin(float& v, Id& i, int& l) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const Id oi = __shfl_xor(i, off, 64);
    const int ol = __shfl_xor(l, off, 64);
    if (better(ov, oi, v, i) || (ov == v && oi == i && ol < l)) {
      v = ov;
      i = oi;
      l = ol;
    }
  }
}

// Smallest (v, i) of a 256-thread workgroup, in every thread; s_v / s_i: LDS, one slot per wave.  Two barriers.
template <typename Id>
__device__ __forceinline__ void block_argmin4(float& v, Id& i, float* s_v, Id* s_i) {
  wave_argmin(v, i);
  if ((threadIdx.x & 63) == 0) {
    s_v[threadIdx.x >> 6] = v;
    s_i[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  v = s_v[0];
  i = s_i[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (better(s_v[w], s_i[w], v, i)) {
      v = s_v[w];
      i = s_i[w];
    }
  __syncthreads();
}

// This thread's smallest entry strictly after (lv, li) among entries first, first + step, ... < count, or "no entry".
// read(j, v, i) fetches entry j and returns whether it is one.  k rounds of this, each followed by an argmin across the
// threads and advance(), emit the k best in order without storing anything per thread.
template <typename Id, typename Read>
__device__ __forceinline__ void next_after(float lv, Id li, int first, int count, int step, Read read, float& bv, Id& bi) {
  bv = FLT_MAX;
  bi = none<Id>();
  for (int j = first; j < count; j += step) {
    float v;
    Id i;
    if (read(j, v, i) && better(lv, li, v, i) && better(v, i, bv, bi)) {
      bv = v;
      bi = i;
    }
  }
}
template <typename Id>
__device__ __forceinline__ void next_after(float lv, Id li, int first, int count, int step, const float* vs, const Id* is,
                                           float& bv, Id& bi) {
  next_after(lv, li, first, count, step, [=](int j, float& v, Id& i) { v = vs[j]; i = is[j]; return true; }, bv, bi);
}
// (lv, li) <- the round's winner; once it is "no entry" nothing comes after it and the remaining rounds emit padding.
template <typename Id>
__device__ __forceinline__ void advance(float& lv, Id& li, float bv, Id bi) {
  lv = bi == none<Id>() ? FLT_MAX : bv;
  li = bi;
}

// Sorted register list of the K best (value, 64-bit id); an empty slot is (FLT_MAX, -1) and loses to everything.
template <int K>
struct SmallTop {
  float v[K];
  long long id[K];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int p = 0; p < K; ++p) {
      v[p] = FLT_MAX;
      id[p] = -1;
    }
  }
  __device__ __forceinline__ bool better(float x, long long i, float y, long long j) const {
    return x < y || (x == y && (j < 0 || i < j));
  }
  __device__ __forceinline__ void insert(float x, long long i) {
    if (!better(x, i, v[K - 1], id[K - 1])) return;
#pragma unroll
    for (int p = K - 1; p > 0; --p) {
      const bool shift = better(x, i, v[p - 1], id[p - 1]);
      const bool here = !shift && better(x, i, v[p], id[p]);
      const float nv = shift ? v[p - 1] : (here ? x : v[p]);
      const long long ni = shift ? id[p - 1] : (here ? i : id[p]);
      v[p] = nv;
      id[p] = ni;
    }
    if (better(x, i, v[0], id[0])) {
      v[0] = x;
      id[0] = i;
    }
  }
};

// (word, row) pairs of the scans' workgroup lists -> per-query candidate lists; one workgroup per list.  SLOT = false:
// the word is the query and a candidate is its row (flat scan); SLOT = true: the word is a slot of slot_q[], which names
// the query, and a candidate is (slot, row) (IVF-PQ list-major scan).
template <bool SLOT>
__global__ __launch_bounds__(256) void k_bin_pairs(const unsigned* __restrict__ wl, const int* __restrict__ wl_cnt, int wl_cap,
                                                   const int* __restrict__ slot_q, int* __restrict__ cand,
                                                   int* __restrict__ cnt, int cap, int* __restrict__ overflow) {
  int c = wl_cnt[blockIdx.x];
  if (c > wl_cap) {
    if (threadIdx.x == 0) atomicOr(overflow, 1);
    c = wl_cap;
  }
  const unsigned* list = wl + (size_t)blockIdx.x * wl_cap * 2;
  for (int i = threadIdx.x; i < c; i += 256) {
    const int word = (int)list[2 * i], row = (int)list[2 * i + 1];
    const int qi = SLOT ? slot_q[word] : word;
    const int pos = atomicAdd(cnt + qi, 1);
    if (pos >= cap) continue;
    const size_t at = (size_t)qi * cap + pos;
    if (SLOT) {
      cand[at * 2] = word;
      cand[at * 2 + 1] = row;
    } else {
      cand[at] = row;
    }
  }
}

}  // namespace eioku
