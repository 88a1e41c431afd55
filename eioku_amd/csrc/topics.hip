// K17: keyword selection for topic extraction (KeyBERT's extract_keywords: plain top-n and MMR) on gfx950.
//
// One 256-thread workgroup per row.  A row is a document vector x [d] and a list of candidate term ids (CSR); the score of
// term t is s_t = dot(x, w_t) over unit vectors, i.e. KeyBERT's cosine.  The workgroup
//   1. stages x in LDS (16-byte loads) and scores every candidate: 16 lanes per candidate, each lane a fixed set of float4
//      chunks of the term row (16-byte loads), then a 16-lane xor butterfly, so the sum order is fixed and every call
//      gives the same bits;
//   2. picks top_n times.  Plain: the argmax of s among the unpicked candidates.  MMR (lambda >= 0): the first pick is the
//      argmax of s; before each later pick the last picked term row is staged in LDS, every candidate's running maximum
//      m_t = max_k dot(w_t, w_k) is updated with it, and the pick is the argmax of (1 - lambda) * s_t - lambda * m_t in
//      fp32, in that order.  Every argmax is a workgroup reduction on the key (value, -term id, -position): ties go to
//      the smaller vocabulary index;
//   3. writes the picks ordered by s descending (ties: smaller term id), -1 / 0 padding and the pick count.
// Scores and running maxima live in LDS while the row has at most kCap candidates; a longer row keeps them in the call's
// scratch buffer at its CSR offsets.  No atomics and no workgroup waits on another.
#include <algorithm>
#include <climits>
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kCap = 2048;   // candidates per row whose scores and running maxima stay in LDS
constexpr int kMaxTopN = 32;
constexpr int kMaxD = 1024;

struct Best {
  float v;
  int id, pos;
};

// total order: larger value, then smaller term id, then smaller position; NaN ranks as -inf
__device__ __forceinline__ bool better(const Best& a, const Best& b) {
  if (a.v != b.v) return a.v > b.v;
  if (a.id != b.id) return a.id < b.id;
  return a.pos < b.pos;
}

__device__ __forceinline__ float nan_low(float v) { return v != v ? -INFINITY : v; }

// dot(a, b) over d4 float4 chunks by one 16-lane group: lane gl takes chunks gl, gl + 16, ...; every lane of the group
// returns the same bits
__device__ __forceinline__ float dot16(const float4* __restrict__ a, const float4* __restrict__ b, int d4, int gl) {
  float acc = 0.f;
  for (int c = gl; c < d4; c += 16) {
    const float4 p = a[c], q = b[c];
    acc += p.x * q.x + p.y * q.y + p.z * q.z + p.w * q.w;
  }
  acc += __shfl_xor(acc, 8, 64);
  acc += __shfl_xor(acc, 4, 64);
  acc += __shfl_xor(acc, 2, 64);
  acc += __shfl_xor(acc, 1, 64);
  return acc;
}

__device__ __forceinline__ Best block_best(Best b, Best* red, int lane, int wave) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Best o{__shfl_xor(b.v, off, 64), __shfl_xor(b.id, off, 64), __shfl_xor(b.pos, off, 64)};
    if (better(o, b)) b = o;
  }
  if (lane == 0) red[wave] = b;
  __syncthreads();
  Best r = red[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w)
    if (better(red[w], r)) r = red[w];
  return r;
}

__global__ __launch_bounds__(kThreads) void k_keyword_select(const float* __restrict__ x, const float* __restrict__ terms,
                                                             int n_terms, int d, const int32_t* __restrict__ row_ptr,
                                                             const int32_t* __restrict__ cand, int top_n, float lam,
                                                             float* __restrict__ spill_s, float* __restrict__ spill_m,
                                                             int32_t* __restrict__ idx_out, float* __restrict__ score_out,
                                                             int32_t* __restrict__ count_out, int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int d4 = d >> 2;
  float4* xs = (float4*)smem;                     // d floats
  float4* wk = xs + d4;                           // d floats: the last picked term row (MMR)
  float* ls = (float*)(wk + d4);                  // kCap scores
  float* lm = ls + kCap;                          // kCap running maxima
  Best* red = (Best*)(lm + kCap);                 // one per wave
  Best* picks = red + kThreads / 64;              // kMaxTopN: (s, term id, position)

  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 4, gl = tid & 15;
  const int base = row_ptr[0], beg = row_ptr[row], n = row_ptr[row + 1] - beg;
  const int npick = min(top_n, n);
  const bool mmr = lam >= 0.f;
  const Best none{-INFINITY, INT_MAX, INT_MAX};

  if (n > 0) {
    float* S = n > kCap ? spill_s + (beg - base) : ls;
    float* M = n > kCap ? spill_m + (beg - base) : lm;
    const int32_t* rc = cand + beg;
    const float4* xg = (const float4*)(x + (size_t)row * d);
    for (int c = tid; c < d4; c += kThreads) xs[c] = xg[c];
    __syncthreads();

    // scores, and the first pick (argmax s for both modes)
    Best b = none;
    for (int j = grp; j < n; j += kThreads / 16) {
      const int id = rc[j];
      float s = -INFINITY;
      if (id >= 0 && id < n_terms) {
        s = nan_low(dot16(xs, (const float4*)(terms + (size_t)id * d), d4, gl));
      } else if (gl == 0) {
        *err = 1;
      }
      if (gl == 0) {
        S[j] = s;
        if (mmr) M[j] = -INFINITY;
      }
      const Best c{s, id, j};
      if (better(c, b)) b = c;
    }
    for (int i = 0; i < npick; ++i) {
      if (i > 0) {
        b = none;
        if (mmr) {
          const int last = picks[i - 1].id;
          if (last >= 0 && last < n_terms) {
            const float4* wg = (const float4*)(terms + (size_t)last * d);
            for (int c = tid; c < d4; c += kThreads) wk[c] = wg[c];
          } else {
            for (int c = tid; c < d4; c += kThreads) wk[c] = make_float4(0.f, 0.f, 0.f, 0.f);
          }
          __syncthreads();
          for (int j = grp; j < n; j += kThreads / 16) {
            const int id = rc[j];
            float m = M[j];
            if (m != INFINITY && id >= 0 && id < n_terms) {  // +inf marks a picked candidate
              const float sim = dot16(wk, (const float4*)(terms + (size_t)id * d), d4, gl);
              m = fmaxf(m, sim);
              if (gl == 0) M[j] = m;
            }
            const float key = m == INFINITY ? -INFINITY : nan_low((1.f - lam) * S[j] - lam * m);
            const Best c{key, id, j};
            if (better(c, b)) b = c;
          }
        } else {
          for (int j = tid; j < n; j += kThreads) {
            const Best c{S[j], rc[j], j};  // a picked candidate holds -inf
            if (better(c, b)) b = c;
          }
        }
      }
      const Best w = block_best(b, red, lane, wave);
      if (tid == 0) {
        const int pos = min(w.pos, n - 1);
        const float s = mmr ? S[pos] : w.v;
        picks[i] = Best{s, rc[pos], pos};
        if (mmr) M[pos] = INFINITY;
        else S[pos] = -INFINITY;
      }
      __syncthreads();
    }
  }

  // picks ordered by s descending, ties by the smaller term id (then position)
  if (tid < top_n) {
    int32_t* io = idx_out + (size_t)row * top_n;
    float* so = score_out + (size_t)row * top_n;
    if (tid < npick) {
      const Best p = picks[tid];
      const Best pk{nan_low(p.v), p.id, p.pos};
      int rank = 0;
      for (int q = 0; q < npick; ++q) {
        const Best o = picks[q];
        rank += better(Best{nan_low(o.v), o.id, o.pos}, pk);
      }
      io[rank] = p.id;
      so[rank] = p.v;
    } else {
      io[tid] = -1;
      so[tid] = 0.f;
    }
  }
  if (tid == 0) count_out[row] = npick;
}

// a raw pointer on purpose: the workspace lives as long as the process, and a static destructor would free it after
// the runtime is gone
std::mutex g_ks_mu;
void* g_ks_ws = nullptr;
size_t g_ks_bytes = 0;

size_t up256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

extern "C" {

int eioku_keyword_select(const float* x, int n_rows, const float* terms, int n_terms, int d, const int32_t* row_ptr,
                         const int32_t* cand, int top_n, float diversity, int32_t* idx, float* score, int32_t* count,
                         int mem, void* stream_) {
  // argument checks come before the device is touched
  EIOKU_REQUIRE(n_rows >= 0 && n_terms >= 0, "n_rows = %d, n_terms = %d must be >= 0", n_rows, n_terms);
  EIOKU_REQUIRE(top_n >= 1 && top_n <= kMaxTopN, "top_n = %d outside [1, %d]", top_n, kMaxTopN);
  EIOKU_REQUIRE(d > 0 && d % 4 == 0 && d <= kMaxD, "d = %d must be a positive multiple of 4, at most %d", d, kMaxD);
  EIOKU_REQUIRE(diversity <= 1.f, "diversity = %g must be <= 1 (negative: plain top-n)", (double)diversity);
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  EIOKU_REQUIRE_INIT();
  if (n_rows == 0) return EIOKU_OK;
  EIOKU_REQUIRE(x && row_ptr && idx && score && count, "NULL buffer");
  hipStream_t stream = (hipStream_t)stream_;
  std::lock_guard<std::mutex> lock(g_ks_mu);

  // the row offsets size the scratch and bound every candidate read, so they are checked on the host
  std::vector<int32_t> rp(row_ptr, row_ptr + (mem == EIOKU_MEM_HOST ? n_rows + 1 : 0));
  if (mem == EIOKU_MEM_DEVICE) {
    rp.resize((size_t)n_rows + 1);
    EIOKU_HIP_CHECK(hipMemcpyAsync(rp.data(), row_ptr, rp.size() * 4, hipMemcpyDeviceToHost, stream));
    EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  }
  EIOKU_REQUIRE(rp[0] >= 0, "row_ptr[0] = %d must be >= 0", rp[0]);
  int max_len = 0;
  for (int r = 0; r < n_rows; ++r) {
    EIOKU_REQUIRE(rp[r + 1] >= rp[r], "row_ptr decreases at row %d", r);
    max_len = std::max(max_len, rp[r + 1] - rp[r]);
  }
  const size_t nnz = (size_t)(rp[n_rows] - rp[0]);
  EIOKU_REQUIRE(nnz == 0 || (cand && terms && n_terms > 0), "candidates without terms");

  const size_t spill_b = max_len > kCap ? up256(nnz * 4) : 0;
  const bool host = mem == EIOKU_MEM_HOST;
  const size_t x_b = host ? up256((size_t)n_rows * d * 4) : 0, t_b = host ? up256((size_t)n_terms * d * 4) : 0;
  const size_t rp_b = host ? up256(((size_t)n_rows + 1) * 4) : 0, c_b = host ? up256((size_t)rp[n_rows] * 4) : 0;
  const size_t o_b = host ? 3 * up256((size_t)n_rows * top_n * 4) : 0;
  const size_t need = 256 + 2 * spill_b + x_b + t_b + rp_b + c_b + o_b;
  if (g_ks_bytes < need) {
    if (g_ks_ws) (void)hipFree(g_ks_ws);
    g_ks_ws = nullptr;
    g_ks_bytes = 0;
    EIOKU_HIP_CHECK(hipMalloc(&g_ks_ws, need));
    g_ks_bytes = need;
  }
  char* p = (char*)g_ks_ws;
  int* err = (int*)p;
  p += 256;
  float* spill_s = spill_b ? (float*)p : nullptr;
  float* spill_m = spill_b ? (float*)(p + spill_b) : nullptr;
  p += 2 * spill_b;
  const float *dx = x, *dt = terms;
  const int32_t *drp = row_ptr, *dc = cand;
  int32_t *di = idx, *dcount = count;
  float* ds = score;
  if (host) {
    float* hx = (float*)p;
    float* ht = (float*)(p + x_b);
    int32_t* hrp = (int32_t*)(p + x_b + t_b);
    int32_t* hc = (int32_t*)(p + x_b + t_b + rp_b);
    char* o = p + x_b + t_b + rp_b + c_b;
    const size_t ob = up256((size_t)n_rows * top_n * 4);
    EIOKU_HIP_CHECK(hipMemcpyAsync(hx, x, (size_t)n_rows * d * 4, hipMemcpyHostToDevice, stream));
    if (n_terms) EIOKU_HIP_CHECK(hipMemcpyAsync(ht, terms, (size_t)n_terms * d * 4, hipMemcpyHostToDevice, stream));
    EIOKU_HIP_CHECK(hipMemcpyAsync(hrp, rp.data(), rp.size() * 4, hipMemcpyHostToDevice, stream));
    if (rp[n_rows]) EIOKU_HIP_CHECK(hipMemcpyAsync(hc, cand, (size_t)rp[n_rows] * 4, hipMemcpyHostToDevice, stream));
    dx = hx, dt = ht, drp = hrp, dc = hc;
    di = (int32_t*)o, ds = (float*)(o + ob), dcount = (int32_t*)(o + 2 * ob);
  }
  EIOKU_REQUIRE(((uintptr_t)dx & 15) == 0 && ((uintptr_t)dt & 15) == 0, "x and terms must be 16-byte aligned");
  EIOKU_HIP_CHECK(hipMemsetAsync(err, 0, 4, stream));
  const size_t lds = (size_t)2 * d * 4 + (size_t)2 * kCap * 4 + (kThreads / 64 + kMaxTopN) * sizeof(Best);
  hipLaunchKernelGGL(k_keyword_select, dim3((unsigned)n_rows), dim3(kThreads), lds, stream, dx, dt, n_terms, d, drp, dc,
                     top_n, diversity < 0.f ? -1.f : diversity, spill_s, spill_m, di, ds, dcount, err);
  EIOKU_LAUNCH_CHECK();
  int herr = 0;
  EIOKU_HIP_CHECK(hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, stream));
  if (host) {
    EIOKU_HIP_CHECK(hipMemcpyAsync(idx, di, (size_t)n_rows * top_n * 4, hipMemcpyDeviceToHost, stream));
    EIOKU_HIP_CHECK(hipMemcpyAsync(score, ds, (size_t)n_rows * top_n * 4, hipMemcpyDeviceToHost, stream));
    EIOKU_HIP_CHECK(hipMemcpyAsync(count, dcount, (size_t)n_rows * 4, hipMemcpyDeviceToHost, stream));
  }
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  EIOKU_REQUIRE(herr == 0, "a candidate term id is outside [0, %d)", n_terms);
  return EIOKU_OK;
}

}  // extern "C"
