// K14h: the device half of HDBSCAN on cosine distance: core distances and the minimum spanning tree of the
// mutual-reachability graph, in float64 throughout (an MST chosen by float32 distances gives another partition than
// scikit-learn's; DESIGN.md "K14h HDBSCAN").  Nothing of size n x n is stored.
//
//   k_hdb_rows64    fp32 rows -> unit float64 rows (sklearn.preprocessing.normalize: a zero row stays zero)
//   k_hdb_pass<0>   core distance: the min_samples-th smallest cosine distance of every row (self included)
//   k_hdb_pass<1>   Boruvka candidate: per row the smallest (w, j) with w = max(core_i, core_j, d_ij) over the j of
//                   another component
//   k_hdb_min_w / k_hdb_min_pair / k_hdb_hook / k_hdb_jump   the component step (two 64-bit atomicMin passes, hook,
//                   pointer jump)
//
// k_hdb_pass: a workgroup owns 64 rows and walks every 64-column tile itself, so the per-row results stay in LDS
// (<0>) or registers (<1>) and are written once; there are no cross-workgroup atomics in it.  Four waves in 2 x 2, each
// 32 x 32 = 2 x 2 blocks of v_mfma_f64_16x16x4_f64, K in chunks of 32 through LDS.  Lane l supplies A[l & 15][l >> 4] and
// B[l >> 4][l & 15]; accumulator t of lane l is D[(l >> 4) + 4 t][l & 15] (the f64 map, not the f32 one).
//
// The edge order is (w, min(i, j), max(i, j)) with exact float64 compares: strict and total, so the edges every
// component picks form a forest even when all weights are equal, and the only cycles are the two components that pick
// the same edge (the larger root hooks under the smaller).  The round loop is the host's and is bounded.
#include <algorithm>
#include <cmath>
#include <mutex>

#include "common.h"

using namespace eioku;

namespace {

typedef double double4v __attribute__((ext_vector_type(4)));

constexpr int kHT = 64;        // rows per workgroup, columns per tile
constexpr int kHK = 32;        // K chunk
constexpr int kHP = kHK + 4;   // LDS row stride in doubles: rows 4 double-banks apart, k beside them (8 rows x 4 k = the 32 double-banks)
constexpr int kHMaxMs = 32;    // min_samples limit: the per-row list of smallest distances held in LDS
constexpr int kHTopP = kHMaxMs + 1;
constexpr unsigned long long kNone = ~0ull;

__global__ __launch_bounds__(256) void k_hdb_rows64(const float* __restrict__ e, int n, int d, double* __restrict__ x) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  double ss = 0.0;
  for (int k = lane; k < d; k += 64) {
    const double v = (double)e[(size_t)row * d + k];
    ss += v * v;
  }
  ss = wave_reduce_add(ss);
  ss = __shfl(ss, 0, 64);
  double nrm = sqrt(ss);
  if (nrm == 0.0) nrm = 1.0;
  for (int k = lane; k < d; k += 64) x[(size_t)row * d + k] = (double)e[(size_t)row * d + k] / nrm;
}

// MODE 0: core_out[i] written.  MODE 1: core / comp read, best_w / best_j written (best_j = -1: no other component).
template <int MODE>
__global__ __launch_bounds__(256) void k_hdb_pass(const double* __restrict__ x, int n, int d, int min_samples,
                                                  double* __restrict__ core, const int* __restrict__ comp,
                                                  double* __restrict__ best_w, int* __restrict__ best_j) {
  __shared__ __attribute__((aligned(16))) double tiles[2 * kHT * kHP];
  double* const sa = tiles;
  double* const sb = tiles + kHT * kHP;
  // <0>: this tile's distances below the row's threshold, [row][slot].  It lies over the operand tiles, which are dead
  // between the K loop's last barrier and the next tile's first store (a barrier ends the merge).
  double* const cand = tiles;
  static_assert(kHT * kHT <= 2 * kHT * kHP, "cand must fit in the operand tiles");
  __shared__ double top[MODE == 0 ? kHT * kHTopP : 1];   // ascending smallest distances per row
  __shared__ double thr[MODE == 0 ? kHT : 1];
  __shared__ int cnt[MODE == 0 ? kHT : 1];
  __shared__ double red_w[MODE == 1 ? 2 * kHT : 1];
  __shared__ int red_j[MODE == 1 ? 2 * kHT : 1];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int row0 = blockIdx.x * kHT;
  const double inf = __builtin_huge_val();

  if (MODE == 0) {
    for (int t = tid; t < kHT * kHTopP; t += 256) top[t] = inf;
    if (tid < kHT) {
      thr[tid] = inf;
      cnt[tid] = 0;
    }
  }
  // MODE 1: this lane's 8 rows (a, t): local row wr * 32 + a * 16 + (lane >> 4) + 4 t
  double ci[2][4], bw[2][4];
  int pi[2][4], bj[2][4];
  if (MODE == 1) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = row0 + wr * 32 + a * 16 + (lane >> 4) + 4 * t;
        ci[a][t] = i < n ? core[i] : 0.0;
        pi[a][t] = i < n ? comp[i] : -1;
        bw[a][t] = inf;
        bj[a][t] = -1;
      }
  }
  __syncthreads();

  for (int col0 = 0; col0 < n; col0 += kHT) {
    double4v acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[a][b][t] = 0.0;
    for (int k0 = 0; k0 < d; k0 += kHK) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int idx = tid + 256 * q, rr = idx >> 4, c2 = (idx & 15) * 2;
        double2 va = {0.0, 0.0}, vb = {0.0, 0.0};
        if (row0 + rr < n) va = *reinterpret_cast<const double2*>(x + (size_t)(row0 + rr) * d + k0 + c2);
        if (col0 + rr < n) vb = *reinterpret_cast<const double2*>(x + (size_t)(col0 + rr) * d + k0 + c2);
        *reinterpret_cast<double2*>(sa + rr * kHP + c2) = va;
        *reinterpret_cast<double2*>(sb + rr * kHP + c2) = vb;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kHK; k += 4) {
        double fa[2], fb[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) fa[a] = sa[(wr * 32 + a * 16 + (lane & 15)) * kHP + k + (lane >> 4)];
#pragma unroll
        for (int b = 0; b < 2; ++b) fb[b] = sb[(wc * 32 + b * 16 + (lane & 15)) * kHP + k + (lane >> 4)];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
      }
      __syncthreads();
    }
    // epilogue: cosine distance of (i, j), clipped to [0, 2], exactly 0 on the diagonal
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int j = col0 + wc * 32 + b * 16 + (lane & 15);
      double cj = 0.0;
      int pj = -2;
      if (MODE == 1 && j < n) {
        cj = core[j];
        pj = comp[j];
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int rl = wr * 32 + a * 16 + (lane >> 4) + 4 * t, i = row0 + rl;
          if (i >= n || j >= n) continue;
          const double dist = i == j ? 0.0 : fmin(fmax(1.0 - acc[a][b][t], 0.0), 2.0) + 0.0;
          if (MODE == 0) {
            if (dist < thr[rl]) {
              const int slot = atomicAdd(&cnt[rl], 1);  // < 64: a row has 64 columns in a tile
              cand[rl * kHT + slot] = dist;
            }
          } else if (pi[a][t] != pj) {
            const double w = fmax(fmax(ci[a][t], cj), dist);
            if (w < bw[a][t] || (w == bw[a][t] && j < bj[a][t])) {
              bw[a][t] = w;
              bj[a][t] = j;
            }
          }
        }
    }
    if (MODE == 0) {
      __syncthreads();
      if (tid < kHT) {  // one thread per row merges the few candidates into its ascending list
        double* tp = top + tid * kHTopP;
        const int c = cnt[tid];
        for (int s = 0; s < c; ++s) {
          const double v = cand[tid * kHT + s];
          if (v < tp[min_samples - 1]) {
            int p = min_samples - 1;
            while (p > 0 && tp[p - 1] > v) {
              tp[p] = tp[p - 1];
              --p;
            }
            tp[p] = v;
          }
        }
        thr[tid] = tp[min_samples - 1];
        cnt[tid] = 0;
      }
      __syncthreads();
    }
  }

  if (MODE == 0) {
    if (tid < kHT && row0 + tid < n) core[row0 + tid] = top[tid * kHTopP + min_samples - 1];
  } else {
    // a row is spread over the 16 lanes of a (lane >> 4) group in the two waves wc = 0, 1
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        double w = bw[a][t];
        int j = bj[a][t];
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
          const double ow = __shfl_xor(w, off, 64);
          const int oj = __shfl_xor(j, off, 64);
          if (oj >= 0 && (j < 0 || ow < w || (ow == w && oj < j))) {
            w = ow;
            j = oj;
          }
        }
        if ((lane & 15) == 0) {
          const int rl = wr * 32 + a * 16 + (lane >> 4) + 4 * t;
          red_w[wc * kHT + rl] = w;
          red_j[wc * kHT + rl] = j;
        }
      }
    __syncthreads();
    if (tid < kHT && row0 + tid < n) {
      double w = red_w[tid];
      int j = red_j[tid];
      const double ow = red_w[kHT + tid];
      const int oj = red_j[kHT + tid];
      if (oj >= 0 && (j < 0 || ow < w || (ow == w && oj < j))) {
        w = ow;
        j = oj;
      }
      best_w[row0 + tid] = w;
      best_j[row0 + tid] = j;
    }
  }
}

__global__ __launch_bounds__(256) void k_hdb_init(int n, int* __restrict__ comp, int* __restrict__ parent, int* __restrict__ eu) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  comp[i] = i;
  parent[i] = i;
  eu[i] = -1;
}

__global__ __launch_bounds__(256) void k_hdb_reset(int n, unsigned long long* __restrict__ cw, unsigned long long* __restrict__ cp,
                                                   int* __restrict__ hooks) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *hooks = 0;
  if (i >= n) return;
  cw[i] = kNone;
  cp[i] = kNone;
}

// weights are >= +0, so the order of their bit patterns is their order
__global__ __launch_bounds__(256) void k_hdb_min_w(int n, const int* __restrict__ comp, const double* __restrict__ best_w,
                                                   const int* __restrict__ best_j, unsigned long long* __restrict__ cw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || best_j[i] < 0) return;
  atomicMin(&cw[comp[i]], (unsigned long long)__double_as_longlong(best_w[i]));
}

__global__ __launch_bounds__(256) void k_hdb_min_pair(int n, const int* __restrict__ comp, const double* __restrict__ best_w,
                                                      const int* __restrict__ best_j, const unsigned long long* __restrict__ cw,
                                                      unsigned long long* __restrict__ cp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j = best_j[i];
  if (j < 0 || (unsigned long long)__double_as_longlong(best_w[i]) != cw[comp[i]]) return;
  const unsigned long long lo = (unsigned)min(i, j), hi = (unsigned)max(i, j);
  atomicMin(&cp[comp[i]], (lo << 32) | hi);
}

// root c with a picked edge hooks under the root of the edge's far end, unless both picked this edge and c is the smaller
// root.  The edge is kept in slot c: a root is hooked once in its life, so the slots never collide.
__global__ __launch_bounds__(256) void k_hdb_hook(int n, const int* __restrict__ comp, const unsigned long long* __restrict__ cw,
                                                  const unsigned long long* __restrict__ cp, int* __restrict__ parent,
                                                  int* __restrict__ eu, int* __restrict__ ev, double* __restrict__ ew,
                                                  int* __restrict__ hooks) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n || comp[c] != c || cp[c] == kNone) return;
  const int u = (int)(cp[c] >> 32), v = (int)(cp[c] & 0xffffffffu);
  const int c2 = comp[u] == c ? comp[v] : comp[u];
  if (cp[c2] == cp[c] && cw[c2] == cw[c] && c < c2) return;
  parent[c] = c2;
  eu[c] = u;
  ev[c] = v;
  ew[c] = __longlong_as_double((long long)cw[c]);
  atomicAdd(hooks, 1);
}

__global__ __launch_bounds__(256) void k_hdb_jump(int n, int* __restrict__ comp, const int* __restrict__ parent) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int r = comp[i];
  for (int s = 0; s < n; ++s) {  // the hooks of a round form a forest: its depth is below n
    const int p = parent[r];
    if (p == r) break;
    r = p;
  }
  comp[i] = r;
}

// slots 0 .. n-1 without the last root's -> n - 1 edges in slot order
__global__ __launch_bounds__(256) void k_hdb_emit(int n, const int* __restrict__ comp, const int* __restrict__ eu,
                                                  const int* __restrict__ ev, const double* __restrict__ ew, int32_t* __restrict__ out_u,
                                                  int32_t* __restrict__ out_v, double* __restrict__ out_w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int root = comp[0];
  if (i >= n || i == root) return;
  const int k = i - (i > root ? 1 : 0);
  out_u[k] = eu[i];
  out_v[k] = ev[i];
  out_w[k] = ew[i];
}

std::mutex g_hdb_mu;
void* g_hdb_ws = nullptr;
size_t g_hdb_bytes = 0;
constexpr int kHdbMaxStages = 40;
float g_hdb_ms[kHdbMaxStages];
int g_hdb_stages = 0;
hipEvent_t g_hdb_ev[kHdbMaxStages + 1];
bool g_hdb_ev_ready = false;

size_t up256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

extern "C" {

int eioku_hdbscan_mst_cosine(const float* emb, int n, int d, int min_samples, double* core_out, int32_t* edge_u, int32_t* edge_v,
                             double* edge_w, int32_t* rounds_out, int mem, void* stream_) {
  EIOKU_REQUIRE_INIT();
  EIOKU_REQUIRE(n >= 0 && n <= 65536, "n = %d outside [0, 65536]", n);
  EIOKU_REQUIRE(d > 0 && d % 32 == 0, "d = %d must be a positive multiple of 32", d);
  EIOKU_REQUIRE(mem == EIOKU_MEM_HOST || mem == EIOKU_MEM_DEVICE, "bad mem flag %d", mem);
  EIOKU_REQUIRE(n == 0 || (min_samples >= 1 && min_samples <= std::min(n, kHMaxMs)), "min_samples = %d outside [1, min(n, %d)]",
                min_samples, kHMaxMs);
  EIOKU_REQUIRE(rounds_out, "NULL rounds_out");
  *rounds_out = 0;  // HOST on either side: the round loop is the host's
  std::lock_guard<std::mutex> lock(g_hdb_mu);
  g_hdb_stages = 0;
  if (n == 0) return EIOKU_OK;
  EIOKU_REQUIRE(emb && core_out, "NULL buffer");
  EIOKU_REQUIRE(n == 1 || (edge_u && edge_v && edge_w), "NULL edge buffer");
  hipStream_t stream = (hipStream_t)stream_;
  const bool host = mem == EIOKU_MEM_HOST;
  const size_t x_b = up256((size_t)n * d * 8), v8 = up256((size_t)n * 8), v4 = up256((size_t)n * 4);
  const size_t emb_b = host ? up256((size_t)n * d * 4) : 0;
  const size_t need = x_b + 5 * v8 + (host ? v8 : 0) + 5 * v4 + (host ? 2 * v4 : 0) + 256 + emb_b;
  if (g_hdb_bytes < need) {
    if (g_hdb_ws) (void)hipFree(g_hdb_ws);
    g_hdb_ws = nullptr;
    g_hdb_bytes = 0;
    EIOKU_HIP_CHECK(hipMalloc(&g_hdb_ws, need));
    g_hdb_bytes = need;
  }
  if (!g_hdb_ev_ready) {
    for (int i = 0; i <= kHdbMaxStages; ++i) EIOKU_HIP_CHECK(hipEventCreate(&g_hdb_ev[i]));
    g_hdb_ev_ready = true;
  }
  char* p = (char*)g_hdb_ws;
  auto take = [&p](size_t b) {
    char* q = p;
    p += b;
    return q;
  };
  double* x = (double*)take(x_b);
  double* core = (double*)take(v8);
  double* best_w = (double*)take(v8);
  unsigned long long* cw = (unsigned long long*)take(v8);
  unsigned long long* cp = (unsigned long long*)take(v8);
  double* ew = (double*)take(v8);
  double* o_w = host ? (double*)take(v8) : edge_w;
  int* best_j = (int*)take(v4);
  int* comp = (int*)take(v4);
  int* parent = (int*)take(v4);
  int* eu = (int*)take(v4);
  int* ev = (int*)take(v4);
  int32_t* o_u = host ? (int32_t*)take(v4) : edge_u;
  int32_t* o_v = host ? (int32_t*)take(v4) : edge_v;
  int* hooks = (int*)take(256);
  const float* d_emb = emb;
  if (host) {
    float* e = (float*)take(emb_b);
    EIOKU_HIP_CHECK(hipMemcpyAsync(e, emb, (size_t)n * d * 4, hipMemcpyHostToDevice, stream));
    d_emb = e;
  }
  const unsigned rows4 = (unsigned)((n + 3) / 4), lin = (unsigned)((n + 255) / 256), blocks = (unsigned)((n + kHT - 1) / kHT);
  hipLaunchKernelGGL(k_hdb_rows64, dim3(rows4), dim3(256), 0, stream, d_emb, n, d, x);
  EIOKU_HIP_CHECK(hipEventRecord(g_hdb_ev[0], stream));
  hipLaunchKernelGGL(k_hdb_pass<0>, dim3(blocks), dim3(256), 0, stream, x, n, d, min_samples, core, (const int*)nullptr,
                     (double*)nullptr, (int*)nullptr);
  EIOKU_HIP_CHECK(hipEventRecord(g_hdb_ev[1], stream));
  hipLaunchKernelGGL(k_hdb_init, dim3(lin), dim3(256), 0, stream, n, comp, parent, eu);
  EIOKU_LAUNCH_CHECK();
  int stages = 1;
  // Boruvka at least halves the components per round; one round of slack.  Never "until one is left".
  int max_rounds = 1;
  while ((1 << (max_rounds - 1)) < n) ++max_rounds;
  int comps = n, rounds = 0;
  for (; rounds < max_rounds && comps > 1; ++rounds) {
    hipLaunchKernelGGL(k_hdb_pass<1>, dim3(blocks), dim3(256), 0, stream, x, n, d, min_samples, core, comp, best_w, best_j);
    hipLaunchKernelGGL(k_hdb_reset, dim3(lin), dim3(256), 0, stream, n, cw, cp, hooks);
    hipLaunchKernelGGL(k_hdb_min_w, dim3(lin), dim3(256), 0, stream, n, comp, best_w, best_j, cw);
    hipLaunchKernelGGL(k_hdb_min_pair, dim3(lin), dim3(256), 0, stream, n, comp, best_w, best_j, cw, cp);
    hipLaunchKernelGGL(k_hdb_hook, dim3(lin), dim3(256), 0, stream, n, comp, cw, cp, parent, eu, ev, ew, hooks);
    hipLaunchKernelGGL(k_hdb_jump, dim3(lin), dim3(256), 0, stream, n, comp, parent);
    EIOKU_LAUNCH_CHECK();
    EIOKU_HIP_CHECK(hipEventRecord(g_hdb_ev[stages + 1], stream));
    ++stages;
    int h = 0;
    EIOKU_HIP_CHECK(hipMemcpyAsync(&h, hooks, sizeof(int), hipMemcpyDeviceToHost, stream));
    EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
    if (h <= 0 || h >= comps) {
      set_error("hdbscan: round %d hooked %d of %d components", rounds + 1, h, comps);
      return EIOKU_EINVAL;
    }
    comps -= h;
  }
  if (comps > 1) {
    set_error("hdbscan: %d components left after %d rounds (bound ceil(log2 n) + 1)", comps, rounds);
    return EIOKU_EINVAL;
  }
  *rounds_out = rounds;
  const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  EIOKU_HIP_CHECK(hipMemcpyAsync(core_out, core, (size_t)n * 8, back, stream));
  if (n > 1) {
    hipLaunchKernelGGL(k_hdb_emit, dim3(lin), dim3(256), 0, stream, n, comp, eu, ev, ew, o_u, o_v, o_w);
    EIOKU_LAUNCH_CHECK();
    if (host) {
      EIOKU_HIP_CHECK(hipMemcpyAsync(edge_u, o_u, (size_t)(n - 1) * 4, hipMemcpyDeviceToHost, stream));
      EIOKU_HIP_CHECK(hipMemcpyAsync(edge_v, o_v, (size_t)(n - 1) * 4, hipMemcpyDeviceToHost, stream));
      EIOKU_HIP_CHECK(hipMemcpyAsync(edge_w, o_w, (size_t)(n - 1) * 8, hipMemcpyDeviceToHost, stream));
    }
  }
  EIOKU_HIP_CHECK(hipStreamSynchronize(stream));
  for (int s = 0; s < stages; ++s) EIOKU_HIP_CHECK(hipEventElapsedTime(&g_hdb_ms[s], g_hdb_ev[s], g_hdb_ev[s + 1]));
  g_hdb_stages = stages;
  return EIOKU_OK;
}

int eioku_hdbscan_last_stage_ms(double* ms_out, int cap) {
  EIOKU_REQUIRE(ms_out && cap >= 0, "NULL buffer");
  std::lock_guard<std::mutex> lock(g_hdb_mu);
  for (int s = 0; s < g_hdb_stages && s < cap; ++s) ms_out[s] = (double)g_hdb_ms[s];
  return g_hdb_stages;
}

}  // extern "C"
