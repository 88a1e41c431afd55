// K4 conv_igemm_bias_silu: NHWC fp16 convolution as implicit GEMM on v_mfma_f32_16x16x32_f16.
//
// Workgroup (256 threads = 4 waves) -> one 8x16 tile of output pixels of one image x one tile of
// 16*NF output channels.  Per 32-channel input chunk:
//   1. the input halo patch ((8-1)*S+KS) x ((16-1)*S+KS) pixels x 32 channels is loaded ONCE from
//      HBM/L2 with 16-byte coalesced loads (zero filled outside the image / past Cin) into LDS,
//      64 B per pixel, XOR-swizzled so that every ds_read_b128 fragment read is conflict free;
//   2. the weight tile [taps][16*NF][32] (pre-packed contiguously on the host) is copied to LDS;
//   3. for each of the KS*KS taps the MFMA B fragments (activations: 16 pixels x 32 ch) are read
//      straight out of the patch at the tap's shifted position - the 9x im2col re-read never
//      leaves the CU - and multiplied by the A fragments (weights: 16 cout x 32 ch).
// D = W . X^T orientation: each lane ends with 4 consecutive output channels of one pixel, so the
// epilogue (bias, SiLU, fp16 round, residual add, concat-slice offset) stores 8 contiguous bytes.
//
// Numerics: fp16 operands, fp32 MFMA accumulation, bias/SiLU in fp32, one RNE rounding to fp16;
// a residual is added as fp16(float(y16) + float(x16)), i.e. the fp16 network `x + cv2(cv1(x))`.
#include "conv.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <type_traits>

namespace eioku {

namespace {
std::atomic<unsigned> g_route_counts[kRouteSlots];
std::atomic<unsigned> g_epi_launches{0};  // k_conv3x3_flat launches that took the straight-line epilogue (eioku_debug_conv_epi)
}
void route_hit(int id) {
  if (id >= 0 && id < kRouteSlots) g_route_counts[id].fetch_add(1u, std::memory_order_relaxed);
}

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));

// ---- bounds-check build (`make bc` -> libeioku_hip_bc.so, -DEIOKU_BOUNDS_CHECK) -------------------
// Round 2's GPU memory fault was an over-read past the end of a tensor that only faulted when the allocation ended on a
// page boundary.  In the bounds-check build every global access of an activation / residual / image / output tensor
// in this file goes through LDG / STG: the address range is compared with the tensor's extent (set by the host
// wrappers from the slice geometry), a violation bumps a device counter and records the source line - no trap, the
// access is skipped - and tests/test_bounds_gpu.py asserts the counter stayed 0 over the conv test cases and whole
// forwards of three model sizes and four source geometries.  The regular build compiles LDG / STG to plain accesses.
struct BcExt {
  const char* lo = nullptr;
  const char* hi = nullptr;
};
#ifdef EIOKU_BOUNDS_CHECK
__device__ int g_bc_flag[4];  // [0] violations, [1] largest source line of a violation
// bytes the access really touches: a 3-element vector is a 12-byte load (global_load_dwordx3) in a 16-byte type
template <typename V>
struct bc_bytes {
  static constexpr size_t value = sizeof(V);
};
template <>
struct bc_bytes<unsigned __attribute__((ext_vector_type(3)))> {
  static constexpr size_t value = 12;
};
template <typename V>
__device__ __forceinline__ V bc_ld(const void* p, BcExt e, int line) {
  const char* c = reinterpret_cast<const char*>(p);
  if (c < e.lo || c + bc_bytes<V>::value > e.hi) {
    atomicAdd(&g_bc_flag[0], 1);
    atomicMax(&g_bc_flag[1], line);
    V z{};
    return z;
  }
  return *reinterpret_cast<const V*>(p);
}
template <typename V>
__device__ __forceinline__ void bc_st(void* p, V v, BcExt e, int line) {
  const char* c = reinterpret_cast<const char*>(p);
  if (c < e.lo || c + sizeof(V) > e.hi) {
    atomicAdd(&g_bc_flag[0], 1);
    atomicMax(&g_bc_flag[1], line);
    return;
  }
  *reinterpret_cast<V*>(p) = v;
}
#define LDG(V, p, ext) bc_ld<V>((p), (ext), __LINE__)
#define STG(V, p, v, ext) bc_st<V>((p), (v), (ext), __LINE__)
#else
#define LDG(V, p, ext) (*reinterpret_cast<const V*>(p))
#define STG(V, p, v, ext) (*reinterpret_cast<V*>(p) = (v))
#endif

struct ConvArgs {
  const __half* in;
  const uint4* wgt;
  const float* bias;
  __half* out;
  float* out_f32;
  const __half* res;
  int N, H, W, Cin, in_cs;
  int Ho, Wo, Cout, out_cs;
  int res_cs;
  int tiles_w, tiles_h, nchunks, act;
  // k_conv3x3_flat may take its straight-line epilogue (conv_epi_on(): EIOKU_CONV_EPI=0 clears it)
  int epi = 0;
  // fused following 1x1 (persistent kernel, POST): out2 = act2(W2 . act(conv3x3) + b2); `out` is then unused
  const uint4* post_w;
  const float* post_bias;
  __half* post_out;
  int post_out_cs, post_cout, post_act;
  // class-max epilogue (1x1, one cout tile, no activation): per pixel {max_c (conv + bias), argmax} instead of the
  // Cout-wide fp32 row -- what the Detect decode needs from the class branch, 8 bytes instead of 4*nc
  unsigned long long* clsmax;
  // 1x1 with a nearest-2x-upsampled first operand (neck concats [up(x) | skip]): channels [0, c_split) are read from
  // the half-resolution tensor in2 at (y/2, x/2) instead of from `in` -- the upsampled tensor is never written
  const __half* in2;
  int in2_cs, c_split;
  // tensor extents, read by the bounds-check build only
  BcExt x_in, x_in2, x_res, x_out, x_img, x_cls;
};

// Workgroups b, b + 8, b + 16 ... share an XCD and its L2.  A persistent kernel that takes tiles b, b + G, b + 2G ...
// has every tile's spatial neighbours (the halo rows and columns it re-reads: 40 % of an 8 x 16 tile's patch) on other
// XCDs.  With this order XCD x owns the contiguous tiles [x T / 8, (x + 1) T / 8) and its workgroups walk them side by
// side, so halos are L2 hits.  Identity when T is not a multiple of 8 (odd batch sizes).
__device__ __forceinline__ int xcd_tile(int v, int total) {
  return (total & 7) == 0 ? (v & 7) * (total >> 3) + (v >> 3) : v;
}

// x / d for 0 <= x < 2^24 (exact int->float) with a precomputed 1.0f/d: one multiply and a +-1 fix-up instead
// of the ~40-instruction integer division (the flattened kernel does ~20 of them before its first load)
__device__ __forceinline__ int fast_div(int x, int d, float rd) {
  int q = (int)((float)x * rd);
  const int r = x - q * d;
  if (r >= d) ++q;
  if (r < 0) --q;
  return q;
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float silu_f32(float v) {
  return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v));
}
// Four values at once, the same operations bit for bit (__expf(-v) compiles to v_exp_f32(v * -log2e), the constant
// being float(log2 e) = 0x3fb8aa3b): written on vectors so that the multiply and the +1 become v_pk_mul_f32 /
// v_pk_add_f32 (two values per issue slot).  The epilogues of the shallow layers are VALU-bound, not MFMA-bound:
// 745 VALU instructions per 67 MFMAs in k_conv_stem_chain, a third of them SiLU.  (Plain v_mul_f32 / v_add_f32
// instead of the packed forms measured SLOWER here: stem chain 126.8 -> 132.8 us, chain<1> 93.0 -> 96.7 us.)
__device__ __forceinline__ float4v silu4(float4v v) {
  const float4v t = v * float4v{-1.44269504088896340736f, -1.44269504088896340736f, -1.44269504088896340736f,
                                -1.44269504088896340736f};
  float4v d = float4v{__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1]), __builtin_amdgcn_exp2f(t[2]),
                      __builtin_amdgcn_exp2f(t[3])};
  d = d + float4v{1.0f, 1.0f, 1.0f, 1.0f};
  const float4v r = float4v{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1]), __builtin_amdgcn_rcpf(d[2]),
                            __builtin_amdgcn_rcpf(d[3])};
  return v * r;
}

// Epilogue for one accumulator fragment: the lane holds 4 consecutive couts c0..c0+3 of output pixel
// `opix`: bias, SiLU, fp16 RNE, residual add (fp16(fp16(y) + x)), concat-slice store or fp32 store.
// `b` = bias of c0..c0+3 and `rpre` = residual of (opix, c0..c0+3) are passed in registers when the
// caller preloaded them (persistent kernels: a global load inside the tile loop would drain the
// in-order vmcnt queue and with it the next tile's prefetch); have_rpre = false loads it here.
// bias + activation only (the fused 3x3+1x1 path keeps the activated tile on chip)
__device__ __forceinline__ float4v activate_frag(const ConvArgs& a, const float4v& acc, float4 b) {
  float4v v = acc + float4v{b.x, b.y, b.z, b.w};
  if (a.act == kActSiLU) {
    v = silu4(v);
  } else if (a.act == kActReLU) {
    v = __builtin_elementwise_max(v, float4v{0.f, 0.f, 0.f, 0.f});
  }
  return v;
}

// `opix`: output pixel index; element offsets are 32-bit (the host entry points refuse tensors of 2^31 elements): one
// v_mul_lo_u32 per address where size_t arithmetic cost a 64-bit multiply-add pair - per store, in every epilogue
__device__ __forceinline__ void store_frag(const ConvArgs& a, const float4v& acc, unsigned opix, int c0, float4 b,
                                           bool have_rpre = false, u32x2 rpre = u32x2{0, 0}) {
  // native vector types throughout: arrays of the HIP uint2/uint4/__half structs end up in scratch memory
  if (c0 >= a.Cout) return;
  float4v v = acc + float4v{b.x, b.y, b.z, b.w};
  if (a.act == kActSiLU) {
    v = silu4(v);
  } else if (a.act == kActReLU) {
    v = __builtin_elementwise_max(v, float4v{0.f, 0.f, 0.f, 0.f});
  }
  const bool full = c0 + 3 < a.Cout;
  if (a.out_f32) {
    float* o = a.out_f32 + (size_t)(opix * (unsigned)a.Cout + (unsigned)c0);
    if (full && (a.Cout & 3) == 0) {
      STG(float4v, o, v, a.x_out);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < a.Cout) STG(float, o + j, v[j], a.x_out);
    }
    return;
  }
  f16x4 h = __builtin_convertvector(v, f16x4);  // RNE
  if (full) {
    if (a.res) {
      const u32x2 r = have_rpre ? rpre : LDG(u32x2, a.res + (size_t)(opix * (unsigned)a.res_cs + (unsigned)c0), a.x_res);
      float4v sum = __builtin_convertvector(h, float4v) + __builtin_convertvector(__builtin_bit_cast(f16x4, r), float4v);
      if (a.act == kActResReLU) sum = __builtin_elementwise_max(sum, float4v{0.f, 0.f, 0.f, 0.f});
      h = __builtin_convertvector(sum, f16x4);
    }
    STG(u32x2, a.out + (size_t)(opix * (unsigned)a.out_cs + (unsigned)c0), __builtin_bit_cast(u32x2, h), a.x_out);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c0 + j < a.Cout) {
        _Float16 o = h[j];
        if (a.res) {
          float sj = (float)o + (float)LDG(_Float16, a.res + (size_t)(opix * (unsigned)a.res_cs + (unsigned)(c0 + j)), a.x_res);
          if (a.act == kActResReLU) sj = fmaxf(sj, 0.f);
          o = (_Float16)sj;
        }
        STG(_Float16, reinterpret_cast<_Float16*>(a.out) + (size_t)(opix * (unsigned)a.out_cs + (unsigned)(c0 + j)), o, a.x_out);
      }
  }
}

// ---- straight-line epilogue of k_conv3x3_flat (r4) -----------------------------------------------------------------
// The common layer - fp16 output, the whole cout tile inside Cout, SiLU or no activation, no residual or a vector
// residual - does store_frag's arithmetic in store_frag's order (bias add, silu4, RNE, fp16(fp16(y) + x)) with nothing
// decided per fragment: the variant (with / without residual) is a compile-time tag chosen once per launch by a uniform
// branch, SiLU or not is one uniform test per row of NF fragments with no memory access behind it, the row's address
// and its `pixel exists` test are computed once per row, and a fragment is a compile-time offset from the row.
// kEpiGeneric = store_frag (ragged tile, fp32 output, ReLU modes, Cout < 4, EIOKU_CONV_EPI=0).  k_conv3x3_persist does
// NOT use it: three copies of its tile loop in one kernel cost 30-90 VGPRs (a wave of occupancy on most instantiations,
// scratch on the S2 NCH3 ones); DESIGN.md, "Round-4 findings".
enum { kEpiGeneric = 0, kEpiPlain = 1, kEpiRes = 2 };
template <int E>
using EpiTag = std::integral_constant<int, E>;
__device__ __forceinline__ int epi_variant(const ConvArgs& a, int c_end, bool res_vec) {
  if (!a.epi || a.out_f32 || c_end > a.Cout || (a.Cout & 3) != 0 || (a.res && !res_vec)) return kEpiGeneric;
  if (a.act != kActSiLU && a.act != kActNone) return kEpiGeneric;
  return a.res ? kEpiRes : kEpiPlain;
}
// The NF fragments of one output row of the lane: every value first, then - behind the row's one test - nothing but the
// NF stores at immediate offsets from `row` (= the lane's first cout of the tile at the row's pixel).  The empty asm pins
// the values in front of the test, so that the exec-masked block behind it holds the stores and nothing else.
template <int E, int NF>
__device__ __forceinline__ void epi_store_row(const ConvArgs& a, const float4v (&acc)[NF], const float4 (&b)[NF],
                                              const u32x2 (&r)[NF], __half* row, bool ok) {
  float4v v[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) v[f] = acc[f] + float4v{b[f].x, b[f].y, b[f].z, b[f].w};
  if (a.act == kActSiLU) {
#pragma unroll
    for (int f = 0; f < NF; ++f) v[f] = silu4(v[f]);
  }
  u32x2 h[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    f16x4 h4 = __builtin_convertvector(v[f], f16x4);  // RNE
    if (E == kEpiRes) {
      const float4v sum = __builtin_convertvector(h4, float4v) + __builtin_convertvector(__builtin_bit_cast(f16x4, r[f]), float4v);
      h4 = __builtin_convertvector(sum, f16x4);
    }
    h[f] = __builtin_bit_cast(u32x2, h4);
    asm volatile("" : "+v"(h[f]));
  }
  if (ok) {
#pragma unroll
    for (int f = 0; f < NF; ++f) STG(u32x2, row + f * 16, h[f], a.x_out);
  }
}

// ---------------------------------------------------------------------------------------------
// 1x1 convolution = plain GEMM over pixels: a streaming kernel.  The weight tile (all of Cin x
// 16*NF couts) sits in LDS for the whole launch; activations never touch LDS: every lane loads its
// B fragment (16 pixels x 32 channels = 16 B per lane) straight from HBM, one k-step ahead of the
// MFMAs, and waves walk the pixel groups grid-stride with no barrier in the loop.
// ---------------------------------------------------------------------------------------------
template <int NF, bool UP = false, int NWV = 4>
__global__ __launch_bounds__(64 * NWV) void k_conv1x1(ConvArgs a, long long npix) {
  constexpr int NT = 64 * NWV;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* wt = reinterpret_cast<uint4*>(smem);  // [nchunks][16*NF][4 units], swizzled per row
  constexpr int ROWS = 16 * NF;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int co_tile = blockIdx.y;

  const int r = lane & 15, u = lane >> 4;
  const uint4* wt_lane = wt + r * 4 + (u ^ ((r >> 1) & 3));  // fragment (kc, f): + (kc*NF + f)*64 units
  const long long groups = (npix + 31) / 32;  // 32 pixels (2 fragments) per wave step
  const long long gstride = (long long)gridDim.x * NWV;
  long long g = (long long)blockIdx.x * NWV + wave;

  // B fragments are fetched KB k-steps (KB x 2 x 16 B per lane) at a time, one block ahead of the MFMAs.  The
  // loads are unconditional (pixel and chunk indices clamped into the tensor) so that the compiler counts them
  // (vmcnt(N)) instead of draining the queue, prefetch included, before every k-step.
  constexpr int KB = 4;
  const int nkb = (a.nchunks + KB - 1) / KB;
  const bool cin_tail = (a.Cin & 31) != 0;
  const int HWf = a.H * a.W;
  const float r_hw = 1.0f / (float)HWf, r_w = 1.0f / (float)a.W;
  auto load_blk = [&](long long grp, int kb, u32x4 (&b)[KB][2]) {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      long long p = grp * 32 + m * 16 + r;
      if (p >= npix) p = npix - 1;
      const __half* src = a.in + (size_t)p * a.in_cs;
      const __half* src2 = src;
      if (UP) {  // pixel (n, y, x) -> (n, y/2, x/2) of the half-resolution source
        const int pi = (int)p;
        const int n = fast_div(pi, HWf, r_hw), rem = pi - n * HWf;
        const int y = fast_div(rem, a.W, r_w), x = rem - y * a.W;
        src2 = a.in2 + ((size_t)(n * (a.H >> 1) + (y >> 1)) * (a.W >> 1) + (x >> 1)) * a.in2_cs;
      }
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        int c = (kb * KB + j) * 32 + u * 8;  // this lane's 8 channels of the chunk
        // past Cin: any in-range address (zeroed below / never multiplied).  The pixel's first unit, not this lane's unit of
        // chunk 0: with Cin < 32 that unit is past the pixel too, and on the last pixel past the tensor
        if (c >= a.Cin) c = 0;
        const __half* base = (UP && c < a.c_split) ? src2 : src;
        b[j][m] = LDG(u32x4, base + c, (UP && c < a.c_split) ? a.x_in2 : a.x_in);
      }
    }
  };

  float4 biasr[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) biasr[f] = *reinterpret_cast<const float4*>(a.bias + co_tile * ROWS + f * 16 + u * 4);
  u32x4 bn[KB][2];
  if (g < groups) load_blk(g, 0, bn);  // in flight while the weight tile is copied
  {
    // weight tile -> LDS, 8 loads in flight per thread (one load -> one store per iteration made this copy the
    // longest phase of the low-resolution layers: 24 dependent round trips for Cin = 384)
    const uint4* wsrc = a.wgt + (size_t)co_tile * a.nchunks * (ROWS * 4);
    const int NW = a.nchunks * ROWS * 4;
    constexpr int WB = 8;
    for (int i0 = 0; i0 < NW; i0 += NT * WB) {
      u32x4 w[WB];
#pragma unroll
      for (int j = 0; j < WB; ++j) {
        const int idx = i0 + j * NT + tid;
        w[j] = *reinterpret_cast<const u32x4*>(wsrc + (idx < NW ? idx : 0));
      }
#pragma unroll
      for (int j = 0; j < WB; ++j) {
        const int idx = i0 + j * NT + tid;
        const int row = (idx >> 2) % ROWS, unit = idx & 3;
        if (idx < NW) *reinterpret_cast<u32x4*>(wt + (idx & ~3) + (unit ^ ((row >> 1) & 3))) = w[j];
      }
    }
  }
  __syncthreads();
  // FAST (r3): the plain layer - SiLU, fp16 output, no residual, whole cout tile inside Cout - on groups whose 32 pixels all
  // exist runs a straight-line epilogue.  store_frag's run-time branches (and `p < npix`) hid from the compiler how many
  // stores follow the next group's prefetch, so the first use of that prefetch waited with vmcnt(0): for the loads AND for
  // the 2 NF stores just issued, a store round trip per group in kernels that run one wave per SIMD.
  auto run = [&](auto fast_tag, long long gend) {
  constexpr bool FAST = decltype(fast_tag)::value;
  for (; g < gend; g += gstride) {
    float4v acc[2][NF];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[m][f] = float4v{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < nkb; ++kb) {
      u32x4 b[KB][2];
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        b[j][0] = bn[j][0];
        b[j][1] = bn[j][1];
      }
      if (cin_tail && kb == nkb - 1) {
#pragma unroll
        for (int j = 0; j < KB; ++j)
          if ((kb * KB + j) * 32 + u * 8 >= a.Cin) b[j][0] = b[j][1] = u32x4{0, 0, 0, 0};
      }
      {
        // ONE unconditional call (the group past the end re-reads the last pixels: load_blk clamps): with the loads in
        // two branches the compiler could not count them and the block's first use waited with vmcnt(0)
        const bool more = kb + 1 < nkb;
        load_blk(more ? g : g + gstride, more ? kb + 1 : 0, bn);  // this group's next block / the next group's first
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        const int kc = kb * KB + j;
        if (kc < a.nchunks) {
          half8 af[NF];
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            uint4 w = wt_lane[(kc * NF + f) * 64];
            af[f] = *reinterpret_cast<half8*>(&w);
          }
#pragma unroll
          for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int m = 0; m < 2; ++m)
              acc[m][f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[f], __builtin_bit_cast(half8, b[j][m]), acc[m][f], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (FAST) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const unsigned p = (unsigned)(g * 32 + m * 16 + r);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const float4v v = silu4(acc[m][f] + float4v{biasr[f].x, biasr[f].y, biasr[f].z, biasr[f].w});
          const f16x4 h = __builtin_convertvector(v, f16x4);  // RNE, as store_frag
          STG(u32x2, a.out + (size_t)(p * (unsigned)a.out_cs + (unsigned)(co_tile * ROWS + f * 16 + u * 4)), __builtin_bit_cast(u32x2, h), a.x_out);
        }
      }
    } else if (a.clsmax) {
      // lane (r, u) holds classes f*16 + u*4 + j of pixel r: ascending class order inside the lane (strict > keeps
      // the first maximum), then the 4 lanes of the pixel combine (ties: lower class), exactly k_decode's rule
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        float best = -INFINITY;
        int bj = 0x7FFFFFFF;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const float bb[4] = {biasr[f].x, biasr[f].y, biasr[f].z, biasr[f].w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = f * 16 + u * 4 + j;
            const float v = acc[m][f][j] + bb[j];
            if (c < a.Cout && v > best) {
              best = v;
              bj = c;
            }
          }
        }
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
          const float ob = __shfl_xor(best, off, 64);
          const int oj = __shfl_xor(bj, off, 64);
          if (ob > best || (ob == best && oj < bj)) {
            best = ob;
            bj = oj;
          }
        }
        const long long p = g * 32 + m * 16 + r;
        if (u == 0 && p < npix) STG(unsigned long long, a.clsmax + p, ((unsigned long long)(unsigned)bj << 32) | __float_as_uint(best), a.x_cls);
      }
    } else {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const long long p = g * 32 + m * 16 + r;
        if (p >= npix) continue;
#pragma unroll
        for (int f = 0; f < NF; ++f) store_frag(a, acc[m][f], (unsigned)p, co_tile * ROWS + f * 16 + u * 4, biasr[f]);
      }
    }
  }
  };
  const bool fast = !a.clsmax && !a.out_f32 && !a.res && a.act == kActSiLU && (co_tile + 1) * ROWS <= a.Cout && (a.Cout & 3) == 0;
  if (fast) run(std::true_type{}, npix / 32);  // the groups whose pixels all exist; a ragged last group runs below
  run(std::false_type{}, groups);
}

// ---------------------------------------------------------------------------------------------
// Deep-K 3x3 variant for the low-resolution half of the network (Cin >= 128 at 40x40 / 20x20): the
// 8x16 spatial tile wastes up to half of every MFMA on a 20-wide map, so here a workgroup owns 64*MT
// CONSECUTIVE output pixels of the flattened (n, y, x) order, across rows and across frames.  The halo
// patch is cut from a "virtual tall image": frames stacked with ONE shared zero row between them
// (row v = n*(H+1) is y = -1 of frame n and y = H of frame n-1), so a tile that crosses a frame border
// still sees the right zero padding.  Zero positions are written once; per-slot addresses are
// computed once per workgroup; every chunk is (batched global loads -> registers) one step ahead of
// the MFMAs that consume the previous chunk.
// ---------------------------------------------------------------------------------------------
// One 32-channel chunk of a 3x3 convolution out of LDS: 9 taps x (MT pixel fragments x NF cout fragments).
// The fragments of tap t+1 are read while the MFMAs of tap t issue (two register sets), and the
// sched_group_barriers pin that interleaving: left alone the scheduler emits read -> lgkmcnt(0) -> MFMA pairs,
// which exposes the LDS latency once per tap at the 1-2 waves per SIMD these kernels run with.  (Fragments TWO taps
// ahead, three register sets, measured no gain: 1.394 vs 1.391 ms over the conv family.)
// `wt_lane` = weight tile + this lane's swizzled row unit; fragment (tap, f) sits (tap*NF + f)*64 units further.
template <int NF, int MT>
__device__ __forceinline__ void mma_taps(const uint4* patch, const uint4* wt_lane, const int (&bpos)[9][MT],
                                         float4v (&acc)[MT][NF]) {
  half8 af[2][NF], bf[2][MT];
  auto ld = [&](int tap, int s) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      uint4 u = patch[bpos[tap][m]];
      bf[s][m] = *reinterpret_cast<half8*>(&u);
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      uint4 u = wt_lane[(tap * NF + f) * 64];
      af[s][f] = *reinterpret_cast<half8*>(&u);
    }
  };
  ld(0, 0);
  __builtin_amdgcn_sched_group_barrier(0x100, NF + MT, 0);
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int s = tap & 1;
    if (tap + 1 < 9) ld(tap + 1, s ^ 1);
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int m = 0; m < MT; ++m)
        acc[m][f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[s][f], bf[s][m], acc[m][f], 0, 0, 0);
    if (tap + 1 < 9) __builtin_amdgcn_sched_group_barrier(0x100, NF + MT, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, NF * MT, 0);
  }
}

// Generic 3x3 kernel: one 8x16 output tile x one cout tile per workgroup, chunk by chunk (its LDS does not grow with
// Cin).  What no persistent / flattened instantiation takes ends here - YOLOv8m's 96 / 192-channel stride-2 convs at
// 160 / 80 / 40-wide maps.  Staging slots are computed once (the first build of this kernel redid the index arithmetic,
// the bounds tests and a conditional load per unit and chunk, with nothing in flight behind the MFMAs: 200 TFLOP/s on
// 96 -> 192 s2): a slot outside the image (zero padding) or past the patch loads element 0 and is zeroed / parked, so
// the loads are unconditional and one chunk ahead of the taps that consume the previous one (mma_taps).
template <int NF, int KS, int S>
__global__ __launch_bounds__(256) void k_conv_igemm(ConvArgs a) {
  static_assert(KS == 3, "the generic kernel serves 3x3 layers; 1x1 layers have k_conv1x1");
  constexpr Patch G = patch_of(kTH, S);
  constexpr TileLds L = igemm_layout(NF, S);
  constexpr int PH = G.ph, PW = G.pw, PWH = G.pwh, PWS = G.pws;
  constexpr int TAPS = KS * KS;
  constexpr int PAD = KS / 2;
  constexpr int PATCH_U = L.spare;  // uint4 units; the spare unit behind them: where idle slots park their store
  constexpr int WT_U = wt_units(NF);
  constexpr int R = (PH * PW * 4 + 255) / 256;  // patch units staged per thread and chunk
  constexpr int WREG = (WT_U + 255) / 256;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* patch = reinterpret_cast<uint4*>(smem);
  uint4* wt = patch + L.wt;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int bx = blockIdx.x;
  const int tw = bx % a.tiles_w;
  bx /= a.tiles_w;
  const int th = bx % a.tiles_h;
  const int n = bx / a.tiles_h;
  const int oh0 = th * kTH, ow0 = tw * kTW;
  const int ih0 = oh0 * S - PAD, iw0 = ow0 * S - PAD;
  const int co_tile = blockIdx.y;

  int s_g[R], s_l[R];
  unsigned s_ok = 0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int idx = tid + 256 * j;
    const int pix = idx >> 2, unit = idx & 3;
    const int py = pix / PW, px = pix - py * PW;
    const int ih = ih0 + py, iw = iw0 + px;
    const bool in_patch = idx < PH * PW * 4;
    const bool ok = in_patch && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
    const int col = EIOKU_PATCH_COL(px, PWH, S);
    const int p = py * PWS + col;
    s_g[j] = ok ? ((n * a.H + ih) * a.W + iw) * a.in_cs + unit * 8 : 0;
    s_l[j] = in_patch ? p * 4 + (unit ^ ((p >> 1) & 3)) : PATCH_U;
    s_ok |= (ok ? 1u : 0u) << j;
  }
  const uint4* wsrc = a.wgt + (size_t)co_tile * a.nchunks * WT_U + tid;
  const bool cin_tail = (a.Cin & 31) != 0;
  u32x4 sreg[R], wreg[WREG];
  auto fetch = [&](int cc) {
    const bool past = cin_tail && cc * 32 + (tid & 3) * 8 >= a.Cin;  // units past Cin: see k_conv3x3_flat
    const __half* src = a.in + (past ? 0 : cc * 32);
#pragma unroll
    for (int j = 0; j < R; ++j) sreg[j] = LDG(u32x4, src + (past ? 0 : s_g[j]), a.x_in);
#pragma unroll
    for (int j = 0; j < WREG; ++j)
      if (WT_U % 256 == 0 || tid + j * 256 < WT_U) wreg[j] = *reinterpret_cast<const u32x4*>(wsrc + (size_t)cc * WT_U + j * 256);
#pragma unroll
    for (int j = 0; j < R; ++j)
      if (past || !((s_ok >> j) & 1)) sreg[j] = u32x4{0, 0, 0, 0};
  };
  auto commit = [&]() {
#pragma unroll
    for (int j = 0; j < R; ++j) *reinterpret_cast<u32x4*>(patch + s_l[j]) = sreg[j];
#pragma unroll
    for (int j = 0; j < WREG; ++j) {
      const int idx = tid + j * 256;
      const int row = idx >> 2, unit = idx & 3;
      if (WT_U % 256 == 0 || idx < WT_U) *reinterpret_cast<u32x4*>(wt + row * 4 + (unit ^ ((row >> 1) & 3))) = wreg[j];
    }
  };
  fetch(0);

  int bpos[TAPS][2];
#pragma unroll
  for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int py = (wave * 2 + m) * S + tap / KS;
      const int px = (lane & 15) * S + tap % KS;
      const int col = EIOKU_PATCH_COL(px, PWH, S);
      const int p = py * PWS + col;
      bpos[tap][m] = p * 4 + ((lane >> 4) ^ ((p >> 1) & 3));
    }
  const uint4* wt_lane = wt + (lane & 15) * 4 + ((lane >> 4) ^ ((lane >> 1) & 3));

  float4v acc[2][NF];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[m][f] = float4v{0.f, 0.f, 0.f, 0.f};

  for (int cc = 0; cc < a.nchunks; ++cc) {
    commit();
    __syncthreads();
    if (cc + 1 < a.nchunks) fetch(cc + 1);  // in flight behind the 9 taps below
    __builtin_amdgcn_sched_barrier(0);
    mma_taps<NF, 2>(patch, wt_lane, bpos, acc);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
  }

  // ---- epilogue: lane = pixel (lane&15), 4 consecutive couts ((lane>>4)*4 + j) per fragment ----
  const int ow = ow0 + (lane & 15);
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int oh = oh0 + wave * 2 + m;
    if (oh >= a.Ho || ow >= a.Wo) continue;
    const unsigned opix = (unsigned)((n * a.Ho + oh) * a.Wo + ow);
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int c0 = co_tile * 16 * NF + f * 16 + (lane >> 4) * 4;
      store_frag(a, acc[m][f], opix, c0, *reinterpret_cast<const float4*>(a.bias + c0));
    }
  }
}

template <int NF, int S, int MT, int NS>
__global__ __launch_bounds__(256, 2) void k_conv3x3_flat(ConvArgs a, int npix, int PR, int PW) {
  constexpr int TAPS = 9, KS = 3;
  constexpr int WT_U = wt_units(NF);
  constexpr int WREG = (WT_U + 255) / 256;
  constexpr int TPX = 64 * MT;
  const TileLds L = flat_layout(NF, S, PR, PW);
  const int PWH = patch_half(PW);
  const int PWS = patch_pitch(PW, S);
  const int DUMMY = L.spare;  // one spare unit: where slots that carry nothing park their store

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* patch = reinterpret_cast<uint4*>(smem);
  uint4* wt = patch + L.wt;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P0 = blockIdx.x * TPX;
  const int co_tile = blockIdx.y;
  const int HW = a.Ho * a.Wo, VH = a.H + 1;
  const float r_hw = 1.0f / (float)HW, r_wo = 1.0f / (float)a.Wo, r_vh = 1.0f / (float)VH, r_pw = 1.0f / (float)PW;
  auto vrow = [&](int P) {
    const int n = fast_div(P, HW, r_hw), rem = P - n * HW;
    return n * VH + fast_div(rem, a.Wo, r_wo) * S;
  };
  const int Plast = (P0 + TPX < npix ? P0 + TPX : npix) - 1;
  const int v_lo = vrow(P0);
  const int rows = vrow(Plast) + KS - v_lo;

  // staging slots, branch-free in the chunk loop: a slot that maps to padding (or to nothing) loads element 0
  // and stores to the spare unit; the padding itself is zeroed once, below
  int s_g[NS], s_l[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int idx = tid + j * 256;
    const int pix = idx >> 2, unit = idx & 3;
    const int pr = fast_div(pix, PW, r_pw), pc = pix - pr * PW;
    const int v = v_lo + pr;
    const int n = fast_div(v, VH, r_vh), y = v - n * VH - 1, x = pc - 1;
    const bool ok = idx < rows * PW * 4 && y >= 0 && n < a.N && (unsigned)x < (unsigned)a.W;
    const int col = EIOKU_PATCH_COL(pc, PWH, S);
    const int p = pr * PWS + col;
    s_g[j] = ok ? ((n * a.H + y) * a.W + x) * a.in_cs + unit * 8 : 0;
    s_l[j] = ok ? p * 4 + (unit ^ ((p >> 1) & 3)) : DUMMY;
  }
  const uint4* wsrc = a.wgt + (size_t)co_tile * a.nchunks * WT_U + tid;
  u32x4 sreg[NS], wreg[WREG];
  const bool cin_tail = (a.Cin & 31) != 0;
  auto fetch = [&](int cc) {
    // a unit past Cin (Cin = 48, 80, ...) reads element 0 instead: at the last pixel of the tensor the real address
    // would lie past the end of the allocation (an unmapped page when the buffer ends on a page boundary)
    const bool past = cin_tail && cc * 32 + (tid & 3) * 8 >= a.Cin;
    const __half* src = a.in + (past ? 0 : cc * 32);
#pragma unroll
    for (int j = 0; j < NS; ++j) sreg[j] = LDG(u32x4, src + (past ? 0 : s_g[j]), a.x_in);
#pragma unroll
    for (int j = 0; j < WREG; ++j)
      if (WT_U % 256 == 0 || tid + j * 256 < WT_U) wreg[j] = *reinterpret_cast<const u32x4*>(wsrc + (size_t)cc * WT_U + j * 256);
    if (past) {  // channels past Cin (weights there are zero; the data may be anything)
#pragma unroll
      for (int j = 0; j < NS; ++j) sreg[j] = u32x4{0, 0, 0, 0};
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int j = 0; j < NS; ++j) *reinterpret_cast<u32x4*>(patch + s_l[j]) = sreg[j];
#pragma unroll
    for (int j = 0; j < WREG; ++j) {
      const int idx = tid + j * 256;
      const int row = idx >> 2, unit = idx & 3;
      if (WT_U % 256 == 0 || idx < WT_U) *reinterpret_cast<u32x4*>(wt + row * 4 + (unit ^ ((row >> 1) & 3))) = wreg[j];
    }
  };
  fetch(0);

  for (int i = tid; i < rows * PWS * 4; i += 256) patch[i] = make_uint4(0, 0, 0, 0);

  // B-fragment positions of this lane's MT pixels for the 9 taps
  int bpos[TAPS][MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    int P = P0 + (wave * MT + m) * 16 + (lane & 15);
    if (P > Plast) P = Plast;
    const int n = fast_div(P, HW, r_hw), rem = P - n * HW;
    const int yo = fast_div(rem, a.Wo, r_wo), xo = rem - yo * a.Wo;
    const int pr0 = n * VH + yo * S - v_lo;
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      const int pc = xo * S + tap % KS;
      const int col = EIOKU_PATCH_COL(pc, PWH, S);
      const int p = (pr0 + tap / KS) * PWS + col;
      bpos[tap][m] = p * 4 + ((lane >> 4) ^ ((p >> 1) & 3));
    }
  }
  const uint4* wt_lane = wt + (lane & 15) * 4 + ((lane >> 4) ^ ((lane >> 1) & 3));

  float4v acc[MT][NF];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[m][f] = float4v{0.f, 0.f, 0.f, 0.f};

  __syncthreads();  // zero fill complete before the first commit
  for (int cc = 0; cc < a.nchunks; ++cc) {
    commit();
    __syncthreads();
    if (cc + 1 < a.nchunks) fetch(cc + 1);  // in flight behind the 9 taps below
    __builtin_amdgcn_sched_barrier(0);
    mma_taps<NF, MT>(patch, wt_lane, bpos, acc);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
  }

  // ---- epilogue: one uniform choice, then (r4) MT rows of NF straight-line stores.  A residual is loaded for all
  // MT * NF fragments up front (pixels past the end re-read the last one): one round trip per workgroup where
  // store_frag's load -> vmcnt(0) -> add -> store made it one per fragment ----
  const int c_first = co_tile * 16 * NF + (lane >> 4) * 4;
  auto fast = [&](auto tag) {
    constexpr int E = decltype(tag)::value;
    float4 b[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) b[f] = *reinterpret_cast<const float4*>(a.bias + c_first + f * 16);
    u32x2 r[MT][NF];
    unsigned Pc[MT];
    bool ok[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int P = P0 + (wave * MT + m) * 16 + (lane & 15);
      ok[m] = P <= Plast;
      Pc[m] = (unsigned)(ok[m] ? P : Plast);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        r[m][f] = u32x2{0, 0};
        if (E == kEpiRes) r[m][f] = LDG(u32x2, a.res + (size_t)(Pc[m] * (unsigned)a.res_cs + (unsigned)(c_first + f * 16)), a.x_res);
      }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
      epi_store_row<E, NF>(a, acc[m], b, r[m], a.out + (size_t)(Pc[m] * (unsigned)a.out_cs + (unsigned)c_first), ok[m]);
  };
  switch (epi_variant(a, (co_tile + 1) * 16 * NF, a.res != nullptr && a.Cout >= 4)) {
    case kEpiPlain: fast(EpiTag<kEpiPlain>{}); return;
    case kEpiRes: fast(EpiTag<kEpiRes>{}); return;
    default: break;
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int P = P0 + (wave * MT + m) * 16 + (lane & 15);
    if (P > Plast) continue;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int c0 = co_tile * 16 * NF + f * 16 + (lane >> 4) * 4;
      store_frag(a, acc[m][f], (unsigned)P, c0, *reinterpret_cast<const float4*>(a.bias + c0));
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Persistent 3x3 variant for the layers that dominate the pixel count (Cin <= 96): the whole weight
// block of the cout tile (NCH chunks x 9 taps) stays in LDS for the launch, workgroups walk the
// output tiles grid-stride, and the NEXT tile's halo patch is already in flight (registers) while the
// current one is multiplied: one barrier per tile, HBM latency hidden behind the MFMAs.
// ---------------------------------------------------------------------------------------------
template <int NF, int S, int NCH, bool DB, bool POST = false, int NWV = 4>
__global__ __launch_bounds__(64 * NWV) void k_conv3x3_persist(ConvArgs a, int total_tiles) {
  // NWV waves per workgroup, two output rows each: 8x16 tiles (4 waves) or, for the layers whose weight block leaves
  // room for one workgroup per CU only, 16x16 tiles (8 waves: two waves per SIMD instead of one)
  constexpr int KS = 3, TAPS = 9, PAD = 1, kTH = 2 * NWV, NT = 64 * NWV;
  constexpr Patch G = patch_of(kTH, S);
  constexpr PersistLds L = persist_layout(NF, S, NCH, DB, POST, NWV);
  constexpr int PH = G.ph, PW = G.pw, PWH = G.pwh, PWS = G.pws;
  constexpr int PATCH_U = L.patch_u;              // per chunk
  constexpr int WT_U = wt_units(NF);              // per chunk
  constexpr int NLOAD = PH * PW * 4 * NCH;        // staged units per tile
  constexpr int R = (NLOAD + NT - 1) / NT;          // per thread
  static_assert(R <= 32, "slot mask is one 32-bit word");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* wt = reinterpret_cast<uint4*>(smem);                 // [NCH][WT_U]
  uint4* patch = wt + L.patch;                                // [DB ? 2 : 1][NCH][PATCH_U] (+ 1 spare unit)
  // POST: the 1x1 that consumes this conv's output runs here, on the tile still in registers (the intermediate
  // tensor is never written): its weights [NCH2][16*NF][4 units] and a per-wave [32 px][2*NF units] staging tile
  constexpr int U1 = 2 * NF;          // 16-byte units per pixel of the intermediate (16*NF channels)
  constexpr int NCH2 = (NF + 1) / 2;  // 32-channel chunks of the 1x1's K axis
  static_assert(!POST || NF % 2 == 0, "fused 1x1 needs a multiple of 32 intermediate channels");
  uint4* wt2 = wt + L.wt2;                                    // [NCH2][16*NF][4]
  uint4* tbuf = wt + L.tbuf;                                  // [NWV waves][32][U1]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int co_tile = blockIdx.y;
  // per-thread staging slots: slot j -> (chunk, pixel, unit) is tile independent.  The tile loop is branch-free:
  // every slot loads (element 0 when it has nothing to fetch) and stores (to the spare unit when it maps to no
  // patch position); padding is a select to zero at store time, skipped by whole waves on interior tiles.
  int s_off[R];                    // LDS unit index inside one patch buffer (spare unit for unused slots)
  int s_py[R], s_px[R], s_rel[R];  // s_rel: element offset of the slot relative to the tile's (ih0, iw0) pixel
  unsigned s_live = 0;             // bit j: slot j fetches (inside the patch and below Cin)
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int idx = tid + NT * j;
    const int cc = idx / (PH * PW * 4), rem = idx - cc * (PH * PW * 4);
    const int pix = rem >> 2, unit = rem & 3;
    const int py = pix / PW, px = pix - py * PW;
    const int col = EIOKU_PATCH_COL(px, PWH, S);
    const int p = py * PWS + col;
    const bool in_patch = idx < NLOAD;
    s_off[j] = in_patch ? cc * PATCH_U + p * 4 + (unit ^ ((p >> 1) & 3)) : L.spare;
    s_py[j] = py;
    s_px[j] = px;
    s_rel[j] = (py * a.W + px) * a.in_cs + cc * 32 + unit * 8;
    if (in_patch && cc * 32 + unit * 8 < a.Cin) s_live |= 1u << j;
  }
  const int tiles_per_img = a.tiles_w * a.tiles_h;
  const float r_tpi = 1.0f / (float)tiles_per_img, r_tw = 1.0f / (float)a.tiles_w;
  u32x4 stage[R];
  unsigned s_ok = 0;  // bit j: slot j of the staged tile holds fetched data (else zero padding)
  int nx_n = 0, nx_th = 0, nx_tw = 0;  // coordinates of the staged tile
  auto issue = [&](int tile) {
    tile = xcd_tile(tile, total_tiles);
    nx_n = fast_div(tile, tiles_per_img, r_tpi);
    const int t2 = tile - nx_n * tiles_per_img;
    nx_th = fast_div(t2, a.tiles_w, r_tw);
    nx_tw = t2 - nx_th * a.tiles_w;
    const int ih0 = nx_th * kTH * S - PAD, iw0 = nx_tw * kTW * S - PAD;
    const int base = ((nx_n * a.H + ih0) * a.W + iw0) * a.in_cs;  // may be negative; only in-range slots use it
    s_ok = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int ih = ih0 + s_py[j], iw = iw0 + s_px[j];
      const bool ok = ((s_live >> j) & 1) && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
      s_ok |= (ok ? 1u : 0u) << j;
      stage[j] = LDG(u32x4, a.in + (ok ? base + s_rel[j] : 0), a.x_in);
    }
  };

  // B-fragment unit positions inside a chunk's patch: they depend on (lane, tap, m) only
  int bpos[TAPS][2];
#pragma unroll
  for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int py = (wave * 2 + m) * S + tap / KS;
      const int px = (lane & 15) * S + tap % KS;
      const int col = EIOKU_PATCH_COL(px, PWH, S);
      const int p = py * PWS + col;
      bpos[tap][m] = p * 4 + ((lane >> 4) ^ ((p >> 1) & 3));
    }
  const uint4* wt_lane = wt + (lane & 15) * 4 + ((lane >> 4) ^ ((lane >> 1) & 3));
  float4 biasr[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f)
    biasr[f] = *reinterpret_cast<const float4*>(a.bias + co_tile * 16 * NF + f * 16 + (lane >> 4) * 4);
  const bool res_vec = a.res != nullptr && a.Cout >= 4;  // vector residual path (slices are 4-channel aligned)

  int tile = blockIdx.x;
  if (tile < total_tiles) issue(tile);  // first patch in flight while the weight block is copied
  {
    const uint4* wsrc = a.wgt + (size_t)co_tile * NCH * WT_U;
    constexpr int NW = NCH * WT_U;
    constexpr int WB = 8;  // loads in flight per thread
    for (int i0 = 0; i0 < NW; i0 += NT * WB) {
      u32x4 w[WB];
#pragma unroll
      for (int j = 0; j < WB; ++j) {
        const int idx = i0 + j * NT + tid;
        w[j] = *reinterpret_cast<const u32x4*>(wsrc + (idx < NW ? idx : 0));
      }
#pragma unroll
      for (int j = 0; j < WB; ++j) {
        const int idx = i0 + j * NT + tid;
        const int row = (idx % WT_U) >> 2, unit = idx & 3;
        if (idx < NW) *reinterpret_cast<u32x4*>(wt + (idx & ~3) + (unit ^ ((row >> 1) & 3))) = w[j];
      }
    }
  }
  float4 biasr2[NF];
  const uint4* wt2_lane = wt2 + (lane & 15) * 4 + ((lane >> 4) ^ ((lane >> 1) & 3));
  if (POST) {
    for (int idx = tid; idx < NCH2 * 16 * NF * 4; idx += NT) {
      const int row = (idx >> 2) % (16 * NF), unit = idx & 3;
      *reinterpret_cast<u32x4*>(wt2 + (idx & ~3) + (unit ^ ((row >> 1) & 3))) = *reinterpret_cast<const u32x4*>(a.post_w + idx);
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) biasr2[f] = *reinterpret_cast<const float4*>(a.post_bias + f * 16 + (lane >> 4) * 4);
  }
  int buf = 0;
  for (; tile < total_tiles; tile += gridDim.x) {
    uint4* pb = patch + (DB ? buf : 0) * (NCH * PATCH_U);
    if (!DB) __syncthreads();  // single buffer: every wave is done reading the previous tile
    if (s_ok != s_live) {      // border tile (or channel tail): padding slots become zero
#pragma unroll
      for (int j = 0; j < R; ++j)
        if (!((s_ok >> j) & 1)) stage[j] = u32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int j = 0; j < R; ++j) *reinterpret_cast<u32x4*>(pb + s_off[j]) = stage[j];
    __syncthreads();  // also orders the weight copy before the first tile
    const int tn = nx_n, tth = nx_th, ttw = nx_tw;
    const int ow = ttw * kTW + (lane & 15);
    // residual of THIS tile first, then the next tile's patch, so that the residual loads are the older entries of the
    // in-order vmcnt queue.  (That alone does not keep the prefetch in flight: store_frag's run-time branches hide the
    // count from the compiler, and the ISA waits with vmcnt(0) - prefetch included - before the first residual add.)
    u32x2 resv[2][NF];
    if (res_vec) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int oh = tth * kTH + wave * 2 + m;
        const bool ok = oh < a.Ho && ow < a.Wo;
        const unsigned opix = (unsigned)((tn * a.Ho + (ok ? oh : 0)) * a.Wo + (ok ? ow : 0));
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const int c0 = co_tile * 16 * NF + f * 16 + (lane >> 4) * 4;
          resv[m][f] = LDG(u32x2, a.res + (size_t)(opix * (unsigned)a.res_cs + (unsigned)(c0 + 3 < a.Cout ? c0 : 0)), a.x_res);
        }
      }
    }
    const int next = tile + gridDim.x;
    if (next < total_tiles) issue(next);  // in flight during the MFMAs below
    __builtin_amdgcn_sched_barrier(0);

    float4v acc[2][NF];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[m][f] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cc = 0; cc < NCH; ++cc) mma_taps<NF, 2>(pb + cc * PATCH_U, wt_lane + cc * WT_U, bpos, acc);
    __builtin_amdgcn_sched_barrier(0);
    if (POST) {
      // this wave's 32 pixels x 16*NF activated channels -> its LDS tile in B-operand layout (no other wave reads
      // it: LDS operations of one wave execute in order, the wave barrier only stops the compiler reordering)
      uint4* tw = tbuf + wave * 32 * U1;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const float4v v = activate_frag(a, acc[m][f], biasr[f]);
          const f16x4 h = __builtin_convertvector(v, f16x4);
          const int px = m * 16 + (lane & 15);
          const int unit = f * 2 + (lane >> 5), half = (lane >> 4) & 1;
          const int sw = (unit & ~3) | ((unit & 3) ^ ((px >> 1) & 3));
          *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(tw + px * U1 + sw) + half * 8) = __builtin_bit_cast(u32x2, h);
        }
      __builtin_amdgcn_wave_barrier();
      float4v acc2[2][NF];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int f = 0; f < NF; ++f) acc2[m][f] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < NCH2; ++kc) {
        half8 bf[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const int px = m * 16 + (lane & 15);
          uint4 u = tw[px * U1 + kc * 4 + ((lane >> 4) ^ ((px >> 1) & 3))];
          bf[m] = *reinterpret_cast<half8*>(&u);
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          uint4 w = wt2_lane[(kc * NF + f) * 64];
          const half8 af = *reinterpret_cast<half8*>(&w);
#pragma unroll
          for (int m = 0; m < 2; ++m) acc2[m][f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[m], acc2[m][f], 0, 0, 0);
        }
      }
      __builtin_amdgcn_wave_barrier();
      ConvArgs a2 = a;
      a2.out = a.post_out;
      a2.out_cs = a.post_out_cs;
      a2.Cout = a.post_cout;
      a2.act = a.post_act;
      a2.res = nullptr;
      a2.out_f32 = nullptr;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int oh = tth * kTH + wave * 2 + m;
        if (oh >= a.Ho || ow >= a.Wo) continue;
        const unsigned opix = (unsigned)((tn * a.Ho + oh) * a.Wo + ow);
#pragma unroll
        for (int f = 0; f < NF; ++f) store_frag(a2, acc2[m][f], opix, f * 16 + (lane >> 4) * 4, biasr2[f]);
      }
    } else {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int oh = tth * kTH + wave * 2 + m;
        if (oh >= a.Ho || ow >= a.Wo) continue;
        const unsigned opix = (unsigned)((tn * a.Ho + oh) * a.Wo + ow);
#pragma unroll
        for (int f = 0; f < NF; ++f)
          store_frag(a, acc[m][f], opix, co_tile * 16 * NF + f * 16 + (lane >> 4) * 4, biasr[f], res_vec, resv[m][f]);
      }
    }
    buf ^= 1;
  }
}

// ---------------------------------------------------------------------------------------------
// Two chained 3x3 stride-1 convolutions (a C2f Bottleneck: cv1 -> cv2 [+ x]) as ONE persistent launch for the
// shallow layers (16 / 32 channels at 160^2 / 80^2) that are bound by memory traffic and launch count, not by
// MFMA: the intermediate tensor lives only in LDS.  Per 8x16 output tile the workgroup stages the 12x20 input
// halo patch X, evaluates conv A on the 10x18 pixels conv B needs (12 fragments of 16 flattened patch pixels:
// 1.4x conv A's MFMAs, which are idle anyway), writes act(A) as fp16 into the LDS patch P1 with ZEROS where the
// pixel lies outside the map (that is conv B's padding), runs conv B out of P1 and adds the residual -- the
// Bottleneck's own input, i.e. the centre of X -- from LDS.  Values are rounded exactly where the two separate
// launches round them (fp16 intermediate, fp16(fp16(y) + x) residual), so the result is bit-identical.
// HBM per pair: 1.9x-halo read + 1 write instead of 2 reads + residual read + 2 writes.
// ---------------------------------------------------------------------------------------------
// CAT > 0 (C2f with one Bottleneck): the C2f's closing 1x1 over the concat [y0 | y1 | y2] runs here as well.  y2 =
// this launch's output never leaves the CU: each wave writes its 32 pixels of it over the centre of the staged input
// patch (its own residual pixels, already consumed), the CAT leading 32-channel chunks of the concat (y0 | y1) come
// straight from HBM as B fragments (issued before conv A, so their latency is hidden), and the 1x1's weights sit in
// LDS.  Same chunk order and operands as k_conv1x1: bit-identical.  model.2: -157 MB and one launch per forward.
struct ChainCat {
  const uint4* w;      // the 1x1's packed weights [(CAT + 1) chunks][16*NF2][4 units]
  const float* bias;
  __half* out;         // its output slice
  int out_cs, act;
  const __half* cat;   // channel 0 of the concat buffer
  int cat_cs;
  BcExt x_cat, x_out;  // bounds-check build
};

template <int NF, bool DB, int CAT = 0, int NF2 = 2>
__global__ __launch_bounds__(256) void k_conv3x3_chain(ConvArgs a, ChainCat cc, int total_tiles) {
  constexpr int XH = kTH + 4, XW = kTW + 4;  // input patch
  constexpr int PH = kTH + 2, PW = kTW + 2;  // intermediate patch
  constexpr ChainLds L = chain_layout(NF, DB, CAT, NF2);
  constexpr int X_U = L.x_u, P_U = L.p_u;
  static_assert(X_U == XH * XW * 4 && P_U == PH * PW * 4, "the layout's patches are this kernel's");
  constexpr int WT_U = wt_units(NF);
  constexpr int NLOAD = X_U;
  constexpr int R = (NLOAD + 255) / 256;
  constexpr int NPA = PH * PW;           // conv A pixels per tile
  constexpr int MA = (NPA + 63) / 64;    // conv A fragments per wave
  static_assert(NF == 1 || NF == 2, "one 32-channel chunk on both convolutions");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* wtA = reinterpret_cast<uint4*>(smem);
  uint4* wtB = wtA + L.wtB;
  uint4* xbuf = wtA + L.xbuf;                   // [DB ? 2 : 1][X_U] + 4 spare units
  uint4* p1 = wtA + L.p1;                       // [P_U] + 4 spare units (stores of the last fragment's tail)
  uint4* wt2 = wtA + L.wt2;                     // CAT: [(CAT + 1)][16*NF2][4]
  constexpr int W2_U = L.w2_u;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int s_off[R], s_py[R], s_px[R], s_rel[R];
  unsigned s_live = 0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int idx = tid + 256 * j;
    const int pix = idx >> 2, unit = idx & 3;
    const int py = pix / XW, px = pix - py * XW;
    const bool in_patch = idx < NLOAD;
    s_off[j] = in_patch ? pix * 4 + (unit ^ ((pix >> 1) & 3)) : (DB ? 2 : 1) * X_U;
    s_py[j] = py;
    s_px[j] = px;
    s_rel[j] = (py * a.W + px) * a.in_cs + unit * 8;
    if (in_patch && unit * 8 < a.Cin) s_live |= 1u << j;
  }
  const int tiles_per_img = a.tiles_w * a.tiles_h;
  const float r_tpi = 1.0f / (float)tiles_per_img, r_tw = 1.0f / (float)a.tiles_w;
  u32x4 stage[R];
  unsigned s_ok = 0;
  int nx_n = 0, nx_th = 0, nx_tw = 0;
  auto issue = [&](int tile) {
    tile = xcd_tile(tile, total_tiles);
    nx_n = fast_div(tile, tiles_per_img, r_tpi);
    const int t2 = tile - nx_n * tiles_per_img;
    nx_th = fast_div(t2, a.tiles_w, r_tw);
    nx_tw = t2 - nx_th * a.tiles_w;
    const int ih0 = nx_th * kTH - 2, iw0 = nx_tw * kTW - 2;
    const int base = ((nx_n * a.H + ih0) * a.W + iw0) * a.in_cs;
    s_ok = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int ih = ih0 + s_py[j], iw = iw0 + s_px[j];
      const bool ok = ((s_live >> j) & 1) && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
      s_ok |= (ok ? 1u : 0u) << j;
      stage[j] = LDG(u32x4, a.in + (ok ? base + s_rel[j] : 0), a.x_in);
    }
  };

  // conv A: fragment m of this wave = flattened P1 pixels (wave + 4m)*16 .. +15 (clamped: the last fragment's
  // tail computes pixel NPA-1 again and stores nothing)
  int bposA[9][MA];
  int pa_st[MA][NF], pa_y[MA], pa_x[MA];  // pa_st: byte offset in P1 of this lane's 4 channels of fragment (m, f)
#pragma unroll
  for (int m = 0; m < MA; ++m) {
    const int praw = (wave + 4 * m) * 16 + (lane & 15);
    const int p = praw < NPA ? praw : NPA - 1;
    const int py = p / PW, px = p - py * PW;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int unit = f * 2 + (lane >> 5), half = (lane >> 4) & 1;
      pa_st[m][f] = (praw < NPA ? p * 4 + (unit ^ ((p >> 1) & 3)) : P_U + unit) * 16 + half * 8;
    }
    pa_y[m] = py;
    pa_x[m] = px;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int pos = (py + tap / 3) * XW + px + tap % 3;
      bposA[tap][m] = pos * 4 + ((lane >> 4) ^ ((pos >> 1) & 3));
    }
  }
  int bposB[9][2];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int p = (wave * 2 + m + tap / 3) * PW + (lane & 15) + tap % 3;
      bposB[tap][m] = p * 4 + ((lane >> 4) ^ ((p >> 1) & 3));
    }
  const int wsel = (lane & 15) * 4 + ((lane >> 4) ^ ((lane >> 1) & 3));
  const uint4* wtA_lane = wtA + wsel;
  const uint4* wtB_lane = wtB + wsel;
  float4 biasA[NF], biasB[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    biasA[f] = *reinterpret_cast<const float4*>(a.bias + f * 16 + (lane >> 4) * 4);
    biasB[f] = *reinterpret_cast<const float4*>(a.post_bias + f * 16 + (lane >> 4) * 4);
  }

  int tile = blockIdx.x;
  if (tile < total_tiles) issue(tile);
  {
    constexpr int NW = 2 * WT_U, WB = 8;
    for (int i0 = 0; i0 < NW; i0 += 256 * WB) {
      u32x4 w[WB];
#pragma unroll
      for (int j = 0; j < WB; ++j) {
        const int idx = i0 + j * 256 + tid;
        const int k = idx < NW ? idx : 0;
        w[j] = *reinterpret_cast<const u32x4*>(k < WT_U ? a.wgt + k : a.post_w + (k - WT_U));
      }
#pragma unroll
      for (int j = 0; j < WB; ++j) {
        const int idx = i0 + j * 256 + tid;
        const int row = (idx % WT_U) >> 2, unit = idx & 3;
        if (idx < NW) *reinterpret_cast<u32x4*>(wtA + (idx & ~3) + (unit ^ ((row >> 1) & 3))) = w[j];
      }
    }
    // channels 16*NF..31 of P1 are never written: they must read as zero, not as whatever LDS held
    for (int i = tid; i < P_U; i += 256) *reinterpret_cast<u32x4*>(p1 + i) = u32x4{0, 0, 0, 0};
    if (CAT > 0) {
      for (int idx = tid; idx < W2_U; idx += 256) {
        const int row = (idx >> 2) % (16 * NF2), unit = idx & 3;
        *reinterpret_cast<u32x4*>(wt2 + (idx & ~3) + (unit ^ ((row >> 1) & 3))) = *reinterpret_cast<const u32x4*>(cc.w + idx);
      }
    }
  }
  const uint4* wt2_lane = wt2 + wsel;
  float4 bias2[NF2];
  if (CAT > 0) {
#pragma unroll
    for (int f = 0; f < NF2; ++f) bias2[f] = *reinterpret_cast<const float4*>(cc.bias + f * 16 + (lane >> 4) * 4);
  }
  int buf = 0;
  for (; tile < total_tiles; tile += gridDim.x) {
    uint4* xb = xbuf + (DB ? buf : 0) * X_U;
    if (!DB) __syncthreads();  // every wave is done with the previous tile's X (residual) and P1
    if (s_ok != s_live) {
#pragma unroll
      for (int j = 0; j < R; ++j)
        if (!((s_ok >> j) & 1)) stage[j] = u32x4{0, 0, 0, 0};
    }
#pragma unroll
    for (int j = 0; j < R; ++j) *reinterpret_cast<u32x4*>(xb + s_off[j]) = stage[j];
    __syncthreads();
    const int tn = nx_n, tth = nx_th, ttw = nx_tw;
    // CAT: the concat's leading chunks for this wave's 32 pixels (clamped into the map), older than the next tile's
    // prefetch in the vmcnt queue so that waiting for them leaves the prefetch in flight
    u32x4 gB[CAT > 0 ? CAT : 1][2];
    if (CAT > 0) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        int oh = tth * kTH + wave * 2 + m, owc = ttw * kTW + (lane & 15);
        if (oh >= a.Ho) oh = a.Ho - 1;
        if (owc >= a.Wo) owc = a.Wo - 1;
        const __half* src = cc.cat + (((size_t)tn * a.Ho + oh) * a.Wo + owc) * cc.cat_cs + (lane >> 4) * 8;
#pragma unroll
        for (int c = 0; c < CAT; ++c) gB[c][m] = LDG(u32x4, src + c * 32, cc.x_cat);
      }
    }
    const int next = tile + gridDim.x;
    if (next < total_tiles) issue(next);
    __builtin_amdgcn_sched_barrier(0);

    {
      float4v acc[MA][NF];
#pragma unroll
      for (int m = 0; m < MA; ++m)
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[m][f] = float4v{0.f, 0.f, 0.f, 0.f};
      mma_taps<NF, MA>(xb, wtA_lane, bposA, acc);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m = 0; m < MA; ++m) {
        const int ah = tth * kTH - 1 + pa_y[m], aw = ttw * kTW - 1 + pa_x[m];
        const bool inmap = (unsigned)ah < (unsigned)a.H && (unsigned)aw < (unsigned)a.W;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const float4v v = activate_frag(a, acc[m][f], biasA[f]);
          const f16x4 h = __builtin_convertvector(v, f16x4);
          const u32x2 hv = inmap ? __builtin_bit_cast(u32x2, h) : u32x2{0, 0};
          *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(p1) + pa_st[m][f]) = hv;
        }
      }
    }
    __syncthreads();

    float4v acc[2][NF];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[m][f] = float4v{0.f, 0.f, 0.f, 0.f};
    mma_taps<NF, 2>(p1, wtB_lane, bposB, acc);
    __builtin_amdgcn_sched_barrier(0);
    const int ow = ttw * kTW + (lane & 15);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int oh = tth * kTH + wave * 2 + m;
      const int pos = (2 + wave * 2 + m) * XW + 2 + (lane & 15);
      u32x2 resv[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int unit = f * 2 + (lane >> 5), half = (lane >> 4) & 1;
        resv[f] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const char*>(xb + pos * 4 + (unit ^ ((pos >> 1) & 3))) + half * 8);
      }
      if (CAT == 0 && (oh >= a.Ho || ow >= a.Wo)) continue;
      const unsigned opix = (unsigned)((tn * a.Ho + oh) * a.Wo + ow);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        // Cout = 16*NF exactly: always the full-vector store of store_frag, same roundings
        float4v v = acc[m][f] + float4v{biasB[f].x, biasB[f].y, biasB[f].z, biasB[f].w};
        if (a.post_act == kActSiLU) {
          v = silu4(v);
        }
        f16x4 h = __builtin_convertvector(v, f16x4);
        if (a.res) {
          const float4v sum = __builtin_convertvector(h, float4v) + __builtin_convertvector(__builtin_bit_cast(f16x4, resv[f]), float4v);
          h = __builtin_convertvector(sum, f16x4);
        }
        if (CAT > 0) {  // y2 -> this pixel's slot of the staged patch (the residual above was its last reader)
          const int unit = f * 2 + (lane >> 5), half = (lane >> 4) & 1;
          *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(xb + pos * 4 + (unit ^ ((pos >> 1) & 3))) + half * 8) = __builtin_bit_cast(u32x2, h);
        } else {
          STG(u32x2, a.post_out + (size_t)(opix * (unsigned)a.post_out_cs + (unsigned)(f * 16 + (lane >> 4) * 4)), __builtin_bit_cast(u32x2, h), a.x_out);
        }
      }
    }
    if (CAT > 0) {
      __builtin_amdgcn_wave_barrier();  // this wave's own LDS writes above, read back below: in order, no barrier needed
      float4v acc2[2][NF2];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int f = 0; f < NF2; ++f) acc2[m][f] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c <= CAT; ++c) {
        half8 bf[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          if (c < CAT) {
            bf[m] = __builtin_bit_cast(half8, gB[c < CAT ? c : 0][m]);
          } else {
            const int pos = (2 + wave * 2 + m) * XW + 2 + (lane & 15);
            uint4 u = xb[pos * 4 + ((lane >> 4) ^ ((pos >> 1) & 3))];
            bf[m] = *reinterpret_cast<half8*>(&u);
          }
        }
#pragma unroll
        for (int f = 0; f < NF2; ++f) {
          uint4 w = wt2_lane[(c * NF2 + f) * 64];
          const half8 af = *reinterpret_cast<half8*>(&w);
#pragma unroll
          for (int m = 0; m < 2; ++m) acc2[m][f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[m], acc2[m][f], 0, 0, 0);
        }
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int oh = tth * kTH + wave * 2 + m;
        if (oh >= a.Ho || ow >= a.Wo) continue;
        const unsigned opix = (unsigned)((tn * a.Ho + oh) * a.Wo + ow);
#pragma unroll
        for (int f = 0; f < NF2; ++f) {
          float4v v = acc2[m][f] + float4v{bias2[f].x, bias2[f].y, bias2[f].z, bias2[f].w};
          if (cc.act == kActSiLU) v = silu4(v);
          const f16x4 h = __builtin_convertvector(v, f16x4);
          STG(u32x2, cc.out + (size_t)(opix * (unsigned)cc.out_cs + (unsigned)(f * 16 + (lane >> 4) * 4)), __builtin_bit_cast(u32x2, h), cc.x_out);
        }
      }
    }
    buf ^= 1;
  }
}

// ---------------------------------------------------------------------------------------------
// Stem variant (Cin = 8: RGB + 5 zero channels, stride 2).  The generic kernels pad the 8 channels to a
// 32-channel chunk (3/4 of every MFMA and of every LDS byte is zero); here the K axis of a chunk is
// 4 TAPS x 8 channels instead: lane group q of a B fragment reads the pixel of tap 4j+q, so the 3x3
// window is 3 MFMA k-steps instead of 9 and the LDS patch holds one 16-byte unit per pixel.
// SRC 0: fp16 NHWC input.  SRC 1 / 2: the letterboxed network input never exists in memory -- the
// staging slots read the BGR u8 frame (copy / exact 1/2 area modes of K3, same integer arithmetic,
// same fp16 rounding of v/255, 114 grey outside the image) and build the unit on the way to LDS.
// ---------------------------------------------------------------------------------------------
typedef unsigned u32_unaligned __attribute__((aligned(1)));

struct FusedSrc {
  const uint8_t* bgr;
  int src_h, src_w, new_h, new_w, top, left;
  int step = 1, off = 0;  // SRC 1: source pixel of image pixel (y, x) = (step y + off, step x + off)
};

template <int NF, int S, int SRC>
__global__ __launch_bounds__(256) void k_conv3x3_c8(ConvArgs a, FusedSrc fs, int total_tiles) {
  constexpr int KS = 3, PAD = 1;
  constexpr Patch G = patch_of(kTH, S);
  constexpr C8Lds L = c8_layout(NF, S);
  constexpr int PH = G.ph, PW = G.pw, PWH = G.pwh, PWS = G.pws;
  constexpr int PATCH_U = L.patch_u;  // one unit per pixel (+ spare for idle slots)
  constexpr int NPIX = PH * PW;
  constexpr int R = (NPIX + 255) / 256;
  constexpr int ROWS = 16 * NF;
  constexpr int NB = SRC == 0 ? 1 : (SRC == 1 ? 3 : 12);  // raw registers per slot
  // SRC 3 (copy mode, frame rows / padding 4-pixel aligned): a slot is a GROUP of 4 pixels = 12 bytes = one
  // aligned dwordx3 load; the staged columns start 3 pixels left of the patch (x = 32*tw - 4) so that groups
  // never straddle the image edge.  153 groups per tile: one per thread.
  constexpr int GPR = (PW + 3 + 3) / 4;  // groups per patch row
  static_assert(SRC != 3 || (PH * GPR <= 256 && S == 2), "one group per thread");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* wt = reinterpret_cast<uint4*>(smem);  // [3 k-steps][ROWS][4 taps] swizzled per row
  uint4* patch = wt + L.patch;                 // [2][PATCH_U]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int co_tile = blockIdx.y;
  {
    const uint4* wsrc = a.wgt + (size_t)co_tile * (9 * ROWS * 4);  // packed [tap][row][4 units]; unit 0 = channels 0..7
    for (int idx = tid; idx < 3 * ROWS * 4; idx += 256) {
      const int j = idx / (ROWS * 4), row = (idx >> 2) % ROWS, q = idx & 3;
      const int tap = 4 * j + q;
      u32x4 v = u32x4{0, 0, 0, 0};
      if (tap < 9) v = *reinterpret_cast<const u32x4*>(wsrc + (tap * ROWS + row) * 4);
      *reinterpret_cast<u32x4*>(wt + (idx & ~3) + (q ^ ((row >> 1) & 3))) = v;
    }
  }
  int g_off[4] = {0, 0, 0, 0};
  const int g_py = tid / GPR, g_x = (tid - g_py * GPR) * 4 - 3;  // first pixel of the group, patch coordinates
  if (SRC == 3) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int px = g_x + i;
      const int col = EIOKU_PATCH_COL(px, PWH, S);
      g_off[i] = (tid < PH * GPR && px >= 0 && px < PW) ? g_py * PWS + col : PATCH_U - 1;
    }
  }
  u32x3 graw = u32x3{0, 0, 0};
  int s_off[R], s_py[R], s_px[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int idx = tid + 256 * j;
    const int py = idx / PW, px = idx - py * PW;
    const int col = EIOKU_PATCH_COL(px, PWH, S);
    s_off[j] = idx < NPIX ? py * PWS + col : PATCH_U - 1;
    s_py[j] = py;
    s_px[j] = px;
  }
  const int tiles_per_img = a.tiles_w * a.tiles_h;
  const float r_tpi = 1.0f / (float)tiles_per_img, r_tw = 1.0f / (float)a.tiles_w;
  u32x4 stage[SRC == 0 ? R : 1];
  unsigned raw[SRC == 0 ? 1 : R][NB];
  unsigned s_in = 0, s_img = 0;  // bit j: slot inside the network input / inside the image (fused modes)
  int nx_n = 0, nx_th = 0, nx_tw = 0;
  auto issue = [&](int tile) {
    tile = xcd_tile(tile, total_tiles);
    nx_n = fast_div(tile, tiles_per_img, r_tpi);
    const int t2 = tile - nx_n * tiles_per_img;
    nx_th = fast_div(t2, a.tiles_w, r_tw);
    nx_tw = t2 - nx_th * a.tiles_w;
    const int ih0 = nx_th * kTH * S - PAD, iw0 = nx_tw * kTW * S - PAD;
    s_in = 0;
    s_img = 0;
    if (SRC == 3) {
      const int ih = ih0 + g_py, iw = iw0 + g_x;  // iw is a multiple of 4; so are W, left and new_w
      const bool in = tid < PH * GPR && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
      const int y = ih - fs.top, x = iw - fs.left;
      const bool img = in && (unsigned)y < (unsigned)fs.new_h && (unsigned)x < (unsigned)fs.new_w;
      s_in = in;
      s_img = img;
      graw = LDG(u32x3, fs.bgr + (img ? ((size_t)(nx_n * fs.src_h + y) * fs.src_w + x) * 3 : 0), a.x_img);
      return;
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int ih = ih0 + s_py[j], iw = iw0 + s_px[j];
      const bool in = (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
      s_in |= (in ? 1u : 0u) << j;
      if (SRC == 0) {
        stage[j] = LDG(u32x4, a.in + (in ? ((size_t)(nx_n * a.H + ih) * a.W + iw) * a.in_cs : 0), a.x_in);
      } else {
        const int y = ih - fs.top, x = iw - fs.left;
        const bool img = in && (unsigned)y < (unsigned)fs.new_h && (unsigned)x < (unsigned)fs.new_w;
        s_img |= (img ? 1u : 0u) << j;
        const uint8_t* f = fs.bgr + (size_t)nx_n * fs.src_h * fs.src_w * 3;
        if (SRC == 1) {
          const uint8_t* p = f + (img ? ((size_t)(y * fs.step + fs.off) * fs.src_w + (x * fs.step + fs.off)) * 3 : 0);
          if (fs.step > 1) {  // a decimated pixel is never the last one of its row: one unaligned dword instead of 3 bytes
            const unsigned v = LDG(u32_unaligned, p, a.x_img);
#pragma unroll
            for (int c = 0; c < 3; ++c) raw[j][c] = (v >> (8 * c)) & 0xffu;
          } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) raw[j][c] = LDG(uint8_t, p + c, a.x_img);
          }
        } else {
          const uint8_t* p0 = f + (img ? ((size_t)(2 * y) * fs.src_w + 2 * x) * 3 : 0);
          const uint8_t* p1 = p0 + (img ? (size_t)fs.src_w * 3 : 0);
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            raw[j][c] = LDG(uint8_t, p0 + c, a.x_img);
            raw[j][6 + c] = LDG(uint8_t, p1 + c, a.x_img);
          }
        }
      }
    }
  };
  auto unit_of = [&](int j) -> u32x4 {
    if (SRC == 0) {
      return ((s_in >> j) & 1) ? stage[j] : u32x4{0, 0, 0, 0};
    } else {
      int v[3] = {114, 114, 114};
      if ((s_img >> j) & 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          v[c] = SRC == 1 ? (int)raw[j][c] : (int)((raw[j][c] + raw[j][c + 3] + raw[j][6 + c] + raw[j][9 + c] + 2) >> 2);
      }
      // BGR -> RGB, /255, fp16 RNE: K3's values
      constexpr float k255 = 1.0f / 255.0f;  // == division after the fp16 rounding, see SRC 3 below
      f16x4 lo = f16x4{(_Float16)((float)v[2] * k255), (_Float16)((float)v[1] * k255), (_Float16)((float)v[0] * k255),
                       (_Float16)0.f};
      u32x2 l2 = __builtin_bit_cast(u32x2, lo);
      u32x4 u = u32x4{l2[0], l2[1], 0, 0};
      return ((s_in >> j) & 1) ? u : u32x4{0, 0, 0, 0};
    }
  };

  // B-fragment positions: lane group q = lane>>4 reads the pixel of tap 4j+q (taps >= 9: weights are zero)
  int bpos[3][2];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      int tap = 4 * j + (lane >> 4);
      if (tap > 8) tap = 8;
      const int py = (wave * 2 + m) * S + tap / KS;
      const int px = (lane & 15) * S + tap % KS;
      const int col = EIOKU_PATCH_COL(px, PWH, S);
      bpos[j][m] = py * PWS + col;
    }
  const uint4* wt_lane = wt + (lane & 15) * 4 + ((lane >> 4) ^ ((lane >> 1) & 3));
  float4 biasr[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f)
    biasr[f] = *reinterpret_cast<const float4*>(a.bias + co_tile * ROWS + f * 16 + (lane >> 4) * 4);

  int tile = blockIdx.x;
  if (tile < total_tiles) issue(tile);
  int buf = 0;
  for (; tile < total_tiles; tile += gridDim.x) {
    uint4* pb = patch + buf * PATCH_U;
    if (SRC == 3) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // pixel i of the group = bytes 3i..3i+2 (B, G, R) of the 12 loaded ones
        // fp16(v * (1/255)) == fp16(v / 255) for all 256 byte values (tests/test_oracle_yolo.py checks the
        // identity exhaustively), so the fused path spares the 12 IEEE divisions per group
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int byte = 3 * i + c;
          v[c] = s_img ? (float)((graw[byte >> 2] >> (8 * (byte & 3))) & 0xffu) : 114.0f;
        }
        constexpr float k255 = 1.0f / 255.0f;
        f16x4 lo = f16x4{(_Float16)(v[2] * k255), (_Float16)(v[1] * k255), (_Float16)(v[0] * k255), (_Float16)0.f};
        const u32x2 l2 = __builtin_bit_cast(u32x2, lo);
        *reinterpret_cast<u32x4*>(pb + g_off[i]) = s_in ? u32x4{l2[0], l2[1], 0, 0} : u32x4{0, 0, 0, 0};
      }
    } else {
#pragma unroll
      for (int j = 0; j < R; ++j) *reinterpret_cast<u32x4*>(pb + s_off[j]) = unit_of(j);
    }
    __syncthreads();  // double-buffered patch: one barrier per tile (also orders the weight copy before tile 0)
    const int tn = nx_n, tth = nx_th, ttw = nx_tw;
    const int next = tile + gridDim.x;
    if (next < total_tiles) issue(next);
    __builtin_amdgcn_sched_barrier(0);

    float4v acc[2][NF];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[m][f] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      half8 bf[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        uint4 u = pb[bpos[j][m]];
        bf[m] = *reinterpret_cast<half8*>(&u);
      }
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        uint4 w = wt_lane[(j * NF + f) * 64];
        const half8 af = *reinterpret_cast<half8*>(&w);
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[m][f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[m], acc[m][f], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    const int ow = ttw * kTW + (lane & 15);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int oh = tth * kTH + wave * 2 + m;
      if (oh >= a.Ho || ow >= a.Wo) continue;
      const unsigned opix = (unsigned)((tn * a.Ho + oh) * a.Wo + ow);
#pragma unroll
      for (int f = 0; f < NF; ++f) store_frag(a, acc[m][f], opix, co_tile * ROWS + f * 16 + (lane >> 4) * 4, biasr[f]);
    }
    buf ^= 1;
  }
}

// ---------------------------------------------------------------------------------------------
// YOLOv8n front end as ONE launch: letterbox (copy mode) -> stem 3x3/s2 (3 -> 16) -> model.1 3x3/s2 (16 -> 32) ->
// model.2.cv1 1x1 (32 -> 32).  Neither the fp16 network input nor the 320^2 x 16 stem output (105 MB per 64 frames,
// written once and read 1.3x) ever exists in memory.  Per 8x16 tile of model.1's output the workgroup stages the
// 35x67 image patch from the BGR bytes (8-byte RGB0 pixels, columns de-interleaved by parity for the stride-2
// reads), runs the stem on the 17x33 pixels model.1 needs (36 fragments of 16 flattened patch pixels, 4-tap K
// packing and weights in registers exactly as k_conv3x3_c8), writes act(stem) as fp16 into the LDS patch P1 (32 B
// per pixel, zeros outside the map), runs model.1 out of P1 with the generic tap loop and hands its tile to the 1x1
// as the POST path of k_conv3x3_persist does.  Every MFMA sees the operands of the separate launches in the same
// k order, every intermediate is rounded to fp16 where they round it: the result is bit-identical.
// model.1's K chunk is 16 real channels + 16 whose weights are zero: lanes of K groups 2, 3 re-read units 0, 1 of
// P1 (finite values x 0) instead of a zero half that would double the patch.
// ---------------------------------------------------------------------------------------------
struct StemArgs {
  const uint4* wgt;   // stem weights, packed [9 taps][16 rows][4 units]
  const float* bias;
  int act;
  int H0, W0;         // network input (letterboxed) size
};

// DECIM: the image region is a strided sampling of the source (FusedInput::step / off: 1080p -> 360 x 640 is step 3,
// off 1): the 4 pixels of a group are 4 unaligned dword loads (3 bytes each + one ignored) instead of one dwordx3
// MODE 2: exact-1/2 sources (720p -> 360 x 640): cv2.resize swaps INTER_LINEAR for the 2x2 area average there; a group's
// four pixels are 8 source pixels on each of two rows = 2 x 6 unaligned dwords, averaged (a + b + c + d + 2) >> 2 as K3
// does.
template <int MODE>
__global__ __launch_bounds__(256) void k_conv_stem_chain(ConvArgs a, StemArgs st, FusedSrc fs, int total_tiles) {
  constexpr int GPR = 18;                 // 4-pixel groups per patch row: columns -1 .. 70
  constexpr int NG = kSX_H * GPR;         // 630
  constexpr int RG = (NG + 255) / 256;    // 3 groups per thread
  constexpr int NPA = kSP_H * kSP_W;      // 561 stem pixels per tile
  constexpr int KA = (NPA + 63) / 64;     // 9 fragments per wave

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* wt1 = reinterpret_cast<uint4*>(smem);
  uint4* wt2 = wt1 + kSC_WT1;
  uint4* tbuf = wt2 + kSC_WT2;
  uint4* p1 = tbuf + kSC_T;
  unsigned char* xs = reinterpret_cast<unsigned char*>(p1 + kSC_P1_U);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4;
  // staging groups
  int g_y[RG], g_x[RG], g_off[RG][4];
#pragma unroll
  for (int j = 0; j < RG; ++j) {
    const int g = tid + 256 * j;
    const int gy = g / GPR, gx = g - gy * GPR;
    g_y[j] = g < NG ? gy : -100000;  // an impossible row: the slot is then outside the network input
    g_x[j] = 4 * gx - 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pc = 4 * gx - 1 + i;
      g_off[j][i] = (g < NG && pc >= 0 && pc < 2 * kSX_WH - 1 ? gy * kSX_WS + (pc & 1) * kSX_WH + (pc >> 1) : kSX_PX) * 8;
    }
  }
  const int tiles_per_img = a.tiles_w * a.tiles_h;
  const float r_tpi = 1.0f / (float)tiles_per_img, r_tw = 1.0f / (float)a.tiles_w;
  constexpr bool DECIM = MODE == 1, HALF = MODE == 2;
  u32x4 graw[RG];     // copy: 12 packed bytes in [0..2]; DECIM: one pixel per dword
  unsigned gh[HALF ? RG : 1][12];  // HALF: 24 bytes of source row 2y, then 24 of row 2y + 1
  unsigned s_in = 0, s_img = 0;
  bool s_full = false;
  int nx_n = 0, nx_th = 0, nx_tw = 0;
  auto issue = [&](int tile) {
    tile = xcd_tile(tile, total_tiles);
    nx_n = fast_div(tile, tiles_per_img, r_tpi);
    const int t2 = tile - nx_n * tiles_per_img;
    nx_th = fast_div(t2, a.tiles_w, r_tw);
    nx_tw = t2 - nx_th * a.tiles_w;
    const int y0 = nx_th * (4 * kTH) - 3, x0 = nx_tw * (4 * kTW);
    s_in = 0;
    s_img = 0;
    // every staged group (rows y0 .. y0+34, columns x0-4 .. x0+67) inside the image?
    s_full = y0 >= fs.top && y0 + kSX_H <= fs.top + fs.new_h && x0 - 4 >= fs.left && x0 + 4 * GPR - 4 <= fs.left + fs.new_w;
#pragma unroll
    for (int j = 0; j < RG; ++j) {
      const int iy = y0 + g_y[j], ix = x0 + g_x[j];  // ix, W0, left and new_w are multiples of 4: a group is all in or all out
      const bool in = (unsigned)iy < (unsigned)st.H0 && (unsigned)ix < (unsigned)st.W0;
      const int y = iy - fs.top, x = ix - fs.left;
      const bool img = in && (unsigned)y < (unsigned)fs.new_h && (unsigned)x < (unsigned)fs.new_w;
      s_in |= (in ? 1u : 0u) << j;
      s_img |= (img ? 1u : 0u) << j;
      if (HALF) {
        const uint8_t* p = fs.bgr + (img ? ((size_t)(nx_n * fs.src_h + 2 * y) * fs.src_w + 2 * x) * 3 : 0);
        const size_t row = img ? (size_t)fs.src_w * 3 : 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          gh[j][i] = LDG(u32_unaligned, p + 4 * i, a.x_img);
          gh[j][6 + i] = LDG(u32_unaligned, p + row + 4 * i, a.x_img);
        }
      } else if (DECIM) {
        const uint8_t* p = fs.bgr + (img ? ((size_t)(nx_n * fs.src_h + y * fs.step + fs.off) * fs.src_w + x * fs.step + fs.off) * 3 : 0);
        const int ps = img ? fs.step * 3 : 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) graw[j][i] = LDG(u32_unaligned, p + i * ps, a.x_img);
      } else {
        const u32x3 g = LDG(u32x3, fs.bgr + (img ? ((size_t)(nx_n * fs.src_h + y) * fs.src_w + x) * 3 : 0), a.x_img);
        graw[j] = u32x4{g[0], g[1], g[2], 0};
      }
    }
  };

  // stem: A operands (weights) live in registers; B operand of k-step j, K group q = the pixel of tap 4j+q
  half8 wS[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int tap = 4 * j + q;
    u32x4 v = u32x4{0, 0, 0, 0};
    if (tap < 9) v = *reinterpret_cast<const u32x4*>(st.wgt + (tap * 16 + (lane & 15)) * 4);
    wS[j] = __builtin_bit_cast(half8, v);
  }
  int tapoff[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    int tap = 4 * j + q;
    if (tap > 8) tap = 8;
    const int kh = tap / 3, kw = tap - kh * 3;
    tapoff[j] = (kh * kSX_WS + (kw == 1 ? kSX_WH : (kw == 2 ? 1 : 0))) * 8;
  }
  int xbase[KA], pa_st[KA], pa_yx[KA];
#pragma unroll
  for (int k = 0; k < KA; ++k) {
    const int praw = (wave + 4 * k) * 16 + (lane & 15);
    const int p = praw < NPA ? praw : NPA - 1;
    const int py = p / kSP_W, px = p - py * kSP_W;
    xbase[k] = (2 * py * kSX_WS + px) * 8;
    pa_st[k] = (praw < NPA ? py * kSP_WS + (px & 1) * kSP_WH + (px >> 1) : kSP_SLOTS) * 32 + q * 8;
    pa_yx[k] = (py << 8) | px;
  }
  const float4 biasS = *reinterpret_cast<const float4*>(st.bias + q * 4);
  // model.1 out of P1
  int bpos1[9][2];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int kh = tap / 3, kw = tap % 3;
      const int ox = lane & 15;
      const int slot = (2 * (wave * 2 + m) + kh) * kSP_WS + (kw == 1 ? kSP_WH + ox : (kw == 2 ? ox + 1 : ox));
      bpos1[tap][m] = slot * 2 + (q & 1);
    }
  const int wsel = (lane & 15) * 4 + (q ^ ((lane >> 1) & 3));
  const uint4* wt1_lane = wt1 + wsel;
  const uint4* wt2_lane = wt2 + wsel;
  float4 bias1[2], bias2[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    bias1[f] = *reinterpret_cast<const float4*>(a.bias + f * 16 + q * 4);
    bias2[f] = *reinterpret_cast<const float4*>(a.post_bias + f * 16 + q * 4);
  }

  int tile = blockIdx.x;
  if (tile < total_tiles) issue(tile);
  {
    constexpr int NW = kSC_WT1 + kSC_WT2, WB = 6;
    for (int i0 = 0; i0 < NW; i0 += 256 * WB) {
      u32x4 w[WB];
#pragma unroll
      for (int j = 0; j < WB; ++j) {
        const int idx = i0 + j * 256 + tid;
        const int k = idx < NW ? idx : 0;
        w[j] = *reinterpret_cast<const u32x4*>(k < kSC_WT1 ? a.wgt + k : a.post_w + (k - kSC_WT1));
      }
#pragma unroll
      for (int j = 0; j < WB; ++j) {
        const int idx = i0 + j * 256 + tid;
        const int row = ((idx < kSC_WT1 ? idx : idx - kSC_WT1) >> 2) & 31, unit = idx & 3;
        if (idx < NW) *reinterpret_cast<u32x4*>(wt1 + (idx & ~3) + (unit ^ ((row >> 1) & 3))) = w[j];
      }
    }
  }
  for (; tile < total_tiles; tile += gridDim.x) {
    // image patch -> LDS: BGR -> RGB, /255 as a multiply (same fp16, see k_conv3x3_c8), 114 grey outside the image,
    // zero outside the network input (the stem's padding)
    // (a patch wholly inside the image -- tile-uniform -- needs none of the per-pixel selects: the kernel is
    // VALU-bound, see silu4)
    auto commit = [&](auto full_tag) {
      constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
      for (int j = 0; j < RG; ++j) {
        const bool in = (s_in >> j) & 1, img = (s_img >> j) & 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float v[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float fb;
            if (HALF) {
              auto bt = [&](int r, int b) { return (gh[j][6 * r + (b >> 2)] >> (8 * (b & 3))) & 0xffu; };
              fb = (float)((bt(0, 6 * i + c) + bt(0, 6 * i + 3 + c) + bt(1, 6 * i + c) + bt(1, 6 * i + 3 + c) + 2u) >> 2);
            } else {
              const int byte = DECIM ? 4 * i + c : 3 * i + c;
              fb = (float)((graw[j][byte >> 2] >> (8 * (byte & 3))) & 0xffu);
            }
            v[c] = (FULL || img) ? fb : 114.0f;
          }
          constexpr float k255 = 1.0f / 255.0f;
          f16x4 lo = f16x4{(_Float16)(v[2] * k255), (_Float16)(v[1] * k255), (_Float16)(v[0] * k255), (_Float16)0.f};
          const u32x2 l2 = __builtin_bit_cast(u32x2, lo);
          *reinterpret_cast<u32x2*>(xs + g_off[j][i]) = (FULL || in) ? l2 : u32x2{0, 0};
        }
      }
    };
    if (s_full) commit(std::true_type{});
    else commit(std::false_type{});
    __syncthreads();  // also orders the weight copy before the first tile
    const int tn = nx_n, tth = nx_th, ttw = nx_tw;
    const int next = tile + gridDim.x;
    if (next < total_tiles) issue(next);
    __builtin_amdgcn_sched_barrier(0);

    // stem on the 17x33 patch -> P1
    const int r0 = tth * (2 * kTH) - 1, c0 = ttw * (2 * kTW) - 1;
    const bool p1_inside = r0 >= 0 && r0 + kSP_H <= a.H && c0 >= 0 && c0 + kSP_W <= a.W;
#pragma unroll
    for (int k0 = 0; k0 < KA; k0 += 3) {
      float4v acc[3];
      half8 bf[3][3];
#pragma unroll
      for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const u32x2 lo = *reinterpret_cast<const u32x2*>(xs + xbase[k0 + m] + tapoff[j]);
          bf[m][j] = __builtin_bit_cast(half8, u32x4{lo[0], lo[1], 0, 0});
        }
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        acc[m] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wS[j], bf[m][j], acc[m], 0, 0, 0);
      }
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const int k = k0 + m;
        float4v v = acc[m] + float4v{biasS.x, biasS.y, biasS.z, biasS.w};
        if (st.act == kActSiLU) {
          v = silu4(v);
        }
        const f16x4 h = __builtin_convertvector(v, f16x4);
        u32x2 hv = __builtin_bit_cast(u32x2, h);
        if (!p1_inside) {  // tile-uniform: only border tiles pay for the per-pixel map test
          const int ah = r0 + (pa_yx[k] >> 8), aw = c0 + (pa_yx[k] & 255);
          const bool inmap = (unsigned)ah < (unsigned)a.H && (unsigned)aw < (unsigned)a.W;
          hv = inmap ? hv : u32x2{0, 0};
        }
        *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(p1) + pa_st[k]) = hv;
      }
    }
    __syncthreads();

    // model.1 (3x3 / s2) out of P1, then the 1x1 on the tile still on chip
    float4v acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int f = 0; f < 2; ++f) acc[m][f] = float4v{0.f, 0.f, 0.f, 0.f};
    mma_taps<2, 2>(p1, wt1_lane, bpos1, acc);
    __builtin_amdgcn_sched_barrier(0);
    uint4* tw = tbuf + wave * 32 * 4;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const float4v v = activate_frag(a, acc[m][f], bias1[f]);
        const f16x4 h = __builtin_convertvector(v, f16x4);
        const int px = m * 16 + (lane & 15);
        const int unit = f * 2 + (lane >> 5), half = q & 1;
        *reinterpret_cast<u32x2*>(reinterpret_cast<char*>(tw + px * 4 + (unit ^ ((px >> 1) & 3))) + half * 8) = __builtin_bit_cast(u32x2, h);
      }
    __builtin_amdgcn_wave_barrier();
    float4v acc2[2][2];
    {
      half8 bf[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int px = m * 16 + (lane & 15);
        uint4 u = tw[px * 4 + (q ^ ((px >> 1) & 3))];
        bf[m] = *reinterpret_cast<half8*>(&u);
      }
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        uint4 w = wt2_lane[f * 64];
        const half8 af = *reinterpret_cast<half8*>(&w);
#pragma unroll
        for (int m = 0; m < 2; ++m)
          acc2[m][f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[m], float4v{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      }
    }
    __builtin_amdgcn_wave_barrier();
    const int ow = ttw * kTW + (lane & 15);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int oh = tth * kTH + wave * 2 + m;
      if (oh >= a.Ho || ow >= a.Wo) continue;
      const unsigned opix = (unsigned)((tn * a.Ho + oh) * a.Wo + ow);
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        float4v v = acc2[m][f] + float4v{bias2[f].x, bias2[f].y, bias2[f].z, bias2[f].w};
        if (a.post_act == kActSiLU) {
          v = silu4(v);
        }
        const f16x4 h = __builtin_convertvector(v, f16x4);
        STG(u32x2, a.post_out + (size_t)(opix * (unsigned)a.post_out_cs + (unsigned)(f * 16 + q * 4)), __builtin_bit_cast(u32x2, h), a.x_out);
      }
    }
  }
}

// ---- launching: layouts and routes come from conv_plan.h, everything that touches the device is here ----------------
// Workgroups of `Kernel` that can be RESIDENT on one CU, registers included: a persistent grid sized from LDS alone
// runs its surplus workgroups as a second, half-empty round (k_conv3x3_chain<1,...,1,2>: 174 VGPRs = two waves per
// SIMD = two workgroups per CU, launched three per CU because three fit its LDS).  Asked once per kernel.
template <auto Kernel>
int resident_per_cu(int threads, size_t lds) {
  static const int occ = [&] {
    int n = 0;
    const bool ok = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, Kernel, threads, lds) == hipSuccess && n >= 1;
    if (!ok) (void)hipGetLastError();
    return ok ? n : 1;
  }();
  return occ;
}
// Workgroups per CU of a persistent grid: as many `lds`-byte ones as fit `budget` bytes of the CU's LDS, at least one,
// at most `limit` and, where the caller asked the occupancy (`occ` > 0), no more than are resident.
int wg_per_cu(size_t budget, size_t lds, int limit, int occ = 0) {
  const int n = std::max(1, std::min((int)(budget / lds), limit));
  return occ > 0 ? std::min(n, occ) : n;
}
// x extent of that grid: `per_cu` workgroups on every CU, shared among the `ntiles` cout tiles (grid y), never more than
// there are tiles to walk
unsigned persistent_grid(int per_cu, int ntiles, long long total) {
  const long long bx = std::max(1ll, (long long)num_cus() * per_cu / ntiles);
  return (unsigned)std::min(bx, total);
}
// Every launch of the family: lift the kernel's dynamic-LDS ceiling where `lds` needs more than the default 64 KB (per
// kernel, the largest value set so far: an instantiation whose LDS varies at run time is raised again by a larger layer
// and never lowered by a smaller one; host threads meet in the atomic and, to raise, behind one mutex), count the route,
// launch, check.
std::mutex g_lds_attr_mutex;
template <auto Kernel, typename... A>
int launch_kernel(int route, dim3 grid, int threads, size_t lds, hipStream_t stream, const A&... args) {
  static std::atomic<size_t> raised{0};
  if (lds > 64 * 1024 && lds > raised.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lock(g_lds_attr_mutex);
    if (lds > raised.load(std::memory_order_relaxed)) {
      EIOKU_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds));
      raised.store(lds, std::memory_order_release);
    }
  }
  route_hit(route);
  hipLaunchKernelGGL(Kernel, grid, dim3((unsigned)threads), lds, stream, args...);
  EIOKU_LAUNCH_CHECK();
  return EIOKU_OK;
}

template <int NF, int S, int SRC>
int launch_c8(const ConvPlan& p, const ConvArgs& a, const FusedSrc& fs, int ntiles, hipStream_t stream) {
  const int total = a.tiles_w * a.tiles_h * a.N;
  // small LDS footprint: ~6 workgroups per CU keep the byte loads in flight
  const dim3 grid(persistent_grid(6, ntiles, total), (unsigned)ntiles);
  return launch_kernel<k_conv3x3_c8<NF, S, SRC>>(route_id(kRouteC8, NF, S, SRC), grid, p.threads, p.lds, stream, a, fs, total);
}

template <int NF, int S, int NCH, bool DB, bool POST, int NWV>
int launch_persist(const ConvPlan& p, ConvArgs a, int ntiles, hipStream_t stream) {
  constexpr auto K = k_conv3x3_persist<NF, S, NCH, DB, POST, NWV>;
  a.tiles_h = (a.Ho + 2 * NWV - 1) / (2 * NWV);
  const int total = a.tiles_w * a.tiles_h * a.N;
  // 160 KB of LDS per CU: two 78 KB workgroups do fit (measured on model.22.cv3.0.0, 68 -> 57 us)
  const int per_cu = wg_per_cu(160 * 1024, p.lds, 4, resident_per_cu<K>(p.threads, p.lds));
  const dim3 grid(persistent_grid(per_cu, ntiles, total), (unsigned)ntiles);
  return launch_kernel<K>(route_id(kRoutePersist, NF, S, NCH, DB, POST, NWV), grid, p.threads, p.lds, stream, a, total);
}

template <int NF, int CAT, int NF2>
int launch_chain(const ConvArgs& a, const ChainCat& cc, hipStream_t stream) {
  // (a second patch buffer was measured against an extra workgroup per CU: 77 vs 69 us at 160^2; single-buffered it is)
  constexpr auto K = k_conv3x3_chain<NF, false, CAT, NF2>;
  constexpr size_t lds = lds_bytes(chain_layout(NF, false, CAT, NF2).total);
  const int total = a.tiles_w * a.tiles_h * a.N;
  // two 80.3 KB workgroups (32-channel C2f + its closing 1x1) share a CU
  const int per_cu = wg_per_cu(160 * 1024, lds, 4, resident_per_cu<K>(256, lds));
  const dim3 grid(persistent_grid(per_cu, 1, total));  // one cout tile: the whole chip walks the pixel tiles
  return launch_kernel<K>(route_id(kRouteChain, NF, 0, CAT, NF2), grid, 256, lds, stream, a, cc, total);
}

template <int NF, int S, int MT, int NS>
int launch_flat(const ConvPlan& p, const ConvArgs& a, int ntiles, hipStream_t stream) {
  const int npix = a.N * a.Ho * a.Wo, tpx = 64 * MT;
  // the kernel's own test (epi_variant) for the first cout tile: this launch runs the straight-line epilogue somewhere
  if (a.epi && !a.out_f32 && (a.Cout & 3) == 0 && a.Cout >= 16 * NF && (a.act == kActSiLU || a.act == kActNone))
    g_epi_launches.fetch_add(1u, std::memory_order_relaxed);
  const dim3 grid((unsigned)((npix + tpx - 1) / tpx), (unsigned)ntiles);
  return launch_kernel<k_conv3x3_flat<NF, S, MT, NS>>(route_id(kRouteFlat, NF, S, MT, NS), grid, p.threads, p.lds, stream, a, npix,
                                                      p.pr, p.pw);
}

template <int NF, int S>
int launch_igemm(const ConvPlan& p, const ConvArgs& a, int ntiles, hipStream_t stream) {
  const dim3 grid((unsigned)(a.tiles_w * a.tiles_h * a.N), (unsigned)ntiles);
  return launch_kernel<k_conv_igemm<NF, 3, S>>(route_id(kRouteIgemm, NF, 3, S), grid, p.threads, p.lds, stream, a);
}

template <int NF, bool UP>
int launch_1x1(const ConvPlan& p, const ConvArgs& a, int ntiles, hipStream_t stream) {
  constexpr int NWV = 4;
  const long long npix = (long long)a.N * a.H * a.W, groups = (npix + 31) / 32;
  // one pixel group per wave at the most; grid-stride beyond wg_cu workgroups per CU
  const dim3 grid(persistent_grid(p.wg_cu, ntiles, std::max(1ll, (groups + NWV - 1) / NWV)), (unsigned)ntiles);
  return launch_kernel<k_conv1x1<NF, UP, NWV>>(route_id(kRoute1x1, NF, UP, NWV, a.clsmax != nullptr), grid, p.threads, p.lds, stream, a,
                                               npix);
}

// The one way a run-time integer becomes a template argument: f(std::integral_constant<int, V>) for the V of the list
// that equals v, and what f returns; false when none does.  Nested, the lists spell out the instantiated kernels.
template <int... Vs, typename F>
bool with_const(int v, F&& f) {
  return ((v == Vs && f(std::integral_constant<int, Vs>{})) || ...);
}
#define CV(x) decltype(x)::value  // the constant with_const handed to a lambda as x

// Launches the instantiation a plan names.  The lists are the set of instantiated kernels: a plan outside them is an
// error, never another kernel.
int launch_plan(const ConvPlan& p, const ConvArgs& a, const FusedSrc& fs, int ntiles, hipStream_t stream) {
  const int* t = p.t;
  int rc = EIOKU_OK;
  bool hit = false;
  auto s12 = [&](auto&& f) { return with_const<1, 2>(t[1], f); };
  if (p.family == kRouteC8) {
    hit = t[1] == 2 && with_const<1, 2, 3, 4, 5>(t[0], [&](auto nf) {
      return with_const<0, 1, 2, 3>(t[2], [&](auto src) { return rc = launch_c8<CV(nf), 2, CV(src)>(p, a, fs, ntiles, stream), true; });
    });
  } else if (p.family == kRoutePersist) {
    const int key = t[0] * 10 + t[2];  // NF, NCH
    auto s_db = [&](auto k, auto post) {
      return s12([&](auto s) {
        return with_const<0, 1>(t[3], [&](auto db) {
          return rc = launch_persist<CV(k) / 10, CV(s), CV(k) % 10, CV(db) != 0, CV(post) != 0, 4>(p, a, ntiles, stream), true;
        });
      });
    };
    if (t[5] == 8)
      hit = !t[3] && !t[4] && with_const<33, 52>(key, [&](auto k) {
        return s12([&](auto s) { return rc = launch_persist<CV(k) / 10, CV(s), CV(k) % 10, false, false, 8>(p, a, ntiles, stream), true; });
      });
    else if (t[5] == 4 && t[4])
      hit = with_const<21, 41, 22, 42>(key, [&](auto k) { return s_db(k, std::true_type{}); });
    else if (t[5] == 4)
      hit = with_const<11, 21, 31, 41, 51, 61, 12, 22, 32, 42, 52, 13, 23, 33, 43, 53>(key, [&](auto k) { return s_db(k, std::false_type{}); });
  } else if (p.family == kRouteFlat) {
    hit = with_const<2, 3, 4, 5, 6>(t[0], [&](auto nf) {
      return s12([&](auto s) {
        return with_const<1, 2>(t[2], [&](auto mt) {
          return with_const<4, 8>(t[3], [&](auto ns) { return rc = launch_flat<CV(nf), CV(s), CV(mt), CV(ns)>(p, a, ntiles, stream), true; });
        });
      });
    });
  } else if (p.family == kRouteIgemm) {
    hit = t[1] == 3 && with_const<1, 2, 3, 4, 5, 6, 8>(t[0], [&](auto nf) {
      return with_const<1, 2>(t[2], [&](auto s) { return rc = launch_igemm<CV(nf), CV(s)>(p, a, ntiles, stream), true; });
    });
  } else if (p.family == kRoute1x1) {
    hit = t[2] == 4 && with_const<1, 2, 3, 4, 5, 6, 8>(t[0], [&](auto nf) {
      return with_const<0, 1>(t[1], [&](auto up) { return rc = launch_1x1<CV(nf), CV(up) != 0>(p, a, ntiles, stream), true; });
    });
  }
  if (hit) return rc;
  char name[160] = "?";
  if (p.ok()) route_name(name, sizeof name, p.family, t);
  set_error("no kernel is instantiated for the planned route %s", name);
  return EIOKU_EINVAL;
}
#undef CV

}  // namespace

// the shape half of conv_weights_create: what the plan needs of a layer's weights, no device
static int conv_tiling(ConvWeights* cw, int cout, int cin, int ks, int stride) {
  EIOKU_REQUIRE(cout > 0 && cin > 0, "bad conv shape cout=%d cin=%d", cout, cin);
  EIOKU_REQUIRE(ks == 1 || ks == 3, "kernel size %d not supported (1 or 3)", ks);
  EIOKU_REQUIRE((stride == 1) || (stride == 2 && ks == 3), "stride %d with k=%d not supported", stride, ks);
  EIOKU_REQUIRE(cin % 8 == 0, "cin %d must be a multiple of 8 (NHWC 16-byte units)", cin);
  cw->cout = cout;
  cw->cin = cin;
  cw->ks = ks;
  cw->stride = stride;
  cw->nchunks = (cin + 31) / 32;
  cw->nf = pick_nf(cout, ks, cw->nchunks, stride);
  cw->ntiles = (cout + 16 * cw->nf - 1) / (16 * cw->nf);
  return EIOKU_OK;
}

int conv_weights_create(ConvWeights* cw, int cout, int cin, int ks, int stride, const float* w,
                        const float* b) {
  EIOKU_TRY(conv_tiling(cw, cout, cin, ks, stride));
  const int tile = 16 * cw->nf;
  const int taps = ks * ks;
  const size_t wn = (size_t)cw->ntiles * cw->nchunks * taps * tile * 32;
  std::vector<_Float16> pw(wn, (_Float16)0.f);
  for (int co = 0; co < cout; ++co) {
    const int t = co / tile, cit = co % tile;
    for (int ci = 0; ci < cin; ++ci) {
      const int cc = ci / 32, cic = ci % 32;
      for (int tap = 0; tap < taps; ++tap) {
        const float v = w[((size_t)co * cin + ci) * taps + tap];  // [cout][cin][kh][kw]
        pw[((((size_t)t * cw->nchunks + cc) * taps + tap) * tile + cit) * 32 + cic] = (_Float16)v;
      }
    }
  }
  std::vector<float> pb((size_t)cw->ntiles * tile, 0.f);
  if (b)
    for (int co = 0; co < cout; ++co) pb[co] = b[co];
  EIOKU_TRY(cw->d_w.upload(reinterpret_cast<const __half*>(pw.data()), wn));
  return cw->d_b.upload(pb.data(), pb.size());
}

int conv_weights_create_cin8(ConvWeights* cw, int cout, int cin, int ks, int stride, const float* w, const float* b) {
  EIOKU_REQUIRE(cin > 0 && cin <= 8, "bad conv shape cout=%d cin=%d", cout, cin);
  const int taps = ks * ks;
  std::vector<float> w8((size_t)cout * 8 * taps, 0.f);
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int t = 0; t < taps; ++t) w8[((size_t)co * 8 + ci) * taps + t] = w[((size_t)co * cin + ci) * taps + t];
  return conv_weights_create(cw, cout, 8, ks, stride, w8.data(), b);
}

int conv_weights_create_centre(ConvWeights* cw, int cout, int cin, int stride, const float* w, const float* b) {
  std::vector<float> w3((size_t)cout * cin * 9, 0.f);
  for (size_t i = 0; i < (size_t)cout * cin; ++i) w3[i * 9 + 4] = w[i];
  return conv_weights_create(cw, cout, cin, 3, stride, w3.data(), b);
}

// EIOKU_CONV_EPI=0: k_conv3x3_flat runs store_frag's generic epilogue everywhere (byte-identity tests,
// tools/ab_bench.sh)
static bool conv_epi_on() {
  static const bool off = env_off("EIOKU_CONV_EPI");
  return !off;
}

bool conv_clsmax_ok(const ConvWeights& cw, int act) {
  static const bool off = env_off("EIOKU_CLSMAX");
  return !off && cw.ks == 1 && cw.ntiles == 1 && act == kActNone;
}

bool conv_post_ok(const ConvWeights& cw, const ConvWeights& post) {
  static const bool off = env_off("EIOKU_CONV_POST");
  if (off) return false;
  const bool shape = cw.ks == 3 && cw.cin != 8 && cw.nchunks <= 2 && cw.ntiles == 1 && cw.cout == 16 * cw.nf &&
                     (cw.nf == 2 || cw.nf == 4) && post.ks == 1 && post.cin == cw.cout && post.ntiles == 1 &&
                     post.nf == cw.nf && post.cout == 16 * post.nf;
  return shape && lds_bytes(persist_layout(cw.nf, cw.stride, cw.nchunks, false, true).total) <= 150 * 1024;
}

// The 64-channel pairs run as two launches: a one-launch kernel with the weights in registers (r3) was measured slower
// and removed ("Round-3 findings" (c)).
bool conv_chain_ok(const ConvWeights& a, const ConvWeights& b) {
  static const bool off = env_off("EIOKU_CONV_CHAIN");
  if (off) return false;
  auto one = [](const ConvWeights& c) {
    return c.ks == 3 && c.stride == 1 && c.nchunks == 1 && c.ntiles == 1 && (c.nf == 1 || c.nf == 2) && c.cout == 16 * c.nf &&
           c.cin == c.cout;
  };
  return one(a) && one(b) && a.nf == b.nf;
}

// concat = CAT whole 32-channel chunks from memory + this pair's 16*nf output channels; instantiated for YOLOv8n's
// three shallow C2fs: (16 ch, 1 chunk, 32 couts), (32 ch, 2 or 3 chunks, 64 couts)
int chain_cat_chunks(const ConvWeights& a, const ConvWeights& c2) {
  const int c = 16 * a.nf, lead = c2.cin - c;
  if (c2.ks != 1 || c2.ntiles != 1 || c2.cout != 16 * c2.nf || lead <= 0 || lead % 32 != 0) return 0;
  const int cat = lead / 32;
  if (a.nf == 1 && cat == 1 && c2.nf == 2) return 1;
  if (a.nf == 2 && (cat == 2 || cat == 3) && c2.nf == 4) return cat;
  return 0;
}

bool conv_chain_cat_ok(const ConvWeights& a, const ConvWeights& b, const ConvWeights& c2) {
  static const bool off = env_off("EIOKU_CHAIN_CAT");
  return !off && conv_chain_ok(a, b) && chain_cat_chunks(a, c2) > 0;
}

namespace {
// extents of the tensors one launch touches, from the slice geometry (a slice's buffer holds pixels x cstride elements);
// only the bounds-check build reads them
BcExt ext_of(const void* p, size_t bytes) {
  BcExt e;
  e.lo = reinterpret_cast<const char*>(p);
  e.hi = e.lo + (p ? bytes : 0);
  return e;
}
void set_extents(ConvArgs& a, Slice in, Slice res, Slice out, const float* out_f32, const unsigned long long* clsmax,
                 const UpSource* up, const FusedInput* fused) {
  const size_t pin = (size_t)a.N * a.H * a.W, pout = (size_t)a.N * a.Ho * a.Wo;
  a.x_in = ext_of(in.ptr, pin * in.cstride * 2);
  a.x_res = ext_of(res.ptr, pout * res.cstride * 2);
  a.x_out = out_f32 ? ext_of(out_f32, pout * a.Cout * 4) : ext_of(out.ptr, pout * out.cstride * 2);
  a.x_cls = ext_of(clsmax, pout * 8);
  a.x_in2 = up ? ext_of(up->src.ptr, (size_t)a.N * (a.H / 2) * (a.W / 2) * up->src.cstride * 2) : BcExt{};
  a.x_img = fused ? ext_of(fused->bgr, (size_t)a.N * fused->src_h * fused->src_w * 3) : BcExt{};
}
// What every launch of the family is told: layer `cw` on N x H x W input pixels read from `in` and, where a second layer
// `post` runs in the same launch, that layer and its output slice.  Everything else is zero until a caller sets it.
ConvArgs conv_args(const ConvWeights& cw, Slice in, int N, int H, int W, int act, const ConvWeights* post, Slice post_out,
                   int post_act) {
  ConvArgs a{};
  a.in = in.ptr ? in.ptr + in.coff : nullptr;
  a.in_cs = in.cstride;
  a.wgt = reinterpret_cast<const uint4*>(cw.d_w.p);
  a.bias = cw.d_b;
  a.N = N;
  a.H = H;
  a.W = W;
  a.Cin = cw.cin;
  a.Ho = conv_out_dim(H, cw.ks, cw.stride);
  a.Wo = conv_out_dim(W, cw.ks, cw.stride);
  a.Cout = cw.cout;
  a.tiles_w = (a.Wo + kTW - 1) / kTW;
  a.tiles_h = (a.Ho + kTH - 1) / kTH;
  a.nchunks = cw.nchunks;
  a.act = act;
  a.post_w = post ? reinterpret_cast<const uint4*>(post->d_w.p) : nullptr;
  a.post_bias = post ? post->d_b.p : nullptr;
  a.post_out = post && post_out.ptr ? post_out.ptr + post_out.coff : nullptr;
  a.post_out_cs = post_out.cstride;
  a.post_cout = post ? post->cout : 0;
  a.post_act = post_act;
  return a;
}
}  // namespace

int conv_chain_forward(const ConvWeights& ca, const ConvWeights& cb, Slice in, int N, int H, int W, Slice out,
                       bool residual, int act_a, int act_b, hipStream_t stream, const ConvWeights* cat_w, Slice cat_in,
                       Slice cat_out, int cat_act) {
  EIOKU_REQUIRE(ca.d_w && cb.d_w && conv_chain_ok(ca, cb), "this pair of 3x3 layers cannot run as one launch");
  EIOKU_REQUIRE(in.ptr && in.cstride % 8 == 0 && in.coff % 8 == 0, "bad input slice");
  EIOKU_REQUIRE(cat_w || (out.ptr && out.cstride % 4 == 0 && out.coff % 4 == 0), "bad output slice");
  EIOKU_REQUIRE(!cat_w || (cat_w->d_w && conv_chain_cat_ok(ca, cb, *cat_w) && cat_in.ptr && cat_in.cstride % 8 == 0 &&
                           cat_in.coff % 8 == 0 && cat_out.ptr && cat_out.cstride % 4 == 0 && cat_out.coff % 4 == 0),
                "the closing 1x1 cannot join this launch");
  if (N == 0) return EIOKU_OK;
  EIOKU_REQUIRE((long long)N * H * W * in.cstride < (1ll << 31) &&
                    (long long)N * H * W * (out.cstride > cat_out.cstride ? out.cstride : cat_out.cstride) < (1ll << 31) &&
                    (long long)N * H * W * cat_in.cstride < (1ll << 31),
                "tensor exceeds 32-bit element offsets -- split the batch");
  ConvArgs a = conv_args(ca, in, N, H, W, act_a, &cb, out, act_b);
  a.res = residual ? a.in : nullptr;  // the Bottleneck's shortcut is its own input: read from the staged patch
  a.res_cs = in.cstride;
  ChainCat cc{};
  if (cat_w) {
    cc.w = reinterpret_cast<const uint4*>(cat_w->d_w.p);
    cc.bias = cat_w->d_b;
    cc.out = cat_out.ptr + cat_out.coff;
    cc.out_cs = cat_out.cstride;
    cc.act = cat_act;
    cc.cat = cat_in.ptr + cat_in.coff;
    cc.cat_cs = cat_in.cstride;
    cc.x_cat = ext_of(cat_in.ptr, (size_t)N * H * W * cat_in.cstride * 2);
    cc.x_out = ext_of(cat_out.ptr, (size_t)N * H * W * cat_out.cstride * 2);
  }
  a.x_in = a.x_res = ext_of(in.ptr, (size_t)N * H * W * in.cstride * 2);
  a.x_out = ext_of(out.ptr, (size_t)N * H * W * out.cstride * 2);
  prof_start(EIOKU_PROF_CONV, stream);
  // NF, CAT and the closing 1x1's NF of the five instantiations (chain_cat_chunks admits no other)
  const int cat = cat_w ? chain_cat_chunks(ca, *cat_w) : 0;
  int rc = EIOKU_OK;
  with_const<112, 224, 234, 102, 202>(ca.nf * 100 + cat * 10 + (cat ? cat_w->nf : 2), [&](auto k) {
    constexpr int K = decltype(k)::value;
    return rc = launch_chain<K / 100, K / 10 % 10, K % 10>(a, cc, stream), true;
  });
  prof_stop(EIOKU_PROF_CONV, stream);
  return rc;
}

bool conv_stem_chain_ok(const ConvWeights& stem, const ConvWeights& c1, const ConvWeights& post, const FusedInput& f,
                        int W) {
  static const bool off = env_off("EIOKU_STEM_CHAIN");
  if (off) return false;
  const bool shapes = stem.ks == 3 && stem.stride == 2 && stem.cin == 8 && stem.cout == 16 && stem.nf == 1 && stem.ntiles == 1 &&
                      c1.ks == 3 && c1.stride == 2 && c1.cin == 16 && c1.cout == 32 && c1.nf == 2 && c1.ntiles == 1 &&
                      c1.nchunks == 1 && post.ks == 1 && post.cin == 32 && post.cout == 32 && post.nf == 2 && post.ntiles == 1;
  // copy-mode letterbox whose rows and padding are 4-pixel aligned (12-byte group loads)
  // (a decimating copy loads pixel by pixel: no alignment of the source, but the groups still must not straddle the
  // image edge)
  const bool src = f.bgr != nullptr && (f.mode == 0 || f.mode == 2) && f.left % 4 == 0 && f.new_w % 4 == 0 && W % 4 == 0 &&
                   (f.mode == 2 || f.step > 1 || (f.src_w % 4 == 0 && ((uintptr_t)f.bgr & 3) == 0));
  return shapes && src;
}

int conv_stem_chain_forward(const ConvWeights& stem, const ConvWeights& c1, const ConvWeights& post, const FusedInput& f,
                            int N, int H, int W, Slice out, int act0, int act1, int act2, hipStream_t stream) {
  EIOKU_REQUIRE(stem.d_w && c1.d_w && post.d_w && conv_stem_chain_ok(stem, c1, post, f, W), "layers cannot run as the fused front end");
  EIOKU_REQUIRE(out.ptr && out.cstride % 4 == 0 && out.coff % 4 == 0, "bad output slice");
  if (N == 0) return EIOKU_OK;
  EIOKU_REQUIRE((long long)N * (H / 4) * (W / 4) * out.cstride < (1ll << 31), "tensor exceeds 32-bit element offsets -- split the batch");
  // model.1's input = the stem's output map
  ConvArgs a = conv_args(c1, Slice{}, N, conv_out_dim(H, 3, 2), conv_out_dim(W, 3, 2), act1, &post, out, act2);
  a.x_out = ext_of(out.ptr, (size_t)N * a.Ho * a.Wo * out.cstride * 2);
  a.x_img = ext_of(f.bgr, (size_t)N * f.src_h * f.src_w * 3);
  StemArgs st{reinterpret_cast<const uint4*>(stem.d_w.p), stem.d_b, act0, H, W};
  FusedSrc fs{f.bgr, f.src_h, f.src_w, f.new_h, f.new_w, f.top, f.left, f.step, f.off};
  const int total = a.tiles_w * a.tiles_h * N;
  // as many workgroups as fit 150 KB of a CU's LDS, no occupancy clamp
  const dim3 grid(persistent_grid(wg_per_cu(150 * 1024, kStemChainLds, 1 << 30), 1, total));
  prof_start(EIOKU_PROF_CONV, stream);
  int rc = EIOKU_OK;
  with_const<0, 1, 2>(f.mode == 2 ? 2 : (f.step > 1 ? 1 : 0), [&](auto mode) {
    constexpr int MODE = decltype(mode)::value;
    return rc = launch_kernel<k_conv_stem_chain<MODE>>(route_id(kRouteStemChain, MODE), grid, 256, kStemChainLds, stream, a, st, fs, total), true;
  });
  prof_stop(EIOKU_PROF_CONV, stream);
  return rc;
}

bool fused_input_ok(const ConvWeights& cw, const FusedInput& f, Slice res, const float* out_f32) {
  return cw.ks == 3 && cw.cin == 8 && cw.stride == 2 && cw.nf <= 5 && !res.ptr && !out_f32 && (f.mode == 0 || f.mode == 2) &&
         f.bgr != nullptr;
}

// element offsets are 32-bit in every kernel: input, output and residual tensors of pixels x channel stride elements
static int conv_fits_32bit(const ConvWeights& cw, int N, int H, int W, int in_cs, int out_cs, int res_cs) {
  const long long px_in = (long long)N * H * W, px_out = (long long)N * conv_out_dim(H, cw.ks, cw.stride) * conv_out_dim(W, cw.ks, cw.stride);
  EIOKU_REQUIRE(px_in * (in_cs > 8 ? in_cs : 8) < (1ll << 31) && px_out * (out_cs > 1 ? out_cs : 1) < (1ll << 31) &&
                    px_out * (res_cs > 1 ? res_cs : 1) < (1ll << 31),
                "tensor of %lld pixels exceeds the kernels' 32-bit element offsets -- split the batch", px_in);
  return EIOKU_OK;
}

int conv_forward(const ConvWeights& cw, Slice in, int N, int H, int W, Slice out, float* out_f32,
                 Slice res, int act, hipStream_t stream, const FusedInput* fused, const ConvWeights* post, int post_act,
                 unsigned long long* clsmax, const UpSource* up) {
  EIOKU_REQUIRE(cw.d_w, "conv weights not created");
  EIOKU_REQUIRE(!up || (cw.ks == 1 && up->src.ptr && up->c_split % 32 == 0 && up->c_split <= cw.cin && H % 2 == 0 &&
                        W % 2 == 0 && (long long)N * H * W < (1ll << 24) && up->src.cstride % 8 == 0 && up->src.coff % 8 == 0),
                "this layer cannot read an upsampled operand in place");
  EIOKU_REQUIRE(!clsmax || conv_clsmax_ok(cw, act), "class-max output needs a 1x1 conv with one cout tile and no activation");
  EIOKU_REQUIRE(!post || (post->d_w && conv_post_ok(cw, *post) && !res.ptr && !out_f32 && !fused && out.ptr),
                "this pair of layers cannot run as one launch");
  EIOKU_REQUIRE((in.ptr || fused) && (out.ptr || out_f32 || clsmax), "NULL tensor");
  EIOKU_REQUIRE(!fused || fused_input_ok(cw, *fused, res, out_f32), "layer cannot read a fused letterbox input");
  EIOKU_REQUIRE(in.cstride % 8 == 0 && in.coff % 8 == 0, "input slice must be 8-channel aligned");
  // cout < 4 (the 1-class face head) only ever takes the scalar store path
  EIOKU_REQUIRE(out_f32 || cw.cout < 4 || (out.cstride % 4 == 0 && out.coff % 4 == 0),
                "output slice must be 4-channel aligned");
  EIOKU_REQUIRE(!res.ptr || cw.cout < 4 || (res.cstride % 4 == 0 && res.coff % 4 == 0),
                "residual slice must be 4-channel aligned");
  if (N == 0) return EIOKU_OK;
  EIOKU_TRY(conv_fits_32bit(cw, N, H, W, in.cstride, out_f32 ? cw.cout : out.cstride, res.cstride));
  // the letterbox a fused stem reads: its geometry and which of k_conv3x3_c8's staging loops (SRC) can read it
  FusedSrc fs{};
  int src = 0;
  if (fused) {
    fs = FusedSrc{fused->bgr, fused->src_h, fused->src_w, fused->new_h, fused->new_w, fused->top, fused->left,
                  fused->mode == 0 ? fused->step : 1, fused->mode == 0 ? fused->off : 0};
    src = fused->mode == 0 ? 1 : 2;
    // copy mode with 4-pixel aligned rows and padding: 12-byte group loads instead of byte loads
    if (src == 1 && fused->step == 1 && fused->src_w % 4 == 0 && fused->left % 4 == 0 && fused->new_w % 4 == 0 && W % 4 == 0 &&
        ((uintptr_t)fused->bgr & 3) == 0)
      src = 3;
  }
  const ConvPlan p = plan_conv(PlanLayer{cw.ks, cw.stride, cw.cin, cw.cout, cw.nf, cw.nchunks, N, H, W, in.cstride, res.ptr != nullptr,
                                         out_f32 != nullptr, post != nullptr, up != nullptr, clsmax != nullptr, fused != nullptr, src});
  EIOKU_REQUIRE(p.ok(), "%s", p.err);
  ConvArgs a = conv_args(cw, in, N, H, W, act, post, out, post_act);
  a.out = out.ptr ? out.ptr + out.coff : nullptr;  // with `post`: the 1x1's output slice (conv_args' post_out)
  a.out_f32 = out_f32;
  a.res = res.ptr ? res.ptr + res.coff : nullptr;
  a.out_cs = out.cstride;
  a.res_cs = res.cstride;
  a.epi = conv_epi_on() ? 1 : 0;
  a.clsmax = clsmax;
  a.in2 = up ? up->src.ptr + up->src.coff : nullptr;
  a.in2_cs = up ? up->src.cstride : 0;
  a.c_split = up ? up->c_split : 0;
  set_extents(a, in, res, out, out_f32, clsmax, up, fused);
  prof_start(EIOKU_PROF_CONV, stream);
  const int rc = launch_plan(p, a, fs, cw.ntiles, stream);
  prof_stop(EIOKU_PROF_CONV, stream);
  return rc;
}

}  // namespace eioku

// ---------------------------------------------------------------------------------------------
// C ABI: a single convolution (parity tests / building block for callers that own their graph)
// ---------------------------------------------------------------------------------------------
using namespace eioku;

extern "C" {

#ifdef EIOKU_BOUNDS_CHECK
namespace {
__global__ void k_bc_selftest(const unsigned* p, BcExt e, unsigned* sink) {
  // one element inside the extent, one straddling its end, one before its start
  unsigned v = LDG(unsigned, p, e);
  v += LDG(unsigned, reinterpret_cast<const char*>(p) + (e.hi - e.lo) - 2, e);
  v += LDG(unsigned, p - 1, e);
  STG(unsigned, sink, v, e);  // a store outside the extent: counted, not performed
}
}  // namespace
#endif

// Bounds-check instrumentation.  violations: accesses outside their tensor since the last reset
// (-1: this is not the bounds-check build); line: largest conv.hip source line of a violation.  selftest != 0 first
// runs a kernel that makes exactly 3 violations on purpose (the net catches what it should).
int eioku_debug_bounds(int* violations, int* line, int reset, int selftest) {
  EIOKU_REQUIRE(violations && line, "NULL output");
#ifdef EIOKU_BOUNDS_CHECK
  EIOKU_REQUIRE_INIT();
  if (selftest) {
    DevBuf<unsigned> buf;
    EIOKU_TRY(buf.grow(16));
    EIOKU_HIP_CHECK(hipMemset(buf, 0, 64));
    hipLaunchKernelGGL(k_bc_selftest, dim3(1), dim3(1), 0, 0, buf + 4, ext_of(buf + 4, 16), buf + 12);
    EIOKU_LAUNCH_CHECK();
    EIOKU_HIP_CHECK(hipDeviceSynchronize());
    unsigned sink = 1;
    EIOKU_HIP_CHECK(hipMemcpy(&sink, buf + 12, 4, hipMemcpyDeviceToHost));
    EIOKU_REQUIRE(sink == 0, "the bounds-check store went through (%u)", sink);
  }
  EIOKU_HIP_CHECK(hipDeviceSynchronize());
  int h[4] = {0, 0, 0, 0};
  EIOKU_HIP_CHECK(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_bc_flag), sizeof h));
  *violations = h[0];
  *line = h[1];
  if (reset) {
    const int z[4] = {0, 0, 0, 0};
    EIOKU_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_bc_flag), z, sizeof z));
  }
#else
  (void)reset;
  (void)selftest;
  *violations = -1;
  *line = 0;
#endif
  return EIOKU_OK;
}

// Route log: one line "family<FIELDvalue,...> count" per conv-family instantiation launched in this process since the
// last reset.  Host counters only: needs no device and no eioku_init.
int eioku_debug_conv_routes(char* buf, size_t cap, int reset) {
  EIOKU_REQUIRE(buf || cap == 0, "NULL buffer");
  size_t pos = 0;
  bool fits = true;
  for (int fam = 0; fam < kNumRouteFamilies; ++fam) {
    const RouteFamilyDesc& d = kRouteFamilies[fam];
    const int base = route_family_base(fam), slots = route_family_slots(fam);
    for (int i = 0; i < slots; ++i) {
      const unsigned c = reset ? g_route_counts[base + i].exchange(0u, std::memory_order_relaxed)
                               : g_route_counts[base + i].load(std::memory_order_relaxed);
      if (!c || !buf) continue;
      char line[160];
      int vals[6], rest = i;
      for (int f = d.nfields - 1; f >= 0; --f) {
        vals[f] = rest % d.radix[f];
        rest /= d.radix[f];
      }
      int n = route_name(line, sizeof line, fam, vals);
      n += snprintf(line + n, sizeof line - n, " %u\n", c);
      if (pos + (size_t)n + 1 > cap) {
        fits = false;
        continue;
      }
      memcpy(buf + pos, line, (size_t)n);
      pos += (size_t)n;
    }
  }
  if (cap) buf[pos] = 0;
  EIOKU_REQUIRE(fits, "route log does not fit %zu bytes", cap);
  return EIOKU_OK;
}

// Launches, since the last reset, of a kernel whose straight-line epilogue (EIOKU_CONV_EPI) was taken by at least its first
// cout tile: lets a test see that the comparison "switch on against switch off" compares two different loops.
int eioku_debug_conv_epi(int* launches, int reset) {
  EIOKU_REQUIRE(launches, "NULL argument");
  *launches = (int)(reset ? g_epi_launches.exchange(0u, std::memory_order_relaxed) : g_epi_launches.load(std::memory_order_relaxed));
  return EIOKU_OK;
}

// The plan of one layer as eioku_conv2d_f16 would run it on dense tensors: the route in the route log's format and the
// dynamic LDS bytes of the launch, or the error that call would end with.  Host arithmetic only: needs no device and no
// eioku_init.
int eioku_debug_conv_plan(int n, int h, int w, int cin, int cout, int ksize, int stride, int has_residual, int out_f32,
                          char* route, size_t cap, size_t* lds_bytes) {
  EIOKU_REQUIRE(route && cap > 0 && lds_bytes, "NULL output");
  EIOKU_REQUIRE(n > 0 && h > 0 && w > 0, "empty tensor n=%d h=%d w=%d", n, h, w);
  ConvWeights cw;
  EIOKU_TRY(conv_tiling(&cw, cout, cin, ksize, stride));
  EIOKU_TRY(conv_fits_32bit(cw, n, h, w, cin, cout, has_residual ? cout : 0));
  const ConvPlan p = plan_conv(PlanLayer{ksize, stride, cin, cout, cw.nf, cw.nchunks, n, h, w, cin, has_residual != 0, out_f32 != 0,
                                         false, false, false, false, 0});
  EIOKU_REQUIRE(p.ok(), "%s", p.err);
  char name[160];
  EIOKU_REQUIRE((size_t)route_name(name, sizeof name, p.family, p.t) < cap, "route name does not fit %zu bytes", cap);
  strcpy(route, name);
  *lds_bytes = p.lds;
  return EIOKU_OK;
}

int eioku_conv2d_f16(const void* in_nhwc, int n, int h, int w, int in_cstride, int in_coff, int cin,
                     const float* weight_oihw, const float* bias, int cout, int ksize, int stride,
                     int act_silu, const void* residual, int res_cstride, int res_coff, void* out_nhwc,
                     int out_cstride, int out_coff, float* out_f32, void* stream_) {
  EIOKU_REQUIRE_INIT();
  hipStream_t stream = (hipStream_t)stream_;
  ConvWeights cw;
  int rc = conv_weights_create(&cw, cout, cin, ksize, stride, weight_oihw, bias);
  if (rc) return rc;
  Slice in{(__half*)in_nhwc, in_cstride, in_coff};
  Slice out{(__half*)out_nhwc, out_cstride, out_coff};
  Slice res{(__half*)residual, res_cstride, res_coff};
  const int act = act_silu == 1 ? kActSiLU : act_silu == 2 ? kActReLU : act_silu == 3 ? kActResReLU : kActNone;
  rc = conv_forward(cw, in, n, h, w, out, out_f32, res, act, stream);
  if (rc == EIOKU_OK) {
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
      set_error("conv kernel failed: %s", hipGetErrorString(e));
      rc = EIOKU_EHIP;
    }
  }
  return rc;
}

}  // extern "C"
