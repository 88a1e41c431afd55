// Conv family, host side without HIP: the route table, the dynamic-LDS layout of every kernel family and the plan that
// decides which instantiation a layer runs on.  Plain C++17 (constexpr functions of ints: the kernels call them with
// template arguments, the host with run-time integers), so that all of it compiles and runs without a device.
#pragma once

#include <cstddef>
#include <cstdio>
#include <initializer_list>

namespace eioku {

inline int conv_out_dim(int x, int ks, int stride) { return (x + 2 * (ks / 2) - ks) / stride + 1; }

// Route log (eioku_debug_conv_routes): which conv-family instantiation a launch site started, counted where it is
// started.  One fixed table of relaxed atomic counters; a slot is (family, template arguments) in mixed radix, the
// names are formatted only when the log is read.  No device work, no allocation, safe from any number of host threads.
enum RouteFamily { kRouteIgemm = 0, kRouteFlat, kRoutePersist, kRouteChain, kRouteC8, kRouteStemChain, kRoute1x1, kRouteGather,
                   kNumRouteFamilies };
struct RouteFamilyDesc {
  const char* name;
  int nfields;
  const char* field[6];
  int radix[6];  // a field's values are 0 .. radix - 1
};
constexpr RouteFamilyDesc kRouteFamilies[kNumRouteFamilies] = {
    {"igemm", 3, {"NF", "K", "S"}, {9, 4, 3}},
    {"flat", 4, {"NF", "S", "MT", "NS"}, {9, 3, 3, 9}},
    {"persist", 6, {"NF", "S", "NCH", "DB", "POST", "NWV"}, {9, 3, 4, 2, 2, 9}},
    {"chain", 4, {"NF", "DB", "CAT", "NFCAT"}, {3, 2, 4, 5}},
    {"c8", 3, {"NF", "S", "SRC"}, {9, 3, 4}},
    {"stem_chain", 1, {"MODE"}, {3}},
    {"1x1", 4, {"NF", "UP", "NWV", "CLSMAX"}, {9, 2, 9, 2}},
    {"gather", 0, {}, {}},
};
constexpr int route_family_slots(int fam) {
  int n = 1;
  for (int i = 0; i < kRouteFamilies[fam].nfields; ++i) n *= kRouteFamilies[fam].radix[i];
  return n;
}
constexpr int route_family_base(int fam) {
  int b = 0;
  for (int f = 0; f < fam; ++f) b += route_family_slots(f);
  return b;
}
constexpr int kRouteSlots = route_family_base(kNumRouteFamilies);
// slot of (family, field values in the family's order); -1 when a value is outside its radix
template <typename... V>
constexpr int route_id(int fam, V... v) {
  const int vals[] = {0, (int)v...};
  int id = 0;
  for (int i = 0; i < (int)sizeof...(V); ++i) {
    if (vals[i + 1] < 0 || vals[i + 1] >= kRouteFamilies[fam].radix[i]) return -1;
    id = id * kRouteFamilies[fam].radix[i] + vals[i + 1];
  }
  return (int)sizeof...(V) == kRouteFamilies[fam].nfields ? route_family_base(fam) + id : -1;
}
// "family<FIELDvalue,...>" of a slot's field values, the route log's format; returns the length
inline int route_name(char* buf, size_t cap, int fam, const int* vals) {
  const RouteFamilyDesc& d = kRouteFamilies[fam];
  int n = snprintf(buf, cap, "%s", d.name);
  for (int f = 0; f < d.nfields; ++f) n += snprintf(buf + n, cap - n, "%s%s%d", f ? "," : "<", d.field[f], vals[f]);
  return n + snprintf(buf + n, cap - n, "%s", d.nfields ? ">" : "");
}

// ---- dynamic-LDS layouts: offsets of a kernel's regions and its total, in 16-byte units ---------------------------------
constexpr int kTH = 8, kTW = 16;  // output tile of a 4-wave workgroup: two rows of 16 pixels per wave

// Halo patch of `th` x kTW output pixels at stride s: (tile - 1) * s + 3 input pixels each way.  Stride 2 stores a row's
// columns de-interleaved (even | odd, `pwh` each) so that the taps' stride-2 reads are contiguous: `pws` = row pitch.
struct Patch {
  int ph, pw, pwh, pws;
};
constexpr int patch_half(int pw) { return (pw + 1) / 2; }
constexpr int patch_pitch(int pw, int s) { return s == 2 ? 2 * patch_half(pw) : pw; }
// Column of patch pixel px inside its LDS row.  A macro because only kernels use it and they must compile as before:
// behind an (inlined) function call the stride-2 persistent and c8 kernels come out as different machine code.
#define EIOKU_PATCH_COL(px, pwh, s) ((s) == 2 ? (((px) & 1) * (pwh) + ((px) >> 1)) : (px))
constexpr Patch patch_of(int th, int s) {
  return Patch{(th - 1) * s + 3, (kTW - 1) * s + 3, patch_half((kTW - 1) * s + 3), patch_pitch((kTW - 1) * s + 3, s)};
}
constexpr int wt_units(int nf) { return 9 * 16 * nf * 4; }  // one 32-channel chunk of a 3x3 cout tile: [9 taps][16*nf][4]
constexpr size_t lds_bytes(int units) { return (size_t)units * 16; }

// k_conv_igemm, k_conv3x3_flat: [patch: `patch_u`][4 spare: idle slots park their store][wt: one chunk]
struct TileLds {
  int spare, wt, total;
};
constexpr TileLds tile_layout(int patch_u, int nf) { return TileLds{patch_u, patch_u + 4, patch_u + 4 + wt_units(nf)}; }
constexpr TileLds igemm_layout(int nf, int s) { return tile_layout(patch_of(kTH, s).ph * patch_of(kTH, s).pws * 4, nf); }
constexpr TileLds flat_layout(int nf, int s, int pr, int pw) { return tile_layout(pr * patch_pitch(pw, s) * 4, nf); }

// k_conv3x3_persist: [wt: nch chunks][patch: (db ? 2 : 1) x nch x patch_u][1 spare][POST: wt2: the 1x1's (nf + 1) / 2
// chunks of [16*nf][4]][POST: tbuf: per wave [32 px][2*nf]]
struct PersistLds {
  int patch_u, patch, spare, wt2, tbuf, total;  // patch_u: one chunk of one buffer; spare is relative to `patch`
};
constexpr PersistLds persist_layout(int nf, int s, int nch, bool db, bool post = false, int nwv = 4) {
  const int patch_u = patch_of(2 * nwv, s).ph * patch_of(2 * nwv, s).pws * 4, spare = (db ? 2 : 1) * nch * patch_u;
  const int patch = nch * wt_units(nf), wt2 = patch + spare + 1, tbuf = wt2 + (nf + 1) / 2 * 16 * nf * 4;
  return PersistLds{patch_u, patch, spare, wt2, tbuf, post ? tbuf + nwv * 32 * 2 * nf : wt2};
}

// k_conv3x3_chain: [wtA][wtB][xbuf: (db ? 2 : 1) x x_u + 4 spare][p1: p_u + 4 spare (stores of the last fragment's
// tail)][CAT: wt2: (cat + 1) chunks of [16*nf2][4]]
struct ChainLds {
  int x_u, p_u, wtB, xbuf, p1, wt2, w2_u, total;
};
constexpr ChainLds chain_layout(int nf, bool db, int cat = 0, int nf2 = 2) {
  const int x_u = (kTH + 4) * (kTW + 4) * 4, p_u = (kTH + 2) * (kTW + 2) * 4, w2_u = cat > 0 ? (cat + 1) * 16 * nf2 * 4 : 0;
  const int xbuf = 2 * wt_units(nf), p1 = xbuf + (db ? 2 : 1) * x_u + 4, wt2 = p1 + p_u + 4;
  return ChainLds{x_u, p_u, wt_units(nf), xbuf, p1, wt2, w2_u, wt2 + w2_u};
}

// k_conv3x3_c8: [wt: 3 k-steps x [16*nf][4 taps]][patch: 2 x patch_u], one unit per pixel (+ spare for idle slots)
struct C8Lds {
  int patch_u, patch, total;
};
constexpr C8Lds c8_layout(int nf, int s) {
  const int patch_u = patch_of(kTH, s).ph * patch_of(kTH, s).pws + 1;
  return C8Lds{patch_u, 3 * 16 * nf * 4, 3 * 16 * nf * 4 + 2 * patch_u};
}

// k_conv1x1: the whole [nchunks][16*nf][4] weight tile and nothing else
constexpr int conv1x1_units(int nf, int nchunks) { return nchunks * 16 * nf * 4; }

// k_conv_stem_chain: [wt1][wt2][tbuf][p1][xs]
constexpr int kSX_H = 35, kSX_WH = 34, kSX_WS = 68, kSX_PX = kSX_H * kSX_WS;  // image patch, pixels (8 B each)
constexpr int kSP_H = 17, kSP_W = 33, kSP_WH = 17, kSP_WS = 34, kSP_SLOTS = kSP_H * kSP_WS;  // P1, 32 B slots
constexpr int kSC_WT1 = 9 * 32 * 4, kSC_WT2 = 32 * 4, kSC_T = 4 * 32 * 4;
constexpr int kSC_P1_U = (kSP_SLOTS + 1) * 2;       // + one spare slot
constexpr int kSC_XS_U = (kSX_PX + 2) / 2 + 1;      // + spare pixel, 16 B units
constexpr size_t kStemChainLds = lds_bytes(kSC_WT1 + kSC_WT2 + kSC_T + kSC_P1_U + kSC_XS_U);

// ---- weight tiling ---------------------------------------------------------------------------------------------------
// Fewest padded channels first, then the widest tile (fewer re-reads of the input patch).
inline int pick_nf(int cout, int ks, int nchunks, int stride) {
  const int frags = (cout + 15) / 16;
  // (64 -> 80, the class branch's first conv at P3, as ONE 5-fragment 8-wave workgroup of 134 KB instead of 48 + 32
  // couts in two 78 KB workgroups measured no gain: 56.2 vs 56.7 us alone, 41.3 vs 41.3 k frames/s overlapped)
  if (ks == 3 && nchunks <= 3) {
    // persistent kernel: largest tile (<= 4 fragments, no padding waste beyond one fragment) that still fits
    // two workgroups per CU with a single-buffered patch; otherwise fall through to the generic rule
    for (int nf : {4, 3, 2, 1}) {
      const int waste = ((frags + nf - 1) / nf) * nf - frags;
      constexpr int lim_kb = 79;  // two workgroups per 160 KB CU
      if (waste <= (frags >= 4 ? 1 : 0) && lds_bytes(persist_layout(nf, stride, nchunks, false).total) <= (size_t)lim_kb * 1024) {
        // a 1-fragment tile re-reads the halo patch once per 16 couts and is LDS-read bound (3 reads per 2
        // MFMAs): with >= 5 fragments take 3 per tile even if only one workgroup then fits per CU
        if (nf == 1 && frags >= 5 && lds_bytes(persist_layout(3, stride, nchunks, false).total) <= 150 * 1024) return 3;
        return nf;
      }
    }
  }
  const int cands[] = {8, 6, 5, 4, 3, 2, 1};
  int best = 1, best_waste = 1 << 30;
  for (int nf : cands) {
    if (ks == 3 && nf > 6) continue;  // LDS: 9 taps x 16*NF x 64 B
    // 64 KB: with 96-128 KB tiles (NF = 8, 8 waves) the 384/512-channel 1x1 layers are 2-4 us faster each in an
    // isolated trace (-26 us per forward) but the overlapped step is not (40.5 vs 40.4 k frames/s) and the serial
    // profiled step is slower: a workgroup holding most of a CU's LDS keeps the other streams' kernels off that CU
    // beyond 16 chunks (Cin > 512: YOLOv8m / l / x only) a 16-cout tile would re-read the whole input once per 16 couts
    // (Cin = 1152 -> 576: 36 times): up to 128 KB there, one workgroup per CU
    const int lim1 = nchunks > 16 ? 128 : 64;
    if (ks == 1 && nf * nchunks > lim1 && nf > 1) continue;  // 1x1: the whole Cin x tile weight block lives in LDS (nf*nchunks KB)
    int waste = ((frags + nf - 1) / nf) * nf - frags;
    if (waste < best_waste) {
      best_waste = waste;
      best = nf;
    }
  }
  return best;
}

// ---- the plan: which instantiation a layer runs on, decided before anything is launched ------------------------------
struct PlanLayer {  // a layer as conv_forward knows it once its arguments are valid: integers and flags, no pointer
  int ks, stride, cin, cout, nf, nchunks;
  int N, H, W, in_cs;
  bool res, out_f32, post, up, clsmax, fused;
  int src;  // k_conv3x3_c8's SRC: 0 tensor input, 1 / 2 / 3 the fused letterbox modes
};
struct ConvPlan {
  int family = -1, t[6] = {0, 0, 0, 0, 0, 0};  // route family and its template arguments in the route table's order
  int threads = 256;
  size_t lds = 0;   // dynamic LDS bytes of the launch
  int pr = 0, pw = 0;  // flat: rows and columns of the worst-case patch (kernel arguments)
  int wg_cu = 0;       // 1x1: workgroups per CU beyond which the grid strides
  char err[96] = "";   // no kernel runs this layer: the message, and nothing above is set
  bool ok() const { return family >= 0; }
};
inline ConvPlan plan_routed(int family, size_t lds, int t0, int t1 = 0, int t2 = 0, int t3 = 0, int t4 = 0, int t5 = 0) {
  ConvPlan p;
  p.family = family;
  p.lds = lds;
  const int t[6] = {t0, t1, t2, t3, t4, t5};
  for (int i = 0; i < 6; ++i) p.t[i] = t[i];
  return p;
}
// Flattened-pixel deep-K tiles: geometry of the worst-case patch of 64 * mt consecutive pixels, then the largest tile
// whose staging fits the per-thread slot budget.  Not ok(): the layer is left to the kernels further down.
inline ConvPlan plan_flat(const PlanLayer& l, int Ho, int Wo) {
  ConvPlan p;
  // 32-bit element offsets; pixel / virtual-row indices below 2^24 (fast_div)
  if ((long long)l.N * l.H * l.W * l.in_cs >= (1ll << 31) || (long long)l.N * (l.H + 1) * (l.W + 2) >= (1ll << 24)) return p;
  if (l.nf < 2 || l.nf > 6) return p;
  int slots = 0;
  for (int mt : {2, 1}) {
    const int tpx = 64 * mt, r_o = (Wo - 2 + tpx) / Wo + 1, over = (l.H + 1) - Ho * l.stride;
    int cross = (tpx - 1) / (Ho * Wo) + 1;
    if (cross > r_o - 1) cross = r_o - 1;
    const int pr = (r_o - 1) * l.stride + 3 + cross * (over > 0 ? over : 0), pw = (Wo - 1) * l.stride + 3;
    slots = (pr * pw * 4 + 255) / 256;
    p = plan_routed(kRouteFlat, lds_bytes(flat_layout(l.nf, l.stride, pr, pw).total), l.nf, l.stride, mt, slots <= 4 ? 4 : 8);
    p.pr = pr;
    p.pw = pw;
    if (slots <= 8 && p.lds <= 80 * 1024) return p;
  }
  return slots <= 8 && p.lds <= 150 * 1024 ? p : ConvPlan{};
}

inline ConvPlan plan_conv(const PlanLayer& l) {
  const int Ho = conv_out_dim(l.H, l.ks, l.stride), Wo = conv_out_dim(l.W, l.ks, l.stride);
  const int nf = l.nf, s = l.stride, nch = l.nchunks;
  auto persist_b = [&](bool db, bool post = false, int nwv = 4) { return lds_bytes(persist_layout(nf, s, nch, db, post, nwv).total); };
  auto persist = [&](bool db, bool post, int nwv) {
    ConvPlan p = plan_routed(kRoutePersist, persist_b(db, post, nwv), nf, s, nch, db, post, nwv);
    p.threads = 64 * nwv;
    return p;
  };
  auto fail = [](const char* fmt, int a, int b = 0) {
    ConvPlan p;
    snprintf(p.err, sizeof p.err, fmt, a, b);
    return p;
  };
  if (l.ks == 3 && l.cin == 8 && s == 2 && !l.res && !l.out_f32 && nf >= 1 && nf <= 5)
    return plan_routed(kRouteC8, lds_bytes(c8_layout(nf, s).total), nf, s, l.src);
  if (l.fused) return fail("no fused-input kernel for this stem (nf %d)", nf);
  // maps too small for 8x16 tiles (20x20: 52 % of a tiling is outside the map): flattened-pixel tiles whatever
  // the depth.  Measured: 80->80 @20 19.8 -> 13.8 us, 64->64 @20 13.2 -> 10.5; at 40x40 resident weights still
  // win (64->64 20.7 vs 25.8 us), hence the 24-pixel cut.
  constexpr int flat_wo = 24;
  if (l.ks == 3 && nch >= 2 && nch <= 3 && Wo <= flat_wo) {
    const ConvPlan p = plan_flat(l, Ho, Wo);
    if (p.ok()) return p;
  }
  // 3x3 + following 1x1 in one launch (the intermediate tensor never exists).  Instantiated for the two shapes the
  // YOLOv8 backbone has (stride-2 conv -> C2f.cv1 with 32 / 64 channels) and their stride-1 twins.
  // stride-2, 64 couts (model.3 -> model.4.cv1): 98 KB of LDS = one 4-wave workgroup per CU.  An 8-wave 16x16-tile
  // variant (149 KB, two waves on every SIMD) measured 54 -> 50 us alone but a slower overlapped step (41.8 vs 42.2 k
  // frames/s: 149 KB leave no LDS for the other streams' workgroups) and was removed.
  if (l.post) {
    if ((nf == 2 || nf == 4) && (nch == 1 || nch == 2)) return persist(persist_b(true, true) <= 75 * 1024, true, 4);
    return fail("no fused 3x3+1x1 kernel for nf %d nchunks %d", nf, nch);
  }
  if (l.ks == 3 && nch <= 3) {
    // double-buffer the patch only when that still leaves two workgroups per CU
    const bool db = persist_b(true) <= 75 * 1024;
    if (persist_b(db) <= 150 * 1024) {
      // weight block too large for two workgroups per CU: one 8-wave workgroup with a 16x16 tile (two waves per SIMD)
      if (s == 1 && !db && nf == 3 && nch == 3 && persist_b(false) > 80 * 1024 && persist_b(false, false, 8) <= 160 * 1024 && Ho > 8)
        return persist(false, false, 8);
      if (s == 1 && !db && nf == 5 && nch == 2 && Ho > 8) return persist(false, false, 8);
      if (nf >= 1 && nf <= (nch == 1 ? 6 : 5)) return persist(db, false, 4);
    }
  }
  // (YOLOv8m's 96 / 192-channel stride-2 convs at 80 / 40-wide maps have no persistent instantiation and fall through to
  // the generic kernel, 200 TFLOP/s; sending them here with 16 staging slots measured the same: 370 vs 404 us)
  if (l.ks == 3 && nch > 3 && Wo <= 48) {
    const ConvPlan p = plan_flat(l, Ho, Wo);
    if (p.ok()) return p;
  }
  if (nf < 1 || nf == 7 || nf > 8) return fail("unsupported nf %d", nf);
  if (l.ks == 3) return plan_routed(kRouteIgemm, lds_bytes(igemm_layout(nf, s).total), nf, 3, s);
  // Workgroups per CU: few and persistent.  Measured on the 64-frame forward (19 1x1 layers, 8 -> 2 workgroups per
  // CU: 625 -> 555 us): every workgroup pays the weight-tile copy and its dispatch, and one-group-per-wave grids
  // (800 workgroups at 40x40) never reach the grid-stride loop that hides the load latency.  The widest tiles (NF = 8:
  // 64 MFMAs per pixel group and wave) are best with ONE workgroup per CU.
  ConvPlan p = plan_routed(kRoute1x1, lds_bytes(conv1x1_units(nf, nch)), nf, l.up, 4, l.clsmax);
  p.wg_cu = (nf >= 8 || p.lds > 80 * 1024) ? 1 : 2;
  return p;
}

}  // namespace eioku
