// emu_trace.h — test-only: one ray through the production closest-hit kernel
// (wavefront.hip k_extend, a later bounce: the ray read from the path stream)
// on the host, one lane.  Include after wavefront.hip and emu_scene.h
// (tests/ray_emu.cpp, tests/hits_emu.cpp).
#pragma once
#include <cstring>
#include <vector>

#include "../go-raytracing_amd/csrc/wave_layout.h"
#include "../go-raytracing_amd/csrc/wave_variant.h"

namespace emu {

using namespace rtg;

constexpr int kTraceRing = 8;

// The buffers k_extend reads and writes for one path slot, and the WaveArgs
// over them.  The spill area holds what the scene's stack bound leaves beyond
// the ring (wave_layout.h spill_cap_for, as render_wave and wave_run.h size
// it), not the kernels' largest depth: a bound one entry short shows here as
// it would on the device.
struct TraceArgs {
  std::vector<float4> f4 = std::vector<float4>(size_t(kSlotF4), float4{0.0f, 0.0f, 0.0f, 0.0f});
  std::vector<uint32_t> q = std::vector<uint32_t>(CNT_WORDS_Q, 0u), sj = std::vector<uint32_t>(2, 0u);
  std::vector<uint32_t> pixels = std::vector<uint32_t>(1, 0u);
  std::vector<uint32_t> spill;
  std::vector<double> acc = std::vector<double>(3, 0.0);
  std::vector<unsigned long long> counters = std::vector<unsigned long long>(3 * CNT_BLOCK, 0ull);
  int err = 0;
  WaveArgs a{};

  TraceArgs(int max_depth, int stack_needed, int ring = kTraceRing)
      : spill(size_t(spill_cap_for(stack_needed, ring)), 0u) {
    auto arr = [&](int k) { return &f4[size_t(k)]; };
    for (int k = 0; k < 2; ++k) a.s[k] = PathStream{arr(3 * k), arr(3 * k + 1), arr(3 * k + 2)};
    a.hit = arr(6); a.Lout = arr(7);
    a.sj_p = arr(8); a.sj_a = arr(9); a.sj_h = arr(10);
    a.ne_a = arr(11); a.ne_h = arr(12); a.ne_beta = arr(13);
    a.counts = q.data();
    a.sj_info = sj.data();
    a.sj_vis = sj.data() + 1;
    a.pixels = pixels.data();
    a.npix = 1;
    a.acc = acc.data();
    a.max_depth = max_depth;
    a.counters = counters.data();
    a.err = &err;
    a.refill = 1;
    a.spill = spill.data();
    a.spill_lanes = 1;
    a.spill_cap = int(spill.size());
    a.slots = 1;
    a.out_pixels = 1;
  }
  TraceArgs(const TraceArgs&) = delete;
  TraceArgs& operator=(const TraceArgs&) = delete;
};

// key: the path's RNG key (d.w of the stream's ray); bounce: the path's
// bounce as the stream carries it (beta.w bits 16..30), which only the
// rare-primitive variant (kVol: volumes in the world BVH) reads.
template <bool kWide, bool kQuant, bool kVol = false, int kRingN = kTraceRing>
static float4 trace_variant(const DScene& sc, const DCamera& cam, WaveArgs a, float4 o, float4 d, uint32_t key = 0u,
                            uint32_t bounce = 0u) {
  const uint32_t bw = (bounce & 0x7FFFu) << 16;
  float bwf;
  std::memcpy(&d.w, &key, 4);
  std::memcpy(&bwf, &bw, 4);
  a.s[0].o[0] = o;
  a.s[0].d[0] = d;
  a.s[0].beta[0] = float4{1.0f, 1.0f, 1.0f, bwf};
  a.counts[CNT_STREAM0] = 1u;
  for (uint32_t k = 0; k < kSegs; ++k) a.counts[CNT_FETCH_EXT + k * kSegStride] = 0u;
  k_extend<kRingN, false, kVol, false, kQuant, kWide>(sc, cam, a, a.s[0], a.counts + CNT_STREAM0,
                                                          a.counts + CNT_STREAM1, a.counts + CNT_SHADOW,
                                                          a.counts + CNT_FETCH_SH, a.counts + CNT_FETCH_EXT, 0u);
  return a.hit[0];
}

// One shadow ray through the production any-hit kernel (wavefront.hip
// k_shadow, one job: the area-light ray from P along dir to tmax) in the
// variant of the scene's node format; a.spill_sh is the caller's.  Returns
// the job's visibility word (bit 0: the ray passed).
template <bool kWide, bool kQuant, bool kVol = false, int kRingN = kTraceRing>
static uint32_t shadow_variant(const DScene& sc, WaveArgs a, const float* P, const float* dir, float tmax, uint32_t key,
                               uint32_t bounce) {
  float kf;
  std::memcpy(&kf, &key, 4);
  a.sj_p[0] = float4{P[0], P[1], P[2], kf};
  a.sj_a[0] = float4{dir[0], dir[1], dir[2], tmax};
  a.sj_info[0] = 1u | (bounce << 8);
  a.sj_vis[0] = 0u;
  a.counts[cnt_shadow(0)] = 1u;
  for (uint32_t k = 0; k < kSegs; ++k) a.counts[cnt_fetch_sh(0) + k * kSegStride] = 0u;
  k_shadow<kRingN, false, kVol, false, kQuant, kWide>(sc, a, a.counts + cnt_shadow(0), a.counts + cnt_fetch_sh(0),
                                                      a.counts + cnt_fetch_sh(1));
  return a.sj_vis[0];
}

// The hit record k_extend stores (store_hit: t, kind << 28 | idx, instance,
// TLAS ref position) for a path's ray (key: its RNG key) at a given bounce,
// in the variant the product picks for the scene, with a stack ring of
// kRingN entries.
template <int kRingN = kTraceRing>
static float4 trace_path(const EmuScene& E, TraceArgs& T, const float* o, const float* d, uint32_t key = 0u,
                         uint32_t bounce = 0u) {
  const float4 ro{o[0], o[1], o[2], 0.0f}, rd{d[0], d[1], d[2], 0.0f};
  return with_traversal(pick_variant(E.d), [&](auto V, auto Q, auto W) {
    return trace_variant<decltype(W)::value, decltype(Q)::value, decltype(V)::value, kRingN>(E.d, E.cam, T.a, ro, rd, key, bounce);
  });
}

// One shadow ray of a path through k_shadow in the same variant
// (shadow_variant's visibility word).
template <int kRingN = kTraceRing>
static uint32_t shadow_path(const EmuScene& E, TraceArgs& T, const float* P, const float* dir, float tmax, uint32_t key,
                            uint32_t bounce) {
  return with_traversal(pick_variant(E.d), [&](auto V, auto Q, auto W) {
    return shadow_variant<decltype(W)::value, decltype(Q)::value, decltype(V)::value, kRingN>(E.d, T.a, P, dir, tmax, key, bounce);
  });
}

// A hit record's words, and the hittable ids it names as rt_primary_hits
// reports them (probe.hip hit_ids; top = prim = -1 and t = -1 for a miss).
struct Hit {
  uint32_t kh;   // kind << 28 | idx, 0: a miss
  float t;
  int inst, refpos;
};
static Hit unpack(float4 h) {
  uint32_t w[4];
  std::memcpy(w, &h, 16);
  return Hit{w[1], h.x, int(w[2]), int(w[3])};
}
static void hit_ids(const DScene& sc, const Hit& h, int32_t& top, int32_t& prim, float& t) {
  top = prim = -1;
  t = -1.0f;
  if (h.kh == 0u) return;
  const int kind = int(h.kh >> 28), idx = int(h.kh & 0x0FFFFFFFu);
  t = h.t;
  if (kind == PK_PLANE) { top = prim = sc.plane_hidx[idx]; return; }
  top = sc.tlas_ref_top[h.refpos];
  prim = kind == PK_SPHERE ? sc.sphere_hidx[idx] : kind == PK_QUAD ? sc.quad_hidx[idx] : kind == PK_TRI ? sc.tri_hidx[idx]
         : kind == PK_CIRCLE ? sc.circle_hidx[idx] : sc.volume_hidx[idx];
}

// What shade_path and the path probe add to k_extend's hit: the lifted
// volumes' and the lifted world primitives' tests.
static void merge_lifted(const DScene& sc, Hit& r, V3 ro, V3 rd, uint32_t key, uint32_t bounce) {
  Cnt cnt = {};
  if (sc.num_vol_refs > 0) lifted_volumes<false>(sc, ro, rd, key, bounce, r.kh, r.t, r.inst, r.refpos, cnt, sc.vol_recs);
  if (sc.num_prim_recs > 0) lifted_prims<false>(sc, ro, rd, ray_time(key), r.kh, r.t, r.inst, r.refpos, cnt);
}

// The closest hit of one path ray as the pipeline finds it.
static Hit closest(const EmuScene& E, TraceArgs& T, const float* o, const float* d, uint32_t key, uint32_t bounce) {
  Hit r = unpack(trace_path(E, T, o, d, key, bounce));
  merge_lifted(E.d, r, mk(o[0], o[1], o[2]), mk(d[0], d[1], d[2]), key, bounce);
  return r;
}

// One path's bounce through the production shade_path in the variant the
// scene runs (wave_variant.h; kFirst at bounce 0) with a one-slot Lout: what
// shade_path decides, and L, the radiance it added.
struct Shaded {
  bool cont = false, want_shadow = false, lout_set = false;
  uint32_t flags = 0, nstate = 0;
  float tmax_a = 0.0f;
  V3 P{}, sd{}, nbeta{}, ca{}, ch{}, da{}, dh{};
  float4 L{};
};
static Shaded shade_by_kind(const EmuScene& E, TraceArgs& T, float4 h, V3 ro, V3 rd, V3 beta, uint32_t key, int dleft,
                            uint32_t bounce, bool allow) {
  Shaded r;
  Cnt cnt = {};
  T.a.Lout[0] = float4{0.0f, 0.0f, 0.0f, 0.0f};
  with_shading(pick_variant(E.d), [&](auto H, auto S) {
    auto go = [&](auto F) {
      shade_path<false, decltype(H)::value, decltype(S)::value, decltype(F)::value>(
          E.d, E.cam, T.a, E.d.vol_recs, h, ro, rd, beta, key, 0u, dleft, bounce, allow, r.cont, r.want_shadow, r.flags,
          r.nstate, r.tmax_a, r.P, r.sd, r.nbeta, r.ca, r.ch, r.da, r.dh, r.lout_set, cnt);
    };
    if (bounce == 0) go(std::true_type{}); else go(std::false_type{});
  });
  if (!r.want_shadow) r.flags = 0u;
  r.L = T.a.Lout[0];
  return r;
}

}  // namespace emu
