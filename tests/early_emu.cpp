// early_emu.cpp — test-only: rays that miss the world box resolved in k_shade
// (WaveArgs::early_miss, RT_OPT_EARLY_MISS) on the host.  The production
// wavefront kernels (wavefront.hip, one lane per workgroup) run a caller's
// scene description twice over the same DScene: through wave_run.h's schedule
// with the word 0 (every ray queued), and through the same order of launches
// with the word set, in the instrumented variants, so that the two frames can
// be compared bit for bit and the new counters read (tests/test_early_host.py).
// With the word set k_shade keeps the back of the stream and its three count
// sets itself (wavefront.h cnt_back) and applies NEE jobs in place; the
// launches and their arguments are the same.
//
// Also here: world_box_missed against trav_init's early-out, ray by ray.
//
// Built twice: as a plain shared library (no sanitizer, nothing to preload)
// that the tests load with ctypes, like tests/lift_emu.cpp; and, with
// -DEARLY_EMU_MAIN, as a stand-alone program under AddressSanitizer + UBSan
// that renders a closed room and a scene in several batches both ways.  Not a
// product path.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../go-raytracing_amd/csrc/wavefront.hip"
#include "../go-raytracing_amd/csrc/wave_layout.h"
#include "emu_scene.h"
#include "wave_run.h"

using namespace rtg;

namespace {

constexpr int kRing = wave_run::kRing;

int load(const rt_scene_desc* desc, const rt_camera_desc* cam, int node_format, int lift, emu::EmuScene& E) {
  FlattenOptions fo;
  fo.quant_nodes = node_format;
  fo.lift_prims = lift;
  return emu::load_desc(desc, cam, fo, E);
}

// One row per bounce of every batch: what k_shade left for the next bounce.
struct BounceLog {
  int32_t batch, bounce, slots, front, back, jobs;
};

// wave_run::run's order of launches (serial, or the bounce overlap's: bounce
// b's k_shadow / k_nee_apply after bounce b + 1's k_extend) over the
// instrumented kernels.
template <bool kVol, bool kEnvIS, int kShade, bool kQuant, bool kWide>
void run_early(const DScene& sc, const DCamera& cam, WaveArgs a, uint32_t spp, uint32_t spb, int max_depth, float* out,
               bool ovl, std::vector<BounceLog>& log) {
  uint32_t* cnt_stream[2] = {a.counts + CNT_STREAM0, a.counts + CNT_STREAM1};
  uint32_t* fetch_ext = a.counts + CNT_FETCH_EXT;
  for (double* p = a.acc; p < a.acc + size_t(a.npix) * 3; ++p) *p = 0.0;
  auto nee = [&](int b) {
    if (sc.num_lights == 0) return;
    uint32_t* const cnt_sh = a.counts + cnt_shadow(b & 1);
    k_shadow<kRing, true, kVol, kEnvIS, kQuant, kWide>(sc, a, cnt_sh, a.counts + cnt_fetch_sh(b & 1),
                                                       a.counts + cnt_fetch_sh((b + 1) & 1));
    k_nee_apply<kEnvIS>(a, cnt_sh);
  };
  int batch = 0;
  for (uint32_t sa = 0; sa < spp; sa += spb, ++batch) {
    const uint32_t sb = spp - sa < spb ? spp - sa : spb;
    const uint32_t nslots = sb * a.npix;
    // what an earlier batch left in the counters must not matter
    for (uint32_t k = 0; k < 3u; ++k) a.counts[cnt_back(k)] = 0xDEADu;
    k_set_counts(a.counts, nslots);
    int pending = -1;
    for (int b = 0; b < max_depth; ++b) {
      const int c = b & 1, nx = c ^ 1;
      uint32_t* const cnt_sh = a.counts + cnt_shadow(c);
      uint32_t* const fetch_sh = a.counts + cnt_fetch_sh(c);
      if (b == 0)
        k_extend<kRing, true, kVol, true, kQuant, kWide>(sc, cam, a, a.s[c], cnt_stream[c], cnt_stream[nx], cnt_sh, fetch_sh,
                                                         fetch_ext, sa);
      else
        k_extend<kRing, true, kVol, false, kQuant, kWide>(sc, cam, a, a.s[c], cnt_stream[c], cnt_stream[nx], cnt_sh, fetch_sh,
                                                          fetch_ext, sa);
      if (pending >= 0) { nee(pending); pending = -1; }
      if (b == 0) k_shade<true, kEnvIS, kShade, true>(sc, cam, a, a.s[c], cnt_stream[c], a.s[nx], cnt_stream[nx], cnt_sh, sa, 0u);
      else k_shade<true, kEnvIS, kShade, false>(sc, cam, a, a.s[c], cnt_stream[c], a.s[nx], cnt_stream[nx], cnt_sh, sa,
                                                 uint32_t(b));
      log.push_back({batch, b, int32_t(nslots), int32_t(*cnt_stream[nx]),
                     (a.early_miss & EARLY_NEXT) ? int32_t(a.counts[cnt_back(uint32_t(b) + 1u)]) : 0, int32_t(*cnt_sh)});
      if (ovl) pending = b;
      else nee(b);
    }
    if (pending >= 0) nee(pending);
    k_accum(a, sb);
  }
  k_finalize(a, out, 0);
}

// The frame with WaveArgs::early_miss = `early` (wave_run::render's buffers:
// exactly sized, one allocation per array).  work[]: extend rays, shade paths,
// NEE jobs written, shadow rays traced, NEE rays and next rays resolved in
// k_shade.
int render_early(const emu::EmuScene& E, uint32_t seed, uint32_t spp, uint32_t spb, int max_depth, uint32_t early, bool ovl,
                 std::vector<float>& out, uint64_t* work, std::vector<BounceLog>& log) {
  const DScene& d = E.d;
  const DCamera& cam = E.cam;
  const uint32_t npix = uint32_t(cam.width) * uint32_t(cam.height);
  const size_t S = size_t(spb) * npix;
  const bool lit = d.num_lights > 0;
  const int spill_cap = spill_cap_for(int(d.stack_needed), kRing);
  std::vector<std::vector<float4>> f4(slot_f4(lit), std::vector<float4>(S, float4{0.0f, 0.0f, 0.0f, 0.0f}));
  std::vector<uint32_t> q(CNT_WORDS_Q, 0u), sj_info(lit ? S : 0, 0u), sj_vis(lit ? S : 0, 0u);
  std::vector<uint32_t> pixels(npix);
  for (uint32_t i = 0; i < npix; ++i) pixels[i] = npix - 1u - i;
  std::vector<uint32_t> spill(size_t(spill_cap), 0u), spill_sh(size_t(spill_cap), 0u);
  std::vector<double> acc(size_t(npix) * 3, 0.0);
  std::vector<unsigned long long> counters(3 * CNT_BLOCK, 0ull);
  int err = 0;

  WaveArgs a{};
  auto arr = [&](int k) { return f4[size_t(k)].data(); };
  for (int k = 0; k < 2; ++k) a.s[k] = PathStream{arr(3 * k), arr(3 * k + 1), arr(3 * k + 2)};
  a.hit = arr(6); a.Lout = arr(7);
  a.counts = q.data();
  if (lit) {
    a.sj_p = arr(8); a.sj_a = arr(9); a.sj_h = arr(10);
    a.ne_a = arr(11); a.ne_h = arr(12); a.ne_beta = arr(13);
    a.sj_info = sj_info.data();
    a.sj_vis = sj_vis.data();
  }
  a.pixels = pixels.data();
  a.npix = npix;
  a.acc = acc.data();
  a.seed = seed;
  a.max_depth = max_depth;
  a.counters = counters.data();
  a.err = &err;
  a.refill = 1;
  a.spill = spill.data();
  a.spill_sh = spill_sh.data();
  a.spill_lanes = 1;
  a.spill_cap = spill_cap;
  a.slots = uint32_t(S);
  a.out_pixels = uint32_t(npix);
  a.early_miss = early;

  out.assign(size_t(npix) * 3, 0.0f);
  const WaveVariant v = pick_variant(d);
  with_traversal(v, [&](auto V, auto Q, auto W) {
    with_shading(v, [&](auto H, auto F) {
      run_early<decltype(V)::value, decltype(H)::value, decltype(F)::value, decltype(Q)::value, decltype(W)::value>(
          d, cam, a, spp, spb, max_depth, out.data(), ovl, log);
    });
  });
  const unsigned long long* ce = counters.data() + KC_EXTEND * CNT_BLOCK;
  const unsigned long long* cs = counters.data() + KC_SHADE * CNT_BLOCK;
  const unsigned long long* cd = counters.data() + KC_SHADOW * CNT_BLOCK;
  // (block words: samples, then the Cnt fields in declaration order)
  work[0] = ce[1]; work[1] = cs[1]; work[2] = cs[2]; work[3] = cd[2]; work[4] = cs[14]; work[5] = cs[15];
  return err;
}

// Both frames of the scene and how they compare.  Returns the number of
// floats whose bits differ, or a negative status.
long compare(const emu::EmuScene& E, uint32_t seed, uint32_t spp, uint32_t spb, int max_depth, uint32_t early, bool ovl,
             std::vector<float>& f_ref, std::vector<float>& f_new, uint64_t* work, std::vector<BounceLog>& log) {
  size_t slots = 0;
  if (wave_run::render(E, seed, 0u, spp, spb, max_depth, f_ref, &slots)) return -6;
  if (render_early(E, seed, spp, spb, max_depth, early, ovl, f_new, work, log)) return -6;
  long diff = 0;
  for (size_t i = 0; i < f_ref.size(); ++i) diff += memcmp(&f_ref[i], &f_new[i], 4) != 0;
  return diff;
}

}  // namespace

// The description rendered through wave_run.h's schedule (every ray queued)
// and with WaveArgs::early_miss = `early` where the scene is eligible
// (early_miss_eligible; 0 otherwise), `spp` samples in batches of `spb`.
// Returns the number of frame floats whose bits differ (0 = identical), or a
// negative status.  out: the frame with the word set.  work[6]: see
// render_early.  log: up to max_log rows of 6 (batch, bounce, slots of the
// batch, next stream's front count, its back count, NEE jobs written);
// info[0] rows, [1] the word used, [2] node format taken, [3] lifted records,
// [4] lights, [5] check_box, [6] planes.
extern "C" long early_emu_compare(const rt_scene_desc* desc, const rt_camera_desc* cam, int node_format, int lift,
                                  uint32_t seed, uint32_t spp, uint32_t spb, int max_depth, uint32_t early, int overlap,
                                  float* out, uint64_t* work, int32_t* log, int max_log, int32_t* info) {
  emu::EmuScene E;
  if (int rc = load(desc, cam, node_format, lift, E)) return -rc;
  const DScene& sc = E.d;
  const uint32_t word = early_miss_eligible(sc) ? early : 0u;
  std::vector<float> f_ref, f_new;
  std::vector<BounceLog> rows;
  const long diff = compare(E, seed, spp, spb, max_depth, word, overlap != 0, f_ref, f_new, work, rows);
  if (diff < 0) return diff;
  memcpy(out, f_new.data(), f_new.size() * sizeof(float));
  const int n = int(rows.size()) < max_log ? int(rows.size()) : max_log;
  for (int i = 0; i < n; ++i) memcpy(log + 6 * i, &rows[size_t(i)], sizeof(BounceLog));
  info[0] = n; info[1] = int32_t(word); info[2] = sc.wide_nodes ? 2 : sc.quant_nodes ? 1 : 0; info[3] = sc.num_prim_recs;
  info[4] = sc.num_lights; info[5] = sc.tlas.check_box; info[6] = sc.num_planes;
  return diff;
}

// world_box_missed against trav_init, ray by ray: pred[i] = the predicate on
// (o, d, 0.001, hi) with hi = cull_widen(tmax) for a closest-hit ray and tmax
// for an any-hit ray (`any`); done[i] = trav_init ended the ray with TRAV_DONE
// (its root-box early-out: the scene has no plane).  box[6]: the world box.
extern "C" int early_emu_predicate(const rt_scene_desc* desc, const rt_camera_desc* cam, int node_format, int lift, int any,
                                   int n, const float* o, const float* d, const float* tmax, uint8_t* pred, uint8_t* done,
                                   float* box, int32_t* info) {
  emu::EmuScene E;
  if (int rc = load(desc, cam, node_format, lift, E)) return rc;
  const DScene& sc = E.d;
  info[0] = sc.tlas.check_box; info[1] = sc.num_planes; info[2] = sc.wide_nodes ? 2 : sc.quant_nodes ? 1 : 0;
  for (int k = 0; k < 6; ++k) box[k] = sc.tlas.box[k];
  if (!world_box_decides(sc)) return 7;
  uint32_t lds[kLdsStack + kWorldRayWords + kWorldInvWords + kHitWords] = {};
  const TStack S{lds, 1, kLdsStack, nullptr, lds, 1, 0, nullptr, true};
  Cnt cnt = {};
  for (int i = 0; i < n; ++i) {
    const V3 ro = mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    Trav T{};
    int s;
    if (any) {
      pred[i] = world_box_missed(sc, ro, rd, 0.001f, tmax[i]);
      s = sc.wide_nodes ? trav_init<true, false, true>(sc, T, S, ro, rd, 0.0f, 0.001f, tmax[i], 0u, 0u, DOM_VOL_SH_AREA, cnt)
                        : trav_init<true, false, false>(sc, T, S, ro, rd, 0.0f, 0.001f, tmax[i], 0u, 0u, DOM_VOL_SH_AREA, cnt);
    } else {
      pred[i] = world_box_missed(sc, ro, rd, 0.001f, cull_widen(tmax[i]));
      s = sc.wide_nodes ? trav_init<false, false, true>(sc, T, S, ro, rd, 0.0f, 0.001f, tmax[i], 0u, 0u, DOM_VOL, cnt)
                        : trav_init<false, false, false>(sc, T, S, ro, rd, 0.0f, 0.001f, tmax[i], 0u, 0u, DOM_VOL, cnt);
    }
    done[i] = s == TRAV_DONE;
  }
  return 0;
}

#ifdef EARLY_EMU_MAIN
// early_emu NAME WIDTH ASSET_DIR [RINGS COLS]: the named librtscene scene
// (cornell-lucy: a closed room with the camera inside) at 3 spp, depth 3 in
// one batch and at depth 5 in batches of 1 and 2 samples, serial and in the
// bounce overlap's order, both ways.  Prints one line per run; exit status 0
// when every pair of frames is identical and rays took the early paths.
int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: early_emu NAME WIDTH ASSET_DIR [RINGS COLS]\n"); return 2; }
  rts_scene_options opt{};
  opt.width = atoi(argv[2]);
  opt.asset_dir = argv[3];
  opt.lucy_rings = argc > 4 ? atoi(argv[4]) : 8;
  opt.lucy_cols = argc > 5 ? atoi(argv[5]) : 10;
  char err[512] = {0};
  rts_scene* scn = nullptr;
  if (rts_scene_create(argv[1], &opt, &scn, err, sizeof err) != 0) { fprintf(stderr, "%s\n", err); return 3; }
  emu::EmuScene E;
  if (int rc = load(rts_scene_get_desc(scn), rts_scene_get_camera(scn), 0, 1, E)) return rc;
  int bad = early_miss_eligible(E.d) ? 0 : 1;
  const struct { uint32_t spb; int depth; bool ovl; } runs[] = {{3u, 3, false}, {1u, 5, false}, {2u, 5, true}};
  for (const auto& r : runs) {
    std::vector<float> f_ref, f_new;
    std::vector<BounceLog> rows;
    uint64_t work[6] = {};
    const long diff = compare(E, 7u, 3u, r.spb, r.depth, EARLY_NEE | EARLY_NEXT, r.ovl, f_ref, f_new, work, rows);
    int over = 0;
    for (const BounceLog& l : rows) over += l.front + l.back > l.slots;
    printf("{\"spb\": %u, \"depth\": %d, \"overlap\": %d, \"differ\": %ld, \"early_nee\": %llu, \"early_next\": %llu, "
           "\"jobs\": %llu, \"over\": %d}\n",
           r.spb, r.depth, int(r.ovl), diff, (unsigned long long)work[4], (unsigned long long)work[5],
           (unsigned long long)work[2], over);
    bad += diff != 0 || work[4] == 0 || work[5] == 0 || over != 0;
  }
  rts_scene_destroy(scn);
  return bad ? 1 : 0;
}
#endif
