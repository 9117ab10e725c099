// ray_color_emu.cpp — test-only: rt_ray_color's pipeline on the host.  The
// production ray source (go-raytracing_amd/csrc/ray_source.hip k_ray_source)
// and the production later-bounce kernels of wavefront.hip, compiled through
// tests/host_emu (one lane per workgroup, one workgroup per launch) and driven
// like run_batches' ray mode: per batch k_set_counts (stream 0 empty),
// k_ray_source, then k_extend / k_shade <kFirst = false> from bounce 0 on,
// k_shadow, k_nee_apply, k_accum; k_finalize.  Its own batch loop, written
// like tests/wave_run.h's (the camera pipeline, which it is compared with).
// The traversal stack ring is wave_run's 4 entries, so deep traversals spill.
//
// Two builds:
//   * a plain shared library (ray_color_emu_run: a caller's scene description
//     and rays; tests/test_ray_color_kat.py);
//   * -DRAY_COLOR_EMU_MAIN: a stand-alone program over a librtscene scene,
//     under AddressSanitizer + UBSan (tests/test_ray_color_host.py):
//       ray_color_emu <scene> <asset_dir> <depth, 0 = the scene's> <volumes_in_bvh>
//     makes the 16 x 12 camera rays with the production get_ray, runs them
//     through the ray mode with id = pixel, and compares with wave_run::render.
// Not a product path.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../go-raytracing_amd/csrc/wavefront.hip"
#include "../go-raytracing_amd/csrc/ray_source.hip"
#include "../go-raytracing_amd/csrc/wave_layout.h"
#include "emu_scene.h"
#include "wave_run.h"

using namespace rtg;

namespace ray_run {

constexpr int kRing = wave_run::kRing;

// stream_counts: counts[CNT_STREAM0] after each batch's k_ray_source
template <bool kVol, bool kEnvIS, int kShade, bool kQuant, bool kWide = false>
void run(const DScene& sc, const DCamera& cam, WaveArgs a, const RaySource& src, uint32_t spp, uint32_t spb, int max_depth,
         float* out, uint32_t sample_offset, int accumulate, std::vector<uint32_t>& stream_counts) {
  uint32_t* cnt_stream[2] = {a.counts + CNT_STREAM0, a.counts + CNT_STREAM1};
  uint32_t* fetch_ext = a.counts + CNT_FETCH_EXT;
  for (double* p = a.acc; p < a.acc + size_t(a.npix) * 3; ++p) *p = 0.0;
  const int tail_after = getenv("RTG_EMU_TAIL") ? atoi(getenv("RTG_EMU_TAIL")) : -1;
  for (uint32_t sa = 0; sa < spp; sa += spb) {
    const uint32_t sb = spp - sa < spb ? spp - sa : spb;
    const uint32_t s0 = sample_offset + sa;
    const uint32_t nslots = sb * a.npix;
    k_set_counts(a.counts, 0u);
    k_ray_source(a, src, nslots, s0);
    stream_counts.push_back(a.counts[CNT_STREAM0]);
    for (int b = 0; b < max_depth; ++b) {
      const int c = b & 1, nx = c ^ 1;
      uint32_t* const cnt_sh = a.counts + cnt_shadow(c);
      uint32_t* const fetch_sh = a.counts + cnt_fetch_sh(c);
      k_extend<kRing, false, kVol, false, kQuant, kWide>(sc, cam, a, a.s[c], cnt_stream[c], cnt_stream[nx], cnt_sh, fetch_sh,
                                                         fetch_ext, s0);
      k_shade<false, kEnvIS, kShade, false>(sc, cam, a, a.s[c], cnt_stream[c], a.s[nx], cnt_stream[nx], cnt_sh, s0, uint32_t(b));
      if (sc.num_lights > 0) {
        k_shadow<kRing, false, kVol, kEnvIS, kQuant, kWide>(sc, a, cnt_sh, fetch_sh, a.counts + cnt_fetch_sh(nx));
        k_nee_apply<kEnvIS>(a, cnt_sh);
      }
      if (sc.num_lights == 0 && tail_after >= 0 && b == tail_after && b + 1 < max_depth) {
        k_tail<kRing, kVol, kShade, kQuant, kWide>(sc, cam, a, a.s[nx], cnt_stream[nx], fetch_ext);
        break;
      }
    }
    k_accum(a, sb);
  }
  k_finalize(a, out, accumulate);
}

// n rays (2 float4 each: rt_path_ray) through the flattened scene E: spp
// samples from sample_offset in batches of spb to depth max_depth; out: n * 3
// sums.  Returns the kernels' error flag.
inline int render(const emu::EmuScene& E, const DCamera& cam, const float4* rays, uint32_t n, uint32_t seed,
                  uint32_t sample_offset, uint32_t spp, uint32_t spb, int max_depth, int accumulate, std::vector<float>& out,
                  std::vector<uint32_t>& stream_counts) {
  const DScene& d = E.d;
  const size_t S = size_t(spb) * n;
  // exactly-sized buffers, one allocation per array, as wave_run::render
  const bool lit = d.num_lights > 0;
  const int spill_cap = spill_cap_for(int(d.stack_needed), kRing);
  std::vector<std::vector<float4>> f4(slot_f4(lit), std::vector<float4>(S, float4{0.0f, 0.0f, 0.0f, 0.0f}));
  std::vector<uint32_t> q(CNT_WORDS_Q, 0u), sj_info(lit ? S : 0, 0u), sj_vis(lit ? S : 0, 0u);
  std::vector<uint32_t> pixels(n);
  for (uint32_t i = 0; i < n; ++i) pixels[i] = i;   // the identity list of a range (api.cpp)
  std::vector<uint32_t> spill(size_t(spill_cap), 0u), spill_sh(size_t(spill_cap), 0u);
  std::vector<double> acc(size_t(n) * 3, 0.0);
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
  a.npix = n;
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
  a.out_pixels = n;

  // exactly n rays: a read past the array is the sanitizer's to find
  const std::vector<float4> ray_copy(rays, rays + 2 * size_t(n));
  RaySource src{};
  src.rays = ray_copy.data();
  src.num_rays = n;
  if (!accumulate) out.assign(size_t(n) * 3, 0.0f);
  const WaveVariant v = pick_variant(d);
  with_traversal(v, [&](auto V, auto Q, auto W) {
    with_shading(v, [&](auto H, auto F) {
      run<decltype(V)::value, decltype(H)::value, decltype(F)::value, decltype(Q)::value, decltype(W)::value>(
          d, cam, a, src, spp, spb, max_depth, out.data(), sample_offset, accumulate, stream_counts);
    });
  });
  return err;
}

}  // namespace ray_run

static_assert(rsrc::state0(5) == 0x80000005u, "k_ray_source's state word");

#ifndef RAY_COLOR_EMU_MAIN
// The library form.  rays: n rt_path_ray (8 words each).  The camera gives
// background, sky, phantom and its max_depth (the phantom test's depth) only.
// stream_count (may be null): the first batch's stream length.  Returns 0,
// load_desc's code, or 6 when a kernel flagged an internal error.
extern "C" int ray_color_emu_run(const rt_scene_desc* desc, const rt_camera_desc* cam, int node_format, int volumes_in_bvh,
                                 uint32_t seed, uint32_t sample_offset, int spp, int spb, int depth, const float* rays, int n,
                                 float* out, uint32_t* stream_count) {
  emu::EmuScene E;
  FlattenOptions fo;
  fo.quant_nodes = node_format;
  fo.lift_volumes = volumes_in_bvh ? 0 : 1;
  if (int rc = emu::load_desc(desc, cam, fo, E)) return rc;
  DCamera dc{};   // what api.cpp's ray_color_check fills, nothing else
  for (int a = 0; a < 3; ++a) dc.background[a] = E.cam.background[a];
  dc.use_sky = E.cam.use_sky;
  dc.phantom = E.cam.phantom;
  dc.cam_max_depth = E.cam.cam_max_depth;
  dc.width = dc.height = 1;
  std::vector<float> frame;
  std::vector<uint32_t> counts;
  const int err = ray_run::render(E, dc, reinterpret_cast<const float4*>(rays), uint32_t(n), seed, sample_offset, uint32_t(spp),
                                  uint32_t(spb), depth, 0, frame, counts);
  memcpy(out, frame.data(), frame.size() * sizeof(float));
  if (stream_count) *stream_count = counts.empty() ? 0u : counts[0];
  return err ? 6 : 0;
}

#else
namespace {

int fail(const char* what, int s) {
  printf("{\"ok\": 0, \"failed\": \"%s\", \"sample\": %d}\n", what, s);
  return 7;
}

bool same(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const uint32_t seed = 77u;
  if (rsrc::state0(37) != pack_state(37, 0u, true)) return fail("state word", 0);
  emu::EmuScene E;
  rts_scene_options opt{};
  opt.width = 16;
  opt.aspect = 16.0 / 12.0;
  opt.lucy_rings = 30;
  opt.lucy_cols = 40;
  opt.asset_dir = argv[2];
  char errbuf[512] = {0};
  if (rts_scene_create(argv[1], &opt, &E.scn, errbuf, sizeof errbuf) != 0) { fprintf(stderr, "%s\n", errbuf); return 3; }
  FlattenOptions fo;
  fo.lift_prims = 1;                       // the contexts' default
  fo.lift_volumes = atoi(argv[4]) ? 0 : 1;
  if (int rc = emu::load_desc(rts_scene_get_desc(E.scn), rts_scene_get_camera(E.scn), fo, E)) return rc;
  const int depth = atoi(argv[3]) > 0 ? atoi(argv[3]) : E.max_depth;
  const DCamera& cam = E.cam;
  const uint32_t n = uint32_t(cam.width) * uint32_t(cam.height);
  if (cam.width != 16 || cam.height != 12) return fail("frame size", 0);
  DCamera dc{};                            // background, sky, phantom and depth only: no geometry
  for (int a = 0; a < 3; ++a) dc.background[a] = cam.background[a];
  dc.use_sky = cam.use_sky;
  dc.phantom = cam.phantom;
  dc.cam_max_depth = cam.cam_max_depth;
  dc.width = dc.height = 1;

  auto camera_rays = [&](uint32_t s) {
    std::vector<float4> r(2 * size_t(n));
    for (uint32_t p = 0; p < n; ++p) {
      V3 ro, rd;
      float time;
      get_ray(cam, int(p % uint32_t(cam.width)), int(p / uint32_t(cam.width)), path_key(seed, p, s), ro, rd, time);
      r[2 * p] = make_float4(ro.x, ro.y, ro.z, __uint_as_float(p));
      r[2 * p + 1] = make_float4(rd.x, rd.y, rd.z, __uint_as_float(0u));
    }
    return r;
  };
  int err = 0;
  std::vector<float> got, want;
  std::vector<uint32_t> counts;
  // one sample at a time: the frame of the camera pipeline, byte for byte
  for (uint32_t s = 0; s < 2; ++s) {
    const std::vector<float4> rays = camera_rays(s);
    counts.clear();
    err |= ray_run::render(E, dc, rays.data(), n, seed, s, 1, 1, depth, 0, got, counts);
    err |= wave_run::render(E, seed, s, 1, 1, depth, want, nullptr);
    if (!same(got, want)) return fail("one sample against the camera pipeline", int(s));
    if (counts.size() != 1 || counts[0] != n) return fail("stream count", int(s));
  }
  // a ray has one direction for all its samples, a pixel one per sample: three
  // samples of sample 0's rays are the sum of three one-sample calls (fp64, in
  // sample order, rounded once), in batches of 1 and of 2
  const std::vector<float4> rays = camera_rays(0);
  std::vector<double> sum(size_t(n) * 3, 0.0);
  for (uint32_t s = 0; s < 3; ++s) {
    counts.clear();
    err |= ray_run::render(E, dc, rays.data(), n, seed, s, 1, 1, depth, 0, got, counts);
    for (size_t k = 0; k < sum.size(); ++k) sum[k] += double(got[k]);
  }
  std::vector<float> three(sum.size());
  for (size_t k = 0; k < sum.size(); ++k) three[k] = float(sum[k]);
  for (uint32_t spb = 1; spb <= 3; ++spb) {
    counts.clear();
    err |= ray_run::render(E, dc, rays.data(), n, seed, 0, 3, spb, depth, 0, got, counts);
    if (!same(got, three)) return fail("three samples in batches", int(spb));
    if (counts.size() != (3 + spb - 1) / spb) return fail("batches", int(spb));
  }
  // accumulate: the second call adds double(previous) to its sum
  {
    std::vector<float> acc;
    counts.clear();
    err |= ray_run::render(E, dc, rays.data(), n, seed, 0, 2, 2, depth, 0, acc, counts);
    const std::vector<float> first = acc;
    err |= ray_run::render(E, dc, rays.data(), n, seed, 2, 1, 1, depth, 1, acc, counts);
    std::vector<float> third;
    err |= ray_run::render(E, dc, rays.data(), n, seed, 2, 1, 1, depth, 0, third, counts);
    for (size_t k = 0; k < acc.size(); ++k)
      if (acc[k] != float(double(third[k]) + double(first[k]))) return fail("accumulate", int(k));
  }
  // rays 0, 63, 64 and the last made invalid: zeros there, the others' bytes
  // unchanged, and the stream holds the valid rays only
  {
    std::vector<float4> bad = rays;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const uint32_t where[4] = {0u, 63u, 64u, n - 1u};
    bad[2 * where[0]].y = nan;                                          // origin
    bad[2 * where[1] + 1].x = inf;                                      // direction
    bad[2 * where[2] + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);        // zero direction
    bad[2 * where[3]].z = -inf;
    for (uint32_t spb = 1; spb <= 2; ++spb) {
      counts.clear();
      err |= ray_run::render(E, dc, bad.data(), n, seed, 0, 3, spb, depth, 0, got, counts);
      for (uint32_t p = 0; p < n; ++p) {
        const bool inv = std::find(where, where + 4, p) != where + 4;
        for (int c = 0; c < 3; ++c) {
          const float g = got[3 * p + c], w = inv ? 0.0f : three[3 * p + c];
          if (memcmp(&g, &w, 4) != 0) return fail(inv ? "an invalid ray's output" : "a valid ray beside invalid ones", int(p));
        }
      }
      uint32_t left = 3;
      for (uint32_t c : counts) {
        const uint32_t sb = std::min(spb, left);
        if (c != sb * (n - 4u)) return fail("stream count with invalid rays", int(spb));
        left -= sb;
      }
    }
  }
  double total = 0.0;
  for (float v : three) total += double(v);
  printf("{\"ok\": 1, \"rays\": %u, \"depth\": %d, \"overflow\": %d, \"volumes\": %d, \"vol_refs\": %d, \"lifted\": %d, "
         "\"lights\": %d, \"stack_needed\": %d, \"ring\": %d, \"sum\": %.6g}\n",
         n, depth, err, int(E.d.n_volumes), E.d.num_vol_refs, E.d.num_prim_recs, E.d.num_lights, int(E.d.stack_needed),
         ray_run::kRing, total);
  return err ? 6 : 0;
}
#endif
