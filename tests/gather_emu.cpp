// gather_emu.cpp — test-only: rt_gather's pipeline on the host.  The production
// ray sources (go-raytracing_amd/csrc/ray_source.hip: k_gather_source<kind>,
// k_ray_source and the probe kernel k_gather_rays) and the production
// later-bounce kernels of wavefront.hip, compiled through tests/host_emu (one
// lane per workgroup, one workgroup per launch) and driven like run_batches'
// ray mode, with exactly-sized buffers and wave_run's 4-entry traversal ring.
// Its batch loop is tests/ray_color_emu.cpp's with the source kernel chosen by
// kind.  A stand-alone program, built under AddressSanitizer + UBSan
// (tests/test_gather_host.py):
//
//   gather_emu probe <points.bin> <seed> <samples> <out.bin>
//     points.bin: rt_gather_point records.  out.bin: for source 0, 1, 2 and
//     sample 0 .. samples-1 in turn, the rt_path_ray of every point
//     (k_gather_rays), for the numpy restatement to compare with.
//
//   gather_emu <scene> <asset_dir> <depth, 0 = the scene's> <volumes_in_bvh>
//     16 x 12 points in front of the first hits of the scene's camera rays,
//     with normals that are not unit, and per source: the one-sample gather
//     against the ray mode on the probe's rays; sums over batches and
//     accumulate; invalid points.
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
#include "emu_trace.h"
#include "wave_run.h"

using namespace rtg;

namespace gather_run {

constexpr int kRing = wave_run::kRing;

void source(int kind, const WaveArgs& a, const RaySource& src, uint32_t nslots, uint32_t s0) {
  switch (kind) {
    case SRC_CALLER: k_ray_source(a, src, nslots, s0); break;
    case SRC_RAY: k_gather_source<SRC_RAY>(a, src, nslots, s0); break;
    case SRC_COSINE: k_gather_source<SRC_COSINE>(a, src, nslots, s0); break;
    default: k_gather_source<SRC_SPHERE>(a, src, nslots, s0); break;
  }
}

// stream_counts: counts[CNT_STREAM0] after each batch's source kernel
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
    source(src.kind, a, src, nslots, s0);
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

// n records (2 float4 each) under `kind` through the flattened scene E: spp
// samples from sample_offset in batches of spb to depth max_depth; out: n * 3
// sums.  Returns the kernels' error flag.
int render(const emu::EmuScene& E, const DCamera& cam, int kind, const std::vector<float4>& recs, uint32_t seed,
           uint32_t sample_offset, uint32_t spp, uint32_t spb, int max_depth, int accumulate, std::vector<float>& out,
           std::vector<uint32_t>& stream_counts) {
  const DScene& d = E.d;
  const uint32_t n = uint32_t(recs.size() / 2);
  const size_t S = size_t(spb) * n;
  const bool lit = d.num_lights > 0;
  const int spill_cap = spill_cap_for(int(d.stack_needed), kRing);
  std::vector<std::vector<float4>> f4(slot_f4(lit), std::vector<float4>(S, float4{0.0f, 0.0f, 0.0f, 0.0f}));
  std::vector<uint32_t> q(CNT_WORDS_Q, 0u), sj_info(lit ? S : 0, 0u), sj_vis(lit ? S : 0, 0u);
  std::vector<uint32_t> pixels(n);
  for (uint32_t i = 0; i < n; ++i) pixels[i] = i;
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

  const std::vector<float4> copy(recs);   // exactly n records: a read past the array is the sanitizer's to find
  RaySource src{};
  src.rays = copy.data();
  src.num_rays = n;
  src.kind = kind;
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

// k_gather_rays over exactly-sized copies
std::vector<float4> probe(const std::vector<float4>& pts, int kind, uint32_t seed, uint32_t sample) {
  const std::vector<float4> copy(pts);
  std::vector<float4> out(pts.size(), float4{-1.0f, -1.0f, -1.0f, -1.0f});
  k_gather_rays(copy.data(), uint32_t(pts.size() / 2), kind, seed, sample, out.data());
  return out;
}

}  // namespace gather_run

namespace {

int fail(const char* what, int kind, int s) {
  printf("{\"ok\": 0, \"failed\": \"%s\", \"kind\": %d, \"at\": %d}\n", what, kind, s);
  return 7;
}

bool same(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

int probe_main(int argc, char** argv) {
  if (argc < 6) return 2;
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 3;
  std::vector<float4> pts;
  float4 rec;
  while (fread(&rec, sizeof rec, 1, f) == 1) pts.push_back(rec);
  fclose(f);
  if (pts.empty() || pts.size() % 2) return 4;
  const uint32_t seed = uint32_t(strtoul(argv[3], nullptr, 10));
  const int samples = atoi(argv[4]);
  f = fopen(argv[5], "wb");
  if (!f) return 3;
  for (int kind = SRC_RAY; kind <= SRC_SPHERE; ++kind)
    for (int s = 0; s < samples; ++s) {
      const std::vector<float4> r = gather_run::probe(pts, kind, seed, uint32_t(s));
      if (fwrite(r.data(), sizeof(float4), r.size(), f) != r.size()) return 5;
    }
  fclose(f);
  printf("{\"ok\": 1, \"points\": %zu, \"samples\": %d}\n", pts.size() / 2, samples);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && strcmp(argv[1], "probe") == 0) return probe_main(argc, argv);
  if (argc < 5) return 2;
  const uint32_t seed = 77u;
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
  if (cam.width != 16 || cam.height != 12) return fail("frame size", 0, 0);
  DCamera dc{};                            // background, sky, phantom and depth only: no geometry
  for (int a = 0; a < 3; ++a) dc.background[a] = cam.background[a];
  dc.use_sky = cam.use_sky;
  dc.phantom = cam.phantom;
  dc.cam_max_depth = cam.cam_max_depth;
  dc.width = dc.height = 1;

  // The points: a little in front of what each camera ray of sample 0 hits (a
  // miss: one unit along the ray), looking back along the ray with a normal of
  // length 0.5 .. 3.5; ids that are not the index.
  std::vector<float4> pts(2 * size_t(n));
  {
    emu::TraceArgs T(E.max_depth, int(E.d.stack_needed));
    for (uint32_t p = 0; p < n; ++p) {
      V3 ro, rd;
      float time;
      const uint32_t key = path_key(seed, p, 0u);
      get_ray(cam, int(p % uint32_t(cam.width)), int(p / uint32_t(cam.width)), key, ro, rd, time);
      const float o[3] = {ro.x, ro.y, ro.z}, d[3] = {rd.x, rd.y, rd.z};
      const emu::Hit h = emu::closest(E, T, o, d, key, 0u);
      const float t = h.kh != 0u && std::isfinite(h.t) ? 0.98f * h.t : 1.0f;
      const float s = -(0.5f + 0.25f * float(p % 13u)) / len(rd);
      pts[2 * p] = make_float4(ro.x + t * rd.x, ro.y + t * rd.y, ro.z + t * rd.z, __uint_as_float(p * 7u + 3u));
      pts[2 * p + 1] = make_float4(s * rd.x, s * rd.y, s * rd.z, __uint_as_float(0u));
    }
  }

  int err = 0;
  double total = 0.0;
  std::vector<float> got, want;
  std::vector<uint32_t> counts;
  for (int kind = SRC_RAY; kind <= SRC_SPHERE; ++kind) {
    // one sample: the gather is the ray mode on the probe's rays, byte for byte
    for (uint32_t s = 0; s < 2; ++s) {
      const std::vector<float4> rays = gather_run::probe(pts, kind, seed, s);
      if (kind == SRC_RAY && memcmp(rays.data(), pts.data(), pts.size() * sizeof(float4)) != 0)
        return fail("the RAY probe is the points", kind, int(s));
      counts.clear();
      err |= gather_run::render(E, dc, SRC_CALLER, rays, seed, s, 1, 1, depth, 0, want, counts);
      err |= gather_run::render(E, dc, kind, pts, seed, s, 1, 1, depth, 0, got, counts);
      if (!same(got, want)) return fail("one sample against the ray mode", kind, int(s));
      if (counts.size() != 2 || counts[0] != n || counts[1] != n) return fail("stream count", kind, int(s));
    }
    // three samples are the sum of three one-sample calls (fp64, in sample
    // order, rounded once), in batches of 1, 2 and 3
    std::vector<double> sum(size_t(n) * 3, 0.0);
    for (uint32_t s = 0; s < 3; ++s) {
      err |= gather_run::render(E, dc, kind, pts, seed, s, 1, 1, depth, 0, got, counts);
      for (size_t k = 0; k < sum.size(); ++k) sum[k] += double(got[k]);
    }
    std::vector<float> three(sum.size());
    for (size_t k = 0; k < sum.size(); ++k) three[k] = float(sum[k]);
    for (float v : three) total += double(v);
    if (kind == SRC_COSINE) {
      for (uint32_t spb = 1; spb <= 3; ++spb) {
        counts.clear();
        err |= gather_run::render(E, dc, kind, pts, seed, 0, 3, spb, depth, 0, got, counts);
        if (!same(got, three)) return fail("three samples in batches", kind, int(spb));
        if (counts.size() != (3 + spb - 1) / spb) return fail("batches", kind, int(spb));
      }
      // accumulate: the second call adds double(previous) to its sum
      std::vector<float> acc, third;
      err |= gather_run::render(E, dc, kind, pts, seed, 0, 2, 2, depth, 0, acc, counts);
      const std::vector<float> first = acc;
      err |= gather_run::render(E, dc, kind, pts, seed, 2, 1, 1, depth, 1, acc, counts);
      err |= gather_run::render(E, dc, kind, pts, seed, 2, 1, 1, depth, 0, third, counts);
      for (size_t k = 0; k < acc.size(); ++k)
        if (acc[k] != float(double(third[k]) + double(first[k]))) return fail("accumulate", kind, int(k));
    }
    // points 0, 63, 64 and the last made invalid: NaN p, inf p, zero n, and a
    // normal whose fp32 length is 0.  SPHERE does not read n.
    {
      std::vector<float4> bad = pts;
      const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
      const uint32_t where[4] = {0u, 63u, 64u, n - 1u};
      bad[2 * where[0]].y = nan;
      bad[2 * where[1]].x = inf;
      bad[2 * where[2] + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      bad[2 * where[3] + 1] = make_float4(1e-30f, 0.0f, 0.0f, 0.0f);
      const uint32_t ninv = kind == SRC_SPHERE ? 2u : 4u;
      counts.clear();
      err |= gather_run::render(E, dc, kind, bad, seed, 0, 3, 2, depth, 0, got, counts);
      for (uint32_t p = 0; p < n; ++p) {
        const bool inv = std::find(where, where + ninv, p) != where + ninv;
        for (int c = 0; c < 3; ++c) {
          const float g = got[3 * p + c], w = inv ? 0.0f : three[3 * p + c];
          if (memcmp(&g, &w, 4) != 0) return fail(inv ? "an invalid point's output" : "a valid point beside invalid ones", kind, int(p));
        }
      }
      if (counts.size() != 2 || counts[0] != 2u * (n - ninv) || counts[1] != n - ninv)
        return fail("stream count with invalid points", kind, 0);
      // the probe marks the same points, and the ray mode leaves them out too
      const std::vector<float4> rays = gather_run::probe(bad, kind, seed, 0u);
      for (uint32_t p = 0; p < n; ++p) {
        const bool inv = std::find(where, where + ninv, p) != where + ninv;
        const float4 d = rays[2 * p + 1];
        if (inv != (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f)) return fail("the probe's mark", kind, int(p));
        if (memcmp(&rays[2 * p], &bad[2 * p], sizeof(float4)) != 0) return fail("the probe's origin", kind, int(p));
      }
    }
  }
  printf("{\"ok\": 1, \"points\": %u, \"depth\": %d, \"overflow\": %d, \"volumes\": %d, \"vol_refs\": %d, \"lifted\": %d, "
         "\"lights\": %d, \"stack_needed\": %d, \"ring\": %d, \"sum\": %.6g}\n",
         n, depth, err, int(E.d.n_volumes), E.d.num_vol_refs, E.d.num_prim_recs, E.d.num_lights, int(E.d.stack_needed),
         gather_run::kRing, total);
  return err ? 6 : 0;
}
