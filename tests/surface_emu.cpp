// surface_emu.cpp — test-only: rt_gather_surface's pipeline on the host.  The
// production source kernel (go-raytracing_amd/csrc/ray_source.hip
// k_gather_source<SRC_SURFACE>) and the production surface instantiation of
// k_shade (wavefront.hip, AT_SURFACE), compiled through tests/host_emu (one
// lane per workgroup, one workgroup per launch) and driven like run_batches'
// surface mode: per batch k_set_counts (stream 0 empty), the source kernel,
// then at bounce 0 no k_extend and k_shade<AT_SURFACE>, k_shadow, k_nee_apply,
// and from bounce 1 on the later-bounce kernels; k_accum; k_finalize.  The same
// loop runs the ray mode (k_ray_source, k_extend and k_shade<AT_STREAM> from
// bounce 0 on), which the surface mode is compared with.  The traversal stack
// ring is wave_run's 4 entries.
//
// Two builds:
//   * a plain shared library (surface_emu_run: a caller's scene description
//     and points; tests/test_surface_host.py holds it to tests/surface_ref.py);
//   * -DSURFACE_EMU_MAIN: a stand-alone program under AddressSanitizer + UBSan:
//       surface_emu <node format 0 / 1 / 2>
//     builds path_cases' room with six white walls (and a small white triangle,
//     so that the world quads are lifted), makes the grid camera's 24 x 16 rays
//     with the production get_ray, takes each ray's closest hit from the
//     emulated k_extend and checks, for samples 0 and 1 and depths 1, 2 and 5,
//     that the surface mode on {P, id, n} equals the ray mode on the ray, all
//     bytes, with WaveArgs::early_miss 0 and 3; then sums over batches,
//     accumulate, invalid points and the streams' counts.
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

namespace surf_run {

constexpr int kRing = wave_run::kRing;

// per batch: stream 0 after the source kernel; after bounce 0's k_shade the
// survivors (the next stream's front and back) and the NEE jobs queued
struct Counts {
  std::vector<uint32_t> stream0, survivors, jobs;
  void clear() { stream0.clear(); survivors.clear(); jobs.clear(); }
};

template <bool kVol, bool kEnvIS, int kShade, bool kQuant, bool kWide = false>
void run(const DScene& sc, const DCamera& cam, WaveArgs a, const RaySource& src, uint32_t spp, uint32_t spb, int max_depth,
         float* out, uint32_t sample_offset, int accumulate, Counts& cn) {
  uint32_t* cnt_stream[2] = {a.counts + CNT_STREAM0, a.counts + CNT_STREAM1};
  uint32_t* fetch_ext = a.counts + CNT_FETCH_EXT;
  const bool surface = src.kind == SRC_SURFACE;
  for (double* p = a.acc; p < a.acc + size_t(a.npix) * 3; ++p) *p = 0.0;
  for (uint32_t sa = 0; sa < spp; sa += spb) {
    const uint32_t sb = spp - sa < spb ? spp - sa : spb;
    const uint32_t s0 = sample_offset + sa;
    const uint32_t nslots = sb * a.npix;
    k_set_counts(a.counts, 0u);
    if (surface) k_gather_source<SRC_SURFACE>(a, src, nslots, s0);
    else k_ray_source(a, src, nslots, s0);
    cn.stream0.push_back(a.counts[CNT_STREAM0]);
    for (int b = 0; b < max_depth; ++b) {
      const int c = b & 1, nx = c ^ 1;
      uint32_t* const cnt_sh = a.counts + cnt_shadow(c);
      uint32_t* const fetch_sh = a.counts + cnt_fetch_sh(c);
      if (surface && b == 0) {
        // no k_extend: what it would have zeroed, k_set_counts has
        k_shade<false, kEnvIS, kShade, AT_SURFACE>(sc, cam, a, a.s[c], cnt_stream[c], a.s[nx], cnt_stream[nx], cnt_sh, s0, 0u);
      } else {
        k_extend<kRing, false, kVol, false, kQuant, kWide>(sc, cam, a, a.s[c], cnt_stream[c], cnt_stream[nx], cnt_sh, fetch_sh,
                                                           fetch_ext, s0);
        k_shade<false, kEnvIS, kShade, AT_STREAM>(sc, cam, a, a.s[c], cnt_stream[c], a.s[nx], cnt_stream[nx], cnt_sh, s0,
                                                  uint32_t(b));
      }
      if (b == 0) {
        cn.survivors.push_back(*cnt_stream[nx] + ((a.early_miss & EARLY_NEXT) ? a.counts[cnt_back(1u)] : 0u));
        cn.jobs.push_back(*cnt_sh);
      }
      if (sc.num_lights > 0) {
        k_shadow<kRing, false, kVol, kEnvIS, kQuant, kWide>(sc, a, cnt_sh, fetch_sh, a.counts + cnt_fetch_sh(nx));
        k_nee_apply<kEnvIS>(a, cnt_sh);
      }
    }
    k_accum(a, sb);
  }
  k_finalize(a, out, accumulate);
}

// n records (2 float4 each) under `kind` (SRC_CALLER or SRC_SURFACE) through
// the flattened scene E: spp samples from sample_offset in batches of spb to
// depth max_depth; out: n * 3 sums.  early: WaveArgs::early_miss.  Returns the
// kernels' error flag.
int render(const emu::EmuScene& E, const DCamera& cam, int kind, const std::vector<float4>& recs, uint32_t seed,
           uint32_t sample_offset, uint32_t spp, uint32_t spb, int max_depth, int accumulate, uint32_t early,
           std::vector<float>& out, Counts& cn) {
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
  a.early_miss = early_miss_eligible(d) ? early : 0u;

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
          d, cam, a, src, spp, spb, max_depth, out.data(), sample_offset, accumulate, cn);
    });
  });
  return err;
}

// what api.cpp's ray_color_check fills of the camera, nothing else
DCamera path_camera(const DCamera& cam) {
  DCamera dc{};
  for (int a = 0; a < 3; ++a) dc.background[a] = cam.background[a];
  dc.use_sky = cam.use_sky;
  dc.phantom = cam.phantom;
  dc.cam_max_depth = cam.cam_max_depth;
  dc.width = dc.height = 1;
  return dc;
}

}  // namespace surf_run

#ifndef SURFACE_EMU_MAIN
// The library form.  pts: n rt_gather_point (8 words each).  The camera gives
// background, sky, phantom and its max_depth only.  stream_count (may be null):
// the first batch's stream length.  Returns 0, load_desc's code, or 6 when a
// kernel flagged an internal error.
extern "C" int surface_emu_run(const rt_scene_desc* desc, const rt_camera_desc* cam, int node_format, int volumes_in_bvh,
                               uint32_t seed, uint32_t sample_offset, int spp, int spb, int depth, const float* pts, int n,
                               float* out, uint32_t* stream_count) {
  emu::EmuScene E;
  FlattenOptions fo;
  fo.quant_nodes = node_format;
  fo.lift_volumes = volumes_in_bvh ? 0 : 1;
  if (int rc = emu::load_desc(desc, cam, fo, E)) return rc;
  const DCamera dc = surf_run::path_camera(E.cam);
  const float4* p4 = reinterpret_cast<const float4*>(pts);
  const std::vector<float4> recs(p4, p4 + 2 * size_t(n));
  std::vector<float> sums;
  surf_run::Counts cn;
  const int err = surf_run::render(E, dc, SRC_SURFACE, recs, seed, sample_offset, uint32_t(spp), uint32_t(spb), depth, 0, 0u,
                                   sums, cn);
  memcpy(out, sums.data(), sums.size() * sizeof(float));
  if (stream_count) *stream_count = cn.stream0.empty() ? 0u : cn.stream0[0];
  return err ? 6 : 0;
}

#else
namespace {

int fail(const char* what, int a, int b) {
  printf("{\"ok\": 0, \"failed\": \"%s\", \"at\": [%d, %d]}\n", what, a, b);
  return 7;
}

bool same(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

// tests/scene_builder.py's quad and triangle records
rt_hittable quad(const double Q[3], const double u[3], const double v[3], int mat) {
  rt_hittable h{};
  h.kind = RT_QUAD;
  h.material = mat;
  const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2], ln = std::sqrt(nn);
  double D = 0.0;
  for (int a = 0; a < 3; ++a) {
    h.p[a] = Q[a]; h.p[3 + a] = u[a]; h.p[6 + a] = v[a]; h.p[9 + a] = n[a] / nn; h.p[12 + a] = n[a] / ln;
    D += n[a] / ln * Q[a];
    const double c[4] = {Q[a], Q[a] + u[a], Q[a] + v[a], Q[a] + u[a] + v[a]};
    h.bbox[2 * a] = *std::min_element(c, c + 4);
    h.bbox[2 * a + 1] = *std::max_element(c, c + 4);
    if (h.bbox[2 * a + 1] - h.bbox[2 * a] < 1e-4) { h.bbox[2 * a] -= 1e-4; h.bbox[2 * a + 1] += 1e-4; }
  }
  h.p[15] = D;
  return h;
}

rt_hittable triangle(const double A[3], const double B[3], const double Cc[3], int mat) {
  rt_hittable h{};
  h.kind = RT_TRIANGLE;
  h.material = mat;
  const double e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, e2[3] = {Cc[0] - A[0], Cc[1] - A[1], Cc[2] - A[2]};
  const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const double ln = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  for (int a = 0; a < 3; ++a) {
    h.p[a] = A[a]; h.p[3 + a] = B[a]; h.p[6 + a] = Cc[a]; h.p[9 + a] = n[a] / ln;
    h.bbox[2 * a] = std::min(A[a], std::min(B[a], Cc[a]));
    h.bbox[2 * a + 1] = std::max(A[a], std::max(B[a], Cc[a]));
    if (h.bbox[2 * a + 1] - h.bbox[2 * a] < 1e-4) { h.bbox[2 * a] -= 1e-4; h.bbox[2 * a + 1] += 1e-4; }
  }
  return h;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const uint32_t seed = 3u;                 // path_cases.SEED
  constexpr int W = 24, H = 16, kWalls = 6;
  // path_cases._room with white walls: six walls, the lamp, the blocker, and a
  // small triangle that keeps the world BVH from being empty of everything
  // but quads (flatten.cpp lifts the world quads only then)
  rt_texture tex[2] = {};
  tex[0].kind = RT_TEX_SOLID; tex[0].even = tex[0].odd = -1;
  tex[1] = tex[0];
  for (int a = 0; a < 3; ++a) tex[0].albedo[a] = 1.0;
  tex[1].albedo[0] = 12.0; tex[1].albedo[1] = 10.0; tex[1].albedo[2] = 8.0;
  rt_material mats[2] = {};
  mats[0].kind = RT_LAMBERTIAN; mats[0].texture = 0;
  mats[1].kind = RT_DIFFUSE_LIGHT; mats[1].texture = 1;
  const double Q[8][9] = {{-2.5, -2, -4, 5, 0, 0, 0, 4, 0},      {-2.5, -1.5, 1.5, 5, 0, 0, 0, 0, -6},
                          {-2.5, 1.5, -4.5, 5, 0, 0, 0, 0, 6},   {-2, -2, -4.5, 0, 0, 6, 0, 4, 0},
                          {2, -2, 1.5, 0, 0, -6, 0, 4, 0},       {2.5, -2, 1, -5, 0, 0, 0, 4, 0},
                          {-0.5, 1.45, -2.5, 1, 0, 0, 0, 0, 1},  {-1.7, 0.4, -3.2, 1.5, 0, 0, 0, 0, 1.6}};
  std::vector<rt_hittable> hs;
  for (int k = 0; k < 8; ++k) hs.push_back(quad(Q[k], Q[k] + 3, Q[k] + 6, k == 6 ? 1 : 0));
  const double ta[3] = {1.55, -1.4, -2.9}, tb[3] = {1.75, -1.4, -2.9}, tc[3] = {1.65, -1.25, -2.9};
  hs.push_back(triangle(ta, tb, tc, 0));
  std::vector<int32_t> children;
  for (int k = 0; k < 9; ++k) children.push_back(k);
  rt_hittable world{};
  world.kind = RT_LIST;
  world.material = -1;
  world.a = 0;
  world.b = 9;
  for (int a = 0; a < 3; ++a) {
    world.bbox[2 * a] = 1e30; world.bbox[2 * a + 1] = -1e30;
    for (int k = 0; k < 9; ++k) {
      world.bbox[2 * a] = std::min(world.bbox[2 * a], hs[size_t(k)].bbox[2 * a]);
      world.bbox[2 * a + 1] = std::max(world.bbox[2 * a + 1], hs[size_t(k)].bbox[2 * a + 1]);
    }
  }
  hs.push_back(world);
  const int32_t lights[1] = {6};
  rt_scene_desc desc{};
  desc.hittables = hs.data(); desc.num_hittables = int32_t(hs.size());
  desc.children = children.data(); desc.num_children = int32_t(children.size());
  desc.root = 9;
  desc.materials = mats; desc.num_materials = 2;
  desc.textures = tex; desc.num_textures = 2;
  desc.lights = lights; desc.num_lights = 1;
  rt_camera_desc cd{};                        // shade_cases.grid_camera: a pinhole at the origin along -z
  cd.image_width = W; cd.image_height = H; cd.samples_per_pixel = 1; cd.max_depth = 6;
  cd.pixel00[0] = -1.15; cd.pixel00[1] = 0.75; cd.pixel00[2] = -1.0;
  cd.pixel_delta_u[0] = 0.1;
  cd.pixel_delta_v[1] = -0.1;

  emu::EmuScene E;
  FlattenOptions fo;
  fo.lift_prims = 1;                          // the contexts' default
  fo.quant_nodes = atoi(argv[1]);
  if (int rc = emu::load_desc(&desc, &cd, fo, E)) return rc;
  if (E.d.num_prim_recs <= 0 || !early_miss_eligible(E.d)) return fail("the walls are lifted", E.d.num_prim_recs, 0);
  const DCamera& cam = E.cam;
  const DCamera dc = surf_run::path_camera(cam);
  const uint32_t n = uint32_t(W * H);

  int err = 0;
  double total = 0.0;
  uint32_t compared = 0, rays_seen = 0;
  std::vector<float> got, want;
  surf_run::Counts cg, cw;
  std::vector<float4> pts0;                    // sample 0's points, for the sums below
  emu::TraceArgs T(6, int(E.d.stack_needed));
  for (uint32_t s = 0; s < 2; ++s) {
    std::vector<float4> rays, pts;
    for (uint32_t p = 0; p < n; ++p) {
      V3 ro, rd;
      float time;
      const uint32_t key = path_key(seed, p, s);
      get_ray(cam, int(p % uint32_t(W)), int(p / uint32_t(W)), key, ro, rd, time);
      const float o[3] = {ro.x, ro.y, ro.z}, d[3] = {rd.x, rd.y, rd.z};
      const emu::Hit h = emu::closest(E, T, o, d, key, 0u);
      int32_t top, prim;
      float t;
      emu::hit_ids(E.d, h, top, prim, t);
      ++rays_seen;
      if (top < 0 || top >= kWalls) continue;    // a lamp, the blocker, the triangle, a miss
      const V3 P = add(ro, scale(rd, t));        // make_record's point
      const rt_hittable& w = hs[size_t(top)];
      V3 nrm = mk(float(w.p[12]), float(w.p[13]), float(w.p[14]));
      if (!(dot(rd, nrm) < 0.0f)) nrm = neg(nrm);   // set_face
      rays.push_back(make_float4(ro.x, ro.y, ro.z, __uint_as_float(p)));
      rays.push_back(make_float4(rd.x, rd.y, rd.z, __uint_as_float(0u)));
      pts.push_back(make_float4(P.x, P.y, P.z, __uint_as_float(p)));
      pts.push_back(make_float4(nrm.x, nrm.y, nrm.z, __uint_as_float(0u)));
    }
    const uint32_t m = uint32_t(pts.size() / 2);
    compared += m;
    if (s == 0) pts0 = pts;
    for (int depth : {1, 2, 5}) {
      for (uint32_t early : {0u, uint32_t(EARLY_NEE | EARLY_NEXT)}) {
        cg.clear(); cw.clear();
        err |= surf_run::render(E, dc, SRC_CALLER, rays, seed, s, 1, 1, depth, 0, early, want, cw);
        err |= surf_run::render(E, dc, SRC_SURFACE, pts, seed, s, 1, 1, depth, 0, early, got, cg);
        if (!same(got, want)) return fail("the surface mode against the ray mode", int(s), depth * 10 + int(early));
        // dense streams: every valid point is in stream 0, and bounce 0 leaves the ray mode's survivors and jobs
        if (cg.stream0.size() != 1 || cg.stream0[0] != m || cw.stream0[0] != m) return fail("stream 0", int(s), depth);
        if (cg.survivors != cw.survivors || cg.jobs != cw.jobs) return fail("survivors and jobs of bounce 0", int(s), depth);
        if (cg.survivors[0] != (depth > 1 ? m : 0u) || cg.jobs[0] > m || (early == 0u && cg.jobs[0] == 0u))
          return fail("bounce 0's counts", int(cg.survivors[0]), int(cg.jobs[0]));
        for (float v : got) total += double(v);
      }
    }
  }
  if (4u * compared < 3u * rays_seen) return fail("three quarters of the rays are compared", int(compared), int(rays_seen));

  // three samples are the sum of three one-sample calls (fp64, in sample
  // order, rounded once), in batches of 1, 2 and 3; accumulate
  const std::vector<float4>& pts = pts0;
  const uint32_t m = uint32_t(pts.size() / 2);
  const int depth = 5;
  std::vector<double> sum(size_t(m) * 3, 0.0);
  for (uint32_t s = 0; s < 3; ++s) {
    cg.clear();
    err |= surf_run::render(E, dc, SRC_SURFACE, pts, seed, s, 1, 1, depth, 0, 0u, got, cg);
    for (size_t k = 0; k < sum.size(); ++k) sum[k] += double(got[k]);
  }
  std::vector<float> three(sum.size());
  for (size_t k = 0; k < sum.size(); ++k) three[k] = float(sum[k]);
  for (uint32_t spb = 1; spb <= 3; ++spb) {
    cg.clear();
    err |= surf_run::render(E, dc, SRC_SURFACE, pts, seed, 0, 3, spb, depth, 0, 0u, got, cg);
    if (!same(got, three)) return fail("three samples in batches", int(spb), 0);
    if (cg.stream0.size() != (3 + spb - 1) / spb) return fail("batches", int(spb), 0);
  }
  {
    std::vector<float> acc, third;
    err |= surf_run::render(E, dc, SRC_SURFACE, pts, seed, 0, 2, 2, depth, 0, 0u, acc, cg);
    const std::vector<float> first = acc;
    err |= surf_run::render(E, dc, SRC_SURFACE, pts, seed, 2, 1, 1, depth, 1, 0u, acc, cg);
    err |= surf_run::render(E, dc, SRC_SURFACE, pts, seed, 2, 1, 1, depth, 0, 0u, third, cg);
    for (size_t k = 0; k < acc.size(); ++k)
      if (acc[k] != float(double(third[k]) + double(first[k]))) return fail("accumulate", int(k), 0);
  }
  // points 0, 63, 64 and the last made invalid: NaN p, inf p, zero n, and a
  // normal whose fp32 length is 0
  {
    std::vector<float4> bad = pts;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const uint32_t where[4] = {0u, 63u, 64u, m - 1u};
    bad[2 * where[0]].y = nan;
    bad[2 * where[1]].x = inf;
    bad[2 * where[2] + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bad[2 * where[3] + 1] = make_float4(1e-30f, 0.0f, 0.0f, 0.0f);
    cg.clear();
    err |= surf_run::render(E, dc, SRC_SURFACE, bad, seed, 0, 3, 2, depth, 0, 0u, got, cg);
    for (uint32_t p = 0; p < m; ++p) {
      const bool inv = std::find(where, where + 4, p) != where + 4;
      for (int c = 0; c < 3; ++c) {
        const float g = got[3 * p + c], w = inv ? 0.0f : three[3 * p + c];
        if (memcmp(&g, &w, 4) != 0) return fail(inv ? "an invalid point's output" : "a valid point beside invalid ones", int(p), c);
      }
    }
    if (cg.stream0.size() != 2 || cg.stream0[0] != 2u * (m - 4u) || cg.stream0[1] != m - 4u)
      return fail("stream count with invalid points", int(cg.stream0[0]), int(cg.stream0[1]));
    if (cg.survivors[0] != 2u * (m - 4u) || cg.jobs[0] > 2u * (m - 4u)) return fail("queues with invalid points", 0, 0);
  }
  // a normal that is not unit is the same vertex
  {
    std::vector<float4> big = pts;
    for (uint32_t p = 0; p < m; ++p) { big[2 * p + 1].x *= 4.0f; big[2 * p + 1].y *= 4.0f; big[2 * p + 1].z *= 4.0f; }
    err |= surf_run::render(E, dc, SRC_SURFACE, big, seed, 0, 3, 3, depth, 0, 0u, got, cg);
    if (!same(got, three)) return fail("a scaled normal", 0, 0);
  }
  printf("{\"ok\": 1, \"rays\": %u, \"compared\": %u, \"overflow\": %d, \"lifted\": %d, \"lights\": %d, \"format\": %d, "
         "\"ring\": %d, \"sum\": %.6g}\n",
         rays_seen, compared, err, E.d.num_prim_recs, E.d.num_lights, fo.quant_nodes, surf_run::kRing, total);
  return err ? 6 : 0;
}
#endif
