// hits_emu.cpp — test-only: the production closest-hit kernel (wavefront.hip
// k_extend, a later bounce: rays read from the path stream) compiled for the
// host, one lane, over a caller's scene description and given rays.  A plain
// shared library (no sanitizer, nothing to preload) that tests load with
// ctypes next to the oracle (tests/test_scale_host.py).  Like
// tests/ray_emu.cpp, but the scene is an rt_scene_desc, the flatten options
// are the caller's, and the hit record is mapped to hittable ids the way
// probe.hip's path_hits_kernel maps it (rt_primary_hits' conventions: top,
// prim = -1 and t = -1 for a miss).  hits_emu_run takes rays without a path
// (no RNG key: scenes whose hits draw random numbers, volumes, are refused);
// hits_emu_run_paths takes a path's rays with their pixel and bounce and
// runs volume scenes too, in either placement (tests/test_volume_host.py),
// and hits_emu_placement reports where the flattener put the volumes;
// hits_emu_shade follows the closest hit with the production shade_path and
// returns what it decides (tests/test_shade_kat.py); hits_emu_render runs the
// whole wavefront pipeline (wave_run.h) over the description and returns the
// frame (tests/test_path_kat.py), hits_emu_render_opts the same with the
// world-BVH builder named and the node format taken reported
// (tests/test_xform_kat.py).  Not a product path.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../go-raytracing_amd/csrc/wavefront.hip"
#include "../go-raytracing_amd/csrc/wave_layout.h"
#include "emu_scene.h"
#include "emu_trace.h"
#include "wave_run.h"

using namespace rtg;

// Closest hits of n rays (o, d: n * 3 floats each) in the scene `desc`,
// flattened with the given world-BVH builder, mesh builder (BLAS_REFERENCE /
// BLAS_SAH) and node format (0 fp32, 1 quant8, 2 wide8; *format_used: what the
// scene took, as rt_scene_info.node_format reports it).  Returns 0, or: 3 the
// scene needs the rare-primitive kernels, 4 flatten failed, 6 a kernel
// flagged an internal error.
extern "C" int hits_emu_run(const rt_scene_desc* desc, const rt_camera_desc* cam, int tlas_builder, int blas_builder,
                            int node_format, const float* o, const float* d, int n, int32_t* top, int32_t* prim,
                            float* t, int32_t* format_used) {
  emu::EmuScene E;
  FlattenOptions fo;
  fo.tlas_builder = tlas_builder;
  fo.blas_builder = blas_builder;
  fo.quant_nodes = node_format;
  if (int rc = emu::load_desc(desc, cam, fo, E)) return rc;
  const DScene& sc = E.d;
  if (pick_variant(sc).vol || sc.num_vol_refs > 0) {
    fprintf(stderr, "hits_emu: rare-primitive scenes are not supported\n");
    return 3;
  }
  *format_used = sc.wide_nodes ? 2 : sc.quant_nodes ? 1 : 0;
  emu::TraceArgs T(E.max_depth, int(E.d.stack_needed));
  for (int i = 0; i < n; ++i) {
    emu::hit_ids(sc, emu::unpack(emu::trace_path(E, T, o + 3 * i, d + 3 * i)), top[i], prim[i], t[i]);
  }
  return T.err ? 6 : 0;
}

// Where flatten_scene puts the scene's volumes and what the upload derives
// from that (tests/test_volume_host.py).  out[0..7]: num_vol_refs,
// has_volumes, shade_kind, the number of DVolRec records, needs_uv, whether
// the rare-primitive kernels run, the node format used, volumes in all.
// codes[rec * kVolRecQuads + k]: record quad k's axis code (0: a general
// quad, or none); ntests[rec]: the record's test count.  Returns 0, or
// load_desc's code.
extern "C" int hits_emu_placement(const rt_scene_desc* desc, const rt_camera_desc* cam, int lift_volumes, int node_format,
                                  int32_t* out, uint32_t* codes, int32_t* ntests) {
  emu::EmuScene E;
  FlattenOptions fo;
  fo.quant_nodes = node_format;
  fo.lift_volumes = lift_volumes;
  if (int rc = emu::load_desc(desc, cam, fo, E)) return rc;
  const DScene& sc = E.d;
  out[0] = sc.num_vol_refs;
  out[1] = sc.has_volumes;
  out[2] = sc.shade_kind;
  out[3] = int32_t(E.vol_recs.size());
  out[4] = sc.needs_uv;
  out[5] = pick_variant(sc).vol ? 1 : 0;
  out[6] = sc.wide_nodes ? 2 : sc.quant_nodes ? 1 : 0;
  out[7] = int32_t(sc.n_volumes);
  for (int i = 0; i < kVolRecMax * kVolRecQuads; ++i) codes[i] = 0u;
  for (int i = 0; i < kVolRecMax; ++i) ntests[i] = 0;
  for (size_t r = 0; r < E.vol_recs.size() && r < size_t(kVolRecMax); ++r) {
    ntests[r] = E.vol_recs[r].ref.ntests;
    for (int k = 0; k < E.vol_recs[r].nq && k < kVolRecQuads; ++k)
      memcpy(&codes[r * kVolRecQuads + size_t(k)], &E.vol_recs[r].q[k].pad0, 4);
  }
  return 0;
}

// flatten_scene's status for the description (RT_OK or an rt_status), the
// message on stderr: the refusals.
extern "C" int hits_emu_flatten_status(const rt_scene_desc* desc, int lift_volumes) {
  HostScene h;
  std::string err;
  FlattenOptions fo;
  fo.lift_volumes = lift_volumes;
  const int rc = flatten_scene(desc, h, err, fo);
  if (rc) fprintf(stderr, "hits_emu: flatten: %s\n", err.c_str());
  return rc;
}

// Closest hits of n path rays at bounce `bounce` (pix[i]: the path's pixel;
// the RNG key is production's for (seed, pixel, sample)), as the pipeline
// finds them: k_extend in the variant pick_variant names (volumes left in
// the world BVH are tested there), then the lifted volumes' test as k_shade
// and the path probe apply it (lifted_volumes).  Any scene the flattener
// takes.  lift_volumes: RT_VOLUMES_LIFTED (1) or RT_VOLUMES_IN_BVH (0).
// Returns as hits_emu_run.
extern "C" int hits_emu_run_paths(const rt_scene_desc* desc, const rt_camera_desc* cam, int tlas_builder, int node_format,
                                  int lift_volumes, uint32_t seed, uint32_t sample, int bounce, const int32_t* pix,
                                  const float* o, const float* d, int n, int32_t* top, int32_t* prim, float* t,
                                  int32_t* format_used) {
  emu::EmuScene E;
  FlattenOptions fo;
  fo.tlas_builder = tlas_builder;
  fo.quant_nodes = node_format;
  fo.lift_volumes = lift_volumes;
  if (int rc = emu::load_desc(desc, cam, fo, E)) return rc;
  const DScene& sc = E.d;
  *format_used = sc.wide_nodes ? 2 : sc.quant_nodes ? 1 : 0;
  emu::TraceArgs T(E.max_depth, int(E.d.stack_needed));
  for (int i = 0; i < n; ++i) {
    const uint32_t key = path_key(seed, uint32_t(pix[i]), sample);
    emu::hit_ids(sc, emu::closest(E, T, o + 3 * i, d + 3 * i, key, uint32_t(bounce)), top[i], prim[i], t[i]);
  }
  return T.err ? 6 : 0;
}

static void put3(float* dst, int i, const V3& v) { dst[3 * i] = v.x; dst[3 * i + 1] = v.y; dst[3 * i + 2] = v.z; }

// How the flattener hands the environment's texels to the device: 1 RGBE
// words (every texel re-encodes exactly), 0 fp32 texels, -1 no environment;
// or -(10 + load_desc's code).
extern "C" int hits_emu_env_format(const rt_scene_desc* desc, const rt_camera_desc* cam) {
  emu::EmuScene E;
  FlattenOptions fo;
  if (int rc = emu::load_desc(desc, cam, fo, E)) return -(10 + rc);
  if (!E.d.env.valid) return -1;
  return E.d.env.rgbe ? 1 : 0;
}

// One bounce of n paths through the production pipeline's two halves: the
// closest hit as hits_emu_run_paths finds it (k_extend, one lane), then
// shade_path in the variant pick_variant names for the scene (shade kind, the
// importance-sampled HDRI only beside a light, kFirst at bounce 0), with a
// one-slot Lout.  Per path: seed / sample / pix[i] key it, (o, d, beta) are
// its incoming ray and throughput, dleft the depth left, allow whether an
// emitter it hits counts (camera.go:477).  o == NULL (bounce 0 only): the
// camera ray is made by the production get_ray for pixel pix[i] and returned
// in ray (n * 6).  Out: hit (0 miss) and t of the closest hit; cont (a
// scattered ray goes on: P, sd, nbeta); Ladd, the radiance the bounce added
// (beta * miss colour or emission); flags (bit 0 / 1: the area / HDRI shadow
// ray wanted) with ca, da, tmax_a and ch, dh, the NEE contributions and
// directions (tests/test_shade_kat.py).  Returns as hits_emu_run.
extern "C" int hits_emu_shade(const rt_scene_desc* desc, const rt_camera_desc* cam, int node_format, uint32_t seed,
                              uint32_t sample, int bounce, int dleft, int allow, const int32_t* pix, const float* o,
                              const float* d, const float* beta, int n, float* ray, int32_t* hit, float* t, int32_t* cont,
                              float* P, float* sd, float* nbeta, float* Ladd, uint32_t* flags, float* ca, float* da,
                              float* tmax_a, float* ch, float* dh) {
  emu::EmuScene E;
  FlattenOptions fo;
  fo.quant_nodes = node_format;
  if (int rc = emu::load_desc(desc, cam, fo, E)) return rc;
  if (!o && bounce != 0) return 2;
  const DScene& sc = E.d;
  emu::TraceArgs T(E.max_depth, int(E.d.stack_needed));
  for (int i = 0; i < n; ++i) {
    const uint32_t key = path_key(seed, uint32_t(pix[i]), sample);
    V3 ro, rd;
    if (o) {
      ro = mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]);
      rd = mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    } else {
      float time;
      get_ray(E.cam, pix[i] % E.cam.width, pix[i] / E.cam.width, key, ro, rd, time);
    }
    if (ray) { put3(ray, 2 * i, ro); put3(ray, 2 * i + 1, rd); }
    const float fo3[3] = {ro.x, ro.y, ro.z}, fd3[3] = {rd.x, rd.y, rd.z};
    const float4 h = emu::trace_path(E, T, fo3, fd3, key, uint32_t(bounce));
    {   // the hit reported: with the lifted tests applied, as shade_path applies them to its own copy
      emu::Hit m = emu::unpack(h);
      emu::merge_lifted(sc, m, ro, rd, key, uint32_t(bounce));
      hit[i] = m.kh != 0u ? 1 : 0;
      t[i] = m.kh != 0u ? m.t : -1.0f;
    }
    const emu::Shaded r = emu::shade_by_kind(E, T, h, ro, rd, mk(beta[3 * i], beta[3 * i + 1], beta[3 * i + 2]), key, dleft,
                                             uint32_t(bounce), allow != 0);
    cont[i] = r.cont ? 1 : 0;
    flags[i] = r.flags;
    tmax_a[i] = r.tmax_a;
    put3(P, i, r.P); put3(sd, i, r.sd); put3(nbeta, i, r.nbeta); put3(ca, i, r.ca); put3(da, i, r.da);
    put3(ch, i, r.ch); put3(dh, i, r.dh);
    put3(Ladd, i, r.lout_set ? mk(r.L.x, r.L.y, r.L.z) : mk(0.0f, 0.0f, 0.0f));
  }
  return T.err ? 6 : 0;
}

// One frame of the description through the production wavefront pipeline on
// the host (wave_run.h: camera -> extend -> shade -> shadow -> NEE apply ->
// accumulate -> finalize, the kernel variants pick_variant names, one batch):
// spp samples from sample_offset to `depth` (rt_render_params), the camera's
// own max_depth kept for the phantom-HDRI rule.  out: H * W * 3 float sums,
// what rt_render returns.  volumes_in_bvh: RT_OPT_VOLUMES' value,
// RT_VOLUMES_LIFTED (0) or RT_VOLUMES_IN_BVH (1).  Returns 0, load_desc's code, or
// 6 when a kernel flagged an internal error.
// (hits_emu_render_opts: with the world-BVH builder the caller names,
// BLAS_REFERENCE / BLAS_SAH, and *format_used, the node format the scene
// took as hits_emu_run reports it; tests/test_xform_kat.py.)
extern "C" int hits_emu_render_opts(const rt_scene_desc* desc, const rt_camera_desc* cam, int node_format, int tlas_builder,
                                    uint32_t seed, uint32_t sample_offset, int spp, int depth, float* out,
                                    int volumes_in_bvh, int32_t* format_used) {
  emu::EmuScene E;
  FlattenOptions fo;
  fo.quant_nodes = node_format;
  fo.tlas_builder = tlas_builder;
  fo.lift_volumes = volumes_in_bvh ? 0 : 1;
  if (int rc = emu::load_desc(desc, cam, fo, E)) return rc;
  const DScene& sc = E.d;
  *format_used = sc.wide_nodes ? 2 : sc.quant_nodes ? 1 : 0;
  std::vector<float> frame;
  const int err = wave_run::render(E, seed, sample_offset, uint32_t(spp), uint32_t(spp), depth, frame, nullptr);
  memcpy(out, frame.data(), frame.size() * sizeof(float));
  return err ? 6 : 0;
}

extern "C" int hits_emu_render(const rt_scene_desc* desc, const rt_camera_desc* cam, int node_format, uint32_t seed,
                               uint32_t sample_offset, int spp, int depth, float* out, int volumes_in_bvh) {
  int32_t used = 0;
  return hits_emu_render_opts(desc, cam, node_format, FlattenOptions().tlas_builder, seed, sample_offset, spp, depth, out,
                              volumes_in_bvh, &used);
}

// ---- the traversal stack bound (tests/test_stack_host.py) -------------------
namespace {

constexpr int kPeakRing = wave_run::kRing;       // the smallest ring the host pipeline runs with
constexpr uint32_t kUnwritten = 0xFFFFFFFDu;     // no item (tags end at 13), no entry distance (a NaN), not ITEM_POP / ITEM_NONE
constexpr int kPeakGuard = 8;

// A spill area of kStackMax words (+ guard words) filled with kUnwritten: what
// a traversal wrote shows as the highest word that changed.  push spills the
// ring's oldest entry to word sp - ring when depth sp becomes sp + 1, so the
// highest word written, k, means the stack held k + ring + 1 words.
struct PeakArea {
  std::vector<uint32_t> w = std::vector<uint32_t>(size_t(kStackMax + kPeakGuard), kUnwritten);
  void reset() { std::fill(w.begin(), w.end(), kUnwritten); }
  int top() const {
    int k = int(w.size()) - 1;
    while (k >= 0 && w[size_t(k)] == kUnwritten) --k;
    return k;
  }
};

}  // namespace

// What the flattener derives for the traversal stack.  out[0]: flatten_scene's
// status (the others are then 0); [1] stack_needed, [2] tlas_need4, [3]
// blas_need4, [4] max_leaf_inst, [5] dfs_order, [6] the node format taken, [7]
// stack_needed8, [8] tlas_need8, [9] blas_need8 (the 8-wide figures only
// where that format is taken), [10] BVH4 nodes, [11] 8-wide nodes, [12] BLASes,
// [13] the bound the kernels' spill area is sized from (scene_scalars).
// nodes4 (cap4 nodes x 5 words: the four child items, then the mask of used
// slots), nodes8 (cap8 x 32 words: the records as they are) and roots (the
// world root item in both forms, then per BLAS its root item in both forms;
// at most cap_roots words) may be null.
extern "C" int hits_emu_stack_info(const rt_scene_desc* desc, int tlas_builder, int blas_builder, int node_format, int32_t* out,
                                   uint32_t* nodes4, int cap4, uint32_t* nodes8, int cap8, uint32_t* roots, int cap_roots) {
  HostScene h;
  std::string err;
  FlattenOptions fo;
  fo.tlas_builder = tlas_builder;
  fo.blas_builder = blas_builder;
  fo.quant_nodes = node_format;
  for (int i = 0; i < 14; ++i) out[i] = 0;
  out[0] = flatten_scene(desc, h, err, fo);
  if (out[0]) { fprintf(stderr, "hits_emu: flatten: %s\n", err.c_str()); return 0; }
  out[1] = h.stack_needed; out[2] = h.tlas_need4; out[3] = h.blas_need4; out[4] = h.max_leaf_inst; out[5] = h.dfs_order;
  out[6] = h.wide_nodes ? 2 : h.quant_nodes ? 1 : 0;
  out[7] = h.stack_needed8; out[8] = h.tlas_need8; out[9] = h.blas_need8;
  out[10] = int32_t(h.nodes4.size()); out[11] = int32_t(h.nodes8.size()); out[12] = int32_t(h.blas.size());
  DScene d{};
  scene_scalars(h, d, err);
  out[13] = d.stack_needed;
  const float inf = std::numeric_limits<float>::infinity();
  if (nodes4)
    for (size_t i = 0; i < h.nodes4.size() && i < size_t(cap4); ++i) {
      uint32_t used = 0;
      for (int c = 0; c < 4; ++c) {
        nodes4[5 * i + size_t(c)] = h.nodes4[i].item[c];
        if (h.nodes4[i].xlo[c] != inf) used |= 1u << c;
      }
      nodes4[5 * i + 4] = used;
    }
  if (nodes8)
    for (size_t i = 0; i < h.nodes8.size() && i < size_t(cap8); ++i) memcpy(nodes8 + 32 * i, &h.nodes8[i], 128);
  if (roots) {
    std::vector<uint32_t> r{h.tlas.root_item, h.root8};
    for (size_t b = 0; b < h.blas.size(); ++b) {
      r.push_back(h.blas[b].root_item);
      r.push_back(b < h.blas_root8.size() ? h.blas_root8[b] : 0u);
    }
    for (size_t i = 0; i < r.size() && i < size_t(cap_roots); ++i) roots[i] = r[i];
  }
  return 0;
}

// n rays through the production kernels with the smallest ring the host
// pipeline runs with, and each ray's peak stack depth in words, read off the
// spill area (PeakArea).  any == 0: closest hits (k_extend in the variant
// pick_variant names, the rare-primitive / reference-order one included;
// top / prim / t as hits_emu_run_paths); any == 1: shadow rays from o along d
// to tmax[i] through k_shadow (vis[i]: 1 the ray passed).  tight == 1: the
// kernels see the product's spill capacity, spill_cap_for(the scene's bound,
// ring); tight == 0: kStackMax words, so a ray that needs more than the bound
// shows as a peak above it and not as a dropped entry.  peak[i]: 0 when the
// ray never left the ring (at most `ring` words), else its deepest stack.
// info[0] the node format taken, [1] the scene's bound, [2] the ring, [3] the
// spill capacity given, [4] words written at or past that capacity (never:
// TStack checks), [5] the kernels' error flag.  Returns 0 or load_desc's code.
extern "C" int hits_emu_stack_trace(const rt_scene_desc* desc, const rt_camera_desc* cam, int tlas_builder, int blas_builder,
                                    int node_format, int tight, int any, int bounce, const float* o, const float* d,
                                    const float* tmax, int n, int32_t* top, int32_t* prim, float* t, int32_t* vis,
                                    int32_t* peak, int32_t* info) {
  emu::EmuScene E;
  FlattenOptions fo;
  fo.tlas_builder = tlas_builder;
  fo.blas_builder = blas_builder;
  fo.quant_nodes = node_format;
  if (int rc = emu::load_desc(desc, cam, fo, E)) return rc;
  const DScene& sc = E.d;
  emu::TraceArgs T(E.max_depth, int(sc.stack_needed), kPeakRing);
  PeakArea area;
  const int cap = tight ? spill_cap_for(int(sc.stack_needed), kPeakRing) : kStackMax;
  T.a.spill = area.w.data();
  T.a.spill_sh = area.w.data();
  T.a.spill_cap = cap;
  int past = 0;
  for (int i = 0; i < n; ++i) {
    area.reset();
    if (any) {
      vis[i] = int32_t(emu::shadow_path<kPeakRing>(E, T, o + 3 * i, d + 3 * i, tmax[i], 0u, uint32_t(bounce)) & 1u);
    } else {
      emu::hit_ids(sc, emu::unpack(emu::trace_path<kPeakRing>(E, T, o + 3 * i, d + 3 * i, 0u, uint32_t(bounce))), top[i], prim[i],
                   t[i]);
    }
    const int k = area.top();
    peak[i] = k < 0 ? 0 : k + kPeakRing + 1;
    if (k >= cap) ++past;
  }
  info[0] = sc.wide_nodes ? 2 : sc.quant_nodes ? 1 : 0;
  info[1] = int32_t(sc.stack_needed);
  info[2] = kPeakRing;
  info[3] = cap;
  info[4] = past;
  info[5] = T.err;
  return 0;
}

// TStack alone (device_common.h): `n` distinct words pushed onto a stack of
// `ring` LDS entries (a power of two) over a spill area of spill_cap words,
// then popped.  popped[i]: the i-th word popped (n of them); *err: the flag
// push raises; *first_err: the depth at which it was first raised (-1:
// never); *past: spill words written at or beyond spill_cap.  With n <= ring
// + spill_cap the words come back in reverse order and the flag stays clear;
// the push that makes the depth ring + spill_cap + 1 raises it.
extern "C" int hits_emu_stack_unit(int ring, int spill_cap, int n, uint32_t* popped, int32_t* err, int32_t* first_err,
                                   int32_t* past) {
  if (ring <= 0 || (ring & (ring - 1)) != 0 || spill_cap < 0 || spill_cap > kStackMax || n < 0) return 2;
  std::vector<uint32_t> lds(size_t(ring) + 16, 0u), spill(size_t(kStackMax + kPeakGuard), kUnwritten);
  const TStack S{lds.data(), 1, ring, spill.data(), lds.data(), 1, spill_cap};
  int e = 0, sp = 0;
  *first_err = -1;
  for (int i = 0; i < n; ++i) {
    S.push(sp, 0x1000u + uint32_t(i), &e);
    ++sp;
    if (e && *first_err < 0) *first_err = sp;
  }
  for (int i = 0; i < n; ++i) { --sp; popped[i] = S.pop(sp); }
  *err = e;
  *past = 0;
  for (size_t k = size_t(spill_cap); k < spill.size(); ++k) *past += spill[k] != kUnwritten;
  return 0;
}

// hits_emu_render_opts with the mesh builder named too (RT_OPT_BLAS_BUILDER).
extern "C" int hits_emu_render_blas(const rt_scene_desc* desc, const rt_camera_desc* cam, int node_format, int tlas_builder,
                                    int blas_builder, uint32_t seed, int spp, int depth, float* out, int32_t* info) {
  emu::EmuScene E;
  FlattenOptions fo;
  fo.quant_nodes = node_format;
  fo.tlas_builder = tlas_builder;
  fo.blas_builder = blas_builder;
  if (int rc = emu::load_desc(desc, cam, fo, E)) return rc;
  const DScene& sc = E.d;
  info[0] = sc.wide_nodes ? 2 : sc.quant_nodes ? 1 : 0;
  info[1] = int32_t(sc.stack_needed);
  info[2] = spill_cap_for(int(sc.stack_needed), wave_run::kRing);
  std::vector<float> frame;
  const int err = wave_run::render(E, seed, 0u, uint32_t(spp), uint32_t(spp), depth, frame, nullptr);
  memcpy(out, frame.data(), frame.size() * sizeof(float));
  return err ? 6 : 0;
}
