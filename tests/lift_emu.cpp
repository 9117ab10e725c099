// lift_emu.cpp — test-only: world quads / spheres lifted out of the world BVH
// (FlattenOptions::lift_prims, DPrimRec) on the host.  The production
// closest-hit and any-hit kernels (wavefront.hip k_extend / k_shadow, one
// lane) over a caller's scene description flattened with lifting on or off,
// followed by what the shading code adds when primitives are lifted
// (device_common.h lifted_prims, shade_path's NEE tests), so that the two
// placements can be compared record for record (tests/test_lift_host.py).
//
// Built twice: as a plain shared library (no sanitizer, nothing to preload)
// that the tests load with ctypes next to the oracle, like tests/hits_emu.cpp;
// and, with -DLIFT_EMU_MAIN, as a stand-alone program under AddressSanitizer +
// UBSan that flattens a named librtscene scene both ways in every node format
// and world builder and compares the hits of its camera rays.  Not a product
// path.
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

using namespace rtg;

namespace {

// The description flattened as a context flattens it.
int load(const rt_scene_desc* desc, const rt_camera_desc* cam, int tlas_builder, int node_format, int lift,
         emu::EmuScene& E) {
  FlattenOptions fo;
  fo.tlas_builder = tlas_builder;
  fo.quant_nodes = node_format;
  fo.lift_prims = lift;
  return emu::load_desc(desc, cam, fo, E);
}

int format_of(const DScene& sc) { return sc.wide_nodes ? 2 : sc.quant_nodes ? 1 : 0; }

uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
template <class T>
uint64_t fnv_vec(uint64_t h, const std::vector<T>& v) {
  const uint64_t n = v.size();
  h = fnv(h, &n, sizeof n);
  return v.empty() ? h : fnv(h, v.data(), v.size() * sizeof(T));
}
// Everything of the flatten output that a lift could change: the trees in
// every form, the leaves, the refs and what is parallel to them, the world
// primitives, the header and the stack bounds.
uint64_t flatten_hash(const HostScene& h) {
  uint64_t x = 1469598103934665603ull;
  x = fnv_vec(x, h.nodes); x = fnv_vec(x, h.nodes4); x = fnv_vec(x, h.leaves); x = fnv_vec(x, h.refs);
  x = fnv_vec(x, h.ref_rank); x = fnv_vec(x, h.ref_top); x = fnv_vec(x, h.quad_hidx); x = fnv_vec(x, h.sphere_hidx);
  x = fnv_vec(x, h.quad_wref); x = fnv_vec(x, h.sphere_wref); x = fnv_vec(x, h.litems); x = fnv_vec(x, h.tri_hidx);
  for (const DNode8& n : h.nodes8) x = fnv(x, &n, 104);   // (the record's tail is unused)
  for (const DQuad& q : h.quads) { x = fnv(x, &q.Qx, 28); x = fnv(x, &q.ux, 12); x = fnv(x, &q.vx, 12); x = fnv(x, &q.wx, 12); }
  for (const DSphere& s : h.spheres) x = fnv(x, &s, 28);
  x = fnv(x, h.tlas.box, sizeof h.tlas.box);
  const int32_t w[] = {int32_t(h.tlas.root_item), h.tlas.check_box, int32_t(h.root8), h.stack_needed, h.stack_needed8,
                       h.tlas_depth, h.tlas_need4, h.tlas_need8, h.max_leaf_inst, h.quant_nodes, h.wide_nodes, h.dfs_order};
  return fnv(x, w, sizeof w);
}

// World quads / spheres still inside the world BVH: inline items
// (ITEM_WQUAD / ITEM_WSPHERE) and refs of the world's mixed leaves, in the
// BVH4 tree from the world root (instances are not entered) and, in the
// 8-wide format, among the leaf items.
void world_prims_in_bvh(const HostScene& h, int& inline_items, int& leaf_refs, int& inline_items8) {
  inline_items = leaf_refs = inline_items8 = 0;
  auto item = [&](uint32_t it, auto&& self) -> void {
    const uint32_t tag = it >> ITEM_SHIFT, idx = it & ITEM_MASK;
    if (tag == ITEM_WQUAD || tag == ITEM_WSPHERE) { inline_items++; return; }
    if (tag == ITEM_LEAF) {
      const DLeaf& L = h.leaves[idx];
      if (leaf_kind(L.info) != PK_MIXED) return;
      for (int k = 0; k < leaf_count(L.info); ++k) {
        const int kind = int(h.refs[L.first + uint32_t(k)] >> REF_SHIFT);
        if (kind == PK_QUAD || kind == PK_SPHERE) leaf_refs++;
      }
      return;
    }
    if (tag == ITEM_NODE)
      for (uint32_t c : h.nodes4[idx].item) self(c, self);
  };
  item(h.tlas.root_item, item);
  if (h.wide_nodes) {
    // the 8-wide world tree's leaves are among litems (BLAS mixed leaves hold
    // object-space primitives: only world leaves carry the inline world tags)
    auto tag_of = [](uint32_t it) { return it >> ITEM_SHIFT; };
    for (uint32_t it : h.litems)
      if (tag_of(it) == ITEM_WQUAD || tag_of(it) == ITEM_WSPHERE) inline_items8++;
    if (tag_of(h.root8) == ITEM_WQUAD || tag_of(h.root8) == ITEM_WSPHERE) inline_items8++;
  }
}

}  // namespace

// What flatten_scene makes of the description.  out[0] flatten's status (the
// rest 0 then), [1] lifted records, [2] inline world quad / sphere items left
// in the world BVH, [3] quad / sphere refs left in world leaves, [4] the node
// format taken, [5] dfs_order, [6] stack_needed, [7] tlas_depth, [8] BVH4
// nodes, [9] refs, [10] quads, [11] spheres, [12] inline world quad / sphere
// items among the 8-wide format's leaf items.  recs[8 * r + ..]: record r's
// kind, index in its array, ref position, DFS rank, axis code, has_box, the
// primitive's hittable id, the ref position its quad_wref / sphere_wref entry
// names.  boxes[6 * r + ..]: its box (xmin xmax ymin ymax zmin zmax).  *hash:
// a hash of the flatten output (flatten_hash).
extern "C" int lift_emu_flatten(const rt_scene_desc* desc, int tlas_builder, int node_format, int lift, int32_t* out,
                                int32_t* recs, float* boxes, uint64_t* hash) {
  HostScene h;
  std::string err;
  FlattenOptions fo;
  fo.tlas_builder = tlas_builder;
  fo.quant_nodes = node_format;
  fo.lift_prims = lift;
  for (int i = 0; i < 13; ++i) out[i] = 0;
  out[0] = flatten_scene(desc, h, err, fo);
  if (out[0]) { fprintf(stderr, "lift_emu: flatten: %s\n", err.c_str()); return 0; }
  int inl = 0, refs = 0, inl8 = 0;
  world_prims_in_bvh(h, inl, refs, inl8);
  out[12] = inl8;
  out[1] = int32_t(h.prim_recs.size()); out[2] = inl; out[3] = refs;
  out[4] = h.wide_nodes ? 2 : h.quant_nodes ? 1 : 0;
  out[5] = h.dfs_order; out[6] = h.stack_needed; out[7] = h.tlas_depth; out[8] = int32_t(h.nodes4.size());
  out[9] = int32_t(h.refs.size()); out[10] = int32_t(h.quads.size()); out[11] = int32_t(h.spheres.size());
  for (size_t r = 0; r < h.prim_recs.size() && r < size_t(kPrimRecMax); ++r) {
    const DPrimRec& R = h.prim_recs[r];
    int32_t* o = recs + 8 * r;
    uint32_t code = 0;
    memcpy(&code, &R.q.pad0, 4);
    o[0] = R.kind; o[1] = R.idx; o[2] = R.refpos; o[3] = h.ref_rank[size_t(R.refpos)];
    o[4] = R.kind == PK_QUAD ? int32_t(code) : 0; o[5] = R.has_box;
    o[6] = R.kind == PK_QUAD ? h.quad_hidx[size_t(R.idx)] : h.sphere_hidx[size_t(R.idx)];
    o[7] = R.kind == PK_QUAD ? h.quad_wref[size_t(R.idx)] : h.sphere_wref[size_t(R.idx)];
    for (int a = 0; a < 3; ++a) { boxes[6 * r + 2 * size_t(a)] = R.lo[a]; boxes[6 * r + 2 * size_t(a) + 1] = R.hi[a]; }
  }
  *hash = flatten_hash(h);
  return 0;
}

// Closest hits of n path rays at bounce `bounce` (pix[i]: the path's pixel;
// the RNG key is production's for (seed, pixel, sample)), with lifting on or
// off.  Per ray: top, prim (hittable ids; -1 a miss), t (-1), the instance
// (-1 none) and the DFS rank of the hit's top-level object (its ref position
// names a different slot in the two placements, its rank does not; -1 a miss
// or a plane).  Returns 0, load_desc's code, or 6 when a kernel flagged an
// internal error.
extern "C" int lift_emu_paths(const rt_scene_desc* desc, const rt_camera_desc* cam, int tlas_builder, int node_format,
                              int lift, uint32_t seed, uint32_t sample, int bounce, const int32_t* pix, const float* o,
                              const float* d, int n, int32_t* top, int32_t* prim, float* t, int32_t* inst, int32_t* rank,
                              int32_t* info) {
  emu::EmuScene E;
  if (int rc = load(desc, cam, tlas_builder, node_format, lift, E)) return rc;
  const DScene& sc = E.d;
  info[0] = format_of(sc);
  info[1] = sc.num_prim_recs;
  emu::TraceArgs T(E.max_depth, int(sc.stack_needed));
  for (int i = 0; i < n; ++i) {
    const uint32_t key = path_key(seed, uint32_t(pix[i]), sample);
    const emu::Hit h = emu::closest(E, T, o + 3 * i, d + 3 * i, key, uint32_t(bounce));
    emu::hit_ids(sc, h, top[i], prim[i], t[i]);
    inst[i] = rank[i] = -1;
    if (h.kh != 0u) {
      inst[i] = h.inst;
      rank[i] = h.refpos >= 0 ? sc.ref_rank[h.refpos] : -1;
    }
  }
  return T.err ? 6 : 0;
}

// The NEE shadow rays of n paths at bounce `bounce` and what becomes of them:
// k_extend's hit (unmerged: shade_path merges the lifted primitives itself),
// shade_path in the variant pick_variant names (the lift variant when
// primitives are lifted: a ray a lifted primitive occludes is cleared there),
// then k_shadow for every ray the job still carries.  vis[i]: bit 0 / 1 the
// area / HDRI ray is unoccluded; traced[i]: the rays k_shadow walked.
extern "C" int lift_emu_nee(const rt_scene_desc* desc, const rt_camera_desc* cam, int tlas_builder, int node_format, int lift,
                            uint32_t seed, uint32_t sample, int bounce, int dleft, const int32_t* pix, const float* o,
                            const float* d, int n, int32_t* vis, int32_t* traced) {
  emu::EmuScene E;
  if (int rc = load(desc, cam, tlas_builder, node_format, lift, E)) return rc;
  emu::TraceArgs T(E.max_depth, int(E.d.stack_needed));
  std::vector<uint32_t> spill_sh(T.spill.size() + 1, 0u);
  T.a.spill_sh = spill_sh.data();
  const uint32_t bn = uint32_t(bounce);
  for (int i = 0; i < n; ++i) {
    const uint32_t key = path_key(seed, uint32_t(pix[i]), sample);
    const V3 ro = mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    const float4 h = emu::trace_path(E, T, o + 3 * i, d + 3 * i, key, bn);
    const emu::Shaded r = emu::shade_by_kind(E, T, h, ro, rd, mk(1.0f, 1.0f, 1.0f), key, dleft, bn, true);
    const float P[3] = {r.P.x, r.P.y, r.P.z}, da[3] = {r.da.x, r.da.y, r.da.z}, dh[3] = {r.dh.x, r.dh.y, r.dh.z};
    uint32_t v = 0;
    if ((r.flags & 2u) && (emu::shadow_path(E, T, P, dh, std::numeric_limits<float>::infinity(), key, bn) & 1u)) v |= 2u;
    if ((r.flags & 1u) && (emu::shadow_path(E, T, P, da, r.tmax_a, key, bn) & 1u)) v |= 1u;
    vis[i] = int32_t(v);
    traced[i] = int32_t(r.flags & 3u);
  }
  return T.err ? 6 : 0;
}

#ifdef LIFT_EMU_MAIN
// lift_emu NAME WIDTH ASSET_DIR [LUCY_RINGS LUCY_COLS]: the named scene
// flattened with lifting on and off under both world builders and the three
// node formats; the closest hits of its camera rays (sample 0) must agree.
// Prints one line per combination; exit status 0 when all agree.
int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: lift_emu NAME WIDTH ASSET_DIR [RINGS COLS]\n"); return 2; }
  rts_scene_options opt{};
  opt.width = atoi(argv[2]);
  opt.asset_dir = argv[3];
  opt.lucy_rings = argc > 4 ? atoi(argv[4]) : 30;
  opt.lucy_cols = argc > 5 ? atoi(argv[5]) : 40;
  char err[512] = {0};
  rts_scene* scn = nullptr;
  if (rts_scene_create(argv[1], &opt, &scn, err, sizeof err) != 0) { fprintf(stderr, "%s\n", err); return 3; }
  const rt_scene_desc* desc = rts_scene_get_desc(scn);
  const rt_camera_desc* cam = rts_scene_get_camera(scn);
  int bad = 0;
  for (int tlas = 0; tlas < 2; ++tlas)
    for (int fmt = 0; fmt < 3; ++fmt) {
      emu::EmuScene E[2];
      for (int lift = 0; lift < 2; ++lift)
        if (int rc = load(desc, cam, tlas, fmt, lift, E[lift])) return rc;
      emu::TraceArgs T0(E[0].max_depth, int(E[0].d.stack_needed)), T1(E[1].max_depth, int(E[1].d.stack_needed));
      const int W = E[0].cam.width, Hh = E[0].cam.height;
      int diff = 0, hits = 0;
      for (int p = 0; p < W * Hh; ++p) {
        const uint32_t key = path_key(7u, uint32_t(p), 0u);
        V3 ro, rd;
        float time;
        get_ray(E[0].cam, p % W, p / W, key, ro, rd, time);
        const float o[3] = {ro.x, ro.y, ro.z}, d[3] = {rd.x, rd.y, rd.z};
        const emu::Hit a = emu::closest(E[0], T0, o, d, key, 0u), b = emu::closest(E[1], T1, o, d, key, 0u);
        int32_t ta, pa, tb, pb;
        float fa, fb;
        emu::hit_ids(E[0].d, a, ta, pa, fa);
        emu::hit_ids(E[1].d, b, tb, pb, fb);
        hits += a.kh != 0u;
        if (ta != tb || pa != pb || memcmp(&fa, &fb, 4) != 0) ++diff;
      }
      printf("{\"tlas\": %d, \"format\": %d, \"format_used\": %d, \"lifted\": %d, \"rays\": %d, \"hits\": %d, \"differ\": %d}\n",
             tlas, fmt, format_of(E[1].d), E[1].d.num_prim_recs, W * Hh, hits, diff);
      bad += diff + (E[0].d.num_prim_recs != 0) + T0.err + T1.err;
    }
  rts_scene_destroy(scn);
  return bad ? 1 : 0;
}
#endif
