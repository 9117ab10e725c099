// variant_probe.cpp — CPU-only check of the kernel-variant rule
// (wave_variant.h pick_variant / with_nodes / with_shading) and of the scene
// scalars it reads (flatten.cpp scene_scalars).  Built and run by
// tests/test_variant_host.py (g++, no GPU).
//
//   variant_probe roundtrip
//       every WaveVariant through the dispatchers; one JSON line.
//   variant_probe scene NAME WIDTH ASSET_DIR
//       the named librtscene scene flattened in every node format with the
//       world primitives lifted or not; one JSON line per combination.
//   variant_probe badlift
//       scene_scalars on a hand-made HostScene with lifted primitives beside
//       a Noise texture; one JSON line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <tuple>

#include "../go-raytracing_amd/csrc/flatten.h"
#include "../go-raytracing_amd/csrc/wave_variant.h"
#include "../include/rtscene.h"

using namespace rtg;

static int roundtrip() {
  const int shades[6] = {SHADE_LEAN, SHADE_MAT, SHADE_VOL, SHADE_FULL, SHADE_LEAN | SHADE_LIFT, SHADE_MAT | SHADE_LIFT};
  int cases = 0, bad = 0;
  std::set<std::tuple<bool, bool, int, bool, bool>> seen[2];   // (V, E, S, Q, W) reached, by vol
  for (int vol = 0; vol < 2; ++vol)
    for (int envis = 0; envis < 2; ++envis)
      for (int nodes = 0; nodes < 3; ++nodes)   // neither, quant, wide
        for (int shade : shades) {
          const WaveVariant v{vol != 0, envis != 0, nodes == 1, nodes == 2, shade};
          const bool want_w = v.wide && !v.vol;
          auto check = [&](auto V) {
            constexpr bool kV = decltype(V)::value;
            with_nodes<kV>(v, [&](auto Q, auto W) {
              with_shading(v, [&](auto E, auto S) {
                constexpr bool kQ = decltype(Q)::value, kW = decltype(W)::value, kE = decltype(E)::value;
                constexpr int kS = decltype(S)::value;
                static_assert(!(kV && kW), "with_nodes<true> instantiated the 8-wide arm");
                ++cases;
                if (kQ != v.quant || kW != want_w || kE != v.envis || kS != v.shade) ++bad;
                seen[kV ? 1 : 0].insert(std::make_tuple(kV, kE, kS, kQ, kW));
              });
            });
          };
          if (vol) check(std::true_type{}); else check(std::false_type{});
        }
  // an unknown shading kind takes the lean arm
  int unknown = -1;
  with_shading(WaveVariant{false, false, false, false, 5}, [&](auto, auto S) { unknown = decltype(S)::value; });
  printf("{\"cases\": %d, \"bad\": %d, \"distinct_novol\": %zu, \"distinct_vol\": %zu, \"unknown_arm\": %d}\n", cases, bad,
         seen[0].size(), seen[1].size(), unknown);
  return bad ? 1 : 0;
}

static int scene(const char* name, int width, const char* assets) {
  rts_scene_options opt{};
  opt.width = width;
  opt.lucy_rings = 60;
  opt.lucy_cols = 80;
  opt.asset_dir = assets;
  rts_scene* sc = nullptr;
  char err[512] = {0};
  if (rts_scene_create(name, &opt, &sc, err, sizeof err) != 0) { fprintf(stderr, "%s\n", err); return 3; }
  for (int nf = 0; nf < 3; ++nf)
    for (int lift = 0; lift < 2; ++lift) {
      FlattenOptions fo;
      fo.quant_nodes = nf;
      fo.lift_prims = lift;
      HostScene h;
      std::string ferr;
      if (int rc = flatten_scene(rts_scene_get_desc(sc), h, ferr, fo)) { fprintf(stderr, "flatten %d %s\n", rc, ferr.c_str()); return 4; }
      DScene d{};
      if (int rc = scene_scalars(h, d, ferr)) { fprintf(stderr, "scene_scalars %d %s\n", rc, ferr.c_str()); return 5; }
      const WaveVariant v = pick_variant(d);
      printf("{\"nf\": %d, \"lift\": %d, \"shade_kind\": %d, \"vol\": %d, \"format\": %d, \"envis\": %d, \"prim_recs\": %d, "
             "\"shade\": %d}\n",
             nf, lift, d.shade_kind, v.vol ? 1 : 0, v.wide ? 2 : v.quant ? 1 : 0, v.envis ? 1 : 0, d.num_prim_recs, v.shade);
    }
  rts_scene_destroy(sc);
  return 0;
}

static int badlift() {
  HostScene h;
  h.prim_recs.push_back(DPrimRec{});
  DTexture t{};
  t.kind = RT_TEX_NOISE;
  h.textures.push_back(t);
  DScene d{};
  std::string err;
  const int rc = scene_scalars(h, d, err);
  printf("{\"rc\": %d, \"invalid\": %d, \"err\": \"%s\"}\n", rc, RT_ERR_INVALID, err.c_str());
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "roundtrip")) return roundtrip();
  if (argc >= 5 && !strcmp(argv[1], "scene")) return scene(argv[2], atoi(argv[3]), argv[4]);
  if (argc >= 2 && !strcmp(argv[1], "badlift")) return badlift();
  fprintf(stderr, "usage: variant_probe roundtrip | scene NAME WIDTH ASSET_DIR | badlift\n");
  return 2;
}
