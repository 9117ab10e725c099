// wave_variant.h — which variant of the wavefront kernels a scene runs: the
// one statement of the rule, and the one runtime -> template dispatcher.  The
// product (wavefront.hip run_variant, launch_wavefront) and every host
// emulation of the kernels (tests/) pick through these.  Host-only; depends on
// dev_layout.h alone.
#pragma once
#include <type_traits>
#include <utility>

#include "dev_layout.h"

namespace rtg {

struct WaveVariant {
  bool vol;     // the rare-primitive traversal kernels (kVol)
  bool envis;   // the importance-sampled HDRI as a NEE light (kEnvIS)
  bool quant;   // DNodeQ nodes (kQuant)
  bool wide;    // DNode8 nodes (kWide)
  int shade;    // SHADE_* | SHADE_LIFT (kShade)
};

inline WaveVariant pick_variant(const DScene& sc) {
  WaveVariant v{};
  // the kVol kernels carry the volumes left in the world BVH, the rare
  // primitives (circles) and the reference-order closest hit of RotateX/Z
  // scenes (DScene.dfs_order)
  v.vol = sc.has_volumes != 0 || sc.n_circles > 0 || sc.dfs_order != 0;
  // the importance-sampled HDRI is a NEE light only beside an area light
  // (sampleLightMIS needs one, camera.go:502): without lights the kEnvIS code
  // is dead, and its registers spilled (C5: 34 VGPRs in bounce 0's shading)
  v.envis = sc.env.valid && sc.env.use_is && sc.num_lights > 0;
  // node format: the 8-wide format has no rare-primitive variant (flatten
  // builds it only for scenes that do not need one), then quant8, then fp32
  v.wide = sc.wide_nodes != 0 && !v.vol;
  v.quant = sc.quant_nodes != 0 && !v.wide;
  // the variants that test the lifted world primitives (lean / material
  // scenes only, flatten_scene)
  v.shade = sc.shade_kind | (sc.num_prim_recs > 0 ? SHADE_LIFT : 0);
  return v;
}

// f(Q, W) with std::bool_constant arguments for the node format.  kVol stays
// the caller's template parameter (the translation units split on it);
// with_nodes<true> never instantiates W = true.
template <bool kVol, class F>
auto with_nodes(const WaveVariant& v, F&& f) {
  if constexpr (!kVol) {
    if (v.wide) return f(std::false_type{}, std::true_type{});
  }
  if (v.quant) return f(std::true_type{}, std::false_type{});
  return f(std::false_type{}, std::false_type{});
}

// f(E, S) with std::bool_constant / std::integral_constant<int, SHADE_*>
// arguments: the six shading arms that exist.  An unknown kind shades lean.
template <class F>
auto with_shading(const WaveVariant& v, F&& f) {
  auto by_shade = [&](auto E) {
    auto arm = [&](auto S) { return f(E, S); };
    switch (v.shade) {
      case SHADE_FULL: return arm(std::integral_constant<int, SHADE_FULL>{});
      case SHADE_VOL: return arm(std::integral_constant<int, SHADE_VOL>{});
      case SHADE_MAT: return arm(std::integral_constant<int, SHADE_MAT>{});
      case SHADE_MAT | SHADE_LIFT: return arm(std::integral_constant<int, SHADE_MAT | SHADE_LIFT>{});
      case SHADE_LEAN | SHADE_LIFT: return arm(std::integral_constant<int, SHADE_LEAN | SHADE_LIFT>{});
      default: return arm(std::integral_constant<int, SHADE_LEAN>{});
    }
  };
  return v.envis ? by_shade(std::true_type{}) : by_shade(std::false_type{});
}

// f(V, Q, W) for callers that compile both values of kVol (the host
// emulations of the kernels; the product's translation units split on it).
template <class F>
auto with_traversal(const WaveVariant& v, F&& f) {
  if (v.vol) return with_nodes<true>(v, [&](auto Q, auto W) { return f(std::true_type{}, Q, W); });
  return with_nodes<false>(v, [&](auto Q, auto W) { return f(std::false_type{}, Q, W); });
}

}  // namespace rtg
