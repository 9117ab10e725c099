// query_emu.cpp — test-only: the ray-query kernels (query.hip k_query)
// compiled for the host over a caller's scene description and rays.  A plain
// shared library (no sanitizer, nothing to preload) that tests load with
// ctypes next to the oracle (tests/test_query_host.py), as tests/hits_emu.cpp
// is for k_extend.  The kernel addresses its LDS columns, its spill column
// and its rays by threadIdx / blockIdx, so a 256-lane block is emulated by
// running the kernel once per lane with the indices set, the block's lanes
// in ascending or in descending order: every lane's state lies in its own
// column, so the order must not show.  Not a product path.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../go-raytracing_amd/csrc/query.hip"
#include "../go-raytracing_amd/csrc/wave_layout.h"
#include "emu_scene.h"

using namespace rtg;

namespace {

template <bool kAny>
void run_grid(const DScene& sc, const QueryArgs& a, int blocks, int descending) {
  blockDim = dim3(256);
  gridDim = dim3(uint32_t(blocks));
  for (int b = 0; b < blocks; ++b) {
    for (int k = 0; k < 256; ++k) {
      blockIdx = dim3(uint32_t(b));
      threadIdx = dim3(uint32_t(descending ? 255 - k : k));
      with_traversal(pick_variant(sc), [&](auto V, auto Q, auto) {
        k_query<kAny, decltype(V)::value, decltype(Q)::value>(sc, a);
      });
    }
  }
  blockDim = dim3(1); gridDim = dim3(1); blockIdx = dim3(0); threadIdx = dim3(0);
}

}  // namespace

// n rays (rt_ray) through k_query in the variant the product picks for the
// scene `desc`, flattened with the given world-BVH builder, mesh builder, node
// format (0 fp32, 1 quant8, 2 wide8) and lift_prims (RT_OPT_LIFT_PRIMS as a
// context has it: 1 lifted).  any == 0: hits receives n rt_ray_hit; any == 1:
// occ receives n bytes.  blocks: the persistent grid (>= 1; fewer than the
// chunks makes a block loop).  info[0] the node format taken, [1] the scene's
// stack bound, [2] the spill capacity, [3] the lifted primitives, [4] the
// kernels' error flag, [5] 1 when the rare-primitive (kVol) variant ran.
// Returns 0, or: 2 the scene holds a volume (rt_trace_rays' RT_ERR_UNSUPPORTED),
// load_desc's code, 6 a kernel flagged an internal error.
extern "C" int query_emu_run(const rt_scene_desc* desc, const rt_camera_desc* cam, int tlas_builder, int blas_builder,
                             int node_format, int lift_prims, int any, int blocks, int descending, float time,
                             const rt_ray* rays, int n, rt_ray_hit* hits, uint8_t* occ, int32_t* info) {
  emu::EmuScene E;
  FlattenOptions fo;
  fo.tlas_builder = tlas_builder;
  fo.blas_builder = blas_builder;
  fo.quant_nodes = node_format;
  fo.lift_prims = lift_prims;
  if (int rc = emu::load_desc(desc, cam, fo, E)) return rc;
  const DScene& sc = E.d;
  if (sc.n_volumes > 0) return 2;
  if (blocks < 1 || n < 0) return 1;
  const int cap = spill_cap_for(int(sc.stack_needed), kLdsStack);
  std::vector<uint32_t> spill(size_t(blocks) * 256u * size_t(cap), 0u);
  int err = 0;
  QueryArgs a{};
  a.rays = reinterpret_cast<const float4*>(rays);
  a.out = any ? static_cast<void*>(occ) : static_cast<void*>(hits);
  a.n = uint32_t(n);
  a.time = time;
  a.spill = spill.data();
  a.spill_lanes = uint32_t(blocks) * 256u;
  a.spill_cap = cap;
  a.err = &err;
  if (any) run_grid<true>(sc, a, blocks, descending);
  else run_grid<false>(sc, a, blocks, descending);
  info[0] = sc.wide_nodes ? 2 : sc.quant_nodes ? 1 : 0;
  info[1] = int32_t(sc.stack_needed);
  info[2] = cap;
  info[3] = sc.num_prim_recs;
  info[4] = err;
  info[5] = pick_variant(sc).vol ? 1 : 0;
  return err ? 6 : 0;
}
