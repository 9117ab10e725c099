// hits_emu.cpp — test-only: the production closest-hit kernel (wavefront.hip
// k_extend, a later bounce: rays read from the path stream) compiled for the
// host, one lane, over a caller's scene description and given rays.  A plain
// shared library (no sanitizer, nothing to preload) that tests load with
// ctypes next to the oracle (tests/test_scale_host.py).  Like
// tests/ray_emu.cpp, but the scene is an rt_scene_desc, the flatten options
// are the caller's, and the hit record is mapped to hittable ids the way
// probe.hip's path_hits_kernel maps it (rt_primary_hits' conventions: top,
// prim = -1 and t = -1 for a miss).  Not a product path.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../go-raytracing_amd/csrc/wavefront.hip"
#include "emu_scene.h"
#include "emu_trace.h"

using namespace rtg;

namespace {

// probe.hip hit_ids
void hit_ids(const DScene& sc, int kind, int idx, int refpos, int32_t& top, int32_t& prim) {
  if (kind == PK_PLANE) { top = prim = sc.plane_hidx[idx]; return; }
  top = sc.tlas_ref_top[refpos];
  if (kind == PK_SPHERE) prim = sc.sphere_hidx[idx];
  else if (kind == PK_QUAD) prim = sc.quad_hidx[idx];
  else if (kind == PK_TRI) prim = sc.tri_hidx[idx];
  else if (kind == PK_CIRCLE) prim = sc.circle_hidx[idx];
  else prim = sc.volume_hidx[idx];
}

}  // namespace

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
  if (sc.has_volumes || sc.num_vol_refs > 0 || sc.n_circles > 0 || sc.dfs_order) {
    fprintf(stderr, "hits_emu: rare-primitive scenes are not supported\n");
    return 3;
  }
  *format_used = sc.wide_nodes ? 2 : sc.quant_nodes ? 1 : 0;
  emu::TraceArgs T(E.max_depth);
  for (int i = 0; i < n; ++i) {
    const float4 h = emu::trace_one(E, T, o + 3 * i, d + 3 * i);
    uint32_t w[4];
    memcpy(w, &h, 16);
    top[i] = prim[i] = -1;
    t[i] = -1.0f;
    if (w[1] != 0u) {
      hit_ids(sc, int(w[1] >> 28), int(w[1] & 0x0FFFFFFFu), int(w[3]), top[i], prim[i]);
      t[i] = h.x;
    }
  }
  return T.err ? 6 : 0;
}
