// hit_ids.h — a closest hit's hittable ids, shared by the probes (probe.hip)
// and the ray queries (query.hip).  Include after device_common.h.
#pragma once
#include "dev_layout.h"

namespace rtg {

// Hittable ids of a closest hit (kind, primitive index, TLAS ref position).
__device__ __forceinline__ void hit_ids(const DScene& sc, int kind, int idx, int refpos, int& top, int& prim) {
  if (kind == PK_PLANE) { top = prim = sc.plane_hidx[idx]; return; }
  top = sc.tlas_ref_top[refpos];
  if (kind == PK_SPHERE) prim = sc.sphere_hidx[idx];
  else if (kind == PK_QUAD) prim = sc.quad_hidx[idx];
  else if (kind == PK_TRI) prim = sc.tri_hidx[idx];
  else if (kind == PK_CIRCLE) prim = sc.circle_hidx[idx];
  else prim = sc.volume_hidx[idx];
}

}  // namespace rtg
