// query.h — launch interface of query.hip: closest hit and occlusion for a
// caller's rays (rt_trace_rays / rt_occluded).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_layout.h"

namespace rtg {

// One launch's rays and results.  A ray is two float4 (rt_ray: origin.xyz,
// tmin; direction.xyz, tmax); a closest hit is two float4 (rt_ray_hit: t, top,
// prim, material; normal.xyz, flags), an occlusion result one byte.
struct QueryArgs {
  const float4* rays;    // 2 * n
  void* out;             // closest hit: float4[2 * n]; any hit: uint8_t[n]
  uint32_t n;            // <= kQueryMaxRays
  float time;            // the rays' ray.Time()
  uint32_t* spill;       // traversal-stack spill area: spill_cap entries x spill_lanes
  uint32_t spill_lanes;  // >= the grid's lanes (blocks * 256)
  int32_t spill_cap;
  int* err;              // the traversal's stack-overflow flag
};

constexpr uint32_t kQueryMaxRays = 1u << 30;   // per launch; callers split longer arrays
constexpr uint32_t kQueryFront = 1u, kQueryInvalid = 2u;   // rt_ray_hit.flags (RT_HIT_FRONT, RT_HIT_INVALID_RAY)

// Blocks of the persistent grid for n rays: at most the resident blocks of
// the scene's kernel variant times `cus`, at most one per 256-ray chunk, and
// at most max_blocks when that is > 0 (RT_OPT_MAX_BLOCKS).
int query_blocks(const DScene& sc, bool any, uint32_t n, int cus, int max_blocks);
// a.spill must hold spill_cap * blocks * 256 words.
hipError_t launch_query(const DScene& sc, bool any, const QueryArgs& a, int blocks, hipStream_t st);

}  // namespace rtg
