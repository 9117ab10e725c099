// ray_source.h — launch interface of ray_source.hip: the caller's rays as
// bounce 0 of the wavefront pipeline (rt_ray_color).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wavefront.h"

namespace rtg {

// The rays of one rt_ray_color range.  A ray is two float4 (rt_path_ray:
// origin.xyz, id; direction.xyz, reserved), indexed by the entries of the
// twin's "pixel list" (WaveArgs::pixels), which name rays of this range.  Its
// own struct, like QueryArgs: WaveArgs keeps its size and offsets.
struct RaySource {
  const float4* rays;   // 2 * (rays of the range)
  uint32_t num_rays;    // rays of the range: every list entry is below it
};

// Slot i of a batch of `nslots` (= samples * a.npix) takes ray
// a.pixels[i % a.npix] at sample sample_base + i / a.npix: Lout[i] = 0, and,
// for a ray that passes the guard, stream 0 gets (origin, slot), (direction,
// key), (1, 1, 1, state(a.max_depth, bounce 0, emitters count)).  The valid
// rays are dense in stream 0; a.counts[CNT_STREAM0], which must be 0 when the
// kernel starts (k_set_counts), ends as their number.
hipError_t launch_ray_source(const WaveArgs& a, const RaySource& src, uint32_t nslots, uint32_t sample_base, int cus,
                             hipStream_t st);

// list[k] = k for k < n: the list of a range whose rays are taken in order.
hipError_t launch_ray_identity(uint32_t* list, uint32_t n, int cus, hipStream_t st);

}  // namespace rtg
