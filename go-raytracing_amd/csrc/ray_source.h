// ray_source.h — launch interface of ray_source.hip: the caller's rays, or rays
// drawn on the device from the caller's points, as bounce 0 of the wavefront
// pipeline (rt_ray_color, rt_gather), and rt_gather_sh's SH projection behind it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wavefront.h"

namespace rtg {

// How a 32-B record becomes the ray of one sample.  SRC_CALLER (the value of
// a zero-initialised RaySource) is rt_ray_color: the record is the ray.  The
// others are rt_gather's sources (1 + rtgpu.h's RT_GATHER_* value): the record
// is a point and its normal, and the direction is a function of the sample's
// path key.  SRC_SURFACE is rt_gather_surface: the record is a point and its
// normal and no ray is made of it; stream 0 carries the vertex (p, unit(n)) and
// bounce 0 shades it without tracing (run_batches' surface mode).
enum : int32_t { SRC_CALLER = 0, SRC_RAY = 1, SRC_COSINE = 2, SRC_SPHERE = 3, SRC_SURFACE = 4 };

// The rays of one rt_ray_color / rt_gather range.  A record is two float4
// (rt_path_ray: origin.xyz, id; direction.xyz, reserved; rt_gather_point has
// the same layout with the normal as the direction), indexed by the entries of
// the twin's "pixel list" (WaveArgs::pixels), which name records of this
// range.  Its own struct, like QueryArgs: WaveArgs keeps its size and offsets.
struct RaySource {
  const float4* rays;   // 2 * (records of the range)
  uint32_t num_rays;    // records of the range: every list entry is below it
  int32_t kind;         // SRC_*: launch-uniform, it selects the kernel
};

// Slot i of a batch of `nslots` (= samples * a.npix) takes record
// a.pixels[i % a.npix] at sample sample_base + i / a.npix: Lout[i] = 0, and,
// for a record whose ray is valid, stream 0 gets (origin, slot), (direction,
// key), (1, 1, 1, state(a.max_depth, bounce 0, emitters count)); under
// SRC_SURFACE the second is (unit normal, key).  The valid
// rays are dense in stream 0; a.counts[CNT_STREAM0], which must be 0 when the
// kernel starts (k_set_counts), ends as their number.
hipError_t launch_ray_source(const WaveArgs& a, const RaySource& src, uint32_t nslots, uint32_t sample_base, int cus,
                             hipStream_t st);

// list[k] = k for k < n: the list of a range whose rays are taken in order.
hipError_t launch_ray_identity(uint32_t* list, uint32_t n, int cus, hipStream_t st);

// rt_gather_rays: out[2k], out[2k+1] = the rt_path_ray that sample `sample` of
// point k traces under `kind` (SRC_RAY .. SRC_SPHERE) and `seed`, or
// (p, id), (0, 0, 0, 0) for an invalid point.
hipError_t launch_gather_rays(const float4* pts, uint32_t n, int32_t kind, uint32_t seed, uint32_t sample, float4* out,
                              int cus, hipStream_t st);

// rt_gather_sh (WavePlan::sh_acc): the sums of one point, 3 per coefficient.
constexpr int kShMaxBands = 3;   // rtgpu.h's RT_SH_MAX_BANDS
constexpr int sh_floats(int bands) { return 3 * bands * bands; }

// After a batch's k_accum: acc[(k * 3 + c) * a.npix + pi] += sum over the
// batch's nsamp samples q, in that order, of double(Lout[q * a.npix + pi].c) *
// double(Y_k(d)), d the SRC_SPHERE direction of record a.pixels[pi] at sample
// sample_base + q, for k < bands^2.  src.kind must be SRC_SPHERE.  An invalid
// point's sums are left as they are.
hipError_t launch_sh_accum(const WaveArgs& a, const RaySource& src, uint32_t nsamp, uint32_t sample_base, int bands,
                           double* acc, int cus, hipStream_t st);
// out[pixels[pi] * 3 bands^2 + j] = float(acc[j * npix + pi] (+ out with `accumulate`)) (as k_finalize).
hipError_t launch_sh_finalize(const double* acc, const uint32_t* pixels, uint32_t npix, int bands, float* out,
                              int accumulate, int cus, hipStream_t st);

}  // namespace rtg
