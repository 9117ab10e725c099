// features.h — host-side launch interface of features.hip (the feature pass
// of rt_render_features: per-sample albedo / normal / depth / coverage at the
// camera ray's closest hit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_layout.h"

namespace rtg {

constexpr int kFeatFloats = 8;   // albedo.rgb, normal.xyz, depth, coverage

// One batch of one twin, after the bounce-0 k_extend: the hit records of the
// batch's `nslots` slots (slot i = sample sample_base + i / npix of pixel
// pixels[i % npix], as k_extend's camera rays) -> one 32-B record per slot in
// two float4 arrays (fa: albedo.rgb, normal.x; fb: normal.yz, depth, coverage).
hipError_t launch_features(const DScene& sc, const DCamera& cam, const float4* hit, const uint32_t* pixels,
                           uint32_t npix, uint32_t nslots, uint32_t seed, uint32_t sample_base, float4* fa,
                           float4* fb, hipStream_t st);
// acc[pi * 8 + k] += the batch's `nsamp` records of listed pixel pi, in slot
// order, in fp64 (as k_accum).
hipError_t launch_feat_accum(const float4* fa, const float4* fb, uint32_t npix, uint32_t nsamp, double* acc,
                             int num_cus, hipStream_t st);
// out[pixels[pi] * 8 + k] = float(acc (+ out with `accumulate`)) (as k_finalize).
hipError_t launch_feat_finalize(const double* acc, const uint32_t* pixels, uint32_t npix, float* out, int accumulate,
                                int num_cus, hipStream_t st);

}  // namespace rtg
