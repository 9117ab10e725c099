// moments.h — host-side launch interface of moments.hip (the moments mode of
// a render, rt_render_moments: per pixel the sum and the sum of squares of its
// samples' luminance).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtg {

constexpr int kMomFloats = 2;   // per pixel: m1 = sum Y, m2 = sum Y^2

// acc[pi * 2 + k] += the moments of Lout[q * npix + pi], q = 0 .. nsamp - 1, in
// that order, in fp64 (the samples k_accum sums, in its order).
hipError_t launch_moment_accum(const float4* Lout, uint32_t npix, uint32_t nsamp, double* acc, int num_cus,
                               hipStream_t st);
// out[pixels[pi] * 2 + k] = float(acc (+ out with `accumulate`)) (as k_finalize).
hipError_t launch_moment_finalize(const double* acc, const uint32_t* pixels, uint32_t npix, float* out, int accumulate,
                                  int num_cus, hipStream_t st);

}  // namespace rtg
