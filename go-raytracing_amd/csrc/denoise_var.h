// denoise_var.h — launch interface of denoise_var.hip (rt_denoise_variance):
// the variance-guided a-trous filter over a frame's radiance sums, guided by
// its feature image and its luminance moments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtg {

// What every kernel of one rt_denoise_variance call shares.
struct DvArgs {
  const float* accum;    // W*H*3 radiance sums (the call's input)
  const float* feat;     // W*H*8 feature sums (16-B aligned: read as two float4 per pixel)
  const float* moments;  // W*H*2 luminance moments (null in the spatial case)
  float* out;            // W*H*3 filtered sums (the last pass writes it)
  float* out_var;        // W*H final variance (the last pass writes it; may be null)
  float4* guide;         // W*H: mean normal.xyz, mean depth (k_dv_prepare writes it)
  float4* img[2];        // W*H each, ping-pong: e.rgb, mean coverage k
  float* var[2];         // W*H each, ping-pong: the variance of l(e) (0 where k < 0.5)
  int32_t w, h;
  float spp;             // float(samples per pixel) of the inputs
  int32_t normal_power_log2, demodulate;
  int32_t spatial;       // 1: v0 is the 7x7 spatial estimate (spp < spatial_below)
  float sigma_lum, sigma_depth, albedo_eps;
};

constexpr int kDvMaxIterations = 8;

// float4 + float elements of the working images per pixel: guide and two
// images, two variance planes.
constexpr size_t kDvWorkBytesPerPixel = 3 * sizeof(float4) + 2 * sizeof(float);

#ifndef RTG_HOST_EMU
// The initial variance (k_dv_prepare, k_dv_spatial in the spatial case) and
// `iterations` (0..kDvMaxIterations) passes on `st`, one launch each.  With 0
// iterations nothing is written to a.out / a.out_var: the variance is left
// in a.var[0] for the caller to copy.
hipError_t launch_denoise_var(const DvArgs& a, int iterations, int num_cus, hipStream_t st);
#endif

}  // namespace rtg
