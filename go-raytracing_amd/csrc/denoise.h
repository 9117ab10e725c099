// denoise.h — launch interface of denoise.hip (rt_denoise): the edge-avoiding
// a-trous filter over a frame's radiance sums, guided by its feature image.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtg {

// What every pass of one rt_denoise call shares.
struct DnArgs {
  const float* accum;   // W*H*3 radiance sums (the call's input)
  const float* feat;    // W*H*8 feature sums (16-B aligned: read as two float4 per pixel)
  float* out;           // W*H*3 filtered sums (the last pass writes it)
  float4* guide;        // W*H: mean normal.xyz, mean depth (the first pass writes it)
  float4* img[2];       // W*H each, ping-pong: e.rgb, mean coverage k
  int32_t w, h;
  float spp;            // float(samples per pixel) of both inputs
  int32_t normal_power_log2, demodulate;
  float sigma_color, sigma_depth, albedo_eps;
};

// One pass.
struct DnPass {
  const float4* src;    // the previous pass's image (null in the first pass: the taps come from accum / feat)
  float4* dst;          // this pass's image (null in the last pass: the result goes to DnArgs::out)
  int32_t step;         // 2^i
  float sig2;           // (sigma_color * 2^-i)^2 + 1e-8
};

constexpr int kDnMaxIterations = 8;

#ifndef RTG_HOST_EMU
// `iterations` (1..kDnMaxIterations) passes on `st`, one launch each.
hipError_t launch_denoise(const DnArgs& a, int iterations, int num_cus, hipStream_t st);
#endif

}  // namespace rtg
