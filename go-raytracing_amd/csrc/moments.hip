// moments.hip — the moments mode of a render (rt_render_moments): per listed
// pixel m1 = sum_s Y_s and m2 = sum_s Y_s^2 over the call's samples, with
//   Y = (0.2126 * L.x + 0.7152 * L.y) + 0.0722 * L.z
// of the sample's finished radiance L = Lout[s * npix + pi], in fp64
// (-ffp-contract=off: the products and sums as written, no fused
// multiply-add).  The render itself is untouched: after a batch's last bounce
// k_moment_accum reads the Lout entries k_accum reads, in k_accum's order, so
// the moments are as independent of the schedule as the frame is; after the
// last batch k_moment_finalize rounds each moment to float once and scatters
// it through the pixel list (k_finalize's expression, `accumulate` included).
// One listed pixel per lane: each sample's load is one coalesced 16-B load
// per lane, 2 fp64 of state per pixel kept in the context between batches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "moments.h"

namespace rtg {

__global__ __launch_bounds__(256) void k_moment_accum(const float4* Lout, uint32_t npix, uint32_t nsamp, double* acc) {
  const uint32_t gs = gridDim.x * blockDim.x;
  for (uint32_t pi = blockIdx.x * blockDim.x + threadIdx.x; pi < npix; pi += gs) {
    double m1 = acc[size_t(pi) * kMomFloats], m2 = acc[size_t(pi) * kMomFloats + 1];
    for (uint32_t s = 0; s < nsamp; ++s) {
      const float4 L = Lout[size_t(s) * npix + pi];
      const double Y = (0.2126 * double(L.x) + 0.7152 * double(L.y)) + 0.0722 * double(L.z);
      m1 += Y;
      m2 += Y * Y;
    }
    acc[size_t(pi) * kMomFloats] = m1;
    acc[size_t(pi) * kMomFloats + 1] = m2;
  }
}

__global__ __launch_bounds__(256) void k_moment_finalize(const double* acc, const uint32_t* pixels, uint32_t npix,
                                                         float* out, int accumulate) {
  const uint32_t gs = gridDim.x * blockDim.x;
  for (uint32_t pi = blockIdx.x * blockDim.x + threadIdx.x; pi < npix; pi += gs) {
    float* o = out + size_t(pixels[pi]) * kMomFloats;
    double m1 = acc[size_t(pi) * kMomFloats], m2 = acc[size_t(pi) * kMomFloats + 1];
    if (accumulate) { m1 += double(o[0]); m2 += double(o[1]); }
    o[0] = float(m1);
    o[1] = float(m2);
  }
}

static int mom_grid(uint32_t items, int cus) {
  const long long need = (items + 255u) / 256u, cap = (long long)(cus > 0 ? cus : 256) * 8;
  return int(need < 1 ? 1 : need < cap ? need : cap);
}

hipError_t launch_moment_accum(const float4* Lout, uint32_t npix, uint32_t nsamp, double* acc, int num_cus,
                               hipStream_t st) {
  if (npix == 0) return hipSuccess;
  hipLaunchKernelGGL(k_moment_accum, dim3(mom_grid(npix, num_cus)), dim3(256), 0, st, Lout, npix, nsamp, acc);
  return hipGetLastError();
}

hipError_t launch_moment_finalize(const double* acc, const uint32_t* pixels, uint32_t npix, float* out, int accumulate,
                                  int num_cus, hipStream_t st) {
  if (npix == 0) return hipSuccess;
  hipLaunchKernelGGL(k_moment_finalize, dim3(mom_grid(npix, num_cus)), dim3(256), 0, st, acc, pixels, npix, out,
                     accumulate);
  return hipGetLastError();
}

}  // namespace rtg
