// ray_source.hip — rt_ray_color's ray source: the caller's rays written as
// bounce 0's path stream, in front of the unchanged bounce loop of
// wavefront.hip (run_batches' ray mode).
//
// A render's bounce 0 has no stream: its kernels regenerate GetRay from the
// slot index.  Here the rays are data, so k_ray_source writes them out once as
// stream 0 in the later bounces' record format and bounce 0 runs the
// later-bounce kernels over it.  Per slot: two 16-B loads (the ray), one 16-B
// store (Lout = 0) and, for a ray that passes the guard, three 16-B stores
// (the stream record); all coalesced and non-temporal like the path streams.
// A ray with a non-finite component or a zero direction is left out of the
// stream (it traces nothing and its radiance stays 0): the valid rays of a
// 256-slot chunk keep their order and the chunks reserve their places with
// one atomic each (block_reserve2's scheme, one queue), so the stream follows
// the caller's ray order chunk by chunk and the XCD claim segments of
// k_extend see neighbouring rays together.  Stream order never changes a
// result.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_layout.h"
#include "device_common.h"
#include "wavefront.h"
#include "ray_source.h"

namespace rtg {
namespace rsrc {

#ifdef RTG_HOST_EMU
__device__ __forceinline__ float4 ldnt(const float4* p) { return *p; }
__device__ __forceinline__ void stnt(float4* p, float4 v) { *p = v; }
#else
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ldnt(const float4* p) {
  const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void stnt(float4* p, float4 v) {
  v4f w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, reinterpret_cast<v4f*>(p));
}
#endif

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// The guard at the ray load (query.hip's valid_ray without the interval: a
// path's interval is always (0.001, +inf)).
__device__ __forceinline__ bool valid_ray(float4 o4, float4 d4) {
  const bool fin = finite_f(o4.x) && finite_f(o4.y) && finite_f(o4.z) && finite_f(d4.x) && finite_f(d4.y) && finite_f(d4.z);
  const bool dir = d4.x != 0.0f || d4.y != 0.0f || d4.z != 0.0f;
  return fin && dir;
}

// wavefront.hip's pack_state(depth, 0, true): depth_left | bounce 0 << 16 | allow << 31
__host__ __device__ constexpr uint32_t state0(int depth) { return uint32_t(depth & 0xFFFF) | 0x80000000u; }

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
  return uint32_t(__popcll(m & ((1ull << __lane_id()) - 1ull)));
}

}  // namespace rsrc

// 256-thread blocks in a grid-stride walk over 256-slot chunks; the trip count
// is block-uniform, so every thread reaches both barriers of every chunk.
static __global__ __launch_bounds__(256) void k_ray_source(WaveArgs a, RaySource src, uint32_t nslots, uint32_t sample_base) {
  __shared__ uint32_t s_w[2][4];   // per wave: its valid rays, then their offset in the chunk (double-buffered)
  __shared__ uint32_t s_b[2];      // the chunk's first stream position
  const uint32_t nchunks = (nslots + blockDim.x - 1u) / blockDim.x;
  const int w = int(threadIdx.x >> 6);
  uint32_t par = 0;
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x, par ^= 1u) {
    const uint32_t i = c * blockDim.x + threadIdx.x;
    bool valid = false;
    float4 o4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d4 = o4;
    if (i < nslots) {
      const uint32_t ray = a.pixels[i % a.npix];
      rsrc::stnt(&a.Lout[i], make_float4(0.0f, 0.0f, 0.0f, 0.0f));
      if (ray < src.num_rays) {
        o4 = rsrc::ldnt(&src.rays[2u * size_t(ray)]);
        d4 = rsrc::ldnt(&src.rays[2u * size_t(ray) + 1u]);
        valid = rsrc::valid_ray(o4, d4);
      }
    }
    const unsigned long long m = __ballot(valid);
    if (__lane_id() == 0) s_w[par][w] = uint32_t(__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) {
      const int nw = int((blockDim.x + 63u) >> 6);
      uint32_t tot = 0;
      for (int k = 0; k < nw; ++k) { const uint32_t n = s_w[par][k]; s_w[par][k] = tot; tot += n; }
      s_b[par] = tot ? atomicAdd(a.counts + CNT_STREAM0, tot) : 0u;
    }
    __syncthreads();
    if (valid) {
      // at most nslots valid rays in all: the position is below a.slots
      const uint32_t p = s_b[par] + s_w[par][w] + rsrc::lanes_below(m);
      const uint32_t key = path_key(a.seed, __float_as_uint(o4.w), sample_base + i / a.npix);
      rsrc::stnt(&a.s[0].o[p], make_float4(o4.x, o4.y, o4.z, __uint_as_float(i)));
      rsrc::stnt(&a.s[0].d[p], make_float4(d4.x, d4.y, d4.z, __uint_as_float(key)));
      rsrc::stnt(&a.s[0].beta[p], make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(rsrc::state0(a.max_depth))));
    }
  }
}

// The identity "pixel list" of a range: entry k names ray k.
static __global__ __launch_bounds__(256) void k_ray_identity(uint32_t* list, uint32_t n) {
  const uint32_t gs = gridDim.x * blockDim.x;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gs) list[k] = k;
}

#ifndef RTG_HOST_EMU
hipError_t launch_ray_identity(uint32_t* list, uint32_t n, int cus, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!list) return hipErrorInvalidValue;
  const long long need = (n + 255u) / 256u, resident = (long long)(cus > 0 ? cus : 1) * 8;
  hipLaunchKernelGGL(k_ray_identity, dim3(uint32_t(need < resident ? need : resident)), dim3(256), 0, st, list, n);
  return hipGetLastError();
}

hipError_t launch_ray_source(const WaveArgs& a, const RaySource& src, uint32_t nslots, uint32_t sample_base, int cus,
                             hipStream_t st) {
  if (nslots == 0) return hipSuccess;
  if (!src.rays || a.npix == 0 || nslots > a.slots || nslots % a.npix != 0) return hipErrorInvalidValue;
  // memory-bound and short: a few blocks per CU cover the latency, and never more than one per chunk
  const long long need = (nslots + 255u) / 256u, resident = (long long)(cus > 0 ? cus : 1) * 8;
  hipLaunchKernelGGL(k_ray_source, dim3(uint32_t(need < resident ? need : resident)), dim3(256), 0, st, a, src, nslots,
                     sample_base);
  return hipGetLastError();
}
#endif  // RTG_HOST_EMU

}  // namespace rtg
