// ray_source.hip — the ray sources of rt_ray_color and rt_gather: the caller's
// rays, or rays drawn per sample from the caller's points, written as bounce
// 0's path stream, in front of the unchanged bounce loop of wavefront.hip
// (run_batches' ray mode).
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
// result.  Behind the bounce loop, rt_gather_sh's projection of the finished
// radiances onto the SH basis (k_sh_accum, k_sh_finalize, below).
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

// One record under one source kind (ray_source.h's SRC_*) and the sample's
// path key: is there a ray, and which.  SRC_CALLER: the record is the ray.
// rt_gather's sources (rtgpu.h): the origin is the point; SRC_RAY's direction
// is the normal as given, SRC_COSINE's is unit(n) + RandomUnitVector
// (Lambertian.Scatter's direction, material.go:33-80: density cos/pi about
// unit(n)) and SRC_SPHERE's is RandomUnitVector alone, drawn at the key's
// (bounce 0, DOM_SOURCE, 0).  A point with a non-finite component, or, where
// the normal is read, a normal with one or with a length that len() gives as 0
// or not finite, has no ray (and draws nothing).  fp32 in the order written.
// `kind` is launch-uniform: a constant where the caller is a template.
__device__ __forceinline__ bool source_ray(int kind, float4 o4, float4 d4, uint32_t key, V3& ro, V3& rd) {
  ro = mk(o4.x, o4.y, o4.z);
  rd = mk(d4.x, d4.y, d4.z);
  if (kind == SRC_CALLER) return rsrc::valid_ray(o4, d4);
  bool ok = rsrc::finite_f(o4.x) && rsrc::finite_f(o4.y) && rsrc::finite_f(o4.z);
  if (kind != SRC_SPHERE) {
    const float l = len(rd);
    ok = ok && rsrc::finite_f(d4.x) && rsrc::finite_f(d4.y) && rsrc::finite_f(d4.z) && l != 0.0f && rsrc::finite_f(l);
  }
  if (ok && kind == SRC_COSINE) {
    const V3 nh = unit(rd);
    const V3 d = add(nh, random_unit_vector(key, 0u, DOM_SOURCE, 0u));
    rd = near_zero(d) ? nh : d;
  }
  if (ok && kind == SRC_SPHERE) rd = random_unit_vector(key, 0u, DOM_SOURCE, 0u);
  return ok;
}

// 256-thread blocks in a grid-stride walk over 256-slot chunks; the trip count
// is block-uniform, so every thread reaches both barriers of every chunk.  A
// generated direction (kKind != SRC_CALLER) is complete, rejection loop and
// all, before the vote: lanes diverge inside source_ray and nowhere else.
// bdim, gdim: the kernel's blockDim.x and gridDim.x, read in the kernel itself
// (read here they compile to the non-uniform-block form and k_ray_source's
// code would change).
template <int kKind>
__device__ __forceinline__ void ray_source_chunks(const WaveArgs& a, const RaySource& src, uint32_t nslots, uint32_t sample_base,
                                                  uint32_t bdim, uint32_t gdim) {
  __shared__ uint32_t s_w[2][4];   // per wave: its valid rays, then their offset in the chunk (double-buffered)
  __shared__ uint32_t s_b[2];      // the chunk's first stream position
  const uint32_t nchunks = (nslots + bdim - 1u) / bdim;
  const int w = int(threadIdx.x >> 6);
  uint32_t par = 0;
  for (uint32_t c = blockIdx.x; c < nchunks; c += gdim, par ^= 1u) {
    const uint32_t i = c * bdim + threadIdx.x;
    bool valid = false;
    float4 o4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d4 = o4;
    uint32_t key = 0u;
    if (i < nslots) {
      const uint32_t ray = a.pixels[i % a.npix];
      rsrc::stnt(&a.Lout[i], make_float4(0.0f, 0.0f, 0.0f, 0.0f));
      if (ray < src.num_rays) {
        o4 = rsrc::ldnt(&src.rays[2u * size_t(ray)]);
        d4 = rsrc::ldnt(&src.rays[2u * size_t(ray) + 1u]);
        if (kKind == SRC_CALLER) {
          valid = rsrc::valid_ray(o4, d4);
        } else if (kKind == SRC_SURFACE) {
          // no ray and no draw: the record stays a vertex, (p, unit(n)), under
          // the guard of the sources that read the normal (source_ray's SRC_RAY)
          V3 ro, rd;
          key = path_key(a.seed, __float_as_uint(o4.w), sample_base + i / a.npix);
          valid = source_ray(SRC_RAY, o4, d4, key, ro, rd);
          if (valid) rd = unit(rd);
          d4 = make_float4(rd.x, rd.y, rd.z, d4.w);
        } else {   // the ray's origin is the point; its direction takes the normal's place
          V3 ro, rd;
          key = path_key(a.seed, __float_as_uint(o4.w), sample_base + i / a.npix);
          valid = source_ray(kKind, o4, d4, key, ro, rd);
          d4 = make_float4(rd.x, rd.y, rd.z, d4.w);
        }
      }
    }
    const unsigned long long m = __ballot(valid);
    if (__lane_id() == 0) s_w[par][w] = uint32_t(__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) {
      const int nw = int((bdim + 63u) >> 6);
      uint32_t tot = 0;
      for (int k = 0; k < nw; ++k) { const uint32_t n = s_w[par][k]; s_w[par][k] = tot; tot += n; }
      s_b[par] = tot ? atomicAdd(a.counts + CNT_STREAM0, tot) : 0u;
    }
    __syncthreads();
    if (valid) {
      // at most nslots valid rays in all: the position is below a.slots
      const uint32_t p = s_b[par] + s_w[par][w] + rsrc::lanes_below(m);
      if (kKind == SRC_CALLER) key = path_key(a.seed, __float_as_uint(o4.w), sample_base + i / a.npix);
      rsrc::stnt(&a.s[0].o[p], make_float4(o4.x, o4.y, o4.z, __uint_as_float(i)));
      rsrc::stnt(&a.s[0].d[p], make_float4(d4.x, d4.y, d4.z, __uint_as_float(key)));
      rsrc::stnt(&a.s[0].beta[p], make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(rsrc::state0(a.max_depth))));
    }
  }
}

// rt_ray_color's source: the caller's rays.
static __global__ __launch_bounds__(256) void k_ray_source(WaveArgs a, RaySource src, uint32_t nslots, uint32_t sample_base) {
  ray_source_chunks<SRC_CALLER>(a, src, nslots, sample_base, blockDim.x, gridDim.x);
}

// rt_gather's sources: one kernel per kind (SRC_RAY, SRC_COSINE, SRC_SPHERE),
// and rt_gather_surface's (SRC_SURFACE): stream 0 gets (p, slot), (unit(n),
// key), (1, 1, 1, state) for k_shade's surface instantiation, which runs in
// bounce 0's k_extend's place (wavefront.hip, AT_SURFACE).
template <int kKind>
static __global__ __launch_bounds__(256) void k_gather_source(WaveArgs a, RaySource src, uint32_t nslots, uint32_t sample_base) {
  static_assert(kKind == SRC_RAY || kKind == SRC_COSINE || kKind == SRC_SPHERE || kKind == SRC_SURFACE, "a gather source");
  ray_source_chunks<kKind>(a, src, nslots, sample_base, blockDim.x, gridDim.x);
}

// rt_gather_rays: the ray sample `sample` of every point traces, one point per
// thread and trip: two 16-B loads, two 16-B stores, neighbours adjacent.
static __global__ __launch_bounds__(256) void k_gather_rays(const float4* pts, uint32_t n, int kind, uint32_t seed,
                                                            uint32_t sample, float4* out) {
  const uint32_t gs = gridDim.x * blockDim.x;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gs) {
    const float4 o4 = rsrc::ldnt(&pts[2u * size_t(k)]);
    const float4 d4 = rsrc::ldnt(&pts[2u * size_t(k) + 1u]);
    V3 ro, rd;
    const bool valid = source_ray(kind, o4, d4, path_key(seed, __float_as_uint(o4.w), sample), ro, rd);
    if (!valid) rd = mk(0.0f, 0.0f, 0.0f);
    rsrc::stnt(&out[2u * size_t(k)], o4);   // (p, id) as given, so rt_ray_color's guard sees what this one saw
    rsrc::stnt(&out[2u * size_t(k) + 1u], make_float4(rd.x, rd.y, rd.z, __uint_as_float(0u)));
  }
}

// ---- rt_gather_sh: the SH projection of a probe (rtgpu.h) -------------------
// The render is rt_gather's under SRC_SPHERE, untouched.  After a batch's last
// bounce k_sh_accum reads the Lout entries k_accum reads, in k_accum's order,
// and weights each sample's radiance with the SH basis at the sample's
// direction, which it draws again from the key through source_ray: the path
// streams carry no bounce-0 direction and gain none.  One listed point per
// lane: per point one 16-B load of the record's first half (p, id) and
// 3 * kBands^2 fp64 sums in registers over the sample loop (kBands is a
// template parameter so that one band does not carry nine bands' registers);
// per sample one coalesced 16-B load of Lout, one direction and 3 * kBands^2
// fp64 multiply-adds (the product of two floats is exact in fp64).  The sums
// live between batches in acc[(k * 3 + c) * npix + pi], coefficient-major, so
// the lanes of a wave load and store adjacent doubles.  An invalid point is
// skipped before any draw: its sums stay 0.
namespace shp {

// The basis of rtgpu.h in fp32, in the order written (-ffp-contract=off).
template <int kBands>
__device__ __forceinline__ void basis(V3 d, float (&Y)[kBands * kBands]) {
  const float x = d.x, y = d.y, z = d.z;
  Y[0] = 0.282095f;
  if constexpr (kBands >= 2) {
    Y[1] = 0.488603f * y;
    Y[2] = 0.488603f * z;
    Y[3] = 0.488603f * x;
  }
  if constexpr (kBands >= 3) {
    Y[4] = 1.092548f * (x * y);
    Y[5] = 1.092548f * (y * z);
    Y[6] = 0.315392f * (3.0f * (z * z) - 1.0f);
    Y[7] = 1.092548f * (x * z);
    Y[8] = 0.546274f * (x * x - y * y);
  }
}

}  // namespace shp

template <int kBands>
static __global__ __launch_bounds__(256) void k_sh_accum(const float4* Lout, const uint32_t* pixels, RaySource src,
                                                         uint32_t npix, uint32_t nsamp, uint32_t seed, uint32_t sample_base,
                                                         double* acc) {
  static_assert(kBands >= 1 && kBands <= 3, "rtgpu.h's RT_SH_MAX_BANDS");
  constexpr int K = kBands * kBands;
  const uint32_t gs = gridDim.x * blockDim.x;
  for (uint32_t pi = blockIdx.x * blockDim.x + threadIdx.x; pi < npix; pi += gs) {
    const uint32_t ray = pixels[pi];
    if (ray >= src.num_rays) continue;
    const float4 o4 = rsrc::ldnt(&src.rays[2u * size_t(ray)]);
    if (!(rsrc::finite_f(o4.x) && rsrc::finite_f(o4.y) && rsrc::finite_f(o4.z))) continue;   // source_ray's guard, before any draw
    double a[K * 3];
#pragma unroll
    for (int j = 0; j < K * 3; ++j) a[j] = acc[size_t(j) * npix + pi];
    for (uint32_t s = 0; s < nsamp; ++s) {
      const float4 L = Lout[size_t(s) * npix + pi];
      V3 ro, rd;
      source_ray(SRC_SPHERE, o4, o4, path_key(seed, __float_as_uint(o4.w), sample_base + s), ro, rd);   // n is not read
      float Y[K];
      shp::basis<kBands>(rd, Y);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double y = double(Y[k]);
        a[k * 3] += double(L.x) * y;
        a[k * 3 + 1] += double(L.y) * y;
        a[k * 3 + 2] += double(L.z) * y;
      }
    }
#pragma unroll
    for (int j = 0; j < K * 3; ++j) acc[size_t(j) * npix + pi] = a[j];
  }
}

// out[pixels[pi] * nc + j] = float(acc[j * npix + pi] (+ out with `accumulate`))
// for the nc = 3 * bands^2 sums of each listed point (k_finalize's expression).
static __global__ __launch_bounds__(256) void k_sh_finalize(const double* acc, const uint32_t* pixels, uint32_t npix,
                                                            uint32_t nc, float* out, int accumulate) {
  const uint32_t gs = gridDim.x * blockDim.x;
  for (uint32_t pi = blockIdx.x * blockDim.x + threadIdx.x; pi < npix; pi += gs) {
    float* o = out + size_t(pixels[pi]) * nc;
    for (uint32_t j = 0; j < nc; ++j) {
      double v = acc[size_t(j) * npix + pi];
      if (accumulate) v += double(o[j]);
      o[j] = float(v);
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
  const dim3 grid(uint32_t(need < resident ? need : resident)), block(256);
  switch (src.kind) {
    case SRC_CALLER: hipLaunchKernelGGL(k_ray_source, grid, block, 0, st, a, src, nslots, sample_base); break;
    case SRC_RAY: hipLaunchKernelGGL(k_gather_source<SRC_RAY>, grid, block, 0, st, a, src, nslots, sample_base); break;
    case SRC_COSINE: hipLaunchKernelGGL(k_gather_source<SRC_COSINE>, grid, block, 0, st, a, src, nslots, sample_base); break;
    case SRC_SPHERE: hipLaunchKernelGGL(k_gather_source<SRC_SPHERE>, grid, block, 0, st, a, src, nslots, sample_base); break;
    case SRC_SURFACE: hipLaunchKernelGGL(k_gather_source<SRC_SURFACE>, grid, block, 0, st, a, src, nslots, sample_base); break;
    default: return hipErrorInvalidValue;   // a missing kernel is an error
  }
  return hipGetLastError();
}

hipError_t launch_gather_rays(const float4* pts, uint32_t n, int32_t kind, uint32_t seed, uint32_t sample, float4* out,
                              int cus, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!pts || !out || kind < SRC_RAY || kind > SRC_SPHERE) return hipErrorInvalidValue;
  const long long need = (n + 255u) / 256u, resident = (long long)(cus > 0 ? cus : 1) * 8;
  hipLaunchKernelGGL(k_gather_rays, dim3(uint32_t(need < resident ? need : resident)), dim3(256), 0, st, pts, n, int(kind),
                     seed, sample, out);
  return hipGetLastError();
}

hipError_t launch_sh_accum(const WaveArgs& a, const RaySource& src, uint32_t nsamp, uint32_t sample_base, int bands,
                           double* acc, int cus, hipStream_t st) {
  if (a.npix == 0 || nsamp == 0) return hipSuccess;
  if (!src.rays || !acc || src.kind != SRC_SPHERE || size_t(nsamp) * a.npix > a.slots) return hipErrorInvalidValue;
  const long long need = (a.npix + 255u) / 256u, resident = (long long)(cus > 0 ? cus : 1) * 8;
  const dim3 grid(uint32_t(need < resident ? need : resident)), block(256);
  switch (bands) {
    case 1: hipLaunchKernelGGL(k_sh_accum<1>, grid, block, 0, st, a.Lout, a.pixels, src, a.npix, nsamp, a.seed, sample_base, acc); break;
    case 2: hipLaunchKernelGGL(k_sh_accum<2>, grid, block, 0, st, a.Lout, a.pixels, src, a.npix, nsamp, a.seed, sample_base, acc); break;
    case 3: hipLaunchKernelGGL(k_sh_accum<3>, grid, block, 0, st, a.Lout, a.pixels, src, a.npix, nsamp, a.seed, sample_base, acc); break;
    default: return hipErrorInvalidValue;   // a missing kernel is an error
  }
  return hipGetLastError();
}

hipError_t launch_sh_finalize(const double* acc, const uint32_t* pixels, uint32_t npix, int bands, float* out,
                              int accumulate, int cus, hipStream_t st) {
  if (npix == 0) return hipSuccess;
  if (!acc || !pixels || !out || bands < 1 || bands > kShMaxBands) return hipErrorInvalidValue;
  const long long need = (npix + 255u) / 256u, resident = (long long)(cus > 0 ? cus : 1) * 8;
  hipLaunchKernelGGL(k_sh_finalize, dim3(uint32_t(need < resident ? need : resident)), dim3(256), 0, st, acc, pixels, npix,
                     uint32_t(sh_floats(bands)), out, accumulate);
  return hipGetLastError();
}
#endif  // RTG_HOST_EMU

}  // namespace rtg
