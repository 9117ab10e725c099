// probe.hip — the small kernels beside the wavefront pipeline
// (wavefront.hip, the render path):
//   * tonemap_kernel: the reference's RGBA8 quantisation of a pass
//     (bucket_renderer.go:276-285, utils.go:85-90) for rt_tonemap_rgba8;
//   * primary_kernel: the parity probe rt_primary_hits — one sample's
//     GetRay (camera.go:368-434) + closest hit (world.Hit, camera.go:449)
//     per pixel, through the same traversal as k_extend (device_common.h
//     traverse / trav_step), reporting the hit hittable ids and t.
// Arithmetic is fp32 in the Go operation order (-ffp-contract=off), which the
// CPU oracle's fp32 mode reproduces.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_layout.h"
#include "device_common.h"
#include "hit_ids.h"
#include "probe.h"

namespace rtg {

// ----------------------------------------------------------------------------
// Kernels
// ----------------------------------------------------------------------------
// bucket_renderer.go:276-285: scale 1/spp, LinearToGamma (utils.go:85-90),
// clamp [0,0.999], uint8(256*x) — in fp64 like the reference.
__global__ void tonemap_kernel(const float* accum, int n, int spp, uint8_t* rgba) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double sc = 1.0 / double(spp);
  uint8_t o[4];
  for (int c = 0; c < 3; ++c) {
    double v = double(accum[size_t(i) * 3 + c]) * sc;
    double g = v > 0.0 ? sqrt(v) : 0.0;
    if (g < 0.0) g = 0.0;
    if (g > 0.999) g = 0.999;
    o[c] = uint8_t(256.0 * g);
  }
  o[3] = 255;
  reinterpret_cast<uchar4*>(rgba)[i] = make_uchar4(o[0], o[1], o[2], o[3]);
}

// rt_render_rgba8: the same quantisation for the pixels of a bucket list only
// (one workgroup per bucket): pixels outside them keep the framebuffer's
// previous value, as renderBucketWithQuality writes only its bucket.
__global__ __launch_bounds__(256) void tonemap_buckets_kernel(const float* accum, int width, const int4* buckets,
                                                              int spp, uint8_t* rgba) {
  const int4 b = buckets[blockIdx.x];   // x, y, w, h
  const double sc = 1.0 / double(spp);
  for (int k = threadIdx.x; k < b.z * b.w; k += blockDim.x) {
    const size_t i = size_t(b.y + k / b.z) * size_t(width) + size_t(b.x + k % b.z);
    uint8_t o[4];
    for (int c = 0; c < 3; ++c) {
      const double v = double(accum[i * 3 + c]) * sc;
      double g = v > 0.0 ? sqrt(v) : 0.0;
      if (g < 0.0) g = 0.0;
      if (g > 0.999) g = 0.999;
      o[c] = uint8_t(256.0 * g);
    }
    o[3] = 255;
    reinterpret_cast<uchar4*>(rgba)[i] = make_uchar4(o[0], o[1], o[2], o[3]);
  }
}

// Path probes (rt_extend_hits / rt_shadow_visibility): one sample per pixel
// rendered to depth bounce + 1, so the records of bounce `bounce` are the
// last the pipeline wrote.  Pixels whose path ended before that bounce keep
// the fill values (ids -2, t -1, ray 0, no NEE rays).
__global__ __launch_bounds__(256) void path_fill_kernel(uint32_t n, int32_t* top, int32_t* prim, float* t, float* ray,
                                                        int32_t* nee) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  top[i] = -2;
  prim[i] = -2;
  t[i] = -1.0f;
  for (int k = 0; k < 6; ++k) ray[size_t(i) * 6 + k] = 0.0f;
  nee[i] = 0;
}

// k_extend's hit records of one bounce (wavefront.hip store_hit: t,
// kind<<28|idx, instance, TLAS ref position; stream position i < *count)
// -> hittable ids per pixel, with the lifted volumes' test applied as
// k_shade applies it (lifted_volumes), and the incoming ray: bounce 0
// regenerates the camera ray (slot i = pixel list entry i), later bounces
// read it from the stream k_extend traced (o.w = slot, d.w = path key).
__global__ __launch_bounds__(256) void path_hits_kernel(DScene sc, DCamera cam, const float4* hit, const float4* so,
                                                        const float4* sd, const uint32_t* count,
                                                        const uint32_t* pixels, uint32_t npix, uint32_t seed,
                                                        uint32_t sample, int bounce, int32_t* out_top,
                                                        int32_t* out_prim, float* out_t, float* out_ray) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= npix || i >= *count) return;   // one sample per pixel: at most npix paths
  uint32_t slot, key;
  V3 ro, rd;
  if (bounce == 0) {
    slot = i;
    const uint32_t pix = pixels[i];
    key = path_key(seed, pix, sample);
    float tm;
    get_ray(cam, int(pix % uint32_t(cam.width)), int(pix / uint32_t(cam.width)), key, ro, rd, tm);
  } else {
    const float4 o4 = so[i], d4 = sd[i];
    slot = __float_as_uint(o4.w);
    key = __float_as_uint(d4.w);
    ro = mk(o4.x, o4.y, o4.z);
    rd = mk(d4.x, d4.y, d4.z);
  }
  const float4 h = hit[i];
  uint32_t kh = __float_as_uint(h.y);
  float ht = h.x;
  int hinst = int(__float_as_uint(h.z)), hrefpos = int(__float_as_uint(h.w));
  Cnt cnt = {};
  if (sc.num_vol_refs > 0) lifted_volumes<false>(sc, ro, rd, key, uint32_t(bounce), kh, ht, hinst, hrefpos, cnt, sc.vol_recs);
  if (sc.num_prim_recs > 0) lifted_prims<false>(sc, ro, rd, ray_time(key), kh, ht, hinst, hrefpos, cnt);   // as shade_path
  int top = -1, prim = -1;
  if (kh != 0u) hit_ids(sc, int(kh >> 28), int(kh & 0x0FFFFFFFu), hrefpos, top, prim);
  const uint32_t p = pixels[slot % npix];
  out_top[p] = top;
  out_prim[p] = prim;
  out_t[p] = kh ? ht : -1.0f;
  float* r = out_ray + size_t(p) * 6;
  r[0] = ro.x; r[1] = ro.y; r[2] = ro.z; r[3] = rd.x; r[4] = rd.y; r[5] = rd.z;
}

// The NEE jobs of one bounce (job j < *count): the shadow rays k_shade set
// up (sj_info bits 0 / 1: area-light / HDRI ray; a lifted volume that
// occludes a ray has already cleared its bit) and what k_shadow found
// (sj_vis bits: unoccluded) -> flags | vis << 2 per pixel.
__global__ __launch_bounds__(256) void nee_probe_kernel(const uint32_t* sj_info, const uint32_t* sj_vis,
                                                        const float4* ne_a, const uint32_t* count,
                                                        const uint32_t* pixels, uint32_t npix, int32_t* out_nee) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= npix || j >= *count) return;
  const uint32_t slot = __float_as_uint(ne_a[j].w);
  // (bits 2 / 3 of sj_info: the ray is occluded by a world primitive lifted out of the BVH that k_shadow
  // walked, WaveArgs::nee_probe)
  const uint32_t info = sj_info[j], occ = (info >> 2) & 3u;
  out_nee[pixels[slot % npix]] = int32_t((info & 3u) | ((sj_vis[j] & 3u & ~occ) << 2));
}

// Parity probe: first-bounce closest hit of one sample per pixel.
template <int STACK, bool kQuant>
__global__ __launch_bounds__(256) void primary_kernel(DScene sc, DCamera cam, uint32_t seed, int sample,
                                                      int32_t* out_top, int32_t* out_prim, float* out_t, int* err) {
  __shared__ uint32_t lds_stack[(STACK + kWorldRayWords + kHitWords) * 256];   // stack + world ray
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  if (i >= cam.width * cam.height) return;
  const int px = i % cam.width, py = i / cam.width;
  uint32_t key = path_key(seed, uint32_t(i), uint32_t(sample));
  V3 ro, rd;
  float time;
  get_ray(cam, px, py, key, ro, rd, time);
  Best b{};
  Cnt cnt = {};
  bool hit = traverse<false, false, true, kQuant>(sc, ro, rd, time, 0.001f, __builtin_inff(), lds_stack_only(lds_stack + tid, 256, STACK), b, key,
                                    0, DOM_VOL, cnt, err);
  int top = -1, prim = -1;
  if (hit) hit_ids(sc, b.kind, b.idx, b.refpos, top, prim);
  out_top[i] = top;
  out_prim[i] = prim;
  out_t[i] = hit ? b.t : -1.0f;
}

// ----------------------------------------------------------------------------
// Host launchers
// ----------------------------------------------------------------------------
hipError_t launch_tonemap(const float* accum, int n, int spp, uint8_t* rgba, hipStream_t st) {
  hipLaunchKernelGGL(tonemap_kernel, dim3((n + 255) / 256), dim3(256), 0, st, accum, n, spp, rgba);
  return hipGetLastError();
}

hipError_t launch_primary(const DScene& sc, const DCamera& cam, uint32_t seed, int sample, int32_t* top,
                          int32_t* prim, float* t, int* err, int stack, hipStream_t st) {
  int n = cam.width * cam.height;
  dim3 grid((n + 255) / 256), block(256);
  const bool q = sc.quant_nodes != 0;   // the node format the renders traverse
  if (stack <= 32) {
    if (q) hipLaunchKernelGGL((primary_kernel<32, true>), grid, block, 0, st, sc, cam, seed, sample, top, prim, t, err);
    else hipLaunchKernelGGL((primary_kernel<32, false>), grid, block, 0, st, sc, cam, seed, sample, top, prim, t, err);
  } else if (stack <= 64) {
    if (q) hipLaunchKernelGGL((primary_kernel<64, true>), grid, block, 0, st, sc, cam, seed, sample, top, prim, t, err);
    else hipLaunchKernelGGL((primary_kernel<64, false>), grid, block, 0, st, sc, cam, seed, sample, top, prim, t, err);
  } else {   // deep scenes (RotateX / RotateZ chains: two words per entry), 145 KB of LDS per block
    if (q) hipLaunchKernelGGL((primary_kernel<128, true>), grid, block, 0, st, sc, cam, seed, sample, top, prim, t, err);
    else hipLaunchKernelGGL((primary_kernel<128, false>), grid, block, 0, st, sc, cam, seed, sample, top, prim, t, err);
  }
  return hipGetLastError();
}

hipError_t launch_tonemap_buckets(const float* accum, int width, const int4* buckets, int nb, int spp, uint8_t* rgba,
                                  hipStream_t st) {
  if (nb <= 0) return hipSuccess;
  hipLaunchKernelGGL(tonemap_buckets_kernel, dim3(nb), dim3(256), 0, st, accum, width, buckets, spp, rgba);
  return hipGetLastError();
}

// Coalesced streaming read (16 B per lane, grid-stride, non-temporal as the
// path streams): the measured HBM read peak the bench line reports beside the
// 8 TB/s spec.  The sum is stored only if it equals a value no
// input produces, so the loads stay and nothing is written.
__global__ __launch_bounds__(256) void stream_read_kernel(const float4* __restrict__ src, size_t n, float* sink) {
  float s = 0.0f;
  const size_t gs = size_t(gridDim.x) * blockDim.x;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += gs) {
    typedef float v4 __attribute__((ext_vector_type(4)));
    const v4 v = __builtin_nontemporal_load(reinterpret_cast<const v4*>(src + i));
    s += v.x + v.y + v.z + v.w;
  }
  if (s == -1.2345e-38f) sink[0] = s;
}

hipError_t launch_stream_read(const float4* src, size_t n, float* sink, int reps, hipStream_t st) {
  int dev = 0, cus = 1;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 256;
  for (int r = 0; r < reps; ++r)
    hipLaunchKernelGGL(stream_read_kernel, dim3(cus * 8), dim3(256), 0, st, src, n, sink);
  return hipGetLastError();
}

hipError_t launch_path_fill(uint32_t n, int32_t* top, int32_t* prim, float* t, float* ray, int32_t* nee,
                            hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(path_fill_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, top, prim, t, ray, nee);
  return hipGetLastError();
}

hipError_t launch_path_hits(const DScene& sc, const DCamera& cam, const float4* hit, const float4* so, const float4* sd,
                            const uint32_t* count, const uint32_t* pixels, uint32_t npix, uint32_t seed,
                            uint32_t sample, int bounce, int32_t* top, int32_t* prim, float* t, float* ray,
                            hipStream_t st) {
  if (npix == 0) return hipSuccess;
  hipLaunchKernelGGL(path_hits_kernel, dim3((npix + 255u) / 256u), dim3(256), 0, st, sc, cam, hit, so, sd, count, pixels,
                     npix, seed, sample, bounce, top, prim, t, ray);
  return hipGetLastError();
}

hipError_t launch_nee_probe(const uint32_t* sj_info, const uint32_t* sj_vis, const float4* ne_a, const uint32_t* count,
                            const uint32_t* pixels, uint32_t npix, int32_t* nee, hipStream_t st) {
  if (npix == 0) return hipSuccess;
  hipLaunchKernelGGL(nee_probe_kernel, dim3((npix + 255u) / 256u), dim3(256), 0, st, sj_info, sj_vis, ne_a, count,
                     pixels, npix, nee);
  return hipGetLastError();
}

}  // namespace rtg
