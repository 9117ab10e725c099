// features.hip — the feature pass (rt_render_features): per-sample surface
// features of the camera ray's closest hit, for the denoiser (denoise.hip).
//
// The pass runs the production pipeline's camera-ray generation and bounce-0
// closest hit (wavefront.hip k_extend<kFirst>, launched by run_batches in its
// feature mode) and then, instead of k_shade, k_features: it reads the hit
// records k_extend wrote, applies the lifted volumes' test as k_shade and the
// path probe do, and builds the hit's record (make_record) and texture value
// (tex_value) exactly as shading would.  So the features belong to the very
// camera rays (path keys) a render with the same seed / sample_offset traces.
//   Lambertian / Isotropic: albedo = the texture value at the hit
//   Metal: Albedo; Dielectric: (1, 1, 1)
//   miss, DiffuseLight: all eight floats 0 (coverage 0: noise-free at the
//     camera ray, the denoiser passes such pixels through)
// normal = HitRecord.Normal (face-forwarded; (1, 0, 0) for a volume,
// volume.go:72-76; under a wrapper chain the geometric world-space normal,
// instance_normal below), depth = the reference's ray parameter t (direction
// not normalised).
// Sums follow k_accum / k_finalize: fp64 per listed pixel in slot order
// across the batches, one rounding to float per call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_layout.h"
#include "device_common.h"
#include "features.h"

namespace rtg {

// The guide normal of a hit under a wrapper chain (an instance): the
// object-space HitRecord.Normal mapped to world space by the chain's true
// inverse and renormalised.  The integrator's own normal there (make_record /
// unwrap_hit, the reference as written) is not a guide a filter can use:
// RotateX.Hit / RotateZ.Hit turn the normal by the ray's angle again instead
// of back (transform.go:256-265, :337-346), so it neither matches the surface
// nor faces the ray, and a sphere's (P - c) / r from the fp32 hit point is off
// unit length by up to ~1e-4 at CornellBox scale.  Rotations are orthogonal
// and Scale maps a normal by 1 / factor (transform.go:432-437), so the
// object-space face-forwarding (SetFaceNormal) carries over: n . rd < 0.
// Hits of world-space primitives keep HitRecord.Normal as it is.
__device__ __forceinline__ V3 instance_normal(const DScene& sc, const Best& b, V3 ro, V3 rd, float time) {
  const DInstance& in = sc.instances[GIX(b.inst, sc.n_instances, 21)];
  V3 o = ro, d = rd;
  to_object(in, o, d);
  Best bo = b;
  bo.inst = -1;
  V3 N = make_record<false>(sc, bo, o, d, time).N;   // object space, face-forwarded against the object-space ray
  for (int i = in.nwrap - 1; i >= 0; --i) {
    const float* p = in.prm[i];
    const float s = p[0], c = p[1];
    V3 m = N;
    switch (in.kind[i]) {
      case W_ROT_Y: m.x = c * N.x + s * N.z; m.z = -s * N.x + c * N.z; break;
      case W_ROT_X: m.y = c * N.y + s * N.z; m.z = -s * N.y + c * N.z; break;
      case W_ROT_Z: m.x = c * N.x + s * N.y; m.y = -s * N.x + c * N.y; break;
      case W_SCALE: m = mk(N.x * p[3], N.y * p[4], N.z * p[5]); break;
      default: break;   // W_TRANSLATE
    }
    N = m;
  }
  return unit(N);
}

// One path slot per lane, 256 per block: the hit record is one coalesced
// 16-B load, the feature record two coalesced 16-B stores.
__global__ __launch_bounds__(256) void k_features(DScene sc, DCamera cam, const float4* hit, const uint32_t* pixels,
                                                  uint32_t npix, uint32_t nslots, uint32_t seed, uint32_t sample_base,
                                                  float4* fa, float4* fb) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nslots) return;
  const uint32_t pix = pixels[i % npix];
  const uint32_t key = path_key(seed, pix, sample_base + i / npix);
  V3 ro, rd;
  float time;
  get_ray(cam, int(pix % uint32_t(cam.width)), int(pix / uint32_t(cam.width)), key, ro, rd, time);
  const float4 h = hit[i];
  uint32_t kh = __float_as_uint(h.y);
  float ht = h.x;
  int hinst = int(__float_as_uint(h.z)), hrefpos = int(__float_as_uint(h.w));
  Cnt cnt = {};
  if (sc.num_vol_refs > 0) lifted_volumes<false>(sc, ro, rd, key, 0u, kh, ht, hinst, hrefpos, cnt, sc.vol_recs);
  if (sc.num_prim_recs > 0) lifted_prims<false>(sc, ro, rd, time, kh, ht, hinst, hrefpos, cnt);
  float4 ra = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rb = ra;
  if (kh != 0u) {
    Best b{};
    b.t = ht; b.kind = int(kh >> 28); b.idx = int(kh & 0x0FFFFFFFu); b.inst = hinst;
    b.refpos = 0; b.primpos = 0;
    const Rec rec = make_record<true>(sc, b, ro, rd, time);
    const DMaterial& m = sc.materials[GIX(rec.mat, sc.num_materials, 42)];
    V3 alb = mk(0.0f, 0.0f, 0.0f);
    bool covered = true;
    if (m.kind == 1 || m.kind == 5) alb = tex_value<true>(sc, m.tex, rec.u, rec.v, rec.P);   // Lambertian, Isotropic
    else if (m.kind == 2) alb = ld3(m.albedo);                                               // Metal
    else if (m.kind == 3) alb = mk(1.0f, 1.0f, 1.0f);                                        // Dielectric
    else covered = false;                                                                    // DiffuseLight
    if (covered) {
      const bool wrapped = b.inst >= 0 && b.kind != PK_PLANE && b.kind != PK_VOLUME;
      const V3 N = wrapped ? instance_normal(sc, b, ro, rd, time) : rec.N;
      ra = make_float4(alb.x, alb.y, alb.z, N.x);
      rb = make_float4(N.y, N.z, ht, 1.0f);
    }
  }
  fa[i] = ra;
  fb[i] = rb;
}

__global__ __launch_bounds__(256) void k_feat_accum(const float4* fa, const float4* fb, uint32_t npix, uint32_t nsamp,
                                                    double* acc) {
  const uint32_t gs = gridDim.x * blockDim.x;
  for (uint32_t pi = blockIdx.x * blockDim.x + threadIdx.x; pi < npix; pi += gs) {
    double s[kFeatFloats];
    for (int k = 0; k < kFeatFloats; ++k) s[k] = acc[size_t(pi) * kFeatFloats + k];
    for (uint32_t q = 0; q < nsamp; ++q) {
      const float4 a = fa[size_t(q) * npix + pi], b = fb[size_t(q) * npix + pi];
      s[0] += double(a.x); s[1] += double(a.y); s[2] += double(a.z); s[3] += double(a.w);
      s[4] += double(b.x); s[5] += double(b.y); s[6] += double(b.z); s[7] += double(b.w);
    }
    for (int k = 0; k < kFeatFloats; ++k) acc[size_t(pi) * kFeatFloats + k] = s[k];
  }
}

__global__ __launch_bounds__(256) void k_feat_finalize(const double* acc, const uint32_t* pixels, uint32_t npix,
                                                       float* out, int accumulate) {
  const uint32_t gs = gridDim.x * blockDim.x;
  for (uint32_t pi = blockIdx.x * blockDim.x + threadIdx.x; pi < npix; pi += gs) {
    float* o = out + size_t(pixels[pi]) * kFeatFloats;
    for (int k = 0; k < kFeatFloats; ++k) {
      double s = acc[size_t(pi) * kFeatFloats + k];
      if (accumulate) s += double(o[k]);
      o[k] = float(s);
    }
  }
}

static int feat_grid(uint32_t items, int cus) {
  const long long need = (items + 255u) / 256u, cap = (long long)(cus > 0 ? cus : 256) * 8;
  return int(need < 1 ? 1 : need < cap ? need : cap);
}

hipError_t launch_features(const DScene& sc, const DCamera& cam, const float4* hit, const uint32_t* pixels,
                           uint32_t npix, uint32_t nslots, uint32_t seed, uint32_t sample_base, float4* fa,
                           float4* fb, hipStream_t st) {
  if (nslots == 0) return hipSuccess;
  hipLaunchKernelGGL(k_features, dim3((nslots + 255u) / 256u), dim3(256), 0, st, sc, cam, hit, pixels, npix, nslots,
                     seed, sample_base, fa, fb);
  return hipGetLastError();
}

hipError_t launch_feat_accum(const float4* fa, const float4* fb, uint32_t npix, uint32_t nsamp, double* acc,
                             int num_cus, hipStream_t st) {
  if (npix == 0) return hipSuccess;
  hipLaunchKernelGGL(k_feat_accum, dim3(feat_grid(npix, num_cus)), dim3(256), 0, st, fa, fb, npix, nsamp, acc);
  return hipGetLastError();
}

hipError_t launch_feat_finalize(const double* acc, const uint32_t* pixels, uint32_t npix, float* out, int accumulate,
                                int num_cus, hipStream_t st) {
  if (npix == 0) return hipSuccess;
  hipLaunchKernelGGL(k_feat_finalize, dim3(feat_grid(npix, num_cus)), dim3(256), 0, st, acc, pixels, npix, out,
                     accumulate);
  return hipGetLastError();
}

}  // namespace rtg
