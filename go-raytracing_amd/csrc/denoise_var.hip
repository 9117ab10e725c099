// denoise_var.hip — rt_denoise_variance: the spatial part of SVGF (Schied et
// al. 2017) over a frame's radiance sums: denoise.hip's a-trous filter with
// its colour weight replaced by a luminance weight scaled by the pixel's own
// standard deviation, and the variance carried through the passes.
//
// The means c, a, n, z, k, the pass-through rule k < 0.5, e = c / max(a,
// albedo_eps), the 5x5 B3 taps (row-major, dy outer, taps outside the image
// and uncovered taps skipped), w_n, w_z and the remodulation are denoise.hip's.
// l(e) = (0.2126 e.x + 0.7152 e.y) + 0.0722 e.z.
//
// k_dv_prepare: e, k -> img[0], n, z -> guide, and the initial variance v0 of
//   l(e_p) -> var[0] (0 for an uncovered pixel):
//     n = spp, mu = m1 / n, var_Y = max(0, m2 / n - mu * mu) / (n - 1)
//     v0 = (var_Y / max(mu * mu, 1e-12)) * (l(e_p) * l(e_p))
// k_dv_spatial (spp < spatial_below instead): over the 7x7 unit-step window,
//   row-major, w = w_n * w_z (1 for the centre), uncovered pixels skipped,
//     sw += w, s1 += w * l_q, s2 += w * (l_q * l_q)
//     v0 = max(0, s2 / sw - (s1 / sw) * (s1 / sw))
// k_dv_atrous, pass i, step 2^i:
//     g = sum_3x3 gw * v_q / sum_3x3 gw   (unit step; covered in-image neighbours;
//         gw = (1/4, 1/8, 1/16) * (w_n * w_z), 1/4 for the centre: the
//         prefilter stops at the edges the taps stop at, so a surface's
//         variance never widens its neighbour's weight)
//     w_l = exp(-(|l(e_p) - l(e_q)| / (sigma_lum * sqrt(g) + 1e-6)))
//     hw = (h_dy * h_dx) * ((w_n * w_z) * w_l)      (1 for the centre's weight)
//     e' = sum hw e_q / sum hw,  v' = sum (hw * hw) v_q / (sum hw * sum hw)
//   sigma_lum is not halved per pass: the shrinking variance narrows it.
// The last pass writes e * max(a, albedo_eps) * spp to `out` and v to
// `out_var`; a passed-through pixel keeps the caller's sums bit for bit and
// gets variance 0.  All fp32, -ffp-contract=off; tests/denoise_var_ref.py
// restates it in numpy with the same operation order.
//
// One launch per kernel above: prepare (+ spatial) + one per pass.  Every
// pass reads 36 B per tap (e.rgb + k, n.xyz + z as two 16-B loads, v as one
// 4-B load) with lanes on consecutive pixels of a row, so each tap row's loads
// are coalesced.  No LDS tile, as in denoise.hip: the unit-step stencils (the
// 7x7 estimate, the 3x3 prefilter) re-read rows that the CU's vector cache
// holds; a tiled variant was not tried (DESIGN.md "Radiance moments and the
// variance-guided filter").  The kernels use no LDS and no barrier and are
// correct for any block and grid size (grid-stride loops): the host emulation
// (tests/denoise_var_emu.cpp) runs them with one lane per block.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "denoise_var.h"

namespace rtg {

// One pass.
struct DvPass {
  const float4* src;    // the previous image (img[0] of k_dv_prepare for the first pass)
  float4* dst;          // this pass's image (null in the last pass: the result goes to DvArgs::out)
  const float* vsrc;    // the previous variance
  float* vdst;          // this pass's variance (null in the last pass: DvArgs::out_var, if any)
  int32_t step;         // 2^i
};

struct DvTap {
  float ex, ey, ez, k;   // filtered quantity, mean coverage
  float nx, ny, nz, z;   // mean normal, mean depth
};

__device__ __forceinline__ DvTap dv_load(const float4* img, const float4* guide, size_t q) {
  const float4 e = img[q], g = guide[q];
  DvTap t;
  t.ex = e.x; t.ey = e.y; t.ez = e.z; t.k = e.w;
  t.nx = g.x; t.ny = g.y; t.nz = g.z; t.z = g.w;
  return t;
}

__device__ __forceinline__ float dv_lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

// w_n * w_z of denoise.hip.
__device__ __forceinline__ float dv_geom(const DvArgs& a, const DvTap& p, const DvTap& q, float zden) {
  const float d = (p.nx * q.nx + p.ny * q.ny) + p.nz * q.nz;
  float wn = d > 0.0f ? d : 0.0f;
  for (int r = 0; r < a.normal_power_log2; ++r) wn = wn * wn;
  const float wz = expf(-(fabsf(p.z - q.z) / zden));
  return wn * wz;
}

__global__ __launch_bounds__(256) void k_dv_prepare(DvArgs a) {
  const size_t n = size_t(a.w) * size_t(a.h);
  const size_t gs = size_t(gridDim.x) * blockDim.x;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += gs) {
    const float4* f4 = reinterpret_cast<const float4*>(a.feat);
    const float4 fa = f4[2 * i], fb = f4[2 * i + 1];
    const float* c = a.accum + 3 * i;
    const float k = fb.w / a.spp;
    float ex = c[0] / a.spp, ey = c[1] / a.spp, ez = c[2] / a.spp;
    if (a.demodulate) {
      const float ax = fa.x / a.spp, ay = fa.y / a.spp, az = fa.z / a.spp;
      ex = ex / (ax > a.albedo_eps ? ax : a.albedo_eps);
      ey = ey / (ay > a.albedo_eps ? ay : a.albedo_eps);
      ez = ez / (az > a.albedo_eps ? az : a.albedo_eps);
    }
    a.guide[i] = make_float4(fa.w / a.spp, fb.x / a.spp, fb.y / a.spp, fb.z / a.spp);
    a.img[0][i] = make_float4(ex, ey, ez, k);
    float v = 0.0f;
    if (!a.spatial && !(k < 0.5f)) {
      const float mu = a.moments[2 * i] / a.spp;
      const float r = a.moments[2 * i + 1] / a.spp - mu * mu;
      const float vy = (r > 0.0f ? r : 0.0f) / (a.spp - 1.0f);
      const float mu2 = mu * mu;
      const float le = dv_lum(ex, ey, ez);
      v = (vy / (mu2 > 1e-12f ? mu2 : 1e-12f)) * (le * le);
    }
    a.var[0][i] = v;
  }
}

__global__ __launch_bounds__(256) void k_dv_spatial(DvArgs a) {
  const size_t n = size_t(a.w) * size_t(a.h);
  const size_t gs = size_t(gridDim.x) * blockDim.x;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += gs) {
    const int x = int(i % size_t(a.w)), y = int(i / size_t(a.w));
    const DvTap p = dv_load(a.img[0], a.guide, i);
    if (p.k < 0.5f) continue;   // k_dv_prepare left its variance 0
    const float zden = a.sigma_depth * fabsf(p.z) + 1e-6f;
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -3; dy <= 3; ++dy) {
      const int qy = y + dy;
      if (qy < 0 || qy >= a.h) continue;
      for (int dx = -3; dx <= 3; ++dx) {
        const int qx = x + dx;
        if (qx < 0 || qx >= a.w) continue;
        float wgt = 1.0f;
        DvTap q = p;
        if (dx != 0 || dy != 0) {
          q = dv_load(a.img[0], a.guide, size_t(qy) * size_t(a.w) + size_t(qx));
          if (q.k < 0.5f) continue;
          wgt = dv_geom(a, p, q, zden);
        }
        const float lq = dv_lum(q.ex, q.ey, q.ez);
        sw = sw + wgt;
        s1 = s1 + wgt * lq;
        s2 = s2 + wgt * (lq * lq);
      }
    }
    const float mean = s1 / sw;
    const float r = s2 / sw - mean * mean;
    a.var[0][i] = r > 0.0f ? r : 0.0f;
  }
}

template <bool kLast>
__global__ __launch_bounds__(256) void k_dv_atrous(DvArgs a, DvPass ps) {
  const size_t n = size_t(a.w) * size_t(a.h);
  const size_t gs = size_t(gridDim.x) * blockDim.x;
  const float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  const float gk[3] = {0.25f, 0.5f, 0.25f};
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += gs) {
    const int x = int(i % size_t(a.w)), y = int(i / size_t(a.w));
    const DvTap p = dv_load(ps.src, a.guide, i);
    if (p.k < 0.5f) {   // passed through: the caller's sums, bit for bit; variance 0
      if (kLast) {
        a.out[3 * i] = a.accum[3 * i]; a.out[3 * i + 1] = a.accum[3 * i + 1]; a.out[3 * i + 2] = a.accum[3 * i + 2];
        if (a.out_var) a.out_var[i] = 0.0f;
      } else {
        ps.dst[i] = make_float4(p.ex, p.ey, p.ez, p.k);
        ps.vdst[i] = 0.0f;
      }
      continue;
    }
    const float zden = a.sigma_depth * fabsf(p.z) + 1e-6f;
    // the 3x3 Gaussian of the variance around p
    float gsum = 0.0f, gw = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
      const int qy = y + dy;
      if (qy < 0 || qy >= a.h) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int qx = x + dx;
        if (qx < 0 || qx >= a.w) continue;
        const size_t qi = size_t(qy) * size_t(a.w) + size_t(qx);
        float wgt = 1.0f;
        if (dx != 0 || dy != 0) {
          const DvTap q = dv_load(ps.src, a.guide, qi);
          if (q.k < 0.5f) continue;
          wgt = dv_geom(a, p, q, zden);
        }
        const float wq = (gk[dy + 1] * gk[dx + 1]) * wgt;
        gw = gw + wq;
        gsum = gsum + wq * ps.vsrc[qi];
      }
    }
    const float lden = a.sigma_lum * sqrtf(gsum / gw) + 1e-6f;
    const float lp = dv_lum(p.ex, p.ey, p.ez);
    float wsum = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
      const int qy = y + dy * ps.step;
      if (qy < 0 || qy >= a.h) continue;
      for (int dx = -2; dx <= 2; ++dx) {
        const int qx = x + dx * ps.step;
        if (qx < 0 || qx >= a.w) continue;
        const size_t qi = size_t(qy) * size_t(a.w) + size_t(qx);
        float wgt = 1.0f;
        DvTap q = p;
        if (dx != 0 || dy != 0) {
          q = dv_load(ps.src, a.guide, qi);
          if (q.k < 0.5f) continue;
          const float wl = expf(-(fabsf(lp - dv_lum(q.ex, q.ey, q.ez)) / lden));
          wgt = dv_geom(a, p, q, zden) * wl;
        }
        const float hw = (hk[dy + 2] * hk[dx + 2]) * wgt;
        wsum = wsum + hw;
        sx = sx + hw * q.ex; sy = sy + hw * q.ey; sz = sz + hw * q.ez;
        sv = sv + (hw * hw) * ps.vsrc[qi];
      }
    }
    const float ox = sx / wsum, oy = sy / wsum, oz = sz / wsum;
    const float ov = sv / (wsum * wsum);
    if (kLast) {
      float mx = 1.0f, my = 1.0f, mz = 1.0f;
      if (a.demodulate) {
        const float4 fa = reinterpret_cast<const float4*>(a.feat)[2 * i];
        const float ax = fa.x / a.spp, ay = fa.y / a.spp, az = fa.z / a.spp;
        mx = ax > a.albedo_eps ? ax : a.albedo_eps;
        my = ay > a.albedo_eps ? ay : a.albedo_eps;
        mz = az > a.albedo_eps ? az : a.albedo_eps;
      }
      a.out[3 * i] = (ox * mx) * a.spp; a.out[3 * i + 1] = (oy * my) * a.spp; a.out[3 * i + 2] = (oz * mz) * a.spp;
      if (a.out_var) a.out_var[i] = ov;
    } else {
      ps.dst[i] = make_float4(ox, oy, oz, p.k);
      ps.vdst[i] = ov;
    }
  }
}

// The kernels of one call in order, shared by the product launcher and the
// host emulation: prepare(), spatial() if the call takes the spatial
// estimate, then pass(last, ps) for pass i (pass i reads img / var [i & 1]).
template <class Prepare, class Spatial, class Pass>
inline void dv_for_each_kernel(const DvArgs& a, int iterations, Prepare&& prepare, Spatial&& spatial, Pass&& pass) {
  prepare();
  if (a.spatial) spatial();
  for (int i = 0; i < iterations; ++i) {
    DvPass ps;
    const bool last = i == iterations - 1;
    ps.src = a.img[i & 1];
    ps.vsrc = a.var[i & 1];
    ps.dst = last ? nullptr : a.img[(i & 1) ^ 1];
    ps.vdst = last ? nullptr : a.var[(i & 1) ^ 1];
    ps.step = 1 << i;
    pass(last, ps);
  }
}

#ifndef RTG_HOST_EMU
hipError_t launch_denoise_var(const DvArgs& a, int iterations, int num_cus, hipStream_t st) {
  const size_t n = size_t(a.w) * size_t(a.h);
  const size_t need = (n + 255) / 256, cap = size_t(num_cus > 0 ? num_cus : 256) * 32;
  const dim3 grid(uint32_t(need < cap ? need : cap)), block(256);
  dv_for_each_kernel(
      a, iterations, [&] { hipLaunchKernelGGL(k_dv_prepare, grid, block, 0, st, a); },
      [&] { hipLaunchKernelGGL(k_dv_spatial, grid, block, 0, st, a); },
      [&](bool last, const DvPass& ps) {
        if (last) hipLaunchKernelGGL((k_dv_atrous<true>), grid, block, 0, st, a, ps);
        else hipLaunchKernelGGL((k_dv_atrous<false>), grid, block, 0, st, a, ps);
      });
  return hipGetLastError();
}
#endif

}  // namespace rtg
