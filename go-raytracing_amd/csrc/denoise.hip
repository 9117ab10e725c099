// denoise.hip — rt_denoise: an edge-avoiding a-trous wavelet filter
// (Dammertz et al. 2010) over a frame's radiance sums, guided by the feature
// image rt_render_features returns (features.hip).
//
// Per-pixel means c = accum / spp and a, n, z, k = feat / spp (albedo, normal
// (not renormalised), depth, coverage).  A pixel with k < 0.5 (sky, emitters:
// noise-free at the camera ray) is copied to the output bit for bit and is
// never a neighbour.  The others filter e = c / max(a, albedo_eps) per
// channel (demodulate; else e = c): for i = 0 .. iterations - 1, step s = 2^i,
//   e'(p) = sum_q h(q) w(p, q) e(q) / sum_q h(q) w(p, q)
// over the 5x5 taps q = p + (dx, dy) * s, row-major with dy outer, taps outside
// the image skipped; h = outer product of [1/16, 1/4, 3/8, 1/4, 1/16];
//   w = w_n * w_z * w_c (1 for the centre tap)
//   w_n = max(0, n_p . n_q)^(2^normal_power_log2), by squarings
//   w_z = exp(-|z_p - z_q| / (sigma_depth * |z_p| + 1e-6))
//   w_c = exp(-|e_p - e_q|^2 / (sigma_i^2 + 1e-8)), sigma_i = sigma_color * 2^-i
// and the output is e * max(a, albedo_eps) * spp (e * spp without
// demodulation): sums again.  All fp32, -ffp-contract=off;
// tests/denoise_ref.py restates it in numpy with the same operation order.
//
// One launch per iteration.  The first pass reads the caller's arrays
// (demodulating each tap) and writes the packed guide image (n.xyz, z) beside
// its result; later passes read 32 B per tap as two 16-B loads: e.rgb + k from
// the previous pass's image, n.xyz + z from the guide.  The last pass
// remodulates into the caller's W*H*3 array.  Lanes map to consecutive pixels
// of a row, so each of a tap row's loads is coalesced.  No LDS tile: a block's
// 25 taps per pixel fall on 5 rows of 256 + 4 * step pixels, which the
// CU's vector cache and the L2 serve (at steps >= 4 a haloed tile would not
// fit the LDS anyway).  Measured at 1200x675, 5 passes: 0.29 ms, a tenth of
// the 1-spp preview pass it follows, so the simpler kernel stays (DESIGN.md
// "Feature buffers and denoiser" has the numbers and what was not tried).
// The kernel is correct for any block and grid size (grid-stride loop): the
// host emulation (tests/denoise_emu.cpp) runs it with one lane per block.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "denoise.h"

namespace rtg {

struct DnTap {
  float ex, ey, ez, k;   // filtered quantity, mean coverage
  float nx, ny, nz, z;   // mean normal, mean depth
};

// Pixel q's data for a pass: from the caller's sums in the first pass, from
// the previous pass's image and the guide afterwards.
template <bool kFirst>
__device__ __forceinline__ DnTap dn_load(const DnArgs& a, const DnPass& ps, size_t q) {
  DnTap t;
  if (kFirst) {
    const float4* f4 = reinterpret_cast<const float4*>(a.feat);
    const float4 fa = f4[2 * q], fb = f4[2 * q + 1];
    const float* c = a.accum + 3 * q;
    t.nx = fa.w / a.spp; t.ny = fb.x / a.spp; t.nz = fb.y / a.spp; t.z = fb.z / a.spp;
    t.k = fb.w / a.spp;
    t.ex = c[0] / a.spp; t.ey = c[1] / a.spp; t.ez = c[2] / a.spp;
    if (a.demodulate) {
      const float ax = fa.x / a.spp, ay = fa.y / a.spp, az = fa.z / a.spp;
      t.ex = t.ex / (ax > a.albedo_eps ? ax : a.albedo_eps);
      t.ey = t.ey / (ay > a.albedo_eps ? ay : a.albedo_eps);
      t.ez = t.ez / (az > a.albedo_eps ? az : a.albedo_eps);
    }
  } else {
    const float4 e = ps.src[q], g = a.guide[q];
    t.ex = e.x; t.ey = e.y; t.ez = e.z; t.k = e.w;
    t.nx = g.x; t.ny = g.y; t.nz = g.z; t.z = g.w;
  }
  return t;
}

template <bool kFirst, bool kLast>
__global__ __launch_bounds__(256) void k_atrous(DnArgs a, DnPass ps) {
  const size_t n = size_t(a.w) * size_t(a.h);
  const size_t gs = size_t(gridDim.x) * blockDim.x;
  const float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += gs) {
    const int x = int(i % size_t(a.w)), y = int(i / size_t(a.w));
    const DnTap p = dn_load<kFirst>(a, ps, i);
    if (kFirst) a.guide[i] = make_float4(p.nx, p.ny, p.nz, p.z);
    if (p.k < 0.5f) {   // passed through: the caller's sums, bit for bit
      if (kLast) {
        a.out[3 * i] = a.accum[3 * i]; a.out[3 * i + 1] = a.accum[3 * i + 1]; a.out[3 * i + 2] = a.accum[3 * i + 2];
      } else {
        ps.dst[i] = make_float4(p.ex, p.ey, p.ez, p.k);
      }
      continue;
    }
    const float zden = a.sigma_depth * fabsf(p.z) + 1e-6f;
    float wsum = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
      const int qy = y + dy * ps.step;
      if (qy < 0 || qy >= a.h) continue;
      for (int dx = -2; dx <= 2; ++dx) {
        const int qx = x + dx * ps.step;
        if (qx < 0 || qx >= a.w) continue;
        float wgt = 1.0f;
        DnTap q = p;
        if (dx != 0 || dy != 0) {
          q = dn_load<kFirst>(a, ps, size_t(qy) * size_t(a.w) + size_t(qx));
          if (q.k < 0.5f) continue;
          const float d = (p.nx * q.nx + p.ny * q.ny) + p.nz * q.nz;
          float wn = d > 0.0f ? d : 0.0f;
          for (int r = 0; r < a.normal_power_log2; ++r) wn = wn * wn;
          const float wz = expf(-(fabsf(p.z - q.z) / zden));
          const float ux = p.ex - q.ex, uy = p.ey - q.ey, uz = p.ez - q.ez;
          const float d2 = (ux * ux + uy * uy) + uz * uz;
          const float wc = expf(-(d2 / ps.sig2));
          wgt = (wn * wz) * wc;
        }
        const float hw = (hk[dy + 2] * hk[dx + 2]) * wgt;
        wsum = wsum + hw;
        sx = sx + hw * q.ex; sy = sy + hw * q.ey; sz = sz + hw * q.ez;
      }
    }
    const float ox = sx / wsum, oy = sy / wsum, oz = sz / wsum;
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
    } else {
      ps.dst[i] = make_float4(ox, oy, oz, p.k);
    }
  }
}

// The passes of one call, shared by the product launcher and the host
// emulation: launch(first, last, pass) runs pass i.
template <class Launch>
inline void dn_for_each_pass(const DnArgs& a, int iterations, Launch&& launch) {
  for (int i = 0; i < iterations; ++i) {
    DnPass ps;
    const bool first = i == 0, last = i == iterations - 1;
    ps.src = first ? nullptr : a.img[(i - 1) & 1];
    ps.dst = last ? nullptr : a.img[i & 1];
    ps.step = 1 << i;
    const float sigma = ldexpf(a.sigma_color, -i);
    ps.sig2 = sigma * sigma + 1e-8f;
    launch(first, last, ps);
  }
}

#ifndef RTG_HOST_EMU
hipError_t launch_denoise(const DnArgs& a, int iterations, int num_cus, hipStream_t st) {
  const size_t n = size_t(a.w) * size_t(a.h);
  const size_t need = (n + 255) / 256, cap = size_t(num_cus > 0 ? num_cus : 256) * 32;
  const dim3 grid(uint32_t(need < cap ? need : cap)), block(256);
  dn_for_each_pass(a, iterations, [&](bool first, bool last, const DnPass& ps) {
    if (first && last) hipLaunchKernelGGL((k_atrous<true, true>), grid, block, 0, st, a, ps);
    else if (first) hipLaunchKernelGGL((k_atrous<true, false>), grid, block, 0, st, a, ps);
    else if (last) hipLaunchKernelGGL((k_atrous<false, true>), grid, block, 0, st, a, ps);
    else hipLaunchKernelGGL((k_atrous<false, false>), grid, block, 0, st, a, ps);
  });
  return hipGetLastError();
}
#endif

}  // namespace rtg
