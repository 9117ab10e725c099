// query.hip — ray queries: closest hit (rt_trace_rays) and occlusion
// (rt_occluded) for rays the caller supplies, through the render's own
// traversal (device_common.h trav_init / trav_step, the lifted primitives as
// traverse() folds them in, make_record for the winner).
//
// k_query<kAny, kVol, kQuant>: 256-thread blocks in a persistent grid; each
// block walks chunks of 256 consecutive rays, lane l of the block taking ray
// chunk * 256 + l: two 16-B loads for the ray, two 16-B stores for the hit
// (one byte for an occlusion result), coalesced and non-temporal like the
// path streams, so L2 and the Infinity Cache keep the BVH.  Per-lane state is
// k_extend's: the kLdsStack-entry LDS ring with the world ray (and its 1/d)
// and the hit words beside it, and a spill column per lane in global memory.
// Left out on purpose (DESIGN.md "Ray queries"): the claim pools, the
// prefetched next ray, the LDS node cache, a refill of idle lanes — a wave
// holds its 64 rays until the longest has ended.
// Arithmetic is fp32 in the Go operation order (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_layout.h"
#include "device_common.h"
#include "hit_ids.h"
#include "wave_variant.h"
#include "wavefront.h"
#include "query.h"

namespace rtg {
namespace qry {

#ifdef RTG_HOST_EMU
__device__ __forceinline__ float4 ldnt(const float4* p) { return *p; }
__device__ __forceinline__ void stnt(float4* p, float4 v) { *p = v; }
__device__ __forceinline__ void stnt(uint8_t* p, uint8_t v) { *p = v; }
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
__device__ __forceinline__ void stnt(uint8_t* p, uint8_t v) { __builtin_nontemporal_store(v, p); }
#endif

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// The guard at the ray load: a ray that fails it traces nothing.
__device__ __forceinline__ bool valid_ray(float4 o4, float4 d4) {
  const bool fin = finite_f(o4.x) && finite_f(o4.y) && finite_f(o4.z) && finite_f(d4.x) && finite_f(d4.y) && finite_f(d4.z);
  const bool dir = d4.x != 0.0f || d4.y != 0.0f || d4.z != 0.0f;
  const float tmin = o4.w, tmax = d4.w;
  return fin && dir && tmin == tmin && tmax == tmax && !(tmax < tmin);
}

}  // namespace qry

// Waves per SIMD requested, from the resource log of this file (DESIGN.md
// "Ray queries").  Plain variants: 6 waves (84-VGPR cap; 80 / 77 VGPRs used,
// nothing spilled).  At k_extend's 7 waves (72 VGPRs) they spill 3 VGPRs
// (16 B of scratch per lane) and measured 11-12 % slower (closest hit) and
// 6-10 % slower (any hit) on the headline scene's rays; 8 waves cannot be
// resident beside 22.5 KB of LDS per block.  The rare-primitive (kVol)
// variants use 121 / 127 VGPRs unspilled: 4 waves (128 VGPRs), as the kVol
// traversal kernels of wavefront.hip.
#ifndef RTG_QUERY_WAVES
#define RTG_QUERY_WAVES 6   // (a build-time override for A/B runs: make EXTRA=-DRTG_QUERY_WAVES=7, tools/query_rate.py)
#endif
constexpr int kQueryWaves = RTG_QUERY_WAVES, kQueryVolWaves = 4;
#define QUERY_WAVES(kVol) ((kVol) ? kQueryVolWaves : kQueryWaves)

template <bool kAny, bool kVol, bool kQuant>
static __global__ __launch_bounds__(256, QUERY_WAVES(kVol)) void k_query(DScene sc, QueryArgs a) {
  // stack ring + world ray + its 1/d (+ hit record: closest hit only)
  __shared__ uint32_t lds_stack[(kLdsStack + kWorldRayWords + kWorldInvWords + (kAny ? 0 : kHitWords)) * 256];
  const TStack S{lds_stack + threadIdx.x, 256, kLdsStack, a.spill + blockIdx.x * 256u, lds_stack, int(a.spill_lanes),
                 a.spill_cap, nullptr, true};
  const float4* const rays = a.rays;
  const uint32_t nchunks = (a.n + 255u) >> 8;
  Cnt cnt = {};
  Trav T{};   // fully initialised: no undef state flows through the divergent loop
  for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const uint32_t i = (c << 8) + threadIdx.x;
    if (i >= a.n) continue;   // the last chunk's tail
    const float4 o4 = qry::ldnt(&rays[2u * size_t(i)]), d4 = qry::ldnt(&rays[2u * size_t(i) + 1u]);
    const bool valid = qry::valid_ray(o4, d4);
    const V3 ro = mk(o4.x, o4.y, o4.z), rd = mk(d4.x, d4.y, d4.z);
    const float tmin = o4.w, tmax = d4.w;
    int s = TRAV_DONE;
    if (valid) {
      s = trav_init<kAny, false, false>(sc, T, S, ro, rd, a.time, tmin, tmax, 0u, 0u, DOM_VOL, cnt);
      while (s == TRAV_RUNNING) s = trav_step<kAny, false, kVol, kQuant>(sc, T, S, cnt, a.err);
    }
    if constexpr (kAny) {
      // the lifted world quads / spheres: the any-hit test of them (traverse())
      bool occ = s == TRAV_ANYHIT;
      if (valid && !occ) occ = lifted_prims_any<false>(sc, ro, rd, a.time, tmin, tmax, cnt);
      qry::stnt(static_cast<uint8_t*>(a.out) + i, uint8_t(occ ? 1 : 0));
    } else {
      float4 h0 = make_float4(-1.0f, __uint_as_float(0xFFFFFFFFu), __uint_as_float(0xFFFFFFFFu), __uint_as_float(0xFFFFFFFFu));
      float4 h1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(valid ? 0u : kQueryInvalid));
      if (valid) {
        Best b = trav_best(T, S);
        resolve_inst(sc, b);
        // the lifted world quads / spheres compete as in traverse()
        for (int k = 0; k < sc.num_prim_recs; ++k) {
          const KPrimRec R = kprimrec(sc.prim_recs, k);
          float t = 0.0f;
          if (!prim_rec_t<false, false>(R, ro, rd, a.time, tmin, __builtin_inff(), t, cnt) || !(t < tmax)) continue;
          const int kind = R->kind, refpos = R->refpos;
          if (b.kind == 0 || t < b.t || (t == b.t && tie_wins(sc, kind, refpos, 0, b.kind, b.refpos, b.primpos))) {
            b.t = t; b.kind = kind; b.idx = R->idx; b.inst = -1; b.refpos = refpos; b.primpos = 0;
          }
        }
        if (b.kind != 0) {
          int top = -1, prim = -1;
          hit_ids(sc, b.kind, b.idx, b.refpos, top, prim);
          const Rec rec = make_record<false>(sc, b, ro, rd, a.time);
          h0 = make_float4(b.t, __uint_as_float(uint32_t(top)), __uint_as_float(uint32_t(prim)), __uint_as_float(uint32_t(rec.mat)));
          h1 = make_float4(rec.N.x, rec.N.y, rec.N.z, __uint_as_float(rec.front ? kQueryFront : 0u));
        }
      }
      float4* const out = static_cast<float4*>(a.out);
      qry::stnt(&out[2u * size_t(i)], h0);
      qry::stnt(&out[2u * size_t(i) + 1u], h1);
    }
  }
}

#ifndef RTG_HOST_EMU
namespace qry {

using QueryFn = void (*)(DScene, QueryArgs);

// The variant pick_variant names for the scene.  The ray queries traverse the
// 4-wide arrays under RT_NODES_WIDE8 too (fp32 DNode4, as launch_primary).
template <bool kAny>
static QueryFn kernel_for(const WaveVariant& v) {
  if (v.vol) return v.quant ? k_query<kAny, true, true> : k_query<kAny, true, false>;
  return v.quant ? k_query<kAny, false, true> : k_query<kAny, false, false>;
}
static QueryFn kernel_for(const DScene& sc, bool any) {
  const WaveVariant v = pick_variant(sc);
  return any ? kernel_for<true>(v) : kernel_for<false>(v);
}

}  // namespace qry

int query_blocks(const DScene& sc, bool any, uint32_t n, int cus, int max_blocks) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)qry::kernel_for(sc, any), 256, 0) != hipSuccess || per_cu < 1)
    per_cu = 1;
  long long g = (long long)per_cu * (cus > 0 ? cus : 1);
  const long long need = (n + 255u) / 256u;
  if (g > need) g = need;
  if (max_blocks > 0 && g > max_blocks) g = max_blocks;
  return int(g < 1 ? 1 : g);
}

hipError_t launch_query(const DScene& sc, bool any, const QueryArgs& a, int blocks, hipStream_t st) {
  if (a.n == 0) return hipSuccess;
  if (a.n > kQueryMaxRays || blocks < 1 || size_t(blocks) * 256u > a.spill_lanes) return hipErrorInvalidValue;
  hipLaunchKernelGGL(qry::kernel_for(sc, any), dim3(blocks), dim3(256), 0, st, sc, a);
  return hipGetLastError();
}
#endif  // RTG_HOST_EMU

}  // namespace rtg
