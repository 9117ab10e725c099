// adaptive.hip — the device side of rt_render_adaptive: which pixels still
// need samples, as an ascending list of pixel ids, and the bookkeeping of each
// pixel's sample count.  The renders themselves are rt_render_moments's,
// untouched: a round is an ordinary render over the list this file writes.
//
// Selection, per pixel p with n = counts[p] samples and moments m1, m2 (all
// fp32, the operations as written, -ffp-contract=off; tests/adaptive_ref.py
// restates it in numpy):
//     nf = float(n), mu = m1 / nf, var = max(0, m2 / nf - mu * mu) / (nf - 1)
//     tol = rel_error * max(mu, lum_floor)
//     unconverged(p) = active(p) and var > tol * tol
//   active(p): 0 < counts[p] < max_spp, and counts[p] == cur when cur > 0.
//   neighbourhood 0: p is listed iff unconverged(p);
//   neighbourhood 1: p is listed iff active(p) and p or one of its 8
//     neighbours inside the image is unconverged.
//
// k_ad_flag    : active / unconverged of every pixel -> flags (one byte each)
// k_ad_count   : block b owns the ids [b * per, (b + 1) * per), per a multiple
//                of the block size; per step of blockDim ids, every wave votes
//                (__ballot) and adds the popcount; the waves' sums meet in LDS
//                and the block writes one count
// k_ad_scan    : one block: exclusive scan of the block counts in place, a
//                running carry over steps of its size; the carry left over is
//                the list's length -> total
// k_ad_scatter : k_ad_count's walk again: list[block offset + ids listed in
//                the block's earlier steps + earlier waves' votes of this step
//                + votes of the lanes below mine] = id
// No atomics, so the list is ascending and the same from run to run, whatever
// the grid.  Every kernel derives its ranges from blockDim / gridDim and is
// correct for any block size up to kAdBlock, one lane per block included (the
// host emulation, tests/adaptive_emu.cpp).  LDS: kAdMaxWaves words in the count
// and scatter kernels, kAdBlock words in the scan.  No scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "adaptive.h"

namespace rtg {

constexpr uint32_t kAdWave = 64;   // gfx950 runs wave64 only

__device__ __forceinline__ bool ad_unconverged(const AdArgs& a, uint32_t n, float m1, float m2) {
  const float nf = float(n);
  const float mu = m1 / nf;
  const float r = m2 / nf - mu * mu;
  const float var = (r > 0.0f ? r : 0.0f) / (nf - 1.0f);
  const float tol = a.rel_error * (mu > a.lum_floor ? mu : a.lum_floor);
  return var > tol * tol;
}

__global__ __launch_bounds__(kAdBlock) void k_ad_flag(AdArgs a) {
  const size_t n = size_t(a.w) * size_t(a.h);
  const size_t gs = size_t(gridDim.x) * blockDim.x;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += gs) {
    const uint32_t c = a.counts[i];
    const bool active = c != 0u && c < a.max_spp && (a.cur == 0u || c == a.cur);
    uint8_t f = 0;
    if (active) f = ad_unconverged(a, c, a.moments[2 * i], a.moments[2 * i + 1]) ? 3 : 1;
    a.flags[i] = f;
  }
}

// Whether pixel i is listed.
__device__ __forceinline__ bool ad_keep(const AdArgs& a, size_t i) {
  const uint8_t f = a.flags[i];
  if (!(f & 1)) return false;
  if (f & 2) return true;
  if (!a.neighbourhood) return false;
  const int x = int(i % size_t(a.w)), y = int(i / size_t(a.w));
  for (int dy = -1; dy <= 1; ++dy) {
    const int qy = y + dy;
    if (qy < 0 || qy >= a.h) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx;
      if (qx < 0 || qx >= a.w) continue;
      if (a.flags[size_t(qy) * size_t(a.w) + size_t(qx)] & 2) return true;   // unconverged implies active
    }
  }
  return false;
}

// The ids block b walks: [lo, hi) in `steps` steps of blockDim ids.  Every
// block takes the same number of steps, so the barriers inside the walk are
// reached by all its lanes.
struct AdRange {
  size_t lo, hi, steps;
};

__device__ __forceinline__ AdRange ad_range(size_t n) {
  const size_t bd = blockDim.x;
  const size_t chunks = (n + bd - 1) / bd;
  AdRange r;
  r.steps = (chunks + gridDim.x - 1) / gridDim.x;
  const size_t lo = size_t(blockIdx.x) * r.steps * bd;
  r.lo = lo < n ? lo : n;
  r.hi = r.lo + r.steps * bd < n ? r.lo + r.steps * bd : n;
  return r;
}

__global__ __launch_bounds__(kAdBlock) void k_ad_count(AdArgs a) {
  __shared__ uint32_t wave_n[kAdMaxWaves];
  const AdRange r = ad_range(size_t(a.w) * size_t(a.h));
  const uint32_t lane = uint32_t(__lane_id()), wave = threadIdx.x / kAdWave;
  uint32_t mine = 0;   // this wave's votes so far (the same in all its lanes)
  for (size_t s = 0; s < r.steps; ++s) {
    const size_t i = r.lo + s * blockDim.x + threadIdx.x;
    const bool keep = i < r.hi && ad_keep(a, i);
    mine += uint32_t(__popcll(__ballot(keep)));
  }
  if (lane == 0) wave_n[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t nw = (blockDim.x + kAdWave - 1) / kAdWave;
    uint32_t sum = 0;
    for (uint32_t w = 0; w < nw; ++w) sum += wave_n[w];
    a.block_counts[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(kAdBlock) void k_ad_scan(uint32_t* block_counts, uint32_t nb, uint32_t* total) {
  __shared__ uint32_t s[kAdBlock];
  const uint32_t tid = threadIdx.x, bd = blockDim.x;
  uint32_t carry = 0;   // the counts before this step (the same in every lane)
  for (uint32_t base = 0; base < nb; base += bd) {
    const uint32_t idx = base + tid;
    const uint32_t v = idx < nb ? block_counts[idx] : 0u;
    s[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < bd; off <<= 1) {
      const uint32_t t = tid >= off ? s[tid - off] : 0u;
      __syncthreads();
      s[tid] += t;
      __syncthreads();
    }
    if (idx < nb) block_counts[idx] = carry + (s[tid] - v);
    carry += s[bd - 1];
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

__global__ __launch_bounds__(kAdBlock) void k_ad_scatter(AdArgs a) {
  __shared__ uint32_t wave_n[kAdMaxWaves];
  const AdRange r = ad_range(size_t(a.w) * size_t(a.h));
  const uint32_t lane = uint32_t(__lane_id()), wave = threadIdx.x / kAdWave;
  const uint32_t nw = (blockDim.x + kAdWave - 1) / kAdWave;
  uint32_t base = a.block_counts[blockIdx.x];   // k_ad_scan left the block's offset here
  for (size_t s = 0; s < r.steps; ++s) {
    const size_t i = r.lo + s * blockDim.x + threadIdx.x;
    const bool keep = i < r.hi && ad_keep(a, i);
    const unsigned long long votes = __ballot(keep);
    if (lane == 0) wave_n[wave] = uint32_t(__popcll(votes));
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < nw; ++w) {
      if (w < wave) before += wave_n[w];
      all += wave_n[w];
    }
    if (keep) a.list[base + before + uint32_t(__popcll(votes & ((1ull << lane) - 1ull)))] = uint32_t(i);
    base += all;
    __syncthreads();   // the next step's counts replace these
  }
}

__global__ __launch_bounds__(kAdBlock) void k_ad_set_counts(const uint32_t* list, uint32_t n, uint32_t* counts,
                                                            uint32_t value) {
  const uint32_t gs = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) counts[list[i]] = value;
}

__global__ __launch_bounds__(kAdBlock) void k_ad_scatter_counts(const uint32_t* list, uint32_t n,
                                                                const uint32_t* counts, uint32_t* out) {
  const uint32_t gs = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) out[list[i]] = counts[list[i]];
}

// rt_normalize_samples.  `out` may be `sums`: every element is read by the
// lane that writes it, before it writes.
__global__ __launch_bounds__(kAdBlock) void k_normalize(const float* sums, int32_t channels, const uint32_t* counts,
                                                        size_t n, float target, float* out) {
  const size_t gs = size_t(gridDim.x) * blockDim.x;
  for (size_t p = size_t(blockIdx.x) * blockDim.x + threadIdx.x; p < n; p += gs) {
    const uint32_t c = counts[p];
    const size_t o = p * size_t(channels);
    if (c == 0u) {   // not a pixel of the frame: its bits as they are
      const uint32_t* src = reinterpret_cast<const uint32_t*>(sums);
      uint32_t* dst = reinterpret_cast<uint32_t*>(out);
      for (int32_t k = 0; k < channels; ++k) dst[o + k] = src[o + k];
      continue;
    }
    const float nf = float(c);
    for (int32_t k = 0; k < channels; ++k) out[o + k] = (sums[o + k] / nf) * target;
  }
}

// The selection kernels of one round in order, shared by the product launcher
// and the host emulation.  flag, count and scatter run over the pixels (count
// and scatter on the same grid: one block_counts word per block); scan is one
// block over that grid's counts.
template <class Flag, class Count, class Scan, class Scatter>
inline void ad_for_each_kernel(Flag&& flag, Count&& count, Scan&& scan, Scatter&& scatter) {
  flag();
  count();
  scan();
  scatter();
}

#ifndef RTG_HOST_EMU
uint32_t ad_grid(size_t n, int num_cus) {
  const size_t need = (n + kAdBlock - 1) / kAdBlock, cap = size_t(num_cus > 0 ? num_cus : 256) * 8;
  return uint32_t(need < 1 ? 1 : need < cap ? need : cap);
}

hipError_t launch_adaptive_select(const AdArgs& a, int num_cus, hipStream_t st) {
  const dim3 grid(ad_grid(size_t(a.w) * size_t(a.h), num_cus)), block(kAdBlock);
  ad_for_each_kernel([&] { hipLaunchKernelGGL(k_ad_flag, grid, block, 0, st, a); },
                     [&] { hipLaunchKernelGGL(k_ad_count, grid, block, 0, st, a); },
                     [&] { hipLaunchKernelGGL(k_ad_scan, dim3(1), block, 0, st, a.block_counts, grid.x, a.total); },
                     [&] { hipLaunchKernelGGL(k_ad_scatter, grid, block, 0, st, a); });
  return hipGetLastError();
}

hipError_t launch_ad_set_counts(const uint32_t* list, uint32_t n, uint32_t* counts, uint32_t value, int num_cus,
                                hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ad_set_counts, dim3(ad_grid(n, num_cus)), dim3(kAdBlock), 0, st, list, n, counts, value);
  return hipGetLastError();
}

hipError_t launch_ad_scatter_counts(const uint32_t* list, uint32_t n, const uint32_t* counts, uint32_t* out,
                                    int num_cus, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ad_scatter_counts, dim3(ad_grid(n, num_cus)), dim3(kAdBlock), 0, st, list, n, counts, out);
  return hipGetLastError();
}

hipError_t launch_normalize(const float* sums, int32_t channels, const uint32_t* counts, size_t n, int32_t target_spp,
                            float* out, int num_cus, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_normalize, dim3(ad_grid(n, num_cus)), dim3(kAdBlock), 0, st, sums, channels, counts, n,
                     float(target_spp), out);
  return hipGetLastError();
}
#endif

}  // namespace rtg
