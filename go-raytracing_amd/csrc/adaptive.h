// adaptive.h — launch interface of adaptive.hip (rt_render_adaptive): the
// selection of the pixels that still need samples, as an ascending list on
// the device, and the count bookkeeping around the rounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtg {

// What the selection kernels of one round share.
struct AdArgs {
  const float* moments;     // W*H*2 luminance moments (m1, m2) of each pixel's samples so far
  const uint32_t* counts;   // W*H samples so far: 0 = not in the call, >= max_spp = done
  uint8_t* flags;           // W*H: bit 0 = active, bit 1 = unconverged (k_ad_flag writes it)
  uint32_t* block_counts;   // one word per block of k_ad_count / k_ad_scatter's grid: the block's
                            // count, then (k_ad_scan, in place) the list offset of its first pixel
  uint32_t* total;          // one word: the list's length
  uint32_t* list;           // W*H: the active pixels' ids, ascending
  int32_t w, h;
  uint32_t max_spp;
  uint32_t cur;             // > 0: only pixels with counts == cur are active (a render's round:
                            // a pixel that left the active set has fewer); 0: every pixel with
                            // 0 < counts < max_spp, each with its own count (rt_adaptive_select)
  int32_t neighbourhood;    // 1: the 3x3 dilation
  float rel_error, lum_floor;
};

// Most waves per block the selection kernels' LDS has room for (256 lanes).
constexpr int kAdMaxWaves = 4;
constexpr int kAdBlock = 256;
constexpr int kAdMaxChannels = 8;

#ifndef RTG_HOST_EMU
// Blocks of k_ad_count / k_ad_scatter for `n` pixels: a.block_counts holds that many words.
uint32_t ad_grid(size_t n, int num_cus);
// One round's selection on `st`: flags, block counts, their scan, the list.
// a.total holds the length afterwards; the list is a pure function of the inputs.
hipError_t launch_adaptive_select(const AdArgs& a, int num_cus, hipStream_t st);
// counts[list[i]] = value for i < n (after round 0, and after every later round).
hipError_t launch_ad_set_counts(const uint32_t* list, uint32_t n, uint32_t* counts, uint32_t value, int num_cus,
                                hipStream_t st);
// out[list[i]] = counts[list[i]] for i < n: the call's pixels' counts into the caller's image.
hipError_t launch_ad_scatter_counts(const uint32_t* list, uint32_t n, const uint32_t* counts, uint32_t* out,
                                    int num_cus, hipStream_t st);
// out[p][c] = (sums[p][c] / float(counts[p])) * float(target_spp); counts[p] == 0 copies the bits.
hipError_t launch_normalize(const float* sums, int32_t channels, const uint32_t* counts, size_t n, int32_t target_spp,
                            float* out, int num_cus, hipStream_t st);
#endif

}  // namespace rtg
