// wave_layout.h — the batch layout of a wavefront render, as arithmetic.
//
// Everything render_wave (api.cpp) decides before it touches the device: the
// schedule knobs, how many twins a render gets, how tiles and pixels are
// dealt to them, how many path slots a batch holds, and where each twin's
// arrays lie inside the batch buffers (element offsets, not pointers).  Host
// only, no HIP calls: tests/wave_layout_probe.cpp runs it under ASan / UBSan,
// and tests/wave_emu.cpp sizes its buffers by it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "wavefront.h"

namespace rtg {

// ---- schedule knobs

// The context's schedule options (rt_ctx_set_option; 0 = automatic).
struct WaveOptions {
  size_t slots = 0;   // RT_OPT_BATCH_SLOTS
  int refill = 0;     // RT_OPT_REFILL
  int blocks = 0;     // RT_OPT_MAX_BLOCKS
  int tail = 0;       // RT_OPT_TAIL: 0 automatic, 1 off, > 1 the rays-left threshold
  int streams = 0;    // RT_OPT_STREAMS: 1..kMaxTwins
  int overlap = 0;    // RT_OPT_OVERLAP: 0 automatic, 1 off, 2 on
  int early_miss = 0; // RT_OPT_EARLY_MISS: 0 automatic, 1 off, 2 on
};

// The resolved knobs of one render: option, then environment, then automatic.
struct WaveKnobs {
  int streams = 0;        // twins asked for (0 = automatic: choose_twins)
  int overlap = 0;        // bounce overlap: 2 on, anything else off
  size_t slots = 0;       // path slots per batch (0 = automatic: auto_target)
  int refill = 16;        // lanes that must want an item before a wave claims a new run, 1..64
  int max_blocks = 0;     // > 0: cap on the persistent traversal grids
  int debug_sync = 0;     // synchronise after every launch
  uint32_t tail_rays = 0; // k_tail takes over at most this many paths left (0 = never)
  int tail_first = kTailFirstDefault;
  int early_miss = 0;     // rays that miss the world box resolved in k_shade: 1 off, anything else on where eligible
};

// The environment's tuning knobs, each the default of the option beside it:
//
//   RTGPU_STREAMS     RT_OPT_STREAMS     > 0: twins, at most kMaxTwins
//   RTGPU_OVERLAP     RT_OPT_OVERLAP     1 off, 2 on
//   RTGPU_SLOTS       RT_OPT_BATCH_SLOTS > 0: path slots per batch
//   RTGPU_REFILL      RT_OPT_REFILL      clamped to 1..64 (the wave size: beyond
//                                        it no wave would ever claim); unset 16
//   RTGPU_MAX_BLOCKS  RT_OPT_MAX_BLOCKS  > 0: cap on the persistent grids
//   RTGPU_TAIL_RAYS   RT_OPT_TAIL (auto) >= 0: the automatic rays-left threshold
//                                        of k_tail (0 = never); unset kTailRaysDefault
//   RTGPU_TAIL_FIRST  -                  bounce of k_tail's extra rays-left check;
//                                        unset kTailFirstDefault
//   RTGPU_DEBUG_SYNC  -                  > 0: synchronise after every launch
//   RTGPU_EARLY_MISS  RT_OPT_EARLY_MISS  1 off, 2 on
struct WaveEnv {
  int streams, overlap, refill, max_blocks, tail_rays, tail_first, debug_sync;
  size_t slots;
  int early_miss;
};

inline WaveEnv read_wave_env() {
  auto num = [](const char* name, long unset) {
    const char* e = getenv(name);
    return e ? atol(e) : unset;
  };
  WaveEnv v{};
  v.streams = int(std::min<long>(kMaxTwins, std::max<long>(0, num("RTGPU_STREAMS", 0))));
  v.overlap = int(num("RTGPU_OVERLAP", 0));
  v.slots = size_t(std::max<long>(0, num("RTGPU_SLOTS", 0)));
  v.refill = int(std::min<long>(64, std::max<long>(1, num("RTGPU_REFILL", 16))));
  v.max_blocks = int(std::max<long>(0, num("RTGPU_MAX_BLOCKS", 0)));
  const long tail = num("RTGPU_TAIL_RAYS", -1);
  v.tail_rays = tail >= 0 ? int(tail) : kTailRaysDefault;
  v.tail_first = int(num("RTGPU_TAIL_FIRST", kTailFirstDefault));
  v.debug_sync = num("RTGPU_DEBUG_SYNC", 0) > 0 ? 1 : 0;
  v.early_miss = int(num("RTGPU_EARLY_MISS", 0));
  return v;
}

// Read once per process, at the first render.
inline const WaveEnv& wave_env() {
  static const WaveEnv env = read_wave_env();
  return env;
}

// `probing`: a path probe reads bounce k's records back from the wavefront
// kernels' arrays, so no long-tail kernel (it carries paths in registers).
inline WaveKnobs resolve_knobs(const WaveOptions& opt, bool probing, const WaveEnv& env = wave_env()) {
  WaveKnobs k;
  k.streams = opt.streams ? opt.streams : env.streams;
  k.overlap = opt.overlap ? opt.overlap : env.overlap;
  k.slots = opt.slots ? opt.slots : env.slots;
  k.refill = opt.refill ? opt.refill : env.refill;
  k.max_blocks = opt.blocks ? opt.blocks : env.max_blocks;
  k.debug_sync = env.debug_sync;
  k.tail_rays = probing || opt.tail == 1 ? 0u : uint32_t(opt.tail > 1 ? opt.tail : env.tail_rays);
  k.tail_first = env.tail_first;
  k.early_miss = opt.early_miss ? opt.early_miss : env.early_miss;
  return k;
}

// ---- twins

// Twins per render unless RT_OPT_STREAMS / RTGPU_STREAMS say otherwise: three
// for renders of more than kThreeTwinSamples samples (pixels x spp), two
// below.  CornellBoxLucy full frame (405 M samples): one stream 1770, two
// 1937-1952, three 1967-1970 Msamples/s; its 1/8 shards (51 M) are faster on
// two (8-way shard prediction 6.94 / 6.99 vs 6.84 / 6.84 on three), its 1/2
// shards (202 M) on three (2-way 1.908 / 1.917 vs 1.941 / 1.951), its 1/4
// shards (101 M) alike (3.73 / 3.74 vs 3.75 / 3.75; round 4).
constexpr int kDefaultTwins = 2;
constexpr uint64_t kThreeTwinSamples = uint64_t(1) << 26;
// With the bounce overlap each twin runs two streams: at most two twins, so
// that the four streams keep a hardware queue each (GPU_MAX_HW_QUEUES = 4).
constexpr int kOverlapTwins = 2;

inline uint64_t tile_pixels(const std::vector<int4>& tiles) {
  uint64_t n = 0;
  for (const int4& tl : tiles) n += uint64_t(tl.z) * uint64_t(tl.w);
  return n;
}

// Bounce overlap (run_batches) for scenes with lights: a second stream per
// twin.  Off by default: measured slower on C4 at every twin count (DESIGN §3
// "Bounce overlap": the full frame 2150 -> 2046 / 2025 Msamples/s on one / two
// twins, 8-way shard sums 218.8 -> 223.7 / 230.7 ms).
inline bool use_overlap(const WaveKnobs& k, bool lit) { return lit && k.overlap == 2; }

// Rays that miss the world box resolved in k_shade (WaveArgs::early_miss;
// DESIGN §3 "Rays that miss the world box"): the bits of the word.  On
// unless turned off, in the renders where it is exact and pays: the scene is
// eligible (`eligible`, early_miss_eligible: the root-box test alone decides
// such a ray, and world primitives are lifted), and no path probe reads a
// bounce's arrays (`probing`).
// The survivors' part (EARLY_NEXT) stays off in a render that may hand its
// paths to k_tail, which reads one range of the stream (run_batches: no
// lights, a tail threshold, depth above 8).
inline uint32_t early_miss_bits(const WaveKnobs& k, bool eligible, bool probing, bool lit, int max_depth) {
  if (k.early_miss == 1 || !eligible || probing) return 0u;
  const bool may_tail = !lit && k.tail_rays > 0 && max_depth > 8;
  return EARLY_NEE | (may_tail ? 0u : EARLY_NEXT);
}

// Twins (wavefront.hip run_batches): tiles dealt in turn to `nt` parts of the
// pixel list, each rendered on its own stream so one part's kernel tails
// overlap another's next kernel.  Automatic = twins: CornellBoxLucy full
// frame 1770 (one stream) -> 1880 Msamples/s, and the 1/8 shards gain more.
// Scenes whose shading runs the lifted volumes' tests (`shade_vol`, SHADE_VOL:
// C3's fog) render fastest on one stream: CornellBoxScene 600x600x1000 one /
// two / three parts 1605 / 1563 / 1557 Msamples/s (round 4).
inline int choose_twins(const WaveKnobs& k, bool shade_vol, bool overlap, uint64_t tile_px, int spp, size_t ntiles) {
  int automatic = shade_vol ? 1 : tile_px * uint64_t(std::max(1, spp)) > kThreeTwinSamples ? 3 : kDefaultTwins;
  if (overlap) automatic = std::min(automatic, kOverlapTwins);
  const int want = k.streams ? k.streams : automatic;
  return int(std::max<size_t>(1, std::min<size_t>(size_t(std::max(1, want)), ntiles)));
}

// Tile k goes to twin k % nt; the pixel list (y * width + x) holds twin 0's
// pixels, then twin 1's, ..., row-major inside each tile (x, y, w, h).
inline void deal_pixels(const std::vector<int4>& tiles, int width, int nt, std::vector<uint32_t>& out,
                        uint32_t twin_npix[kMaxTwins]) {
  out.clear();
  for (int t = 0; t < kMaxTwins; ++t) twin_npix[t] = 0;
  for (int t = 0; t < nt; ++t) {
    const size_t before = out.size();
    for (size_t k = size_t(t); k < tiles.size(); k += size_t(nt)) {
      const int4& tl = tiles[k];
      for (int y = tl.y; y < tl.y + tl.w; ++y)
        for (int x = tl.x; x < tl.x + tl.z; ++x) out.push_back(uint32_t(y) * uint32_t(width) + uint32_t(x));
    }
    twin_npix[t] = uint32_t(out.size() - before);
  }
}

// A pixel list that is already on the device (rt_render_adaptive's rounds)
// is cut where it lies: twin t renders [n * t / nt, n * (t + 1) / nt).
// choose_twins is fed the list's length for `ntiles`, so nt <= n and no part
// is empty; an empty list has no parts (nothing is launched for it).
inline void split_list(uint32_t n, int nt, uint32_t twin_npix[kMaxTwins]) {
  for (int t = 0; t < kMaxTwins; ++t) twin_npix[t] = 0;
  if (n == 0 || nt < 1) return;
  nt = std::min(nt, kMaxTwins);
  for (int t = 0; t < nt; ++t)
    twin_npix[t] = uint32_t(uint64_t(n) * uint64_t(t + 1) / uint64_t(nt) - uint64_t(n) * uint64_t(t) / uint64_t(nt));
}

// ---- path slots per batch

// Per slot: kSlotF4 float4 arrays (wavefront.h) + job info + visibility
// words; kSlotF4Dark arrays and no job words in a scene without lights
// (C5: 128 instead of 232 B, three batches of 1.38G slots instead of four).
inline size_t slot_f4(bool lit) { return size_t(lit ? kSlotF4 : kSlotF4Dark); }
inline size_t slot_job_words(bool lit) { return lit ? 2 : 0; }
inline size_t slot_bytes(bool lit) { return slot_f4(lit) * sizeof(float4) + slot_job_words(lit) * sizeof(uint32_t); }

constexpr size_t kMinSlots = size_t(1) << 20;
// at most 1.5 * 2^30 slots: a twin's slot indices stay below 2^31
constexpr size_t kMaxSlots = size_t(3) << 29;

// Automatic path slots per batch: as many as fit in 85 % of the free HBM
// (`reusable_bytes`: the current batch buffers, which the next replace), up
// to kMaxSlots.  Larger batches amortise every launch's ramp-down tail;
// measured on CornellBoxLucy (Msamples/s): 8M slots 501, 32M 686, 128M 759,
// 210M 799, the whole 405M-sample frame in one batch 833; on HDRITestScene
// 1920x1080 x 2000 spp, 8 batches of 518M slots 9571, 5 of 829M 9703, 4 of
// 1037M 9820 (profiles/r06_c5_slots_ab.log).
inline size_t auto_target(size_t free_bytes, size_t reusable_bytes, bool lit) {
  return std::min(kMaxSlots, std::max(kMinSlots, (free_bytes + reusable_bytes) / 100 * 85 / slot_bytes(lit)));
}

// When the automatic size does not fit after all (another process, or another
// context, took memory since it was chosen), render_wave halves and retries,
// down to kMinSlots or one sample per batch.
inline size_t halve(size_t target) { return std::max(kMinSlots, target / 2); }
inline bool can_halve(size_t target, uint32_t spb) { return target > kMinSlots && spb > 1; }

struct BatchSize {
  uint32_t spb;      // samples per batch: the samples are split evenly over the batches
  size_t nslots;     // spb * npix, over all twins
  size_t f4_bytes;   // `wstate`: every twin's slot_f4 float4 arrays of its slots
  size_t wq_bytes;   // `wq`: every twin's CNT_WORDS_Q queue counters plus its job words
};

// `wq` has room for kMaxTwins twins' counters whatever `nt` a render uses, so
// the buffers of one render serve the next with another twin count.
inline BatchSize size_batch(uint32_t spp, uint32_t npix, size_t target, bool lit) {
  const uint32_t max_spb = uint32_t(std::max<size_t>(1, std::min<size_t>(spp, target / npix)));
  const uint32_t nbatch = (spp + max_spb - 1) / max_spb;
  BatchSize b{};
  b.spb = (spp + nbatch - 1) / nbatch;
  b.nslots = size_t(b.spb) * npix;
  b.f4_bytes = b.nslots * slot_f4(lit) * sizeof(float4);
  b.wq_bytes = (b.nslots * slot_job_words(lit) + size_t(kMaxTwins) * CNT_WORDS_Q) * sizeof(uint32_t);
  return b;
}

// ---- traversal-stack spill

// Spill entries per lane: what the scene's stack bound leaves beyond the
// `ring` entries held in LDS (flatten: stack_needed <= kStackMax; a deeper
// push is flagged).
inline int spill_cap_for(int stack_needed, int ring) { return std::max(1, std::min(kStackMax, stack_needed) - ring); }

struct SpillLayout {
  uint32_t lanes;      // lanes that can be resident at once
  int cap;             // entries per lane
  size_t area_words;   // one area: lanes * cap
  int areas;           // one per twin, two with the bounce overlap (k_shadow beside k_extend)
  size_t words() const { return size_t(areas) * area_words; }
};

inline SpillLayout spill_layout(int nt, bool overlap, int num_cus, int cap) {
  SpillLayout s{};
  s.lanes = uint32_t(std::max(1, num_cus)) * kSpillLanesPerCU;
  s.cap = cap;
  s.area_words = size_t(s.lanes) * size_t(cap);
  s.areas = nt * (overlap ? 2 : 1);
  return s;
}

// ---- each twin's slices

struct TwinSlice {
  size_t S;              // path slots: spb * npix
  size_t f4_off;         // float4s into `wstate`: slot_f4 arrays of S
  size_t q_off;          // words into `wq`: CNT_WORDS_Q counters, then the job words (2 arrays of S)
  size_t pix_off;        // pixels into `wpix`; x 3 into `wacc`, x kFeatFloats into `wfacc`
  uint32_t npix;
  size_t spill_off;      // words into `wspill`: k_extend's / k_tail's area
  size_t spill_sh_off;   // k_shadow's: its own area with the bounce overlap
};

// What the slices are cut from, in the offsets' units: float4s of `wstate`,
// words of `wq`, pixels that `wpix` / `wacc` (/ `wfacc`) hold, words of `wspill`.
struct WaveCaps {
  size_t f4, q, pix, spill;
};

struct WaveLayout {
  int nt = 0;
  bool lit = false;
  TwinSlice tw[kMaxTwins] = {};
  size_t spill_area = 0;   // words of one spill area
  WaveCaps cap = {};
};

inline WaveLayout slice_twins(uint32_t spb, const uint32_t twin_npix[kMaxTwins], int nt, bool lit, bool overlap,
                              const SpillLayout& spill, const WaveCaps& cap) {
  WaveLayout L;
  L.nt = nt;
  L.lit = lit;
  L.spill_area = spill.area_words;
  L.cap = cap;
  size_t f4 = 0, q = 0, pix = 0;
  for (int t = 0; t < nt; ++t) {
    TwinSlice& s = L.tw[t];
    s.S = size_t(spb) * twin_npix[t];
    s.f4_off = f4;
    s.q_off = q;
    s.pix_off = pix;
    s.npix = twin_npix[t];
    s.spill_off = size_t(t) * spill.area_words;
    s.spill_sh_off = overlap ? size_t(nt + t) * spill.area_words : s.spill_off;
    f4 += slot_f4(lit) * s.S;
    q += CNT_WORDS_Q + slot_job_words(lit) * s.S;
    pix += s.npix;
  }
  return L;
}

// False when a slice leaves its buffer, or a twin's slot count does not fit
// WaveArgs::slots or reaches 2^31 (the kernels' slot indices are 32-bit).
inline bool check(const WaveLayout& L) {
  if (L.nt < 1 || L.nt > kMaxTwins) return false;
  for (int t = 0; t < L.nt; ++t) {
    const TwinSlice& s = L.tw[t];
    if (s.S > size_t(UINT32_MAX) || s.S >= (size_t(1) << 31)) return false;
    if (s.f4_off + slot_f4(L.lit) * s.S > L.cap.f4) return false;
    if (s.q_off + CNT_WORDS_Q + slot_job_words(L.lit) * s.S > L.cap.q) return false;
    if (s.pix_off + s.npix > L.cap.pix) return false;
    if (s.spill_off + L.spill_area > L.cap.spill || s.spill_sh_off + L.spill_area > L.cap.spill) return false;
  }
  return true;
}

// Points `a` at twin `s`'s arrays inside the batch buffers.  Without lights
// no kernel touches the NEE job arrays: their pointers stay null.
inline void bind_twin(WaveArgs& a, float4* wstate, uint32_t* wq, const uint32_t* wpix, double* wacc, uint32_t* wspill,
                      const TwinSlice& s, bool lit) {
  float4* const f = wstate + s.f4_off;
  uint32_t* const q = wq + s.q_off;
  const size_t S = s.S;
  for (int k = 0; k < 2; ++k) {
    float4* sb = f + size_t(3 * k) * S;
    a.s[k] = PathStream{sb, sb + S, sb + 2 * S};
  }
  a.hit = f + 6 * S; a.Lout = f + 7 * S;
  a.counts = q;
  if (lit) {
    a.sj_p = f + 8 * S; a.sj_a = f + 9 * S; a.sj_h = f + 10 * S;
    a.ne_a = f + 11 * S; a.ne_h = f + 12 * S; a.ne_beta = f + 13 * S;
    a.sj_info = q + CNT_WORDS_Q;
    a.sj_vis = a.sj_info + S;
  }
  a.pixels = wpix + s.pix_off;
  a.npix = s.npix;
  a.acc = wacc + s.pix_off * 3;
  a.spill = wspill + s.spill_off;
  a.spill_sh = wspill + s.spill_sh_off;
  a.slots = uint32_t(S);
}

// ---- timing events (rt_set_kernel_timing)

// Worst case: 2 events per timed launch, 3 timed launches per bounce, per
// batch and twin.
inline size_t timing_events_wanted(uint32_t spp, uint32_t spb, int max_depth, int nt, size_t limit) {
  const size_t batches = (spp + spb - 1) / spb;
  return std::min(limit, batches * size_t(std::max(1, max_depth)) * 6 * size_t(nt) + 4);
}

}  // namespace rtg
