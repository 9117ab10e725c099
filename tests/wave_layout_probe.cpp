// wave_layout_probe.cpp — test-only sweep of go-raytracing_amd/csrc/wave_layout.h,
// the arithmetic that decides where every kernel of a wavefront render may
// write.  Built with g++ under AddressSanitizer + UBSan by
// tests/test_wave_layout.py; needs no device.
//
// usage: wave_layout_probe      prints {"cases": N, "fails": F}; exit 1 if F
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../go-raytracing_amd/csrc/wave_layout.h"

using namespace rtg;

namespace {

long g_cases = 0, g_fails = 0;

#define EXPECT(cond, ...)                                      \
  do {                                                         \
    if (!(cond)) {                                             \
      if (++g_fails <= 20) {                                   \
        fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
        fprintf(stderr, __VA_ARGS__);                          \
        fputc('\n', stderr);                                   \
      }                                                        \
    }                                                          \
  } while (0)

struct Image {
  int w, h;
  std::vector<int4> tiles;
};

// 16x16 tiles of a w x h image, row by row (ragged at the right and bottom).
Image tile_image(int w, int h) {
  Image im{w, h, {}};
  for (int y = 0; y < h; y += 16)
    for (int x = 0; x < w; x += 16) im.tiles.push_back(int4{x, y, std::min(16, w - x), std::min(16, h - y)});
  return im;
}

using Span = std::pair<size_t, size_t>;   // [first, second)

// Every span inside [0, cap) and no two overlapping.
bool disjoint_inside(std::vector<Span> v, size_t cap) {
  std::sort(v.begin(), v.end());
  size_t end = 0;
  for (const Span& s : v) {
    if (s.first < end || s.second < s.first || s.second > cap) return false;
    end = s.second;
  }
  return true;
}

void check_pixels(const Image& im, int nt, const std::vector<uint32_t>& list, const uint32_t twin_npix[kMaxTwins]) {
  std::map<uint32_t, size_t> owner;   // pixel -> its tile
  for (size_t k = 0; k < im.tiles.size(); ++k) {
    const int4& tl = im.tiles[k];
    for (int y = tl.y; y < tl.y + tl.w; ++y)
      for (int x = tl.x; x < tl.x + tl.z; ++x) owner[uint32_t(y) * uint32_t(im.w) + uint32_t(x)] = k;
  }
  EXPECT(list.size() == owner.size(), "%zu listed, %zu in the tiles", list.size(), owner.size());
  std::vector<uint32_t> sorted(list);
  std::sort(sorted.begin(), sorted.end());
  size_t i = 0;
  bool perm = sorted.size() == owner.size();
  for (auto it = owner.begin(); perm && it != owner.end(); ++it, ++i) perm = sorted[i] == it->first;
  EXPECT(perm, "the pixel list is no permutation of the tiles' pixels");
  size_t sum = 0, at = 0;
  for (int t = 0; t < kMaxTwins; ++t) {
    sum += twin_npix[t];
    EXPECT(t < nt || twin_npix[t] == 0, "twin %d beyond nt has pixels", t);
  }
  EXPECT(sum == list.size(), "twin_npix sums to %zu of %zu", sum, list.size());
  if (!perm || sum != list.size()) return;
  // twin t holds tiles t, t + nt, ... in that order, each row-major
  for (int t = 0; t < nt; ++t) {
    size_t last_tile = 0;
    uint32_t last_px = 0;
    for (size_t k = 0; k < twin_npix[t]; ++k, ++at) {
      const size_t tile = owner[list[at]];
      EXPECT(tile % size_t(nt) == size_t(t), "tile %zu in twin %d of %d", tile, t, nt);
      if (k) {
        EXPECT(tile >= last_tile, "twin %d: tile order", t);
        if (tile == last_tile) EXPECT(list[at] > last_px, "twin %d: not row-major inside tile %zu", t, tile);
      }
      last_tile = tile;
      last_px = list[at];
    }
  }
}

// Binds every twin to real buffers of exactly the sized bytes and touches
// both ends of every array (ASan sees an array that leaves its buffer).
void check_arrays(const WaveLayout& lay, const BatchSize& bs, const SpillLayout& spill, size_t npix, bool feat) {
  std::vector<float4> wstate(bs.f4_bytes / sizeof(float4));
  std::vector<uint32_t> wq(bs.wq_bytes / sizeof(uint32_t)), wpix(npix), wspill(spill.words());
  std::vector<double> wacc(npix * 3), wfacc(feat ? npix * kFeatFloats : 0);
  std::vector<Span> f4s, qs, accs, faccs;
  for (int t = 0; t < lay.nt; ++t) {
    const TwinSlice& s = lay.tw[t];
    WaveArgs a{};
    bind_twin(a, wstate.data(), wq.data(), wpix.data(), wacc.data(), wspill.data(), s, lay.lit);
    EXPECT(a.slots == s.S && a.npix == s.npix, "twin %d: slots / npix", t);
    std::vector<float4*> arrs = {a.s[0].o, a.s[0].d, a.s[0].beta, a.s[1].o, a.s[1].d, a.s[1].beta, a.hit, a.Lout};
    if (lay.lit) {
      for (float4* p : {a.sj_p, a.sj_a, a.sj_h, a.ne_a, a.ne_h, a.ne_beta}) arrs.push_back(p);
      EXPECT(a.sj_info && a.sj_vis, "twin %d: job words missing", t);
    } else {
      EXPECT(!a.sj_p && !a.sj_a && !a.sj_h && !a.ne_a && !a.ne_h && !a.ne_beta && !a.sj_info && !a.sj_vis,
             "twin %d: a dark scene's NEE job pointers are not null", t);
    }
    EXPECT(arrs.size() == slot_f4(lay.lit), "twin %d: %zu float4 arrays", t, arrs.size());
    for (float4* p : arrs) {
      const size_t off = size_t(p - wstate.data());
      f4s.push_back({off, off + s.S});
      EXPECT(off >= s.f4_off && off + s.S <= s.f4_off + slot_f4(lay.lit) * s.S, "twin %d: array outside its slice", t);
      if (s.S) p[0].x = p[s.S - 1].w = 1.0f;
    }
    const size_t q0 = size_t(a.counts - wq.data());
    qs.push_back({q0, q0 + CNT_WORDS_Q});
    a.counts[0] = a.counts[CNT_WORDS_Q - 1] = 1u;
    if (lay.lit) {
      for (uint32_t* p : {a.sj_info, a.sj_vis}) {
        const size_t off = size_t(p - wq.data());
        qs.push_back({off, off + s.S});
        if (s.S) p[0] = p[s.S - 1] = 1u;
      }
    }
    const size_t px = size_t(a.pixels - wpix.data());
    EXPECT(px == s.pix_off, "twin %d: pixel offset", t);
    const size_t ac = size_t(a.acc - wacc.data());
    accs.push_back({ac, ac + size_t(s.npix) * 3});
    if (feat) faccs.push_back({s.pix_off * kFeatFloats, (s.pix_off + s.npix) * kFeatFloats});
    if (s.npix) {
      wpix[px] = wpix[px + s.npix - 1] = 1u;
      a.acc[0] = a.acc[size_t(s.npix) * 3 - 1] = 1.0;
    }
    a.spill[0] = a.spill[spill.area_words - 1] = 1u;
    a.spill_sh[0] = a.spill_sh[spill.area_words - 1] = 1u;
  }
  EXPECT(disjoint_inside(f4s, wstate.size()), "float4 arrays overlap or leave wstate");
  EXPECT(disjoint_inside(qs, wq.size()), "queue counters / job words overlap or leave wq");
  EXPECT(disjoint_inside(accs, wacc.size()), "fp64 sums overlap or leave wacc");
  EXPECT(disjoint_inside(faccs, wfacc.size()), "feature sums overlap or leave wfacc");
}

void check_case(const Image& im, int streams, bool overlap, bool lit, bool feat, uint32_t spp, size_t target) {
  ++g_cases;
  WaveKnobs knobs;
  knobs.streams = streams;
  const int nt = choose_twins(knobs, false, overlap, tile_pixels(im.tiles), int(spp), im.tiles.size());
  EXPECT(nt >= 1 && size_t(nt) <= im.tiles.size() && nt == std::min<int>(streams, int(im.tiles.size())), "nt %d", nt);
  std::vector<uint32_t> list;
  uint32_t twin_npix[kMaxTwins];
  deal_pixels(im.tiles, im.w, nt, list, twin_npix);
  // the list depends on the image and nt alone: checked once for each
  static std::map<std::pair<const Image*, int>, bool> seen;
  if (!seen[{&im, nt}]) {
    seen[{&im, nt}] = true;
    check_pixels(im, nt, list, twin_npix);
  }
  const uint32_t npix = uint32_t(list.size());
  EXPECT(npix == tile_pixels(im.tiles), "npix");

  const BatchSize bs = size_batch(spp, npix, target, lit);
  EXPECT(bs.spb >= 1 && bs.spb <= spp, "spb %u", bs.spb);
  EXPECT(size_t((spp + bs.spb - 1) / bs.spb) * bs.spb >= spp, "the batches do not cover the samples");
  EXPECT(bs.nslots == size_t(bs.spb) * npix && bs.nslots <= std::max<size_t>(target, npix), "nslots %zu target %zu", bs.nslots, target);
  EXPECT(bs.wq_bytes >= size_t(kMaxTwins) * CNT_WORDS_Q * sizeof(uint32_t), "wq has no room for kMaxTwins counter blocks");
  EXPECT(bs.f4_bytes + bs.wq_bytes == bs.nslots * slot_bytes(lit) + size_t(kMaxTwins) * CNT_WORDS_Q * sizeof(uint32_t),
         "size_batch and slot_bytes disagree");

  const SpillLayout spill = spill_layout(nt, overlap, 2, spill_cap_for(12, kLdsStack));
  EXPECT(spill.areas == nt * (overlap ? 2 : 1) && spill.area_words == size_t(2) * kSpillLanesPerCU * 4, "spill layout");
  const WaveCaps cap{bs.f4_bytes / sizeof(float4), bs.wq_bytes / sizeof(uint32_t), npix, spill.words()};
  const WaveLayout lay = slice_twins(bs.spb, twin_npix, nt, lit, overlap, spill, cap);
  EXPECT(check(lay), "check refuses the layout it was sized for");

  std::vector<Span> f4s, qs, pxs, sps;
  size_t slots = 0;
  for (int t = 0; t < nt; ++t) {
    const TwinSlice& s = lay.tw[t];
    EXPECT(s.S == size_t(bs.spb) * twin_npix[t] && s.npix == twin_npix[t], "twin %d: S", t);
    slots += s.S;
    f4s.push_back({s.f4_off, s.f4_off + slot_f4(lit) * s.S});
    qs.push_back({s.q_off, s.q_off + CNT_WORDS_Q + slot_job_words(lit) * s.S});
    pxs.push_back({s.pix_off, s.pix_off + s.npix});
    sps.push_back({s.spill_off, s.spill_off + spill.area_words});
    if (overlap) sps.push_back({s.spill_sh_off, s.spill_sh_off + spill.area_words});
    else EXPECT(s.spill_sh_off == s.spill_off, "twin %d: k_shadow's area without overlap", t);
  }
  EXPECT(slots == bs.nslots, "the twins' slots sum to %zu of %zu", slots, bs.nslots);
  EXPECT(disjoint_inside(f4s, cap.f4), "float4 slices overlap or leave f4_bytes");
  EXPECT(disjoint_inside(qs, cap.q), "queue slices overlap or leave wq_bytes");
  EXPECT(disjoint_inside(pxs, cap.pix), "pixel slices overlap or leave the list");
  EXPECT(sps.size() == size_t(spill.areas) && disjoint_inside(sps, cap.spill), "spill areas overlap or leave wspill");

  // one element less in any buffer is refused
  WaveLayout less = lay;
  less.cap.f4 -= 1;
  EXPECT(!check(less), "check accepts a short wstate");
  less = lay;
  less.cap.q = qs.back().second - 1;
  EXPECT(!check(less), "check accepts a short wq");
  less = lay;
  less.cap.pix -= 1;
  EXPECT(!check(less), "check accepts a short pixel list");
  less = lay;
  less.cap.spill -= 1;
  EXPECT(!check(less), "check accepts a short wspill");

  if (bs.f4_bytes <= (size_t(1) << 20)) check_arrays(lay, bs, spill, npix, feat);
}

void check_knobs() {
  // option beats environment beats automatic; the environment is read once
  const WaveKnobs env = resolve_knobs(WaveOptions{}, false);
  EXPECT(env.streams == kMaxTwins && env.overlap == 2 && env.slots == 123456 && env.refill == 64 && env.max_blocks == 77 &&
             env.debug_sync == 1 && env.tail_rays == 555u && env.tail_first == 3,
         "environment knobs: %d %d %zu %d %d %d %u %d", env.streams, env.overlap, env.slots, env.refill, env.max_blocks,
         env.debug_sync, env.tail_rays, env.tail_first);
  WaveOptions opt;
  opt.slots = 999;
  opt.refill = 7;
  opt.blocks = 11;
  opt.tail = 4242;
  opt.streams = 3;
  opt.overlap = 1;
  const WaveKnobs o = resolve_knobs(opt, false);
  EXPECT(o.streams == 3 && o.overlap == 1 && o.slots == 999 && o.refill == 7 && o.max_blocks == 11 && o.tail_rays == 4242u,
         "options do not beat the environment");
  EXPECT(o.debug_sync == 1 && o.tail_first == 3, "knobs without an option");
  opt.tail = 1;
  EXPECT(resolve_knobs(opt, false).tail_rays == 0u, "RT_OPT_TAIL 1 = off");
  EXPECT(resolve_knobs(WaveOptions{}, true).tail_rays == 0u, "a probe runs no tail kernel");
  for (const char* n : {"RTGPU_STREAMS", "RTGPU_OVERLAP", "RTGPU_SLOTS", "RTGPU_REFILL", "RTGPU_MAX_BLOCKS", "RTGPU_TAIL_RAYS",
                        "RTGPU_TAIL_FIRST", "RTGPU_DEBUG_SYNC"})
    unsetenv(n);
  EXPECT(resolve_knobs(WaveOptions{}, false).slots == 123456, "the environment is read once");
  const WaveKnobs a = resolve_knobs(WaveOptions{}, false, read_wave_env());
  EXPECT(a.streams == 0 && a.overlap == 0 && a.slots == 0 && a.refill == 16 && a.max_blocks == 0 && a.debug_sync == 0 &&
             a.tail_rays == uint32_t(kTailRaysDefault) && a.tail_first == kTailFirstDefault,
         "automatic knobs");
  setenv("RTGPU_REFILL", "0", 1);
  setenv("RTGPU_TAIL_RAYS", "0", 1);
  setenv("RTGPU_STREAMS", "-3", 1);
  const WaveKnobs c = resolve_knobs(WaveOptions{}, false, read_wave_env());
  EXPECT(c.refill == 1 && c.tail_rays == 0u && c.streams == 0, "clamps: %d %u %d", c.refill, c.tail_rays, c.streams);

  // automatic twins
  EXPECT(choose_twins(a, false, false, 1000, 10, 64) == kDefaultTwins, "automatic twins");
  EXPECT(choose_twins(a, false, false, uint64_t(1) << 20, 65, 64) == 3, "three twins above kThreeTwinSamples");
  EXPECT(choose_twins(a, false, false, uint64_t(1) << 20, 64, 64) == kDefaultTwins, "two twins at kThreeTwinSamples");
  EXPECT(choose_twins(a, false, true, uint64_t(1) << 20, 65, 64) == kOverlapTwins, "overlap: at most two twins");
  EXPECT(choose_twins(a, true, false, uint64_t(1) << 20, 65, 64) == 1, "SHADE_VOL: one twin");
  EXPECT(choose_twins(a, false, false, uint64_t(1) << 20, 65, 2) == 2 && choose_twins(a, false, false, 256, 1, 1) == 1,
         "automatic twins beyond the tiles");
  EXPECT(use_overlap(env, true) && !use_overlap(env, false) && !use_overlap(o, true) && !use_overlap(a, true), "use_overlap");
}

void check_sizes() {
  for (int lit = 0; lit < 2; ++lit) {
    EXPECT(slot_bytes(lit != 0) == (lit ? 232u : 128u), "slot bytes");
    EXPECT(auto_target(0, 0, lit != 0) == kMinSlots, "auto_target: floor");
    EXPECT(auto_target(size_t(1) << 45, 0, lit != 0) == kMaxSlots, "auto_target: ceiling");
    const size_t free_b = size_t(100) << 30, reuse = size_t(20) << 30;
    EXPECT(auto_target(free_b, reuse, lit != 0) == (free_b + reuse) / 100 * 85 / slot_bytes(lit != 0), "auto_target: 85 %%");
  }
  EXPECT(kMaxSlots < (size_t(1) << 31) && kMinSlots < kMaxSlots, "slot bounds");
  for (int ring : {4, 8})
    for (int n : {1, 8, 9, 64, 128, 200})
      EXPECT(spill_cap_for(n, ring) == std::max(1, std::min(128, n) - ring), "spill_cap_for(%d, %d) = %d", n, ring,
             spill_cap_for(n, ring));

  // slot counts that WaveArgs::slots or a 32-bit slot index cannot hold
  const SpillLayout spill = spill_layout(1, false, 1, 1);
  const WaveCaps huge{size_t(1) << 60, size_t(1) << 60, size_t(1) << 60, size_t(1) << 60};
  uint32_t np[kMaxTwins] = {};
  np[0] = 1u << 16;
  EXPECT(!check(slice_twins(1u << 15, np, 1, true, false, spill, huge)), "check accepts S = 2^31");
  np[0] = 477218589u;   // x 9 = 2^32 + 5
  const WaveLayout over = slice_twins(9, np, 1, true, false, spill, huge);
  EXPECT(over.tw[0].S == (size_t(1) << 32) + 5 && !check(over), "check accepts S = 2^32 + 5");
  np[0] = 0x7FFFFFFFu;
  EXPECT(check(slice_twins(1, np, 1, true, false, spill, huge)), "check refuses S = 2^31 - 1");
  np[0] = 1u << 16;
  np[1] = 1u << 10;
  EXPECT(!check(slice_twins(1u << 15, np, 2, false, false, spill_layout(2, false, 1, 1), huge)), "check accepts one twin of 2^31");
}

// The OOM halving from `target` ends at kMinSlots or at one sample per batch.
void check_halving(uint32_t spp, uint32_t npix, size_t target, bool lit) {
  ++g_cases;
  int steps = 0;
  for (;; ++steps) {
    const BatchSize bs = size_batch(spp, npix, target, lit);
    if (!can_halve(target, bs.spb)) {
      EXPECT(target == kMinSlots || bs.spb == 1, "halving stopped at target %zu spb %u", target, bs.spb);
      break;
    }
    const size_t next = halve(target);
    EXPECT(next < target && next >= kMinSlots, "halve(%zu) = %zu", target, next);
    if (next >= target || steps > 64) break;
    target = next;
  }
  EXPECT(steps <= 64, "the halving does not end");
}

}  // namespace

int main() {
  // before the first read (wave_env)
  setenv("RTGPU_STREAMS", "9", 1);
  setenv("RTGPU_OVERLAP", "2", 1);
  setenv("RTGPU_SLOTS", "123456", 1);
  setenv("RTGPU_REFILL", "100", 1);
  setenv("RTGPU_MAX_BLOCKS", "77", 1);
  setenv("RTGPU_TAIL_RAYS", "555", 1);
  setenv("RTGPU_TAIL_FIRST", "3", 1);
  setenv("RTGPU_DEBUG_SYNC", "1", 1);
  check_knobs();
  check_sizes();

  // 1, 2, 3, 5 and 64 whole tiles, and a 40x23 image's ragged ones
  std::vector<Image> images = {tile_image(16, 16), tile_image(32, 16), tile_image(48, 16), tile_image(80, 16),
                               tile_image(128, 128), tile_image(40, 23)};
  EXPECT(images[4].tiles.size() == 64 && images[5].tiles.size() == 6 && tile_pixels(images[5].tiles) == 920, "test images");
  for (const Image& im : images) {
    const size_t npix = size_t(tile_pixels(im.tiles));
    for (int streams = 1; streams <= kMaxTwins; ++streams)
      for (int overlap = 0; overlap < 2; ++overlap)
        for (int lit = 0; lit < 2; ++lit)
          for (int feat = 0; feat < 2; ++feat)
            for (uint32_t spp : {1u, 3u, 4096u}) {
              for (size_t target : {npix / 2, npix, kMinSlots, kMaxSlots})
                check_case(im, streams, overlap != 0, lit != 0, feat != 0, spp, target);
              // a target halved until it stops
              size_t target = auto_target(size_t(1) << 45, 0, lit != 0);
              for (int steps = 0; steps < 64; ++steps) {   // check_halving: it ends well before
                check_case(im, streams, overlap != 0, lit != 0, feat != 0, spp, target);
                if (!can_halve(target, size_batch(spp, uint32_t(npix), target, lit != 0).spb)) break;
                target = halve(target);
              }
            }
    for (uint32_t spp : {1u, 3u, 4096u})
      for (size_t target : {kMaxSlots, kMaxSlots - 12345, size_t(5) << 20, kMinSlots + 1, kMinSlots})
        for (int lit = 0; lit < 2; ++lit) check_halving(spp, uint32_t(npix), target, lit != 0);
  }
  check_halving(4096, 1920 * 1080, kMaxSlots, true);
  printf("{\"cases\": %ld, \"fails\": %ld}\n", g_cases, g_fails);
  return g_fails ? 1 : 0;
}
