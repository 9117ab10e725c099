// wave_run.h — test-only: the host build of the production wavefront pipeline
// (go-raytracing_amd/csrc/wavefront.hip kernels: camera, extend, shade,
// shadow, NEE apply, accumulate, finalize) with one lane per workgroup and
// one workgroup per launch, driven like run_batches() over a scene flattened
// by flatten.cpp (emu_scene.h).  tests/wave_emu.cpp runs it over a librtscene
// scene under AddressSanitizer + UBSan; tests/hits_emu.cpp (hits_emu_render)
// over a caller's description as a plain library.  The traversal stack ring
// is 4 entries so deep traversals take the spill path.  Include after
// wavefront.hip (which brings wave_variant.h), wave_layout.h and emu_scene.h.
// Not a product path.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace wave_run {

using namespace rtg;

constexpr int kRing = 4;

// sample_offset: rt_render_params.sample_offset (run_batches' sample_base is
// sample_offset + the batch's first sample)
template <bool kVol, bool kEnvIS, int kShade, bool kQuant, bool kWide = false>
void run(const DScene& sc, const DCamera& cam, WaveArgs a, uint32_t spp, uint32_t spb, int max_depth, float* out,
         uint32_t sample_offset = 0) {
  uint32_t* cnt_stream[2] = {a.counts + CNT_STREAM0, a.counts + CNT_STREAM1};
  uint32_t* fetch_ext = a.counts + CNT_FETCH_EXT;
  for (double* p = a.acc; p < a.acc + size_t(a.npix) * 3; ++p) *p = 0.0;
  const int tail_after = getenv("RTG_EMU_TAIL") ? atoi(getenv("RTG_EMU_TAIL")) : -1;
  // RTG_EMU_OVERLAP=1: the bounce overlap's order (run_batches, WavePlan::
  // overlap): bounce b's k_shadow / k_nee_apply only after bounce b + 1's
  // k_extend has run to its end, the most any interleaving of the two streams
  // can separate them
  const bool ovl = getenv("RTG_EMU_OVERLAP") && atoi(getenv("RTG_EMU_OVERLAP")) > 0;
  auto nee = [&](int b) {   // as run_batches: no lights, no NEE launches
    if (sc.num_lights == 0) return;
    uint32_t* const cnt_sh = a.counts + cnt_shadow(b & 1);
    k_shadow<kRing, false, kVol, kEnvIS, kQuant, kWide>(sc, a, cnt_sh, a.counts + cnt_fetch_sh(b & 1),
                                                        a.counts + cnt_fetch_sh((b + 1) & 1));
    k_nee_apply<kEnvIS>(a, cnt_sh);
  };
  for (uint32_t sa = 0; sa < spp; sa += spb) {
    const uint32_t sb = spp - sa < spb ? spp - sa : spb;
    const uint32_t s0 = sample_offset + sa;
    const uint32_t nslots = sb * a.npix;
    k_set_counts(a.counts, nslots);
    int pending = -1;   // the bounce whose NEE kernels have not run yet (ovl)
    for (int b = 0; b < max_depth; ++b) {
      const int c = b & 1, nx = c ^ 1;
      uint32_t* const cnt_sh = a.counts + cnt_shadow(c);
      uint32_t* const fetch_sh = a.counts + cnt_fetch_sh(c);
      if (b == 0)
        k_extend<kRing, false, kVol, true, kQuant, kWide>(sc, cam, a, a.s[c], cnt_stream[c], cnt_stream[nx], cnt_sh, fetch_sh,
                                                          fetch_ext, s0);
      else
        k_extend<kRing, false, kVol, false, kQuant, kWide>(sc, cam, a, a.s[c], cnt_stream[c], cnt_stream[nx], cnt_sh, fetch_sh,
                                                           fetch_ext, s0);
      if (pending >= 0) { nee(pending); pending = -1; }
      if (b == 0) k_shade<false, kEnvIS, kShade, true>(sc, cam, a, a.s[c], cnt_stream[c], a.s[nx], cnt_stream[nx], cnt_sh, s0, 0u);
      else k_shade<false, kEnvIS, kShade, false>(sc, cam, a, a.s[c], cnt_stream[c], a.s[nx], cnt_stream[nx], cnt_sh, s0,
                                                  uint32_t(b));
      if (ovl) pending = b;
      else nee(b);
      // RTG_EMU_TAIL=b: after bounce b the long-tail kernel carries every
      // path left to its end (run_batches' hand-off, scenes without lights)
      if (sc.num_lights == 0 && tail_after >= 0 && b == tail_after && b + 1 < max_depth) {
        k_tail<kRing, kVol, kShade, kQuant, kWide>(sc, cam, a, a.s[nx], cnt_stream[nx], fetch_ext);
        break;
      }
    }
    if (pending >= 0) nee(pending);
    k_accum(a, sb);
  }
  k_finalize(a, out, 0);
}

// One frame of the flattened scene E: spp samples from sample_offset in
// batches of spb, to depth max_depth, into out (H * W * 3 sums, the buffer
// rt_render returns), through the kernel variants the product picks for the
// scene (wave_variant.h).  Returns the kernels' error flag; *slots: the path
// slots of a batch.
inline int render(const emu::EmuScene& E, uint32_t seed, uint32_t sample_offset, uint32_t spp, uint32_t spb, int max_depth,
                  std::vector<float>& out, size_t* slots) {
  const DScene& d = E.d;
  const DCamera& cam = E.cam;
  const uint32_t npix = uint32_t(cam.width) * uint32_t(cam.height);
  const size_t S = size_t(spb) * npix;
  if (slots) *slots = S;

  // exactly-sized buffers, one allocation per array (render_wave in api.cpp
  // carves the same arrays out of one buffer; separate ones let ASan see a
  // store that leaves its array)
  // Sized as production sizes them (wave_layout.h): a scene without lights
  // gets the first kSlotF4Dark arrays and no job words, and the spill areas
  // hold what the scene's stack bound leaves beyond the ring.
  const bool lit = d.num_lights > 0;
  const int spill_cap = spill_cap_for(int(d.stack_needed), kRing);
  std::vector<std::vector<float4>> f4(slot_f4(lit), std::vector<float4>(S, float4{0.0f, 0.0f, 0.0f, 0.0f}));
  std::vector<uint32_t> q(CNT_WORDS_Q, 0u), sj_info(lit ? S : 0, 0u), sj_vis(lit ? S : 0, 0u);
  std::vector<uint32_t> pixels(npix);
  // bucket-like pixel list: reversed, so slot -> pixel is not the identity
  for (uint32_t i = 0; i < npix; ++i) pixels[i] = npix - 1u - i;
  std::vector<uint32_t> spill(size_t(spill_cap), 0u), spill_sh(size_t(spill_cap), 0u);
  std::vector<double> acc(size_t(npix) * 3, 0.0);
  std::vector<unsigned long long> counters(3 * CNT_BLOCK, 0ull);
  int err = 0;

  WaveArgs a{};
  auto arr = [&](int k) { return f4[size_t(k)].data(); };
  for (int k = 0; k < 2; ++k) a.s[k] = PathStream{arr(3 * k), arr(3 * k + 1), arr(3 * k + 2)};
  a.hit = arr(6); a.Lout = arr(7);
  a.counts = q.data();
  if (lit) {   // as bind_twin: without lights the NEE job pointers stay null
    a.sj_p = arr(8); a.sj_a = arr(9); a.sj_h = arr(10);
    a.ne_a = arr(11); a.ne_h = arr(12); a.ne_beta = arr(13);
    a.sj_info = sj_info.data();
    a.sj_vis = sj_vis.data();
  }
  a.pixels = pixels.data();
  a.npix = npix;
  a.acc = acc.data();
  a.seed = seed;
  a.max_depth = max_depth;
  a.counters = counters.data();
  a.err = &err;
  a.refill = 1;                      // one lane per wave: claim whenever idle
  a.spill = spill.data();
  a.spill_sh = spill_sh.data();
  a.spill_lanes = 1;
  a.spill_cap = spill_cap;
  a.slots = uint32_t(S);
  a.out_pixels = uint32_t(npix);

  out.assign(size_t(npix) * 3, 0.0f);
  const WaveVariant v = pick_variant(d);
  with_traversal(v, [&](auto V, auto Q, auto W) {
    with_shading(v, [&](auto H, auto F) {
      run<decltype(V)::value, decltype(H)::value, decltype(F)::value, decltype(Q)::value, decltype(W)::value>(
          d, cam, a, spp, spb, max_depth, out.data(), sample_offset);
    });
  });
  return err;
}

}  // namespace wave_run
