// wavefront.h — state and launch interface of the wavefront pipeline.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_layout.h"
#include "features.h"   // run_batches' feature mode launches features.hip's kernels
#include "moments.h"    // ... and its moments mode moments.hip's

namespace rtg {

struct RaySource;   // ray_source.h

// Per-bounce path stream: one dense record per live path, indexed by its
// position in this bounce's stream (SoA of 16-B fields, one dwordx4 per lane
// per array, so every kernel reads and writes it coalesced).
// The ray time (camera.go:370) is not carried: it is the path key's camera
// draw, recomputed where needed (ray_time).  The radiance is not carried
// either: it accumulates in place in Lout[slot].
struct PathStream {
  float4* o;        // ray origin.xyz, path slot (sample_in_batch * npix + pixel_in_list)
  float4* d;        // ray direction.xyz, RNG path key
  float4* beta;     // throughput.xyz, state (depth_left | bounce<<16 | allow<<31)
};

// float4 arrays per path slot: two path streams (3 each), hit, Lout, six NEE
// job fields; plus two uint32 job words (sj_info, sj_vis).  Scenes without
// lights write no NEE job (sampleLightMIS needs a light, camera.go:502): their
// slots hold the first kSlotF4Dark arrays only, and no job words.
constexpr int kSlotF4 = 14;
constexpr int kSlotF4Dark = 8;

struct WaveArgs {
  PathStream s[2];  // ping-pong: bounce b reads s[b&1], writes survivors to s[(b&1)^1]
  float4* hit;      // per stream position: t, kind<<28|idx (0 = miss), instance, -
  float4* Lout;     // per path slot: radiance.xyz, accumulated in place (k_camera zeroes it,
                    // k_shade adds emission / background, k_nee_apply the direct light)
  // NEE shadow jobs (one per path that samples a light at this bounce), dense
  float4* sj_p;     // shadow origin.xyz, RNG path key
  float4* sj_a;     // area-light shadow dir.xyz, tmax
  float4* sj_h;     // HDRI shadow dir.xyz, -
  uint32_t* sj_info;  // flags (1 area ray, 2 HDRI ray) | bounce << 8 (bits 2 / 3: nee_probe below)
  uint32_t* sj_vis;   // written by k_shadow: bit r set = ray r unoccluded
  float4* ne_a;     // area-light contribution if visible .xyz (without HDRI importance
                    // sampling: already times the throughput), path slot
  float4* ne_h;     // HDRI contribution if visible .xyz (HDRI importance sampling only)
  float4* ne_beta;  // throughput at the NEE bounce .xyz (HDRI importance sampling only)
  uint32_t* counts; // queue counters, one 128-B line each (CNT_* below)
  const uint32_t* pixels;   // pixel list (y*W + x) of this call's buckets
  uint32_t npix;
  double* acc;      // per listed pixel fp64 sums
  uint32_t seed;
  int32_t max_depth;
  unsigned long long* counters;
  int* err;
  int32_t refill;   // lanes per wave lacking a prefetched item that trigger a claim
  // The path probes' renders (rt_shadow_visibility): a shadow ray that a
  // lifted world primitive occludes stays in its job (traced as the
  // reference traces it) with bit 2 (area) / 3 (HDRI) of sj_info set, which
  // the probe reads as "occluded".  0 in every other render: k_shade clears
  // such a ray and writes no job when none is left.  (In the padding before
  // `spill`: the struct's size and the other offsets are unchanged.)
  uint32_t nee_probe;
  uint32_t* spill;  // traversal-stack spill area: spill_cap entries x spill_lanes (k_extend, k_tail)
  uint32_t* spill_sh;   // k_shadow's (its own area when it overlaps the next k_extend: WavePlan::overlap)
  uint32_t spill_lanes;
  int32_t spill_cap;
  uint32_t slots;   // capacity of every per-slot array (RTG_GUARD bounds checks)
  uint32_t out_pixels;  // pixels of the output frame (RTG_GUARD: k_finalize's scattered store)
  // Rays that miss the world box (world_box_missed) resolved in k_shade
  // instead of in the queues (RT_OPT_EARLY_MISS).  Bit 0
  // (EARLY_NEE): an NEE job whose rays all miss it is applied by k_shade
  // itself (k_shadow would answer "visible" at once) and not written.  Bit 1
  // (EARLY_NEXT): a survivor whose next ray misses it goes to the back of the
  // next stream, filled downwards from `slots` and counted in cnt_back; the
  // next k_extend reads only the front, and the next k_shade shades a back
  // entry with a miss for its hit record.  The host sets the bits only where
  // the box test alone decides such a ray (world_box_decides) and no probe
  // reads a bounce's arrays; 0 = every ray is queued.
  uint32_t early_miss;
};

// Queue counters, each on its own 128-B line (same-line atomics serialise);
// the claim counters are 8 each, one per queue segment / XCD (wavefront.hip
// pool_take, shade_claim), 32 words apart.  The NEE job count and k_shadow's
// claim counters come in two sets, by bounce parity: bounce b's k_shadow /
// k_nee_apply may still run while bounce b + 1's k_extend (which zeroes the
// set of bounce b + 1) runs (WavePlan::overlap).
// The back counts (WaveArgs::early_miss: survivors kept at the back of the
// stream, which k_extend never sees) come in three sets, by bounce modulo 3:
// k_shade b reads set b, adds to set b + 1 and zeroes set b + 2 for the next
// bounce, so no other kernel has to reset them.
enum : int { CNT_STREAM0 = 0, CNT_STREAM1 = 32, CNT_SHADOW = 64, CNT_FETCH_EXT = 128, CNT_FETCH_SH = 384,
             CNT_SHADE_SEG = 896, CNT_BACK = 1152, CNT_WORDS_Q = 1248 };
__host__ __device__ constexpr int cnt_back(uint32_t bounce) { return CNT_BACK + 32 * int(bounce % 3u); }
__host__ __device__ constexpr int cnt_shadow(int parity) { return CNT_SHADOW + 32 * parity; }
__host__ __device__ constexpr int cnt_fetch_sh(int parity) { return CNT_FETCH_SH + 256 * parity; }

// Traversal kernels: an LDS stack ring of kLdsStack entries per lane, the
// rest of the depth (up to kStackMax) spills to global memory.  (A 16-entry
// ring at 6 waves per SIMD measured 745 against 757 Msamples/s for 8 entries
// at 7 waves, round 1.)
constexpr int kLdsStack = 8;
// 128 covers the 8-wide format's bound (flatten.h kStackMax8; BVH4 scenes
// need at most 64, the probe kernels' LDS stack).
constexpr int kStackMax = 128;
constexpr int kSpillLanesPerCU = 2048;   // max resident threads per CU

// Deep renders without lights hand their last paths to one persistent
// launch (k_tail) once at most this many are left (RT_OPT_TAIL).
constexpr int kTailRaysDefault = 1 << 23;
constexpr int kTailFirstDefault = 7;

struct WavePlan {
  uint32_t tail_rays;       // > 0: k_tail takes over at most this many paths left (no lights, depth > 8)
  int32_t tail_first;       // an extra rays-left check after this bounce (the regular ones: 7, 11, 15, ...)
  uint32_t spp;
  uint32_t samples_per_batch;
  uint32_t sample_offset;
  int32_t max_depth;
  int32_t num_cus;
  int32_t max_blocks;       // > 0: cap on the persistent traversal grids (RT_OPT_MAX_BLOCKS)
  int32_t debug_sync;       // RTGPU_DEBUG_SYNC=1: synchronise after every launch, name a failing kernel
  int32_t num_twins;        // 1..kMaxTwins parts of the pixel list on their own streams (run_batches)
  // Bounce overlap (scenes with lights): twin t's k_shadow / k_nee_apply of
  // bounce b run on aux[t] while its k_extend of bounce b + 1 runs on its own
  // stream; ev_shade[t] / ev_nee[t] order them (run_batches).
  int32_t overlap;
  const hipStream_t* aux;
  const hipEvent_t* ev_shade;
  const hipEvent_t* ev_nee;
  uint32_t* probe_host;     // pinned words (two per twin: [t] and [kMaxTwins + t]) for the long-tail early exit
  int* bounces_run;         // out (may be null): bounces the last batch ran (< max_depth after the early exit)
  // Per-launch timing (rt_set_kernel_timing): events 2k and 2k+1 are
  // recorded before and after one extend / shade / shadow launch on its
  // stream; ev_class[2k] names the kernel (low 4 bits, KC_*) and the twin
  // that launched it (bits 4-5).
  hipEvent_t* events;       // nullptr: timing off
  uint8_t* ev_class;
  int max_events;
  int* num_events;
  // Feature mode (rt_render_features, features.hip): non-null = each batch
  // runs bounce 0's k_extend only, then k_features on its hit records (into
  // the unused stream arrays s[0].o / s[0].d: bounce 0 has no stream) and the
  // feature accumulate; feat_acc[t] holds twin t's 8 fp64 sums per listed
  // pixel, and launch_wavefront's `out` is the W*H*8 feature image.
  double* const* feat_acc;
  // Moments mode (rt_render_moments, moments.hip): non-null = the render runs
  // as ever and each batch's k_accum is followed by k_moment_accum over the
  // same Lout entries, k_finalize by k_moment_finalize into `mom_out` (the
  // W*H*2 moments image); mom_acc[t] holds twin t's 2 fp64 sums per listed
  // pixel.  Not with feat_acc or an instrumented run.
  double* const* mom_acc;
  float* mom_out;
  // Ray mode (rt_ray_color, ray_source.hip): non-null = bounce 0's rays are the
  // caller's.  Each batch's k_set_counts (stream 0 empty) is followed by
  // k_ray_source, which writes the valid rays as stream 0 and zeroes Lout, and
  // bounce 0 runs the later-bounce kernels over that stream (launch_bounce 0);
  // the twins' "pixel lists" hold ray indices into ray_src->rays, and
  // launch_wavefront's `out` is the range's 3 floats per ray.  Not with
  // feat_acc, mom_acc, the path probes or an instrumented run.
  // Surface mode (rt_gather_surface), carried by ray_src->kind == SRC_SURFACE:
  // stream 0 holds given vertices (point, unit normal), bounce 0 launches no
  // k_extend and k_shade's surface instantiation in k_shade's place, then
  // k_shadow / k_nee_apply as ever; from bounce 1 on it is the ray mode.  Not
  // with sh_acc either.
  const RaySource* ray_src;
  // SH mode (rt_gather_sh, ray_source.hip): non-null = the ray mode runs as
  // ever under SRC_SPHERE and each batch's k_accum is followed by k_sh_accum
  // over the same Lout entries; k_sh_finalize takes k_finalize's place and
  // writes `sh_out`, the range's 3 * sh_bands^2 floats per point (no rgb sum is
  // written: launch_wavefront's `out` is not read).  sh_acc[t] holds twin t's
  // fp64 sums, coefficient-major over its listed points.  Only together with
  // ray_src; not with feat_acc, mom_acc, the path probes or an instrumented run.
  double* const* sh_acc;
  float* sh_out;
  int32_t sh_bands;
};

enum : uint32_t { EARLY_NEE = 1u, EARLY_NEXT = 2u };   // WaveArgs::early_miss
enum : uint8_t { KC_EXTEND = 0, KC_SHADE = 1, KC_SHADOW = 2, KC_OTHER = 3 };
constexpr int KC_TWIN_SHIFT = 4;   // ev_class bits 4-5: the twin that launched it
// Most halves ("twins") a render's pixel list is split into, each on its own
// stream (RT_OPT_STREAMS).
constexpr int kMaxTwins = 4;
// Counter blocks (16 x u64 each): one per kernel class.
constexpr int CNT_BLOCK = 24;

#ifdef RTG_GUARD
hipError_t guard_report(unsigned int out[4]);   // diagnostic build: first bad index of the renders
#endif
// as[t] / sts[t] for t < plan.num_twins: each twin's buffers and stream.
hipError_t launch_wavefront(const DScene& sc, const DCamera& cam, const WaveArgs* as, const hipStream_t* sts,
                            const WavePlan& plan, bool count, float* out, int accumulate);

}  // namespace rtg
