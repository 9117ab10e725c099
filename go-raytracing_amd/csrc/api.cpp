// api.cpp — implementation of the C-ABI in include/rtgpu.h.
//
// rt_ctx owns one device's copy of the flattened scene and the scratch
// buffers of the render launch.  Each entry point sets its device first
// (cgo calls can land on any OS thread).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rtgpu.h"
#include "dev_layout.h"
#include "build.h"
#include "flatten.h"
#include "probe.h"
#include "query.h"
#include "ray_source.h"
#include "wavefront.h"
#include "wave_layout.h"
#include "denoise.h"
#include "denoise_var.h"
#include "adaptive.h"

using namespace rtg;

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

struct rt_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::string error;
  bool has_scene = false;
  DScene dscene{};
  HostScene host;
  std::vector<DevBuf> scene_bufs;
  size_t scene_bytes = 0;
  // scratch
  DevBuf counters, errflag, accum, rgba, probe;
  // errflag words: [0] sticky render flag (set by the traversal on a stack
  // overflow, cleared only after the host has read it), [1] probe flag
  int* err_pinned = nullptr;        // host copy of errflag[0], read by check_render_error
  hipEvent_t err_ev = nullptr;      // after the copy of the latest render's flag
  bool err_pending = false;         // a render's flag copy is in flight
  hipEvent_t kev0 = nullptr, kev1 = nullptr;   // render kernel only
  bool kev_recorded = false;
  // wavefront state
  DevBuf wstate, wq, wpix, wacc, wspill;
  uint32_t* probe_pinned = nullptr;
  int num_cus = 0;
  std::vector<uint32_t> pix_host;
  uint32_t* pix_pinned = nullptr;
  size_t pix_pinned_n = 0;
  hipEvent_t pix_ev = nullptr;
  // per-launch kernel timing (rt_set_kernel_timing)
  bool timing = false;
  std::vector<hipEvent_t> tev;
  std::vector<uint8_t> tev_class;
  int tev_used = 0;
  // (contexts lift the world quads / spheres, RT_OPT_LIFT_PRIMS; the struct's own default keeps them in the BVH)
  FlattenOptions fopt = [] { FlattenOptions o; o.lift_prims = 1; return o; }();
  // schedule options (RT_OPT_BATCH_SLOTS / RT_OPT_REFILL / RT_OPT_MAX_BLOCKS /
  // RT_OPT_TAIL / RT_OPT_STREAMS / RT_OPT_OVERLAP; 0 = automatic): they change
  // how the work is dealt, never the result
  WaveOptions wopt;
  // rt_render_features (RenderRun::feat): wfacc = 8 fp64 sums per listed
  // pixel, feat = the host variant's device image
  DevBuf wfacc, feat;
  // rt_denoise: the guide image and the two ping-pong images (one allocation),
  // and the host variant's device copies of its arrays
  DevBuf dn_work, dn_in, dn_feat, dn_out;
  // rt_render_moments (RenderRun::mom_out): wmacc = 2 fp64 sums per listed
  // pixel, mom = the host variant's device image
  DevBuf wmacc, mom;
  // rt_denoise_variance: its working images (one allocation), and the host
  // variant's device copies of the moments and the variance (the other
  // arrays share rt_denoise's copies)
  DevBuf dv_work, dv_mom, dv_var;
  // rt_render_adaptive: ad_work = the working count image, the call's pixel
  // list, the selection's flags and block counts (one allocation; the active
  // list itself is written into wpix, where render_wave reads it), ad_counts =
  // the host variants' device copy of the caller's count image, ad_pinned =
  // where a round's list length reaches the host
  DevBuf ad_work, ad_counts;
  uint32_t* ad_pinned = nullptr;
  // bounce overlap (WavePlan::overlap): each twin's k_shadow / k_nee_apply
  // stream and the events that order it against the twin's own stream
  // (created at the first overlapped render)
  hipStream_t aux_st[kMaxTwins] = {};
  hipEvent_t ev_shade[kMaxTwins] = {}, ev_nee[kMaxTwins] = {};
  // twins of the last render (render_wave): the second's stream, the join
  // events, and where each twin's hit records and pixels are
  hipStream_t twin_st[kMaxTwins - 1] = {};   // twins 1.. (twin 0 runs on the caller's stream)
  hipEvent_t twin_ev0 = nullptr, twin_end[kMaxTwins - 1] = {};
  int num_twins = 1;
  WaveArgs twin_args[kMaxTwins] = {};   // each twin's buffers (the path probes read them)
  int bounces_run = 0;                  // bounces the last render's last batch ran (WavePlan::bounces_run)
  // device BVH build (RT_BLAS_DEVICE) of the last upload
  uint32_t dev_nodes = 0, dev_leaves = 0;   // nodes / leaves added on the device
  double build_ms = 0.0;                    // wall time of the device builds
  // multi-device context (rt_ctx_create_multi): this context is devices[0]
  // and owns one sub-context per further device; a render deals the buckets
  // round-robin over all of them (bucket_renderer.go:193-213's worker pool,
  // one GPU per worker)
  std::vector<rt_ctx*> subs;
  // rt_render_rgba8: the frame's device sums and RGBA8 framebuffer, kept
  // between calls (pixels outside a call's buckets keep their values)
  DevBuf frame, frame_rgba, frame_buckets;
  size_t frame_n = 0;
  hipEvent_t fan_ev = nullptr;    // caller-stream point the devices' renders start after
  hipEvent_t join_ev = nullptr;   // end of this device's share of a render
  // RT_OPT_DEALING: how a multi-device render deals its tiles (set on the
  // primary; RT_DEAL_STATIC round-robin, RT_DEAL_DYNAMIC claimed runs)
  int opt_dealing = RT_DEAL_STATIC;
  int opt_first_share = 0;        // RT_OPT_DEAL_FIRST: first run, percent of a fair share (0 = default)
  hipEvent_t dyn_ev0 = nullptr;   // start of this device's runs in a dynamic render
  bool dyn_span = false;          // the last render was dynamic: its kernel span starts at dyn_ev0
  int32_t dealt_tiles = 0, dealt_runs = 0;   // this device's share of the last multi-device render
  // ray queries (rt_trace_rays / rt_occluded, query.hip): the host variants'
  // staging copies of the rays and the results, and the traversal-stack
  // spill area of the query grid (grown on demand); q_ev follows the latest
  // query launch on q_st, so a query on another stream starts after it (they
  // share the spill area)
  DevBuf q_rays, q_out, q_spill;
  hipEvent_t q_ev = nullptr;
  hipStream_t q_st = nullptr;
  bool q_pending = false;
  // rt_ray_color's and rt_gather's host variants: their staging copies of the
  // records and the sums (rt_gather_rays: of the points and the rays);
  // rc_ev follows the latest call's work on rc_st, so a call on another stream
  // starts after it (they share the batch buffers)
  DevBuf rc_rays, rc_rgb;
  // rt_gather_sh (RenderRun::sh_bands): 3 * bands^2 fp64 sums per listed point
  DevBuf wshacc;
  hipEvent_t rc_ev = nullptr;
  hipStream_t rc_st = nullptr;
  bool rc_pending = false;
};

namespace {

constexpr int CNT_WORDS = 3 * CNT_BLOCK;   // extend, shade, shadow blocks
constexpr int MAX_TIMING_EVENTS = 1 << 16;

int set_err(rt_ctx* c, int code, const std::string& m) {
  if (c) c->error = m;
  return code;
}

int hip_fail(rt_ctx* c, hipError_t e, const char* what) {
  return set_err(c, e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP,
                 std::string(what) + ": " + hipGetErrorString(e));
}

#define HIPCHK(expr)                                  \
  do {                                                \
    hipError_t _e = (expr);                           \
    if (_e != hipSuccess) return hip_fail(ctx, _e, #expr); \
  } while (0)

#ifdef RTG_GUARD
// Diagnostic builds: every scratch buffer is followed by kCanary bytes of a
// known pattern, checked after each render (guard_canaries): a store past
// the end of an allocation whose indices were in range for what the kernels
// were told (an undersized buffer) shows up there, which no index check can
// see.
constexpr size_t kCanary = 16384;
constexpr unsigned char kCanaryByte = 0xA5;
#endif

int ensure(rt_ctx* ctx, DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return RT_OK;
  if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; }
  if (bytes == 0) bytes = 16;
#ifdef RTG_GUARD
  hipError_t e = hipMalloc(&b.p, bytes + kCanary);
  if (e == hipSuccess) e = hipMemset(static_cast<char*>(b.p) + bytes, kCanaryByte, kCanary);
#else
  hipError_t e = hipMalloc(&b.p, bytes);
#endif
  if (e != hipSuccess) return hip_fail(ctx, e, "hipMalloc");
  b.bytes = bytes;
  return RT_OK;
}

#ifdef RTG_GUARD
// Number of canary bytes of `b` that no longer hold the pattern (blocks).
size_t canary_damage(const DevBuf& b) {
  if (!b.p) return 0;
  std::vector<unsigned char> h(kCanary);
  if (hipMemcpy(h.data(), static_cast<const char*>(b.p) + b.bytes, kCanary, hipMemcpyDeviceToHost) != hipSuccess) return kCanary;
  size_t bad = 0;
  for (unsigned char c : h) bad += c != kCanaryByte;
  return bad;
}
#endif

// Copies `v` to a new device buffer with room for `extra` more elements and
// kSceneSlack bytes past them: the traversal reads a record as whole 16-B
// vectors from its 4-B-aligned start (the phase-2 gather, device_common.h),
// which may run up to 112 B past the record.
constexpr size_t kSceneSlack = 128;
template <typename T>
int upload_vec(rt_ctx* ctx, const std::vector<T>& v, const T** dst, size_t extra = 0) {
  DevBuf b;
  size_t bytes = (v.size() + extra) * sizeof(T) + kSceneSlack;
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) return hip_fail(ctx, e, "hipMalloc(scene)");
  b.bytes = bytes;
  // On the context's stream, in order with the kernels upload_one launches
  // there (k_tri_shade, k_quantize, the device BVH build), which read these
  // arrays.  (A blocking hipMemcpy from pageable memory may return before its
  // DMA lands, and the context's non-blocking stream is not ordered after
  // it: with three contexts uploading at once on one GPU, k_tri_shade read
  // triangles that were not there yet.)  upload_one synchronises the stream
  // before it returns, so `v` outlives the copy.
  e = hipMemsetAsync(b.p, 0, bytes, ctx->stream);
  if (e == hipSuccess && !v.empty())
    e = hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) { (void)hipFree(b.p); return hip_fail(ctx, e, "hipMemcpy(scene)"); }
  ctx->scene_bufs.push_back(b);
  ctx->scene_bytes += bytes;
  *dst = static_cast<const T*>(b.p);
  return RT_OK;
}

void free_scene(rt_ctx* ctx) {
  for (auto& b : ctx->scene_bufs) (void)hipFree(b.p);
  ctx->scene_bufs.clear();
  ctx->scene_bytes = 0;
  ctx->has_scene = false;
}

void free_buf(DevBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.bytes = 0;
}

int make_camera(rt_ctx* ctx, const rt_camera_desc* c, DCamera& o) {
  if (!c) return set_err(ctx, RT_ERR_INVALID, "camera is NULL");
  if (c->image_width <= 0 || c->image_height <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size");
  for (int a = 0; a < 3; ++a) {
    o.center[a] = float(c->center[a]);
    o.pixel00[a] = float(c->pixel00[a]);
    o.du[a] = float(c->pixel_delta_u[a]);
    o.dv[a] = float(c->pixel_delta_v[a]);
    o.disk_u[a] = float(c->defocus_disk_u[a]);
    o.disk_v[a] = float(c->defocus_disk_v[a]);
    o.background[a] = float(c->background[a]);
  }
  o.defocus = c->defocus_angle > 0.0 ? 1 : 0;   // camera.go:380
  o.use_sky = c->use_sky_gradient ? 1 : 0;
  o.phantom = c->phantom_hdri ? 1 : 0;
  o.cam_max_depth = c->max_depth;
  o.width = c->image_width;
  o.height = c->image_height;
  o.slow = (c->camera_motion || c->free_camera) ? 1 : 0;   // camera.go:373
  o.free_cam = c->free_camera ? 1 : 0;
  for (int a = 0; a < 3; ++a) {
    o.c_orig[a] = float(c->center_motion_orig[a]);
    o.c_dir[a] = float(c->center_motion_dir[a]);
    o.la_orig[a] = float(c->look_at_motion_orig[a]);
    o.la_dir[a] = float(c->look_at_motion_dir[a]);
    o.vup[a] = float(c->vup[a]);
    o.fwd[a] = float(c->forward[a]);
  }
  o.vw = float(c->viewport_width);
  o.vh = float(c->viewport_height);
  o.focus = float(c->focus_dist);
  o.radius = float(c->defocus_radius);
  if (o.slow && !(c->viewport_width > 0.0 && c->viewport_height > 0.0))
    return set_err(ctx, RT_ERR_INVALID, "moving / free camera needs viewport_width and viewport_height");
  return RT_OK;
}

// rt.generateBuckets (bucket_renderer.go:77-125): grid buckets sorted by the
// squared distance of their centre from the image centre (stable here).
std::vector<rt_bucket> default_buckets(int w, int h, int bs) {
  std::vector<rt_bucket> b;
  for (int y = 0; y < h; y += bs)
    for (int x = 0; x < w; x += bs) b.push_back({x, y, std::min(bs, w - x), std::min(bs, h - y)});
  int cx = w / 2, cy = h / 2;
  std::stable_sort(b.begin(), b.end(), [&](const rt_bucket& p, const rt_bucket& q) {
    double dx0 = double(p.x + p.width / 2 - cx), dy0 = double(p.y + p.height / 2 - cy);
    double dx1 = double(q.x + q.width / 2 - cx), dy1 = double(q.y + q.height / 2 - cy);
    return dx0 * dx0 + dy0 * dy0 < dx1 * dx1 + dy1 * dy1;
  });
  return b;
}

// Buckets -> 16x16 work tiles (one workgroup each).
int make_tiles(rt_ctx* ctx, const rt_render_params* p, int W, int H, std::vector<int4>& tiles) {
  std::vector<rt_bucket> bk;
  if (p->buckets && p->num_buckets > 0) bk.assign(p->buckets, p->buckets + p->num_buckets);
  else if (p->buckets == nullptr) bk = default_buckets(W, H, 32);
  for (const rt_bucket& b : bk) {
    if (b.width <= 0 || b.height <= 0 || b.x < 0 || b.y < 0 || b.x + b.width > W || b.y + b.height > H)
      return set_err(ctx, RT_ERR_INVALID, "bucket outside the image");
    for (int y = b.y; y < b.y + b.height; y += 16)
      for (int x = b.x; x < b.x + b.width; x += 16)
        tiles.push_back(make_int4(x, y, std::min(16, b.x + b.width - x), std::min(16, b.y + b.height - y)));
  }
  return RT_OK;
}

// Device errors of earlier renders (the traversal's stack-overflow flag,
// device_common.h trav_step).  The flag word is sticky on the device: each
// render enqueues an async copy of it to pinned memory; this reads that copy
// once the copy has landed (wait: block until it has) and, if set, clears the
// device word in stream order and reports RT_ERR_DEVICE.  rt_render_device
// calls it without waiting on entry; every synchronising entry point
// (rt_render, rt_sync, rt_last_render_kernel_ms, the count runs) waits.
int check_render_error(rt_ctx* ctx, bool wait) {
  if (!ctx->err_pending) return RT_OK;
  if (wait) {
    HIPCHK(hipEventSynchronize(ctx->err_ev));
  } else {
    const hipError_t q = hipEventQuery(ctx->err_ev);
    if (q == hipErrorNotReady) return RT_OK;
    if (q != hipSuccess) return hip_fail(ctx, q, "hipEventQuery(render error flag)");
  }
  ctx->err_pending = false;
  if (*ctx->err_pinned == 0) return RT_OK;
  *ctx->err_pinned = 0;
  HIPCHK(hipMemsetAsync(ctx->errflag.p, 0, sizeof(int), ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return set_err(ctx, RT_ERR_DEVICE, "device traversal stack overflow in a render (its frame is wrong)");
}

// How render_impl / render_wave run a render: where, what the caller wants
// back, and which variant of the path.
struct RenderRun {
  hipStream_t st = nullptr;
  double* ms = nullptr;                          // out: the render's span on `st` (the call then synchronises)
  unsigned long long* host_counters = nullptr;   // out: CNT_WORDS work counters of an instrumented run (synchronises)
  bool feat = false;      // rt_render_features: bounce 0's feature pass into the W*H*8 image `d_out` (WavePlan::feat_acc)
  float* mom_out = nullptr;   // rt_render_moments: also the W*H*2 moments image (WavePlan::mom_acc / mom_out)
  bool probing = false;   // path_probe: every bounce through the wavefront kernels
  // rt_render_adaptive's later rounds: the pixels are the first list_n ids
  // already in `wpix` (no tiles are dealt or staged), and the render continues
  // the span rt_last_render_kernel_ms reports instead of starting a new one
  bool from_list = false;
  uint32_t list_n = 0;
  // rt_ray_color (WavePlan::ray_src; with from_list): the list's entries name
  // rays of `rays`, bounce 0 traces those, and `d_out` holds 3 floats per ray
  const RaySource* rays = nullptr;
  // rt_gather_sh (WavePlan::sh_acc; with rays under SRC_SPHERE): `d_out` holds
  // 3 * sh_bands^2 floats per point in the rgb sums' place
  int sh_bands = 0;
};

// LDS stack ring (kLdsStack entries per lane) + global spill up to
// kStackMax: scenes of any supported depth run with the small ring.
#ifdef RTG_DIAG_RING
constexpr int kRing = RTG_DIAG_RING;   // diagnostic builds (RTG_GUARD): the ring they were compiled for
#else
constexpr int kRing = kLdsStack;
#endif

// The pixel list to `wpix` through pinned staging (async-safe).
int stage_pixels(rt_ctx* ctx, hipStream_t st) {
  const size_t bytes = ctx->pix_host.size() * sizeof(uint32_t);
  HIPCHK(hipEventSynchronize(ctx->pix_ev));   // the last render's copy has left the staging buffer
  if (ctx->pix_pinned_n < ctx->pix_host.size()) {
    if (ctx->pix_pinned) (void)hipHostFree(ctx->pix_pinned);
    ctx->pix_pinned = nullptr;
    ctx->pix_pinned_n = 0;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&ctx->pix_pinned), bytes));
    ctx->pix_pinned_n = ctx->pix_host.size();
  }
  std::memcpy(ctx->pix_pinned, ctx->pix_host.data(), bytes);
  HIPCHK(hipMemcpyAsync(ctx->wpix.p, ctx->pix_pinned, bytes, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ctx->pix_ev, st));
  return RT_OK;
}

// The bounce overlap's streams and events, created at the first overlapped render.
int ensure_overlap_streams(rt_ctx* ctx) {
  if (ctx->aux_st[0]) return RT_OK;
  for (int t = 0; t < kMaxTwins; ++t) {
    HIPCHK(hipStreamCreateWithFlags(&ctx->aux_st[t], hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_shade[t], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_nee[t], hipEventDisableTiming));
  }
  return RT_OK;
}

// Per-launch timing (rt_set_kernel_timing): at least `want` events for `plan`.
int provision_timing(rt_ctx* ctx, WavePlan& plan, size_t want) {
  while (ctx->tev.size() < want) {
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreate(&e));
    ctx->tev.push_back(e);
  }
  ctx->tev_class.resize(ctx->tev.size());
  plan.events = ctx->tev.data();
  plan.ev_class = ctx->tev_class.data();
  plan.max_events = int(ctx->tev.size());
  plan.num_events = &ctx->tev_used;
  return RT_OK;
}

#ifdef RTG_GUARD
// Diagnostic build: reports the first out-of-range index of this render and
// every scratch buffer whose canary was overwritten.
int guard_render_report(rt_ctx* ctx, int nt) {
  unsigned int gr[4] = {0, 0, 0, 0};
  HIPCHK(guard_report(gr));
  if (gr[0]) fprintf(stderr, "RTG_GUARD: %u bad indices, first at site %u: index %u >= length %u\n", gr[0], gr[1], gr[2], gr[3]);
  const struct { const char* name; const DevBuf* b; } bufs[] = {
      {"wstate", &ctx->wstate}, {"wq", &ctx->wq}, {"wpix", &ctx->wpix}, {"wacc", &ctx->wacc}, {"wfacc", &ctx->wfacc},
      {"wmacc", &ctx->wmacc}, {"wshacc", &ctx->wshacc},
      {"wspill", &ctx->wspill}, {"counters", &ctx->counters}, {"accum", &ctx->accum}, {"frame", &ctx->frame}};
  for (const auto& x : bufs)
    if (const size_t bad = canary_damage(*x.b))
      fprintf(stderr, "RTG_GUARD: %zu canary bytes past %s (%zu bytes) overwritten (%d twins)\n", bad, x.name, x.b->bytes, nt);
  return RT_OK;
}
#endif

// Wavefront render (wavefront.hip) of the tiles' pixels, or (run.from_list)
// of a pixel list that is already in `wpix`.  wave_layout.h decides the
// schedule and where every twin's arrays lie; this allocates, binds and
// launches.
int render_wave(rt_ctx* ctx, const DCamera& dc, const rt_render_params* p, const std::vector<int4>& tiles, float* d_out,
                const RenderRun& run) {
  hipStream_t st = run.st;
  const bool count = run.host_counters != nullptr;
  const bool lit = ctx->dscene.num_lights > 0;
  const uint32_t spp = uint32_t(p->samples_per_pixel);
  int rc;
  // the knobs, the twins, and the pixel list dealt to them
  const WaveKnobs knobs = resolve_knobs(ctx->wopt, run.probing);
  const bool overlap = use_overlap(knobs, lit);
  if (run.from_list && run.list_n == 0) return RT_OK;   // an empty list launches nothing
  const int nt = run.from_list
                     ? choose_twins(knobs, ctx->dscene.shade_kind == SHADE_VOL, overlap, run.list_n,
                                    p->samples_per_pixel, run.list_n)
                     : choose_twins(knobs, ctx->dscene.shade_kind == SHADE_VOL, overlap, tile_pixels(tiles),
                                    p->samples_per_pixel, tiles.size());
  uint32_t twin_npix[kMaxTwins];
  if (run.from_list) split_list(run.list_n, nt, twin_npix);
  else deal_pixels(tiles, dc.width, nt, ctx->pix_host, twin_npix);
  const uint32_t npix = run.from_list ? run.list_n : uint32_t(ctx->pix_host.size());
  // path slots per batch, and the batch buffers: an automatic size that does
  // not fit after all is halved and tried again
  size_t target = knobs.slots;
  const bool auto_slots = target == 0;
  if (auto_slots) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = size_t(8) << 30;
    target = auto_target(free_b, ctx->wstate.bytes + ctx->wq.bytes, lit);
  }
  BatchSize bs{};
  for (;;) {
    bs = size_batch(spp, npix, target, lit);
    if (ctx->wstate.p && ctx->wq.p && ctx->wstate.bytes >= bs.f4_bytes && ctx->wq.bytes >= bs.wq_bytes) break;
    free_buf(ctx->wstate);
    free_buf(ctx->wq);
    rc = ensure(ctx, ctx->wstate, bs.f4_bytes);
    if (!rc) rc = ensure(ctx, ctx->wq, bs.wq_bytes);
    if (!rc) break;
    if (rc != RT_ERR_OOM || !auto_slots || !can_halve(target, bs.spb)) return rc;
    free_buf(ctx->wstate);
    free_buf(ctx->wq);
    (void)hipGetLastError();
    ctx->error.clear();
    target = halve(target);
  }
  // the other buffers
  const SpillLayout spill = spill_layout(nt, overlap, ctx->num_cus, spill_cap_for(int(ctx->dscene.stack_needed), kRing));
  if (run.from_list) {   // the list is there already: growing `wpix` now would lose it
    if (!ctx->wpix.p || ctx->wpix.bytes < size_t(npix) * sizeof(uint32_t))
      return set_err(ctx, RT_ERR_INVALID, "pixel list longer than its buffer");
  } else if ((rc = ensure(ctx, ctx->wpix, npix * sizeof(uint32_t)))) {
    return rc;
  }
  if ((rc = ensure(ctx, ctx->wacc, size_t(npix) * 3 * sizeof(double)))) return rc;
  if (run.feat && (rc = ensure(ctx, ctx->wfacc, size_t(npix) * kFeatFloats * sizeof(double)))) return rc;
  if (run.mom_out && (rc = ensure(ctx, ctx->wmacc, size_t(npix) * kMomFloats * sizeof(double)))) return rc;
  if (run.sh_bands && (rc = ensure(ctx, ctx->wshacc, size_t(npix) * sh_floats(run.sh_bands) * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, ctx->counters, CNT_WORDS * sizeof(unsigned long long)))) return rc;
  if ((rc = ensure(ctx, ctx->wspill, spill.words() * sizeof(uint32_t)))) return rc;
  if (!run.from_list && (rc = stage_pixels(ctx, st))) return rc;
  if (count) HIPCHK(hipMemsetAsync(ctx->counters.p, 0, CNT_WORDS * sizeof(unsigned long long), st));
  if (overlap && (rc = ensure_overlap_streams(ctx))) return rc;
  // each twin's slices of those buffers, checked against what the buffers
  // hold: nothing is launched otherwise
  WaveCaps cap{};
  cap.f4 = ctx->wstate.bytes / sizeof(float4);
  cap.q = std::min(ctx->wq.bytes, bs.wq_bytes) / sizeof(uint32_t);
  cap.pix = std::min(ctx->wpix.bytes / sizeof(uint32_t), ctx->wacc.bytes / (3 * sizeof(double)));
  if (run.feat) cap.pix = std::min(cap.pix, ctx->wfacc.bytes / (kFeatFloats * sizeof(double)));
  if (run.mom_out) cap.pix = std::min(cap.pix, ctx->wmacc.bytes / (kMomFloats * sizeof(double)));
  if (run.sh_bands) cap.pix = std::min(cap.pix, ctx->wshacc.bytes / (sh_floats(run.sh_bands) * sizeof(double)));
  cap.spill = ctx->wspill.bytes / sizeof(uint32_t);
  const WaveLayout lay = slice_twins(bs.spb, twin_npix, nt, lit, overlap, spill, cap);
  if (!check(lay))
    return set_err(ctx, RT_ERR_INVALID, "batch layout refused: a twin's slices leave the batch buffers or its slots reach 2^31");
  WaveArgs as[kMaxTwins]{};
  double* feat_acc[kMaxTwins] = {};   // feature mode: each twin's slice of wfacc
  double* mom_acc[kMaxTwins] = {};    // moments mode: each twin's slice of wmacc
  double* sh_acc[kMaxTwins] = {};     // SH mode: each twin's slice of wshacc (coefficient-major within the twin)
  hipStream_t sts[kMaxTwins] = {st};
  for (int t = 1; t < kMaxTwins; ++t) sts[t] = ctx->twin_st[t - 1];
  for (int t = 0; t < nt; ++t) {
    WaveArgs& a = as[t];
    bind_twin(a, static_cast<float4*>(ctx->wstate.p), static_cast<uint32_t*>(ctx->wq.p),
              static_cast<const uint32_t*>(ctx->wpix.p), static_cast<double*>(ctx->wacc.p),
              static_cast<uint32_t*>(ctx->wspill.p), lay.tw[t], lit);
    if (run.feat) feat_acc[t] = static_cast<double*>(ctx->wfacc.p) + lay.tw[t].pix_off * kFeatFloats;
    if (run.mom_out) mom_acc[t] = static_cast<double*>(ctx->wmacc.p) + lay.tw[t].pix_off * kMomFloats;
    if (run.sh_bands) sh_acc[t] = static_cast<double*>(ctx->wshacc.p) + lay.tw[t].pix_off * sh_floats(run.sh_bands);
    a.seed = p->seed;
    a.max_depth = p->max_depth;
    a.counters = static_cast<unsigned long long*>(ctx->counters.p);
    a.err = static_cast<int*>(ctx->errflag.p);
    a.refill = knobs.refill;
    a.nee_probe = run.probing ? 1u : 0u;
    a.early_miss = early_miss_bits(knobs, early_miss_eligible(ctx->dscene), run.probing, lit, p->max_depth);
    a.spill_lanes = spill.lanes;
    a.spill_cap = spill.cap;
    a.out_pixels = run.rays ? run.rays->num_rays : uint32_t(dc.width) * uint32_t(dc.height);
    ctx->twin_args[t] = a;
  }
  ctx->num_twins = nt;
  WavePlan plan{};
  plan.spp = spp;
  plan.samples_per_batch = bs.spb;
  plan.sample_offset = uint32_t(p->sample_offset);
  plan.max_depth = p->max_depth;
  if (run.feat) {   // bounce 0's closest hit only, whatever depth the caller's params name
    plan.max_depth = 1;
    plan.feat_acc = feat_acc;
  }
  if (run.mom_out) {
    plan.mom_acc = mom_acc;
    plan.mom_out = run.mom_out;
  }
  plan.ray_src = run.rays;
  if (run.sh_bands) {
    plan.sh_acc = sh_acc;
    plan.sh_out = d_out;
    plan.sh_bands = run.sh_bands;
  }
  plan.num_cus = ctx->num_cus;
  plan.max_blocks = knobs.max_blocks;
  plan.num_twins = nt;
  plan.overlap = overlap ? 1 : 0;
  plan.aux = ctx->aux_st;
  plan.ev_shade = ctx->ev_shade;
  plan.ev_nee = ctx->ev_nee;
  plan.debug_sync = knobs.debug_sync;
  plan.probe_host = ctx->probe_pinned;
  plan.bounces_run = &ctx->bounces_run;
  plan.tail_rays = knobs.tail_rays;
  plan.tail_first = knobs.tail_first;
  ctx->tev_used = 0;
  if (ctx->timing &&
      (rc = provision_timing(ctx, plan, timing_events_wanted(spp, bs.spb, p->max_depth, nt, MAX_TIMING_EVENTS))))
    return rc;
  // fan out to the twins' streams, launch, join
  if (run.ms) HIPCHK(hipEventRecord(ctx->ev0, st));
  if (!run.from_list) HIPCHK(hipEventRecord(ctx->kev0, st));
  if (nt > 1) {   // the other twins' streams start after the caller's stream reached here
    HIPCHK(hipEventRecord(ctx->twin_ev0, st));
    for (int t = 1; t < nt; ++t) HIPCHK(hipStreamWaitEvent(ctx->twin_st[t - 1], ctx->twin_ev0, 0));
  }
  HIPCHK(launch_wavefront(ctx->dscene, dc, as, sts, plan, count, d_out, p->accumulate ? 1 : 0));
  for (int t = 1; t < nt; ++t) {   // ... and the caller's stream continues once they have finished
    HIPCHK(hipEventRecord(ctx->twin_end[t - 1], ctx->twin_st[t - 1]));
    HIPCHK(hipStreamWaitEvent(st, ctx->twin_end[t - 1], 0));
  }
  HIPCHK(hipEventRecord(ctx->kev1, st));
  ctx->kev_recorded = true;
  if (run.ms) HIPCHK(hipEventRecord(ctx->ev1, st));
  // the render's error flag follows it to the host asynchronously; it is
  // read by the next entry point that synchronises (check_render_error)
  HIPCHK(hipMemcpyAsync(ctx->err_pinned, ctx->errflag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(ctx->err_ev, st));
  ctx->err_pending = true;
#ifdef RTG_GUARD
  if ((rc = guard_render_report(ctx, nt))) return rc;
#endif
  if (count || run.ms) {
    if ((rc = check_render_error(ctx, true))) return rc;
    if (run.ms) {
      float f = 0.f;
      HIPCHK(hipEventElapsedTime(&f, ctx->ev0, ctx->ev1));
      *run.ms = f;
    }
    if (count)
      HIPCHK(hipMemcpy(run.host_counters, ctx->counters.p, CNT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  }
  return RT_OK;
}

// Shared render path: tiles -> render kernel -> fixed-order reduce into `out`.
int render_impl(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* p, float* d_out, const RenderRun& run) {
  if (!ctx->has_scene) return set_err(ctx, RT_ERR_NO_SCENE, "no scene uploaded");
  if (!p) return set_err(ctx, RT_ERR_INVALID, "params is NULL");
  if (p->samples_per_pixel <= 0 || p->max_depth < 0 || p->sample_offset < 0)
    return set_err(ctx, RT_ERR_INVALID, "bad samples/depth/offset");
  DCamera dc{};
  int rc = make_camera(ctx, cam, dc);
  if (rc) return rc;
  std::vector<int4> tiles;
  rc = make_tiles(ctx, p, dc.width, dc.height, tiles);
  if (rc) return rc;
  if (tiles.empty()) return RT_OK;
  return render_wave(ctx, dc, p, tiles, d_out, run);
}

// Samples a render covers (rt_stats::samples): the buckets' pixels x spp.
uint64_t covered_samples(const rt_camera_desc* cam, const rt_render_params* params) {
  uint64_t px = 0;
  if (params->buckets) for (int i = 0; i < params->num_buckets; ++i) px += uint64_t(params->buckets[i].width) * params->buckets[i].height;
  else px = uint64_t(cam->image_width) * cam->image_height;
  return px * uint64_t(params->samples_per_pixel);
}

// ---- multi-device contexts (rt_ctx_create_multi)
// Runs f(k, ctx_k) for the context and each sub-context, one host thread per
// device (each sets its device first); the first failure's status is
// returned with its message on `ctx`.
template <class F>
int fan_out(rt_ctx* ctx, F f) {
  if (ctx->subs.empty()) return f(0, ctx);
  std::vector<rt_ctx*> cs{ctx};
  cs.insert(cs.end(), ctx->subs.begin(), ctx->subs.end());
  std::vector<int> rc(cs.size(), RT_OK);
  std::vector<std::thread> th;
  for (size_t k = 0; k < cs.size(); ++k)
    th.emplace_back([&, k] {
      if (hipSetDevice(cs[k]->device) != hipSuccess) { rc[k] = set_err(cs[k], RT_ERR_HIP, "hipSetDevice"); return; }
      rc[k] = f(int(k), cs[k]);
    });
  for (auto& t : th) t.join();
  for (size_t k = 0; k < cs.size(); ++k)
    if (rc[k]) {
      if (k) ctx->error = "device " + std::to_string(cs[k]->device) + ": " + cs[k]->error;
      return rc[k];
    }
  return RT_OK;
}

// One device's share of a multi-device render: its buckets into the
// caller's frame on devices[0], on its own stream after the caller's stream
// has reached fan_ev.
int render_share(rt_ctx* ctx, rt_ctx* primary, const rt_camera_desc* cam, const rt_render_params* p,
                 const std::vector<rt_bucket>& share, float* d_out, hipStream_t caller) {
  ctx->kev_recorded = false;
  ctx->dyn_span = false;
  ctx->dealt_tiles = int32_t(share.size());
  ctx->dealt_runs = share.empty() ? 0 : 1;
  if (share.empty()) return RT_OK;
  rt_render_params q = *p;
  q.buckets = share.data();
  q.num_buckets = int32_t(share.size());
  const bool first = ctx == primary;
  hipStream_t s = first ? caller : ctx->stream;
  if (!first) HIPCHK(hipStreamWaitEvent(s, primary->fan_ev, 0));
  int rc = render_impl(ctx, cam, &q, d_out, RenderRun{s});
  if (rc) return rc;
  if (!first) HIPCHK(hipEventRecord(ctx->join_ev, s));
  return RT_OK;
}

// Dynamic dealing (RT_DEAL_DYNAMIC): the reference's worker pool fed by a
// channel (bucket_renderer.go:193-213), one worker per device.  Each
// device's host thread claims a run of consecutive tiles from one shared
// counter, renders it on its own stream, waits for it, and claims again
// until no tile is left, so a device that runs slower (clock, peer-write
// contention) or starts later renders fewer tiles.  A run is a share of the
// tiles left (guided self-scheduling): 1/(2n) of them, the first run
// RT_OPT_DEAL_FIRST percent of a fair share (default 50), none smaller than
// 1/16 of a fair share — each run is one render of its own, with its own
// launch tails, so the runs stay few.  Each pixel is still rendered by
// exactly one device with the same RNG keys, so the frame is bit-identical
// to the static split's and to one device's.
int render_dynamic(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* p,
                   const std::vector<rt_bucket>& tiles, float* d_out, hipStream_t st) {
  rt_ctx* const primary = ctx;
  const size_t n = 1 + ctx->subs.size(), T = tiles.size();
  const size_t fair = (T + n - 1) / n;
  const size_t min_run = std::max<size_t>(1, fair / 16);
  const size_t first_pct = size_t(ctx->opt_first_share ? ctx->opt_first_share : 50);
  const size_t first = std::max(min_run, fair * first_pct / 100);
  std::atomic<size_t> next{0};
  HIPCHK(hipEventRecord(primary->fan_ev, st));
  int rc = fan_out(primary, [&](int, rt_ctx* c) -> int {
    rt_ctx* ctx = c;   // HIPCHK reports on this device's context
    c->kev_recorded = false;
    c->dyn_span = false;
    c->dealt_tiles = 0;
    c->dealt_runs = 0;
    hipStream_t s = c->stream;
    HIPCHK(hipStreamWaitEvent(s, primary->fan_ev, 0));
    HIPCHK(hipEventRecord(c->dyn_ev0, s));
    for (;;) {
      // claim [cur, cur + run): a share of what is left
      size_t cur = next.load(std::memory_order_relaxed), run = 0;
      do {
        if (cur >= T) break;
        const size_t left = T - cur;
        run = c->dealt_runs == 0 ? first : std::max(min_run, (left + 2 * n - 1) / (2 * n));
        run = std::min(run, left);
      } while (!next.compare_exchange_weak(cur, cur + run, std::memory_order_relaxed));
      if (cur >= T) break;
      rt_render_params q = *p;
      q.buckets = tiles.data() + cur;
      q.num_buckets = int32_t(run);
      const int r = render_impl(c, cam, &q, d_out, RenderRun{s});
      if (r) return r;
      c->dealt_tiles += int32_t(run);
      c->dealt_runs += 1;
      // the next claim follows this device's progress
      HIPCHK(hipStreamSynchronize(s));
    }
    c->dyn_span = c->dealt_runs > 0;
    HIPCHK(hipEventRecord(c->join_ev, s));
    return RT_OK;
  });
  if (rc) return rc;
  // the caller's stream continues after every device's runs (already done:
  // each thread waited for its last run)
  HIPCHK(hipStreamWaitEvent(st, primary->join_ev, 0));
  for (rt_ctx* sub : primary->subs) HIPCHK(hipStreamWaitEvent(st, sub->join_ev, 0));
  return RT_OK;
}

// Deals the buckets round-robin over the devices (tile k to
// device k mod G balances the centre-heavy cost of the centre-out bucket
// order) and renders every share concurrently; the caller's stream waits for
// all of them.  Each pixel has one owner, so the frame equals one device's.
int render_multi(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* p, float* d_out, hipStream_t st) {
  if (!p || !cam) return set_err(ctx, RT_ERR_INVALID, "camera / params is NULL");
  if (cam->image_width <= 0 || cam->image_height <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size");
  std::vector<rt_bucket> bk;
  if (p->buckets && p->num_buckets > 0) bk.assign(p->buckets, p->buckets + p->num_buckets);
  else if (p->buckets == nullptr) bk = default_buckets(cam->image_width, cam->image_height, 32);
  const size_t n = 1 + ctx->subs.size();
  // dealt at the kernels' 16x16 tile grain (finer than whole buckets: the
  // centre-heavy cost spreads more evenly over the devices)
  std::vector<rt_bucket> tiles;
  for (const rt_bucket& b : bk)
    for (int y = b.y; y < b.y + b.height; y += 16)
      for (int x = b.x; x < b.x + b.width; x += 16)
        tiles.push_back({x, y, std::min(16, b.x + b.width - x), std::min(16, b.y + b.height - y)});
  if (ctx->opt_dealing == RT_DEAL_DYNAMIC) return render_dynamic(ctx, cam, p, tiles, d_out, st);
  std::vector<std::vector<rt_bucket>> share(n);
  for (size_t i = 0; i < tiles.size(); ++i) share[i % n].push_back(tiles[i]);
  HIPCHK(hipEventRecord(ctx->fan_ev, st));
  int rc = fan_out(ctx, [&](int k, rt_ctx* c) -> int { return render_share(c, ctx, cam, p, share[size_t(k)], d_out, st); });
  if (rc) return rc;
  for (size_t k = 1; k < n; ++k)
    if (!share[k].empty()) HIPCHK(hipStreamWaitEvent(st, ctx->subs[k - 1]->join_ev, 0));
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

static bool create_twin_streams(rt_ctx* ctx) {
  if (hipEventCreateWithFlags(&ctx->twin_ev0, hipEventDisableTiming) != hipSuccess) return false;
  for (int t = 0; t + 1 < kMaxTwins; ++t)
    if (hipStreamCreateWithFlags(&ctx->twin_st[t], hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->twin_end[t], hipEventDisableTiming) != hipSuccess)
      return false;
  return true;
}

int rt_ctx_create(int device, rt_ctx** out) {
  if (!out) return RT_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RT_ERR_HIP;
  if (device < 0 || device >= n) return RT_ERR_INVALID;
  rt_ctx* ctx = new rt_ctx();
  ctx->device = device;
  ctx->errflag.bytes = 2 * sizeof(int);
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->err_ev, hipEventDisableTiming) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&ctx->err_pinned), sizeof(int)) != hipSuccess ||
      hipMalloc(&ctx->errflag.p, 2 * sizeof(int)) != hipSuccess ||
      hipMemset(ctx->errflag.p, 0, 2 * sizeof(int)) != hipSuccess ||
      hipEventCreate(&ctx->kev0) != hipSuccess || hipEventCreate(&ctx->kev1) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->pix_ev, hipEventDisableTiming) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&ctx->probe_pinned), 64) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->fan_ev, hipEventDisableTiming) != hipSuccess ||
      !create_twin_streams(ctx) ||
      hipEventCreateWithFlags(&ctx->join_ev, hipEventDisableTiming) != hipSuccess ||
      hipEventCreate(&ctx->dyn_ev0) != hipSuccess ||
      hipDeviceGetAttribute(&ctx->num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
    delete ctx;
    return RT_ERR_HIP;
  }
  *out = ctx;
  return RT_OK;
}

int rt_device_count(int32_t* n) {
  if (!n) return RT_ERR_INVALID;
  *n = 0;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return RT_ERR_HIP;
  *n = c;
  return RT_OK;
}

int rt_ctx_create_multi(const int32_t* devices, int32_t num_devices, rt_ctx** out) {
  if (!out) return RT_ERR_INVALID;
  *out = nullptr;
  if (!devices || num_devices <= 0) return RT_ERR_INVALID;
  rt_ctx* ctx = nullptr;
  int rc = rt_ctx_create(devices[0], &ctx);
  if (rc) return rc;
  for (int k = 1; k < num_devices; ++k) {
    rt_ctx* sub = nullptr;
    if ((rc = rt_ctx_create(devices[k], &sub))) { rt_ctx_destroy(ctx); return rc; }
    ctx->subs.push_back(sub);
    if (devices[k] != devices[0]) {
      // each device's k_finalize writes its pixels straight into the
      // caller's frame on devices[0] (xGMI peer writes, no staging copy)
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, devices[k], devices[0]) != hipSuccess || !can) {
        rt_ctx_destroy(ctx);
        return RT_ERR_UNSUPPORTED;
      }
      (void)hipSetDevice(devices[k]);
      const hipError_t e = hipDeviceEnablePeerAccess(devices[0], 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { rt_ctx_destroy(ctx); return RT_ERR_HIP; }
      (void)hipGetLastError();   // clear a sticky "already enabled"
    }
  }
  *out = ctx;
  return RT_OK;
}

int rt_ctx_num_devices(const rt_ctx* ctx) { return ctx ? 1 + int(ctx->subs.size()) : 0; }

int rt_last_dealing(const rt_ctx* ctx, int32_t* tiles, int32_t* runs, int32_t max_devices) {
  if (!ctx || !tiles || !runs || max_devices < 0) return RT_ERR_INVALID;
  for (int32_t k = 0; k < max_devices && k <= int32_t(ctx->subs.size()); ++k) {
    const rt_ctx* c = k == 0 ? ctx : ctx->subs[size_t(k - 1)];
    tiles[k] = c->dealt_tiles;
    runs[k] = c->dealt_runs;
  }
  return RT_OK;
}

void rt_ctx_destroy(rt_ctx* ctx) {
  if (!ctx) return;
  for (rt_ctx* s : ctx->subs) rt_ctx_destroy(s);
  ctx->subs.clear();
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  free_scene(ctx);
  free_buf(ctx->counters); free_buf(ctx->errflag);
  free_buf(ctx->accum); free_buf(ctx->rgba); free_buf(ctx->probe);
  if (ctx->err_pinned) (void)hipHostFree(ctx->err_pinned);
  if (ctx->err_ev) (void)hipEventDestroy(ctx->err_ev);
  free_buf(ctx->wstate); free_buf(ctx->wq); free_buf(ctx->wpix); free_buf(ctx->wacc);
  free_buf(ctx->wspill);
  free_buf(ctx->rc_rays); free_buf(ctx->rc_rgb);
  free_buf(ctx->wfacc); free_buf(ctx->feat);
  free_buf(ctx->dn_work); free_buf(ctx->dn_in); free_buf(ctx->dn_feat); free_buf(ctx->dn_out);
  free_buf(ctx->wmacc); free_buf(ctx->mom);
  free_buf(ctx->wshacc);
  free_buf(ctx->dv_work); free_buf(ctx->dv_mom); free_buf(ctx->dv_var);
  free_buf(ctx->ad_work); free_buf(ctx->ad_counts);
  if (ctx->ad_pinned) (void)hipHostFree(ctx->ad_pinned);
  free_buf(ctx->frame); free_buf(ctx->frame_rgba); free_buf(ctx->frame_buckets);
  free_buf(ctx->q_rays); free_buf(ctx->q_out); free_buf(ctx->q_spill);
  if (ctx->q_ev) (void)hipEventDestroy(ctx->q_ev);
  if (ctx->rc_ev) (void)hipEventDestroy(ctx->rc_ev);
  if (ctx->pix_pinned) (void)hipHostFree(ctx->pix_pinned);
  if (ctx->probe_pinned) (void)hipHostFree(ctx->probe_pinned);
  (void)hipEventDestroy(ctx->pix_ev);
  for (hipEvent_t e : ctx->tev) (void)hipEventDestroy(e);
  (void)hipEventDestroy(ctx->kev0);
  (void)hipEventDestroy(ctx->kev1);
  (void)hipEventDestroy(ctx->ev0);
  (void)hipEventDestroy(ctx->ev1);
  if (ctx->fan_ev) (void)hipEventDestroy(ctx->fan_ev);
  if (ctx->twin_ev0) (void)hipEventDestroy(ctx->twin_ev0);
  for (int t = 0; t < kMaxTwins; ++t) {
    if (ctx->aux_st[t]) { (void)hipStreamSynchronize(ctx->aux_st[t]); (void)hipStreamDestroy(ctx->aux_st[t]); }
    if (ctx->ev_shade[t]) (void)hipEventDestroy(ctx->ev_shade[t]);
    if (ctx->ev_nee[t]) (void)hipEventDestroy(ctx->ev_nee[t]);
  }
  for (int t = 0; t + 1 < kMaxTwins; ++t) {
    if (ctx->twin_end[t]) (void)hipEventDestroy(ctx->twin_end[t]);
    if (ctx->twin_st[t]) { (void)hipStreamSynchronize(ctx->twin_st[t]); (void)hipStreamDestroy(ctx->twin_st[t]); }
  }
  if (ctx->join_ev) (void)hipEventDestroy(ctx->join_ev);
  if (ctx->dyn_ev0) (void)hipEventDestroy(ctx->dyn_ev0);
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char* rt_last_error(const rt_ctx* ctx) { return ctx ? ctx->error.c_str() : "null context"; }

int rt_ctx_set_option(rt_ctx* ctx, int32_t key, int32_t value) {
  if (!ctx) return RT_ERR_INVALID;
  for (rt_ctx* s : ctx->subs) {   // multi-device: every device's context
    const int rc = rt_ctx_set_option(s, key, value);
    if (rc) return set_err(ctx, rc, s->error);
  }
  if (key == RT_OPT_BLAS_BUILDER) {
    if (value != RT_BLAS_REFERENCE && value != RT_BLAS_SAH && value != RT_BLAS_DEVICE)
      return set_err(ctx, RT_ERR_INVALID, "bad BLAS builder");
    ctx->fopt.blas_builder = value == RT_BLAS_SAH ? BLAS_SAH : value == RT_BLAS_DEVICE ? BLAS_DEVICE : BLAS_REFERENCE;
    return RT_OK;
  }
  if (key == RT_OPT_TLAS_BUILDER) {
    if (value != RT_BLAS_REFERENCE && value != RT_BLAS_SAH) return set_err(ctx, RT_ERR_INVALID, "bad TLAS builder");
    ctx->fopt.tlas_builder = value == RT_BLAS_SAH ? BLAS_SAH : BLAS_REFERENCE;
    return RT_OK;
  }
  if (key == RT_OPT_NODE_FORMAT) {
    if (value != RT_NODES_FP32 && value != RT_NODES_QUANT8 && value != RT_NODES_WIDE8)
      return set_err(ctx, RT_ERR_INVALID, "bad node format");
    ctx->fopt.quant_nodes = value == RT_NODES_QUANT8 ? 1 : value == RT_NODES_WIDE8 ? 2 : 0;
    return RT_OK;
  }
  if (key == RT_OPT_VOLUMES) {
    if (value != RT_VOLUMES_LIFTED && value != RT_VOLUMES_IN_BVH) return set_err(ctx, RT_ERR_INVALID, "bad volumes option");
    ctx->fopt.lift_volumes = value == RT_VOLUMES_LIFTED ? 1 : 0;
    return RT_OK;
  }
  if (key == RT_OPT_LIFT_PRIMS) {
    if (value != RT_PRIMS_LIFTED && value != RT_PRIMS_IN_BVH) return set_err(ctx, RT_ERR_INVALID, "bad lift-prims option");
    ctx->fopt.lift_prims = value == RT_PRIMS_LIFTED ? 1 : 0;
    return RT_OK;
  }
  if (key == RT_OPT_BVH4_COLLAPSE) {
    if (value != RT_COLLAPSE_SAH && value != RT_COLLAPSE_GREEDY) return set_err(ctx, RT_ERR_INVALID, "bad collapse option");
    ctx->fopt.greedy_collapse = value == RT_COLLAPSE_GREEDY ? 1 : 0;
    return RT_OK;
  }
  if (key == RT_OPT_BATCH_SLOTS) {
    if (value < 0) return set_err(ctx, RT_ERR_INVALID, "bad batch slots");
    ctx->wopt.slots = size_t(value);
    return RT_OK;
  }
  if (key == RT_OPT_REFILL) {
    if (value < 0 || value > 64) return set_err(ctx, RT_ERR_INVALID, "refill must be 0 (default) or 1..64");
    ctx->wopt.refill = value;
    return RT_OK;
  }
  if (key == RT_OPT_STREAMS) {
    if (value < 0 || value > kMaxTwins) return set_err(ctx, RT_ERR_INVALID, "streams must be 0 (default) or 1..4");
    ctx->wopt.streams = value;
    return RT_OK;
  }
  if (key == RT_OPT_OVERLAP) {
    if (value < 0 || value > 2) return set_err(ctx, RT_ERR_INVALID, "overlap must be 0 (default), 1 (off) or 2 (on)");
    ctx->wopt.overlap = value;
    return RT_OK;
  }
  if (key == RT_OPT_EARLY_MISS) {
    if (value < 0 || value > 2) return set_err(ctx, RT_ERR_INVALID, "early miss must be 0 (default), 1 (off) or 2 (on)");
    ctx->wopt.early_miss = value;
    return RT_OK;
  }
  if (key == RT_OPT_TAIL) {
    if (value < 0) return set_err(ctx, RT_ERR_INVALID, "bad tail option");
    ctx->wopt.tail = value;
    return RT_OK;
  }
  if (key == RT_OPT_MAX_BLOCKS) {
    if (value < 0) return set_err(ctx, RT_ERR_INVALID, "bad max blocks");
    ctx->wopt.blocks = value;
    return RT_OK;
  }
  if (key == RT_OPT_DEALING) {
    if (value != RT_DEAL_STATIC && value != RT_DEAL_DYNAMIC) return set_err(ctx, RT_ERR_INVALID, "bad dealing mode");
    ctx->opt_dealing = value;
    return RT_OK;
  }
  if (key == RT_OPT_DEAL_FIRST) {
    if (value < 0 || value > 100) return set_err(ctx, RT_ERR_INVALID, "first run must be 0 (default) or 1..100 percent");
    ctx->opt_first_share = value;
    return RT_OK;
  }
  return set_err(ctx, RT_ERR_INVALID, "unknown option " + std::to_string(key));
}

// RT_BLAS_DEVICE: build every queued mesh BLAS on the device (build.hip),
// point its header at the new root and redo the stack bound.
static int device_builds(rt_ctx* ctx) {
  HostScene& h = ctx->host;
  DScene& d = ctx->dscene;
  const auto t0 = std::chrono::steady_clock::now();
  size_t cap = 0;
  for (const auto& j : h.device_builds) cap += j.n;
  DeviceBuildTarget tgt{};
  tgt.nodes = const_cast<DNode4*>(d.nodes);
  tgt.nodes_used = uint32_t(h.nodes4.size());
  tgt.nodes_cap = uint32_t(h.nodes4.size() + cap);
  tgt.leaves = const_cast<DLeaf*>(d.leaves);
  tgt.leaves_used = uint32_t(h.leaves.size());
  tgt.leaves_cap = uint32_t(h.leaves.size() + cap);
  tgt.tris = const_cast<DTri*>(d.tris);
  tgt.tri_aux = const_cast<DTriAux*>(d.tri_aux);
  tgt.tri_rank = const_cast<int32_t*>(d.tri_rank);
  tgt.tri_hidx = const_cast<int32_t*>(d.tri_hidx);
  int need = h.blas_need4;
  for (const auto& j : h.device_builds) {
    DevBuf boxes;
    int rc = ensure(ctx, boxes, j.boxes.size() * sizeof(DRefBox));
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(boxes.p, j.boxes.data(), j.boxes.size() * sizeof(DRefBox), hipMemcpyHostToDevice,
                                  ctx->stream);   // ordered before the build's kernels on the same stream
    DeviceBuildJob job{j.blas, j.tri_first, j.n, {j.lo[0], j.lo[1], j.lo[2]}, {j.hi[0], j.hi[1], j.hi[2]}};
    DeviceBuildResult res{};
    if (e == hipSuccess) e = build_mesh_blas(job, static_cast<const DRefBox*>(boxes.p), tgt, res, ctx->stream);
    free_buf(boxes);
    if (e != hipSuccess) return hip_fail(ctx, e, "device BVH build");
    if (uint64_t(tgt.nodes_used) + res.nodes_added >= kMaxNodes4)
      return set_err(ctx, RT_ERR_UNSUPPORTED, "device-built BVH exceeds 32-bit BVH4 node offsets");
    tgt.nodes_used += res.nodes_added;
    tgt.leaves_used += res.leaves_added;
    ctx->dev_nodes += res.nodes_added;
    ctx->dev_leaves += res.leaves_added;
    need = std::max(need, res.need4);
    h.blas[size_t(j.blas)].root_item = res.root_item;
    HIPCHK(hipMemcpyAsync(const_cast<DBvh*>(d.blas) + j.blas, &h.blas[size_t(j.blas)], sizeof(DBvh), hipMemcpyHostToDevice,
                          ctx->stream));
  }
  h.stack_needed = (h.tlas_need4 + h.max_leaf_inst + 1 + need + 2) * (h.dfs_order ? 2 : 1);
  if (h.stack_needed > kStackMax)
    return set_err(ctx, RT_ERR_UNSUPPORTED, "device-built BVH too deep for the traversal stack");
  d.stack_needed = h.stack_needed;
  d.n_nodes = tgt.nodes_used;
  d.n_leaves = tgt.leaves_used;
  ctx->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return RT_OK;
}

static int upload_one(rt_ctx* ctx, const rt_scene_desc* scene);

int rt_scene_upload(rt_ctx* ctx, const rt_scene_desc* scene) {
  if (!ctx) return RT_ERR_INVALID;
  // multi-device: flattened and uploaded on every device concurrently
  return fan_out(ctx, [&](int, rt_ctx* c) { return upload_one(c, scene); });
}

static int upload_one(rt_ctx* ctx, const rt_scene_desc* scene) {
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  free_scene(ctx);
  std::string err;
  int rc = flatten_scene(scene, ctx->host, err, ctx->fopt);
  if (rc) return set_err(ctx, rc, err);
  HostScene& h = ctx->host;
  DScene& d = ctx->dscene;
  d = DScene{};
  size_t dev_tris = 0;   // room for the device-built BLASes: < n nodes, <= n leaves each
  for (const auto& j : h.device_builds) dev_tris += j.n;
#define UP(vec, field) if ((rc = upload_vec(ctx, h.vec, &d.field))) { free_scene(ctx); return rc; }
  if ((rc = upload_vec(ctx, h.nodes4, &d.nodes, dev_tris))) { free_scene(ctx); return rc; }
  if ((rc = upload_vec(ctx, h.leaves, &d.leaves, dev_tris))) { free_scene(ctx); return rc; }
  UP(refs, refs);
  UP(ref_rank, ref_rank);
  UP(ref_box, ref_box);
  UP(ref_top, tlas_ref_top);
  UP(spheres, spheres);
  UP(sphere_hidx, sphere_hidx);
  UP(quads, quads);
  UP(quad_hidx, quad_hidx);
  UP(quad_wref, quad_wref);
  UP(sphere_wref, sphere_wref);
  UP(tris, tris);
  UP(tri_aux, tri_aux);
  UP(tri_hidx, tri_hidx);
  UP(planes, planes);
  UP(plane_hidx, plane_hidx);
  UP(instances, instances);
  UP(blas, blas);
  UP(volumes, volumes);
  UP(volume_hidx, volume_hidx);
  UP(vol_refs, vol_refs);
  UP(materials, materials);
  UP(textures, textures);
  UP(lights, lights);
  UP(sphere_rank, sphere_rank);
  UP(quad_rank, quad_rank);
  UP(tri_rank, tri_rank);
  UP(circles, circles);
  UP(circle_rank, circle_rank);
  UP(circle_hidx, circle_hidx);
  UP(perlins, perlins);
  UP(images, images);
  UP(image_texels, image_texels);
  UP(env_texels, env.texels);
  {
    const uint32_t* rgbe = nullptr;
    if (!h.env_rgbe.empty() && (rc = upload_vec(ctx, h.env_rgbe, &rgbe))) { free_scene(ctx); return rc; }
    d.env.rgbe = rgbe;
  }
  UP(env_pdf, env.pdf);
  UP(env_marginal, env.marginal);
  UP(env_conditional, env.conditional);
  if (h.wide_nodes) {
    UP(nodes8, nodes8);
    UP(litems, litems);
    UP(wtris, wtris);
  }
#undef UP
  // every scalar of the scene (counts, node format, shading variant): flatten.h
  if ((rc = scene_scalars(h, d, err))) { free_scene(ctx); return set_err(ctx, rc, err); }
  ctx->dev_nodes = ctx->dev_leaves = 0;
  ctx->build_ms = 0.0;
  if (!h.device_builds.empty() && (rc = device_builds(ctx))) { free_scene(ctx); return rc; }
  // RT_NODES_QUANT8: the traversal's quantised nodes, from every final node
  // (host + device built)
  if (d.quant_nodes) {
    if ((rc = upload_vec(ctx, std::vector<DNodeQ>(), &d.qnodes, d.n_nodes))) { free_scene(ctx); return rc; }
    if (hipError_t qe = quantize_nodes(d.nodes, const_cast<DNodeQ*>(d.qnodes), d.n_nodes, ctx->stream)) {
      rc = hip_fail(ctx, qe, "node quantisation");
      free_scene(ctx);
      return rc;
    }
  }
  // the winners' shading records, from the final triangle order (host +
  // device built)
  if ((rc = upload_vec(ctx, std::vector<DTriShade>(), &d.tri_shade, d.n_tris))) { free_scene(ctx); return rc; }
  if (hipError_t te = pack_tri_shade(d.tris, d.tri_aux, const_cast<DTriShade*>(d.tri_shade), d.n_tris, ctx->stream)) {
    rc = hip_fail(ctx, te, "triangle shading records");
    free_scene(ctx);
    return rc;
  }
  // the lifted volumes as DVolRec records (k_shade keeps them in LDS)
  const std::vector<DVolRec> vrecs = build_vol_recs(h);
  if (!vrecs.empty() && (rc = upload_vec(ctx, vrecs, &d.vol_recs))) { free_scene(ctx); return rc; }
  // the world quads / spheres lifted out of the world BVH (k_shade's lift variants)
  if (d.num_prim_recs > 0 && (rc = upload_vec(ctx, h.prim_recs, &d.prim_recs))) { free_scene(ctx); return rc; }
  build_inst_entries(h);   // BLAS roots are final now
  if ((rc = upload_vec(ctx, h.inst_entries, &d.inst_entry))) { free_scene(ctx); return rc; }
  // every copy and upload kernel has landed before the scene is used (by
  // any stream) and before the host arrays can change
  if (hipError_t se = hipStreamSynchronize(ctx->stream)) {
    rc = hip_fail(ctx, se, "scene upload");
    free_scene(ctx);
    return rc;
  }
  ctx->has_scene = true;
  return RT_OK;
}

int rt_last_build_ms(const rt_ctx* ctx, double* ms) {
  if (!ctx || !ms) return RT_ERR_INVALID;
  *ms = ctx->build_ms;
  return RT_OK;
}

int rt_scene_lifted_prims(const rt_ctx* ctx, int32_t* count) {
  if (!ctx || !count) return RT_ERR_INVALID;
  if (!ctx->has_scene) return RT_ERR_NO_SCENE;
  *count = int32_t(ctx->host.prim_recs.size());
  return RT_OK;
}

int rt_scene_get_info(const rt_ctx* ctx, rt_scene_info* o) {
  if (!ctx || !o) return RT_ERR_INVALID;
  if (!ctx->has_scene) return RT_ERR_NO_SCENE;
  const HostScene& h = ctx->host;
  o->nodes = int(h.nodes4.size() + ctx->dev_nodes);   // device BVH4 nodes
  o->leaves = int(h.leaves.size() + ctx->dev_leaves);
  o->refs = int(h.refs.size());
  o->spheres = int(h.spheres.size());
  o->quads = int(h.quads.size());
  o->triangles = int(h.tris.size());
  o->planes = int(h.planes.size());
  o->instances = int(h.instances.size());
  o->blases = int(h.blas.size());
  o->volumes = int(h.volumes.size());
  o->materials = int(h.materials.size());
  o->textures = int(h.textures.size());
  o->lights = int(h.lights.size());
  o->stack_needed = h.stack_needed;
  o->tlas_depth = h.tlas_depth;
  o->blas_depth = h.blas_depth;
  o->device_bytes = int64_t(ctx->scene_bytes);
  o->node_format = h.wide_nodes ? RT_NODES_WIDE8 : h.quant_nodes ? RT_NODES_QUANT8 : RT_NODES_FP32;
  o->nodes8 = int(h.nodes8.size());
  return RT_OK;
}

int rt_render(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params, float* accum_rgb,
              rt_stats* stats) {
  if (!ctx || !cam || !accum_rgb) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (cam->image_width <= 0 || cam->image_height <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size");
  const size_t n = size_t(cam->image_width) * cam->image_height * 3;
  int rc = ensure(ctx, ctx->accum, n * sizeof(float));
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(ctx->accum.p, accum_rgb, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  double ms = 0.0;
  if (ctx->subs.empty()) {
    rc = render_impl(ctx, cam, params, static_cast<float*>(ctx->accum.p), RenderRun{ctx->stream, &ms});
    if (rc) return rc;
  } else {
    // every device writes its buckets into this device's frame
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = render_multi(ctx, cam, params, static_cast<float*>(ctx->accum.p), ctx->stream))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if ((rc = rt_sync(ctx))) return rc;
  }
  HIPCHK(hipMemcpyAsync(accum_rgb, ctx->accum.p, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (stats) {
    stats->kernel_ms = ms;
    stats->samples = covered_samples(cam, params);
  }
  return RT_OK;
}

int rt_render_device(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params, float* accum_rgb_device,
                     void* hip_stream) {
  if (!ctx || !cam || !accum_rgb_device) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
  // an earlier render's device error surfaces here at the latest (or at the
  // next rt_sync / rt_last_render_kernel_ms)
  int rc = check_render_error(ctx, false);
  if (rc) return rc;
  if (ctx->subs.empty()) return render_impl(ctx, cam, params, accum_rgb_device, RenderRun{st});
  for (rt_ctx* s : ctx->subs) {
    HIPCHK(hipSetDevice(s->device));
    if ((rc = check_render_error(s, false))) return set_err(ctx, rc, s->error);
  }
  HIPCHK(hipSetDevice(ctx->device));
  return render_multi(ctx, cam, params, accum_rgb_device, st);
}

// The feature pass (features.hip) through the render path in its feature
// mode.  A multi-device context runs it on its first device only, like the
// probes.
int rt_render_features(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params, float* feat,
                       rt_stats* stats) {
  if (!ctx || !cam || !params || !feat) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (cam->image_width <= 0 || cam->image_height <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size");
  if (!ctx->has_scene) return set_err(ctx, RT_ERR_NO_SCENE, "no scene uploaded");
  const size_t n = size_t(cam->image_width) * cam->image_height * kFeatFloats;
  int rc = ensure(ctx, ctx->feat, n * sizeof(float));
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(ctx->feat.p, feat, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  double ms = 0.0;
  RenderRun run{ctx->stream, &ms};
  run.feat = true;
  if ((rc = render_impl(ctx, cam, params, static_cast<float*>(ctx->feat.p), run))) return rc;
  HIPCHK(hipMemcpyAsync(feat, ctx->feat.p, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (stats) {
    stats->kernel_ms = ms;
    stats->samples = covered_samples(cam, params);
  }
  return RT_OK;
}

int rt_render_features_device(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                              float* feat_device, void* hip_stream) {
  if (!ctx || !cam || !params || !feat_device) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
  int rc = check_render_error(ctx, false);
  if (rc) return rc;
  RenderRun run{st};
  run.feat = true;
  return render_impl(ctx, cam, params, feat_device, run);
}

int rt_denoise_default_params(rt_denoise_params* p) {
  if (!p) return RT_ERR_INVALID;
  p->iterations = 5;
  p->normal_power_log2 = 5;
  p->demodulate = 1;
  p->sigma_color = 4.0f;
  p->sigma_depth = 0.1f;
  p->albedo_eps = 1e-3f;
  return RT_OK;
}

// rt_denoise / rt_denoise_device: the passes of denoise.hip on `st` over
// device arrays, with the context's guide and ping-pong images.
static int denoise_impl(rt_ctx* ctx, const float* accum, const float* feat, int32_t w, int32_t h, int32_t spp,
                        const rt_denoise_params* params, float* out, hipStream_t st) {
  rt_denoise_params dp;
  rt_denoise_default_params(&dp);
  if (params) dp = *params;
  if (w <= 0 || h <= 0 || spp <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size or samples");
  if (dp.iterations < 0 || dp.iterations > kDnMaxIterations) return set_err(ctx, RT_ERR_INVALID, "iterations outside 0..8");
  if (dp.normal_power_log2 < 0 || dp.normal_power_log2 > 16) return set_err(ctx, RT_ERR_INVALID, "normal_power_log2 outside 0..16");
  if (!(dp.sigma_color > 0.0f) || !(dp.sigma_depth >= 0.0f) || !(dp.albedo_eps > 0.0f))
    return set_err(ctx, RT_ERR_INVALID, "sigma_color / albedo_eps must be > 0, sigma_depth >= 0");
  const size_t n = size_t(w) * size_t(h);
  if (reinterpret_cast<uintptr_t>(feat) % 16 != 0) return set_err(ctx, RT_ERR_INVALID, "feature image not 16-B aligned");
  {   // the passes read the input while the last one writes the output
    const char* a0 = reinterpret_cast<const char*>(accum);
    const char* o0 = reinterpret_cast<const char*>(out);
    if (a0 < o0 + n * 12 && o0 < a0 + n * 12) return set_err(ctx, RT_ERR_INVALID, "output overlaps the input");
  }
  if (dp.iterations == 0) {
    HIPCHK(hipMemcpyAsync(out, accum, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    return RT_OK;
  }
  int rc = ensure(ctx, ctx->dn_work, n * 3 * sizeof(float4));
  if (rc) return rc;
  DnArgs a{};
  a.accum = accum; a.feat = feat; a.out = out;
  a.guide = static_cast<float4*>(ctx->dn_work.p);
  a.img[0] = a.guide + n; a.img[1] = a.guide + 2 * n;
  a.w = w; a.h = h; a.spp = float(spp);
  a.normal_power_log2 = dp.normal_power_log2; a.demodulate = dp.demodulate ? 1 : 0;
  a.sigma_color = dp.sigma_color; a.sigma_depth = dp.sigma_depth; a.albedo_eps = dp.albedo_eps;
  HIPCHK(launch_denoise(a, dp.iterations, ctx->num_cus, st));
  return RT_OK;
}

int rt_denoise(rt_ctx* ctx, const float* accum_rgb, const float* feat, int32_t width, int32_t height, int32_t spp,
               const rt_denoise_params* params, float* out_rgb) {
  if (!ctx || !accum_rgb || !feat || !out_rgb) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (width <= 0 || height <= 0 || spp <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size or samples");
  const size_t n = size_t(width) * size_t(height);
  int rc;
  if ((rc = ensure(ctx, ctx->dn_in, n * 3 * sizeof(float)))) return rc;
  if ((rc = ensure(ctx, ctx->dn_feat, n * kFeatFloats * sizeof(float)))) return rc;
  if ((rc = ensure(ctx, ctx->dn_out, n * 3 * sizeof(float)))) return rc;
  HIPCHK(hipMemcpyAsync(ctx->dn_in.p, accum_rgb, n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->dn_feat.p, feat, n * kFeatFloats * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = denoise_impl(ctx, static_cast<const float*>(ctx->dn_in.p), static_cast<const float*>(ctx->dn_feat.p), width,
                         height, spp, params, static_cast<float*>(ctx->dn_out.p), ctx->stream)))
    return rc;
  HIPCHK(hipMemcpyAsync(out_rgb, ctx->dn_out.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return RT_OK;
}

int rt_denoise_device(rt_ctx* ctx, const float* accum_dev, const float* feat_dev, int32_t width, int32_t height,
                      int32_t spp, const rt_denoise_params* params, float* out_dev, void* hip_stream) {
  if (!ctx || !accum_dev || !feat_dev || !out_dev) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
  return denoise_impl(ctx, accum_dev, feat_dev, width, height, spp, params, out_dev, st);
}

// The render in its moments mode (moments.hip): the frame as rt_render
// writes it, and the luminance moments of the same samples.
static const char kMomentsMulti[] = "rt_render_moments on a multi-device context is not supported";

int rt_render_moments(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params, float* accum_rgb,
                      float* moments, rt_stats* stats) {
  if (!ctx || !cam || !params || !accum_rgb || !moments) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->subs.empty()) return set_err(ctx, RT_ERR_UNSUPPORTED, kMomentsMulti);
  if (cam->image_width <= 0 || cam->image_height <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size");
  const size_t n = size_t(cam->image_width) * cam->image_height;
  int rc;
  if ((rc = ensure(ctx, ctx->accum, n * 3 * sizeof(float)))) return rc;
  if ((rc = ensure(ctx, ctx->mom, n * kMomFloats * sizeof(float)))) return rc;
  HIPCHK(hipMemcpyAsync(ctx->accum.p, accum_rgb, n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->mom.p, moments, n * kMomFloats * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  double ms = 0.0;
  RenderRun run{ctx->stream, &ms};
  run.mom_out = static_cast<float*>(ctx->mom.p);
  if ((rc = render_impl(ctx, cam, params, static_cast<float*>(ctx->accum.p), run))) return rc;
  HIPCHK(hipMemcpyAsync(accum_rgb, ctx->accum.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(moments, ctx->mom.p, n * kMomFloats * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (stats) {
    stats->kernel_ms = ms;
    stats->samples = covered_samples(cam, params);
  }
  return RT_OK;
}

int rt_render_moments_device(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                             float* accum_rgb_device, float* moments_device, void* hip_stream) {
  if (!ctx || !cam || !params || !accum_rgb_device || !moments_device) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->subs.empty()) return set_err(ctx, RT_ERR_UNSUPPORTED, kMomentsMulti);
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
  int rc = check_render_error(ctx, false);
  if (rc) return rc;
  RenderRun run{st};
  run.mom_out = moments_device;
  return render_impl(ctx, cam, params, accum_rgb_device, run);
}

// ---- adaptive sampling: rounds of the moments-mode render over the pixels
// adaptive.hip's selection lists, until none is left or the budget is spent.
static const char kAdaptiveMulti[] = "rt_render_adaptive on a multi-device context is not supported";

int rt_adaptive_default_params(rt_adaptive_params* p) {
  if (!p) return RT_ERR_INVALID;
  p->min_spp = 16;
  p->step_spp = 16;
  p->neighbourhood = 1;
  p->rel_error = 0.05f;
  p->lum_floor = 0.01f;
  return RT_OK;
}

namespace {

int adaptive_check_params(rt_ctx* ctx, const rt_adaptive_params& ap, int32_t max_spp) {
  if (ap.min_spp < 2) return set_err(ctx, RT_ERR_INVALID, "min_spp must be >= 2");
  if (ap.step_spp < 1) return set_err(ctx, RT_ERR_INVALID, "step_spp must be >= 1");
  if (ap.neighbourhood != 0 && ap.neighbourhood != 1) return set_err(ctx, RT_ERR_INVALID, "neighbourhood outside {0, 1}");
  if (!std::isfinite(ap.rel_error) || !std::isfinite(ap.lum_floor) || ap.rel_error < 0.0f || ap.lum_floor < 0.0f)
    return set_err(ctx, RT_ERR_INVALID, "rel_error / lum_floor must be finite and >= 0");
  if (max_spp < 1) return set_err(ctx, RT_ERR_INVALID, "max_spp must be >= 1");
  if ((int64_t(max_spp) - int64_t(ap.min_spp)) / int64_t(ap.step_spp) + 1 > 256)
    return set_err(ctx, RT_ERR_INVALID, "more than 256 rounds possible");
  return RT_OK;
}

// The context's working arrays for an image of n pixels (one allocation that
// grows, like rt_denoise's), and `wpix` sized for a list of all of them: the
// selection writes there, and a later ensure() would move it.
struct AdWork {
  uint32_t* counts;   // n: each pixel's samples so far (0: not in the call)
  uint32_t* list;     // n: the call's pixels, as round 0 dealt them
  uint32_t* blocks;   // grid: the selection's block counts
  uint32_t* total;    // 1: the active list's length
  uint8_t* flags;     // n
  uint32_t grid;
};

int adaptive_buffers(rt_ctx* ctx, size_t n, AdWork& w) {
  w.grid = ad_grid(n, ctx->num_cus);
  const size_t words = 2 * n + w.grid + 4;
  int rc;
  if ((rc = ensure(ctx, ctx->ad_work, words * sizeof(uint32_t) + n))) return rc;
  if ((rc = ensure(ctx, ctx->wpix, n * sizeof(uint32_t)))) return rc;
  if (!ctx->ad_pinned) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&ctx->ad_pinned), 4 * sizeof(uint32_t)));
  w.counts = static_cast<uint32_t*>(ctx->ad_work.p);
  w.list = w.counts + n;
  w.blocks = w.list + n;
  w.total = w.blocks + w.grid;
  w.flags = reinterpret_cast<uint8_t*>(w.total + 4);
  return RT_OK;
}

// One selection on `st` into `wpix`; waits for it: the host sizes the next
// render by the list's length.
int adaptive_select(rt_ctx* ctx, const float* d_mom, const AdWork& w, int32_t W, int32_t H, uint32_t max_spp,
                    uint32_t cur, const rt_adaptive_params& ap, hipStream_t st, uint32_t* n_out) {
  AdArgs a{};
  a.moments = d_mom;
  a.counts = w.counts;
  a.flags = w.flags;
  a.block_counts = w.blocks;
  a.total = w.total;
  a.list = static_cast<uint32_t*>(ctx->wpix.p);
  a.w = W; a.h = H;
  a.max_spp = max_spp;
  a.cur = cur;
  a.neighbourhood = ap.neighbourhood;
  a.rel_error = ap.rel_error; a.lum_floor = ap.lum_floor;
  HIPCHK(launch_adaptive_select(a, ctx->num_cus, st));
  HIPCHK(hipMemcpyAsync(ctx->ad_pinned, w.total, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  *n_out = *ctx->ad_pinned;
  if (size_t(*n_out) > size_t(W) * size_t(H)) return set_err(ctx, RT_ERR_DEVICE, "selection list longer than the image");
  return RT_OK;
}

constexpr size_t kAdMaxPixels = size_t(1) << 31;   // pixel ids are 32-bit

// The rounds, over device arrays on `st`.  Returns with the last round
// enqueued; the callers wait for it.
int adaptive_impl(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* p, const rt_adaptive_params* ap_in,
                  float* d_accum, float* d_mom, uint32_t* d_counts, hipStream_t st, rt_adaptive_stats* stats) {
  if (!ctx->has_scene) return set_err(ctx, RT_ERR_NO_SCENE, "no scene uploaded");
  rt_adaptive_params ap;
  rt_adaptive_default_params(&ap);
  if (ap_in) ap = *ap_in;
  const int32_t max_spp = p->samples_per_pixel;
  int rc = adaptive_check_params(ctx, ap, max_spp);
  if (rc) return rc;
  if (p->max_depth < 0) return set_err(ctx, RT_ERR_INVALID, "bad depth");
  if (p->sample_offset != 0 || p->accumulate != 0)
    return set_err(ctx, RT_ERR_INVALID, "rt_render_adaptive takes sample_offset 0 and accumulate 0");
  DCamera dc{};
  if ((rc = make_camera(ctx, cam, dc))) return rc;
  const size_t n = size_t(dc.width) * size_t(dc.height);
  if (n > kAdMaxPixels) return set_err(ctx, RT_ERR_INVALID, "image too large");
  std::vector<int4> tiles;
  if ((rc = make_tiles(ctx, p, dc.width, dc.height, tiles))) return rc;
  rt_adaptive_stats s{};
  s.rounds = 1;
  ctx->kev_recorded = false;
  if (tiles.empty()) {
    if (stats) *stats = s;
    return RT_OK;
  }
  AdWork w{};
  if ((rc = adaptive_buffers(ctx, n, w))) return rc;
  HIPCHK(hipMemsetAsync(w.counts, 0, n * sizeof(uint32_t), st));
  // round 0: the buckets' pixels, overwriting
  rt_render_params q = *p;
  uint32_t cur = uint32_t(std::min(ap.min_spp, max_spp));
  q.samples_per_pixel = int32_t(cur);
  RenderRun run{st};
  run.mom_out = d_mom;
  if ((rc = render_wave(ctx, dc, &q, tiles, d_accum, run))) return rc;
  const uint32_t listed = uint32_t(ctx->pix_host.size());
  HIPCHK(hipMemcpyAsync(w.list, ctx->wpix.p, size_t(listed) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  HIPCHK(launch_ad_set_counts(w.list, listed, w.counts, cur, ctx->num_cus, st));
  s.samples = uint64_t(listed) * cur;
  uint32_t active = listed;
  // rounds r >= 1: the pixels still active, continuing their sample sequence
  const std::vector<int4> none;
  while (cur < uint32_t(max_spp)) {
    if ((rc = adaptive_select(ctx, d_mom, w, dc.width, dc.height, uint32_t(max_spp), cur, ap, st, &active))) return rc;
    if (active == 0) break;
    const uint32_t step = std::min(uint32_t(ap.step_spp), uint32_t(max_spp) - cur);
    q.samples_per_pixel = int32_t(step);
    q.sample_offset = int32_t(cur);
    q.accumulate = 1;
    RenderRun more{st};
    more.mom_out = d_mom;
    more.from_list = true;
    more.list_n = active;
    if ((rc = render_wave(ctx, dc, &q, none, d_accum, more))) return rc;
    HIPCHK(launch_ad_set_counts(static_cast<const uint32_t*>(ctx->wpix.p), active, w.counts, cur + step, ctx->num_cus, st));
    cur += step;
    s.samples += uint64_t(active) * step;
    s.rounds += 1;
  }
  s.pixels_at_max = cur >= uint32_t(max_spp) ? int32_t(active) : 0;
  HIPCHK(launch_ad_scatter_counts(w.list, listed, w.counts, d_counts, ctx->num_cus, st));
  HIPCHK(hipEventRecord(ctx->kev1, st));   // the span covers every round and selection
  ctx->kev_recorded = true;
  if (stats) *stats = s;
  return RT_OK;
}

// After the call's last work on `st` has finished: its span, device errors.
int adaptive_finish(rt_ctx* ctx, rt_adaptive_stats* stats) {
  int rc = check_render_error(ctx, true);
  if (rc) return rc;
  if (stats && ctx->kev_recorded) {
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, ctx->kev0, ctx->kev1));
    stats->kernel_ms = f;
  }
  return RT_OK;
}

}  // namespace

int rt_render_adaptive(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                       const rt_adaptive_params* adaptive, float* accum_rgb, float* moments, uint32_t* counts,
                       rt_adaptive_stats* stats) {
  if (!ctx || !cam || !params || !accum_rgb || !moments || !counts) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->subs.empty()) return set_err(ctx, RT_ERR_UNSUPPORTED, kAdaptiveMulti);
  if (cam->image_width <= 0 || cam->image_height <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size");
  if (!ctx->has_scene) return set_err(ctx, RT_ERR_NO_SCENE, "no scene uploaded");
  const size_t n = size_t(cam->image_width) * cam->image_height;
  int rc;
  if ((rc = ensure(ctx, ctx->accum, n * 3 * sizeof(float)))) return rc;
  if ((rc = ensure(ctx, ctx->mom, n * kMomFloats * sizeof(float)))) return rc;
  if ((rc = ensure(ctx, ctx->ad_counts, n * sizeof(uint32_t)))) return rc;
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(ctx->accum.p, accum_rgb, n * 3 * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ctx->mom.p, moments, n * kMomFloats * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ctx->ad_counts.p, counts, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if ((rc = adaptive_impl(ctx, cam, params, adaptive, static_cast<float*>(ctx->accum.p), static_cast<float*>(ctx->mom.p),
                          static_cast<uint32_t*>(ctx->ad_counts.p), st, stats)))
    return rc;
  HIPCHK(hipMemcpyAsync(accum_rgb, ctx->accum.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(moments, ctx->mom.p, n * kMomFloats * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(counts, ctx->ad_counts.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return adaptive_finish(ctx, stats);
}

int rt_render_adaptive_device(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                              const rt_adaptive_params* adaptive, float* accum_rgb_device, float* moments_device,
                              uint32_t* counts_device, rt_adaptive_stats* stats, void* hip_stream) {
  if (!ctx || !cam || !params || !accum_rgb_device || !moments_device || !counts_device) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->subs.empty()) return set_err(ctx, RT_ERR_UNSUPPORTED, kAdaptiveMulti);
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
  int rc = check_render_error(ctx, false);
  if (rc) return rc;
  if ((rc = adaptive_impl(ctx, cam, params, adaptive, accum_rgb_device, moments_device, counts_device, st, stats)))
    return rc;
  HIPCHK(hipStreamSynchronize(st));
  return adaptive_finish(ctx, stats);
}

int rt_adaptive_select(rt_ctx* ctx, const float* moments, const uint32_t* counts, int32_t width, int32_t height,
                       int32_t max_spp, const rt_adaptive_params* params, uint32_t* list_out, uint32_t* n_out) {
  if (!ctx || !moments || !counts || !list_out || !n_out) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (width <= 0 || height <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size");
  rt_adaptive_params ap;
  rt_adaptive_default_params(&ap);
  if (params) ap = *params;
  int rc = adaptive_check_params(ctx, ap, max_spp);
  if (rc) return rc;
  const size_t n = size_t(width) * size_t(height);
  if (n > kAdMaxPixels) return set_err(ctx, RT_ERR_INVALID, "image too large");
  AdWork w{};
  if ((rc = adaptive_buffers(ctx, n, w))) return rc;
  if ((rc = ensure(ctx, ctx->mom, n * kMomFloats * sizeof(float)))) return rc;
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(ctx->mom.p, moments, n * kMomFloats * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(w.counts, counts, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  uint32_t m = 0;
  if ((rc = adaptive_select(ctx, static_cast<const float*>(ctx->mom.p), w, width, height, uint32_t(max_spp), 0u, ap, st,
                            &m)))
    return rc;
  if (m) HIPCHK(hipMemcpy(list_out, ctx->wpix.p, size_t(m) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  *n_out = m;
  return RT_OK;
}

static int normalize_check(rt_ctx* ctx, int32_t channels, int32_t width, int32_t height, int32_t target_spp) {
  if (width <= 0 || height <= 0 || target_spp <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size or samples");
  if (channels < 1 || channels > kAdMaxChannels) return set_err(ctx, RT_ERR_INVALID, "channels outside 1..8");
  return RT_OK;
}

int rt_normalize_samples(rt_ctx* ctx, const float* sums, int32_t channels, const uint32_t* counts, int32_t width,
                         int32_t height, int32_t target_spp, float* out) {
  if (!ctx || !sums || !counts || !out) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  int rc = normalize_check(ctx, channels, width, height, target_spp);
  if (rc) return rc;
  const size_t n = size_t(width) * size_t(height);
  if ((rc = ensure(ctx, ctx->dn_in, n * size_t(channels) * sizeof(float)))) return rc;
  if ((rc = ensure(ctx, ctx->ad_counts, n * sizeof(uint32_t)))) return rc;
  hipStream_t st = ctx->stream;
  float* d = static_cast<float*>(ctx->dn_in.p);
  HIPCHK(hipMemcpyAsync(d, sums, n * size_t(channels) * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ctx->ad_counts.p, counts, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIPCHK(launch_normalize(d, channels, static_cast<const uint32_t*>(ctx->ad_counts.p), n, target_spp, d, ctx->num_cus, st));
  HIPCHK(hipMemcpyAsync(out, d, n * size_t(channels) * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return RT_OK;
}

int rt_normalize_samples_device(rt_ctx* ctx, const float* sums_dev, int32_t channels, const uint32_t* counts_dev,
                                int32_t width, int32_t height, int32_t target_spp, float* out_dev, void* hip_stream) {
  if (!ctx || !sums_dev || !counts_dev || !out_dev) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  int rc = normalize_check(ctx, channels, width, height, target_spp);
  if (rc) return rc;
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
  HIPCHK(launch_normalize(sums_dev, channels, counts_dev, size_t(width) * size_t(height), target_spp, out_dev,
                          ctx->num_cus, st));
  return RT_OK;
}

int rt_denoise_variance_default_params(rt_denoise_var_params* p) {
  if (!p) return RT_ERR_INVALID;
  p->iterations = 5;
  p->normal_power_log2 = 5;
  p->demodulate = 1;
  p->spatial_below = 4;
  p->sigma_lum = 8.0f;
  p->sigma_depth = 0.1f;
  p->albedo_eps = 1e-3f;
  return RT_OK;
}

static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const char* a0 = static_cast<const char*>(a);
  const char* b0 = static_cast<const char*>(b);
  return a && b && a0 < b0 + nb && b0 < a0 + na;
}

// rt_denoise_variance / _device: the kernels of denoise_var.hip on `st` over
// device arrays, with the context's working images.
static int denoise_var_impl(rt_ctx* ctx, const float* accum, const float* feat, const float* moments, int32_t w,
                            int32_t h, int32_t spp, const rt_denoise_var_params* params, float* out, float* out_var,
                            hipStream_t st) {
  rt_denoise_var_params dp;
  rt_denoise_variance_default_params(&dp);
  if (params) dp = *params;
  if (w <= 0 || h <= 0 || spp <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size or samples");
  if (dp.iterations < 0 || dp.iterations > kDvMaxIterations) return set_err(ctx, RT_ERR_INVALID, "iterations outside 0..8");
  if (dp.normal_power_log2 < 0 || dp.normal_power_log2 > 16) return set_err(ctx, RT_ERR_INVALID, "normal_power_log2 outside 0..16");
  if (!(dp.sigma_lum > 0.0f) || !(dp.sigma_depth >= 0.0f) || !(dp.albedo_eps > 0.0f))
    return set_err(ctx, RT_ERR_INVALID, "sigma_lum / albedo_eps must be > 0, sigma_depth >= 0");
  if (dp.spatial_below < 2) return set_err(ctx, RT_ERR_INVALID, "spatial_below must be >= 2");
  const bool spatial = spp < dp.spatial_below;
  if (!spatial && !moments) return set_err(ctx, RT_ERR_INVALID, "moments is NULL while spp >= spatial_below");
  const size_t n = size_t(w) * size_t(h);
  if (reinterpret_cast<uintptr_t>(feat) % 16 != 0) return set_err(ctx, RT_ERR_INVALID, "feature image not 16-B aligned");
  // the passes read the inputs while the last one writes the outputs
  if (ranges_overlap(accum, n * 12, out, n * 12)) return set_err(ctx, RT_ERR_INVALID, "output overlaps the input");
  if (out_var && (ranges_overlap(out_var, n * 4, accum, n * 12) || ranges_overlap(out_var, n * 4, feat, n * 32) ||
                  ranges_overlap(out_var, n * 4, moments, n * 8) || ranges_overlap(out_var, n * 4, out, n * 12)))
    return set_err(ctx, RT_ERR_INVALID, "out_var overlaps an input or out_rgb");
  if (dp.iterations == 0 && !out_var) {
    HIPCHK(hipMemcpyAsync(out, accum, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    return RT_OK;
  }
  int rc = ensure(ctx, ctx->dv_work, n * kDvWorkBytesPerPixel);
  if (rc) return rc;
  DvArgs a{};
  a.accum = accum; a.feat = feat; a.moments = spatial ? nullptr : moments; a.out = out; a.out_var = out_var;
  a.guide = static_cast<float4*>(ctx->dv_work.p);
  a.img[0] = a.guide + n; a.img[1] = a.guide + 2 * n;
  a.var[0] = reinterpret_cast<float*>(a.guide + 3 * n); a.var[1] = a.var[0] + n;
  a.w = w; a.h = h; a.spp = float(spp);
  a.normal_power_log2 = dp.normal_power_log2; a.demodulate = dp.demodulate ? 1 : 0;
  a.spatial = spatial ? 1 : 0;
  a.sigma_lum = dp.sigma_lum; a.sigma_depth = dp.sigma_depth; a.albedo_eps = dp.albedo_eps;
  HIPCHK(launch_denoise_var(a, dp.iterations, ctx->num_cus, st));
  if (dp.iterations == 0) {   // the input, and the initial variance
    HIPCHK(hipMemcpyAsync(out, accum, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(out_var, a.var[0], n * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  return RT_OK;
}

int rt_denoise_variance(rt_ctx* ctx, const float* accum_rgb, const float* feat, const float* moments, int32_t width,
                        int32_t height, int32_t spp, const rt_denoise_var_params* params, float* out_rgb,
                        float* out_var) {
  if (!ctx || !accum_rgb || !feat || !out_rgb) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (width <= 0 || height <= 0 || spp <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size or samples");
  const size_t n = size_t(width) * size_t(height);
  // the host arrays' own overlaps (the device copies below never overlap)
  if (ranges_overlap(accum_rgb, n * 12, out_rgb, n * 12)) return set_err(ctx, RT_ERR_INVALID, "output overlaps the input");
  if (out_var && (ranges_overlap(out_var, n * 4, accum_rgb, n * 12) || ranges_overlap(out_var, n * 4, feat, n * 32) ||
                  ranges_overlap(out_var, n * 4, moments, n * 8) || ranges_overlap(out_var, n * 4, out_rgb, n * 12)))
    return set_err(ctx, RT_ERR_INVALID, "out_var overlaps an input or out_rgb");
  int rc;
  if ((rc = ensure(ctx, ctx->dn_in, n * 3 * sizeof(float)))) return rc;
  if ((rc = ensure(ctx, ctx->dn_feat, n * kFeatFloats * sizeof(float)))) return rc;
  if ((rc = ensure(ctx, ctx->dn_out, n * 3 * sizeof(float)))) return rc;
  if (moments && (rc = ensure(ctx, ctx->dv_mom, n * kMomFloats * sizeof(float)))) return rc;
  if (out_var && (rc = ensure(ctx, ctx->dv_var, n * sizeof(float)))) return rc;
  HIPCHK(hipMemcpyAsync(ctx->dn_in.p, accum_rgb, n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->dn_feat.p, feat, n * kFeatFloats * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (moments)
    HIPCHK(hipMemcpyAsync(ctx->dv_mom.p, moments, n * kMomFloats * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = denoise_var_impl(ctx, static_cast<const float*>(ctx->dn_in.p), static_cast<const float*>(ctx->dn_feat.p),
                             moments ? static_cast<const float*>(ctx->dv_mom.p) : nullptr, width, height, spp, params,
                             static_cast<float*>(ctx->dn_out.p), out_var ? static_cast<float*>(ctx->dv_var.p) : nullptr,
                             ctx->stream)))
    return rc;
  HIPCHK(hipMemcpyAsync(out_rgb, ctx->dn_out.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (out_var) HIPCHK(hipMemcpyAsync(out_var, ctx->dv_var.p, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return RT_OK;
}

int rt_denoise_variance_device(rt_ctx* ctx, const float* accum_dev, const float* feat_dev, const float* moments_dev,
                               int32_t width, int32_t height, int32_t spp, const rt_denoise_var_params* params,
                               float* out_dev, float* out_var_dev, void* hip_stream) {
  if (!ctx || !accum_dev || !feat_dev || !out_dev) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
  return denoise_var_impl(ctx, accum_dev, feat_dev, moments_dev, width, height, spp, params, out_dev, out_var_dev, st);
}

int rt_sync(rt_ctx* ctx) {
  if (!ctx) return RT_ERR_INVALID;
  return fan_out(ctx, [](int, rt_ctx* c) -> int {
    rt_ctx* ctx = c;   // HIPCHK reports on this device's context
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return check_render_error(ctx, true);
  });
}

int rt_last_render_kernel_ms(rt_ctx* ctx, double* ms) {
  if (!ctx || !ms) return RT_ERR_INVALID;
  // multi-device: the slowest device's render kernels
  std::vector<double> per(1 + ctx->subs.size(), -1.0);
  int rc = fan_out(ctx, [&](int k, rt_ctx* c) -> int {
    rt_ctx* ctx = c;
    if (!ctx->kev_recorded) return RT_OK;
    HIPCHK(hipEventSynchronize(ctx->kev1));
    float f = 0.f;
    // a dynamic render: from this device's first run to the end of its last
    HIPCHK(hipEventElapsedTime(&f, ctx->dyn_span ? ctx->dyn_ev0 : ctx->kev0, ctx->kev1));
    per[size_t(k)] = f;
    return check_render_error(ctx, true);
  });
  if (rc) return rc;
  const double mx = *std::max_element(per.begin(), per.end());
  if (mx < 0.0) return set_err(ctx, RT_ERR_INVALID, "no render recorded");
  *ms = mx;
  return RT_OK;
}

namespace {
void fill_counts(const unsigned long long* c, rt_work_counts* out) {
  out->samples = c[0];
  out->rays = c[1];
  out->shadow_rays = c[2];
  out->node_visits = c[3];
  out->sphere_tests = c[4];
  out->quad_tests = c[5];
  out->tri_tests = c[6];
  out->plane_tests = c[7];
  out->instance_visits = c[8];
  out->volume_tests = c[9];
  out->material_fetches = c[10];
  out->env_lookups = c[11];
  out->instance_box_tests = c[12];
  out->stack_spills = c[13];
  out->early_shadow_rays = c[14];
  out->early_rays = c[15];
}
}  // namespace

int rt_count_work_by_kernel(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                            rt_work_counts* out) {
  if (!ctx || !cam || !out) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  unsigned long long c[CNT_WORDS] = {0};
  double ms = 0.0;
  int rc = render_impl(ctx, cam, params, nullptr, RenderRun{ctx->stream, &ms, c});
  if (rc) return rc;
  for (int k = 0; k < 3; ++k) fill_counts(c + k * CNT_BLOCK, out + k);
  return RT_OK;
}

int rt_count_work(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params, rt_work_counts* out) {
  if (!out) return RT_ERR_INVALID;
  rt_work_counts k[3];
  int rc = rt_count_work_by_kernel(ctx, cam, params, k);
  if (rc) return rc;
  k[1].rays = 0;          // shade's: paths shaded (the extend rays again)
  k[1].shadow_rays = 0;   // shade's: NEE jobs (the shadow kernel counts the rays)
  const uint64_t* a = reinterpret_cast<const uint64_t*>(&k[0]);
  const uint64_t* b = reinterpret_cast<const uint64_t*>(&k[1]);
  const uint64_t* d = reinterpret_cast<const uint64_t*>(&k[2]);
  uint64_t* o = reinterpret_cast<uint64_t*>(out);
  for (size_t i = 0; i < sizeof(rt_work_counts) / sizeof(uint64_t); ++i) o[i] = a[i] + b[i] + d[i];
  return RT_OK;
}

int rt_measure_read_bandwidth(rt_ctx* ctx, uint64_t bytes, int32_t reps, double* gbs) {
  if (!ctx || !gbs || reps <= 0 || bytes < (uint64_t(1) << 20)) return RT_ERR_INVALID;
  *gbs = 0.0;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t n = size_t(bytes / sizeof(float4));
  void* buf = nullptr;
  float* sink = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  auto done = [&](int rc) {
    if (buf) (void)hipFree(buf);
    if (sink) (void)hipFree(sink);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
  };
  if (hipMalloc(&buf, n * sizeof(float4)) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&sink), sizeof(float)) != hipSuccess ||
      hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
    return done(set_err(ctx, RT_ERR_HIP, "rt_measure_read_bandwidth: allocation failed"));
  hipError_t e = hipMemsetAsync(buf, 0, n * sizeof(float4), ctx->stream);
  if (e == hipSuccess) e = launch_stream_read(static_cast<const float4*>(buf), n, sink, 1, ctx->stream);   // warm-up
  if (e == hipSuccess) e = hipEventRecord(e0, ctx->stream);
  if (e == hipSuccess) e = launch_stream_read(static_cast<const float4*>(buf), n, sink, reps, ctx->stream);
  if (e == hipSuccess) e = hipEventRecord(e1, ctx->stream);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float ms = 0.0f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  if (e != hipSuccess) return done(hip_fail(ctx, e, "rt_measure_read_bandwidth"));
  *gbs = ms > 0.0f ? double(n) * sizeof(float4) * reps / (double(ms) * 1e6) : 0.0;
  return done(RT_OK);
}

int rt_set_kernel_timing(rt_ctx* ctx, int enable) {
  if (!ctx) return RT_ERR_INVALID;
  ctx->timing = enable != 0;
  return RT_OK;
}

int rt_last_kernel_times(rt_ctx* ctx, rt_kernel_times* out) {
  if (!ctx || !out) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  std::memset(out, 0, sizeof(*out));
  if (ctx->tev_used == 0) return set_err(ctx, RT_ERR_INVALID, "no timed render recorded (rt_set_kernel_timing)");
  HIPCHK(hipEventSynchronize(ctx->kev1));   // after both twins' streams joined
  double* ms[3] = {&out->extend_ms, &out->shade_ms, &out->shadow_ms};
  int32_t* nl[3] = {&out->extend_launches, &out->shade_launches, &out->shadow_launches};
  out->twins = ctx->num_twins;
  // (begin, end) of every launch relative to the first event, per kernel
  // class and twin, in launch order
  std::vector<std::pair<float, float>> iv[3][kMaxTwins];
  for (int i = 0; i + 1 < ctx->tev_used; i += 2) {
    const int c = ctx->tev_class[i] & 15, t = (ctx->tev_class[i] >> KC_TWIN_SHIFT) & (kMaxTwins - 1);
    if (c > KC_SHADOW) continue;
    float b = 0.f, e = 0.f;
    HIPCHK(hipEventElapsedTime(&b, ctx->tev[0], ctx->tev[i]));
    HIPCHK(hipEventElapsedTime(&e, ctx->tev[0], ctx->tev[i + 1]));
    iv[c][t].push_back({b, e});
  }
  for (int c = 0; c < 3; ++c) {
    // twins: the k-th launches of the twins are one launch over the whole
    // render's work; its duration is the union of their intervals
    size_t n = 0;
    for (int t = 0; t < kMaxTwins; ++t) n = std::max(n, iv[c][t].size());
    for (size_t k = 0; k < n; ++k) {
      float b = 0.f, e = 0.f;
      bool any = false;
      for (int t = 0; t < kMaxTwins; ++t) {
        if (k >= iv[c][t].size()) continue;
        const auto& x = iv[c][t][k];
        if (!any) { b = x.first; e = x.second; any = true; }
        else { b = std::min(b, x.first); e = std::max(e, x.second); }
      }
      *ms[c] += double(e - b);
      *nl[c] += 1;
    }
  }
  return RT_OK;
}

int rt_tonemap_rgba8(rt_ctx* ctx, const float* accum_rgb, int32_t width, int32_t height, int32_t spp,
                     uint8_t* rgba_out) {
  if (!ctx || !accum_rgb || !rgba_out || width <= 0 || height <= 0 || spp <= 0) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t n = size_t(width) * height;
  int rc = ensure(ctx, ctx->accum, n * 3 * sizeof(float));
  if (rc) return rc;
  if ((rc = ensure(ctx, ctx->rgba, n * 4))) return rc;
  HIPCHK(hipMemcpyAsync(ctx->accum.p, accum_rgb, n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(launch_tonemap(static_cast<const float*>(ctx->accum.p), int(n), spp, static_cast<uint8_t*>(ctx->rgba.p),
                        ctx->stream));
  HIPCHK(hipMemcpyAsync(rgba_out, ctx->rgba.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return RT_OK;
}

int rt_render_rgba8(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params, uint8_t* rgba_out,
                    rt_stats* stats) {
  if (!ctx || !cam || !params || !rgba_out) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (cam->image_width <= 0 || cam->image_height <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size");
  if (params->samples_per_pixel <= 0) return set_err(ctx, RT_ERR_INVALID, "bad samples");
  const int W = cam->image_width, H = cam->image_height;
  const size_t n = size_t(W) * H;
  int rc;
  if (ctx->frame_n != n) {   // a new frame size: sums and framebuffer start at zero
    if ((rc = ensure(ctx, ctx->frame, n * 3 * sizeof(float)))) return rc;
    if ((rc = ensure(ctx, ctx->frame_rgba, n * 4))) return rc;
    HIPCHK(hipMemsetAsync(ctx->frame.p, 0, n * 3 * sizeof(float), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->frame_rgba.p, 0, n * 4, ctx->stream));
    ctx->frame_n = n;
  }
  std::vector<rt_bucket> bk;
  if (params->buckets && params->num_buckets > 0) bk.assign(params->buckets, params->buckets + params->num_buckets);
  else if (params->buckets == nullptr) bk = default_buckets(W, H, 32);
  for (const rt_bucket& b : bk)
    if (b.width <= 0 || b.height <= 0 || b.x < 0 || b.y < 0 || b.x + b.width > W || b.y + b.height > H)
      return set_err(ctx, RT_ERR_INVALID, "bucket outside the image");
  const auto t0 = std::chrono::steady_clock::now();
  float* fr = static_cast<float*>(ctx->frame.p);
  if (ctx->subs.empty()) rc = render_impl(ctx, cam, params, fr, RenderRun{ctx->stream});
  else rc = render_multi(ctx, cam, params, fr, ctx->stream);
  if (rc) return rc;
  if (!bk.empty()) {   // quantise the rendered buckets on the device (bucket_renderer.go:276-285)
    if ((rc = ensure(ctx, ctx->frame_buckets, bk.size() * sizeof(int4)))) return rc;
    HIPCHK(hipMemcpyAsync(ctx->frame_buckets.p, bk.data(), bk.size() * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
    // the sums hold samples [0, sample_offset + spp) after an accumulating
    // pass that continues the earlier ones, samples [offset, offset + spp)
    // after an overwriting one
    const int32_t nsum = params->accumulate ? params->sample_offset + params->samples_per_pixel : params->samples_per_pixel;
    HIPCHK(launch_tonemap_buckets(fr, W, static_cast<const int4*>(ctx->frame_buckets.p), int(bk.size()), nsum,
                                  static_cast<uint8_t*>(ctx->frame_rgba.p), ctx->stream));
  }
  HIPCHK(hipMemcpyAsync(rgba_out, ctx->frame_rgba.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if ((rc = rt_sync(ctx))) return rc;
  if (stats) {
    stats->kernel_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    uint64_t px = 0;
    for (const rt_bucket& b : bk) px += uint64_t(b.width) * uint64_t(b.height);
    stats->samples = px * uint64_t(params->samples_per_pixel);
  }
  return RT_OK;
}

int rt_read_frame_sums(rt_ctx* ctx, float* accum_out, int64_t num_floats) {
  if (!ctx || !accum_out) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->frame_n == 0 || num_floats != int64_t(ctx->frame_n * 3))
    return set_err(ctx, RT_ERR_INVALID, "no rt_render_rgba8 frame of that size");
  HIPCHK(hipMemcpyAsync(accum_out, ctx->frame.p, ctx->frame_n * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return RT_OK;
}

int rt_primary_hits(rt_ctx* ctx, const rt_camera_desc* cam, uint32_t seed, int32_t sample, int32_t* out_top,
                    int32_t* out_prim, float* out_t) {
  if (!ctx || !cam || !out_top || !out_prim || !out_t) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->has_scene) return set_err(ctx, RT_ERR_NO_SCENE, "no scene uploaded");
  DCamera dc{};
  int rc = make_camera(ctx, cam, dc);
  if (rc) return rc;
  const size_t n = size_t(dc.width) * dc.height;
  if ((rc = ensure(ctx, ctx->probe, n * 12))) return rc;
  int32_t* top = static_cast<int32_t*>(ctx->probe.p);
  int32_t* prim = top + n;
  float* t = reinterpret_cast<float*>(prim + n);
  int* perr = static_cast<int*>(ctx->errflag.p) + 1;   // the probe's own flag word
  HIPCHK(hipMemsetAsync(perr, 0, sizeof(int), ctx->stream));
  HIPCHK(launch_primary(ctx->dscene, dc, seed, sample, top, prim, t, perr,
                        ctx->host.stack_needed <= 32 ? 32 : ctx->host.stack_needed <= 64 ? 64 : 128, ctx->stream));
  HIPCHK(hipMemcpyAsync(out_top, top, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(out_prim, prim, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(out_t, t, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  int flag = 0;
  HIPCHK(hipMemcpy(&flag, perr, sizeof(int), hipMemcpyDeviceToHost));
  if (flag) return set_err(ctx, RT_ERR_DEVICE, "device traversal stack overflow");
  return RT_OK;
}

}  // extern "C"

namespace {
// The path probes: one sample of every pixel rendered by the production
// pipeline to depth bounce + 1 (the rays of bounce k do not depend on the
// depth beyond it: the RNG is keyed by bounce, camera.go:443-518 decides
// nothing by the remaining depth but the phantom HDRI of the camera ray), so
// the records of bounce `bounce` are the last the pipeline wrote: k_extend's
// hit records and the stream it traced, and the NEE jobs with k_shadow's
// visibility words.  `what`: 1 = hits (+ ray), 2 = NEE.  Multi-device
// contexts probe their first device.
int path_probe(rt_ctx* ctx, const rt_camera_desc* cam, uint32_t seed, int32_t sample, int32_t bounce, int what,
               int32_t* out_top, int32_t* out_prim, float* out_t, float* out_ray, int32_t* out_nee) {
  if (!ctx || !cam || sample < 0 || bounce < 0 || bounce > 0x7FFF) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (cam->image_width <= 0 || cam->image_height <= 0) return set_err(ctx, RT_ERR_INVALID, "bad image size");
  if (!ctx->has_scene) return set_err(ctx, RT_ERR_NO_SCENE, "no scene uploaded");
  DCamera dc{};
  int rc = make_camera(ctx, cam, dc);
  if (rc) return rc;
  const size_t n = size_t(cam->image_width) * cam->image_height;
  if ((rc = ensure(ctx, ctx->accum, n * 3 * sizeof(float)))) return rc;
  if ((rc = ensure(ctx, ctx->probe, n * 40))) return rc;
  const rt_render_params p{1, bounce + 1, sample, seed, nullptr, 0, 0};
  // the records of bounce k are read back from the wavefront kernels' arrays:
  // no long-tail kernel (it carries paths in registers)
  RenderRun run{ctx->stream};
  run.probing = true;
  if ((rc = render_impl(ctx, cam, &p, static_cast<float*>(ctx->accum.p), run))) return rc;
  int32_t* top = static_cast<int32_t*>(ctx->probe.p);
  int32_t* prim = top + n;
  float* t = reinterpret_cast<float*>(prim + n);
  float* ray = t + n;
  int32_t* nee = reinterpret_cast<int32_t*>(ray + 6 * n);
  HIPCHK(launch_path_fill(uint32_t(n), top, prim, t, ray, nee, ctx->stream));
  // the long-tail early exit (run_batches) may have ended the render before
  // this bounce: then every path had ended and the fill values stand
  if (ctx->bounces_run > bounce) {
    for (int k = 0; k < ctx->num_twins; ++k) {   // each twin's records (render_wave)
      const WaveArgs& a = ctx->twin_args[k];
      const int c = bounce & 1;
      if (what & 1)
        HIPCHK(launch_path_hits(ctx->dscene, dc, a.hit, a.s[c].o, a.s[c].d, a.counts + (c ? CNT_STREAM1 : CNT_STREAM0),
                                a.pixels, a.npix, seed, uint32_t(sample), bounce, top, prim, t, ray, ctx->stream));
      if ((what & 2) && a.sj_info)   // a scene without lights has no job arrays (render_wave)
        HIPCHK(launch_nee_probe(a.sj_info, a.sj_vis, a.ne_a, a.counts + cnt_shadow(c), a.pixels, a.npix, nee, ctx->stream));
    }
  }
  if (out_top) HIPCHK(hipMemcpyAsync(out_top, top, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_prim) HIPCHK(hipMemcpyAsync(out_prim, prim, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_t) HIPCHK(hipMemcpyAsync(out_t, t, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (out_ray) HIPCHK(hipMemcpyAsync(out_ray, ray, n * 24, hipMemcpyDeviceToHost, ctx->stream));
  if (out_nee) HIPCHK(hipMemcpyAsync(out_nee, nee, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return check_render_error(ctx, true);
}
}  // namespace

extern "C" {

int rt_extend_hits(rt_ctx* ctx, const rt_camera_desc* cam, uint32_t seed, int32_t sample, int32_t bounce,
                   int32_t* out_top, int32_t* out_prim, float* out_t, float* out_ray) {
  if (!out_top || !out_prim || !out_t) return RT_ERR_INVALID;
  return path_probe(ctx, cam, seed, sample, bounce, 1, out_top, out_prim, out_t, out_ray, nullptr);
}

int rt_shadow_visibility(rt_ctx* ctx, const rt_camera_desc* cam, uint32_t seed, int32_t sample, int32_t bounce,
                         int32_t* out_nee) {
  if (!out_nee) return RT_ERR_INVALID;
  return path_probe(ctx, cam, seed, sample, bounce, 2, nullptr, nullptr, nullptr, nullptr, out_nee);
}

int rt_extend_first_hits(rt_ctx* ctx, const rt_camera_desc* cam, uint32_t seed, int32_t sample, int32_t* out_top,
                         int32_t* out_prim, float* out_t) {
  return rt_extend_hits(ctx, cam, seed, sample, 0, out_top, out_prim, out_t, nullptr);
}

}  // extern "C"

// ---- ray queries (query.hip): closest hit and occlusion for the caller's rays
namespace {

constexpr int64_t kQueryStageRays = int64_t(1) << 22;   // rays per staging pass of the host variants (128 MiB)

int query_check(rt_ctx* ctx, const void* rays, int64_t n, const void* out) {
  if (!ctx || !rays || !out || n < 0) return RT_ERR_INVALID;
  return RT_OK;
}

// The refusals of every query, before anything is allocated or launched.
int query_refuse(rt_ctx* ctx, float time) {
  if (!ctx->has_scene) return set_err(ctx, RT_ERR_NO_SCENE, "no scene uploaded");
  if (ctx->dscene.n_volumes > 0)
    return set_err(ctx, RT_ERR_UNSUPPORTED, "ray queries on a scene with volumes are not supported (Volume.Hit needs a path key)");
  if (!std::isfinite(time)) return set_err(ctx, RT_ERR_INVALID, "ray time is not finite");
  return RT_OK;
}

// n > 0 device rays -> n device results on `st`, in launches of at most
// kQueryMaxRays rays.  The spill area is the context's: a query on another
// stream than the latest one's first waits for that one.
int query_device(rt_ctx* ctx, bool any, const rt_ray* rays, int64_t n, float time, void* out, hipStream_t st) {
  const WaveKnobs knobs = resolve_knobs(ctx->wopt, false);
  const int cap = spill_cap_for(int(ctx->dscene.stack_needed), kLdsStack);
  const uint32_t first = uint32_t(std::min<int64_t>(n, int64_t(kQueryMaxRays)));
  const int blocks = query_blocks(ctx->dscene, any, first, ctx->num_cus, knobs.max_blocks);
  const size_t lanes = size_t(blocks) * 256u;
  if (ctx->q_pending && ctx->q_st != st) HIPCHK(hipStreamWaitEvent(st, ctx->q_ev, 0));
  int rc = ensure(ctx, ctx->q_spill, lanes * size_t(cap) * sizeof(uint32_t));
  if (rc) return rc;
  if (!ctx->q_ev) HIPCHK(hipEventCreateWithFlags(&ctx->q_ev, hipEventDisableTiming));
  for (int64_t off = 0; off < n; off += int64_t(kQueryMaxRays)) {
    QueryArgs a{};
    a.rays = reinterpret_cast<const float4*>(rays + off);
    a.out = any ? static_cast<void*>(static_cast<uint8_t*>(out) + off)
                : static_cast<void*>(static_cast<rt_ray_hit*>(out) + off);
    a.n = uint32_t(std::min<int64_t>(n - off, int64_t(kQueryMaxRays)));
    a.time = time;
    a.spill = static_cast<uint32_t*>(ctx->q_spill.p);
    a.spill_lanes = uint32_t(lanes);
    a.spill_cap = cap;
    a.err = static_cast<int*>(ctx->errflag.p);
    // (a shorter last launch never needs more blocks than the first)
    HIPCHK(launch_query(ctx->dscene, any, a, std::min(blocks, int((a.n + 255u) / 256u)), st));
  }
  HIPCHK(hipEventRecord(ctx->q_ev, st));
  ctx->q_st = st;
  ctx->q_pending = true;
  // the error flag follows the query to the host as it follows a render
  HIPCHK(hipMemcpyAsync(ctx->err_pinned, ctx->errflag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(ctx->err_ev, st));
  ctx->err_pending = true;
  return RT_OK;
}

// The host variants: staged through the context's buffers, at most
// kQueryStageRays rays at a time; blocks.
int query_host(rt_ctx* ctx, bool any, const rt_ray* rays, int64_t n, float time, void* out) {
  HIPCHK(hipSetDevice(ctx->device));
  int rc = check_render_error(ctx, true);
  if (rc || (rc = query_refuse(ctx, time)) || n == 0) return rc;
  const size_t out_sz = any ? sizeof(uint8_t) : sizeof(rt_ray_hit);
  const int64_t stage = std::min<int64_t>(n, kQueryStageRays);
  if ((rc = ensure(ctx, ctx->q_rays, size_t(stage) * sizeof(rt_ray)))) return rc;
  if ((rc = ensure(ctx, ctx->q_out, size_t(stage) * out_sz))) return rc;
  for (int64_t off = 0; off < n; off += stage) {
    const int64_t m = std::min<int64_t>(stage, n - off);
    HIPCHK(hipMemcpyAsync(ctx->q_rays.p, rays + off, size_t(m) * sizeof(rt_ray), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = query_device(ctx, any, static_cast<const rt_ray*>(ctx->q_rays.p), m, time, ctx->q_out.p, ctx->stream))) return rc;
    HIPCHK(hipMemcpyAsync(static_cast<char*>(out) + size_t(off) * out_sz, ctx->q_out.p, size_t(m) * out_sz,
                          hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  return check_render_error(ctx, true);
}

int query_async(rt_ctx* ctx, bool any, const rt_ray* rays, int64_t n, float time, void* out, void* hip_stream) {
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
  // an earlier call's device error surfaces here at the latest, as in rt_render_device
  int rc = check_render_error(ctx, false);
  if (rc || (rc = query_refuse(ctx, time)) || n == 0) return rc;
  return query_device(ctx, any, rays, n, time, out, st);
}

// ---- rt_ray_color: the render path in its ray mode (ray_source.hip) ---------

constexpr int64_t kRayColorMaxRays = (int64_t(1) << 31) - 1;

// The refusals that need no device, then the DCamera rayColorInternal reads:
// background, sky, phantom and the depth its test compares with (no geometry).
int ray_color_check(rt_ctx* ctx, const rt_ray_color_params* p, int64_t n, DCamera& dc) {
  if (n < 0 || n > kRayColorMaxRays) return set_err(ctx, RT_ERR_INVALID, "ray count outside 0 .. 2^31 - 1");
  if (p->samples < 1 || p->max_depth < 1 || p->sample_offset < 0 || p->camera_max_depth < 0)
    return set_err(ctx, RT_ERR_INVALID, "bad samples / depth / offset");
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(p->background[a])) return set_err(ctx, RT_ERR_INVALID, "background is not finite");
  if (!ctx->has_scene) return set_err(ctx, RT_ERR_NO_SCENE, "no scene uploaded");
  for (int a = 0; a < 3; ++a) dc.background[a] = float(p->background[a]);
  dc.use_sky = p->use_sky_gradient ? 1 : 0;
  dc.phantom = p->phantom_hdri ? 1 : 0;
  dc.cam_max_depth = p->camera_max_depth ? p->camera_max_depth : p->max_depth;
  dc.width = dc.height = 1;
  return RT_OK;
}

// n > 0 device rays -> n device sums on `st`.  A batch holds at least one
// sample of every ray of a range, so the array is cut into consecutive ranges
// of at most the batch's slots; each range is one render over the identity
// list (ray k of the range -> rgb[3k]), with all its samples, so a ray's sum
// never depends on the cut.  kind (ray_source.h's SRC_*): the records are rays
// (rt_ray_color) or rt_gather's points under one of its sources.
// sh_bands > 0 (rt_gather_sh; kind is SRC_SPHERE): `rgb` holds 3 * sh_bands^2
// floats per point, the SH sums, in the rgb sums' place.
int ray_color_device(rt_ctx* ctx, const DCamera& dc, int32_t kind, const rt_path_ray* rays, int64_t n,
                     const rt_ray_color_params* p, float* rgb, hipStream_t st, int sh_bands = 0) {
  const size_t stride = sh_bands ? size_t(sh_floats(sh_bands)) : 3;   // floats per record of the output
  const bool lit = ctx->dscene.num_lights > 0;
  const WaveKnobs knobs = resolve_knobs(ctx->wopt, false);
  size_t target = knobs.slots;
  if (target == 0) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = size_t(8) << 30;
    target = auto_target(free_b, ctx->wstate.bytes + ctx->wq.bytes, lit);
  }
  const int64_t range = std::max<int64_t>(1, std::min<int64_t>(n, int64_t(std::min(target, kMaxSlots))));
  if (!ctx->rc_ev) HIPCHK(hipEventCreateWithFlags(&ctx->rc_ev, hipEventDisableTiming));
  if (ctx->rc_pending && ctx->rc_st != st) HIPCHK(hipStreamWaitEvent(st, ctx->rc_ev, 0));
  int rc = ensure(ctx, ctx->wpix, size_t(range) * sizeof(uint32_t));
  if (rc) return rc;
  HIPCHK(launch_ray_identity(static_cast<uint32_t*>(ctx->wpix.p), uint32_t(range), ctx->num_cus, st));
  rt_render_params q{};
  q.samples_per_pixel = p->samples;
  q.max_depth = p->max_depth;
  q.sample_offset = p->sample_offset;
  q.seed = p->seed;
  q.accumulate = p->accumulate;
  const std::vector<int4> none;
  ctx->dyn_span = false;
  HIPCHK(hipEventRecord(ctx->kev0, st));   // the span covers every range
  for (int64_t off = 0; off < n; off += range) {
    RaySource src{};
    src.rays = reinterpret_cast<const float4*>(rays + off);
    src.num_rays = uint32_t(std::min<int64_t>(range, n - off));
    src.kind = kind;
    RenderRun run{st};
    run.from_list = true;
    run.list_n = src.num_rays;
    run.rays = &src;
    run.sh_bands = sh_bands;
    if ((rc = render_wave(ctx, dc, &q, none, rgb + stride * size_t(off), run))) return rc;
  }
  HIPCHK(hipEventRecord(ctx->rc_ev, st));
  ctx->rc_st = st;
  ctx->rc_pending = true;
  return RT_OK;
}

// The host variants behind their checks: n host records (rays, or rt_gather's
// points: the same 32 B) staged through the context's buffers, traced, copied
// back; blocks.  invalid: the records the kernel's guard will leave out.
int ray_color_host(rt_ctx* ctx, const DCamera& dc, int32_t kind, const void* recs, int64_t n, const rt_ray_color_params* params,
                   float* rgb, rt_ray_color_stats* stats, uint64_t invalid, int sh_bands = 0) {
  const size_t out_bytes = size_t(n) * (sh_bands ? size_t(sh_floats(sh_bands)) : 3) * sizeof(float);
  int rc = check_render_error(ctx, true);
  if (rc) return rc;
  double ms = 0.0;
  if (n > 0) {
    hipStream_t st = ctx->stream;
    if ((rc = ensure(ctx, ctx->rc_rays, size_t(n) * sizeof(rt_path_ray)))) return rc;
    if ((rc = ensure(ctx, ctx->rc_rgb, out_bytes))) return rc;
    HIPCHK(hipMemcpyAsync(ctx->rc_rays.p, recs, size_t(n) * sizeof(rt_path_ray), hipMemcpyHostToDevice, st));
    if (params->accumulate)
      HIPCHK(hipMemcpyAsync(ctx->rc_rgb.p, rgb, out_bytes, hipMemcpyHostToDevice, st));
    if ((rc = ray_color_device(ctx, dc, kind, static_cast<const rt_path_ray*>(ctx->rc_rays.p), n, params,
                               static_cast<float*>(ctx->rc_rgb.p), st, sh_bands)))
      return rc;
    HIPCHK(hipMemcpyAsync(rgb, ctx->rc_rgb.p, out_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if ((rc = check_render_error(ctx, true))) return rc;
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, ctx->kev0, ctx->kev1));
    ms = f;
  }
  if (stats) {
    stats->kernel_ms = ms;
    stats->samples = uint64_t(n) * uint64_t(params->samples);
    stats->invalid_rays = invalid;
  }
  return RT_OK;
}

// rt_gather's own refusals (the rest are ray_color_check's).
int gather_check(rt_ctx* ctx, int32_t source, int32_t reserved) {
  if (source < RT_GATHER_RAY || source > RT_GATHER_SPHERE) return set_err(ctx, RT_ERR_INVALID, "gather source outside 0 .. 2");
  if (reserved != 0) return set_err(ctx, RT_ERR_INVALID, "rt_gather_params.reserved is not 0");
  return RT_OK;
}

// rt_gather_sh's own refusals (the rest are ray_color_check's).
int gather_sh_check(rt_ctx* ctx, int32_t bands, int32_t reserved) {
  if (bands < 1 || bands > RT_SH_MAX_BANDS) return set_err(ctx, RT_ERR_INVALID, "SH bands outside 1 .. 3");
  if (reserved != 0) return set_err(ctx, RT_ERR_INVALID, "rt_gather_sh_params.reserved is not 0");
  return RT_OK;
}

// rt_gather_surface's own refusals (the rest are ray_color_check's).
int gather_surface_check(rt_ctx* ctx, const int32_t (&reserved)[2]) {
  if (reserved[0] != 0 || reserved[1] != 0) return set_err(ctx, RT_ERR_INVALID, "rt_gather_surface_params.reserved is not 0");
  return RT_OK;
}

// source_ray's guard (ray_source.hip) for the host variant's count; fp32 in its order.
bool gather_point_valid(const rt_gather_point& q, int32_t source) {
  if (!(std::isfinite(q.p[0]) && std::isfinite(q.p[1]) && std::isfinite(q.p[2]))) return false;
  if (source == RT_GATHER_SPHERE) return true;
  if (!(std::isfinite(q.n[0]) && std::isfinite(q.n[1]) && std::isfinite(q.n[2]))) return false;
  const float xx = q.n[0] * q.n[0], yy = q.n[1] * q.n[1], zz = q.n[2] * q.n[2];
  const float l = sqrtf((xx + yy) + zz);
  return l != 0.0f && std::isfinite(l);
}

}  // namespace

extern "C" {

static_assert(sizeof(rt_ray) == 32 && sizeof(rt_ray_hit) == 32, "rt_ray / rt_ray_hit are two 16-B vectors each");

int rt_trace_rays(rt_ctx* ctx, const rt_ray* rays, int64_t n, float time, rt_ray_hit* hits) {
  if (int rc = query_check(ctx, rays, n, hits)) return rc;
  return query_host(ctx, false, rays, n, time, hits);
}

int rt_trace_rays_device(rt_ctx* ctx, const rt_ray* rays_dev, int64_t n, float time, rt_ray_hit* hits_dev, void* hip_stream) {
  if (int rc = query_check(ctx, rays_dev, n, hits_dev)) return rc;
  return query_async(ctx, false, rays_dev, n, time, hits_dev, hip_stream);
}

int rt_occluded(rt_ctx* ctx, const rt_ray* rays, int64_t n, float time, uint8_t* occluded) {
  if (int rc = query_check(ctx, rays, n, occluded)) return rc;
  return query_host(ctx, true, rays, n, time, occluded);
}

int rt_occluded_device(rt_ctx* ctx, const rt_ray* rays_dev, int64_t n, float time, uint8_t* occluded_dev, void* hip_stream) {
  if (int rc = query_check(ctx, rays_dev, n, occluded_dev)) return rc;
  return query_async(ctx, true, rays_dev, n, time, occluded_dev, hip_stream);
}

static_assert(sizeof(rt_path_ray) == 32, "rt_path_ray is two 16-B vectors");

int rt_ray_color(rt_ctx* ctx, const rt_path_ray* rays, int64_t n, const rt_ray_color_params* params, float* rgb,
                 rt_ray_color_stats* stats) {
  if (!ctx || !rays || !params || !rgb) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  DCamera dc{};
  int rc = ray_color_check(ctx, params, n, dc);
  if (rc) return rc;
  uint64_t invalid = 0;
  for (int64_t i = 0; i < n; ++i) {
    const rt_path_ray& r = rays[i];
    if (r.reserved != 0) return set_err(ctx, RT_ERR_INVALID, "a ray's reserved word is not 0");
    const bool fin = std::isfinite(r.o[0]) && std::isfinite(r.o[1]) && std::isfinite(r.o[2]) && std::isfinite(r.d[0]) &&
                     std::isfinite(r.d[1]) && std::isfinite(r.d[2]);
    invalid += !(fin && (r.d[0] != 0.0f || r.d[1] != 0.0f || r.d[2] != 0.0f));   // k_ray_source's guard
  }
  return ray_color_host(ctx, dc, SRC_CALLER, rays, n, params, rgb, stats, invalid);
}

int rt_ray_color_device(rt_ctx* ctx, const rt_path_ray* rays_dev, int64_t n, const rt_ray_color_params* params,
                        float* rgb_dev, void* hip_stream) {
  if (!ctx || !rays_dev || !params || !rgb_dev) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
  DCamera dc{};
  int rc = ray_color_check(ctx, params, n, dc);
  // an earlier call's device error surfaces here at the latest, as in rt_render_device
  if (rc || (rc = check_render_error(ctx, false)) || n == 0) return rc;
  return ray_color_device(ctx, dc, SRC_CALLER, rays_dev, n, params, rgb_dev, st);
}

// ---- rt_gather: rt_ray_color over directions ray_source.hip draws ----------

static_assert(sizeof(rt_gather_point) == sizeof(rt_path_ray) && sizeof(rt_gather_params) == 64, "rt_gather_point is rt_path_ray's layout");
static_assert(SRC_RAY == 1 + RT_GATHER_RAY && SRC_COSINE == 1 + RT_GATHER_COSINE && SRC_SPHERE == 1 + RT_GATHER_SPHERE,
              "ray_source.h's kinds follow rtgpu.h's sources");

int rt_gather(rt_ctx* ctx, const rt_gather_point* pts, int64_t n, const rt_gather_params* params, float* rgb,
              rt_ray_color_stats* stats) {
  if (!ctx || !pts || !params || !rgb) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = gather_check(ctx, params->source, params->reserved)) return rc;
  DCamera dc{};
  int rc = ray_color_check(ctx, &params->path, n, dc);
  if (rc) return rc;
  uint64_t invalid = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (pts[i].reserved != 0) return set_err(ctx, RT_ERR_INVALID, "a point's reserved word is not 0");
    invalid += !gather_point_valid(pts[i], params->source);
  }
  return ray_color_host(ctx, dc, 1 + params->source, pts, n, &params->path, rgb, stats, invalid);
}

int rt_gather_device(rt_ctx* ctx, const rt_gather_point* pts_dev, int64_t n, const rt_gather_params* params,
                     float* rgb_dev, void* hip_stream) {
  if (!ctx || !pts_dev || !params || !rgb_dev) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
  if (int rc = gather_check(ctx, params->source, params->reserved)) return rc;
  DCamera dc{};
  int rc = ray_color_check(ctx, &params->path, n, dc);
  if (rc || (rc = check_render_error(ctx, false)) || n == 0) return rc;
  return ray_color_device(ctx, dc, 1 + params->source, reinterpret_cast<const rt_path_ray*>(pts_dev), n, &params->path,
                          rgb_dev, st);
}

int rt_gather_rays(rt_ctx* ctx, const rt_gather_point* pts, int64_t n, int32_t source, uint32_t seed, int32_t sample,
                   rt_path_ray* out) {
  if (!ctx || !pts || !out) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = gather_check(ctx, source, 0)) return rc;
  if (n < 0 || n > kRayColorMaxRays) return set_err(ctx, RT_ERR_INVALID, "point count outside 0 .. 2^31 - 1");
  if (sample < 0) return set_err(ctx, RT_ERR_INVALID, "bad sample index");
  if (n == 0) return RT_OK;
  // the staging buffers of the host variants: the points in rc_rays, the rays in rc_rgb
  hipStream_t st = ctx->stream;
  const size_t bytes = size_t(n) * sizeof(rt_path_ray);
  int rc = ensure(ctx, ctx->rc_rays, bytes);
  if (rc || (rc = ensure(ctx, ctx->rc_rgb, bytes))) return rc;
  HIPCHK(hipMemcpyAsync(ctx->rc_rays.p, pts, bytes, hipMemcpyHostToDevice, st));
  HIPCHK(launch_gather_rays(static_cast<const float4*>(ctx->rc_rays.p), uint32_t(n), 1 + source, seed, uint32_t(sample),
                            static_cast<float4*>(ctx->rc_rgb.p), ctx->num_cus, st));
  HIPCHK(hipMemcpyAsync(out, ctx->rc_rgb.p, bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return RT_OK;
}

// ---- rt_gather_sh: rt_gather over the sphere, projected by k_sh_accum --------

static_assert(sizeof(rt_gather_sh_params) == sizeof(rt_gather_params) && RT_SH_MAX_BANDS == kShMaxBands,
              "rt_gather_sh_params is rt_gather_params' layout");

int rt_gather_sh(rt_ctx* ctx, const rt_gather_point* pts, int64_t n, const rt_gather_sh_params* params, float* sh,
                 rt_ray_color_stats* stats) {
  if (!ctx || !pts || !params || !sh) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = gather_sh_check(ctx, params->bands, params->reserved)) return rc;
  DCamera dc{};
  int rc = ray_color_check(ctx, &params->path, n, dc);
  if (rc) return rc;
  uint64_t invalid = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (pts[i].reserved != 0) return set_err(ctx, RT_ERR_INVALID, "a point's reserved word is not 0");
    invalid += !gather_point_valid(pts[i], RT_GATHER_SPHERE);
  }
  return ray_color_host(ctx, dc, SRC_SPHERE, pts, n, &params->path, sh, stats, invalid, params->bands);
}

int rt_gather_sh_device(rt_ctx* ctx, const rt_gather_point* pts_dev, int64_t n, const rt_gather_sh_params* params,
                        float* sh_dev, void* hip_stream) {
  if (!ctx || !pts_dev || !params || !sh_dev) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
  if (int rc = gather_sh_check(ctx, params->bands, params->reserved)) return rc;
  DCamera dc{};
  int rc = ray_color_check(ctx, &params->path, n, dc);
  if (rc || (rc = check_render_error(ctx, false)) || n == 0) return rc;
  return ray_color_device(ctx, dc, SRC_SPHERE, reinterpret_cast<const rt_path_ray*>(pts_dev), n, &params->path, sh_dev, st,
                          params->bands);
}

// ---- rt_gather_surface: the point is the path's first diffuse vertex ----------
// (k_gather_source<SRC_SURFACE>, then run_batches' surface mode)

static_assert(sizeof(rt_gather_surface_params) == sizeof(rt_gather_params) &&
                  offsetof(rt_gather_surface_params, reserved) == offsetof(rt_gather_params, source),
              "rt_gather_surface_params is rt_gather_params' layout");

int rt_gather_surface(rt_ctx* ctx, const rt_gather_point* pts, int64_t n, const rt_gather_surface_params* params,
                      float* rgb, rt_ray_color_stats* stats) {
  if (!ctx || !pts || !params || !rgb) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = gather_surface_check(ctx, params->reserved)) return rc;
  DCamera dc{};
  int rc = ray_color_check(ctx, &params->path, n, dc);
  if (rc) return rc;
  uint64_t invalid = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (pts[i].reserved != 0) return set_err(ctx, RT_ERR_INVALID, "a point's reserved word is not 0");
    invalid += !gather_point_valid(pts[i], RT_GATHER_COSINE);
  }
  return ray_color_host(ctx, dc, SRC_SURFACE, pts, n, &params->path, rgb, stats, invalid);
}

int rt_gather_surface_device(rt_ctx* ctx, const rt_gather_point* pts_dev, int64_t n,
                             const rt_gather_surface_params* params, float* rgb_dev, void* hip_stream) {
  if (!ctx || !pts_dev || !params || !rgb_dev) return RT_ERR_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->stream;
  if (int rc = gather_surface_check(ctx, params->reserved)) return rc;
  DCamera dc{};
  int rc = ray_color_check(ctx, &params->path, n, dc);
  if (rc || (rc = check_render_error(ctx, false)) || n == 0) return rc;
  return ray_color_device(ctx, dc, SRC_SURFACE, reinterpret_cast<const rt_path_ray*>(pts_dev), n, &params->path, rgb_dev,
                          st);
}

}  // extern "C"
