/*
 * rtgpu.h — C-ABI drop-in boundary of the MI355X (gfx950) path tracer.
 *
 * The hot path it replaces is the per-pixel samples x bounces loop of
 * byvfx/go-raytracing:
 *   rt.BucketRenderer.renderBucketWithQuality   rt/bucket_renderer.go:257-301
 *   rt.Camera.GetRay                            rt/camera.go:368-435
 *   rt.Camera.RayColor / rayColorInternal       rt/camera.go:438-518
 *   rt.Camera.sampleLightMIS/AreaLight/HDRI     rt/camera.go:538-678
 * and everything those call (Hittable.Hit, Material.Scatter/Emitted/PDF,
 * Texture.Value, HDRIEnvironment.Sample/SampleDirection/PDF).
 *
 * The Go host keeps building scenes with its own builders (scenes.go) and
 * hands the object graph across this boundary once per render, flattened by
 * a type switch over the concrete Go types (see INTEGRATION.md for the cgo
 * binding and the in-package flattener).  The graph is copied before
 * rt_scene_upload returns; C never retains caller memory.
 *
 * Every entry point sets the HIP device of its context itself (cgo calls may
 * land on any OS thread).  Errors are int status codes (RT_OK == 0) plus a
 * per-context message from rt_last_error(); no C++ exception crosses.
 *
 * Plain C types only: no torch, no HIP types in the signatures (the stream
 * argument of the *_device entry points is an opaque hipStream_t).
 */
#ifndef RTGPU_H
#define RTGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 8

/* ---- status codes ------------------------------------------------------ */
enum rt_status {
  RT_OK = 0,
  RT_ERR_INVALID = -1,     /* bad argument / malformed scene graph          */
  RT_ERR_UNSUPPORTED = -2, /* Go type or nesting the GPU path does not take;
                              the caller falls back to rt.BucketRenderer.
                              Includes a BVH whose worst traversal needs more
                              than 128 stack entries; a scene holding a
                              RotateX / RotateZ wrapper traverses in the
                              reference's DFS order with two words per entry
                              (DESIGN.md §3), so its limit is 64 entries    */
  RT_ERR_HIP = -3,         /* HIP runtime error (message in rt_last_error)  */
  RT_ERR_OOM = -4,         /* device allocation failed                      */
  RT_ERR_NO_SCENE = -5,    /* rt_render before rt_scene_upload              */
  RT_ERR_DEVICE = -6       /* kernel-side failure (e.g. traversal stack)    */
};

/* ---- scene graph: one node per concrete rt.Hittable ------------------------
 * Mirrors rt.Hittable (hittable.go:15-18).  `bbox` is the Go object's
 * BoundingBox() as {xmin,xmax,ymin,ymax,zmin,zmax}; `p` holds the Go struct
 * fields (float64) listed per kind.                                          */
enum rt_hittable_kind {
  RT_SPHERE = 1,      /* sphere.go:6-11   p[0..2]=Center.orig p[3..5]=Center.dir
                                          (velocity) p[6]=Radius                */
  RT_QUAD = 2,        /* quad.go:5-14     p[0..2]=Q p[3..5]=u p[6..8]=v
                                          p[9..11]=w p[12..14]=normal p[15]=D   */
  RT_TRIANGLE = 3,    /* triangle.go:8-14 p[0..2]=v0 p[3..5]=v1 p[6..8]=v2
                                          p[9..11]=normal (unit)               */
  RT_PLANE = 4,       /* plane.go:5-10    p[0..2]=Point p[3..5]=Normal (unit)  */
  RT_LIST = 5,        /* hittable_list.go:3-6  children[a .. a+b)              */
  RT_BVH_NODE = 6,    /* bvh.go:13-17     a=left b=right (a==b for the leaf
                                          wrapper BVHNode{leaf,leaf}, bvh.go:141) */
  RT_BVH_LEAF = 7,    /* bvh.go:21-24     children[a .. a+b)                   */
  RT_TRANSLATE = 8,   /* transform.go:78-82   a=Obj p[0..2]=Offset             */
  RT_ROTATE_X = 9,    /* transform.go:194-199 a=Obj p[0]=SinTheta p[1]=CosTheta */
  RT_ROTATE_Y = 10,   /* transform.go:113-118 a=Obj p[0]=SinTheta p[1]=CosTheta */
  RT_ROTATE_Z = 11,   /* transform.go:275-280 a=Obj p[0]=SinTheta p[1]=CosTheta */
  RT_SCALE = 12,      /* transform.go:360-365 a=Obj p[0..2]=Factor p[3..5]=InvFactor */
  RT_VOLUME = 13,     /* volume.go:9-13   a=boundary p[0]=negInvDensity
                                          material=phaseFunction (Isotropic)   */
  RT_CIRCLE = 14      /* circle.go:5-12   p[0..2]=center p[3..5]=normal (unit)
                                          p[6]=radius p[7]=D                   */
};

typedef struct rt_hittable {
  int32_t kind;     /* enum rt_hittable_kind                                 */
  int32_t material; /* index into rt_scene_desc.materials (prims, volume)    */
  int32_t a;        /* child / left / first (see kinds)                      */
  int32_t b;        /* right / count (see kinds)                             */
  double bbox[6];   /* BoundingBox(): xmin,xmax,ymin,ymax,zmin,zmax          */
  double p[16];     /* kind-specific float64 fields                          */
} rt_hittable;

/* ---- materials (material.go:9-288) and textures (texture.go:5-77) -------- */
enum rt_material_kind {
  RT_LAMBERTIAN = 1,    /* material.go:33-80   texture                        */
  RT_METAL = 2,         /* material.go:86-140  albedo, fuzz (already clamped ≤1) */
  RT_DIELECTRIC = 3,    /* material.go:146-196 refraction_index               */
  RT_DIFFUSE_LIGHT = 4, /* material.go:202-236 texture                        */
  RT_ISOTROPIC = 5      /* material.go:243-278 texture                        */
};

typedef struct rt_material {
  int32_t kind;
  int32_t texture;  /* index into textures (Lambertian/DiffuseLight/Isotropic) */
  double albedo[3]; /* Metal.Albedo                                           */
  double fuzz;      /* Metal.Fuzz                                             */
  double refraction_index; /* Dielectric.RefractionIndex                     */
} rt_material;

enum rt_texture_kind {
  RT_TEX_SOLID = 1,   /* SolidColor, texture.go:9-11,43-45                   */
  RT_TEX_CHECKER = 2, /* CheckerTexture, texture.go:13-17,47-77              */
  RT_TEX_NOISE = 3,   /* NoiseTexture, texture.go:19-28,81-85 (Perlin turb)  */
  RT_TEX_IMAGE = 4    /* ImageTexture, image_texture.go:5-41                 */
};

typedef struct rt_texture {
  int32_t kind;
  int32_t even, odd; /* checker: texture indices (must be RT_TEX_SOLID)      */
  double albedo[3];  /* solid colour                                         */
  double inv_scale;  /* checker invScale                                     */
  double scale;      /* noise: NoiseTexture.scale                            */
  int32_t perlin;    /* noise: index into rt_scene_desc.perlins              */
  int32_t image;     /* image: index into rt_scene_desc.images               */
} rt_texture;

/* ImageLoader (image_loader.go:17-24) as the Go loader leaves it: linear
 * float64 rgb after LinearToGamma (image_loader.go:70-76), row-major.       */
typedef struct rt_image {
  int32_t width, height;
  const double* rgb;       /* width*height*3                                */
} rt_image;

/* Perlin (noise.go:8-13): the generator's tables (NewPerlin draws them from
 * math/rand, so the caller passes them).                                   */
typedef struct rt_perlin {
  double randvec[256][3];
  int32_t perm_x[256], perm_y[256], perm_z[256];
} rt_perlin;

/* ---- HDRI environment (hdri.go:13-26, image_loader.go:17-24) ------------- */
typedef struct rt_environment {
  int32_t width, height;          /* ImageLoader dims                         */
  const double* rgb;              /* ImageLoader.data, width*height*3 float64 */
  double rotation;                /* radians (HDRIEnvironment.rotation)       */
  int32_t use_importance_sampling;/* HDRIEnvironment.useImportanceSampling    */
} rt_environment;

typedef struct rt_scene_desc {
  const rt_hittable* hittables;
  int32_t num_hittables;
  const int32_t* children;   /* child index table for RT_LIST / RT_BVH_LEAF   */
  int32_t num_children;
  int32_t root;              /* the world passed to NewBucketRenderer         */
  const rt_material* materials;
  int32_t num_materials;
  const rt_texture* textures;
  int32_t num_textures;
  const int32_t* lights;     /* Camera.Lights (camera.go:38), hittable indices */
  int32_t num_lights;
  const rt_environment* environment; /* Camera.Environment or NULL (camera.go:39) */
  const rt_image* images;    /* ImageTexture images                          */
  int32_t num_images;
  const rt_perlin* perlins;  /* NoiseTexture generators                      */
  int32_t num_perlins;
} rt_scene_desc;

/* ---- camera: the state Camera.Initialize() leaves (camera.go:286-344) ---- */
typedef struct rt_camera_desc {
  int32_t image_width, image_height;
  int32_t samples_per_pixel; /* Camera.SamplesPerPixel                       */
  int32_t max_depth;         /* Camera.MaxDepth (PhantomHDRI primary test)   */
  double center[3];          /* c.center                                     */
  double pixel00[3];         /* c.pixel00Loc                                 */
  double pixel_delta_u[3];
  double pixel_delta_v[3];
  double defocus_angle;      /* c.DefocusAngle (>0 enables the disk)         */
  double defocus_disk_u[3];
  double defocus_disk_v[3];
  double background[3];      /* c.Background                                 */
  int32_t use_sky_gradient;  /* c.UseSkyGradient                             */
  int32_t phantom_hdri;      /* c.PhantomHDRI                                */
  int32_t camera_motion;     /* c.CameraMotion                               */
  int32_t free_camera;       /* c.FreeCamera                                 */
  /* GetRay's slow path (camera.go:390-434), read only when camera_motion or
   * free_camera is set: the basis is rebuilt per sample at rayTime.       */
  double center_motion_orig[3];  /* c.centerMotion.orig (LookFrom)          */
  double center_motion_dir[3];   /* c.centerMotion.dir (LookFrom2-LookFrom or 0) */
  double look_at_motion_orig[3]; /* c.lookAtMotion.orig (LookAt)            */
  double look_at_motion_dir[3];  /* c.lookAtMotion.dir (LookAt2-LookAt or 0) */
  double vup[3];             /* c.Vup                                        */
  double forward[3];         /* c.Forward (free camera: w = -Forward)        */
  double viewport_width;     /* c.viewportWidth  (camera.go:311)             */
  double viewport_height;    /* c.viewportHeight (camera.go:310)             */
  double focus_dist;         /* c.FocusDist                                  */
  double defocus_radius;     /* FocusDist*tan(DefocusAngle/2) (camera.go:356) */
} rt_camera_desc;

/* ---- render call ----------------------------------------------------------- */
typedef struct rt_bucket { int32_t x, y, width, height; } rt_bucket; /* bucket_renderer.go:22-27 */

typedef struct rt_render_params {
  int32_t samples_per_pixel; /* samplesForPass (bucket_renderer.go:175-191)  */
  int32_t max_depth;         /* depthForPass                                 */
  int32_t sample_offset;     /* first global sample index (RNG key)          */
  uint32_t seed;             /* RNG seed (counter-based)      */
  const rt_bucket* buckets;  /* NULL: the whole image                        */
  int32_t num_buckets;
  int32_t accumulate;        /* 1: add into accum; 0: overwrite bucket pixels */
} rt_render_params;

typedef struct rt_stats {
  double kernel_ms;          /* device time of the render kernels            */
  uint64_t samples;          /* pixels x samples rendered                    */
} rt_stats;

/* Per-sample traversal work counted by the instrumented kernel variant
 * (feeds the algorithmic-bytes roofline).           */
typedef struct rt_work_counts {
  uint64_t samples;
  uint64_t rays;             /* closest-hit rays (camera + scattered)        */
  uint64_t shadow_rays;
  uint64_t node_visits;      /* BVH2 node fetches (two child boxes each)     */
  uint64_t sphere_tests, quad_tests, tri_tests, plane_tests;
  uint64_t instance_visits, volume_tests;
  uint64_t material_fetches, env_lookups;
  uint64_t instance_box_tests; /* world-space instance culling boxes (32 B)  */
  uint64_t stack_spills;       /* traversal-stack pushes past the LDS ring (to the global spill area) */
  uint64_t early_shadow_rays;  /* NEE rays the shade kernel resolved itself (RT_OPT_EARLY_MISS): they
                                  missed the world box and never reached the shadow kernel */
  uint64_t early_rays;         /* scattered rays it kept out of the closest-hit kernel's queue likewise */
} rt_work_counts;

/* Summed per-launch durations of the wavefront kernels of the last render
 * (HIP events on the launch's stream; rt_set_kernel_timing(ctx, 1) first).
 * With twin streams (twins > 1, RT_OPT_STREAMS) the twins' launches of one
 * kernel and bounce run concurrently on disjoint parts of the pixels: they
 * count as one launch whose duration is the union of their intervals, so a
 * launch always covers the whole render's work.                           */
typedef struct rt_kernel_times {
  double extend_ms, shade_ms, shadow_ms;
  int32_t extend_launches, shade_launches, shadow_launches, twins;
} rt_kernel_times;

/* Sizes of the flattened device scene (rt_scene_get_info). */
typedef struct rt_scene_info {
  int32_t nodes, leaves, refs, spheres, quads, triangles, planes;
  int32_t instances, blases, volumes, materials, textures, lights;
  int32_t stack_needed, tlas_depth, blas_depth;
  int64_t device_bytes;
  int32_t node_format;  /* the RT_NODES_* format the traversal kernels read
                           (RT_OPT_NODE_FORMAT, or RT_NODES_FP32 when the
                           scene does not take the one asked for)          */
  int32_t nodes8;       /* RT_NODES_WIDE8: 8-wide nodes (else 0)           */
} rt_scene_info;

typedef struct rt_ctx rt_ctx;

int rt_abi_version(void);

/* NewBucketRenderer analogue: one context per device. */
int rt_ctx_create(int device, rt_ctx** out);
void rt_ctx_destroy(rt_ctx* ctx);
const char* rt_last_error(const rt_ctx* ctx);

/* Visible HIP devices (what the Go side passes as the device list, the way
 * main.go:84 sizes the worker pool with runtime.NumCPU()).                 */
int rt_device_count(int32_t* num_devices);

/* One context over several devices (bucket_renderer.go:193-213's worker
 * pool with one GPU per worker).  devices[0] is the primary: the frame of
 * rt_render_device must live there, and rt_render stages through it.
 * rt_scene_upload flattens and uploads on every device concurrently;
 * rt_render / rt_render_device deal the buckets round-robin over the devices
 * (bucket k -> device k mod n) and render every share at once, one host
 * thread per device; each device writes its own pixels straight into the
 * primary's frame (peer access over xGMI), so the frame is bit-identical to a
 * one-device render.  rt_render_device stays asynchronous on the caller's
 * stream.  rt_ctx_set_option / rt_sync / rt_last_render_kernel_ms (the
 * slowest device) cover every device; the probes, counters, per-launch
 * timing and tonemap run on the primary only.  A device list may repeat a
 * device.  RT_ERR_UNSUPPORTED: a device without peer access to devices[0]. */
int rt_ctx_create_multi(const int32_t* devices, int32_t num_devices, rt_ctx** out);
int rt_ctx_num_devices(const rt_ctx* ctx);
/* The last multi-device render's split: per device (in the context's device
 * order, up to max_devices) the tiles it rendered and the runs it claimed
 * (static dealing: one run per device with tiles).                         */
int rt_last_dealing(const rt_ctx* ctx, int32_t* tiles, int32_t* runs, int32_t max_devices);

/* Context options (take effect at the next rt_scene_upload).
 *   RT_OPT_BLAS_BUILDER: how an all-triangle mesh BVH (LoadOBJ ->
 *     NewBVHNode, obj_loader.go:109) is laid out on the device:
 *     RT_BLAS_REFERENCE = the caller's topology node for node;
 *     RT_BLAS_SAH (default) = binned-SAH BVH over the same triangles;
 *     RT_BLAS_DEVICE = LBVH built on the GPU during rt_scene_upload
 *     (Morton sort + Karras hierarchy + refit + BVH4 collapse, build.hip).
 *     All give the same closest hit: the tie rule uses the reference's
 *     DFS ranks, not the device visiting order.
 *   RT_OPT_TLAS_BUILDER: the world BVH (main.go:77 NewBVHNodeFromList):
 *     RT_BLAS_REFERENCE = the caller's topology; RT_BLAS_SAH (default) =
 *     SAH over the same top-level objects, one per leaf, each keeping its
 *     DFS rank and its leaf's test count (volumes).  Scenes holding a
 *     RotateX/RotateZ wrapper always keep the caller's topology.
 *   RT_OPT_NODE_FORMAT: the BVH4 node records the traversal reads:
 *     RT_NODES_FP32 (default) = 128-B nodes, fp32 child boxes rounded
 *     outward from the fp64 boxes; RT_NODES_QUANT8 = 64-B nodes, child
 *     planes as 8-bit steps of a per-node frame, widened by a margin of
 *     2^-17 of the node's largest |coordinate| (half the node bytes, looser
 *     boxes).  The margin covers the slab test's fp32 rounding for ray
 *     origins up to ~20 node magnitudes from the node (tests/quant_probe.cpp);
 *     a ray from farther away (a node near its space's origin seen from
 *     hundreds of magnitudes off) can lose a box at the last ulp, so the
 *     closest hits equal the fp32 format's only within that envelope (every
 *     BASELINE scene is inside it).  Scenes holding a RotateX/RotateZ wrapper
 *     always use RT_NODES_FP32 (their node boxes decide which rays reach
 *     an object, transform.go:201-351).  RT_NODES_WIDE8 = 8-wide nodes of
 *     128 B (one cache line: eight children's 8-bit planes in one frame per
 *     node, the RT_NODES_QUANT8 quantiser with bf16 steps, children visited
 *     in octant order), collapsed from the same SAH BVH2 with the same
 *     SAH-optimal cut; fewer, wider node steps per ray.  Taken by scenes
 *     without RotateX/RotateZ, circles or volumes left in the world BVH and
 *     whose BLASes are host-built (not RT_BLAS_DEVICE); others keep
 *     RT_NODES_FP32.  Hits equal the fp32 format's within the same envelope.
 *     Scale and ray distance, every format and both world-BVH builders: a
 *     box whose slab interval collapses in fp32 (a flat primitive's 2e-4
 *     box seen from >= 2048 units away, or lying at a coordinate >= 2048) is
 *     kept, not culled (tmax >= tmin).  Pinned by
 *     tests/test_scale_host.py and tests/test_gpu_scale.py: first hits equal
 *     the float64 reference arithmetic's for scenes 8 to 524,288 units across,
 *     up to 16 scene sizes from the origin, with ray origins up to 64 scene
 *     sizes outside the scene and axis-parallel rays.  An area light's
 *     shadow ray ends at min(dist - 0.001, dist * (1 - 2^-20)): the reference's
 *     dist - 0.001 (camera.go:639) where fp32 resolves it (unchanged below
 *     dist = 1048), and still short of the light where it does not.  Radiance
 *     at scene coordinates beyond about 8192 keeps a bias of a few percent
 *     against float64: the ray offset 0.001 at a ray's start is then below
 *     half an ulp of the hit point.
 *   RT_OPT_VOLUMES: RT_VOLUMES_LIFTED (default) = Volume objects are kept
 *     out of the world BVH and tested by the shading kernel on every path
 *     ray and NEE shadow ray (same results: the volume test runs over the
 *     ray's whole interval and competes by the tie rule); RT_VOLUMES_IN_BVH
 *     = tested inside the traversal.  Scenes with a Circle or a Noise /
 *     Image texture always keep them in the BVH.
 *   RT_OPT_LIFT_PRIMS: RT_PRIMS_LIFTED (default) = the world-level quads
 *     and spheres (room walls, lights: top-level objects, not those inside
 *     an instance) are kept out of the world BVH and tested by the shading
 *     kernel on every path ray and NEE shadow ray, so rays that enter no
 *     instance leave the traversal kernels at once.  Same results: each
 *     test is confirmed by the fp32 box the traversal would have tested
 *     before it and competes by the tie rule.  (With RT_NODES_QUANT8 /
 *     RT_NODES_WIDE8 the traversal tests a slightly wider box than that
 *     one, so a ray within a few ulps of a primitive's rim can hit it
 *     inside the traversal and miss it lifted, where it decides as with
 *     RT_NODES_FP32 and as the reference; frames of the two placements are
 *     equal with fp32 nodes, and with the quantised formats unless such a
 *     ray occurs.)  All or none are lifted, only when every one of these
 *     holds: there are at most 8; the scene holds no RotateX / RotateZ;
 *     another object (an instance, say) stays in the world BVH; the scene
 *     has no Noise / Image texture and no lifted volume; and its material,
 *     texture and light tables have at most 384 / 384 / 16 entries (the
 *     shading kernel's tables in LDS).  Otherwise, and with
 *     RT_PRIMS_IN_BVH, the traversal tests them.  rt_scene_lifted_prims
 *     reports how many the uploaded scene lifted.
 *   RT_OPT_BVH4_COLLAPSE: how the binary BVHs become the 4-wide nodes the
 *     device traverses: RT_COLLAPSE_SAH (default) = the cut of each subtree
 *     into at most four child items with the least total node surface area
 *     (a dynamic programme); RT_COLLAPSE_GREEDY = open the largest-area
 *     internal child until four items are held.  Same hits either way.   */
/* Schedule options (take effect at the next render; 0 = automatic).  They
 * change how the work is dealt to the GPU, never the image: the closest hit
 * is independent of the traversal schedule.
 *   RT_OPT_BATCH_SLOTS: path slots per batch (default: from 85 % of the
 *     free HBM, at most 2^30, halved until the allocation succeeds).
 *   RT_OPT_REFILL: idle lanes of a wave (1..64) before it claims a new run
 *     of rays (default 16).
 *   RT_OPT_MAX_BLOCKS: cap on the persistent traversal grids (workgroups).
 *   RT_OPT_STREAMS: 1..4: the bucket tiles are dealt to that many parts
 *     ("twins"), each rendered on its own HIP stream, so one part's kernel
 *     tails overlap the others' kernels; 1 keeps one stream.  Default: 3
 *     for renders of more than 2^26 samples (pixels x spp), else 2; scenes
 *     whose shading tests lifted volumes (RT_VOLUMES_LIFTED with a Volume
 *     in the scene) always render on 1 (the shading kernel is the long one
 *     there, and more parts only add launch overlap it cannot use).
 *   RT_OPT_DEALING (multi-device contexts): how a render deals its 16x16
 *     tiles to the devices.  RT_DEAL_STATIC (default) = tile k to device
 *     k mod n, every share rendered at once, asynchronously.
 *     RT_DEAL_DYNAMIC = the reference's worker pool fed by a channel
 *     (bucket_renderer.go:193-213): each device's host thread claims runs of
 *     consecutive tiles from one shared counter and renders each run, then
 *     claims the next, until none are left; a run is a share of the tiles
 *     left (guided self-scheduling), so a slower or later device takes
 *     fewer.  The first run is RT_OPT_DEAL_FIRST percent (1..100, default
 *     50) of a device's fair share; no run is smaller than 1/16 of one.
 *     rt_render_device then returns once every run has been rendered (the
 *     claims follow the devices' progress); the frame is bit-identical to
 *     the static split's and to one device's.  rt_last_dealing reports the
 *     split.
 *   RT_OPT_TAIL: the long tail of deep renders without lights (MaxDepth >
 *     8; RandomScene, HDRITestScene): once at most a threshold of paths is
 *     left, one persistent launch carries each of them through all its
 *     remaining bounces (closest hit and shading in one lane) instead of
 *     two launches per bounce.  Same operations per path in the same order:
 *     the frame is bit-identical.  0 (default) = automatic (2^23 paths,
 *     wavefront.h kTailRaysDefault), 1 = off (every bounce through the
 *     per-bounce kernels), n > 1 = threshold of n paths.
 *   RT_OPT_OVERLAP: in scenes with lights, bounce b's shadow rays
 *     (k_shadow) and their NEE adds (k_nee_apply) run on a second stream
 *     per part while bounce b + 1's closest-hit kernel (k_extend) runs, its
 *     only input being bounce b's scattered rays (the reference's worker
 *     carries one sample through every bounce, bucket_renderer.go:257-301,
 *     camera.go:443-518).  Same operations per path in the same order: the
 *     frame is bit-identical.  0 (default) = automatic (off: measured
 *     slower on CornellBoxLucy), 1 = off, 2 = on (at most two
 *     parts unless RT_OPT_STREAMS says otherwise).
 *   RT_OPT_EARLY_MISS: rays that miss the box of the world BVH are
 *     resolved by the shade kernel that makes them, since the traversal
 *     would end each at its first test.  An NEE job whose shadow rays all
 *     miss it ("visible") is applied there instead of being queued for
 *     k_shadow and k_nee_apply; a path whose scattered ray misses it is kept
 *     at the back of the next stream, which k_extend does not read, and is
 *     shaded at the next bounce as the miss it is.  The test is the
 *     traversal's own, on the values it would read back, and the adds are
 *     the same in the same order: the frame is bit-identical.  Only in
 *     scenes without planes (they are tested before the box) and never in
 *     the path probes' renders; the scattered rays' part is off in renders
 *     that may use the long-tail kernel (RT_OPT_TAIL).
 *     0 (default) = automatic (on where it applies), 1 = off, 2 = on.      */
enum { RT_OPT_BLAS_BUILDER = 1, RT_OPT_TLAS_BUILDER = 2, RT_OPT_NODE_FORMAT = 3,
       RT_OPT_BATCH_SLOTS = 4, RT_OPT_REFILL = 5, RT_OPT_MAX_BLOCKS = 6, RT_OPT_STREAMS = 7,
       RT_OPT_VOLUMES = 8, RT_OPT_BVH4_COLLAPSE = 9, RT_OPT_DEALING = 10, RT_OPT_DEAL_FIRST = 11,
       RT_OPT_TAIL = 12, RT_OPT_OVERLAP = 13, RT_OPT_LIFT_PRIMS = 14,
       RT_OPT_EARLY_MISS = 15 };
enum { RT_PRIMS_LIFTED = 0, RT_PRIMS_IN_BVH = 1 };
enum { RT_DEAL_STATIC = 0, RT_DEAL_DYNAMIC = 1 };
enum { RT_BLAS_REFERENCE = 0, RT_BLAS_SAH = 1, RT_BLAS_DEVICE = 2 };
enum { RT_NODES_FP32 = 0, RT_NODES_QUANT8 = 1, RT_NODES_WIDE8 = 2 };
enum { RT_VOLUMES_LIFTED = 0, RT_VOLUMES_IN_BVH = 1 };
enum { RT_COLLAPSE_SAH = 0, RT_COLLAPSE_GREEDY = 1 };
int rt_ctx_set_option(rt_ctx* ctx, int32_t key, int32_t value);

/* Flatten + upload the Go object graph (copied; caller memory not retained). */
int rt_scene_upload(rt_ctx* ctx, const rt_scene_desc* scene);

int rt_scene_get_info(const rt_ctx* ctx, rt_scene_info* out);

/* World quads / spheres the uploaded scene keeps out of its world BVH
 * (RT_OPT_LIFT_PRIMS; 0 = none lifted). */
int rt_scene_lifted_prims(const rt_ctx* ctx, int32_t* count);

/* Wall time (ms) of the device BVH builds (RT_BLAS_DEVICE) of the last
 * rt_scene_upload on this context; 0 when every BLAS was built on the host. */
int rt_last_build_ms(const rt_ctx* ctx, double* ms);

/* Render the buckets into a caller-owned host buffer of width*height*3 float
 * (sum of per-sample radiance, linear).  Blocks until done.               */
int rt_render(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
              float* accum_rgb, rt_stats* stats);

/* Same, into a device buffer (width*height*3 float) on `hip_stream`;
 * asynchronous.  Used by the multi-GPU driver (tile shard + RCCL combine).
 * A device-side error of a render (RT_ERR_DEVICE: traversal stack overflow,
 * the frame is wrong) is reported by the first of: the next rt_render_device
 * call once that render has finished, rt_sync, rt_last_render_kernel_ms.   */
int rt_render_device(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                     float* accum_rgb_device, void* hip_stream);

/* Blocks until every render enqueued on this context has finished and
 * reports any device-side error of them (RT_ERR_DEVICE), as the Go
 * renderer's pass completion (bucket_renderer.go:212-213, wg.Wait) would.  */
int rt_sync(rt_ctx* ctx);

/* Device time (ms) of the render kernel of the most recent render call on
 * this context (hipEvents recorded on that call's stream around the render
 * kernel only); blocks until that kernel has finished and reports a device
 * error of the renders so far (RT_ERR_DEVICE).                             */
int rt_last_render_kernel_ms(rt_ctx* ctx, double* ms);

/* Instrumented run of the same kernel: traversal/prim counters. */
int rt_count_work(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                  rt_work_counts* out);

/* Same instrumented run, counters split by kernel: out[0] = extend
 * (closest-hit traversal, camera rays), out[1] = shade (materials, NEE
 * set-up, HDRI lookups; there `rays` counts the paths shaded,
 * `shadow_rays` the NEE jobs written, `early_shadow_rays` the NEE rays it
 * resolved without a job and `early_rays` the next rays it kept out of the
 * extend kernel's queue, RT_OPT_EARLY_MISS), out[2] = shadow (any-hit traversal).
 * rt_count_work's `rays` / `shadow_rays` are the extend and shadow ones.   */
int rt_count_work_by_kernel(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                            rt_work_counts out[3]);

/* Per-launch kernel timing of subsequent renders (off by default; one HIP
 * event before every extend/shade/shadow launch and after every shadow).   */
int rt_set_kernel_timing(rt_ctx* ctx, int enable);
/* The measured HBM read peak for the roofline ("plus a
 * measured stream-read kernel peak on the box"): `reps` passes of a
 * coalesced 16-B-per-lane read over a fresh device buffer of `bytes`
 * (>= 1 MiB; larger than the 256-MB Infinity Cache to measure HBM), timed
 * with HIP events on the context's stream, in GB/s.  Blocks.              */
int rt_measure_read_bandwidth(rt_ctx* ctx, uint64_t bytes, int32_t reps, double* gbs);
int rt_last_kernel_times(rt_ctx* ctx, rt_kernel_times* out);

/* RGBA8 quantisation of an accumulated sum (bucket_renderer.go:276-285):
 * c*(1/spp) -> LinearToGamma (utils.go:85-90) -> clamp [0,0.999] ->
 * uint8(256*x).  Host buffers; computed on the device.                    */
int rt_tonemap_rgba8(rt_ctx* ctx, const float* accum_rgb, int32_t width, int32_t height,
                     int32_t samples_per_pixel, uint8_t* rgba_out);

/* One progressive pass as the drop-in needs it (renderBucketWithQuality,
 * bucket_renderer.go:257-301): render the buckets into the context's own
 * device-resident frame sums (overwrite, or add with params->accumulate),
 * quantise the rendered buckets' pixels on the device (:276-285) into its
 * RGBA8 framebuffer, and copy that framebuffer (width*height*4 bytes) to
 * rgba_out.  Pixels outside the buckets keep their previous RGBA8 value.
 * Only the 4 B/px framebuffer crosses PCIe (rt_render + rt_tonemap_rgba8
 * move 28 B/px).  A new image size starts from zero.  Blocks.
 * The quantisation divides by the samples the sums hold: samples_per_pixel
 * for an overwriting pass; with accumulate, sample_offset +
 * samples_per_pixel (an accumulating pass continues the earlier passes'
 * samples, so its sample_offset counts them).
 * stats->kernel_ms is the call's wall time.                               */
int rt_render_rgba8(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                    uint8_t* rgba_out, rt_stats* stats);
/* The frame sums behind rt_render_rgba8's framebuffer (width*height*3
 * floats), e.g. for SaveImage-side checks.                                 */
int rt_read_frame_sums(rt_ctx* ctx, float* accum_out, int64_t num_floats);

/* Parity probe: first-bounce closest hit of sample `sample` for every pixel.
 * out_top = hittable index of the top-level object (child of the world BVH
 * leaf), out_prim = hittable index of the primitive (== top for
 * non-instanced objects), -1 on miss; out_t = hit distance.               */
int rt_primary_hits(rt_ctx* ctx, const rt_camera_desc* cam, uint32_t seed, int32_t sample,
                    int32_t* out_top, int32_t* out_prim, float* out_t);

/* The same ids from the production pipeline: the hit records the render's
 * first-bounce closest-hit kernel (k_extend, persistent, with the context's
 * schedule options) writes for sample `sample` of every pixel
 * (= rt_extend_hits at bounce 0).                                         */
int rt_extend_first_hits(rt_ctx* ctx, const rt_camera_desc* cam, uint32_t seed, int32_t sample,
                         int32_t* out_top, int32_t* out_prim, float* out_t);

/* Path probes past the camera ray: world.Hit of every bounce (camera.go:449
 * in rayColorInternal's recursion) and the NEE shadow rays (camera.go:582,
 * :639), read back from the production pipeline.  Sample `sample` of every
 * pixel is rendered to depth bounce + 1 (the rays of bounce k do not depend
 * on the depth past it), so the records of bounce `bounce` are the last the
 * pipeline wrote.
 * rt_extend_hits: the closest hit of the path's bounce-`bounce` ray, ids as
 * rt_primary_hits (-1 miss; -2 and t = -1: the path ended before this
 * bounce), lifted volumes included; out_ray (may be NULL): the incoming ray,
 * origin xyz and direction xyz (6 floats per pixel, 0 for ended paths).
 * rt_shadow_visibility: per pixel, bit 0 / 1 = the area-light / HDRI shadow
 * ray the bounce traced (a lifted volume that occludes a ray is resolved in
 * shading and leaves its bit clear), bit 2 / 3 = that ray was unoccluded.  */
int rt_extend_hits(rt_ctx* ctx, const rt_camera_desc* cam, uint32_t seed, int32_t sample, int32_t bounce,
                   int32_t* out_top, int32_t* out_prim, float* out_t, float* out_ray);
int rt_shadow_visibility(rt_ctx* ctx, const rt_camera_desc* cam, uint32_t seed, int32_t sample, int32_t bounce,
                         int32_t* out_nee);

/* Feature buffers: per pixel 8 floats, albedo.rgb, normal.xyz, depth,
 * coverage, each summed over the call's samples (the caller divides by the
 * sample count, as for rt_render).  Sample s of a pixel uses the path key of
 * rt_render's sample s (seed, sample_offset + s), so the features belong to
 * the camera rays the frame traced; they are taken at that ray's closest hit
 * as the integrator sees it (the production closest-hit kernel, lifted
 * volumes included).  max_depth is ignored.  Per sample:
 *   Lambertian / Isotropic: coverage 1, albedo = the texture's value at the
 *     hit; Metal: its Albedo; Dielectric: (1,1,1);
 *   normal = HitRecord.Normal (face-forwarded; (1,0,0) for a Volume,
 *     volume.go:72-76), depth = the hit's ray parameter t (direction not
 *     normalised).  Under a wrapper chain (Translate / Rotate / Scale) the
 *     normal is the geometric one: the object-space HitRecord.Normal brought
 *     to world space by each wrapper's true inverse and renormalised, so it
 *     is unit and faces the ray.  (The integrator's own normal there is the
 *     reference's as written: RotateX / RotateZ turn it by the ray's angle
 *     again, transform.go:256-265, :337-346.)
 *   miss or DiffuseLight: all eight floats 0 (noise-free at the camera ray;
 *     rt_denoise passes such pixels through).
 * buckets and accumulate as for rt_render: pixels outside the buckets are
 * untouched, accumulate adds to the buffer's contents.  Sums are fp64 per
 * pixel in sample order, rounded to float once per call: deterministic and
 * independent of the schedule options.  rt_render_features blocks and takes
 * a host buffer of width*height*8 floats; rt_render_features_device takes a
 * device buffer and is asynchronous on `hip_stream` (device errors are
 * reported as for rt_render_device).  A multi-device context runs the
 * feature pass on its first device only, like the probes.
 * rt_last_render_kernel_ms after either call reports the feature pass.      */
int rt_render_features(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                       float* feat, rt_stats* stats);
int rt_render_features_device(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                              float* feat_device, void* hip_stream);

/* Edge-avoiding a-trous denoiser (Dammertz et al. 2010) guided by the feature
 * buffers.  With the per-pixel means c = accum/spp and a, n, z, k = feat/spp
 * (n not renormalised): a pixel with k < 0.5 is copied to the output bit for
 * bit and is never a neighbour; the others filter e = c / max(a, albedo_eps)
 * per channel (demodulate = 1; else e = c) by `iterations` passes, pass i with
 * step 2^i over the 5x5 taps of the B3 spline [1/16, 1/4, 3/8, 1/4, 1/16]
 * (taps outside the image skipped), each tap weighted by
 *   max(0, n_p.n_q)^(2^normal_power_log2)
 *   * exp(-|z_p - z_q| / (sigma_depth * |z_p| + 1e-6))
 *   * exp(-|e_p - e_q|^2 / ((sigma_color * 2^-i)^2 + 1e-8)),
 * and the result is e * max(a, albedo_eps) * spp (e * spp): sums again, so
 * rt_tonemap_rgba8 takes it.  iterations = 0 copies the input.  Meant for the
 * preview passes (1 spp, spp/4); it blurs what the features do not describe
 * (reflections in Metal / Dielectric, shadows' edges): INTEGRATION.md.      */
typedef struct rt_denoise_params {
  int32_t iterations;        /* 0..8 a-trous passes, step 2^i; 0 copies the input      */
  int32_t normal_power_log2; /* w_n = max(0, n_p.n_q)^(2^k), by k squarings (0..16)    */
  int32_t demodulate;        /* 1: filter radiance / max(albedo, albedo_eps)           */
  float sigma_color, sigma_depth, albedo_eps;
} rt_denoise_params;
/* iterations 5, normal_power_log2 5, demodulate 1, sigma_color 4, sigma_depth
 * 0.1, albedo_eps 1e-3 (DESIGN.md "Feature buffers and denoiser").          */
int rt_denoise_default_params(rt_denoise_params* out);
/* Host arrays (accum_rgb, out_rgb: width*height*3; feat: width*height*8;
 * `spp` = the samples both sums hold); blocks.  params NULL = the defaults.
 * RT_ERR_INVALID: null pointers, non-positive sizes or spp, iterations
 * outside 0..8, out_rgb overlapping accum_rgb.                             */
int rt_denoise(rt_ctx* ctx, const float* accum_rgb, const float* feat, int32_t width, int32_t height,
               int32_t spp, const rt_denoise_params* params, float* out_rgb);
/* Same over device arrays (feat_dev 16-B aligned), asynchronous on
 * `hip_stream`: one kernel launch per iteration.                           */
int rt_denoise_device(rt_ctx* ctx, const float* accum_dev, const float* feat_dev, int32_t width, int32_t height,
                      int32_t spp, const rt_denoise_params* params, float* out_dev, void* hip_stream);

/* Radiance moments: a render that also returns, per pixel, the first two
 * moments of its samples' luminance.  `moments` holds width*height*2 floats,
 * per pixel m1 = sum_s Y_s and m2 = sum_s Y_s^2 over the call's samples, with
 *   Y = (0.2126 * L.x + 0.7152 * L.y) + 0.0722 * L.z
 * of the sample's radiance L, the products and sums in fp64 as written (no
 * fused multiply-add), the samples in the order the frame's own sums take
 * them, each moment rounded to float once per call.  accum_rgb is what
 * rt_render / rt_render_device writes for the same parameters, bit for bit:
 * it is the same render with one small kernel more per batch.  buckets and
 * accumulate as for rt_render, for both arrays: pixels outside the buckets are
 * untouched, accumulate adds to the arrays' contents (so a progressive frame
 * keeps the moments of all its samples).  Like the frame, the moments do not
 * depend on the schedule options, the node format or the volume placement.
 * From them the caller has the sample variance of a pixel's luminance,
 * (m2 / n - (m1 / n)^2) * n / (n - 1), and rt_denoise_variance its guide.
 * rt_render_moments blocks and takes host arrays; rt_render_moments_device
 * takes device arrays and is asynchronous on `hip_stream` (device errors are
 * reported as for rt_render_device).  rt_last_render_kernel_ms after either
 * call covers the whole call.  RT_ERR_UNSUPPORTED on a multi-device context
 * (rt_ctx_create_multi): render there with rt_render, or per device.        */
int rt_render_moments(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                      float* accum_rgb, float* moments, rt_stats* stats);
int rt_render_moments_device(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                             float* accum_rgb_device, float* moments_device, void* hip_stream);

/* Variance-guided a-trous denoiser: the spatial part of SVGF (Schied et al.
 * 2017).  rt_denoise with its colour weight replaced by a luminance weight
 * that is scaled by the pixel's own standard deviation, and the variance
 * filtered along with the colour.  All arithmetic is fp32 in a fixed order.
 * As for rt_denoise: the means c = accum/spp and a, n, z, k = feat/spp; a
 * pixel with k < 0.5 is copied to out_rgb bit for bit and is never a
 * neighbour; e = c / max(a, albedo_eps) per channel (demodulate = 1; else
 * e = c); the 5x5 B3 taps h, their order and the skipped taps; w_n, w_z; the
 * result e * max(a, albedo_eps) * spp.  l(e) = (0.2126 e.x + 0.7152 e.y)
 * + 0.0722 e.z.
 * Initial variance v0(p), the variance of the pixel's mean expressed for l(e):
 *   spp >= spatial_below: with n = spp, mu = m1 / n of `moments`
 *     (rt_render_moments of the same samples),
 *       var_Y = max(0, m2 / n - mu^2) / (n - 1)
 *       v0 = var_Y / max(mu^2, 1e-12) * l(e_p)^2
 *     i.e. the relative variance of Y carried over to l(e).  Demodulation
 *     divides each channel by its own per-pixel constant: for a grey albedo
 *     l(e) = Y / a and the transfer is exact, for a coloured one it is an
 *     approximation.
 *   spp < spatial_below (always at 1 spp; `moments` may be NULL): the weighted
 *     variance of l(e_q) over the 7x7 unit-step window of covered pixels q,
 *     weights w = w_n * w_z (1 for the centre), row-major:
 *       v0 = max(0, sum w l^2 / sum w - (sum w l / sum w)^2)
 * Pass i = 0 .. iterations - 1, step 2^i:
 *   g(p) = the 3x3 Gaussian (1/4 centre, 1/8 edges, 1/16 corners) of the
 *     current v at unit step over covered in-image neighbours, each weight
 *     times w_n * w_z (1 for the centre), divided by the sum of the weights
 *     used: like the taps, it does not reach across a geometric edge
 *   w_l = exp(-|l(e_p) - l(e_q)| / (sigma_lum * sqrt(g(p)) + 1e-6))
 *   w = w_n * w_z * w_l (1 for the centre tap)
 *   e'(p) = sum h w e_q / sum h w
 *   v'(p) = sum (h w)^2 v_q / (sum h w)^2
 * sigma_lum is not halved per pass: the shrinking variance narrows the weight.
 * A pixel whose samples disagree (a firefly) has a large v0, accepts its
 * neighbours and is pulled to them, while a neighbour with a small variance
 * still refuses it; rt_denoise, whose weight is centred on the pixel's own
 * noisy value, leaves such a pixel as it is.  out_var, if not NULL, receives
 * the final v (width*height floats; 0 for a passed-through pixel).
 * iterations = 0 copies the input (out_var: v0).                            */
typedef struct rt_denoise_var_params {
  int32_t iterations;        /* 0..8 a-trous passes, step 2^i; 0 copies the input      */
  int32_t normal_power_log2; /* as rt_denoise_params                                   */
  int32_t demodulate;        /* as rt_denoise_params                                   */
  int32_t spatial_below;     /* spp below this: the spatial variance estimate (>= 2)   */
  float sigma_lum, sigma_depth, albedo_eps;
} rt_denoise_var_params;
/* iterations 5, normal_power_log2 5, demodulate 1, spatial_below 4, sigma_lum
 * 8, sigma_depth 0.1, albedo_eps 1e-3 (DESIGN.md "Radiance moments and the
 * variance-guided filter").                                                 */
int rt_denoise_variance_default_params(rt_denoise_var_params* out);
/* Host arrays (accum_rgb, out_rgb: width*height*3; feat: width*height*8;
 * moments: width*height*2; out_var: width*height or NULL; `spp` = the samples
 * the sums hold); blocks.  params NULL = the defaults.  RT_ERR_INVALID: what
 * rt_denoise refuses, spatial_below < 2, moments NULL while spp >=
 * spatial_below, out_var overlapping an input or out_rgb.                   */
int rt_denoise_variance(rt_ctx* ctx, const float* accum_rgb, const float* feat, const float* moments,
                        int32_t width, int32_t height, int32_t spp, const rt_denoise_var_params* params,
                        float* out_rgb, float* out_var);
/* Same over device arrays (feat_dev 16-B aligned), asynchronous on
 * `hip_stream`: one launch for the initial variance (two in the spatial
 * case) and one per iteration.                                              */
int rt_denoise_variance_device(rt_ctx* ctx, const float* accum_dev, const float* feat_dev, const float* moments_dev,
                               int32_t width, int32_t height, int32_t spp, const rt_denoise_var_params* params,
                               float* out_dev, float* out_var_dev, void* hip_stream);

/* Adaptive sampling: a render that stops sampling a pixel once the standard
 * error of its mean luminance, estimated from its own samples, is small
 * enough, and spends the samples where it is not.
 * rt_render_params is read as for rt_render (seed, max_depth, buckets), with
 * samples_per_pixel = max_spp, the budget a uniform render would spend on
 * every pixel; sample_offset and accumulate must be 0.  adaptive NULL = the
 * defaults.  accum_rgb (width*height*3), moments (width*height*2) and counts
 * (width*height uint32) receive, for every pixel of the buckets, the sums and
 * the moments of its first counts[p] samples (sample s is rt_render's sample
 * s of that pixel: the same path key) and counts[p] itself; pixels outside
 * the buckets are untouched in all three.
 * The rounds:
 *   round 0 is rt_render_moments of the buckets' pixels with min(min_spp,
 *     max_spp) samples, offset 0, overwriting;
 *   round r >= 1, with n the samples so far, first selects the active pixels
 *     (below) and then is rt_render_moments over exactly those pixels with
 *     min(step_spp, max_spp - n) samples, sample_offset n, accumulate 1;
 *   a pixel that leaves the active set never returns, so every active pixel
 *     holds the same n;
 *   the call ends when no pixel is active or n = max_spp.
 * A round's arithmetic is the render's own, so a pixel's final value is the
 * chain float(double(previous) + fp64 sum of the round's samples), whichever
 * other pixels were listed and whatever the schedule options.
 * Selection, in fp32 with the operations as written (no fused multiply-add),
 * from the pixel's moments m1, m2 and its n:
 *   nf = float(n), mu = m1 / nf
 *   var = max(0, m2 / nf - mu * mu) / (nf - 1)     (rt_denoise_variance's var_Y)
 *   tol = rel_error * max(mu, lum_floor)
 *   unconverged(p) = var > tol * tol
 * neighbourhood 0: p stays active iff it is active and unconverged;
 * neighbourhood 1: p stays active iff it is active and it, or one of its 8
 * neighbours that is active, is unconverged.  Neighbours outside the image,
 * outside the buckets or already dropped count as converged.  The dilation
 * keeps the pixel whose first few samples all happened to agree next to
 * pixels whose samples did not.  Stopping a pixel on the variance of its own
 * samples makes its mean a biased estimator (pixels whose samples chance to
 * agree stop early): the price of every such scheme.
 * The selection runs on the device without atomics: the active list is in
 * ascending pixel order and identical from run to run.
 * Both variants block: the host reads each round's active count (4 bytes) to
 * size the next render; rt_render_adaptive_device takes device arrays and
 * saves the image copies, not the synchronisation.  rt_last_render_kernel_ms
 * after either call covers the whole call.
 * RT_ERR_INVALID: null pointers, min_spp < 2, step_spp < 1, neighbourhood
 * outside {0, 1}, rel_error / lum_floor negative or not finite, max_spp < 1,
 * more than 256 rounds possible ((max_spp - min_spp) / step_spp + 1 > 256),
 * sample_offset or accumulate not 0.  RT_ERR_NO_SCENE as for rt_render.
 * RT_ERR_UNSUPPORTED on a multi-device context, as for rt_render_moments.   */
typedef struct rt_adaptive_params {
  int32_t min_spp;        /* every listed pixel's first round; >= 2                  */
  int32_t step_spp;       /* samples per later round; >= 1                           */
  int32_t neighbourhood;  /* 0: a pixel's own estimate; 1: 3x3 dilation              */
  float rel_error;        /* target standard error of the mean luminance, relative   */
  float lum_floor;        /* ... to max(mean, lum_floor); >= 0                       */
} rt_adaptive_params;
typedef struct rt_adaptive_stats {
  double kernel_ms;       /* the whole call's span on the stream                     */
  uint64_t samples;       /* samples traced = sum of the listed pixels' counts       */
  int32_t rounds;         /* renders run, >= 1                                       */
  int32_t pixels_at_max;  /* listed pixels that stopped at max_spp, not by the test  */
} rt_adaptive_stats;
/* min_spp 16, step_spp 16, neighbourhood 1, rel_error 0.05, lum_floor 0.01
 * (DESIGN.md "Adaptive sampling").                                          */
int rt_adaptive_default_params(rt_adaptive_params* out);
int rt_render_adaptive(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                       const rt_adaptive_params* adaptive, float* accum_rgb, float* moments, uint32_t* counts,
                       rt_adaptive_stats* stats);
int rt_render_adaptive_device(rt_ctx* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                              const rt_adaptive_params* adaptive, float* accum_rgb_device, float* moments_device,
                              uint32_t* counts_device, rt_adaptive_stats* stats, void* hip_stream);
/* The selection step alone over host arrays (a probe, like rt_primary_hits;
 * needs no scene): counts[p] == 0 = not in the call, counts[p] >= max_spp =
 * done, every other pixel is active with n = counts[p].  Writes the ids
 * (y * width + x) of the pixels that stay active to list_out (room for
 * width*height) in ascending order, and their number to n_out.  params NULL =
 * the defaults; refusals as above.                                          */
int rt_adaptive_select(rt_ctx* ctx, const float* moments, const uint32_t* counts, int32_t width, int32_t height,
                       int32_t max_spp, const rt_adaptive_params* params, uint32_t* list_out, uint32_t* n_out);
/* An adaptive frame for the consumers that take one spp for the whole frame
 * (rt_tonemap_rgba8, rt_denoise, rt_denoise_variance):
 *   out[p][c] = (sums[p][c] / float(counts[p])) * float(target_spp)
 * in fp32 in that order, for `channels` (1..8) floats per pixel; a pixel with
 * counts[p] == 0 is copied bit for bit.  out may be sums.  Host arrays,
 * blocks; the _device variant takes device arrays and is asynchronous on
 * `hip_stream`.  RT_ERR_INVALID: null pointers, non-positive sizes or
 * target_spp, channels outside 1..8.                                        */
int rt_normalize_samples(rt_ctx* ctx, const float* sums, int32_t channels, const uint32_t* counts, int32_t width,
                         int32_t height, int32_t target_spp, float* out);
int rt_normalize_samples_device(rt_ctx* ctx, const float* sums_dev, int32_t channels, const uint32_t* counts_dev,
                                int32_t width, int32_t height, int32_t target_spp, float* out_dev, void* hip_stream);

/* ---- Ray queries: closest hit and occlusion for the caller's own rays ------
 * What does this ray hit in the uploaded scene?  (Picking, autofocus, bakes,
 * a caller's own integrator: INTEGRATION.md.)  Both calls run the render's
 * own traversal, so their answers are the render's.
 *
 * rt_trace_rays: hits[i] is what world.Hit(ray_i, Interval{tmin, tmax})
 * returns, decided the way the render's closest-hit kernel decides it:
 *   the closest hit, and among hits at exactly the same t the one the
 *   reference's left-first traversal reports;
 *   interval ends as the primitive tests have them: spheres and planes take
 *   tmin < t (open, Interval.Surrounds), quads, triangles and circles
 *   tmin <= t (closed, Interval.Contains); the upper end is open for all of
 *   them, t < tmax;
 *   d need not be unit: t is the ray parameter (the hit point is o + t d);
 *   top / prim are the hittable ids in rt_primary_hits' convention, material
 *   the winning primitive's index into rt_scene_desc.materials;
 *   n is HitRecord.Normal (face-forwarded against d, and under transform
 *   wrappers the normal the reference's wrappers hand back), RT_HIT_FRONT is
 *   HitRecord.FrontFace;
 *   a miss is t = -1, top = prim = material = -1, n = 0, flags = 0.
 * A ray with tmin = 0.001f and tmax = +inf gets, bit for bit, the ids and t
 * the render's k_extend finds for that ray (rt_extend_hits).
 *
 * rt_occluded: the any-hit form, the rule of the render's shadow rays:
 * occluded[i] = 1 when anything is hit in the interval, else 0.  The lower
 * end is as above; the upper end is closed for quads, triangles and circles
 * (t <= tmax) and open for spheres and planes (t < tmax).  Keep tmin / tmax
 * away from exact hit distances if the end matters.
 *
 * Planes, circles and the world quads / spheres that the scene upload lifts
 * out of the BVH (RT_OPT_LIFT_PRIMS) take part in both calls.
 *
 * time is the call's ray.Time(): moving spheres are evaluated at it.  A
 * caller with several times makes several calls.
 *
 * A ray with a non-finite origin or direction component, a zero direction, a
 * NaN tmin or tmax, or tmax < tmin is reported as a miss (not occluded) with
 * RT_HIT_INVALID_RAY set; it traces nothing and raises no device error.
 *
 * The host variants block; they stage the arrays through buffers the context
 * owns (grown on demand, freed with it).  The _device variants take device
 * arrays and are asynchronous on `hip_stream` (NULL = the context's stream);
 * a device error surfaces as for rt_render_device (the next call, rt_sync).
 * A multi-device context answers queries on its first device.  n may exceed
 * 2^30: the call then runs several launches.
 * RT_ERR_INVALID: null pointers, n < 0, a non-finite time.  n == 0 is RT_OK
 * and launches nothing.  RT_ERR_NO_SCENE as for rt_render.
 * RT_ERR_UNSUPPORTED: the scene holds an RT_VOLUME.  Volume.Hit draws random
 * numbers from the path's key and a bare ray has none; a variant that takes
 * a key per ray is a follow-up.                                             */
typedef struct rt_ray { float o[3]; float tmin; float d[3]; float tmax; } rt_ray;          /* 32 B */
typedef struct rt_ray_hit { float t; int32_t top; int32_t prim; int32_t material;
                            float n[3]; uint32_t flags; } rt_ray_hit;                      /* 32 B */
enum { RT_HIT_FRONT = 1, RT_HIT_INVALID_RAY = 2 };

int rt_trace_rays(rt_ctx* ctx, const rt_ray* rays, int64_t n, float time, rt_ray_hit* hits);
int rt_trace_rays_device(rt_ctx* ctx, const rt_ray* rays_dev, int64_t n, float time, rt_ray_hit* hits_dev,
                         void* hip_stream);
int rt_occluded(rt_ctx* ctx, const rt_ray* rays, int64_t n, float time, uint8_t* occluded);
int rt_occluded_device(rt_ctx* ctx, const rt_ray* rays_dev, int64_t n, float time, uint8_t* occluded_dev,
                       void* hip_stream);

/* ---- Camera.RayColor for the caller's rays (camera.go:438-518) -------------
 * What radiance arrives along this ray?  (Light probes, irradiance and
 * lightmap bakes, reflection captures, an orthographic, panoramic or fisheye
 * camera, a caller's own sampling pattern: INTEGRATION.md.)  The path integral
 * of the render, started at rays the caller supplies instead of at a camera's
 * pixels.
 *
 * Result: rgb[3*i .. 3*i+2] is the sum, over the call's `samples` samples, of
 * rayColorInternal(ray_i, max_depth): linear radiance, and the caller divides
 * by the sample count, as for rt_render.  Sample s of ray i runs under the
 * path key path_key(seed, rays[i].id, sample_offset + s) and goes through
 * exactly what a render's path goes through from bounce 0 on: the same
 * kernels, the interval (0.001, +inf), the world quads / spheres the upload
 * lifts (RT_OPT_LIFT_PRIMS), volumes in either RT_OPT_VOLUMES placement, next
 * event estimation, the light-hit rule, the clamp, and the long-tail kernel
 * (RT_OPT_TAIL).  Scenes with an RT_VOLUME are served: a path carries the key
 * Volume.Hit draws from.
 *
 * id is only the RNG key's pixel word; it has nothing to do with where the
 * result is written (always slot i).  Rays that share an id and a sample index
 * follow the same random decisions; distinct ids give independent paths.
 * Give every ray of a bake its own id.
 *
 * ray.Time() is the key's camera-domain time draw (camera.go:370), as in a
 * render, so moving spheres blur over a ray's samples.  There is no per-ray
 * time, tmin or tmax.  d need not be unit (camera rays are not unit either).
 *
 * Of the Camera the call reads only what rayColorInternal reads: background,
 * use_sky_gradient, and phantom_hdri with camera_max_depth (the phantom test is
 * depth == camera_max_depth, so it fires only for a ray traced at that depth;
 * 0 = max_depth).  The environment and the lights are the uploaded scene's.
 *
 * The equality that defines it: take the float rays rt_extend_hits reports at
 * bounce 0 for sample s of a camera (GetRay's rays), set id = y*W + x,
 * samples = 1, sample_offset = s and copy the camera's background, sky,
 * phantom and max_depth fields; then rgb is the frame rt_render writes for
 * samples_per_pixel = 1, sample_offset = s, bit for bit, under every node
 * format, schedule option, volume placement and RT_OPT_LIFT_PRIMS setting
 * under which rt_render itself is invariant.
 *
 * Sums are fp64 per ray in sample order across batches, rounded to float once
 * per call; accumulate != 0 adds double(rgb's previous value) to the sum
 * before that rounding (rt_render_params.accumulate's rule).  The result does
 * not depend on RT_OPT_BATCH_SLOTS, RT_OPT_STREAMS, RT_OPT_MAX_BLOCKS,
 * RT_OPT_TAIL or RT_OPT_OVERLAP, nor on how the call cuts the ray array: n may
 * exceed what one batch holds, and the call then renders consecutive ranges
 * of the array in turn.  Neighbouring rays are traced together, so keep rays
 * that are close in space close in the array (scanline or tile order).
 *
 * A ray with a non-finite origin or direction component, or a zero direction,
 * traces nothing: it adds (0,0,0), raises no device error, and is counted in
 * stats->invalid_rays (host variant only).
 *
 * The host variant blocks; it stages the arrays through buffers the context
 * owns (grown on demand, freed with it).  The _device variant takes device
 * arrays and is asynchronous on `hip_stream` (NULL = the context's stream); a
 * device error surfaces as for rt_render_device.  rt_last_render_kernel_ms
 * covers the call.  A multi-device context runs it on its first device.
 * RT_ERR_INVALID: null pointers, n < 0 or n > 2^31 - 1, samples < 1,
 * max_depth < 1, sample_offset < 0, camera_max_depth < 0, a non-finite
 * background, or a ray's reserved != 0 (checked by the host variant only).
 * n == 0 is RT_OK and launches nothing.  RT_ERR_NO_SCENE as for rt_render.
 * Not offered (yet): per-ray tmin / tmax or time, moments or adaptive sampling
 * over rays, feature buffers for rays, dealing rays over several devices, a
 * keyed rt_trace_rays.                                                       */
typedef struct rt_path_ray { float o[3]; uint32_t id; float d[3]; uint32_t reserved; } rt_path_ray;  /* 32 B */

typedef struct rt_ray_color_params {
  int32_t samples;          /* paths per ray, >= 1                                   */
  int32_t max_depth;        /* the depth RayColor is called with, >= 1               */
  int32_t sample_offset;    /* first sample index (RNG key), >= 0                    */
  uint32_t seed;
  int32_t accumulate;       /* as rt_render_params.accumulate                        */
  int32_t use_sky_gradient; /* Camera.UseSkyGradient                                 */
  int32_t phantom_hdri;     /* Camera.PhantomHDRI                                    */
  int32_t camera_max_depth; /* Camera.MaxDepth for the PhantomHDRI test; 0 = max_depth */
  double background[3];     /* Camera.Background                                     */
} rt_ray_color_params;

typedef struct rt_ray_color_stats { double kernel_ms; uint64_t samples; uint64_t invalid_rays; } rt_ray_color_stats;

int rt_ray_color(rt_ctx* ctx, const rt_path_ray* rays, int64_t n, const rt_ray_color_params* params, float* rgb,
                 rt_ray_color_stats* stats /* may be NULL */);
int rt_ray_color_device(rt_ctx* ctx, const rt_path_ray* rays_dev, int64_t n, const rt_ray_color_params* params,
                        float* rgb_dev, void* hip_stream);

/* ---- Gathers: path integrals over directions drawn on the device -----------
 * How much light arrives at this point?  (Irradiance and lightmap bakes,
 * light probes, ambient gathers: INTEGRATION.md §4.)  rt_ray_color with a new
 * direction for every sample of every point, drawn on the device from a 32-B
 * record per point, so nothing per sample crosses the bus.
 *
 * Result: rgb[3*i .. 3*i+2] is the sum, over path.samples samples, of
 * rayColorInternal(ray_{i,s}, max_depth).  Everything rt_ray_color documents
 * holds unchanged: the fp64 per-point sum in sample order rounded once,
 * accumulate, the cut of the array into ranges, the independence of the
 * schedule options, volumes, the ray time from the key's camera draw 2, the
 * first device of a multi-device context, how errors surface, the limits on n
 * and n == 0.
 *
 * Only the ray of sample s is new.  Its key is path_key(seed, pts[i].id,
 * sample_offset + s), its origin is p, and its direction d comes from `source`,
 * in fp32 in the order written with no fused multiply-add:
 *   RT_GATHER_RAY     d = n, as given.  The call is rt_ray_color on the same
 *                     32 bytes, bit for bit (for every point valid here).
 *   RT_GATHER_COSINE  nh = unit(n); u = random_unit_vector(key, bounce 0,
 *                     DOM_SOURCE = 7, index 0); d = nh + u, and d = nh where
 *                     near_zero(d).  Lambertian.Scatter's direction
 *                     (material.go:33-80): density cos(theta)/pi about nh, so
 *                     the irradiance at the point is pi * rgb / samples.
 *   RT_GATHER_SPHERE  d = random_unit_vector(key, 0, DOM_SOURCE, 0); n is not
 *                     read.  The mean over the sphere is rgb / samples.
 * The path's own draws (camera 2, scatter, NEE, volumes) keep their addresses.
 * After 64 rejected tries random_unit_vector returns (0,0,1).
 *
 * A point is invalid when a component of p is non-finite, and, for RAY and
 * COSINE, when a component of n is non-finite or n's fp32 length
 * sqrtf(x*x + y*y + z*z) is 0 or not finite (so a normal whose squared length
 * leaves fp32's range is invalid even for RAY).  An invalid point traces
 * nothing, adds (0,0,0), raises no device error, and is counted in
 * stats->invalid_rays (host variant only).
 *
 * rt_gather_rays is the probe: out[i] is the rt_path_ray that sample `sample`
 * (the index itself: sample_offset + s) of point i traces, and
 * {p, id, (0,0,0), 0} for an invalid point, which rt_ray_color treats as
 * invalid too.  The equality that defines rt_gather: rt_ray_color over
 * rt_gather_rays(.., s) with samples = 1, sample_offset = s is rt_gather with
 * samples = 1, sample_offset = s, bit for bit.  It needs no uploaded scene,
 * blocks, and stages through buffers the context owns.
 *
 * RT_ERR_INVALID: everything rt_ray_color refuses, a source outside 0..2, a
 * non-zero params->reserved, a point's reserved != 0 (host variant only), and
 * for rt_gather_rays sample < 0.
 * Not offered by this call: next-event estimation at the gather point itself
 * (direct light reaches a point only through rays that hit an emitter, as for
 * a camera ray; rt_gather_surface, below, samples the lights at the point as
 * the render does at a diffuse hit).  Not offered (yet): moments or adaptive
 * sampling over points, per-point source kinds.
 * (The projection of a probe onto spherical harmonics is rt_gather_sh, below.) */
enum { RT_GATHER_RAY = 0, RT_GATHER_COSINE = 1, RT_GATHER_SPHERE = 2 };
typedef struct rt_gather_point { float p[3]; uint32_t id; float n[3]; uint32_t reserved; } rt_gather_point; /* 32 B, rt_path_ray's layout */
typedef struct rt_gather_params { rt_ray_color_params path; int32_t source; int32_t reserved; } rt_gather_params; /* 64 B */

int rt_gather(rt_ctx* ctx, const rt_gather_point* pts, int64_t n, const rt_gather_params* params, float* rgb,
              rt_ray_color_stats* stats /* may be NULL */);
int rt_gather_device(rt_ctx* ctx, const rt_gather_point* pts_dev, int64_t n, const rt_gather_params* params,
                     float* rgb_dev, void* hip_stream);
/* probe: the ray sample `sample` of every point traces */
int rt_gather_rays(rt_ctx* ctx, const rt_gather_point* pts, int64_t n, int32_t source, uint32_t seed, int32_t sample,
                   rt_path_ray* out);

/* ---- SH projection of a probe: rt_gather over the sphere, kept by direction -
 * Which light arrives at this point, from where?  A light probe is radiance as
 * a function of direction, stored as a few spherical-harmonic coefficients
 * (INTEGRATION.md §4).  rt_gather(RT_GATHER_SPHERE) folds a point's directions
 * into one sum; this call keeps them apart: every sample's radiance is weighted
 * with the SH basis at its own direction, on the device, so nothing per sample
 * crosses the bus.
 *
 * Rays: the ray of sample s of point i is exactly rt_gather's under
 * RT_GATHER_SPHERE: its key is path_key(seed, pts[i].id, sample_offset + s),
 * its origin is p and its direction is d = random_unit_vector(key, 0,
 * DOM_SOURCE, 0); n is not read.  Everything rt_gather and rt_ray_color
 * document holds unchanged: volumes, next-event estimation along the path,
 * lifted primitives and the long-tail kernel, the independence of the schedule
 * options and of the cut of the array into ranges, the first device of a
 * multi-device context, how device errors surface, n == 0 and the limit on n.
 *
 * Basis: with L the float radiance rayColorInternal(ray_{i,s}, max_depth) of
 * that sample and (x, y, z) = d, in fp32 in the order written with no fused
 * multiply-add (the real, all-positive convention of Ramamoorthi & Hanrahan
 * 2001; the scene's axes as they are):
 *   Y0 = 0.282095f
 *   Y1 = 0.488603f*y       Y2 = 0.488603f*z       Y3 = 0.488603f*x
 *   Y4 = 1.092548f*(x*y)   Y5 = 1.092548f*(y*z)   Y6 = 0.315392f*(3.0f*(z*z) - 1.0f)
 *   Y7 = 1.092548f*(x*z)   Y8 = 0.546274f*(x*x - y*y)
 * bands = b keeps Y0 .. Y(b*b-1): 1, 4 or 9 coefficients per point, and the
 * coefficients of a smaller b are the first of a larger one, bit for bit.
 *
 * Result: sh[(i*b*b + k)*3 + c] = float(sum_s double(L_s.c) * double(Y_k(d_s))).
 * The sum is fp64 in sample order across batches, rounded to float once per
 * call; the product of two floats is exact in fp64.  accumulate != 0 adds
 * double(sh's previous value) to the sum before that rounding, so a probe is
 * refined over calls with growing sample_offset.  The sums are not scaled:
 * the projection coefficients of the radiance are c_k = (4 pi / samples) * sh,
 * and the irradiance about a unit normal n is
 *   E(n) = sum_l A_l sum_m c_lm Y_lm(n),  A_0 = pi, A_1 = 2 pi / 3, A_2 = pi / 4
 * (l = 0: k = 0; l = 1: k = 1..3; l = 2: k = 4..8), evaluated by the caller.
 *
 * A point with a non-finite component of p is invalid: it traces nothing and
 * draws nothing, adds 0 to every coefficient (with accumulate it keeps its
 * previous values), raises no device error, and is counted in
 * stats->invalid_rays (host variant only).
 *
 * The equality that defines it: for every s < samples take the rays of
 * rt_gather_rays(pts, RT_GATHER_SPHERE, seed, sample_offset + s) and
 * rt_ray_color over them with samples = 1 and that offset; project those in
 * fp64 by the formulas above, in order s, and round once: that is rt_gather_sh,
 * bit for bit.
 *
 * RT_ERR_INVALID: everything rt_ray_color refuses, bands outside 1..3, a
 * non-zero params->reserved, a point's reserved != 0 (host variant only).
 * Not offered (yet): bands above 3, a cosine- or otherwise-weighted
 * projection, irradiance evaluation on the device, moments per coefficient.   */
enum { RT_SH_MAX_BANDS = 3 };
typedef struct rt_gather_sh_params {
  rt_ray_color_params path;   /* as rt_gather_params.path                         */
  int32_t bands;              /* 1..3: bands*bands coefficients per point (1,4,9) */
  int32_t reserved;           /* 0                                                */
} rt_gather_sh_params;        /* 64 B, rt_gather_params' layout */

int rt_gather_sh(rt_ctx* ctx, const rt_gather_point* pts, int64_t n, const rt_gather_sh_params* params,
                 float* sh /* n * bands*bands * 3 */, rt_ray_color_stats* stats /* may be NULL */);
int rt_gather_sh_device(rt_ctx* ctx, const rt_gather_point* pts_dev, int64_t n, const rt_gather_sh_params* params,
                        float* sh_dev, void* hip_stream);

/* ---- Surface gathers: next-event estimation at the gather point ------------
 * What does the render put on this texel?  (Irradiance and lightmap bakes
 * under small lights: INTEGRATION.md §4.)  rt_gather(RT_GATHER_COSINE) starts
 * a plain ray at every point, so direct light reaches a texel only through
 * rays that happen to hit an emitter.  This call treats the point as the
 * render's own first diffuse vertex instead: it samples the lights at the
 * point (sampleLightMIS, camera.go:502-678) and continues the scattered path
 * under the light-hit rule.
 *
 * Sample s of point i runs under key = path_key(seed, pts[i].id,
 * sample_offset + s).  It is the path rayColorInternal(., max_depth) continues
 * after its world.Hit at bounce 0 returned a front-face hit with P = p,
 * Normal = nh = unit(n), and a Lambertian of SolidColor(1,1,1).  From there,
 * in fp32 in the order written with no fused multiply-add:
 *   Emission        none is added at the vertex.
 *   Scattered ray   origin p, direction sd = nh + random_unit_vector(key,
 *                   bounce 0, DOM_SCATTER = 1, index 0), and sd = nh where
 *                   near_zero(sd): Lambertian.Scatter with the path's own
 *                   scatter draw of bounce 0 (not DOM_SOURCE).  The
 *                   attenuation is (1,1,1).
 *   NEE             when the scene has lights: the render's set-up at bounce 0
 *                   with rec.P = p, rec.N = nh, att = 1: the light select at
 *                   (0, DOM_NEE, 0), sampleHDRILight when the environment is
 *                   importance-sampled, sampleAreaLight with its cuts (cos <= 0,
 *                   cosLight < 0.001), the weight pdfL / (pdfL + pdfB), the
 *                   factor num_lights, the clamp at 20 and the shadow-ray end
 *                   min(dist - 0.001, dist * (1 - 2^-20)); lifted volumes and
 *                   lifted world primitives clear a shadow ray as in a render.
 *   Continuation    the path goes on at bounce 1 with depth_left =
 *                   max_depth - 1 and, by the light-hit rule, counts an emitter
 *                   it hits only when the scene has no lights.  max_depth = 1
 *                   is therefore a direct-only bake; with no lights in the
 *                   scene the call traces what RT_GATHER_COSINE traces, from
 *                   another RNG address.
 * Result: rgb[3*i .. 3*i+2] is the sum of those path radiances over
 * path.samples samples.  pi * rgb / samples is the radiosity-consistent
 * irradiance at the point as the render estimates it.
 *
 * How it differs from RT_GATHER_COSINE: this is the reference's estimator as
 * written.  With lights present a light sample adds emission * cos / pdfL
 * (no 1/pi of the Lambertian BRDF) weighted by pdfL / (pdfL + pdfB) and clamped
 * at 20, and a scattered ray that then hits an emitter adds nothing, so its
 * expectation differs from COSINE's unbiased one: in direct light by about
 * pi * weight, brighter wherever the weight is near 1 (a small or far light).
 * It equals the rendered radiance of a white Lambertian texel: what rt_render
 * shows of the same wall.
 *
 * The equality that defines it: take any rt_path_ray r whose closest hit is a
 * front or back face of a Lambertian SolidColor(1,1,1) quad with an
 * axis-aligned normal, no lifted volume entered before that hit.  Take t and n
 * from rt_trace_rays(r, tmin = 0.001f, tmax = +inf) and P = o + d*t per
 * component in fp32 (the product rounded, then the sum).  Then
 * rt_gather_surface({P, r.id, n}, params) equals rt_ray_color(r, params.path),
 * all bytes, under every node format, volume placement, RT_OPT_LIFT_PRIMS
 * setting and schedule option.
 *
 * Everything else is rt_gather's rule, unchanged: the fp64 in-order per-point
 * sum rounded once, accumulate, the cut of the array into ranges, the
 * independence of RT_OPT_BATCH_SLOTS, RT_OPT_STREAMS, RT_OPT_MAX_BLOCKS,
 * RT_OPT_TAIL, RT_OPT_OVERLAP and RT_OPT_EARLY_MISS, volumes in both
 * placements, the scattered ray's time from the key's camera draw 2 (shadow
 * rays run at time 0), the first device of a multi-device context, how errors
 * surface, n <= 2^31 - 1 and n == 0.
 *
 * A point is invalid by RT_GATHER_COSINE's rule: a non-finite component of p
 * or n, or an fp32 length of n that is 0 or not finite.  It draws nothing,
 * adds (0,0,0), and is counted in stats->invalid_rays (host variant only).
 *
 * RT_ERR_INVALID: everything rt_ray_color refuses, a non-zero
 * params->reserved[k], a point's reserved != 0 (host variant only).
 * Not offered (yet): a surface albedo or a BSDF other than white Lambertian
 * at the point, an SH or moments variant, a probe for the NEE records,
 * unbiased MIS at the first vertex (a departure from the reference), dealing
 * points over several devices.                                              */
typedef struct rt_gather_surface_params {
  rt_ray_color_params path;   /* as rt_gather_params.path */
  int32_t reserved[2];        /* 0                        */
} rt_gather_surface_params;   /* 64 B, rt_gather_params' layout */

int rt_gather_surface(rt_ctx* ctx, const rt_gather_point* pts, int64_t n, const rt_gather_surface_params* params,
                      float* rgb, rt_ray_color_stats* stats /* may be NULL */);
int rt_gather_surface_device(rt_ctx* ctx, const rt_gather_point* pts_dev, int64_t n,
                             const rt_gather_surface_params* params, float* rgb_dev, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RTGPU_H */
