"""go-raytracing_amd — MI355X-native path tracer for byvfx/go-raytracing scenes.

Python binding (ctypes) over the two native libraries built in ``lib/``:

* ``librtgpu.so``  — the drop-in C-ABI of ``include/rtgpu.h`` (scene graph
  upload, GPU render, tonemap, parity probes).  This is what the Go host binds
  through cgo.
* ``librtscene.so`` — the C++ mirror of the reference's host-side ``rt`` API
  (``scenes.go`` builders, ``NewBVHNode``, loaders, ``NewBucketRenderer``;
  ``include/rtscene.h``), standing in for the Go host (no Go toolchain here).

There is no CPU fallback: if the libraries are missing or no GPU is present the
calls fail loudly.  The package directory has a hyphen, so import it with
``load_package()`` from ``__graft_entry__`` / tests (importlib by path).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# RTGPU_LIB_DIR: an alternative in-tree build (A/B experiments), e.g. lib_w5
LIB_DIR = os.path.join(PKG_DIR, os.environ.get("RTGPU_LIB_DIR", "lib"))
REPO_DIR = os.path.dirname(PKG_DIR)
ASSET_DIR = os.path.join(REPO_DIR, "assets")

RT_OK = 0
RT_OPT_BLAS_BUILDER, RT_OPT_TLAS_BUILDER, RT_OPT_NODE_FORMAT = 1, 2, 3
RT_OPT_BATCH_SLOTS, RT_OPT_REFILL, RT_OPT_MAX_BLOCKS, RT_OPT_STREAMS = 4, 5, 6, 7
RT_OPT_VOLUMES = 8
RT_VOLUMES_LIFTED, RT_VOLUMES_IN_BVH = 0, 1
RT_OPT_BVH4_COLLAPSE = 9
RT_COLLAPSE_SAH, RT_COLLAPSE_GREEDY = 0, 1
RT_BLAS_REFERENCE, RT_BLAS_SAH, RT_BLAS_DEVICE = 0, 1, 2
RT_NODES_FP32, RT_NODES_QUANT8, RT_NODES_WIDE8 = 0, 1, 2
RT_OPT_DEALING, RT_OPT_DEAL_FIRST = 10, 11
RT_OPT_TAIL = 12
RT_OPT_OVERLAP = 13
RT_OPT_LIFT_PRIMS = 14
RT_OPT_EARLY_MISS = 15
RT_PRIMS_LIFTED, RT_PRIMS_IN_BVH = 0, 1
RT_DEAL_STATIC, RT_DEAL_DYNAMIC = 0, 1
STATUS = {0: "RT_OK", -1: "RT_ERR_INVALID", -2: "RT_ERR_UNSUPPORTED", -3: "RT_ERR_HIP", -4: "RT_ERR_OOM",
          -5: "RT_ERR_NO_SCENE", -6: "RT_ERR_DEVICE"}

# hittable kinds (rtgpu.h)
RT_SPHERE, RT_QUAD, RT_TRIANGLE, RT_PLANE, RT_LIST, RT_BVH_NODE, RT_BVH_LEAF = 1, 2, 3, 4, 5, 6, 7
RT_TRANSLATE, RT_ROTATE_X, RT_ROTATE_Y, RT_ROTATE_Z, RT_SCALE, RT_VOLUME = 8, 9, 10, 11, 12, 13
RT_CIRCLE = 14
RT_LAMBERTIAN, RT_METAL, RT_DIELECTRIC, RT_DIFFUSE_LIGHT, RT_ISOTROPIC = 1, 2, 3, 4, 5
RT_TEX_SOLID, RT_TEX_CHECKER, RT_TEX_NOISE, RT_TEX_IMAGE = 1, 2, 3, 4


class RtHittable(C.Structure):
    _fields_ = [("kind", C.c_int32), ("material", C.c_int32), ("a", C.c_int32), ("b", C.c_int32),
                ("bbox", C.c_double * 6), ("p", C.c_double * 16)]


class RtMaterial(C.Structure):
    _fields_ = [("kind", C.c_int32), ("texture", C.c_int32), ("albedo", C.c_double * 3), ("fuzz", C.c_double),
                ("refraction_index", C.c_double)]


class RtTexture(C.Structure):
    _fields_ = [("kind", C.c_int32), ("even", C.c_int32), ("odd", C.c_int32), ("albedo", C.c_double * 3),
                ("inv_scale", C.c_double), ("scale", C.c_double), ("perlin", C.c_int32), ("image", C.c_int32)]


class RtImage(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb", C.POINTER(C.c_double))]


class RtPerlin(C.Structure):
    _fields_ = [("randvec", (C.c_double * 3) * 256), ("perm_x", C.c_int32 * 256), ("perm_y", C.c_int32 * 256),
                ("perm_z", C.c_int32 * 256)]


class RtEnvironment(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb", C.POINTER(C.c_double)),
                ("rotation", C.c_double), ("use_importance_sampling", C.c_int32)]


class RtSceneDesc(C.Structure):
    _fields_ = [("hittables", C.POINTER(RtHittable)), ("num_hittables", C.c_int32),
                ("children", C.POINTER(C.c_int32)), ("num_children", C.c_int32), ("root", C.c_int32),
                ("materials", C.POINTER(RtMaterial)), ("num_materials", C.c_int32),
                ("textures", C.POINTER(RtTexture)), ("num_textures", C.c_int32),
                ("lights", C.POINTER(C.c_int32)), ("num_lights", C.c_int32),
                ("environment", C.POINTER(RtEnvironment)),
                ("images", C.POINTER(RtImage)), ("num_images", C.c_int32),
                ("perlins", C.POINTER(RtPerlin)), ("num_perlins", C.c_int32)]


class RtCameraDesc(C.Structure):
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("samples_per_pixel", C.c_int32),
                ("max_depth", C.c_int32), ("center", C.c_double * 3), ("pixel00", C.c_double * 3),
                ("pixel_delta_u", C.c_double * 3), ("pixel_delta_v", C.c_double * 3),
                ("defocus_angle", C.c_double), ("defocus_disk_u", C.c_double * 3),
                ("defocus_disk_v", C.c_double * 3), ("background", C.c_double * 3),
                ("use_sky_gradient", C.c_int32), ("phantom_hdri", C.c_int32), ("camera_motion", C.c_int32),
                ("free_camera", C.c_int32), ("center_motion_orig", C.c_double * 3),
                ("center_motion_dir", C.c_double * 3), ("look_at_motion_orig", C.c_double * 3),
                ("look_at_motion_dir", C.c_double * 3), ("vup", C.c_double * 3), ("forward", C.c_double * 3),
                ("viewport_width", C.c_double), ("viewport_height", C.c_double), ("focus_dist", C.c_double),
                ("defocus_radius", C.c_double)]


class RtBucket(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class RtRenderParams(C.Structure):
    _fields_ = [("samples_per_pixel", C.c_int32), ("max_depth", C.c_int32), ("sample_offset", C.c_int32),
                ("seed", C.c_uint32), ("buckets", C.POINTER(RtBucket)), ("num_buckets", C.c_int32),
                ("accumulate", C.c_int32)]


class RtStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("samples", C.c_uint64)]


class RtDenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("normal_power_log2", C.c_int32), ("demodulate", C.c_int32),
                ("sigma_color", C.c_float), ("sigma_depth", C.c_float), ("albedo_eps", C.c_float)]


class RtDenoiseVarParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("normal_power_log2", C.c_int32), ("demodulate", C.c_int32),
                ("spatial_below", C.c_int32), ("sigma_lum", C.c_float), ("sigma_depth", C.c_float),
                ("albedo_eps", C.c_float)]


class RtAdaptiveParams(C.Structure):
    _fields_ = [("min_spp", C.c_int32), ("step_spp", C.c_int32), ("neighbourhood", C.c_int32),
                ("rel_error", C.c_float), ("lum_floor", C.c_float)]


class RtAdaptiveStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("samples", C.c_uint64), ("rounds", C.c_int32),
                ("pixels_at_max", C.c_int32)]


class RtRay(C.Structure):
    """rt_ray (32 B): origin, tmin, direction, tmax."""
    _fields_ = [("o", C.c_float * 3), ("tmin", C.c_float), ("d", C.c_float * 3), ("tmax", C.c_float)]


class RtRayHit(C.Structure):
    """rt_ray_hit (32 B): t, top, prim, material, normal, flags."""
    _fields_ = [("t", C.c_float), ("top", C.c_int32), ("prim", C.c_int32), ("material", C.c_int32),
                ("n", C.c_float * 3), ("flags", C.c_uint32)]


RT_HIT_FRONT = 1
RT_HIT_INVALID_RAY = 2
# numpy views of arrays of the two structs
RAY_DTYPE = np.dtype([("o", np.float32, 3), ("tmin", np.float32), ("d", np.float32, 3), ("tmax", np.float32)])
RAY_HIT_DTYPE = np.dtype([("t", np.float32), ("top", np.int32), ("prim", np.int32), ("material", np.int32),
                          ("n", np.float32, 3), ("flags", np.uint32)])


def make_rays(o, d, tmin=0.001, tmax=float("inf")) -> np.ndarray:
    """An array of rt_ray (RAY_DTYPE) from origins and directions (n, 3) and
    per-ray or scalar tmin / tmax."""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and directions differ in shape")
    rays = np.zeros(o.shape[0], RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    rays["tmin"] = np.broadcast_to(np.asarray(tmin, np.float32), (o.shape[0],))
    rays["tmax"] = np.broadcast_to(np.asarray(tmax, np.float32), (o.shape[0],))
    return rays


class RtPathRay(C.Structure):
    """rt_path_ray (32 B): origin, id (the RNG key's pixel word), direction, reserved (0)."""
    _fields_ = [("o", C.c_float * 3), ("id", C.c_uint32), ("d", C.c_float * 3), ("reserved", C.c_uint32)]


class RtRayColorParams(C.Structure):
    _fields_ = [("samples", C.c_int32), ("max_depth", C.c_int32), ("sample_offset", C.c_int32), ("seed", C.c_uint32),
                ("accumulate", C.c_int32), ("use_sky_gradient", C.c_int32), ("phantom_hdri", C.c_int32),
                ("camera_max_depth", C.c_int32), ("background", C.c_double * 3)]


class RtRayColorStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("samples", C.c_uint64), ("invalid_rays", C.c_uint64)]


PATH_RAY_DTYPE = np.dtype([("o", np.float32, 3), ("id", np.uint32), ("d", np.float32, 3), ("reserved", np.uint32)])


def make_path_rays(o, d, ids=None) -> np.ndarray:
    """An array of rt_path_ray (PATH_RAY_DTYPE) from origins and directions
    (n, 3); ids: each ray's RNG key word (default: its index)."""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and directions differ in shape")
    rays = np.zeros(o.shape[0], PATH_RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    rays["id"] = np.arange(o.shape[0], dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32).reshape(-1)
    return rays


def ray_color_params(samples: int, depth: int, seed: int = 1, sample_offset: int = 0, camera=None,
                     accumulate: bool = False, **sky) -> RtRayColorParams:
    """rt_ray_color_params.  camera: an RtCameraDesc whose background,
    use_sky_gradient, phantom_hdri and max_depth (as camera_max_depth) are
    copied; **sky: any of those four fields by name, overriding the camera's."""
    p = RtRayColorParams()
    p.samples, p.max_depth, p.sample_offset, p.seed = samples, depth, sample_offset, seed
    p.accumulate = 1 if accumulate else 0
    if camera is not None:
        p.background = camera.background
        p.use_sky_gradient, p.phantom_hdri, p.camera_max_depth = camera.use_sky_gradient, camera.phantom_hdri, camera.max_depth
    for k, v in sky.items():
        if k == "background":
            p.background = (C.c_double * 3)(*[float(x) for x in v])
        elif k in ("use_sky_gradient", "phantom_hdri", "camera_max_depth"):
            setattr(p, k, int(v))
        else:
            raise TypeError(f"unknown rt_ray_color_params field {k!r}")
    return p


# rt_gather's direction sources
RT_GATHER_RAY = 0
RT_GATHER_COSINE = 1
RT_GATHER_SPHERE = 2


class RtGatherPoint(C.Structure):
    """rt_gather_point (32 B, rt_path_ray's layout): position, id (the RNG key's pixel word), normal, reserved (0)."""
    _fields_ = [("p", C.c_float * 3), ("id", C.c_uint32), ("n", C.c_float * 3), ("reserved", C.c_uint32)]


class RtGatherParams(C.Structure):
    _fields_ = [("path", RtRayColorParams), ("source", C.c_int32), ("reserved", C.c_int32)]


GATHER_POINT_DTYPE = np.dtype([("p", np.float32, 3), ("id", np.uint32), ("n", np.float32, 3), ("reserved", np.uint32)])


def make_gather_points(p, n, ids=None) -> np.ndarray:
    """An array of rt_gather_point (GATHER_POINT_DTYPE) from positions and
    normals (n, 3); ids: each point's RNG key word (default: its index)."""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    n = np.asarray(n, np.float32).reshape(-1, 3)
    if p.shape != n.shape:
        raise ValueError("positions and normals differ in shape")
    pts = np.zeros(p.shape[0], GATHER_POINT_DTYPE)
    pts["p"], pts["n"] = p, n
    pts["id"] = np.arange(p.shape[0], dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32).reshape(-1)
    return pts


def gather_params(source: int, samples: int, depth: int, seed: int = 1, sample_offset: int = 0, camera=None,
                  accumulate: bool = False, **sky) -> RtGatherParams:
    """rt_gather_params: `source` (RT_GATHER_*) and the path fields of ray_color_params."""
    g = RtGatherParams()
    g.path = ray_color_params(samples, depth, seed, sample_offset, camera, accumulate, **sky)
    g.source = source
    return g


RT_SH_MAX_BANDS = 3


class RtGatherShParams(C.Structure):
    """rt_gather_sh_params (64 B, rt_gather_params' layout)."""
    _fields_ = [("path", RtRayColorParams), ("bands", C.c_int32), ("reserved", C.c_int32)]


def gather_sh_params(bands: int, samples: int, depth: int, seed: int = 1, sample_offset: int = 0, camera=None,
                     accumulate: bool = False, **sky) -> RtGatherShParams:
    """rt_gather_sh_params: `bands` (1..3) and the path fields of ray_color_params."""
    g = RtGatherShParams()
    g.path = ray_color_params(samples, depth, seed, sample_offset, camera, accumulate, **sky)
    g.bands = bands
    return g


class RtGatherSurfaceParams(C.Structure):
    """rt_gather_surface_params (64 B, rt_gather_params' layout)."""
    _fields_ = [("path", RtRayColorParams), ("reserved", C.c_int32 * 2)]


def surface_params(samples: int, depth: int, seed: int = 1, sample_offset: int = 0, camera=None,
                   accumulate: bool = False, **sky) -> RtGatherSurfaceParams:
    """rt_gather_surface_params: the path fields of ray_color_params."""
    g = RtGatherSurfaceParams()
    g.path = ray_color_params(samples, depth, seed, sample_offset, camera, accumulate, **sky)
    return g


class RtWorkCounts(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples", "rays", "shadow_rays", "node_visits", "sphere_tests",
                                          "quad_tests", "tri_tests", "plane_tests", "instance_visits",
                                          "volume_tests", "material_fetches", "env_lookups",
                                          "instance_box_tests", "stack_spills", "early_shadow_rays",
                                          "early_rays")]


class RtKernelTimes(C.Structure):
    _fields_ = [("extend_ms", C.c_double), ("shade_ms", C.c_double), ("shadow_ms", C.c_double),
                ("extend_launches", C.c_int32), ("shade_launches", C.c_int32), ("shadow_launches", C.c_int32),
                ("twins", C.c_int32)]


class RtSceneInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nodes", "leaves", "refs", "spheres", "quads", "triangles", "planes",
                                         "instances", "blases", "volumes", "materials", "textures", "lights",
                                         "stack_needed", "tlas_depth", "blas_depth")] + [("device_bytes", C.c_int64)] + \
        [("node_format", C.c_int32), ("nodes8", C.c_int32)]


class RtsSceneOptions(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("width", C.c_int32), ("aspect", C.c_double), ("spp", C.c_int32),
                ("max_depth", C.c_int32), ("asset_dir", C.c_char_p), ("obj_path", C.c_char_p),
                ("lucy_rings", C.c_int32), ("lucy_cols", C.c_int32), ("camera_motion", C.c_int32),
                ("look_from2", C.c_double * 3), ("look_at2", C.c_double * 3), ("free_camera", C.c_int32),
                ("forward", C.c_double * 3)]


_rtgpu = None
_rtscene = None


def _load(name: str) -> C.CDLL:
    path = os.path.join(LIB_DIR, name)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it first (python -c 'import __graft_entry__ as g; g.build()')")
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


def rtgpu() -> C.CDLL:
    """The C-ABI library (include/rtgpu.h)."""
    global _rtgpu
    if _rtgpu is None:
        lib = _load("librtgpu.so")
        P, I32, U32 = C.c_void_p, C.c_int32, C.c_uint32
        lib.rt_abi_version.restype = C.c_int
        lib.rt_ctx_create.argtypes = [C.c_int, C.POINTER(P)]
        # (A/B builds of older revisions, RTGPU_LIB_DIR, may lack the newer entry points)
        if hasattr(lib, "rt_ctx_create_multi"):
            lib.rt_ctx_create_multi.argtypes = [C.POINTER(I32), I32, C.POINTER(P)]
            lib.rt_ctx_num_devices.argtypes = [P]
            lib.rt_device_count.argtypes = [C.POINTER(I32)]
        if hasattr(lib, "rt_last_dealing"):
            lib.rt_last_dealing.argtypes = [P, C.POINTER(I32), C.POINTER(I32), I32]
        lib.rt_ctx_destroy.argtypes = [P]
        lib.rt_ctx_destroy.restype = None
        lib.rt_last_error.argtypes = [P]
        lib.rt_last_error.restype = C.c_char_p
        lib.rt_scene_upload.argtypes = [P, C.POINTER(RtSceneDesc)]
        lib.rt_scene_get_info.argtypes = [P, C.POINTER(RtSceneInfo)]
        lib.rt_last_build_ms.argtypes = [P, C.POINTER(C.c_double)]
        if hasattr(lib, "rt_scene_lifted_prims"):   # (an older build under RTGPU_LIB_DIR has none)
            lib.rt_scene_lifted_prims.argtypes = [P, C.POINTER(I32)]
        lib.rt_render.argtypes = [P, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams), C.POINTER(C.c_float),
                                  C.POINTER(RtStats)]
        lib.rt_render_device.argtypes = [P, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams), P, P]
        lib.rt_last_render_kernel_ms.argtypes = [P, C.POINTER(C.c_double)]
        lib.rt_sync.argtypes = [P]
        lib.rt_count_work.argtypes = [P, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams),
                                      C.POINTER(RtWorkCounts)]
        lib.rt_count_work_by_kernel.argtypes = [P, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams),
                                                C.POINTER(RtWorkCounts)]
        lib.rt_set_kernel_timing.argtypes = [P, C.c_int]
        if hasattr(lib, "rt_measure_read_bandwidth"):
            lib.rt_measure_read_bandwidth.argtypes = [P, C.c_uint64, I32, C.POINTER(C.c_double)]
        lib.rt_ctx_set_option.argtypes = [P, I32, I32]
        lib.rt_last_kernel_times.argtypes = [P, C.POINTER(RtKernelTimes)]
        lib.rt_tonemap_rgba8.argtypes = [P, C.POINTER(C.c_float), I32, I32, I32, C.POINTER(C.c_uint8)]
        lib.rt_primary_hits.argtypes = [P, C.POINTER(RtCameraDesc), U32, I32, C.POINTER(I32), C.POINTER(I32),
                                        C.POINTER(C.c_float)]
        if hasattr(lib, "rt_render_rgba8"):
            lib.rt_render_rgba8.argtypes = [P, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams),
                                            C.POINTER(C.c_uint8), C.POINTER(RtStats)]
            lib.rt_read_frame_sums.argtypes = [P, C.POINTER(C.c_float), C.c_int64]
        if hasattr(lib, "rt_extend_first_hits"):
            lib.rt_extend_first_hits.argtypes = [P, C.POINTER(RtCameraDesc), U32, I32, C.POINTER(I32),
                                                 C.POINTER(I32), C.POINTER(C.c_float)]
        if hasattr(lib, "rt_extend_hits"):
            lib.rt_extend_hits.argtypes = [P, C.POINTER(RtCameraDesc), U32, I32, I32, C.POINTER(I32), C.POINTER(I32),
                                           C.POINTER(C.c_float), C.POINTER(C.c_float)]
            lib.rt_shadow_visibility.argtypes = [P, C.POINTER(RtCameraDesc), U32, I32, I32, C.POINTER(I32)]
        if hasattr(lib, "rt_render_features"):
            lib.rt_render_features.argtypes = [P, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams),
                                               C.POINTER(C.c_float), C.POINTER(RtStats)]
            lib.rt_render_features_device.argtypes = [P, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams), P, P]
            lib.rt_denoise_default_params.argtypes = [C.POINTER(RtDenoiseParams)]
            lib.rt_denoise.argtypes = [P, C.POINTER(C.c_float), C.POINTER(C.c_float), I32, I32, I32,
                                       C.POINTER(RtDenoiseParams), C.POINTER(C.c_float)]
            lib.rt_denoise_device.argtypes = [P, P, P, I32, I32, I32, C.POINTER(RtDenoiseParams), P, P]
        if hasattr(lib, "rt_render_moments"):
            lib.rt_render_moments.argtypes = [P, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams),
                                              C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(RtStats)]
            lib.rt_render_moments_device.argtypes = [P, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams), P, P, P]
            lib.rt_denoise_variance_default_params.argtypes = [C.POINTER(RtDenoiseVarParams)]
            lib.rt_denoise_variance.argtypes = [P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                I32, I32, I32, C.POINTER(RtDenoiseVarParams), C.POINTER(C.c_float),
                                                C.POINTER(C.c_float)]
            lib.rt_denoise_variance_device.argtypes = [P, P, P, P, I32, I32, I32, C.POINTER(RtDenoiseVarParams), P, P,
                                                       P]
        if hasattr(lib, "rt_render_adaptive"):
            U32P = C.POINTER(U32)
            lib.rt_adaptive_default_params.argtypes = [C.POINTER(RtAdaptiveParams)]
            lib.rt_render_adaptive.argtypes = [P, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams),
                                               C.POINTER(RtAdaptiveParams), C.POINTER(C.c_float),
                                               C.POINTER(C.c_float), U32P, C.POINTER(RtAdaptiveStats)]
            lib.rt_render_adaptive_device.argtypes = [P, C.POINTER(RtCameraDesc), C.POINTER(RtRenderParams),
                                                      C.POINTER(RtAdaptiveParams), P, P, P,
                                                      C.POINTER(RtAdaptiveStats), P]
            lib.rt_adaptive_select.argtypes = [P, C.POINTER(C.c_float), U32P, I32, I32, I32,
                                               C.POINTER(RtAdaptiveParams), U32P, U32P]
            lib.rt_normalize_samples.argtypes = [P, C.POINTER(C.c_float), I32, U32P, I32, I32, I32,
                                                 C.POINTER(C.c_float)]
            lib.rt_normalize_samples_device.argtypes = [P, P, I32, P, I32, I32, I32, P, P]
        if hasattr(lib, "rt_trace_rays"):
            lib.rt_trace_rays.argtypes = [P, C.POINTER(RtRay), C.c_int64, C.c_float, C.POINTER(RtRayHit)]
            lib.rt_trace_rays_device.argtypes = [P, P, C.c_int64, C.c_float, P, P]
            lib.rt_occluded.argtypes = [P, C.POINTER(RtRay), C.c_int64, C.c_float, C.POINTER(C.c_uint8)]
            lib.rt_occluded_device.argtypes = [P, P, C.c_int64, C.c_float, P, P]
        if hasattr(lib, "rt_ray_color"):
            lib.rt_ray_color.argtypes = [P, C.POINTER(RtPathRay), C.c_int64, C.POINTER(RtRayColorParams),
                                         C.POINTER(C.c_float), C.POINTER(RtRayColorStats)]
            lib.rt_ray_color_device.argtypes = [P, P, C.c_int64, C.POINTER(RtRayColorParams), P, P]
        if hasattr(lib, "rt_gather"):
            lib.rt_gather.argtypes = [P, C.POINTER(RtGatherPoint), C.c_int64, C.POINTER(RtGatherParams),
                                      C.POINTER(C.c_float), C.POINTER(RtRayColorStats)]
            lib.rt_gather_device.argtypes = [P, P, C.c_int64, C.POINTER(RtGatherParams), P, P]
            lib.rt_gather_rays.argtypes = [P, C.POINTER(RtGatherPoint), C.c_int64, I32, U32, I32, C.POINTER(RtPathRay)]
        if hasattr(lib, "rt_gather_sh"):
            lib.rt_gather_sh.argtypes = [P, C.POINTER(RtGatherPoint), C.c_int64, C.POINTER(RtGatherShParams),
                                         C.POINTER(C.c_float), C.POINTER(RtRayColorStats)]
            lib.rt_gather_sh_device.argtypes = [P, P, C.c_int64, C.POINTER(RtGatherShParams), P, P]
        if hasattr(lib, "rt_gather_surface"):
            lib.rt_gather_surface.argtypes = [P, C.POINTER(RtGatherPoint), C.c_int64, C.POINTER(RtGatherSurfaceParams),
                                              C.POINTER(C.c_float), C.POINTER(RtRayColorStats)]
            lib.rt_gather_surface_device.argtypes = [P, P, C.c_int64, C.POINTER(RtGatherSurfaceParams), P, P]
        _rtgpu = lib
    return _rtgpu


def rtscene() -> C.CDLL:
    """The host rt mirror (include/rtscene.h)."""
    global _rtscene
    if _rtscene is None:
        rtgpu()
        lib = _load("librtscene.so")
        P, I32 = C.c_void_p, C.c_int32
        lib.rts_scene_create.argtypes = [C.c_char_p, C.POINTER(RtsSceneOptions), C.POINTER(P), C.c_char_p, I32]
        lib.rts_scene_destroy.argtypes = [P]
        lib.rts_scene_destroy.restype = None
        lib.rts_scene_get_desc.argtypes = [P]
        lib.rts_scene_get_desc.restype = C.POINTER(RtSceneDesc)
        lib.rts_scene_get_camera.argtypes = [P]
        lib.rts_scene_get_camera.restype = C.POINTER(RtCameraDesc)
        lib.rts_scene_world_objects.argtypes = [P, C.POINTER(I32), I32]
        lib.rts_scene_world_objects.restype = I32
        lib.rts_renderer_create.argtypes = [P, I32, I32, I32, C.c_uint32, C.POINTER(P), C.c_char_p, I32]
        lib.rts_renderer_destroy.argtypes = [P]
        lib.rts_renderer_destroy.restype = None
        lib.rts_renderer_render_pass.argtypes = [P, I32]
        lib.rts_renderer_render_all.argtypes = [P]
        lib.rts_renderer_is_completed.argtypes = [P]
        lib.rts_renderer_framebuffer.argtypes = [P]
        lib.rts_renderer_framebuffer.restype = C.POINTER(C.c_uint8)
        lib.rts_renderer_accum.argtypes = [P]
        lib.rts_renderer_accum.restype = C.POINTER(C.c_float)
        lib.rts_renderer_duration_ms.argtypes = [P]
        lib.rts_renderer_duration_ms.restype = C.c_double
        lib.rts_renderer_save_png.argtypes = [P, C.c_char_p]
        lib.rts_renderer_last_error.argtypes = [P]
        lib.rts_renderer_last_error.restype = C.c_char_p
        if hasattr(lib, "rts_renderer_timings"):
            lib.rts_renderer_timings.argtypes = [P, C.POINTER(C.c_double)]
        lib.rts_load_hdr.argtypes = [C.c_char_p, C.POINTER(I32), C.POINTER(I32), C.POINTER(C.c_double), C.c_int64]
        lib.rts_write_synthetic_lucy_obj.argtypes = [C.c_char_p, I32, I32]
        lib.rts_obj_triangle_count.argtypes = [C.c_char_p]
        lib.rts_write_png.argtypes = [C.c_char_p, C.POINTER(C.c_uint8), I32, I32]
        _rtscene = lib
    return _rtscene


class RTError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


def _f32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _u32p(a: np.ndarray):
    if a.dtype != np.uint32 or not a.flags["C_CONTIGUOUS"]:
        raise TypeError("a contiguous uint32 array is needed")
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


# ---------------------------------------------------------------------------
# Scenes (scenes.go builders, via librtscene)
# ---------------------------------------------------------------------------
class Scene:
    """A BASELINE scene built by the host rt mirror; world wrapped in
    NewBVHNodeFromList like main.go:77."""

    def __init__(self, name: str, *, seed: int = 0x5EED, width: int = 0, aspect: float = 0.0, spp: int = 0,
                 max_depth: int = 0, asset_dir: Optional[str] = None, obj_path: Optional[str] = None,
                 lucy_rings: int = 0, lucy_cols: int = 0, motion: Optional[Sequence[Sequence[float]]] = None,
                 free_forward: Optional[Sequence[float]] = None):
        """`motion=(look_from2, look_at2)` applies Camera.SetMotion and
        `free_forward=(x, y, z)` Camera.EnableFreeCamera(LookFrom, forward,
        Vup) to the scene's camera before Build() (camera.go:204-232)."""
        lib = rtscene()
        self.name = name
        opt = RtsSceneOptions(seed, width, aspect, spp, max_depth, (asset_dir or ASSET_DIR).encode(),
                              obj_path.encode() if obj_path else None, lucy_rings, lucy_cols)
        if motion is not None:
            opt.camera_motion = 1
            opt.look_from2[:] = [float(x) for x in motion[0]]
            opt.look_at2[:] = [float(x) for x in motion[1]]
        if free_forward is not None:
            opt.free_camera = 1
            opt.forward[:] = [float(x) for x in free_forward]
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = lib.rts_scene_create(name.encode(), C.byref(opt), C.byref(h), err, 512)
        if rc != RT_OK:
            raise RTError(rc, err.value.decode())
        self._h = h
        self._lib = lib

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.rts_scene_destroy(self._h)
            self._h = None

    @property
    def desc(self):
        return self._lib.rts_scene_get_desc(self._h)

    @property
    def camera(self) -> RtCameraDesc:
        return self._lib.rts_scene_get_camera(self._h).contents

    @property
    def width(self) -> int:
        return self.camera.image_width

    @property
    def height(self) -> int:
        return self.camera.image_height

    def world_objects(self) -> np.ndarray:
        n = self._lib.rts_scene_world_objects(self._h, None, 0)
        out = np.zeros(max(n, 1), np.int32)
        self._lib.rts_scene_world_objects(self._h, _i32p(out), n)
        return out[:n]

    def hittables(self) -> np.ndarray:
        d = self.desc.contents
        return np.ctypeslib.as_array(C.cast(d.hittables, C.POINTER(C.c_byte)),
                                     shape=(d.num_hittables * C.sizeof(RtHittable),)).view(
            np.dtype([("kind", "<i4"), ("material", "<i4"), ("a", "<i4"), ("b", "<i4"), ("bbox", "<f8", 6),
                      ("p", "<f8", 16)])).copy()

    def children(self) -> np.ndarray:
        d = self.desc.contents
        if d.num_children == 0:
            return np.zeros(0, np.int32)
        return np.ctypeslib.as_array(d.children, shape=(d.num_children,)).copy()


def buckets_array(buckets: Sequence[Sequence[int]]):
    arr = (RtBucket * max(len(buckets), 1))()
    for i, b in enumerate(buckets):
        arr[i] = RtBucket(*[int(v) for v in b])
    return arr


def generate_buckets(width: int, height: int, bucket_size: int = 32):
    """rt.generateBuckets (bucket_renderer.go:77-125): centre-out order (stable)."""
    bs = []
    for y in range(0, height, bucket_size):
        for x in range(0, width, bucket_size):
            bs.append((x, y, min(bucket_size, width - x), min(bucket_size, height - y)))
    cx, cy = width // 2, height // 2
    bs.sort(key=lambda b: (b[0] + b[2] // 2 - cx) ** 2 + (b[1] + b[3] // 2 - cy) ** 2)
    return bs


def split_buckets(buckets, tile: int = 16):
    """Each bucket cut into tile x tile sub-buckets, in bucket order (the
    kernels' own work tiles are 16x16, api.cpp make_tiles)."""
    out = []
    for x, y, w, h in buckets:
        for ty in range(y, y + h, tile):
            for tx in range(x, x + w, tile):
                out.append((tx, ty, min(tile, x + w - tx), min(tile, y + h - ty)))
    return out


def shard_buckets(buckets, rank: int, world: int, tile: int = 0):
    """Round-robin tile sharding across ranks (bucket k -> rank k mod world):
    the centre-heavy cost of the centre-out bucket order is spread evenly
    (SURVEY.md §8(e)).  tile > 0 deals tile x tile sub-buckets instead (finer
    grain, better balance).  The RNG is keyed by global pixel id, so the
    combined frame is identical for any world size and grain."""
    if tile:
        buckets = split_buckets(buckets, tile)
    return [b for i, b in enumerate(buckets) if i % world == rank]


def make_params(spp: int, depth: int, seed: int = 1, sample_offset: int = 0, buckets=None, accumulate: bool = False):
    keep = None
    if buckets is not None:
        keep = buckets_array(buckets)
        p = RtRenderParams(spp, depth, sample_offset, seed, C.cast(keep, C.POINTER(RtBucket)), len(buckets),
                           1 if accumulate else 0)
    else:
        p = RtRenderParams(spp, depth, sample_offset, seed, None, 0, 1 if accumulate else 0)
    p._keep = keep
    return p


def denoise_params(**overrides) -> RtDenoiseParams:
    """rt_denoise_default_params with keyword overrides (iterations,
    normal_power_log2, demodulate, sigma_color, sigma_depth, albedo_eps)."""
    dp = RtDenoiseParams()
    rc = rtgpu().rt_denoise_default_params(C.byref(dp))
    if rc != RT_OK:
        raise RTError(rc, "rt_denoise_default_params failed")
    for k, v in overrides.items():
        if k not in dict(RtDenoiseParams._fields_):
            raise TypeError(f"unknown denoise parameter {k!r}")
        setattr(dp, k, v)
    return dp


def denoise_variance_params(**overrides) -> RtDenoiseVarParams:
    """rt_denoise_variance_default_params with keyword overrides (iterations,
    normal_power_log2, demodulate, spatial_below, sigma_lum, sigma_depth,
    albedo_eps)."""
    dp = RtDenoiseVarParams()
    rc = rtgpu().rt_denoise_variance_default_params(C.byref(dp))
    if rc != RT_OK:
        raise RTError(rc, "rt_denoise_variance_default_params failed")
    for k, v in overrides.items():
        if k not in dict(RtDenoiseVarParams._fields_):
            raise TypeError(f"unknown denoise parameter {k!r}")
        setattr(dp, k, v)
    return dp


def adaptive_params(**overrides) -> RtAdaptiveParams:
    """rt_adaptive_default_params with keyword overrides (min_spp, step_spp,
    neighbourhood, rel_error, lum_floor)."""
    ap = RtAdaptiveParams()
    rc = rtgpu().rt_adaptive_default_params(C.byref(ap))
    if rc != RT_OK:
        raise RTError(rc, "rt_adaptive_default_params failed")
    for k, v in overrides.items():
        if k not in dict(RtAdaptiveParams._fields_):
            raise TypeError(f"unknown adaptive parameter {k!r}")
        setattr(ap, k, v)
    return ap


# ---------------------------------------------------------------------------
# GPU context (rt_ctx)
# ---------------------------------------------------------------------------
def device_count() -> int:
    """Visible HIP devices (rt_device_count)."""
    n = C.c_int32()
    rc = rtgpu().rt_device_count(C.byref(n))
    if rc != RT_OK:
        raise RTError(rc, "rt_device_count failed (no GPU?)")
    return n.value


class Context:
    """One device's flattened scene + render entry points (rtgpu.h).  With
    `devices=[d0, d1, ...]` one context over several devices
    (rt_ctx_create_multi): renders deal the buckets round-robin over them."""

    def __init__(self, device: int = 0, devices: Optional[Sequence[int]] = None):
        self._lib = rtgpu()
        h = C.c_void_p()
        if devices is not None and len(devices) > 0:
            arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            rc = self._lib.rt_ctx_create_multi(arr, len(devices), C.byref(h))
            if rc != RT_OK:
                raise RTError(rc, f"rt_ctx_create_multi(devices={list(devices)}) failed")
            device = int(devices[0])
        else:
            rc = self._lib.rt_ctx_create(device, C.byref(h))
            if rc != RT_OK:
                raise RTError(rc, f"rt_ctx_create(device={device}) failed (no GPU?)")
        self._h = h
        self.device = device

    @property
    def num_devices(self) -> int:
        return int(self._lib.rt_ctx_num_devices(self._h))

    def set_dealing(self, mode: str = "static", first_share: int = 0):
        """Multi-device tile dealing (RT_OPT_DEALING): "static" (tile k to
        device k mod n) or "dynamic" (runs claimed from a shared counter as
        devices finish, bucket_renderer.go:193-213); first_share = the first
        run in percent of a fair share (0: default)."""
        self.set_option(RT_OPT_DEALING, {"static": RT_DEAL_STATIC, "dynamic": RT_DEAL_DYNAMIC}[mode])
        self.set_option(RT_OPT_DEAL_FIRST, first_share)

    def last_dealing(self):
        """(tiles, runs) per device of the last multi-device render."""
        n = self.num_devices
        tiles, runs = (C.c_int32 * n)(), (C.c_int32 * n)()
        self._check(self._lib.rt_last_dealing(self._h, tiles, runs, n))
        return list(tiles), list(runs)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rt_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _check(self, rc: int):
        if rc != RT_OK:
            raise RTError(rc, self._lib.rt_last_error(self._h).decode())

    def upload(self, scene_desc) -> None:
        self._check(self._lib.rt_scene_upload(self._h, scene_desc))

    def info(self) -> RtSceneInfo:
        i = RtSceneInfo()
        self._check(self._lib.rt_scene_get_info(self._h, C.byref(i)))
        return i

    def render(self, camera: RtCameraDesc, params: RtRenderParams, accum: Optional[np.ndarray] = None):
        if accum is None:
            accum = np.zeros((camera.image_height, camera.image_width, 3), np.float32)
        st = RtStats()
        self._check(self._lib.rt_render(self._h, C.byref(camera), C.byref(params), _f32p(accum), C.byref(st)))
        return accum, st

    def render_rgba8(self, camera: RtCameraDesc, params: RtRenderParams):
        """One progressive pass (rt_render_rgba8): render + device quantisation;
        returns the (H, W, 4) RGBA8 framebuffer and the stats."""
        out = np.zeros((camera.image_height, camera.image_width, 4), np.uint8)
        st = RtStats()
        self._check(self._lib.rt_render_rgba8(self._h, C.byref(camera), C.byref(params),
                                              out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(st)))
        return out, st

    def frame_sums(self, camera: RtCameraDesc) -> np.ndarray:
        """The device frame sums behind render_rgba8's framebuffer."""
        out = np.zeros((camera.image_height, camera.image_width, 3), np.float32)
        self._check(self._lib.rt_read_frame_sums(self._h, _f32p(out), out.size))
        return out

    def render_device(self, camera: RtCameraDesc, params: RtRenderParams, dev_ptr: int, stream: int = 0):
        self._check(self._lib.rt_render_device(self._h, C.byref(camera), C.byref(params), C.c_void_p(dev_ptr),
                                               C.c_void_p(stream)))

    def render_features(self, camera: RtCameraDesc, params: RtRenderParams, feat: Optional[np.ndarray] = None):
        """Feature buffers (rt_render_features): (H, W, 8) float32 sums over the
        call's samples of albedo.rgb, normal.xyz, depth, coverage at the camera
        rays' closest hits (the same path keys as render()), and the stats."""
        if feat is None:
            feat = np.zeros((camera.image_height, camera.image_width, 8), np.float32)
        st = RtStats()
        self._check(self._lib.rt_render_features(self._h, C.byref(camera), C.byref(params), _f32p(feat),
                                                 C.byref(st)))
        return feat, st

    def render_features_device(self, camera: RtCameraDesc, params: RtRenderParams, dev_ptr: int, stream: int = 0):
        self._check(self._lib.rt_render_features_device(self._h, C.byref(camera), C.byref(params),
                                                        C.c_void_p(dev_ptr), C.c_void_p(stream)))

    def denoise(self, accum: np.ndarray, feat: np.ndarray, spp: int, **params) -> np.ndarray:
        """rt_denoise: the a-trous filter over (H, W, 3) radiance sums guided by
        the (H, W, 8) feature sums of the same `spp` samples; returns filtered
        sums.  Keyword arguments override denoise_params()'s defaults."""
        h, w = accum.shape[:2]
        out = np.zeros((h, w, 3), np.float32)
        dp = denoise_params(**params)
        self._check(self._lib.rt_denoise(self._h, _f32p(accum), _f32p(feat), w, h, spp, C.byref(dp), _f32p(out)))
        return out

    def denoise_device(self, accum_ptr: int, feat_ptr: int, width: int, height: int, spp: int, out_ptr: int,
                       stream: int = 0, **params):
        """rt_denoise_device: the same over device arrays, asynchronous on `stream`."""
        dp = denoise_params(**params)
        self._check(self._lib.rt_denoise_device(self._h, C.c_void_p(accum_ptr), C.c_void_p(feat_ptr), width, height,
                                                spp, C.byref(dp), C.c_void_p(out_ptr), C.c_void_p(stream)))

    def render_moments(self, camera: RtCameraDesc, params: RtRenderParams, accum: Optional[np.ndarray] = None,
                       moments: Optional[np.ndarray] = None):
        """rt_render_moments: render()'s frame (the same bits) and the (H, W, 2)
        float32 luminance moments (sum Y, sum Y^2) of the same samples; returns
        (accum, moments, stats).  Both arrays accumulate with params.accumulate."""
        if accum is None:
            accum = np.zeros((camera.image_height, camera.image_width, 3), np.float32)
        if moments is None:
            moments = np.zeros((camera.image_height, camera.image_width, 2), np.float32)
        st = RtStats()
        self._check(self._lib.rt_render_moments(self._h, C.byref(camera), C.byref(params), _f32p(accum),
                                                _f32p(moments), C.byref(st)))
        return accum, moments, st

    def render_moments_device(self, camera: RtCameraDesc, params: RtRenderParams, dev_ptr: int, moments_ptr: int,
                              stream: int = 0):
        self._check(self._lib.rt_render_moments_device(self._h, C.byref(camera), C.byref(params), C.c_void_p(dev_ptr),
                                                       C.c_void_p(moments_ptr), C.c_void_p(stream)))

    def denoise_variance(self, accum: np.ndarray, feat: np.ndarray, moments: Optional[np.ndarray], spp: int,
                         return_variance: bool = False, **params):
        """rt_denoise_variance: the variance-guided a-trous filter over (H, W, 3)
        radiance sums, guided by the (H, W, 8) feature sums and the (H, W, 2)
        moments of the same `spp` samples (moments may be None below
        spatial_below samples); returns the filtered sums, with
        return_variance also the (H, W) final variance.  Keyword arguments
        override denoise_variance_params()'s defaults."""
        h, w = accum.shape[:2]
        out = np.zeros((h, w, 3), np.float32)
        var = np.zeros((h, w), np.float32) if return_variance else None
        dp = denoise_variance_params(**params)
        self._check(self._lib.rt_denoise_variance(self._h, _f32p(accum), _f32p(feat),
                                                  None if moments is None else _f32p(moments), w, h, spp,
                                                  C.byref(dp), _f32p(out), None if var is None else _f32p(var)))
        return (out, var) if return_variance else out

    def denoise_variance_device(self, accum_ptr: int, feat_ptr: int, moments_ptr: int, width: int, height: int,
                                spp: int, out_ptr: int, var_ptr: int = 0, stream: int = 0, **params):
        """rt_denoise_variance_device: the same over device arrays (0 = NULL for
        moments_ptr / var_ptr), asynchronous on `stream`."""
        dp = denoise_variance_params(**params)
        self._check(self._lib.rt_denoise_variance_device(self._h, C.c_void_p(accum_ptr), C.c_void_p(feat_ptr),
                                                         C.c_void_p(moments_ptr or None), width, height, spp,
                                                         C.byref(dp), C.c_void_p(out_ptr), C.c_void_p(var_ptr or None),
                                                         C.c_void_p(stream)))

    def render_adaptive(self, camera: RtCameraDesc, params: RtRenderParams, accum: Optional[np.ndarray] = None,
                        moments: Optional[np.ndarray] = None, counts: Optional[np.ndarray] = None, **adaptive):
        """rt_render_adaptive: params.samples_per_pixel is the budget max_spp; a
        pixel stops being sampled once its luminance's standard error is small
        enough.  Returns (accum, moments, counts, stats): the (H, W, 3) sums and
        (H, W, 2) moments of each pixel's first counts[p] samples and the
        (H, W) uint32 counts.  Keyword arguments override adaptive_params()'s
        defaults.  Blocks."""
        h, w = camera.image_height, camera.image_width
        if accum is None:
            accum = np.zeros((h, w, 3), np.float32)
        if moments is None:
            moments = np.zeros((h, w, 2), np.float32)
        if counts is None:
            counts = np.zeros((h, w), np.uint32)
        ap = adaptive_params(**adaptive)
        st = RtAdaptiveStats()
        self._check(self._lib.rt_render_adaptive(self._h, C.byref(camera), C.byref(params), C.byref(ap),
                                                 _f32p(accum), _f32p(moments), _u32p(counts), C.byref(st)))
        return accum, moments, counts, st

    def render_adaptive_device(self, camera: RtCameraDesc, params: RtRenderParams, dev_ptr: int, moments_ptr: int,
                               counts_ptr: int, stream: int = 0, **adaptive) -> RtAdaptiveStats:
        """rt_render_adaptive_device: the same into device arrays (counts: 4-byte
        unsigned words); blocks, like the host variant."""
        ap = adaptive_params(**adaptive)
        st = RtAdaptiveStats()
        self._check(self._lib.rt_render_adaptive_device(self._h, C.byref(camera), C.byref(params), C.byref(ap),
                                                        C.c_void_p(dev_ptr), C.c_void_p(moments_ptr),
                                                        C.c_void_p(counts_ptr), C.byref(st), C.c_void_p(stream)))
        return st

    def adaptive_select(self, moments: np.ndarray, counts: np.ndarray, max_spp: int, **adaptive) -> np.ndarray:
        """rt_adaptive_select: the ascending ids of the pixels of (H, W, 2)
        moments / (H, W) uint32 counts that stay active (counts 0: not in the
        call, >= max_spp: done)."""
        h, w = counts.shape
        ap = adaptive_params(**adaptive)
        out = np.zeros(h * w, np.uint32)
        n = C.c_uint32(0)
        self._check(self._lib.rt_adaptive_select(self._h, _f32p(moments), _u32p(counts), w, h, max_spp, C.byref(ap),
                                                 _u32p(out), C.byref(n)))
        return out[:n.value].copy()

    def normalize_samples(self, sums: np.ndarray, counts: np.ndarray, target_spp: int,
                          out: Optional[np.ndarray] = None) -> np.ndarray:
        """rt_normalize_samples: (H, W, C) sums over counts[p] samples each to
        sums over target_spp samples, (sums / counts) * target_spp; `out` may
        be `sums`."""
        h, w = counts.shape
        channels = sums.size // (h * w)
        if out is None:
            out = np.zeros(sums.shape, np.float32)
        self._check(self._lib.rt_normalize_samples(self._h, _f32p(sums), channels, _u32p(counts), w, h, target_spp,
                                                   _f32p(out)))
        return out

    def normalize_samples_device(self, sums_ptr: int, channels: int, counts_ptr: int, width: int, height: int,
                                 target_spp: int, out_ptr: int, stream: int = 0):
        """rt_normalize_samples_device: the same over device arrays, asynchronous on `stream`."""
        self._check(self._lib.rt_normalize_samples_device(self._h, C.c_void_p(sums_ptr), channels,
                                                          C.c_void_p(counts_ptr), width, height, target_spp,
                                                          C.c_void_p(out_ptr), C.c_void_p(stream)))

    def sync(self) -> None:
        """Wait for every enqueued render; raises RTError(RT_ERR_DEVICE) on a device error."""
        self._check(self._lib.rt_sync(self._h))

    def last_render_kernel_ms(self) -> float:
        ms = C.c_double()
        self._check(self._lib.rt_last_render_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def count_work(self, camera: RtCameraDesc, params: RtRenderParams) -> dict:
        w = RtWorkCounts()
        self._check(self._lib.rt_count_work(self._h, C.byref(camera), C.byref(params), C.byref(w)))
        return {n: int(getattr(w, n)) for n, _ in RtWorkCounts._fields_}

    def count_work_by_kernel(self, camera: RtCameraDesc, params: RtRenderParams) -> dict:
        """{"extend": counts, "shade": counts, "shadow": counts} (rt_count_work_by_kernel)."""
        w = (RtWorkCounts * 3)()
        self._check(self._lib.rt_count_work_by_kernel(self._h, C.byref(camera), C.byref(params), w))
        return {k: {n: int(getattr(w[i], n)) for n, _ in RtWorkCounts._fields_}
                for i, k in enumerate(("extend", "shade", "shadow"))}

    def set_option(self, key: int, value: int):
        self._check(self._lib.rt_ctx_set_option(self._h, key, value))

    def set_blas_builder(self, builder: str):
        """Mesh BLAS layout, next upload: "sah" (default, host binned SAH), "reference" (the
        caller's BVH topology) or "device" (LBVH built on the GPU, build.hip)."""
        self.set_option(RT_OPT_BLAS_BUILDER,
                        {"reference": RT_BLAS_REFERENCE, "sah": RT_BLAS_SAH, "device": RT_BLAS_DEVICE}[builder])

    def last_build_ms(self) -> float:
        """Wall time of the device BVH builds of the last upload (0 for host-built BLASes)."""
        ms = C.c_double()
        self._check(self._lib.rt_last_build_ms(self._h, C.byref(ms)))
        return ms.value

    def set_lift_prims(self, lifted: bool):
        """World quads / spheres tested by the shading kernel (default) or inside the traversal
        (RT_OPT_LIFT_PRIMS); next upload.  Same frames either way."""
        self.set_option(RT_OPT_LIFT_PRIMS, RT_PRIMS_LIFTED if lifted else RT_PRIMS_IN_BVH)

    def lifted_prims(self) -> int:
        """World quads / spheres the uploaded scene keeps out of its world BVH (0: none lifted)."""
        n = C.c_int32()
        self._check(self._lib.rt_scene_lifted_prims(self._h, C.byref(n)))
        return n.value

    def set_tlas_builder(self, builder: str):
        """World BVH layout: "sah" (default) or "reference"; next upload."""
        self.set_option(RT_OPT_TLAS_BUILDER, {"reference": RT_BLAS_REFERENCE, "sah": RT_BLAS_SAH}[builder])

    def set_node_format(self, fmt: str):
        """BVH4 node records: "fp32" (default, 128 B) or "quant8" (64 B,
        8-bit child planes with a conservative margin); next upload."""
        self.set_option(RT_OPT_NODE_FORMAT, {"fp32": RT_NODES_FP32, "quant8": RT_NODES_QUANT8, "wide8": RT_NODES_WIDE8}[fmt])

    def set_collapse(self, collapse: str):
        """BVH2 -> BVH4 collapse: "sah" (default, least total node area) or
        "greedy" (largest-area child first); same hits; next upload."""
        self.set_option(RT_OPT_BVH4_COLLAPSE, {"sah": RT_COLLAPSE_SAH, "greedy": RT_COLLAPSE_GREEDY}[collapse])

    def set_schedule(self, batch_slots: int = 0, refill: int = 0, max_blocks: int = 0, streams: int = 0):
        """Schedule options (0 = automatic) for the next renders: path slots per
        batch, idle lanes before a wave claims more rays, cap on the persistent
        traversal grids, one or two twin streams.  They never change the image
        (DESIGN.md §3)."""
        self.set_option(RT_OPT_BATCH_SLOTS, batch_slots)
        self.set_option(RT_OPT_REFILL, refill)
        self.set_option(RT_OPT_MAX_BLOCKS, max_blocks)
        self.set_option(RT_OPT_STREAMS, streams)

    def set_tail(self, paths: int = 0):
        """RT_OPT_TAIL for the next renders: 0 automatic, 1 off (every bounce
        through the per-bounce kernels), n > 1 = hand the paths left to the
        long-tail kernel once at most n remain (deep scenes without lights).
        Never changes the image."""
        self.set_option(RT_OPT_TAIL, paths)

    def set_overlap(self, mode: int = 0):
        """RT_OPT_OVERLAP for the next renders: 0 automatic (off), 1 off, 2 on
        (scenes with lights).  Bounce b's shadow rays and NEE adds run beside
        bounce b + 1's closest-hit kernel on a second stream per part.  Never
        changes the image."""
        self.set_option(RT_OPT_OVERLAP, mode)

    def set_early_miss(self, mode: int = 0):
        """RT_OPT_EARLY_MISS for the next renders: 0 automatic (on where it
        applies), 1 off, 2 on.  The shade kernel resolves the rays that miss
        the world BVH's box itself: an NEE job whose shadow rays all miss it is
        applied in place, a path whose scattered ray misses it skips the
        closest-hit kernel's queue.  Never changes the image."""
        self.set_option(RT_OPT_EARLY_MISS, mode)

    def measure_read_bandwidth(self, nbytes: int = 4 << 30, reps: int = 10) -> float:
        """The measured HBM read peak (GB/s): `reps` coalesced passes over a
        fresh `nbytes` device buffer (rt_measure_read_bandwidth)."""
        gbs = C.c_double(0.0)
        self._check(self._lib.rt_measure_read_bandwidth(self._h, C.c_uint64(nbytes), reps, C.byref(gbs)))
        return float(gbs.value)

    def set_kernel_timing(self, enable: bool = True):
        self._check(self._lib.rt_set_kernel_timing(self._h, 1 if enable else 0))

    def last_kernel_times(self) -> dict:
        t = RtKernelTimes()
        self._check(self._lib.rt_last_kernel_times(self._h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in RtKernelTimes._fields_}

    def tonemap(self, accum: np.ndarray, spp: int) -> np.ndarray:
        h, w = accum.shape[:2]
        a = np.ascontiguousarray(accum, np.float32)
        out = np.zeros((h, w, 4), np.uint8)
        self._check(self._lib.rt_tonemap_rgba8(self._h, _f32p(a), w, h, spp,
                                               out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def primary_hits(self, camera: RtCameraDesc, seed: int, sample: int = 0):
        n = camera.image_width * camera.image_height
        top = np.zeros(n, np.int32)
        prim = np.zeros(n, np.int32)
        t = np.zeros(n, np.float32)
        self._check(self._lib.rt_primary_hits(self._h, C.byref(camera), seed, sample, _i32p(top), _i32p(prim),
                                              _f32p(t)))
        return top, prim, t

    def extend_first_hits(self, camera: RtCameraDesc, seed: int, sample: int = 0):
        """primary_hits' ids from the production pipeline's first k_extend."""
        n = camera.image_width * camera.image_height
        top = np.zeros(n, np.int32)
        prim = np.zeros(n, np.int32)
        t = np.zeros(n, np.float32)
        self._check(self._lib.rt_extend_first_hits(self._h, C.byref(camera), seed, sample, _i32p(top), _i32p(prim),
                                                   _f32p(t)))
        return top, prim, t

    def extend_hits(self, camera: RtCameraDesc, seed: int, sample: int, bounce: int):
        """Closest hit of every pixel's bounce-`bounce` ray from the production
        k_extend (rt_extend_hits): top, prim (-1 miss, -2 path ended), t, and
        the incoming ray (n, 6) float32 (origin, direction)."""
        n = camera.image_width * camera.image_height
        top = np.zeros(n, np.int32)
        prim = np.zeros(n, np.int32)
        t = np.zeros(n, np.float32)
        ray = np.zeros((n, 6), np.float32)
        self._check(self._lib.rt_extend_hits(self._h, C.byref(camera), seed, sample, bounce, _i32p(top), _i32p(prim),
                                             _f32p(t), _f32p(ray)))
        return top, prim, t, ray

    def shadow_visibility(self, camera: RtCameraDesc, seed: int, sample: int, bounce: int) -> np.ndarray:
        """NEE shadow rays of bounce `bounce` per pixel (rt_shadow_visibility):
        bits 0/1 area/HDRI ray traced, bits 2/3 unoccluded."""
        n = camera.image_width * camera.image_height
        nee = np.zeros(n, np.int32)
        self._check(self._lib.rt_shadow_visibility(self._h, C.byref(camera), seed, sample, bounce, _i32p(nee)))
        return nee

    # ---- ray queries (rt_trace_rays / rt_occluded)
    def trace_rays_raw(self, rays: np.ndarray, time: float = 0.0) -> np.ndarray:
        """rt_trace_rays over an array of rt_ray (RAY_DTYPE): the rt_ray_hit
        records (RAY_HIT_DTYPE)."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        hits = np.zeros(rays.shape[0], RAY_HIT_DTYPE)
        self._check(self._lib.rt_trace_rays(self._h, rays.ctypes.data_as(C.POINTER(RtRay)), rays.shape[0], time,
                                            hits.ctypes.data_as(C.POINTER(RtRayHit))))
        return hits

    def trace_rays(self, o, d, tmin=0.001, tmax=float("inf"), time: float = 0.0):
        """Closest hit of every ray o + t d over (tmin, tmax) in the uploaded
        scene (rt_trace_rays): (top, prim, t, material, n, flags); a miss has
        ids -1, t -1, n 0; flags: RT_HIT_FRONT, RT_HIT_INVALID_RAY."""
        h = self.trace_rays_raw(make_rays(o, d, tmin, tmax), time)
        return (h["top"].copy(), h["prim"].copy(), h["t"].copy(), h["material"].copy(), h["n"].copy(),
                h["flags"].copy())

    def occluded(self, o, d, tmin=0.001, tmax=float("inf"), time: float = 0.0) -> np.ndarray:
        """1 where anything is hit in the interval, else 0 (rt_occluded, the
        shadow rays' any-hit rule)."""
        rays = make_rays(o, d, tmin, tmax)
        occ = np.zeros(rays.shape[0], np.uint8)
        self._check(self._lib.rt_occluded(self._h, rays.ctypes.data_as(C.POINTER(RtRay)), rays.shape[0], time,
                                          occ.ctypes.data_as(C.POINTER(C.c_uint8))))
        return occ

    def trace_rays_device(self, rays_ptr: int, n: int, hits_ptr: int, time: float = 0.0, stream: int = 0):
        """rt_trace_rays_device: n rt_ray at device address rays_ptr -> n
        rt_ray_hit at hits_ptr, asynchronous on `stream`."""
        self._check(self._lib.rt_trace_rays_device(self._h, C.c_void_p(rays_ptr), n, time, C.c_void_p(hits_ptr),
                                                   C.c_void_p(stream)))

    def occluded_device(self, rays_ptr: int, n: int, occluded_ptr: int, time: float = 0.0, stream: int = 0):
        """rt_occluded_device: n rt_ray at rays_ptr -> n bytes at occluded_ptr."""
        self._check(self._lib.rt_occluded_device(self._h, C.c_void_p(rays_ptr), n, time, C.c_void_p(occluded_ptr),
                                                 C.c_void_p(stream)))

    # ---- Camera.RayColor for the caller's rays (rt_ray_color)
    def ray_color(self, rays: np.ndarray, samples: int, depth: int, seed: int = 1, sample_offset: int = 0, camera=None,
                  accum: Optional[np.ndarray] = None, **sky):
        """The path integral along the caller's rays (rt_ray_color): rays is an
        array of rt_path_ray (PATH_RAY_DTYPE, make_path_rays); returns the (n, 3)
        float32 sums over `samples` paths per ray (divide by the sample count) and
        the stats.  accum: sums of earlier calls to add to (accumulate).  camera
        and **sky as ray_color_params."""
        rays = np.ascontiguousarray(rays, PATH_RAY_DTYPE)
        n = rays.shape[0]
        p = ray_color_params(samples, depth, seed, sample_offset, camera, accum is not None, **sky)
        if accum is None:
            accum = np.zeros((n, 3), np.float32)
        if accum.dtype != np.float32 or accum.size != 3 * n or not accum.flags["C_CONTIGUOUS"]:
            raise ValueError("accum must be a contiguous float32 array of 3 floats per ray")
        st = RtRayColorStats()
        self._check(self._lib.rt_ray_color(self._h, rays.ctypes.data_as(C.POINTER(RtPathRay)), n, C.byref(p),
                                           _f32p(accum), C.byref(st)))
        return accum, st

    def ray_color_device(self, rays_ptr: int, n: int, params: RtRayColorParams, rgb_ptr: int, stream: int = 0):
        """rt_ray_color_device: n rt_path_ray at device address rays_ptr -> 3 n
        floats at rgb_ptr, asynchronous on `stream`."""
        self._check(self._lib.rt_ray_color_device(self._h, C.c_void_p(rays_ptr), n, C.byref(params),
                                                  C.c_void_p(rgb_ptr), C.c_void_p(stream)))

    # ---- path integrals over directions drawn on the device (rt_gather)
    def gather(self, pts: np.ndarray, source: int, samples: int, depth: int, seed: int = 1, sample_offset: int = 0,
               camera=None, accum: Optional[np.ndarray] = None, **sky):
        """rt_gather: pts is an array of rt_gather_point (GATHER_POINT_DTYPE,
        make_gather_points); returns the (n, 3) float32 sums over `samples`
        paths per point, each along a direction `source` draws for it, and the
        stats.  COSINE: irradiance = pi * rgb / samples; SPHERE: the mean over
        the sphere = rgb / samples.  The rest as ray_color."""
        pts = np.ascontiguousarray(pts, GATHER_POINT_DTYPE)
        n = pts.shape[0]
        p = gather_params(source, samples, depth, seed, sample_offset, camera, accum is not None, **sky)
        if accum is None:
            accum = np.zeros((n, 3), np.float32)
        if accum.dtype != np.float32 or accum.size != 3 * n or not accum.flags["C_CONTIGUOUS"]:
            raise ValueError("accum must be a contiguous float32 array of 3 floats per point")
        st = RtRayColorStats()
        self._check(self._lib.rt_gather(self._h, pts.ctypes.data_as(C.POINTER(RtGatherPoint)), n, C.byref(p),
                                        _f32p(accum), C.byref(st)))
        return accum, st

    def gather_device(self, pts_ptr: int, n: int, params: RtGatherParams, rgb_ptr: int, stream: int = 0):
        """rt_gather_device: n rt_gather_point at device address pts_ptr -> 3 n
        floats at rgb_ptr, asynchronous on `stream`."""
        self._check(self._lib.rt_gather_device(self._h, C.c_void_p(pts_ptr), n, C.byref(params), C.c_void_p(rgb_ptr),
                                               C.c_void_p(stream)))

    def gather_rays(self, pts: np.ndarray, source: int, seed: int = 1, sample: int = 0) -> np.ndarray:
        """rt_gather_rays: the rt_path_ray (PATH_RAY_DTYPE) that sample `sample`
        of every point traces; needs no uploaded scene."""
        pts = np.ascontiguousarray(pts, GATHER_POINT_DTYPE)
        out = np.zeros(pts.shape[0], PATH_RAY_DTYPE)
        self._check(self._lib.rt_gather_rays(self._h, pts.ctypes.data_as(C.POINTER(RtGatherPoint)), pts.shape[0], source,
                                             seed, sample, out.ctypes.data_as(C.POINTER(RtPathRay))))
        return out

    # ---- SH projection of a probe (rt_gather_sh)
    def gather_sh(self, pts: np.ndarray, bands: int, samples: int, depth: int, seed: int = 1, sample_offset: int = 0,
                  camera=None, accum: Optional[np.ndarray] = None, **sky):
        """rt_gather_sh: pts as for gather (n is not read); returns the
        (n, bands^2, 3) float32 sums over `samples` directions on the sphere of
        radiance times the real SH basis at the direction, and the stats.  The
        projection coefficients are 4 pi / samples times the sums.  accum: sums
        of earlier calls to add to.  The rest as gather."""
        pts = np.ascontiguousarray(pts, GATHER_POINT_DTYPE)
        n = pts.shape[0]
        p = gather_sh_params(bands, samples, depth, seed, sample_offset, camera, accum is not None, **sky)
        k = bands * bands if 1 <= bands <= RT_SH_MAX_BANDS else 1          # (the call refuses other bands)
        if accum is None:
            accum = np.zeros((n, k, 3), np.float32)
        if accum.dtype != np.float32 or accum.size != 3 * k * n or not accum.flags["C_CONTIGUOUS"]:
            raise ValueError("accum must be a contiguous float32 array of 3 * bands^2 floats per point")
        st = RtRayColorStats()
        self._check(self._lib.rt_gather_sh(self._h, pts.ctypes.data_as(C.POINTER(RtGatherPoint)), n, C.byref(p),
                                           _f32p(accum), C.byref(st)))
        return accum.reshape(n, k, 3), st

    def gather_sh_device(self, pts_ptr: int, n: int, params: RtGatherShParams, sh_ptr: int, stream: int = 0):
        """rt_gather_sh_device: n rt_gather_point at device address pts_ptr ->
        3 * bands^2 * n floats at sh_ptr, asynchronous on `stream`."""
        self._check(self._lib.rt_gather_sh_device(self._h, C.c_void_p(pts_ptr), n, C.byref(params), C.c_void_p(sh_ptr),
                                                  C.c_void_p(stream)))

    # ---- next-event estimation at the gather point (rt_gather_surface)
    def gather_surface(self, pts: np.ndarray, samples: int, depth: int, seed: int = 1, sample_offset: int = 0,
                       camera=None, accum: Optional[np.ndarray] = None, **sky):
        """rt_gather_surface: pts as for gather; every point is shaded as the
        render's first diffuse vertex (white Lambertian, normal unit(n)): the
        lights are sampled at the point and the scattered path goes on under
        the light-hit rule.  Returns the (n, 3) float32 sums over `samples`
        paths per point and the stats; pi * rgb / samples is the irradiance
        as the render estimates it, depth = 1 the direct light alone.  The
        rest as gather."""
        pts = np.ascontiguousarray(pts, GATHER_POINT_DTYPE)
        n = pts.shape[0]
        p = surface_params(samples, depth, seed, sample_offset, camera, accum is not None, **sky)
        if accum is None:
            accum = np.zeros((n, 3), np.float32)
        if accum.dtype != np.float32 or accum.size != 3 * n or not accum.flags["C_CONTIGUOUS"]:
            raise ValueError("accum must be a contiguous float32 array of 3 floats per point")
        st = RtRayColorStats()
        self._check(self._lib.rt_gather_surface(self._h, pts.ctypes.data_as(C.POINTER(RtGatherPoint)), n, C.byref(p),
                                                _f32p(accum), C.byref(st)))
        return accum, st

    def gather_surface_device(self, pts_ptr: int, n: int, params: RtGatherSurfaceParams, rgb_ptr: int, stream: int = 0):
        """rt_gather_surface_device: n rt_gather_point at device address
        pts_ptr -> 3 n floats at rgb_ptr, asynchronous on `stream`."""
        self._check(self._lib.rt_gather_surface_device(self._h, C.c_void_p(pts_ptr), n, C.byref(params),
                                                       C.c_void_p(rgb_ptr), C.c_void_p(stream)))


# ---------------------------------------------------------------------------
# rt.NewBucketRenderer analogue (progressive 3-pass, RGBA8 framebuffer)
# ---------------------------------------------------------------------------
class BucketRenderer:
    """NewBucketRenderer(camera, world, bucketSize, numWorkers) on the GPU
    (bucket_renderer.go:54-74); passes as in renderPass (:170-214)."""

    def __init__(self, scene: Scene, bucket_size: int = 32, num_workers: int = 0, device: int = 0, seed: int = 1):
        self._lib = rtscene()
        self.scene = scene
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = self._lib.rts_renderer_create(scene._h, bucket_size, num_workers, device, seed, C.byref(h), err, 512)
        if rc != RT_OK:
            raise RTError(rc, err.value.decode())
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.rts_renderer_destroy(self._h)
            self._h = None

    def _check(self, rc):
        if rc != RT_OK:
            raise RTError(rc, self._lib.rts_renderer_last_error(self._h).decode())

    def render_pass(self, p: int):
        self._check(self._lib.rts_renderer_render_pass(self._h, p))

    def render_all(self):
        self._check(self._lib.rts_renderer_render_all(self._h))

    def is_completed(self) -> bool:
        return bool(self._lib.rts_renderer_is_completed(self._h))

    def framebuffer(self) -> np.ndarray:
        w, h = self.scene.width, self.scene.height
        p = self._lib.rts_renderer_framebuffer(self._h)
        return np.ctypeslib.as_array(p, shape=(h, w, 4)).copy()

    def accum(self) -> np.ndarray:
        w, h = self.scene.width, self.scene.height
        return np.ctypeslib.as_array(self._lib.rts_renderer_accum(self._h), shape=(h, w, 3)).copy()

    def duration_ms(self) -> float:
        return float(self._lib.rts_renderer_duration_ms(self._h))

    def timings(self) -> dict:
        """Construction ms (context + scene upload), each pass's wall ms (host
        buffers + tonemap) and its device render ms."""
        t = (C.c_double * 7)()
        self._check(self._lib.rts_renderer_timings(self._h, t))
        return {"create_ms": t[0], "pass_wall_ms": [t[1], t[2], t[3]], "pass_render_ms": [t[4], t[5], t[6]]}

    def save_image(self, path: str):
        self._check(self._lib.rts_renderer_save_png(self._h, path.encode()))


def load_hdr(path: str):
    lib = rtscene()
    w = C.c_int32()
    h = C.c_int32()
    rc = lib.rts_load_hdr(path.encode(), C.byref(w), C.byref(h), None, 0)
    if rc != RT_OK:
        raise RTError(rc, path)
    out = np.zeros((h.value, w.value, 3), np.float64)
    rc = lib.rts_load_hdr(path.encode(), C.byref(w), C.byref(h), out.ctypes.data_as(C.POINTER(C.c_double)),
                          out.size)
    if rc != RT_OK:
        raise RTError(rc, path)
    return out


def write_png(path: str, rgba: np.ndarray):
    a = np.ascontiguousarray(rgba, np.uint8)
    rc = rtscene().rts_write_png(path.encode(), a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0])
    if rc != RT_OK:
        raise RTError(rc, path)
