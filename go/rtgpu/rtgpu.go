// Package rtgpu is the cgo binding of librtgpu.so (include/rtgpu.h), the
// MI355X path tracer that replaces the per-pixel loop of rt.BucketRenderer
// (rt/bucket_renderer.go:257-301 -> rt/camera.go:368-518).
//
// COMPILE-UNVERIFIED: the build image of this repository has no Go toolchain.
// The struct layouts below are pinned against include/rtgpu.h by
// tests/test_go_binding.py (gcc offsetof vs. the Go field list parsed from
// this file); everything else is reviewed, not compiled.
//
// Install (see INTEGRATION.md §2): copy this directory to <go-raytracing>/rtgpu
// and link the repository's headers and library next to it:
//
//	ln -s /path/to/repo/include rtgpu/include
//	ln -s /path/to/repo/go-raytracing_amd/lib rtgpu/lib
//
// Package rt never sees a C type: it fills the pointer-free mirror structs
// declared here (Node, Material, Texture, Perlin, CameraDesc, Bucket) and
// this package passes them across the boundary.  The library copies every
// array before rt_scene_upload / rt_render return and keeps no caller
// memory, so the Go memory is pinned only for the duration of one call.
package rtgpu

/*
#cgo CFLAGS: -I${SRCDIR}/include
#cgo LDFLAGS: -L${SRCDIR}/lib -lrtgpu -Wl,-rpath,${SRCDIR}/lib
#include <stdlib.h>
#include "rtgpu.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"unsafe"
)

// ABIVersion is the RT_ABI_VERSION this binding was written against.
const ABIVersion = 8 // RT_ABI_VERSION

// Hittable kinds (enum rt_hittable_kind).
const (
	KindSphere    int32 = 1  // RT_SPHERE
	KindQuad      int32 = 2  // RT_QUAD
	KindTriangle  int32 = 3  // RT_TRIANGLE
	KindPlane     int32 = 4  // RT_PLANE
	KindList      int32 = 5  // RT_LIST
	KindBVHNode   int32 = 6  // RT_BVH_NODE
	KindBVHLeaf   int32 = 7  // RT_BVH_LEAF
	KindTranslate int32 = 8  // RT_TRANSLATE
	KindRotateX   int32 = 9  // RT_ROTATE_X
	KindRotateY   int32 = 10 // RT_ROTATE_Y
	KindRotateZ   int32 = 11 // RT_ROTATE_Z
	KindScale     int32 = 12 // RT_SCALE
	KindVolume    int32 = 13 // RT_VOLUME
	KindCircle    int32 = 14 // RT_CIRCLE
)

// Material kinds (enum rt_material_kind).
const (
	MatLambertian   int32 = 1 // RT_LAMBERTIAN
	MatMetal        int32 = 2 // RT_METAL
	MatDielectric   int32 = 3 // RT_DIELECTRIC
	MatDiffuseLight int32 = 4 // RT_DIFFUSE_LIGHT
	MatIsotropic    int32 = 5 // RT_ISOTROPIC
)

// Texture kinds (enum rt_texture_kind).
const (
	TexSolid   int32 = 1 // RT_TEX_SOLID
	TexChecker int32 = 2 // RT_TEX_CHECKER
	TexNoise   int32 = 3 // RT_TEX_NOISE
	TexImage   int32 = 4 // RT_TEX_IMAGE
)

// Status codes (enum rt_status).
const (
	StatusOK          = 0  // RT_OK
	StatusInvalid     = -1 // RT_ERR_INVALID
	StatusUnsupported = -2 // RT_ERR_UNSUPPORTED
	StatusHIP         = -3 // RT_ERR_HIP
	StatusOOM         = -4 // RT_ERR_OOM
	StatusNoScene     = -5 // RT_ERR_NO_SCENE
	StatusDevice      = -6 // RT_ERR_DEVICE
)

// Context options (rt_ctx_set_option).
const (
	OptBLASBuilder  int32 = 1 // RT_OPT_BLAS_BUILDER
	OptTLASBuilder  int32 = 2 // RT_OPT_TLAS_BUILDER
	OptNodeFormat   int32 = 3 // RT_OPT_NODE_FORMAT
	OptBatchSlots   int32 = 4 // RT_OPT_BATCH_SLOTS
	OptRefill       int32 = 5 // RT_OPT_REFILL
	OptMaxBlocks    int32 = 6 // RT_OPT_MAX_BLOCKS
	OptStreams      int32 = 7 // RT_OPT_STREAMS
	OptVolumes      int32 = 8 // RT_OPT_VOLUMES
	VolumesLifted   int32 = 0 // RT_VOLUMES_LIFTED
	VolumesInBVH    int32 = 1 // RT_VOLUMES_IN_BVH
	OptBVH4Collapse int32 = 9 // RT_OPT_BVH4_COLLAPSE
	CollapseSAH     int32 = 0 // RT_COLLAPSE_SAH
	CollapseGreedy  int32 = 1 // RT_COLLAPSE_GREEDY
	BuildReference  int32 = 0 // RT_BLAS_REFERENCE
	BuildSAH        int32 = 1 // RT_BLAS_SAH
	BuildDevice     int32 = 2 // RT_BLAS_DEVICE
	NodesFP32       int32 = 0 // RT_NODES_FP32
	NodesQuant8     int32 = 1 // RT_NODES_QUANT8
	NodesWide8      int32 = 2 // RT_NODES_WIDE8
	OptDealing      int32 = 10 // RT_OPT_DEALING
	OptDealFirst    int32 = 11 // RT_OPT_DEAL_FIRST
	OptTail         int32 = 12 // RT_OPT_TAIL
	OptOverlap      int32 = 13 // RT_OPT_OVERLAP
	OptLiftPrims    int32 = 14 // RT_OPT_LIFT_PRIMS
	OptEarlyMiss    int32 = 15 // RT_OPT_EARLY_MISS
	PrimsLifted     int32 = 0  // RT_PRIMS_LIFTED
	PrimsInBVH      int32 = 1  // RT_PRIMS_IN_BVH
	DealStatic      int32 = 0  // RT_DEAL_STATIC
	DealDynamic     int32 = 1  // RT_DEAL_DYNAMIC
)

// Node mirrors rt_hittable: one node per concrete rt.Hittable.  P holds the
// kind's float64 fields in the order rtgpu.h documents per kind.
//
//rtgpu:mirror rt_hittable
type Node struct {
	Kind     int32       `c:"kind"`
	Material int32       `c:"material"`
	A        int32       `c:"a"`
	B        int32       `c:"b"`
	BBox     [6]float64  `c:"bbox"`
	P        [16]float64 `c:"p"`
}

// Material mirrors rt_material.
//
//rtgpu:mirror rt_material
type Material struct {
	Kind            int32      `c:"kind"`
	Texture         int32      `c:"texture"`
	Albedo          [3]float64 `c:"albedo"`
	Fuzz            float64    `c:"fuzz"`
	RefractionIndex float64    `c:"refraction_index"`
}

// Texture mirrors rt_texture (the 4-byte hole after Odd is C's padding).
//
//rtgpu:mirror rt_texture
type Texture struct {
	Kind     int32      `c:"kind"`
	Even     int32      `c:"even"`
	Odd      int32      `c:"odd"`
	_        int32      `c:"-"`
	Albedo   [3]float64 `c:"albedo"`
	InvScale float64    `c:"inv_scale"`
	Scale    float64    `c:"scale"`
	Perlin   int32      `c:"perlin"`
	Image    int32      `c:"image"`
}

// Perlin mirrors rt_perlin: the tables NewPerlin drew (rt/noise.go:8-13).
//
//rtgpu:mirror rt_perlin
type Perlin struct {
	RandVec [256][3]float64 `c:"randvec"`
	PermX   [256]int32      `c:"perm_x"`
	PermY   [256]int32      `c:"perm_y"`
	PermZ   [256]int32      `c:"perm_z"`
}

// CameraDesc mirrors rt_camera_desc: the state Camera.Initialize leaves
// (rt/camera.go:286-344).
//
//rtgpu:mirror rt_camera_desc
type CameraDesc struct {
	ImageWidth       int32      `c:"image_width"`
	ImageHeight      int32      `c:"image_height"`
	SamplesPerPixel  int32      `c:"samples_per_pixel"`
	MaxDepth         int32      `c:"max_depth"`
	Center           [3]float64 `c:"center"`
	Pixel00          [3]float64 `c:"pixel00"`
	PixelDeltaU      [3]float64 `c:"pixel_delta_u"`
	PixelDeltaV      [3]float64 `c:"pixel_delta_v"`
	DefocusAngle     float64    `c:"defocus_angle"`
	DefocusDiskU     [3]float64 `c:"defocus_disk_u"`
	DefocusDiskV     [3]float64 `c:"defocus_disk_v"`
	Background       [3]float64 `c:"background"`
	UseSkyGradient   int32      `c:"use_sky_gradient"`
	PhantomHDRI      int32      `c:"phantom_hdri"`
	CameraMotion     int32      `c:"camera_motion"`
	FreeCamera       int32      `c:"free_camera"`
	CenterMotionOrig [3]float64 `c:"center_motion_orig"`
	CenterMotionDir  [3]float64 `c:"center_motion_dir"`
	LookAtMotionOrig [3]float64 `c:"look_at_motion_orig"`
	LookAtMotionDir  [3]float64 `c:"look_at_motion_dir"`
	Vup              [3]float64 `c:"vup"`
	Forward          [3]float64 `c:"forward"`
	ViewportWidth    float64    `c:"viewport_width"`
	ViewportHeight   float64    `c:"viewport_height"`
	FocusDist        float64    `c:"focus_dist"`
	DefocusRadius    float64    `c:"defocus_radius"`
}

// Bucket mirrors rt_bucket (rt.Bucket with int32 fields).
//
//rtgpu:mirror rt_bucket
type Bucket struct {
	X      int32 `c:"x"`
	Y      int32 `c:"y"`
	Width  int32 `c:"width"`
	Height int32 `c:"height"`
}

// Stats mirrors rt_stats.
//
//rtgpu:mirror rt_stats
type Stats struct {
	KernelMs float64 `c:"kernel_ms"`
	Samples  uint64  `c:"samples"`
}

// SceneInfo mirrors rt_scene_info.
//
//rtgpu:mirror rt_scene_info
type SceneInfo struct {
	Nodes       int32 `c:"nodes"`
	Leaves      int32 `c:"leaves"`
	Refs        int32 `c:"refs"`
	Spheres     int32 `c:"spheres"`
	Quads       int32 `c:"quads"`
	Triangles   int32 `c:"triangles"`
	Planes      int32 `c:"planes"`
	Instances   int32 `c:"instances"`
	BLASes      int32 `c:"blases"`
	Volumes     int32 `c:"volumes"`
	Materials   int32 `c:"materials"`
	Textures    int32 `c:"textures"`
	Lights      int32 `c:"lights"`
	StackNeeded int32 `c:"stack_needed"`
	TLASDepth   int32 `c:"tlas_depth"`
	BLASDepth   int32 `c:"blas_depth"`
	DeviceBytes int64 `c:"device_bytes"`
	NodeFormat  int32 `c:"node_format"`
	Nodes8      int32 `c:"nodes8"`
}

// Image is an ImageLoader's pixels (rt/image_loader.go:17-24): linear
// float64 rgb, row-major, Width*Height*3 values.  Width == 0 is an
// ImageLoader without data (ImageTexture.Value returns cyan).
type Image struct {
	Width, Height int
	RGB           []float64
}

// Environment is an HDRIEnvironment (rt/hdri.go:13-26).  The library builds
// the importance-sampling tables itself (hdri.go:145-224).
type Environment struct {
	Image              Image
	Rotation           float64 // radians
	ImportanceSampling bool
}

// Scene is the flattened object graph rt_scene_upload takes.
type Scene struct {
	Nodes     []Node
	Children  []int32 // child index table of KindList / KindBVHLeaf nodes
	Root      int32
	Materials []Material
	Textures  []Texture
	Lights    []int32 // Camera.Lights as node indices
	Env       *Environment
	Images    []Image
	Perlins   []Perlin
}

// Error is a non-OK status of an entry point with rt_last_error's message.
type Error struct {
	Status  int
	Message string
}

func (e *Error) Error() string { return fmt.Sprintf("rtgpu: status %d: %s", e.Status, e.Message) }

// IsUnsupported reports whether err is RT_ERR_UNSUPPORTED: a Go type or
// nesting the GPU path does not take; the caller renders on the CPU.
func IsUnsupported(err error) bool {
	var e *Error
	return errors.As(err, &e) && e.Status == StatusUnsupported
}

// Ctx is a context over one or several devices (rt_ctx).  Not safe for
// concurrent use.
type Ctx struct {
	p *C.rt_ctx
}

// DeviceCount is the number of visible HIP devices (rt_device_count).
func DeviceCount() (int, error) {
	var n C.int32_t
	if rc := C.rt_device_count(&n); rc != C.RT_OK {
		return 0, &Error{int(rc), "rt_device_count failed"}
	}
	return int(n), nil
}

// New creates a context after checking the ABI: on HIP device devices[0]
// alone, or over every listed device (rt_ctx_create_multi: each render deals
// its buckets round-robin over them, like bucket_renderer.go:193-213's
// worker pool with one GPU per worker).  No devices: every visible device.
func New(devices ...int) (*Ctx, error) {
	if v := int(C.rt_abi_version()); v != ABIVersion {
		return nil, &Error{StatusInvalid, fmt.Sprintf("librtgpu ABI %d, binding expects %d", v, ABIVersion)}
	}
	if len(devices) == 0 {
		n, err := DeviceCount()
		if err != nil {
			return nil, err
		}
		if n == 0 {
			return nil, &Error{StatusHIP, "no HIP device"}
		}
		for d := 0; d < n; d++ {
			devices = append(devices, d)
		}
	}
	var p *C.rt_ctx
	if len(devices) == 1 {
		if rc := C.rt_ctx_create(C.int(devices[0]), &p); rc != C.RT_OK {
			return nil, &Error{int(rc), "rt_ctx_create failed"}
		}
		return &Ctx{p: p}, nil
	}
	list := (*C.int32_t)(C.calloc(C.size_t(len(devices)), C.sizeof_int32_t))
	defer C.free(unsafe.Pointer(list))
	ids := unsafe.Slice(list, len(devices))
	for i, d := range devices {
		ids[i] = C.int32_t(d)
	}
	if rc := C.rt_ctx_create_multi(list, C.int32_t(len(devices)), &p); rc != C.RT_OK {
		return nil, &Error{int(rc), "rt_ctx_create_multi failed"}
	}
	return &Ctx{p: p}, nil
}

// NumDevices is the number of devices the context renders on.
func (c *Ctx) NumDevices() int { return int(C.rt_ctx_num_devices(c.p)) }

// LastDealing reports the last multi-device render's split: the tiles each
// device rendered and the runs it claimed (rt_last_dealing).
func (c *Ctx) LastDealing() (tiles, runs []int32, err error) {
	n := c.NumDevices()
	tiles, runs = make([]int32, n), make([]int32, n)
	if n == 0 {
		return tiles, runs, nil
	}
	err = c.check(C.rt_last_dealing(c.p, (*C.int32_t)(unsafe.Pointer(&tiles[0])),
		(*C.int32_t)(unsafe.Pointer(&runs[0])), C.int32_t(n)))
	return tiles, runs, err
}

// Close releases the context and its device memory.
func (c *Ctx) Close() {
	if c.p != nil {
		C.rt_ctx_destroy(c.p)
		c.p = nil
	}
}

func (c *Ctx) check(rc C.int) error {
	if rc == C.RT_OK {
		return nil
	}
	return &Error{int(rc), C.GoString(C.rt_last_error(c.p))}
}

// SetOption sets a context option (OptBLASBuilder / OptTLASBuilder /
// OptNodeFormat / OptVolumes / OptBVH4Collapse, or a schedule option: OptBatchSlots, OptRefill,
// OptMaxBlocks, OptStreams, OptDealing, OptDealFirst, which never change
// the image).  The scene
// options take effect at the next Upload, the schedule options at the next
// render.
func (c *Ctx) SetOption(key, value int32) error {
	return c.check(C.rt_ctx_set_option(c.p, C.int32_t(key), C.int32_t(value)))
}

// SetMeshBuilder chooses how mesh BVHs are laid out on the device
// (BuildReference / BuildSAH / BuildDevice).
func (c *Ctx) SetMeshBuilder(b int32) error { return c.SetOption(OptBLASBuilder, b) }

// Upload flattens and copies the scene to the device.  The descriptor and
// its small C-side arrays (rt_image, rt_environment) hold Go pointers that
// are pinned for the call only: the library copies everything before
// returning (rtgpu.h: "C never retains caller memory").
func (c *Ctx) Upload(s *Scene) error {
	if len(s.Nodes) == 0 {
		return &Error{StatusInvalid, "empty scene"}
	}
	var pin runtime.Pinner
	defer pin.Unpin()

	d := (*C.rt_scene_desc)(C.calloc(1, C.sizeof_rt_scene_desc))
	defer C.free(unsafe.Pointer(d))

	pin.Pin(&s.Nodes[0])
	d.hittables = (*C.rt_hittable)(unsafe.Pointer(&s.Nodes[0]))
	d.num_hittables = C.int32_t(len(s.Nodes))
	if len(s.Children) > 0 {
		pin.Pin(&s.Children[0])
		d.children = (*C.int32_t)(unsafe.Pointer(&s.Children[0]))
	}
	d.num_children = C.int32_t(len(s.Children))
	d.root = C.int32_t(s.Root)
	if len(s.Materials) > 0 {
		pin.Pin(&s.Materials[0])
		d.materials = (*C.rt_material)(unsafe.Pointer(&s.Materials[0]))
	}
	d.num_materials = C.int32_t(len(s.Materials))
	if len(s.Textures) > 0 {
		pin.Pin(&s.Textures[0])
		d.textures = (*C.rt_texture)(unsafe.Pointer(&s.Textures[0]))
	}
	d.num_textures = C.int32_t(len(s.Textures))
	if len(s.Lights) > 0 {
		pin.Pin(&s.Lights[0])
		d.lights = (*C.int32_t)(unsafe.Pointer(&s.Lights[0]))
	}
	d.num_lights = C.int32_t(len(s.Lights))
	if len(s.Perlins) > 0 {
		pin.Pin(&s.Perlins[0])
		d.perlins = (*C.rt_perlin)(unsafe.Pointer(&s.Perlins[0]))
	}
	d.num_perlins = C.int32_t(len(s.Perlins))

	if n := len(s.Images); n > 0 {
		imgs := unsafe.Slice((*C.rt_image)(C.calloc(C.size_t(n), C.sizeof_rt_image)), n)
		defer C.free(unsafe.Pointer(&imgs[0]))
		for i := range s.Images {
			imgs[i].width, imgs[i].height, imgs[i].rgb = imageArgs(&pin, &s.Images[i])
		}
		d.images = &imgs[0]
		d.num_images = C.int32_t(n)
	}
	if s.Env != nil {
		env := (*C.rt_environment)(C.calloc(1, C.sizeof_rt_environment))
		defer C.free(unsafe.Pointer(env))
		env.width, env.height, env.rgb = imageArgs(&pin, &s.Env.Image)
		env.rotation = C.double(s.Env.Rotation)
		if s.Env.ImportanceSampling {
			env.use_importance_sampling = 1
		}
		d.environment = env
	}
	return c.check(C.rt_scene_upload(c.p, d))
}

func imageArgs(pin *runtime.Pinner, im *Image) (C.int32_t, C.int32_t, *C.double) {
	if im.Width <= 0 || im.Height <= 0 || len(im.RGB) < im.Width*im.Height*3 {
		return 0, 0, nil // ImageLoader without data
	}
	pin.Pin(&im.RGB[0])
	return C.int32_t(im.Width), C.int32_t(im.Height), (*C.double)(unsafe.Pointer(&im.RGB[0]))
}

// Info returns the sizes of the flattened device scene.
func (c *Ctx) Info() (SceneInfo, error) {
	var info SceneInfo
	err := c.check(C.rt_scene_get_info(c.p, (*C.rt_scene_info)(unsafe.Pointer(&info))))
	return info, err
}

// LiftedPrims returns how many world quads / spheres the uploaded scene keeps
// out of its world BVH (rt_scene_lifted_prims, OptLiftPrims; 0: none lifted).
func (c *Ctx) LiftedPrims() (int, error) {
	var n C.int32_t
	err := c.check(C.rt_scene_lifted_prims(c.p, &n))
	return int(n), err
}

// RenderParams is one rt_render call: samplesForPass / depthForPass of
// bucket_renderer.go:175-191 over a set of buckets.
type RenderParams struct {
	SamplesPerPixel int
	MaxDepth        int
	SampleOffset    int
	Seed            uint32
	Buckets         []Bucket // nil: the whole image
	Accumulate      bool     // false: overwrite the buckets' pixels
}

// Render renders into accum (Width*Height*3 float32, the per-pixel sum of
// sample radiance, linear) and blocks until done.
func (c *Ctx) Render(cam *CameraDesc, p RenderParams, accum []float32) (Stats, error) {
	var st Stats
	if len(accum) < int(cam.ImageWidth)*int(cam.ImageHeight)*3 {
		return st, &Error{StatusInvalid, "accum buffer smaller than width*height*3"}
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	prm := (*C.rt_render_params)(C.calloc(1, C.sizeof_rt_render_params))
	defer C.free(unsafe.Pointer(prm))
	prm.samples_per_pixel = C.int32_t(p.SamplesPerPixel)
	prm.max_depth = C.int32_t(p.MaxDepth)
	prm.sample_offset = C.int32_t(p.SampleOffset)
	prm.seed = C.uint32_t(p.Seed)
	if len(p.Buckets) > 0 {
		pin.Pin(&p.Buckets[0])
		prm.buckets = (*C.rt_bucket)(unsafe.Pointer(&p.Buckets[0]))
		prm.num_buckets = C.int32_t(len(p.Buckets))
	}
	if p.Accumulate {
		prm.accumulate = 1
	}
	rc := C.rt_render(c.p, (*C.rt_camera_desc)(unsafe.Pointer(cam)), prm,
		(*C.float)(unsafe.Pointer(&accum[0])), (*C.rt_stats)(unsafe.Pointer(&st)))
	return st, c.check(rc)
}

// RenderRGBA is one progressive pass as renderBucketWithQuality does it
// (bucket_renderer.go:257-301): the buckets are rendered into the context's
// device-resident sums and quantised on the device (:276-285); only the
// RGBA8 framebuffer (width*height*4 bytes) comes back.  Pixels outside the
// buckets keep their previous value (rt_render_rgba8).
func (c *Ctx) RenderRGBA(cam *CameraDesc, p RenderParams, rgba []byte) (Stats, error) {
	var st Stats
	if len(rgba) < int(cam.ImageWidth)*int(cam.ImageHeight)*4 {
		return st, &Error{StatusInvalid, "rgba buffer smaller than width*height*4"}
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	prm := (*C.rt_render_params)(C.calloc(1, C.sizeof_rt_render_params))
	defer C.free(unsafe.Pointer(prm))
	prm.samples_per_pixel = C.int32_t(p.SamplesPerPixel)
	prm.max_depth = C.int32_t(p.MaxDepth)
	prm.sample_offset = C.int32_t(p.SampleOffset)
	prm.seed = C.uint32_t(p.Seed)
	if len(p.Buckets) > 0 {
		pin.Pin(&p.Buckets[0])
		prm.buckets = (*C.rt_bucket)(unsafe.Pointer(&p.Buckets[0]))
		prm.num_buckets = C.int32_t(len(p.Buckets))
	}
	if p.Accumulate {
		prm.accumulate = 1
	}
	rc := C.rt_render_rgba8(c.p, (*C.rt_camera_desc)(unsafe.Pointer(cam)), prm,
		(*C.uint8_t)(unsafe.Pointer(&rgba[0])), (*C.rt_stats)(unsafe.Pointer(&st)))
	return st, c.check(rc)
}

// Sync waits for every render enqueued on the context and reports a
// device-side error of any of them.
func (c *Ctx) Sync() error { return c.check(C.rt_sync(c.p)) }

// Tonemap quantises an accumulated sum to RGBA8 exactly as
// bucket_renderer.go:276-285 does (1/spp, LinearToGamma, clamp, 256x).
func (c *Ctx) Tonemap(accum []float32, width, height, spp int, rgba []byte) error {
	if len(accum) < width*height*3 || len(rgba) < width*height*4 {
		return &Error{StatusInvalid, "tonemap buffer too small"}
	}
	return c.check(C.rt_tonemap_rgba8(c.p, (*C.float)(unsafe.Pointer(&accum[0])), C.int32_t(width),
		C.int32_t(height), C.int32_t(spp), (*C.uint8_t)(unsafe.Pointer(&rgba[0]))))
}

// RenderFeatures fills feat (Width*Height*8 float32: per pixel the sums over
// the call's samples of albedo.rgb, normal.xyz, depth, coverage at the camera
// rays' closest hits) for the same path keys as Render with the same Seed and
// SampleOffset (rt_render_features); MaxDepth is ignored.  Blocks.
func (c *Ctx) RenderFeatures(cam *CameraDesc, p RenderParams, feat []float32) (Stats, error) {
	var st Stats
	if len(feat) < int(cam.ImageWidth)*int(cam.ImageHeight)*8 {
		return st, &Error{StatusInvalid, "feature buffer smaller than width*height*8"}
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	prm := (*C.rt_render_params)(C.calloc(1, C.sizeof_rt_render_params))
	defer C.free(unsafe.Pointer(prm))
	prm.samples_per_pixel = C.int32_t(p.SamplesPerPixel)
	prm.max_depth = C.int32_t(p.MaxDepth)
	prm.sample_offset = C.int32_t(p.SampleOffset)
	prm.seed = C.uint32_t(p.Seed)
	if len(p.Buckets) > 0 {
		pin.Pin(&p.Buckets[0])
		prm.buckets = (*C.rt_bucket)(unsafe.Pointer(&p.Buckets[0]))
		prm.num_buckets = C.int32_t(len(p.Buckets))
	}
	if p.Accumulate {
		prm.accumulate = 1
	}
	rc := C.rt_render_features(c.p, (*C.rt_camera_desc)(unsafe.Pointer(cam)), prm,
		(*C.float)(unsafe.Pointer(&feat[0])), (*C.rt_stats)(unsafe.Pointer(&st)))
	return st, c.check(rc)
}

// DenoiseParams mirrors rt_denoise_params.
//
//rtgpu:mirror rt_denoise_params
type DenoiseParams struct {
	Iterations      int32   `c:"iterations"`
	NormalPowerLog2 int32   `c:"normal_power_log2"`
	Demodulate      int32   `c:"demodulate"`
	SigmaColor      float32 `c:"sigma_color"`
	SigmaDepth      float32 `c:"sigma_depth"`
	AlbedoEps       float32 `c:"albedo_eps"`
}

// DefaultDenoiseParams returns rt_denoise_default_params.
func DefaultDenoiseParams() DenoiseParams {
	var p DenoiseParams
	C.rt_denoise_default_params((*C.rt_denoise_params)(unsafe.Pointer(&p)))
	return p
}

// Denoise filters accum (Width*Height*3 sums of spp samples) guided by feat
// (RenderFeatures of the same samples) into out (rt_denoise); p nil = the
// defaults.  For the preview passes: the final pass is shown as rendered.
func (c *Ctx) Denoise(accum, feat []float32, width, height, spp int, p *DenoiseParams, out []float32) error {
	if len(accum) < width*height*3 || len(feat) < width*height*8 || len(out) < width*height*3 {
		return &Error{StatusInvalid, "denoise buffer too small"}
	}
	dp := DefaultDenoiseParams()
	if p != nil {
		dp = *p
	}
	return c.check(C.rt_denoise(c.p, (*C.float)(unsafe.Pointer(&accum[0])), (*C.float)(unsafe.Pointer(&feat[0])),
		C.int32_t(width), C.int32_t(height), C.int32_t(spp), (*C.rt_denoise_params)(unsafe.Pointer(&dp)),
		(*C.float)(unsafe.Pointer(&out[0]))))
}

// RenderMoments renders as Render does (accum receives the same bits) and
// also fills moments (Width*Height*2 float32: per pixel the sum and the sum
// of squares of the samples' luminance), the guide of DenoiseVariance
// (rt_render_moments).  Both buffers accumulate with p.Accumulate.  Blocks.
func (c *Ctx) RenderMoments(cam *CameraDesc, p RenderParams, accum, moments []float32) (Stats, error) {
	var st Stats
	if len(accum) < int(cam.ImageWidth)*int(cam.ImageHeight)*3 {
		return st, &Error{StatusInvalid, "accum buffer smaller than width*height*3"}
	}
	if len(moments) < int(cam.ImageWidth)*int(cam.ImageHeight)*2 {
		return st, &Error{StatusInvalid, "moments buffer smaller than width*height*2"}
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	prm := (*C.rt_render_params)(C.calloc(1, C.sizeof_rt_render_params))
	defer C.free(unsafe.Pointer(prm))
	prm.samples_per_pixel = C.int32_t(p.SamplesPerPixel)
	prm.max_depth = C.int32_t(p.MaxDepth)
	prm.sample_offset = C.int32_t(p.SampleOffset)
	prm.seed = C.uint32_t(p.Seed)
	if len(p.Buckets) > 0 {
		pin.Pin(&p.Buckets[0])
		prm.buckets = (*C.rt_bucket)(unsafe.Pointer(&p.Buckets[0]))
		prm.num_buckets = C.int32_t(len(p.Buckets))
	}
	if p.Accumulate {
		prm.accumulate = 1
	}
	rc := C.rt_render_moments(c.p, (*C.rt_camera_desc)(unsafe.Pointer(cam)), prm,
		(*C.float)(unsafe.Pointer(&accum[0])), (*C.float)(unsafe.Pointer(&moments[0])),
		(*C.rt_stats)(unsafe.Pointer(&st)))
	return st, c.check(rc)
}

// DenoiseVarParams mirrors rt_denoise_var_params.
//
//rtgpu:mirror rt_denoise_var_params
type DenoiseVarParams struct {
	Iterations      int32   `c:"iterations"`
	NormalPowerLog2 int32   `c:"normal_power_log2"`
	Demodulate      int32   `c:"demodulate"`
	SpatialBelow    int32   `c:"spatial_below"`
	SigmaLum        float32 `c:"sigma_lum"`
	SigmaDepth      float32 `c:"sigma_depth"`
	AlbedoEps       float32 `c:"albedo_eps"`
}

// DefaultDenoiseVarParams returns rt_denoise_variance_default_params.
func DefaultDenoiseVarParams() DenoiseVarParams {
	var p DenoiseVarParams
	C.rt_denoise_variance_default_params((*C.rt_denoise_var_params)(unsafe.Pointer(&p)))
	return p
}

// DenoiseVariance filters accum (Width*Height*3 sums of spp samples) guided
// by feat (RenderFeatures) and moments (RenderMoments) of the same samples
// into out (rt_denoise_variance); p nil = the defaults.  moments may be nil
// when spp is below SpatialBelow; outVar, if not nil, receives the filtered
// variance (Width*Height).
func (c *Ctx) DenoiseVariance(accum, feat, moments []float32, width, height, spp int, p *DenoiseVarParams,
	out, outVar []float32) error {
	if len(accum) < width*height*3 || len(feat) < width*height*8 || len(out) < width*height*3 {
		return &Error{StatusInvalid, "denoise buffer too small"}
	}
	if (moments != nil && len(moments) < width*height*2) || (outVar != nil && len(outVar) < width*height) {
		return &Error{StatusInvalid, "denoise buffer too small"}
	}
	dp := DefaultDenoiseVarParams()
	if p != nil {
		dp = *p
	}
	var mp, vp *C.float
	if moments != nil {
		mp = (*C.float)(unsafe.Pointer(&moments[0]))
	}
	if outVar != nil {
		vp = (*C.float)(unsafe.Pointer(&outVar[0]))
	}
	return c.check(C.rt_denoise_variance(c.p, (*C.float)(unsafe.Pointer(&accum[0])),
		(*C.float)(unsafe.Pointer(&feat[0])), mp, C.int32_t(width), C.int32_t(height), C.int32_t(spp),
		(*C.rt_denoise_var_params)(unsafe.Pointer(&dp)), (*C.float)(unsafe.Pointer(&out[0])), vp))
}

// AdaptiveParams mirrors rt_adaptive_params.
//
//rtgpu:mirror rt_adaptive_params
type AdaptiveParams struct {
	MinSpp        int32   `c:"min_spp"`
	StepSpp       int32   `c:"step_spp"`
	Neighbourhood int32   `c:"neighbourhood"`
	RelError      float32 `c:"rel_error"`
	LumFloor      float32 `c:"lum_floor"`
}

// AdaptiveStats mirrors rt_adaptive_stats.
//
//rtgpu:mirror rt_adaptive_stats
type AdaptiveStats struct {
	KernelMs    float64 `c:"kernel_ms"`
	Samples     uint64  `c:"samples"`
	Rounds      int32   `c:"rounds"`
	PixelsAtMax int32   `c:"pixels_at_max"`
}

// DefaultAdaptiveParams returns rt_adaptive_default_params.
func DefaultAdaptiveParams() AdaptiveParams {
	var p AdaptiveParams
	C.rt_adaptive_default_params((*C.rt_adaptive_params)(unsafe.Pointer(&p)))
	return p
}

// RenderAdaptive renders with p.SamplesPerPixel as the budget of every pixel
// and stops sampling a pixel once the standard error of its mean luminance is
// small enough (rt_render_adaptive); ap nil = the defaults.  accum
// (Width*Height*3), moments (Width*Height*2) and counts (Width*Height) receive
// the sums and moments of each bucket pixel's first counts[p] samples and
// counts[p]; pixels outside the buckets are untouched.  p.SampleOffset must be
// 0 and p.Accumulate false.  Blocks.
func (c *Ctx) RenderAdaptive(cam *CameraDesc, p RenderParams, ap *AdaptiveParams, accum, moments []float32,
	counts []uint32) (AdaptiveStats, error) {
	var st AdaptiveStats
	n := int(cam.ImageWidth) * int(cam.ImageHeight)
	if len(accum) < n*3 || len(moments) < n*2 || len(counts) < n {
		return st, &Error{StatusInvalid, "adaptive buffer too small"}
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	prm := (*C.rt_render_params)(C.calloc(1, C.sizeof_rt_render_params))
	defer C.free(unsafe.Pointer(prm))
	prm.samples_per_pixel = C.int32_t(p.SamplesPerPixel)
	prm.max_depth = C.int32_t(p.MaxDepth)
	prm.sample_offset = C.int32_t(p.SampleOffset)
	prm.seed = C.uint32_t(p.Seed)
	if len(p.Buckets) > 0 {
		pin.Pin(&p.Buckets[0])
		prm.buckets = (*C.rt_bucket)(unsafe.Pointer(&p.Buckets[0]))
		prm.num_buckets = C.int32_t(len(p.Buckets))
	}
	if p.Accumulate {
		prm.accumulate = 1
	}
	dp := DefaultAdaptiveParams()
	if ap != nil {
		dp = *ap
	}
	rc := C.rt_render_adaptive(c.p, (*C.rt_camera_desc)(unsafe.Pointer(cam)), prm,
		(*C.rt_adaptive_params)(unsafe.Pointer(&dp)), (*C.float)(unsafe.Pointer(&accum[0])),
		(*C.float)(unsafe.Pointer(&moments[0])), (*C.uint32_t)(unsafe.Pointer(&counts[0])),
		(*C.rt_adaptive_stats)(unsafe.Pointer(&st)))
	return st, c.check(rc)
}

// NormalizeSamples turns sums over counts[p] samples per pixel (channels
// floats each: 3 for a frame, 2 for moments, 8 for features) into sums over
// targetSpp samples, (sums / counts) * targetSpp, which Tonemap, Denoise and
// DenoiseVariance take (rt_normalize_samples).  out may be sums.
func (c *Ctx) NormalizeSamples(sums []float32, channels int, counts []uint32, width, height, targetSpp int,
	out []float32) error {
	n := width * height
	if n <= 0 || channels <= 0 || len(sums) < n*channels || len(counts) < n || len(out) < n*channels {
		return &Error{StatusInvalid, "normalize buffer too small"}
	}
	return c.check(C.rt_normalize_samples(c.p, (*C.float)(unsafe.Pointer(&sums[0])), C.int32_t(channels),
		(*C.uint32_t)(unsafe.Pointer(&counts[0])), C.int32_t(width), C.int32_t(height), C.int32_t(targetSpp),
		(*C.float)(unsafe.Pointer(&out[0]))))
}

// Ray mirrors rt_ray: the ray O + t D over the interval (TMin, TMax).
//
//rtgpu:mirror rt_ray
type Ray struct {
	O    [3]float32 `c:"o"`
	TMin float32    `c:"tmin"`
	D    [3]float32 `c:"d"`
	TMax float32    `c:"tmax"`
}

// RayHit mirrors rt_ray_hit.  A miss has T = -1, Top = Prim = Material = -1,
// N = 0 and Flags = 0.
//
//rtgpu:mirror rt_ray_hit
type RayHit struct {
	T        float32    `c:"t"`
	Top      int32      `c:"top"`
	Prim     int32      `c:"prim"`
	Material int32      `c:"material"`
	N        [3]float32 `c:"n"`
	Flags    uint32     `c:"flags"`
}

// RayHit.Flags bits.
const (
	HitFront      = 1 // RT_HIT_FRONT
	HitInvalidRay = 2 // RT_HIT_INVALID_RAY
)

// Hit reports whether the record is a hit.
func (h *RayHit) Hit() bool { return h.Prim >= 0 }

// TraceRays finds the closest hit of every ray in the uploaded scene
// (rt_trace_rays): what world.Hit(ray, Interval{TMin, TMax}) returns, decided
// as the render's closest-hit kernel decides it.  D need not be unit; T is
// the ray parameter.  time is the rays' ray.Time() (moving spheres).  A ray
// with a non-finite or zero component set, or TMax < TMin, comes back as a
// miss with HitInvalidRay.  Scenes holding a Volume are refused
// (IsUnsupported).  Blocks.
func (c *Ctx) TraceRays(rays []Ray, time float32, hits []RayHit) error {
	if len(hits) < len(rays) {
		return &Error{StatusInvalid, "hit buffer too small"}
	}
	if len(rays) == 0 {
		return nil
	}
	return c.check(C.rt_trace_rays(c.p, (*C.rt_ray)(unsafe.Pointer(&rays[0])), C.int64_t(len(rays)), C.float(time),
		(*C.rt_ray_hit)(unsafe.Pointer(&hits[0]))))
}

// Occluded writes 1 for every ray that hits anything in its interval and 0
// for the others (rt_occluded, the rule of the render's shadow rays).  Blocks.
func (c *Ctx) Occluded(rays []Ray, time float32, occluded []byte) error {
	if len(occluded) < len(rays) {
		return &Error{StatusInvalid, "occlusion buffer too small"}
	}
	if len(rays) == 0 {
		return nil
	}
	return c.check(C.rt_occluded(c.p, (*C.rt_ray)(unsafe.Pointer(&rays[0])), C.int64_t(len(rays)), C.float(time),
		(*C.uint8_t)(unsafe.Pointer(&occluded[0]))))
}

// PathRay mirrors rt_path_ray: the ray O + t D and the pixel word of its RNG
// key.  ID has nothing to do with where the result is written; rays that
// share an ID and a sample index follow the same random decisions.  Reserved
// must be 0.
//
//rtgpu:mirror rt_path_ray
type PathRay struct {
	O        [3]float32 `c:"o"`
	ID       uint32     `c:"id"`
	D        [3]float32 `c:"d"`
	Reserved uint32     `c:"reserved"`
}

// RayColorParams mirrors rt_ray_color_params.  Of the Camera only what
// rayColorInternal reads: Background, UseSkyGradient, and PhantomHDRI with
// CameraMaxDepth (0 = MaxDepth).
//
//rtgpu:mirror rt_ray_color_params
type RayColorParams struct {
	Samples        int32      `c:"samples"`
	MaxDepth       int32      `c:"max_depth"`
	SampleOffset   int32      `c:"sample_offset"`
	Seed           uint32     `c:"seed"`
	Accumulate     int32      `c:"accumulate"`
	UseSkyGradient int32      `c:"use_sky_gradient"`
	PhantomHDRI    int32      `c:"phantom_hdri"`
	CameraMaxDepth int32      `c:"camera_max_depth"`
	Background     [3]float64 `c:"background"`
}

// RayColorStats mirrors rt_ray_color_stats.
//
//rtgpu:mirror rt_ray_color_stats
type RayColorStats struct {
	KernelMs    float64 `c:"kernel_ms"`
	Samples     uint64  `c:"samples"`
	InvalidRays uint64  `c:"invalid_rays"`
}

// RayColor is Camera.RayColor for the caller's rays (rt_ray_color): rgb[3*i..]
// receives the sum over p.Samples paths of rayColorInternal(rays[i],
// p.MaxDepth), linear; the caller divides by the sample count.  Sample s of
// ray i runs under the key (p.Seed, rays[i].ID, p.SampleOffset + s) through
// the render's own kernels, so scenes holding a Volume are served.  D need not
// be unit.  A ray with a non-finite component or a zero direction adds
// nothing and is counted in the stats.  Blocks.
func (c *Ctx) RayColor(rays []PathRay, p RayColorParams, rgb []float32) (RayColorStats, error) {
	var st RayColorStats
	if len(rgb) < 3*len(rays) {
		return st, &Error{StatusInvalid, "radiance buffer too small"}
	}
	if len(rays) == 0 {
		return st, nil
	}
	rc := C.rt_ray_color(c.p, (*C.rt_path_ray)(unsafe.Pointer(&rays[0])), C.int64_t(len(rays)),
		(*C.rt_ray_color_params)(unsafe.Pointer(&p)), (*C.float)(unsafe.Pointer(&rgb[0])),
		(*C.rt_ray_color_stats)(unsafe.Pointer(&st)))
	return st, c.check(rc)
}

// Direction sources of Gather.
const (
	GatherRay    int32 = 0 // RT_GATHER_RAY
	GatherCosine int32 = 1 // RT_GATHER_COSINE
	GatherSphere int32 = 2 // RT_GATHER_SPHERE
)

// GatherPoint mirrors rt_gather_point (PathRay's layout): a position, the
// pixel word of its RNG key, and a normal that need not be unit.  Reserved
// must be 0.
//
//rtgpu:mirror rt_gather_point
type GatherPoint struct {
	P        [3]float32 `c:"p"`
	ID       uint32     `c:"id"`
	N        [3]float32 `c:"n"`
	Reserved uint32     `c:"reserved"`
}

// GatherParams mirrors rt_gather_params.  Path holds the words of a
// RayColorParams (56 B, 8-aligned); Gather fills it.
//
//rtgpu:mirror rt_gather_params
type GatherParams struct {
	Path     [7]uint64 `c:"path"`
	Source   int32     `c:"source"`
	Reserved int32     `c:"reserved"`
}

// Gather is RayColor over directions drawn on the device (rt_gather): sample s
// of point i starts at pts[i].P under the key (p.Seed, pts[i].ID,
// p.SampleOffset + s) along pts[i].N (GatherRay), along unit(N) plus a random
// unit vector (GatherCosine: density cos/pi about the normal, so the
// irradiance is pi * rgb / samples), or along a random unit vector
// (GatherSphere: the mean over the sphere is rgb / samples).  Everything else
// is RayColor's.  A point with a non-finite component, or a normal of length 0
// or not finite where it is read, adds nothing and is counted in the stats.
// Blocks.
func (c *Ctx) Gather(pts []GatherPoint, source int32, p RayColorParams, rgb []float32) (RayColorStats, error) {
	var st RayColorStats
	if len(rgb) < 3*len(pts) {
		return st, &Error{StatusInvalid, "radiance buffer too small"}
	}
	if len(pts) == 0 {
		return st, nil
	}
	var gp GatherParams
	*(*RayColorParams)(unsafe.Pointer(&gp.Path)) = p
	gp.Source = source
	rc := C.rt_gather(c.p, (*C.rt_gather_point)(unsafe.Pointer(&pts[0])), C.int64_t(len(pts)),
		(*C.rt_gather_params)(unsafe.Pointer(&gp)), (*C.float)(unsafe.Pointer(&rgb[0])),
		(*C.rt_ray_color_stats)(unsafe.Pointer(&st)))
	return st, c.check(rc)
}

// The largest band count GatherSH takes.
const (
	SHMaxBands int32 = 3 // RT_SH_MAX_BANDS
)

// GatherSHParams mirrors rt_gather_sh_params (GatherParams' layout).  Path
// holds the words of a RayColorParams (56 B, 8-aligned); GatherSH fills it.
//
//rtgpu:mirror rt_gather_sh_params
type GatherSHParams struct {
	Path     [7]uint64 `c:"path"`
	Bands    int32     `c:"bands"`
	Reserved int32     `c:"reserved"`
}

// GatherSH is Gather under GatherSphere kept by direction (rt_gather_sh): a
// light probe.  sh[(i*bands*bands+k)*3 + c] receives the sum over p.Samples
// directions d on the sphere of the radiance along d times Y_k(d), the real
// spherical-harmonic basis of Ramamoorthi & Hanrahan in the scene's axes, for
// k < bands*bands (bands 1..3: 1, 4 or 9 coefficients per point).  The
// projection coefficients are 4*pi/samples times the sums; the irradiance
// about a unit normal n is the sum of A_l c_lm Y_lm(n) with A = pi, 2*pi/3,
// pi/4.  p.Accumulate adds sh's previous values, so a probe is refined over
// calls with a growing p.SampleOffset.  N is not read.  A point with a
// non-finite position adds nothing and is counted in the stats.  Blocks.
func (c *Ctx) GatherSH(pts []GatherPoint, bands int32, p RayColorParams, sh []float32) (RayColorStats, error) {
	var st RayColorStats
	if bands < 1 || bands > SHMaxBands {
		return st, &Error{StatusInvalid, "SH bands outside 1 .. 3"}
	}
	if len(sh) < 3*int(bands*bands)*len(pts) {
		return st, &Error{StatusInvalid, "coefficient buffer too small"}
	}
	if len(pts) == 0 {
		return st, nil
	}
	var gp GatherSHParams
	*(*RayColorParams)(unsafe.Pointer(&gp.Path)) = p
	gp.Bands = bands
	rc := C.rt_gather_sh(c.p, (*C.rt_gather_point)(unsafe.Pointer(&pts[0])), C.int64_t(len(pts)),
		(*C.rt_gather_sh_params)(unsafe.Pointer(&gp)), (*C.float)(unsafe.Pointer(&sh[0])),
		(*C.rt_ray_color_stats)(unsafe.Pointer(&st)))
	return st, c.check(rc)
}

// Layout checks: each mirror is exactly as large as its C struct.
var (
	_ [unsafe.Sizeof(GatherSHParams{}) - uintptr(C.sizeof_rt_gather_sh_params)]byte
	_ [uintptr(C.sizeof_rt_gather_sh_params) - unsafe.Sizeof(GatherSHParams{})]byte
	_ [unsafe.Sizeof(GatherPoint{}) - uintptr(C.sizeof_rt_gather_point)]byte
	_ [uintptr(C.sizeof_rt_gather_point) - unsafe.Sizeof(GatherPoint{})]byte
	_ [unsafe.Sizeof(GatherParams{}) - uintptr(C.sizeof_rt_gather_params)]byte
	_ [uintptr(C.sizeof_rt_gather_params) - unsafe.Sizeof(GatherParams{})]byte
	_ [unsafe.Sizeof(PathRay{}) - uintptr(C.sizeof_rt_path_ray)]byte
	_ [uintptr(C.sizeof_rt_path_ray) - unsafe.Sizeof(PathRay{})]byte
	_ [unsafe.Sizeof(RayColorParams{}) - uintptr(C.sizeof_rt_ray_color_params)]byte
	_ [uintptr(C.sizeof_rt_ray_color_params) - unsafe.Sizeof(RayColorParams{})]byte
	_ [unsafe.Sizeof(RayColorStats{}) - uintptr(C.sizeof_rt_ray_color_stats)]byte
	_ [uintptr(C.sizeof_rt_ray_color_stats) - unsafe.Sizeof(RayColorStats{})]byte
	_ [unsafe.Sizeof(Ray{}) - uintptr(C.sizeof_rt_ray)]byte
	_ [uintptr(C.sizeof_rt_ray) - unsafe.Sizeof(Ray{})]byte
	_ [unsafe.Sizeof(RayHit{}) - uintptr(C.sizeof_rt_ray_hit)]byte
	_ [uintptr(C.sizeof_rt_ray_hit) - unsafe.Sizeof(RayHit{})]byte
	_ [unsafe.Sizeof(AdaptiveParams{}) - uintptr(C.sizeof_rt_adaptive_params)]byte
	_ [uintptr(C.sizeof_rt_adaptive_params) - unsafe.Sizeof(AdaptiveParams{})]byte
	_ [unsafe.Sizeof(AdaptiveStats{}) - uintptr(C.sizeof_rt_adaptive_stats)]byte
	_ [uintptr(C.sizeof_rt_adaptive_stats) - unsafe.Sizeof(AdaptiveStats{})]byte
	_ [unsafe.Sizeof(DenoiseVarParams{}) - uintptr(C.sizeof_rt_denoise_var_params)]byte
	_ [uintptr(C.sizeof_rt_denoise_var_params) - unsafe.Sizeof(DenoiseVarParams{})]byte
	_ [unsafe.Sizeof(DenoiseParams{}) - uintptr(C.sizeof_rt_denoise_params)]byte
	_ [uintptr(C.sizeof_rt_denoise_params) - unsafe.Sizeof(DenoiseParams{})]byte
	_ [unsafe.Sizeof(Node{}) - uintptr(C.sizeof_rt_hittable)]byte
	_ [uintptr(C.sizeof_rt_hittable) - unsafe.Sizeof(Node{})]byte
	_ [unsafe.Sizeof(Material{}) - uintptr(C.sizeof_rt_material)]byte
	_ [uintptr(C.sizeof_rt_material) - unsafe.Sizeof(Material{})]byte
	_ [unsafe.Sizeof(Texture{}) - uintptr(C.sizeof_rt_texture)]byte
	_ [uintptr(C.sizeof_rt_texture) - unsafe.Sizeof(Texture{})]byte
	_ [unsafe.Sizeof(Perlin{}) - uintptr(C.sizeof_rt_perlin)]byte
	_ [uintptr(C.sizeof_rt_perlin) - unsafe.Sizeof(Perlin{})]byte
	_ [unsafe.Sizeof(CameraDesc{}) - uintptr(C.sizeof_rt_camera_desc)]byte
	_ [uintptr(C.sizeof_rt_camera_desc) - unsafe.Sizeof(CameraDesc{})]byte
	_ [unsafe.Sizeof(Bucket{}) - uintptr(C.sizeof_rt_bucket)]byte
	_ [uintptr(C.sizeof_rt_bucket) - unsafe.Sizeof(Bucket{})]byte
	_ [unsafe.Sizeof(Stats{}) - uintptr(C.sizeof_rt_stats)]byte
	_ [uintptr(C.sizeof_rt_stats) - unsafe.Sizeof(Stats{})]byte
	_ [unsafe.Sizeof(SceneInfo{}) - uintptr(C.sizeof_rt_scene_info)]byte
	_ [uintptr(C.sizeof_rt_scene_info) - unsafe.Sizeof(SceneInfo{})]byte
)
