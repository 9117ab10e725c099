// wave_emu.cpp — test-only host build of the production wavefront pipeline
// (go-raytracing_amd/csrc/wavefront.hip kernels: camera, extend, shade,
// shadow, NEE apply, accumulate, finalize) with one lane per workgroup and
// one workgroup per launch, driven like run_batches() over a librtscene scene
// flattened by flatten.cpp.  Runs under AddressSanitizer + UBSan in the CPU
// suite (tests/test_flatten_host.py): every stream / queue / job index the
// kernels compute is checked against exactly-sized host buffers.  The
// traversal stack ring is 4 entries so deep traversals take the spill path.
// Not a product path: the product is the gfx950 build in librtgpu.so.
//
// usage: wave_emu <scene> <width> <spp> <seed> <asset_dir> <out.f32> [batch_spp]
// writes H*W*3 float sums (the accumulation buffer rt_render returns).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../go-raytracing_amd/csrc/wavefront.hip"
#include "../go-raytracing_amd/csrc/wave_layout.h"
#include "emu_scene.h"
#include "wave_run.h"

using namespace rtg;

int main(int argc, char** argv) {
  if (argc < 7) return 2;
  const uint32_t spp = uint32_t(atoi(argv[3]));
  const uint32_t seed = uint32_t(strtoul(argv[4], nullptr, 10));
  const uint32_t spb = argc > 7 ? uint32_t(atoi(argv[7])) : spp;
  emu::EmuScene E;
  if (int rc = emu::load(argv[1], atoi(argv[2]), argv[5], E)) return rc;
  const DScene& d = E.d;
  const DCamera& cam = E.cam;
  // the pipeline itself, its buffers and its kernel variants: wave_run.h
  std::vector<float> out;
  size_t S = 0;
  const int err = wave_run::render(E, seed, 0u, spp, spb, E.max_depth, out, &S);
  FILE* f = fopen(argv[6], "wb");
  if (!f) return 5;
  fwrite(out.data(), sizeof(float), out.size(), f);
  fclose(f);
  printf("{\"width\": %d, \"height\": %d, \"slots\": %zu, \"overflow\": %d, \"wide\": %d, \"nodes8\": %zu, \"rgbe\": %d, "
         "\"lifted\": %d}\n",
         cam.width, cam.height, S, err, d.wide_nodes, E.h.nodes8.size(), d.env.rgbe != nullptr ? 1 : 0, d.num_prim_recs);
  return err ? 6 : 0;
}
