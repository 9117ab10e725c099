// ray_emu.cpp — test-only: the production closest-hit kernel (wavefront.hip
// k_extend, a later bounce: rays read from the path stream) compiled for the
// host, one lane, over given rays.  Reads "ox oy oz dx dy dz" lines from
// stdin, prints "kind idx t(bits) inst refpos" per ray: the hit record
// k_extend stores (store_hit).  Used to replay single rays of a GPU render
// on the host (tools/format_diff.py finds them).  Not a product path.
//
// usage: ray_emu <scene> <width> <asset_dir>   (RTG_EMU_QUANT / RTG_EMU_FULL_LUCY as wave_emu)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../go-raytracing_amd/csrc/wavefront.hip"
#include "emu_scene.h"
#include "emu_trace.h"

using namespace rtg;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  emu::EmuScene E;
  if (int rc = emu::load(argv[1], atoi(argv[2]), argv[3], E)) return rc;
  const DScene& d = E.d;
  if (pick_variant(d).vol) {
    fprintf(stderr, "ray_emu: rare-primitive scenes are not supported\n");
    return 3;
  }
  emu::TraceArgs T(E.max_depth, int(E.d.stack_needed));
  float o[3], dd[3];
  while (scanf("%f %f %f %f %f %f", &o[0], &o[1], &o[2], &dd[0], &dd[1], &dd[2]) == 6) {
    const float4 h = emu::trace_path(E, T, o, dd);
    uint32_t w[4];
    memcpy(w, &h, 16);
    printf("%u %u %.9g %d %d\n", w[1] >> 28, w[1] & 0x0FFFFFFFu, double(h.x), int(w[2]), int(w[3]));
  }
  return T.err ? 6 : 0;
}
