// Host emulation of the denoiser (tests/test_denoise_host.py): denoise.hip's
// production kernels compiled for the host through tests/host_emu, one lane
// per block, every block of every pass in turn, over exactly-sized buffers
// under AddressSanitizer + UBSan.  The pass sequence is denoise.hip's own
// (dn_for_each_pass), as launch_denoise runs it.
//
//   denoise_emu W H SPP ITER NPOW DEMOD SIGMA_COLOR SIGMA_DEPTH EPS in.f32 feat.f32 out.f32 [GRID]
// in/out: W*H*3 float sums, feat: W*H*8.  GRID blocks per pass (default one
// per pixel; fewer exercise the grid-stride loop).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../go-raytracing_amd/csrc/denoise.hip"

using namespace rtg;

static bool read_f32(const char* path, std::vector<float>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const size_t got = fread(v.data(), sizeof(float), v.size(), f);
  fclose(f);
  return got == v.size();
}

int main(int argc, char** argv) {
  if (argc < 13) { fprintf(stderr, "usage: see the file comment\n"); return 2; }
  const int w = atoi(argv[1]), h = atoi(argv[2]), spp = atoi(argv[3]), iters = atoi(argv[4]);
  if (w <= 0 || h <= 0 || spp <= 0 || iters < 0 || iters > kDnMaxIterations) return 2;
  const size_t n = size_t(w) * size_t(h);
  std::vector<float> in(n * 3), feat(n * 8), out(n * 3);
  if (!read_f32(argv[10], in) || !read_f32(argv[11], feat)) { fprintf(stderr, "short input\n"); return 2; }
  const uint32_t grid = argc > 13 ? uint32_t(atoi(argv[13])) : uint32_t(n);
  if (iters == 0) {
    out = in;   // rt_denoise: a plain copy
  } else {
    std::vector<float4> guide(n), img0(n), img1(n);
    DnArgs a{};
    a.accum = in.data(); a.feat = feat.data(); a.out = out.data();
    a.guide = guide.data(); a.img[0] = img0.data(); a.img[1] = img1.data();
    a.w = w; a.h = h; a.spp = float(spp);
    a.normal_power_log2 = atoi(argv[5]); a.demodulate = atoi(argv[6]);
    a.sigma_color = float(atof(argv[7])); a.sigma_depth = float(atof(argv[8])); a.albedo_eps = float(atof(argv[9]));
    gridDim = dim3(grid);
    blockDim = dim3(1);
    threadIdx = dim3(0);
    dn_for_each_pass(a, iters, [&](bool first, bool last, const DnPass& ps) {
      for (uint32_t b = 0; b < grid; ++b) {
        blockIdx = dim3(b);
        if (first && last) k_atrous<true, true>(a, ps);
        else if (first) k_atrous<true, false>(a, ps);
        else if (last) k_atrous<false, true>(a, ps);
        else k_atrous<false, false>(a, ps);
      }
    });
  }
  FILE* f = fopen(argv[12], "wb");
  if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) return 3;
  fclose(f);
  return 0;
}
