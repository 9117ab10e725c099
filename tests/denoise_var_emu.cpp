// Host emulation of the variance-guided denoiser (tests/test_denoise_var_host.py):
// denoise_var.hip's production kernels compiled for the host through
// tests/host_emu, one lane per block, every block of every kernel in turn,
// over exactly-sized buffers under AddressSanitizer + UBSan.  The kernel
// sequence is denoise_var.hip's own (dv_for_each_kernel), as
// launch_denoise_var runs it.
//
//   denoise_var_emu W H SPP ITER NPOW DEMOD SPATIAL_BELOW SIGMA_LUM SIGMA_DEPTH EPS
//                   in.f32 feat.f32 moments.f32|- out.f32 var.f32 [GRID]
// in/out: W*H*3 float sums, feat: W*H*8, moments: W*H*2 ("-": none), var: W*H.
// GRID blocks per kernel (default one per pixel; fewer exercise the
// grid-stride loops).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../go-raytracing_amd/csrc/denoise_var.hip"

using namespace rtg;

static bool read_f32(const char* path, std::vector<float>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const size_t got = fread(v.data(), sizeof(float), v.size(), f);
  fclose(f);
  return got == v.size();
}

static bool write_f32(const char* path, const std::vector<float>& v) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
  fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 16) { fprintf(stderr, "usage: see the file comment\n"); return 2; }
  const int w = atoi(argv[1]), h = atoi(argv[2]), spp = atoi(argv[3]), iters = atoi(argv[4]);
  const int spatial_below = atoi(argv[7]);
  if (w <= 0 || h <= 0 || spp <= 0 || iters < 0 || iters > kDvMaxIterations || spatial_below < 2) return 2;
  const bool have_mom = strcmp(argv[13], "-") != 0;
  const bool spatial = spp < spatial_below;
  if (!spatial && !have_mom) return 2;   // rt_denoise_variance refuses it
  const size_t n = size_t(w) * size_t(h);
  std::vector<float> in(n * 3), feat(n * 8), mom(have_mom ? n * 2 : 0), out(n * 3), var(n);
  if (!read_f32(argv[11], in) || !read_f32(argv[12], feat) || (have_mom && !read_f32(argv[13], mom))) {
    fprintf(stderr, "short input\n");
    return 2;
  }
  const uint32_t grid = argc > 16 ? uint32_t(atoi(argv[16])) : uint32_t(n);
  std::vector<float4> guide(n), img0(n), img1(n);
  std::vector<float> var0(n), var1(n);
  DvArgs a{};
  a.accum = in.data(); a.feat = feat.data(); a.moments = spatial ? nullptr : mom.data();
  a.out = out.data(); a.out_var = var.data();
  a.guide = guide.data(); a.img[0] = img0.data(); a.img[1] = img1.data();
  a.var[0] = var0.data(); a.var[1] = var1.data();
  a.w = w; a.h = h; a.spp = float(spp);
  a.normal_power_log2 = atoi(argv[5]); a.demodulate = atoi(argv[6]);
  a.spatial = spatial ? 1 : 0;
  a.sigma_lum = float(atof(argv[8])); a.sigma_depth = float(atof(argv[9])); a.albedo_eps = float(atof(argv[10]));
  gridDim = dim3(grid);
  blockDim = dim3(1);
  threadIdx = dim3(0);
  auto each_block = [&](auto&& kernel) {
    for (uint32_t b = 0; b < grid; ++b) {
      blockIdx = dim3(b);
      kernel();
    }
  };
  dv_for_each_kernel(
      a, iters, [&] { each_block([&] { k_dv_prepare(a); }); }, [&] { each_block([&] { k_dv_spatial(a); }); },
      [&](bool last, const DvPass& ps) {
        each_block([&] {
          if (last) k_dv_atrous<true>(a, ps);
          else k_dv_atrous<false>(a, ps);
        });
      });
  if (iters == 0) {   // rt_denoise_variance: the input, and the initial variance
    out = in;
    var = var0;
  }
  if (!write_f32(argv[14], out) || !write_f32(argv[15], var)) return 3;
  return 0;
}
