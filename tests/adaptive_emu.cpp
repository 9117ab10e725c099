// Host emulation of the adaptive-sampling device code (tests/test_adaptive_host.py):
// adaptive.hip's production kernels compiled for the host through
// tests/host_emu, one lane per block, every block of every kernel in turn,
// over exactly-sized buffers under AddressSanitizer + UBSan.  The selection's
// kernel sequence is adaptive.hip's own (ad_for_each_kernel), as
// launch_adaptive_select runs it.
//
//   adaptive_emu select W H MAX_SPP CUR NEIGHBOURHOOD REL_ERROR LUM_FLOOR
//                moments.f32 counts.u32 list.u32 GRID
//     moments: W*H*2 floats, counts: W*H words; writes the list (its length
//     is the file's) and prints the length.
//   adaptive_emu normalize W H CHANNELS TARGET_SPP sums.f32 counts.u32 out.f32 GRID ALIAS
//     ALIAS 1: the kernel writes over its input.
// GRID blocks per kernel (fewer than pixels exercise the strided walks).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../go-raytracing_amd/csrc/adaptive.hip"

using namespace rtg;

template <class T>
static bool read_all(const char* path, std::vector<T>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  const size_t got = fread(v.data(), sizeof(T), v.size(), f);
  fclose(f);
  return got == v.size();
}

template <class T>
static bool write_all(const char* path, const T* p, size_t n) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(p, sizeof(T), n, f) == n;
  fclose(f);
  return ok;
}

template <class K>
static void each_block(uint32_t grid, K&& kernel) {
  gridDim = dim3(grid);
  blockDim = dim3(1);
  threadIdx = dim3(0);
  for (uint32_t b = 0; b < grid; ++b) {
    blockIdx = dim3(b);
    kernel();
  }
}

static int run_select(int argc, char** argv) {
  if (argc != 13) return 2;
  const int w = atoi(argv[2]), h = atoi(argv[3]);
  const uint32_t grid = uint32_t(atoi(argv[12]));
  if (w <= 0 || h <= 0 || grid == 0) return 2;
  const size_t n = size_t(w) * size_t(h);
  std::vector<float> mom(n * 2);
  std::vector<uint32_t> counts(n), list(n), blocks(grid), total(1);
  std::vector<uint8_t> flags(n);
  if (!read_all(argv[9], mom) || !read_all(argv[10], counts)) { fprintf(stderr, "short input\n"); return 2; }
  AdArgs a{};
  a.moments = mom.data(); a.counts = counts.data(); a.flags = flags.data();
  a.block_counts = blocks.data(); a.total = total.data(); a.list = list.data();
  a.w = w; a.h = h;
  a.max_spp = uint32_t(atoi(argv[4])); a.cur = uint32_t(atoi(argv[5]));
  a.neighbourhood = atoi(argv[6]);
  a.rel_error = float(atof(argv[7])); a.lum_floor = float(atof(argv[8]));
  ad_for_each_kernel([&] { each_block(grid, [&] { k_ad_flag(a); }); },
                     [&] { each_block(grid, [&] { k_ad_count(a); }); },
                     [&] { each_block(1, [&] { k_ad_scan(a.block_counts, grid, a.total); }); },
                     [&] { each_block(grid, [&] { k_ad_scatter(a); }); });
  if (total[0] > n) { fprintf(stderr, "list longer than the image\n"); return 3; }
  if (!write_all(argv[11], list.data(), total[0])) return 3;
  printf("%u\n", total[0]);
  return 0;
}

static int run_normalize(int argc, char** argv) {
  if (argc != 11) return 2;
  const int w = atoi(argv[2]), h = atoi(argv[3]), ch = atoi(argv[4]), target = atoi(argv[5]);
  const uint32_t grid = uint32_t(atoi(argv[9]));
  const bool alias = atoi(argv[10]) != 0;
  if (w <= 0 || h <= 0 || ch < 1 || ch > kAdMaxChannels || target < 1 || grid == 0) return 2;
  const size_t n = size_t(w) * size_t(h);
  std::vector<float> sums(n * size_t(ch)), out(alias ? 0 : n * size_t(ch));
  std::vector<uint32_t> counts(n);
  if (!read_all(argv[6], sums) || !read_all(argv[7], counts)) { fprintf(stderr, "short input\n"); return 2; }
  float* o = alias ? sums.data() : out.data();
  each_block(grid, [&] { k_normalize(sums.data(), ch, counts.data(), n, float(target), o); });
  return write_all(argv[8], o, n * size_t(ch)) ? 0 : 3;
}

int main(int argc, char** argv) {
  if (argc >= 2 && strcmp(argv[1], "select") == 0) return run_select(argc, argv);
  if (argc >= 2 && strcmp(argv[1], "normalize") == 0) return run_normalize(argc, argv);
  fprintf(stderr, "usage: see the file comment\n");
  return 2;
}
