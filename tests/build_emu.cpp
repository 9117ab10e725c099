// Host emulation of the device BVH build (tests/test_device_build_host.py):
// build.hip's production kernels compiled for the host through
// tests/host_emu, one lane per launch index, in build_mesh_blas's sequence
// (k_morton, a stable sort on the 30 key bits in rocprim's place, k_karras,
// k_refit, the k_collapse level loop, k_gather) over exactly sized heap
// buffers under AddressSanitizer + UBSan.  The scratch arrays have the
// driver's sizes (n elements each) and the node and leaf arrays end at the
// capacity device_builds gives a job (base + n), so a write past either is a
// heap overflow.
//
//   build_emu N TRI_FIRST NODES_BASE LEAVES_BASE ORDER SEED in.bin out.bin
// in.bin:  frame lo[3], hi[3] (float), then N boxes of 8 floats (DRefBox).
// ORDER:   the lane order of every kernel launch: 0 ascending, 1 descending,
//          2 shuffled (SEED).
// out.bin: uint32 nodes_added, leaves_added, need4, levels; then
//          uint32 codes[N]              Morton code of triangle i
//          uint32 perm[N]               sorted position -> triangle
//          DNode4 nodes[NODES_BASE + N] (0xCD bytes where nothing was written)
//          DLeaf  leaves[LEAVES_BASE + N] (likewise)
//          uint32 entries[NODES_BASE + N] queue entries k_collapse consumed per node slot
//          int32  rank[TRI_FIRST + N]   tri_rank after k_gather (input: -1 below TRI_FIRST, then 0..N-1)
//          float  v0x[TRI_FIRST + N]    DTri::v0[0] after k_gather<DTri> (input: -1, then 0.5 + i)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../go-raytracing_amd/csrc/build.hip"

using namespace rtg;

static std::vector<uint32_t> lane_order(uint32_t count, int mode, uint32_t& seed) {
  std::vector<uint32_t> o(count);
  std::iota(o.begin(), o.end(), 0u);
  if (mode == 1) std::reverse(o.begin(), o.end());
  if (mode == 2)
    for (uint32_t i = count; i > 1; --i) {   // Fisher-Yates on an LCG
      seed = seed * 1664525u + 1013904223u;
      std::swap(o[i - 1], o[(seed >> 8) % i]);
    }
  return o;
}

template <class F>
static void launch(uint32_t count, int mode, uint32_t& seed, F&& lane) {
  gridDim = dim3(count);
  blockDim = dim3(1);
  threadIdx = dim3(0);
  for (uint32_t b : lane_order(count, mode, seed)) {
    blockIdx = dim3(b);
    lane();
  }
}

template <class T>
static bool put(FILE* f, const std::vector<T>& v) {
  return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  if (argc != 9) { fprintf(stderr, "usage: see the file comment\n"); return 2; }
  const uint32_t n = uint32_t(atoi(argv[1])), tri_first = uint32_t(atoi(argv[2]));
  const uint32_t nodes_base = uint32_t(atoi(argv[3])), leaves_base = uint32_t(atoi(argv[4]));
  const int mode = atoi(argv[5]);
  uint32_t seed = uint32_t(atoi(argv[6]));
  if (n <= kMaxLeaf || mode < 0 || mode > 2) return 2;
  float frame[6];
  std::vector<DRefBox> boxes(n);
  {
    FILE* f = fopen(argv[7], "rb");
    if (!f) return 2;
    const bool ok = fread(frame, sizeof(float), 6, f) == 6 && fread(boxes.data(), sizeof(DRefBox), n, f) == n;
    fclose(f);
    if (!ok) { fprintf(stderr, "short input\n"); return 2; }
  }

  // build_mesh_blas's scratch, at its sizes
  std::vector<uint32_t> keys_in(n), keys_out(n), vals_in(n), vals_out(n), flags(n, 0u), ctr(4);
  std::vector<uint2> child(n, uint2{0xCDCDCDCDu, 0xCDCDCDCDu}), range(n, uint2{0xCDCDCDCDu, 0xCDCDCDCDu});
  std::vector<int> parent_int(n, -2), parent_leaf(n, -2);
  const float nan = __builtin_nanf("");
  std::vector<DRefBox> node_box(n, DRefBox{{nan, nan, nan}, nan, {nan, nan, nan}, nan});
  std::vector<Entry> qa(n), qb(n);
  // the job's share of the scene arrays: nothing beyond base + n
  std::vector<DNode4> nodes(size_t(nodes_base) + n);
  std::vector<DLeaf> leaves(size_t(leaves_base) + n);
  memset(static_cast<void*>(nodes.data()), 0xCD, nodes.size() * sizeof(DNode4));
  memset(static_cast<void*>(leaves.data()), 0xCD, leaves.size() * sizeof(DLeaf));
  std::vector<uint32_t> entries(nodes.size(), 0u);

  float sc[3];   // the Morton frame, as build_mesh_blas derives it from the job
  for (int a = 0; a < 3; ++a) {
    const float ext = frame[3 + a] - frame[a];
    sc[a] = ext > 0.0f ? 1024.0f / ext : 0.0f;
  }
  launch(n, mode, seed, [&] {
    k_morton(boxes.data(), n, frame[0], frame[1], frame[2], sc[0], sc[1], sc[2], keys_in.data(), vals_in.data());
  });
  {   // rocprim::radix_sort_pairs over bits [0, 30): a stable sort
    std::vector<uint32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
      return (keys_in[a] & 0x3FFFFFFFu) < (keys_in[b] & 0x3FFFFFFFu);
    });
    for (uint32_t i = 0; i < n; ++i) { keys_out[i] = keys_in[idx[i]]; vals_out[i] = vals_in[idx[i]]; }
  }
  launch(n - 1, mode, seed, [&] {
    k_karras(keys_out.data(), int(n), child.data(), range.data(), parent_int.data(), parent_leaf.data());
  });
  launch(n, mode, seed, [&] {
    k_refit(int(n), vals_out.data(), boxes.data(), child.data(), parent_int.data(), parent_leaf.data(),
            node_box.data(), flags.data());
  });

  ctr[0] = 1u; ctr[1] = 0u; ctr[2] = 0u; ctr[3] = 0u;
  qa[0] = Entry{0u, nodes_base, 0, 0};
  uint32_t n_in = 1, levels = 0;
  Entry *in = qa.data(), *out = qb.data();
  for (; n_in > 0; ++levels) {
    if (levels > 200) { fprintf(stderr, "more than 200 levels\n"); return 4; }
    ctr[2] = 0u;
    for (uint32_t k = 0; k < n_in; ++k) {
      if (in[k].slot >= entries.size()) { fprintf(stderr, "queue entry with slot %u\n", in[k].slot); return 4; }
      ++entries[in[k].slot];
    }
    launch(n_in, mode, seed, [&] {
      k_collapse(in, n_in, out, &ctr[2], child.data(), range.data(), node_box.data(), boxes.data(), vals_out.data(),
                 nodes.data(), &ctr[0], nodes_base, leaves.data(), &ctr[1], leaves_base, tri_first,
                 reinterpret_cast<int*>(&ctr[3]));
    });
    n_in = ctr[2];
    std::swap(in, out);
  }

  // gather(): into a scratch of n, then copied back over [tri_first, tri_first + n)
  std::vector<int32_t> rank(size_t(tri_first) + n, -1), rank_tmp(n);
  std::vector<DTri> tris(size_t(tri_first) + n), tris_tmp(n);
  for (auto& t : tris) { t = DTri{}; t.v0[0] = -1.0f; }
  for (uint32_t i = 0; i < n; ++i) { rank[tri_first + i] = int32_t(i); tris[tri_first + i].v0[0] = 0.5f + float(i); }
  launch(n, mode, seed, [&] { k_gather<int32_t>(rank.data() + tri_first, rank_tmp.data(), vals_out.data(), n); });
  launch(n, mode, seed, [&] { k_gather<DTri>(tris.data() + tri_first, tris_tmp.data(), vals_out.data(), n); });
  std::copy(rank_tmp.begin(), rank_tmp.end(), rank.begin() + tri_first);
  std::copy(tris_tmp.begin(), tris_tmp.end(), tris.begin() + tri_first);
  std::vector<float> v0x(tris.size());
  for (size_t i = 0; i < tris.size(); ++i) v0x[i] = tris[i].v0[0];

  FILE* f = fopen(argv[8], "wb");
  if (!f) return 3;
  const std::vector<uint32_t> head{ctr[0], ctr[1], ctr[3], levels};
  const bool ok = put(f, head) && put(f, keys_in) && put(f, vals_out) && put(f, nodes) && put(f, leaves) &&
                  put(f, entries) && put(f, rank) && put(f, v0x);
  fclose(f);
  return ok ? 0 : 3;
}
