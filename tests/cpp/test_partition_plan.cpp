// Host restatement of the partition decision (vvc-mip-gpu_amd/csrc/partition_plan.h) as a
// stand-alone program: tests/test_partition_cpu.py writes per-CU costs to a file, this program
// partitions them with partition_frames (the walk the kernel runs level by level) and writes
// every output back; the test compares them with tests/partition_ref.py.  Built with
// -fsanitize=address,undefined as well.
//
//   test_partition_plan IN OUT
//   IN : int32 width, height, nframes, has_penalty; int32 penalty[47];
//        int32 best_cost[nframes][nctus*5380]; uint8 best_mode[nframes][nctus*5380]
//   OUT: uint8 leaf[nframes][nctus*5380]; int32 ctu_cost[nframes][nctus];
//        int32 ctu_leaves[nframes][nctus]; mip_pred_item items[nframes][nctus][1024]
#include <cstdio>
#include <vector>

#include "partition_plan.h"

static_assert(sizeof(mip_pred_item) == 24, "mip_pred_item layout");
static_assert(sizeof(mip_part_state) == 8 && sizeof(mip_part_step) == 12, "table records");

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE *f, const T *p, size_t n) { return fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t hdr[4], pen[mipgpu::kPartShapes];
  if (!rd(in, hdr, 4) || !rd(in, pen, mipgpu::kPartShapes)) return 2;
  const int w = hdr[0], h = hdr[1], nf = hdr[2];
  const size_t nctus = (size_t)((w + 127) / 128) * ((h + 127) / 128), ncu = nctus * MIP_CUS_PER_CTU_ABI;
  std::vector<int32_t> cost(nf * ncu);
  std::vector<uint8_t> mode(nf * ncu);
  if (!rd(in, cost.data(), cost.size()) || !rd(in, mode.data(), mode.size())) return 2;
  fclose(in);

  // argument rules (before any work)
  std::vector<uint8_t> leaf(nf * ncu, 0xee);
  std::vector<int32_t> ctu_cost(nf * nctus, -7), ctu_leaves(nf * nctus, -7);
  std::vector<mip_pred_item> items(nf * nctus * MIP_PART_MAX_LEAVES);
  int32_t bad[mipgpu::kPartShapes] = {};
  bad[46] = mipgpu::kPartMaxPenalty + 1;
  if (mipgpu::partition_frames(cost.data(), mode.data(), w, h, nf, bad, leaf.data(), nullptr, nullptr, nullptr) == 0) return 3;
  bad[46] = -1;
  if (mipgpu::partition_frames(cost.data(), mode.data(), w, h, nf, bad, leaf.data(), nullptr, nullptr, nullptr) == 0) return 3;
  if (mipgpu::partition_frames(cost.data(), nullptr, w, h, nf, nullptr, nullptr, nullptr, nullptr, items.data()) == 0) return 3;
  if (mipgpu::partition_frames(cost.data(), mode.data(), w, h, nf, nullptr, nullptr, nullptr, nullptr, nullptr) == 0) return 3;
  if (leaf[0] != 0xee) return 3;

  if (mipgpu::partition_frames(cost.data(), mode.data(), w, h, nf, hdr[3] ? pen : nullptr, leaf.data(), ctu_cost.data(),
                               ctu_leaves.data(), items.data()) != 0)
    return 4;
  // each output alone gives the same values
  std::vector<int32_t> only(nf * nctus, -7);
  if (mipgpu::partition_frames(cost.data(), nullptr, w, h, nf, hdr[3] ? pen : nullptr, nullptr, only.data(), nullptr, nullptr) != 0 ||
      only != ctu_cost)
    return 5;
  FILE *out = fopen(argv[2], "wb");
  if (!out) return 2;
  const bool ok = wr(out, leaf.data(), leaf.size()) && wr(out, ctu_cost.data(), ctu_cost.size()) &&
                  wr(out, ctu_leaves.data(), ctu_leaves.size()) && wr(out, items.data(), items.size());
  fclose(out);
  if (!ok) return 2;
  printf("partition_plan: ok\n");
  return 0;
}
