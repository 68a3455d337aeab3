// Host walk of the Planar / DC baseline costs (vvc-mip-gpu_amd/csrc/intra_plan.h) as a
// stand-alone program: tests/test_intra_plan.py writes frames to a file, this program runs
// intra_frames_host and intra_merge_host (the arithmetic the kernel runs one lane per 4x4
// block) and writes every output back; the test compares them with tests/intra_ref.py.  It also
// checks the kernel's lane-slot lists against the shape table.  Built with
// -fsanitize=address,undefined as well.
//
//   test_intra_plan IN OUT
//   IN : int32 width, height, nframes, bias[2]; uint16 frames[nframes][H][W];
//        uint16 refs[nframes][H][W]; uint8 unavail[nctus*5380];
//        uint8 best_mode[nframes][nctus*5380]; int32 best_cost[nframes][nctus*5380]
//   OUT: int32 cost, sad, satd [nframes][nctus*5380][2]; uint8 best_mode; int32 best_cost (merged)
#include <cstdio>
#include <vector>

#include "intra_plan.h"

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE *f, const T *p, size_t n) { return fwrite(p, sizeof(T), n, f) == n; }

// Every CU but the 64x64 ones owns exactly its 4x4 blocks, each once, row-major, in an aligned
// group of one wave, inside its 32x32 block.
static bool slots_ok() {
  using namespace mipgpu;
  int per = 0;
  const std::vector<uint32_t> slots = intra_build_slots(&per);
  if (slots.empty() || per < 64 || per % 64 || slots.size() != (size_t)kIntraBlocks * per) return false;
  std::vector<int> seen(MIP_CUS_PER_CTU, 0);
  for (int b = 0; b < kIntraBlocks; b++)
    for (int at = 0; at < per; at++) {
      const uint32_t word = slots[(size_t)b * per + at];
      if (word & kIntraNoSlot) continue;
      const IntraSlot c = intra_slot_decode(word);
      const int n = 1 << (c.lw + c.lh - 4), t = at % n;
      if (n > 64 || c.cu < 4 || c.cu >= MIP_CUS_PER_CTU) return false;
      if (c.bi != t % (1 << (c.lw - 2)) || c.bj != t / (1 << (c.lw - 2))) return false;
      if (slots[(size_t)b * per + at - t] != (word & ~(0x3fu << 13))) return false;  // the group's first slot: same CU
      if (4 * c.cx + (1 << c.lw) > 32 || 4 * c.cy + (1 << c.lh) > 32) return false;
      seen[c.cu]++;
    }
  int k = 0;
  for (int s = 0; s < MIP_NUM_SHAPES; s++) {
    const mip_shape_desc &sd = kIntraShapes[s];
    for (int cu = 0; cu < sd.ncu; cu++, k++)
      if (seen[k] != (sd.w == 64 && sd.h == 64 ? 0 : (sd.w / 4) * (sd.h / 4))) return false;
  }
  return k == MIP_CUS_PER_CTU;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  if (!slots_ok()) return 6;
  FILE *in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t hdr[5];
  if (!rd(in, hdr, 5)) return 2;
  const int w = hdr[0], h = hdr[1], nf = hdr[2];
  const size_t fs = (size_t)w * h, ncu = (size_t)((w + 127) / 128) * ((h + 127) / 128) * MIP_CUS_PER_CTU;
  // (exact-size heap arrays: a read past a frame's end is an AddressSanitizer report)
  std::vector<uint16_t> frames(nf * fs), refs(nf * fs);
  std::vector<uint8_t> unavail(ncu), mode(nf * ncu);
  std::vector<int32_t> best(nf * ncu);
  if (!rd(in, frames.data(), frames.size()) || !rd(in, refs.data(), refs.size()) || !rd(in, unavail.data(), ncu) ||
      !rd(in, mode.data(), mode.size()) || !rd(in, best.data(), best.size()))
    return 2;
  fclose(in);

  // argument rules (before any work)
  std::vector<int32_t> cost(nf * ncu * 2, -7), sad(cost), satd(cost);
  if (mipgpu::intra_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, nullptr, nullptr, nullptr) == 0) return 3;
  if (mipgpu::intra_frames_host(frames.data(), refs.data(), nullptr, w, h, nf, cost.data(), nullptr, nullptr) == 0) return 3;
  if (mipgpu::intra_frames_host(frames.data(), refs.data(), unavail.data(), w + 2, h, nf, cost.data(), nullptr, nullptr) == 0) return 3;
  const int32_t low[2] = {-1, 0}, high[2] = {0, mipgpu::kIntraMaxBias + 1}, edge[2] = {mipgpu::kIntraMaxBias, 0};
  if (mipgpu::intra_bias_ok(low) || mipgpu::intra_bias_ok(high) || !mipgpu::intra_bias_ok(edge) || !mipgpu::intra_bias_ok(nullptr)) return 3;
  if (cost[0] != -7) return 3;

  if (mipgpu::intra_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, cost.data(), sad.data(), satd.data()) != 0) return 4;
  // each table alone gives the same values
  std::vector<int32_t> only(nf * ncu * 2, -7);
  if (mipgpu::intra_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, nullptr, nullptr, only.data()) != 0 || only != satd)
    return 5;
  mipgpu::intra_merge_host(cost.data(), nf * ncu, hdr + 3, mode.data(), best.data());
  FILE *out = fopen(argv[2], "wb");
  if (!out) return 2;
  const bool ok = wr(out, cost.data(), cost.size()) && wr(out, sad.data(), sad.size()) && wr(out, satd.data(), satd.size()) &&
                  wr(out, mode.data(), mode.size()) && wr(out, best.data(), best.size());
  fclose(out);
  if (!ok) return 2;
  printf("intra_plan: ok\n");
  return 0;
}
