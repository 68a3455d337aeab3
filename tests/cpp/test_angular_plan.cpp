// Host walk of the angular intra costs (vvc-mip-gpu_amd/csrc/angular_plan.h) as a stand-alone
// program: tests/test_angular_plan.py writes frames to a file, this program runs
// angular_frames_host (the arithmetic the kernel runs one lane per 4x4 block: tables, best
// angular mode, merge) and writes every output back; the test compares them with
// tests/angular_ref.py.  It also checks the argument rules, the per-sample predictor against
// the per-block step, and lists the CUs whose corner sample an engine filter leaves undefined
// (work_plan.h filter_poison).  Built with -fsanitize=address,undefined as well.
//
//   test_angular_plan run IN OUT
//   IN : int32 width, height, nframes, bias, nmodes (0: all); uint8 modes[nmodes];
//        uint16 frames[nframes][H][W]; uint16 refs[nframes][H][W]; uint8 unavail[nctus*5380];
//        uint8 best_mode[nframes][nctus*5380]; int32 best_cost[nframes][nctus*5380]
//   OUT: int32 cost, sad, satd [nframes][nctus*5380][65]; uint8 ang_mode; int32 ang_cost;
//        uint8 best_mode; int32 best_cost (merged)
//   test_angular_plan corner W H [W H ...]
//   prints "W H filter cu" for every CU (index inside the frame's CU list) with x > 0 and y > 0
//   whose corner sample is in the undefined set of that filter (0..7)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "angular_plan.h"
#include "work_plan.h"

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE *f, const T *p, size_t n) { return fwrite(p, sizeof(T), n, f) == n; }

static int corners(int argc, char **argv) {
  using namespace mipgpu;
  for (int at = 2; at + 1 < argc; at += 2) {
    const int w = atoi(argv[at]), h = atoi(argv[at + 1]);
    if (w <= 0 || h <= 0 || w % 4 || h % 4) return 2;
    const int cols = (w + 127) / 128, nctus = cols * ((h + 127) / 128);
    for (int filter = 0; filter < 8; filter++) {
      const Poison ps = filter_poison(w, h, filter);
      if (!ps.any) continue;
      for (int c = 0; c < nctus; c++) {
        int k = 0;
        for (int s = 0; s < MIP_NUM_SHAPES; s++) {
          const mip_shape_desc &sd = kShapes[s];
          for (int cu = 0; cu < sd.ncu; cu++, k++) {
            const int x = 128 * (c % cols) + axis_pos(sd.xb, sd.xs, sd.xd, cu % sd.ncols);
            const int y = 128 * (c / cols) + axis_pos(sd.yb, sd.ys, sd.yd, cu / sd.ncols);
            if (x > 0 && y > 0 && ps.at((long long)(y - 1) * w + x - 1, w)) printf("%d %d %d %d\n", w, h, filter, c * MIP_CUS_PER_CTU + k);
          }
        }
      }
    }
  }
  printf("corners: ok\n");
  return 0;
}

// The tables' angles and inverses, the packing, and the list rules.
static bool rules_ok() {
  using namespace mipgpu;
  for (int m = MIP_ANGULAR_FIRST; m <= MIP_ANGULAR_LAST; m++) {
    const int a = ang_angle(m), inv = ang_inverse(m);
    if (a < -32 || a > 32 || ang_angle(68 - m) != a) return false;  // the classes mirror at mode 34
    if (a && inv != (16384 + (a < 0 ? -a : a) / 2) / (a < 0 ? -a : a)) return false;
    if (!a && (inv != 0 || (m != 18 && m != 50))) return false;
    const AngMode md = ang_unpack(ang_pack(m));
    if (md.m != m || md.angle != a || md.inv != inv) return false;
    const int code = MIP_MODE_ANGULAR(m);
    if (code < 0x82 || code > 0xc2 || code == MIP_MODE_PLANAR || code == MIP_MODE_DC) return false;
  }
  if (ang_angle(2) != 32 || ang_angle(34) != -32 || ang_angle(66) != 32 || ang_angle(19) != -1 || ang_angle(51) != 1) return false;
  AngList l;
  const uint8_t good[3] = {18, 34, 50}, same[2] = {20, 20}, down[2] = {21, 20}, low[1] = {1}, high[1] = {67};
  uint8_t all[66];
  for (int q = 0; q < 66; q++) all[q] = (uint8_t)(2 + q);
  if (!ang_list(nullptr, 0, &l) || l.n != 65 || !ang_list(good, 3, &l) || l.n != 3 || !ang_list(all, 65, &l)) return false;
  if (!ang_list(good, 3, &l) || !ang_listed(l.listed, 16) || !ang_listed(l.listed, 32) || !ang_listed(l.listed, 48) || ang_listed(l.listed, 0) ||
      ang_listed(l.listed, 64))
    return false;
  if (ang_list(nullptr, 3, &l) || ang_list(good, 0, &l) || ang_list(good, -1, &l) || ang_list(all, 66, &l) || ang_list(same, 2, &l) ||
      ang_list(down, 2, &l) || ang_list(low, 1, &l) || ang_list(high, 1, &l))
    return false;
  return ang_bias_ok(0) && ang_bias_ok(kAngMaxBias) && !ang_bias_ok(-1) && !ang_bias_ok(kAngMaxBias + 1);
}

int main(int argc, char **argv) {
  if (argc >= 2 && std::string(argv[1]) == "corner") return corners(argc, argv);
  if (argc != 4 || std::string(argv[1]) != "run") return 2;
  if (!rules_ok()) return 6;
  FILE *in = fopen(argv[2], "rb");
  if (!in) return 2;
  int32_t hdr[5];
  if (!rd(in, hdr, 5)) return 2;
  const int w = hdr[0], h = hdr[1], nf = hdr[2], bias = hdr[3], nmodes = hdr[4];
  const size_t fs = (size_t)w * h, ncu = (size_t)((w + 127) / 128) * ((h + 127) / 128) * MIP_CUS_PER_CTU;
  // (exact-size heap arrays: a read past a frame's end is an AddressSanitizer report)
  std::vector<uint8_t> list(nmodes);
  std::vector<uint16_t> frames(nf * fs), refs(nf * fs);
  std::vector<uint8_t> unavail(ncu), mode(nf * ncu);
  std::vector<int32_t> best(nf * ncu);
  if (!rd(in, list.data(), list.size()) || !rd(in, frames.data(), frames.size()) || !rd(in, refs.data(), refs.size()) ||
      !rd(in, unavail.data(), ncu) || !rd(in, mode.data(), mode.size()) || !rd(in, best.data(), best.size()))
    return 2;
  fclose(in);
  const uint8_t *modes = nmodes ? list.data() : nullptr;
  using mipgpu::angular_frames_host;

  // argument rules (before any work): no output, half a pair, a bad list, a bad bias
  std::vector<int32_t> cost(nf * ncu * 65, -7), sad(cost), satd(cost), ang_cost(nf * ncu, -7);
  std::vector<uint8_t> ang_mode(nf * ncu, 0x5a);
  const uint8_t twice[2] = {30, 30};
  const std::vector<uint8_t> mode0 = mode;
  const std::vector<int32_t> best0 = best;
#define WALK(m, n, c, am, ac, b, bm, bc) \
  angular_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, m, n, c, nullptr, nullptr, am, ac, b, bm, bc)
  if (WALK(modes, nmodes, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == 0) return 3;
  if (WALK(modes, nmodes, cost.data(), ang_mode.data(), nullptr, 0, nullptr, nullptr) == 0) return 3;
  if (WALK(modes, nmodes, cost.data(), nullptr, nullptr, 0, mode.data(), nullptr) == 0) return 3;
  if (WALK(twice, 2, cost.data(), ang_mode.data(), ang_cost.data(), 0, mode.data(), best.data()) == 0) return 3;
  if (WALK(modes, 66, cost.data(), ang_mode.data(), ang_cost.data(), 0, mode.data(), best.data()) == 0) return 3;
  if (WALK(modes, nmodes, cost.data(), ang_mode.data(), ang_cost.data(), -1, mode.data(), best.data()) == 0) return 3;
  if (WALK(modes, nmodes, cost.data(), ang_mode.data(), ang_cost.data(), (1 << 20) + 1, mode.data(), best.data()) == 0) return 3;
  if (cost[0] != -7 || ang_cost[0] != -7 || ang_mode[0] != 0x5a || mode != mode0 || best != best0) return 3;
#undef WALK

  if (angular_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, modes, nmodes, cost.data(), sad.data(), satd.data(),
                          ang_mode.data(), ang_cost.data(), bias, mode.data(), best.data()) != 0)
    return 4;
  // one table alone gives the same values
  std::vector<int32_t> only(nf * ncu * 65, -7);
  if (angular_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, modes, nmodes, nullptr, nullptr, only.data(), nullptr,
                          nullptr, 0, nullptr, nullptr) != 0 ||
      only != satd)
    return 5;
  // the per-sample predictor (the contract's formula as written) gives the per-block step's SAD,
  // on every 53rd available CU of the first frame and every listed mode
  {
    using namespace mipgpu;
    const int cols = (w + 127) / 128;
    AngList l;
    if (!ang_list(modes, nmodes, &l)) return 7;
    size_t k = 0, seen = 0;
    for (size_t c = 0; c < ncu / MIP_CUS_PER_CTU; c++)
      for (int s = 0; s < MIP_NUM_SHAPES; s++) {
        const mip_shape_desc &sd = kIntraShapes[s];
        for (int cu = 0; cu < sd.ncu; cu++, k++) {
          if (unavail[k] || seen++ % 53) continue;
          const int x = 128 * (int)(c % cols) + intra_axis(sd.xb, sd.xs, sd.xd, cu % sd.ncols);
          const int y = 128 * (int)(c / cols) + intra_axis(sd.yb, sd.ys, sd.yd, cu / sd.ncols);
          std::vector<uint16_t> blk((size_t)sd.w * sd.h);
          for (int q = 0; q < l.n; q++) {
            const int m = ang_unpack(l.packed[q]).m;
            angular_predict_cu_host(refs.data(), w, x, y, intra_log2(sd.w), intra_log2(sd.h), m, blk.data(), sd.w);
            int32_t sum = 0;
            for (int j = 0; j < sd.h; j++)
              for (int i = 0; i < sd.w; i++) sum += intra_abs((int)frames[(size_t)(y + j) * w + x + i] - (int)blk[(size_t)j * sd.w + i]);
            if (sum != sad[k * 65 + m - 2]) return 7;
          }
        }
      }
  }
  FILE *out = fopen(argv[3], "wb");
  if (!out) return 2;
  const bool ok = wr(out, cost.data(), cost.size()) && wr(out, sad.data(), sad.size()) && wr(out, satd.data(), satd.size()) &&
                  wr(out, ang_mode.data(), ang_mode.size()) && wr(out, ang_cost.data(), ang_cost.size()) &&
                  wr(out, mode.data(), mode.size()) && wr(out, best.data(), best.size());
  fclose(out);
  if (!ok) return 2;
  printf("angular_plan: ok\n");
  return 0;
}
