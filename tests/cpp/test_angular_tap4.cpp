// Host walks of the angular family with VVC's 4-tap luma interpolation (vvc-mip-gpu_amd/csrc/
// angular_plan.h: ang_cubic, ang_gauss, ang_filter_gauss, ang_block_tap4_class, ang_sample_tap4 and
// the interp argument of angular_frames_host, angular_refine_frames_host, angular_cu_host and
// angular_predict_cu_host) as a stand-alone program: tests/test_angular_tap4_cpu.py writes frames,
// the two length arrays and a set of (list, seeds) jobs to a file, this program runs the walks with
// MIP_ANG_INTERP_4TAP on exactly frame-sized arrays and writes every output back; the test compares
// them with tests/angular_tap4_ref.py.  Built with -fsanitize=address,undefined.
//
//   test_angular_tap4 run IN OUT
//   IN : int32 width, height, nframes, bias, njobs, extended (0: the walks get no length arrays);
//        uint16 frames[nframes][H][W]; uint16 refs[nframes][H][W]; uint8 unavail[nctus*5380];
//        uint8 ext_top, ext_left [nctus*5380]; uint8 best_mode[nframes][nctus*5380];
//        int32 best_cost[nframes][nctus*5380];
//        per job: int32 seeds (0: the plain walk), nmodes (0: all); uint8 modes[nmodes]
//   OUT: per job int32 cost, sad, satd [nframes][nctus*5380][65]; uint8 ang_mode; int32 ang_cost;
//        uint8 tried (0x5a throughout for the plain walk); uint8 best_mode; int32 best_cost (merged)
//   Per job the per-sample predictor (ang_sample_tap4 through angular_predict_cu_host) is held to
//   the block step's SAD on every 53rd available CU of the first frame; the walks are held to their
//   argument rule (an unknown interp is refused, nothing written); with the default interp the
//   walks give what they give without the argument.
//
//   test_angular_tap4 tables
//   Prints G for lw, lh = 2..6 and m = 2..66 (25 lines of 65 digits), then the 64 coefficient
//   quadruples of ang_coef_word as unpacked by ang_coef (cubic f = 0..31, Gaussian f = 0..31).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "angular_plan.h"

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE *f, const T *p, size_t n) { return fwrite(p, sizeof(T), n, f) == n; }

using namespace mipgpu;

static int print_tables() {
  for (int lw = 2; lw <= 6; lw++)
    for (int lh = 2; lh <= 6; lh++) {
      for (int m = MIP_ANGULAR_FIRST; m <= MIP_ANGULAR_LAST; m++) putchar(ang_filter_gauss(m, lw, lh) ? '1' : '0');
      putchar('\n');
    }
  for (int k = 0; k < kAngCoefWords; k++) {
    const uint32_t w = ang_coef_word(k >> 5, k & 31);
    if (AngCoefTable{}(k >> 5, k & 31) != w) return 3;
    printf("%d %d %d %d\n", ang_coef(w, 0), ang_coef(w, 1), ang_coef(w, 2), ang_coef(w, 3));
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && std::string(argv[1]) == "tables") return print_tables();
  if (argc != 4 || std::string(argv[1]) != "run") return 2;
  FILE *in = fopen(argv[2], "rb");
  if (!in) return 2;
  int32_t hdr[6];
  if (!rd(in, hdr, 6)) return 2;
  const int w = hdr[0], h = hdr[1], nf = hdr[2], bias = hdr[3], njobs = hdr[4];
  const bool extended = hdr[5] != 0;
  const int cols = (w + 127) / 128;
  const size_t fs = (size_t)w * h, ncu = (size_t)cols * ((h + 127) / 128) * MIP_CUS_PER_CTU;
  // (exact-size heap arrays: a read past a frame's end is an AddressSanitizer report)
  std::vector<uint16_t> frames(nf * fs), refs(nf * fs);
  std::vector<uint8_t> unavail(ncu), et(ncu), el(ncu), mode0(nf * ncu);
  std::vector<int32_t> best0(nf * ncu);
  if (!rd(in, frames.data(), frames.size()) || !rd(in, refs.data(), refs.size()) || !rd(in, unavail.data(), ncu) ||
      !rd(in, et.data(), ncu) || !rd(in, el.data(), ncu) || !rd(in, mode0.data(), mode0.size()) || !rd(in, best0.data(), best0.size()))
    return 2;
  const uint8_t *top = extended ? et.data() : nullptr, *left = extended ? el.data() : nullptr;
  FILE *out = fopen(argv[3], "wb");
  if (!out) return 2;
  for (int job = 0; job < njobs; job++) {
    int32_t js[2];
    if (!rd(in, js, 2) || js[1] < 0 || js[1] > 65) return 2;
    std::vector<uint8_t> list(js[1]);
    if (!rd(in, list.data(), list.size())) return 2;
    const uint8_t *modes = js[1] ? list.data() : nullptr;
    std::vector<int32_t> cost(nf * ncu * 65, -7), sad(cost), satd(cost), ang_cost(nf * ncu, -7), best(best0);
    std::vector<uint8_t> ang_mode(nf * ncu, 0x5a), tried(nf * ncu, 0x5a), mode(mode0);
    // an unknown interp: refused, nothing written
    if (angular_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, modes, js[1], cost.data(), nullptr, nullptr, nullptr,
                            nullptr, 0, nullptr, nullptr, top, left, 2) == 0 ||
        angular_refine_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, modes, js[1], 1, cost.data(), nullptr, nullptr,
                                   nullptr, nullptr, nullptr, 0, nullptr, nullptr, top, left, -1) == 0 ||
        cost[0] != -7)
      return 3;
    const int rc = js[0] ? angular_refine_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, modes, js[1], js[0], cost.data(),
                                                      sad.data(), satd.data(), ang_mode.data(), ang_cost.data(), tried.data(), bias,
                                                      mode.data(), best.data(), top, left, MIP_ANG_INTERP_4TAP)
                         : angular_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, modes, js[1], cost.data(), sad.data(),
                                               satd.data(), ang_mode.data(), ang_cost.data(), bias, mode.data(), best.data(), top, left,
                                               MIP_ANG_INTERP_4TAP);
    if (rc != 0) return 4;
    if (job == 0) {  // MIP_ANG_INTERP_2TAP named equals the argument left out (first frame, the cost table)
      std::vector<int32_t> a(ncu * 65, -7), b(a);
      if (angular_frames_host(frames.data(), refs.data(), unavail.data(), w, h, 1, modes, js[1], a.data(), nullptr, nullptr, nullptr, nullptr,
                              0, nullptr, nullptr, top, left, MIP_ANG_INTERP_2TAP) != 0 ||
          angular_frames_host(frames.data(), refs.data(), unavail.data(), w, h, 1, modes, js[1], b.data(), nullptr, nullptr, nullptr, nullptr,
                              0, nullptr, nullptr, top, left) != 0 ||
          a != b)
        return 6;
    }
    // the per-sample predictor gives the walk's SAD (first frame, every 53rd available CU, every
    // mode the CU's table holds)
    size_t k = 0, seen = 0;
    for (size_t c = 0; c < ncu / MIP_CUS_PER_CTU; c++)
      for (int s = 0; s < MIP_NUM_SHAPES; s++) {
        const mip_shape_desc &sd = kIntraShapes[s];
        for (int cu = 0; cu < sd.ncu; cu++, k++) {
          if (unavail[k] || seen++ % 53) continue;
          const int x = 128 * (int)(c % cols) + intra_axis(sd.xb, sd.xs, sd.xd, cu % sd.ncols);
          const int y = 128 * (int)(c / cols) + intra_axis(sd.yb, sd.ys, sd.yd, cu / sd.ncols);
          std::vector<uint16_t> blk((size_t)sd.w * sd.h);
          for (int m = MIP_ANGULAR_FIRST; m <= MIP_ANGULAR_LAST; m++) {
            if (sad[k * 65 + m - 2] == MIP_COST_UNAVAILABLE) continue;
            angular_predict_cu_host(refs.data(), w, x, y, intra_log2(sd.w), intra_log2(sd.h), m, blk.data(), sd.w, extended ? et[k] : 0,
                                    extended ? el[k] : 0, MIP_ANG_INTERP_4TAP);
            int32_t sum = 0;
            for (int j = 0; j < sd.h; j++)
              for (int i = 0; i < sd.w; i++) sum += intra_abs((int)frames[(size_t)(y + j) * w + x + i] - (int)blk[(size_t)j * sd.w + i]);
            if (sum != sad[k * 65 + m - 2]) return 5;
          }
        }
      }
    if (!(wr(out, cost.data(), cost.size()) && wr(out, sad.data(), sad.size()) && wr(out, satd.data(), satd.size()) &&
          wr(out, ang_mode.data(), ang_mode.size()) && wr(out, ang_cost.data(), ang_cost.size()) && wr(out, tried.data(), tried.size()) &&
          wr(out, mode.data(), mode.size()) && wr(out, best.data(), best.size())))
      return 2;
  }
  fclose(in);
  fclose(out);
  printf("angular_tap4: ok\n");
  return 0;
}
