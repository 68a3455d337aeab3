// Host walks of the angular family with extended reference lines (vvc-mip-gpu_amd/csrc/
// angular_plan.h: ang_ext_lengths, AngExtView, the ext_top / ext_left arguments of
// angular_frames_host, angular_refine_frames_host and angular_predict_cu_host) as a stand-alone
// program: tests/test_angular_ext_cpu.py writes frames, the two length arrays and a set of
// (list, seeds) jobs to a file, this program runs the walks on exactly frame-sized arrays and
// writes every output back; the test compares them with tests/angular_ext_ref.py.  Built with
// -fsanitize=address,undefined.
//
//   test_angular_ext run IN OUT
//   IN : int32 width, height, nframes, bias, njobs; uint16 frames[nframes][H][W];
//        uint16 refs[nframes][H][W]; uint8 unavail[nctus*5380]; uint8 ext_top, ext_left [nctus*5380];
//        uint8 best_mode[nframes][nctus*5380]; int32 best_cost[nframes][nctus*5380];
//        per job: int32 seeds (0: the plain walk), nmodes (0: all); uint8 modes[nmodes]
//   OUT: per job int32 cost, sad, satd [nframes][nctus*5380][65]; uint8 ang_mode; int32 ang_cost;
//        uint8 tried (0x5a throughout for the plain walk); uint8 best_mode; int32 best_cost (merged)
//   Per job the per-sample predictor (angular_predict_cu_host with the lengths) is also held to the
//   walk's SAD on every 53rd available CU of the first frame, and the walks are held to their
//   argument rule (one length array alone is refused, nothing written).
//
//   test_angular_ext undefined IN
//   IN : int32 width, height, filter (-1..7); uint8 ext_top, ext_left [nctus*5380]
//   No sample of an extension is in the undefined set of that filter (work_plan.h filter_poison);
//   every length equals ang_ext_lengths over that set and work_plan.h's availability.  Prints the
//   number of extension samples looked at.
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

using namespace mipgpu;

static int undefined_samples(const char *path) {
  FILE *in = fopen(path, "rb");
  if (!in) return 2;
  int32_t hdr[3];
  if (!rd(in, hdr, 3)) return 2;
  const int w = hdr[0], h = hdr[1], filter = hdr[2];
  const int cols = (w + 127) / 128, nctus = cols * ((h + 127) / 128);
  const size_t ncu = (size_t)nctus * MIP_CUS_PER_CTU;
  std::vector<uint8_t> top(ncu), left(ncu);
  if (!rd(in, top.data(), ncu) || !rd(in, left.data(), ncu)) return 2;
  fclose(in);
  const Poison ps = filter_poison(w, h, filter);
  const auto undefined = [&](long long li) { return ps.any && ps.at(li, w); };
  long long seen = 0;
  size_t k = 0;
  for (int c = 0; c < nctus; c++)
    for (int s = 0; s < MIP_NUM_SHAPES; s++) {
      const mip_shape_desc &sd = kShapes[s];
      for (int cu = 0; cu < sd.ncu; cu++, k++) {
        const int x = 128 * (c % cols) + axis_pos(sd.xb, sd.xs, sd.xd, cu % sd.ncols);
        const int y = 128 * (c / cols) + axis_pos(sd.yb, sd.ys, sd.yd, cu / sd.ncols);
        for (int t = 0; t < top[k]; t++, seen++)
          if (y < 1 || x + sd.w + t >= w || undefined((long long)(y - 1) * w + x + sd.w + t)) return 3;
        for (int t = 0; t < left[k]; t++, seen++)
          if (x < 1 || y + sd.h + t >= h || undefined((long long)(y + sd.h + t) * w + x - 1)) return 3;
        const bool off = !cu_defined(w, h, x, y, sd.w, sd.h) || reads_poison(ps, w, x, y, sd.w, sd.h);
        const AngExt e = ang_ext_lengths(w, h, x, y, sd.w, sd.h, off, undefined);
        if (e.top != top[k] || e.left != left[k]) return 4;
      }
    }
  printf("undefined: ok %lld\n", seen);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && std::string(argv[1]) == "undefined") return undefined_samples(argv[2]);
  if (argc != 4 || std::string(argv[1]) != "run") return 2;
  FILE *in = fopen(argv[2], "rb");
  if (!in) return 2;
  int32_t hdr[5];
  if (!rd(in, hdr, 5)) return 2;
  const int w = hdr[0], h = hdr[1], nf = hdr[2], bias = hdr[3], njobs = hdr[4];
  const int cols = (w + 127) / 128;
  const size_t fs = (size_t)w * h, ncu = (size_t)cols * ((h + 127) / 128) * MIP_CUS_PER_CTU;
  // (exact-size heap arrays: a read past a frame's end is an AddressSanitizer report)
  std::vector<uint16_t> frames(nf * fs), refs(nf * fs);
  std::vector<uint8_t> unavail(ncu), et(ncu), el(ncu), mode0(nf * ncu);
  std::vector<int32_t> best0(nf * ncu);
  if (!rd(in, frames.data(), frames.size()) || !rd(in, refs.data(), refs.size()) || !rd(in, unavail.data(), ncu) ||
      !rd(in, et.data(), ncu) || !rd(in, el.data(), ncu) || !rd(in, mode0.data(), mode0.size()) || !rd(in, best0.data(), best0.size()))
    return 2;
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
    // one length array alone: refused, nothing written
    if (angular_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, modes, js[1], cost.data(), nullptr, nullptr, nullptr,
                            nullptr, 0, nullptr, nullptr, et.data(), nullptr) == 0 ||
        angular_refine_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, modes, js[1], 1, cost.data(), nullptr, nullptr,
                                   nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, el.data()) == 0 ||
        cost[0] != -7)
      return 3;
    const int rc = js[0] ? angular_refine_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, modes, js[1], js[0], cost.data(),
                                                      sad.data(), satd.data(), ang_mode.data(), ang_cost.data(), tried.data(), bias,
                                                      mode.data(), best.data(), et.data(), el.data())
                         : angular_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, modes, js[1], cost.data(), sad.data(),
                                               satd.data(), ang_mode.data(), ang_cost.data(), bias, mode.data(), best.data(), et.data(),
                                               el.data());
    if (rc != 0) return 4;
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
            angular_predict_cu_host(refs.data(), w, x, y, intra_log2(sd.w), intra_log2(sd.h), m, blk.data(), sd.w, et[k], el[k]);
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
  printf("angular_ext: ok\n");
  return 0;
}
