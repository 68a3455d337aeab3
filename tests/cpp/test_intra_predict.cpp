// Host restatement of the Planar / DC block output (vvc-mip-gpu_amd/csrc/intra_plan.h
// intra_predict_cu_host: the steps of the prediction kernel's regular items) as a stand-alone
// program: tests/test_intra_predict_cpu.py writes reference frames to a file, this program
// predicts every available CU in both modes and writes the blocks back; the test compares them
// with tests/intra_ref.py.  Built with -fsanitize=address,undefined.
//
//   test_intra_predict IN OUT
//   IN : int32 width, height, nframes; uint16 refs[nframes][H][W]; uint8 unavail[nctus*5380]
//   OUT: per frame, per available CU in index order: uint16 planar[h][w], dc[h][w]
#include <cstdio>
#include <vector>

#include "intra_plan.h"

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE *f, const T *p, size_t n) { return fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
  using namespace mipgpu;
  if (argc != 3) return 2;
  FILE *in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t hdr[3];
  if (!rd(in, hdr, 3)) return 2;
  const int w = hdr[0], h = hdr[1], nf = hdr[2];
  const int cols = (w + 127) / 128, nctus = cols * ((h + 127) / 128);
  const size_t fs = (size_t)w * h, ncu = (size_t)nctus * MIP_CUS_PER_CTU;
  // (exact-size heap arrays: a read past a frame's end is an AddressSanitizer report)
  std::vector<uint16_t> refs(nf * fs);
  std::vector<uint8_t> unavail(ncu);
  if (!rd(in, refs.data(), refs.size()) || !rd(in, unavail.data(), ncu)) return 2;
  fclose(in);
  FILE *out = fopen(argv[2], "wb");
  if (!out) return 2;
  const uint16_t kFill = 0xABCD;
  std::vector<uint16_t> canvas(fs);
  for (int f = 0; f < nf; f++)
    for (int c = 0; c < nctus; c++) {
      size_t k = (size_t)c * MIP_CUS_PER_CTU;
      for (int s = 0; s < MIP_NUM_SHAPES; s++) {
        const mip_shape_desc &sd = kIntraShapes[s];
        const int lw = intra_log2(sd.w), lh = intra_log2(sd.h);
        for (int cu = 0; cu < sd.ncu; cu++, k++) {
          if (unavail[k]) continue;
          const int x = 128 * (c % cols) + intra_axis(sd.xb, sd.xs, sd.xd, cu % sd.ncols);
          const int y = 128 * (c / cols) + intra_axis(sd.yb, sd.ys, sd.yd, cu / sd.ncols);
          const uint16_t *R = refs.data() + f * fs;
          std::vector<uint16_t> blk((size_t)2 * sd.w * sd.h, kFill);
          if (intra_predict_cu_host(R, w, x, y, lw, lh, MIP_MODE_PLANAR, blk.data(), sd.w) != 0) return 3;
          if (intra_predict_cu_host(R, w, x, y, lw, lh, MIP_MODE_DC, blk.data() + sd.w * sd.h, sd.w) != 0) return 3;
          for (uint16_t v : blk)
            if (v > 1023) return 4;  // (every sample written, and clipped)
          if (!wr(out, blk.data(), blk.size())) return 2;
          // any other mode: an error, nothing written
          uint16_t none[16] = {kFill};
          if (intra_predict_cu_host(R, w, x, y, lw, lh, 0, none, sd.w) == 0 || none[0] != kFill) return 5;
          // a pitch above w: the same rows at their place in a frame-shaped canvas, nothing else
          if (cu % 7 == 0 && x + sd.w <= w && y + sd.h <= h) {
            std::fill(canvas.begin(), canvas.end(), kFill);
            if (intra_predict_cu_host(R, w, x, y, lw, lh, MIP_MODE_DC, canvas.data() + (size_t)y * w + x, w) != 0) return 3;
            for (int j = 0; j < h; j++)
              for (int i = 0; i < w; i++) {
                const bool inside = i >= x && i < x + sd.w && j >= y && j < y + sd.h;
                const uint16_t want = inside ? blk[(size_t)sd.w * sd.h + (size_t)(j - y) * sd.w + (i - x)] : kFill;
                if (canvas[(size_t)j * w + i] != want) return 6;
              }
          }
        }
      }
    }
  fclose(out);
  printf("intra_predict: ok\n");
  return 0;
}
