// Stand-alone check of csrc/predict_rule.h (no GPU, no HIP): the write rule of the prediction
// output as the kernels run it, on host arrays of exactly the sizes the rule allows itself to
// index, and the argument rules of the flags word and of mip_predicted_frames_ex.  Built with
// -fsanitize=address,undefined by tests/test_predict_angular_cpu.py.
//
//   test_predict_rule self              the argument rules; prints "predict_rule: ok"
//   test_predict_rule decode IN OUT     IN: int32 w, h, nframes, nitems; int64 out_samples;
//                                       uint8 unavail[nctus * 5380]; mip_pred_item items[nitems].
//                                       OUT: for (REGULAR, ANGULAR) = (0,0) (1,0) (0,1) (1,1), per
//                                       item int32 on, reg, x, y, w, h (zeros after on = 0).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "predict_rule.h"
#include "work_plan.h"

using namespace mipgpu;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

struct Call {  // what pred_decode reads of PredictArgs
  const uint8_t *unavail;
  const uint32_t *geo;
  long long out_samples;
  int ctu_cols, nctus, nframes;
};
struct Shapes {
  mip_shape_desc operator()(int s) const { return kIntraShapes[s]; }
};

static int self_test() {
  // the flags word: exactly MIP_PRED_REGULAR and MIP_PRED_ANGULAR, bit 2 stays an error
  static_assert(MIP_PRED_REGULAR == 1u && MIP_PRED_ANGULAR == 4u && MIP_CHAIN_ANGULAR == 1u, "flag bits");
  for (unsigned f = 0; f < 64; f++) CHECK(pred_flags_ok(f) == (f == 0 || f == 1 || f == 4 || f == 5));
  CHECK(!pred_flags_ok(0x80000000u) && !pred_flags_ok(0x80000005u));
  // the mode codes of the new alternative
  for (int m = -2; m < 300; m++) CHECK(pred_mode_is_angular(m) == (m >= 0x82 && m <= 0xc2));
  CHECK(!pred_mode_is_angular(MIP_MODE_PLANAR) && !pred_mode_is_angular(MIP_MODE_DC));
  // mip_predicted_frames_ex: stage off -- list and bias are not looked at
  AngList list{};
  const uint8_t bad[2] = {20, 20}, good[3] = {2, 34, 66};
  CHECK(predicted_ex_args(0, bad, 2, -1, &list) == kPredictedExOk);
  CHECK(predicted_ex_args(0, nullptr, 7, kAngMaxBias + 1, &list) == kPredictedExOk);
  for (unsigned f = 2; f < 64; f++) CHECK(predicted_ex_args(f, nullptr, 0, 0, &list) == kPredictedExFlags);
  // stage on: mip_angular_device's rules
  CHECK(predicted_ex_args(MIP_CHAIN_ANGULAR, nullptr, 0, 0, &list) == kPredictedExOk && list.n == kAngModes);
  CHECK(predicted_ex_args(MIP_CHAIN_ANGULAR, good, 3, kAngMaxBias, &list) == kPredictedExOk && list.n == 3);
  CHECK(ang_unpack(list.packed[1]).m == 34 && ang_listed(list.listed, 64) && !ang_listed(list.listed, 1));
  CHECK(predicted_ex_args(MIP_CHAIN_ANGULAR, bad, 2, 0, &list) == kPredictedExModes);
  CHECK(predicted_ex_args(MIP_CHAIN_ANGULAR, nullptr, 3, 0, &list) == kPredictedExModes);
  CHECK(predicted_ex_args(MIP_CHAIN_ANGULAR, good, 0, 0, &list) == kPredictedExModes);
  const uint8_t low[1] = {1}, high[1] = {67}, down[2] = {21, 20};
  CHECK(predicted_ex_args(MIP_CHAIN_ANGULAR, low, 1, 0, &list) == kPredictedExModes);
  CHECK(predicted_ex_args(MIP_CHAIN_ANGULAR, high, 1, 0, &list) == kPredictedExModes);
  CHECK(predicted_ex_args(MIP_CHAIN_ANGULAR, down, 2, 0, &list) == kPredictedExModes);
  CHECK(predicted_ex_args(MIP_CHAIN_ANGULAR, good, 3, -1, &list) == kPredictedExBias);
  CHECK(predicted_ex_args(MIP_CHAIN_ANGULAR, good, 3, kAngMaxBias + 1, &list) == kPredictedExBias);
  CHECK(predicted_ex_args(MIP_CHAIN_ANGULAR, bad, 2, -1, &list) == kPredictedExModes);  // (the list is checked first)
  std::printf("predict_rule: ok\n");
  return 0;
}

template <bool REGULAR, bool ANGULAR>
static void decode_all(const Call &a, const std::vector<mip_pred_item> &items, std::vector<int32_t> &out) {
  for (const mip_pred_item &it : items) {
    const Item c = pred_decode<REGULAR, ANGULAR>(a, it, Shapes{});
    CHECK(REGULAR || !c.reg);
    CHECK(!c.reg || c.on);
    if (c.on) CHECK(c.frame == it.frame && c.mode == it.mode && c.pitch == it.pitch && c.offset == it.offset);
    const int32_t row[6] = {c.on, c.reg, c.on ? c.x : 0, c.on ? c.y : 0, c.on ? c.w : 0, c.on ? c.h : 0};
    out.insert(out.end(), row, row + 6);
  }
}

static int decode_file(const char *in, const char *outp) {
  std::FILE *f = std::fopen(in, "rb");
  CHECK(f);
  int32_t head[4];
  int64_t out_samples;
  CHECK(std::fread(head, sizeof head, 1, f) == 1 && std::fread(&out_samples, sizeof out_samples, 1, f) == 1);
  const int w = head[0], h = head[1], nframes = head[2], n = head[3];
  const int cols = (w + 127) / 128, nctus = cols * ((h + 127) / 128);
  std::vector<uint8_t> unavail((size_t)nctus * MIP_CUS_PER_CTU);  // exactly what the rule may index
  CHECK(std::fread(unavail.data(), 1, unavail.size(), f) == unavail.size());
  std::vector<mip_pred_item> items((size_t)n);
  static_assert(sizeof(mip_pred_item) == 24, "mip_pred_item");
  CHECK(std::fread(items.data(), sizeof(mip_pred_item), items.size(), f) == items.size());
  std::fclose(f);
  const std::vector<CuGeo> &geo = cu_geo_table();
  std::vector<uint32_t> packed(geo.size());
  CHECK(packed.size() == (size_t)MIP_CUS_PER_CTU);
  for (size_t i = 0; i < geo.size(); i++) packed[i] = geo[i].shape | (uint32_t)geo[i].x << 8 | (uint32_t)geo[i].y << 16;
  const Call a{unavail.data(), packed.data(), out_samples, cols, nctus, nframes};
  std::vector<int32_t> out;
  decode_all<false, false>(a, items, out);
  decode_all<true, false>(a, items, out);
  decode_all<false, true>(a, items, out);
  decode_all<true, true>(a, items, out);
  f = std::fopen(outp, "wb");
  CHECK(f && std::fwrite(out.data(), sizeof(int32_t), out.size(), f) == out.size());
  std::fclose(f);
  std::printf("predict_rule: decoded %d items\n", n);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !std::strcmp(argv[1], "self")) return self_test();
  if (argc == 4 && !std::strcmp(argv[1], "decode")) return decode_file(argv[2], argv[3]);
  std::fprintf(stderr, "usage: %s self | decode IN OUT\n", argv[0]);
  return 2;
}
