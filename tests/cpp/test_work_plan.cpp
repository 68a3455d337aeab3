// CPU unit test of the search work planner (csrc/work_plan.h).  Built and run by
// tests/test_work_plan.py (g++ and, when present, the ROCm clang++; no GPU).
//  a. Byte identity: digests (FNV-1a 64) of every array an engine uploads -- CTU variant maps,
//     fixup CUs, tasks, jobs, list bounds and costs, fill / undefined-CU / split lists, the
//     item order -- and of the MFMA table blob, for 8 frame sizes x 4 filters x 6 list sets,
//     plus one non-default case per planner knob.  The constants were recorded from the
//     planner as it stood inside mipgpu.cpp (commit 239778b) by a scratch program that
//     included that file, built with hipcc -O3 (the profiling-knob cases with
//     -DMIPGPU_PROFILING_KNOBS and the environment set), and hashed the same arrays in the
//     same order as plan_digest / cv_digest below.
//  b. Structure, asserted directly for every case, so that a failing digest can be diagnosed:
//     every searched CU sits in exactly one job and its mode pairs are covered exactly once;
//     every other CU is in the undefined-CU and fill lists and nowhere else; split lists,
//     list bounds, cost order, task limits, the item order and the variant counts.
//  c. lpt_makespan against a brute-force simulation, the list choices, to_half's exactness.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "work_plan.h"

using namespace mipgpu;

static int fails = 0;
#define CHECK(c, ...)                                 \
  do {                                                \
    if (!(c)) {                                       \
      if (fails++ < 20) {                             \
        std::printf("FAIL %s: ", #c);                 \
        std::printf(__VA_ARGS__);                     \
        std::printf("\n");                            \
      }                                               \
    }                                                 \
  } while (0)

static_assert(sizeof(WaveTask) == 8 && sizeof(Job) == 8 && sizeof(FixupCu) == 8, "records are hashed as raw bytes");

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void *p, size_t n) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  }
  template <class T> void pod(const T &v) { bytes(&v, sizeof v); }
  template <class T> void vec(const std::vector<T> &v) {
    pod<uint64_t>(v.size());
    if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
  }
};

static uint64_t cv_digest(const CtuVariants &cv) {
  Fnv f;
  for (int m = 0; m < kMaps; m++) f.vec(cv.of_ctu[m]);
  for (int m = 0; m < kMaps; m++) f.vec(cv.fixup[m]);
  return f.h;
}

static uint64_t plan_digest(const WorkPlan &wp) {
  Fnv f;
  f.vec(wp.tasks);
  f.vec(wp.jobs);
  f.vec(wp.list_begin);
  f.vec(wp.list_cost);  // raw double bits
  f.vec(wp.fill);
  f.vec(wp.fill_begin);
  f.vec(wp.dfill);
  f.vec(wp.dfill_begin);
  f.vec(wp.split);
  f.vec(wp.split_begin);
  f.pod<int32_t>(wp.max_split);
  f.vec(wp.order);
  f.vec(wp.order_cost);
  f.pod<uint32_t>(wp.nonempty);
  return f.h;
}

// {width, height, filter, cv_digest, plan_digest of non-wide 1, 2, 4 then wide 1, 2, 4 slices}
struct Golden {
  int width, height, filter;
  uint64_t cv, plan[6];
};
static const Golden kDefault[] = {
    {1920, 1080, -1, 0x55cc5c264962e769ull, {0x1fea005250c5d141ull, 0x8ff744fd5d7fd40cull, 0xb9ea7314dbcb544aull, 0xf2e207c2c4f96002ull, 0x54053999a611fcbdull, 0x633e6d2094a0cf4dull}},
    {1920, 1080, 0, 0x957621ec84bed420ull, {0x94f968109d306bf7ull, 0x625f5dca6a84180full, 0x306f36cacfa9f213ull, 0xabceae1ec9799153ull, 0x7bbf250803077160ull, 0x25eb69bfb19e9ed9ull}},
    {1920, 1080, 5, 0x55cc5c264962e769ull, {0x1fea005250c5d141ull, 0x8ff744fd5d7fd40cull, 0xb9ea7314dbcb544aull, 0xf2e207c2c4f96002ull, 0x54053999a611fcbdull, 0x633e6d2094a0cf4dull}},
    {1920, 1080, 2, 0x55cc5c264962e769ull, {0x1fea005250c5d141ull, 0x8ff744fd5d7fd40cull, 0xb9ea7314dbcb544aull, 0xf2e207c2c4f96002ull, 0x54053999a611fcbdull, 0x633e6d2094a0cf4dull}},
    {3840, 2160, -1, 0x56247d3ee5d301e4ull, {0xeca50f29b8bb9702ull, 0xffb08e092b31b9edull, 0x870df7f19db060dcull, 0x973a7b2f6dd98a97ull, 0xae9fd0f1d5ddb070ull, 0xd714a09bbaae0462ull}},
    {3840, 2160, 0, 0x243999403ee06a1dull, {0xb1ca7fc1771724dcull, 0x25e0877d7ea17c23ull, 0x6517525bf42e173full, 0x1de259afa5369f68ull, 0xd6c3d5a8ad4585b6ull, 0xdbcb4a517e8be9deull}},
    {3840, 2160, 5, 0x56247d3ee5d301e4ull, {0xeca50f29b8bb9702ull, 0xffb08e092b31b9edull, 0x870df7f19db060dcull, 0x973a7b2f6dd98a97ull, 0xae9fd0f1d5ddb070ull, 0xd714a09bbaae0462ull}},
    {3840, 2160, 2, 0x56247d3ee5d301e4ull, {0xeca50f29b8bb9702ull, 0xffb08e092b31b9edull, 0x870df7f19db060dcull, 0x973a7b2f6dd98a97ull, 0xae9fd0f1d5ddb070ull, 0xd714a09bbaae0462ull}},
    {416, 240, -1, 0x006e78b6b290ba22ull, {0xc4102166893e8221ull, 0x797381c6eb2cae6bull, 0x5b89183859efc3b3ull, 0x96665b2dfadd9a7dull, 0x55767a4dbf70300cull, 0x4dc993f89b287a3cull}},
    {416, 240, 0, 0x16c1ed8caa6b77acull, {0x7e4740b65f64263dull, 0xfd76cf9324ad30b7ull, 0xb7468a354f51dfc6ull, 0xbf2110dd3db93255ull, 0xb782e506aba6fbebull, 0x558e06efb2c55538ull}},
    {416, 240, 5, 0x0a7d32104e61e416ull, {0xf1f58b7dd96a2ae0ull, 0x992478b1e1001047ull, 0x977e25243c96f02bull, 0x9b8577f3980dd4fbull, 0x05eef94da90f7dd0ull, 0xaa7e89c5873f61b5ull}},
    {416, 240, 2, 0x0a7d32104e61e416ull, {0xf1f58b7dd96a2ae0ull, 0x992478b1e1001047ull, 0x977e25243c96f02bull, 0x9b8577f3980dd4fbull, 0x05eef94da90f7dd0ull, 0xaa7e89c5873f61b5ull}},
    {264, 136, -1, 0xd0e36d67f6c06f49ull, {0x6fa18afdea528bfeull, 0x2e821e0f7e73a314ull, 0x4ad762422c3cffbfull, 0xd344493a69006f26ull, 0xf9da4978af671577ull, 0xc7cc4f5f49339cfeull}},
    {264, 136, 0, 0xaa5dbc20b2d5c8abull, {0x3b6cbe8e15c8dd56ull, 0xdc3cd72a3e3df7bdull, 0xb2d123c49c467ab3ull, 0xb061da5132031e11ull, 0xd02e91d593b67a0dull, 0x0a8382a486ea79fcull}},
    {264, 136, 5, 0x654b779f5900f025ull, {0x9f2bba8d40b67c0cull, 0xeb487449b702c5d4ull, 0xb8cc1f95a2e3db24ull, 0x1c00b423ed0615cfull, 0x03168402e33ac45cull, 0xd5369ffd7f7e459bull}},
    {264, 136, 2, 0x654b779f5900f025ull, {0x9f2bba8d40b67c0cull, 0xeb487449b702c5d4ull, 0xb8cc1f95a2e3db24ull, 0x1c00b423ed0615cfull, 0x03168402e33ac45cull, 0xd5369ffd7f7e459bull}},
    {300, 68, -1, 0x0db4afa4491110e9ull, {0x5b44397b19245c31ull, 0x102fc540aeb81845ull, 0x01fa49a5d42ef8e9ull, 0xfd7a8a47be4ab30cull, 0x491a68766af40337ull, 0x5b91fa4fa83fe58cull}},
    {300, 68, 0, 0xb47962893c939199ull, {0xebb1fe4d6c53def7ull, 0x47e3b85fff808a35ull, 0xb7a453f020db5470ull, 0x8819c2cb96fee9fbull, 0xa468c291bcc49c04ull, 0x68f276a34ec8e9eaull}},
    {300, 68, 5, 0x1335cc232f8ee2d8ull, {0xedd90a41ba2cbbd0ull, 0xf98860b8780e308bull, 0x47fa090e8a6ca95eull, 0x6ac40d42ea9587ccull, 0x85fc03c9ba9bb437ull, 0x346d67c58a6561daull}},
    {300, 68, 2, 0x1335cc232f8ee2d8ull, {0xedd90a41ba2cbbd0ull, 0xf98860b8780e308bull, 0x47fa090e8a6ca95eull, 0x6ac40d42ea9587ccull, 0x85fc03c9ba9bb437ull, 0x346d67c58a6561daull}},
    {132, 4, -1, 0x523bfde5c344d9daull, {0xb561ff708f8f5d0full, 0xd178b9111ba50509ull, 0x8e10599ae81b5bb3ull, 0x2dfbca2914cfd20eull, 0xf1175c3f0abab6f5ull, 0x9e6fb6a87af87043ull}},
    {132, 4, 0, 0xc5a8499fa4507892ull, {0x0e740a0b36a3e712ull, 0x1c0962baa35eca33ull, 0xbac1c768dd7f2d6dull, 0xfb569d5c3d7fcb71ull, 0x820484e64bb48524ull, 0xc8fa658e02d22ccdull}},
    {132, 4, 5, 0x940a6699ee5df2ecull, {0x372a8119ab2408fdull, 0x1e826502b79adbecull, 0x92bb089b18fec55aull, 0x4aeaf42e34e8539aull, 0xb45c7c0ca4a6868bull, 0xa0662ec73094db4aull}},
    {132, 4, 2, 0x940a6699ee5df2ecull, {0x372a8119ab2408fdull, 0x1e826502b79adbecull, 0x92bb089b18fec55aull, 0x4aeaf42e34e8539aull, 0xb45c7c0ca4a6868bull, 0xa0662ec73094db4aull}},
    {4, 132, -1, 0x7caa9e9ca00e628eull, {0x98751bae0ceacdfbull, 0xd1bf7f911b2c846eull, 0xb3cd5709bef203b1ull, 0xfa188bafc7c6c89cull, 0x84fb3dc7444ea9f3ull, 0x5d4a43129d9f8784ull}},
    {4, 132, 0, 0x02342fc6cae7f89aull, {0x98751bae0ceacdfbull, 0xd1bf7f911b2c846eull, 0xb3cd5709bef203b1ull, 0xfa188bafc7c6c89cull, 0x84fb3dc7444ea9f3ull, 0x5d4a43129d9f8784ull}},
    {4, 132, 5, 0x9c88825ed86228ebull, {0x98751bae0ceacdfbull, 0xd1bf7f911b2c846eull, 0xb3cd5709bef203b1ull, 0xfa188bafc7c6c89cull, 0x84fb3dc7444ea9f3ull, 0x5d4a43129d9f8784ull}},
    {4, 132, 2, 0x02342fc6cae7f89aull, {0x98751bae0ceacdfbull, 0xd1bf7f911b2c846eull, 0xb3cd5709bef203b1ull, 0xfa188bafc7c6c89cull, 0x84fb3dc7444ea9f3ull, 0x5d4a43129d9f8784ull}},
    {4, 4, -1, 0x4a0c0ee1b9f96fecull, {0xbedc791c7b28e521ull, 0x9c8f38ba17903941ull, 0xc45f39082a7de88full, 0xe16ac914523b5ebeull, 0x969fdd1202d8b401ull, 0xa6c213165615113full}},
    {4, 4, 0, 0x4a0c0ee1b9f96fecull, {0xbedc791c7b28e521ull, 0x9c8f38ba17903941ull, 0xc45f39082a7de88full, 0xe16ac914523b5ebeull, 0x969fdd1202d8b401ull, 0xa6c213165615113full}},
    {4, 4, 5, 0x4a0c0ee1b9f96fecull, {0xbedc791c7b28e521ull, 0x9c8f38ba17903941ull, 0xc45f39082a7de88full, 0xe16ac914523b5ebeull, 0x969fdd1202d8b401ull, 0xa6c213165615113full}},
    {4, 4, 2, 0x4a0c0ee1b9f96fecull, {0xbedc791c7b28e521ull, 0x9c8f38ba17903941ull, 0xc45f39082a7de88full, 0xe16ac914523b5ebeull, 0x969fdd1202d8b401ull, 0xa6c213165615113full}},
};
static const uint64_t kTableDigest = 0x2c5aff8dd077a407ull;

struct KnobCase {
  const char *name;
  PlanKnobs knobs;
  Golden at[2];
};
static PlanKnobs knobs_of(double cut, bool transpose, bool no_pairs, uint64_t shapes) {
  PlanKnobs k;
  k.cut_factor = cut;
  k.transpose_wide = transpose;
  k.no_pairs = no_pairs;
  k.shapes = shapes;
  return k;
}
static const uint64_t kAllShapes = (1ull << MIP_NUM_SHAPES) - 1;
static const KnobCase kKnobCases[] = {
    {"transpose_wide=false", knobs_of(2.0, false, false, kAllShapes),
     {{1920, 1080, -1, 0x55cc5c264962e769ull, {0xc6ab5cab4407728aull, 0x60f27c72a988a12dull, 0xb894bc12b1417b91ull, 0x007201f74268dbd2ull, 0xcf069b0b277d556eull, 0x7f3cfa2113e2a3edull}},
      {300, 68, 0, 0xb47962893c939199ull, {0xd3aea94076244fd3ull, 0x60d1c2d4ba10a9daull, 0xfa2f4cea6efa6889ull, 0x464011c3c25ddc02ull, 0xfd3c837bc48e16b8ull, 0x9b4e315af46d3798ull}}}},
    {"cut_factor=1", knobs_of(1.0, true, false, kAllShapes),
     {{1920, 1080, -1, 0x55cc5c264962e769ull, {0xad9ecb45ae0fda2cull, 0xcde3c12f6e93e124ull, 0x6600f0a66140fd5full, 0xbc3e184b0b1e6cf0ull, 0x4444010570de8224ull, 0x20b33004fcaa79f1ull}},
      {300, 68, 0, 0xb47962893c939199ull, {0xce7d7f9f8711a83cull, 0x576194de5bddcc92ull, 0xa425fa2d6a3006f5ull, 0x142d0850cb9958e0ull, 0x00d99bb31465c9b6ull, 0x0d6e9b93795f9682ull}}}},
    {"cut_factor=4", knobs_of(4.0, true, false, kAllShapes),
     {{1920, 1080, -1, 0x55cc5c264962e769ull, {0x4bafab23a74d2e61ull, 0x7b4ea5c8a74f5238ull, 0xd3d607b4b0f7c889ull, 0xba1cc2c15d4f7e54ull, 0x88ebe1581c5241d8ull, 0x5f593b39b2ee9d01ull}},
      {300, 68, 0, 0xb47962893c939199ull, {0x1676cf92fcb8bc00ull, 0x4527c9e56142c535ull, 0xab27c69c2b94c8c7ull, 0x886c9f89a58fdb24ull, 0xe9464b4d9d3acfeeull, 0x8f77abfceb619ca7ull}}}},
    {"shapes={0,46}", knobs_of(2.0, true, false, 1ull << 0 | 1ull << 46),
     {{1920, 1080, -1, 0x55cc5c264962e769ull, {0xbf18c6142c4fd3c3ull, 0xc513d0cd2cb81cd4ull, 0x815421b45f142874ull, 0x4936dfaf67290627ull, 0xc5089a659e6f83b4ull, 0x54042fe3bcbb1884ull}},
      {300, 68, 0, 0xb47962893c939199ull, {0xa90ed27d83b8da50ull, 0x88fc0075b2b99e3eull, 0x12ae43219238cb9eull, 0x8a7fe543868597e9ull, 0x5138abfe20ddba6bull, 0x93aa3e827468f38eull}}}},
    {"no_pairs", knobs_of(2.0, true, true, kAllShapes),
     {{1920, 1080, -1, 0x55cc5c264962e769ull, {0x124987e431bbe351ull, 0x10637af380363170ull, 0x11ee0d1945355c4eull, 0x2459aea63eed4d42ull, 0x3ea2e7392199d495ull, 0x8447a75e906716f5ull}},
      {300, 68, 0, 0xb47962893c939199ull, {0xbc5bd3330c6761fbull, 0x3fcd38b55582c331ull, 0x60bfdad02a17a014ull, 0x66ddd39cd930c9d3ull, 0x3ff7bada8af1d0c8ull, 0xc0608cfd4c36d662ull}}}},
};

// ---------------------------------------------------------------- structure
static int pairs_of_class(int cls) {
  const int sid = class_size_id(kClassW[cls], kClassH[cls]);
  return sid == 2 ? 6 : (sid == 1 ? 8 : 16);
}
static double task_cost(const WaveTask &t) { return pair_cost(t.cls, t.ncu) * (t.q1 - t.q0) + 150.0; }

static void check_structure(const char *tag, const CtuVariants &cv, const WorkPlan &wp) {
  const std::vector<CuGeo> &geo = cu_geo_table();
  const int nvar = (int)cv.pattern.size(), sl = wp.slices, waves = wp.wide ? kWideWaves : kSearchWaves;
  CHECK((int)geo.size() == MIP_CUS_PER_CTU, "%s: %zu CUs", tag, geo.size());
  CHECK((int)wp.list_begin.size() == 4 * nvar * sl + 1 && (int)wp.list_cost.size() == 4 * nvar * sl, "%s: list sizes", tag);
  CHECK((int)wp.fill_begin.size() == 4 * nvar + 1 && (int)wp.dfill_begin.size() == 4 * nvar + 1 &&
            (int)wp.split_begin.size() == nvar + 1,
        "%s: fill / dfill / split bounds", tag);
  if (fails) return;
  CHECK(wp.list_begin[0] == 0 && wp.list_begin.back() == (int)wp.tasks.size(), "%s: list_begin ends", tag);
  CHECK(wp.fill_begin[0] == 0 && wp.fill_begin.back() == (int)wp.fill.size(), "%s: fill_begin ends", tag);
  CHECK(wp.dfill_begin[0] == 0 && wp.dfill_begin.back() == (int)wp.dfill.size(), "%s: dfill_begin ends", tag);
  CHECK(wp.split_begin[0] == 0 && wp.split_begin.back() == (int)wp.split.size(), "%s: split_begin ends", tag);
  for (const std::vector<int> *b : {&wp.list_begin, &wp.fill_begin, &wp.dfill_begin, &wp.split_begin})
    CHECK(std::is_sorted(b->begin(), b->end()), "%s: bounds decrease", tag);
  if (fails) return;
  int max_split = 0;
  for (int v = 0; v < nvar; v++) {
    std::vector<int> job_of(MIP_CUS_PER_CTU, -1), ntasks(MIP_CUS_PER_CTU, 0), filled(MIP_CUS_PER_CTU, 0);
    std::vector<std::vector<int>> cover(MIP_CUS_PER_CTU);
    for (int q = 0; q < 4; q++) {
      for (int s = 0; s < sl; s++) {
        const int l = (4 * v + q) * sl + s;
        double sum = 0, prev = 0;
        for (int t = wp.list_begin[l]; t < wp.list_begin[l + 1]; t++) {
          const WaveTask &wt = wp.tasks[t];
          CHECK(wt.cls < kNumClasses && wt.ncu >= 1 && wt.ncu <= class_slots(wt.cls), "%s: task %d: %d CUs of class %d", tag, t,
                wt.ncu, wt.cls);
          CHECK(wt.q0 < wt.q1 && wt.q1 <= pairs_of_class(wt.cls), "%s: task %d: pairs [%d, %d)", tag, t, wt.q0, wt.q1);
          CHECK((size_t)wt.cu0 + wt.ncu <= wp.jobs.size(), "%s: task %d: jobs past the end", tag, t);
          if (fails) return;
          const double c = task_cost(wt);
          CHECK(t == wp.list_begin[l] || c <= prev, "%s: list %d: task %d costs %g after %g", tag, l, t, c, prev);
          prev = c;
          sum += c;
          for (int j = 0; j < wt.ncu; j++) {
            const Job &job = wp.jobs[wt.cu0 + j];
            CHECK(job.cu < MIP_CUS_PER_CTU, "%s: job CU %d", tag, job.cu);
            if (fails) return;
            const CuGeo &g = geo[job.cu];
            const mip_shape_desc &sd = kShapes[g.shape];
            const bool tr = kClassTR[wt.cls];
            CHECK(kClassW[wt.cls] == (tr ? sd.h : sd.w) && kClassH[wt.cls] == (tr ? sd.w : sd.h), "%s: CU %d (%dx%d) in class %d",
                  tag, job.cu, sd.w, sd.h, wt.cls);
            CHECK(g.x / 64 + 2 * (g.y / 64) == q && job.lx == g.x % 64 && job.ly == g.y % 64, "%s: CU %d: quadrant %d, origin %d,%d",
                  tag, job.cu, q, job.lx, job.ly);
            int first = 0;  // first CU of the shape
            for (int k = 0; k < g.shape; k++) first += kShapes[k].ncu;
            CHECK(job.cost == sd.cost_offset + (uint32_t)(job.cu - first) * 2 * sd.modes, "%s: CU %d: cost entry %u", tag, job.cu,
                  job.cost);
            CHECK(job_of[job.cu] < 0 || job_of[job.cu] == (int)wt.cu0 + j, "%s: variant %d: CU %d in two jobs", tag, v, job.cu);
            job_of[job.cu] = (int)wt.cu0 + j;
            ntasks[job.cu]++;
            cover[job.cu].resize(sd.modes, 0);
            for (int p = wt.q0; p < wt.q1; p++) {
              CHECK(p < sd.modes, "%s: CU %d: pair %d of %d", tag, job.cu, p, sd.modes);
              if (p < sd.modes) cover[job.cu][p]++;
            }
          }
        }
        CHECK(wp.list_cost[l] == sum / waves, "%s: list %d: cost %g, its tasks %g", tag, l, wp.list_cost[l], sum / waves);
      }
      // the CUs that are off: the undefined-CU list and their cost entries' 16-byte units
      std::vector<uint32_t> want_fill, got_fill(wp.fill.begin() + wp.fill_begin[4 * v + q], wp.fill.begin() + wp.fill_begin[4 * v + q + 1]);
      for (int i = wp.dfill_begin[4 * v + q]; i < wp.dfill_begin[4 * v + q + 1]; i++) {
        const int cu = wp.dfill[i];
        CHECK(cu < MIP_CUS_PER_CTU && geo[cu].x / 64 + 2 * (geo[cu].y / 64) == q, "%s: undefined CU %d in quadrant %d", tag, cu, q);
        if (fails) return;
        filled[cu]++;
      }
      for (int cu = 0, s = 0, first = 0; cu < MIP_CUS_PER_CTU; cu++) {
        while (cu - first >= kShapes[s].ncu) first += kShapes[s++].ncu;
        if (cv.pattern[v][cu] || geo[cu].x / 64 + 2 * (geo[cu].y / 64) != q) continue;
        const uint32_t off = kShapes[s].cost_offset + (uint32_t)(cu - first) * 2 * kShapes[s].modes;
        for (uint32_t u = 0; u < (uint32_t)(2 * kShapes[s].modes) / 4; u++) want_fill.push_back(off / 4 + u);
      }
      std::sort(got_fill.begin(), got_fill.end());
      std::sort(want_fill.begin(), want_fill.end());
      CHECK(got_fill == want_fill, "%s: variant %d quadrant %d: %zu fill units, want %zu", tag, v, q, got_fill.size(), want_fill.size());
    }
    std::vector<int> in_split(MIP_CUS_PER_CTU, 0);
    for (int i = wp.split_begin[v]; i < wp.split_begin[v + 1]; i++) {
      CHECK(wp.split[i] < MIP_CUS_PER_CTU, "%s: split CU %d", tag, wp.split[i]);
      if (fails) return;
      in_split[wp.split[i]]++;
    }
    max_split = std::max(max_split, wp.split_begin[v + 1] - wp.split_begin[v]);
    for (int cu = 0; cu < MIP_CUS_PER_CTU; cu++) {
      const bool on = cv.pattern[v][cu];
      CHECK((job_of[cu] >= 0) == on, "%s: variant %d: CU %d %s a job", tag, v, cu, on ? "without" : "with");
      CHECK(filled[cu] == (on ? 0 : 1), "%s: variant %d: CU %d %d times in the undefined-CU lists", tag, v, cu, filled[cu]);
      CHECK(in_split[cu] == (ntasks[cu] > 1 ? 1 : 0), "%s: variant %d: CU %d in %d tasks, %d times in the split list", tag, v, cu,
            ntasks[cu], in_split[cu]);
      if (on)
        for (size_t p = 0; p < cover[cu].size(); p++)
          CHECK(cover[cu][p] == 1, "%s: variant %d: CU %d pair %zu searched %d times", tag, v, cu, p, cover[cu][p]);
      CHECK(!on || (int)cover[cu].size() == kShapes[geo[cu].shape].modes, "%s: variant %d: CU %d pairs", tag, v, cu);
    }
  }
  CHECK(wp.max_split == max_split, "%s: max_split %d, largest list %d", tag, wp.max_split, max_split);
  // the item order
  const std::vector<uint8_t> &var = cv.of_ctu[kMapOrig];
  const size_t nitems = var.size() * 4 * sl;
  CHECK(wp.order.size() == nitems && wp.order_cost.size() == nitems, "%s: %zu items ordered, %zu", tag, wp.order.size(), nitems);
  if (fails) return;
  std::vector<int> seen(nitems, 0);
  uint32_t with_tasks = 0;
  for (size_t i = 0; i < nitems; i++) {
    const uint32_t it = wp.order[i];
    CHECK(it < nitems && !seen[it], "%s: order[%zu] = %u", tag, i, it);
    if (fails) return;
    seen[it] = 1;
    CHECK(i == 0 || wp.order_cost[i] <= wp.order_cost[i - 1], "%s: order_cost rises at %zu", tag, i);
    const int l = (var[it / (4 * sl)] * 4 + (int)(it % (4 * sl)) / sl) * sl + (int)(it % sl);
    const bool empty = wp.list_begin[l + 1] == wp.list_begin[l];
    CHECK(empty == (i >= wp.nonempty), "%s: order[%zu] %s tasks, nonempty %u", tag, i, empty ? "without" : "with", wp.nonempty);
    CHECK(wp.order_cost[i] == wp.list_cost[l] + (empty ? kItemOverhead / 8 : kItemOverhead), "%s: order_cost[%zu]", tag, i);
    with_tasks += !empty;
  }
  CHECK(with_tasks == wp.nonempty, "%s: %u items with tasks, nonempty %u", tag, with_tasks, wp.nonempty);
}

static void check_case(const char *name, const Golden &g, const PlanKnobs &knobs) {
  const EnginePlan p = plan_engine(g.width, g.height, g.filter, {1, 2, 4}, knobs);
  char tag[128];
  std::snprintf(tag, sizeof tag, "%s %dx%d filter %d", name, g.width, g.height, g.filter);
  CHECK(cv_digest(p.cv) == g.cv, "%s: CTU variants / fixup CUs digest %016llx", tag, (unsigned long long)cv_digest(p.cv));
  CHECK(p.work.size() == 6, "%s: %zu list sets", tag, p.work.size());
  if (p.work.size() != 6) return;
  for (int i = 0; i < 6; i++) {
    const WorkPlan &wp = p.work[i];
    char wtag[192];
    std::snprintf(wtag, sizeof wtag, "%s slices %d waves %d", tag, wp.slices, wp.wide ? kWideWaves : kSearchWaves);
    CHECK(wp.slices == (1 << (i % 3)) && wp.wide == (i >= 3), "%s: list set %d", wtag, i);
    if (!knobs.no_pairs && knobs.shapes == kAllShapes) check_structure(wtag, p.cv, wp);
    CHECK(plan_digest(wp) == g.plan[i], "%s: digest %016llx", wtag, (unsigned long long)plan_digest(wp));
  }
}

// ---------------------------------------------------------------- the rest
static float half_value(uint16_t h) {
  const int exp = (h >> 10) & 31, man = h & 1023;
  const float v = exp ? std::ldexp(1.0f + man / 1024.0f, exp - 15) : std::ldexp(man / 1024.0f, -14);
  return h & 0x8000 ? -v : v;
}

static double brute_makespan(const std::vector<double> &order_cost, int nframes, int groups) {
  std::vector<double> fin(groups, 0.0);
  for (double c : order_cost)
    for (int f = 0; f < nframes; f++) *std::min_element(fin.begin(), fin.end()) += c;
  return *std::max_element(fin.begin(), fin.end());
}

int main() {
  // knobs: the shipped configuration
  const PlanKnobs def;
  CHECK(def.cut_factor == 2.0 && def.transpose_wide && !def.no_pairs && def.shapes == kAllShapes, "PlanKnobs defaults");

  // to_half: exact for every multiple of 1/64 of magnitude below 32
  for (int k = -2047; k <= 2047; k++) CHECK(half_value(to_half(k / 64.0f)) == k / 64.0f, "to_half(%d/64) = %04x", k, to_half(k / 64.0f));
  CHECK(to_half(0.0f) == 0 && to_half(1.0f) == 0x3c00 && to_half(-0.5f) == 0xb800 && to_half(1 / 64.0f) == 0x2400 &&
            to_half(31.984375f) == 0x4fff,
        "to_half bit patterns");
  {
    const std::vector<uint8_t> t = build_tables();
    Fnv f;
    f.vec(t);
    CHECK(t.size() == 13840 && t.size() == (size_t)kTableBytes, "table blob of %zu bytes", t.size());
    CHECK(f.h == kTableDigest, "table digest %016llx", (unsigned long long)f.h);
  }

  // a. + b.: every size x filter x list set
  CHECK(sizeof kDefault / sizeof kDefault[0] == 32, "32 default cases");
  for (const Golden &g : kDefault) check_case("default", g, PlanKnobs());
  for (const KnobCase &k : kKnobCases)
    for (const Golden &g : k.at) check_case(k.name, g, k.knobs);

  // variant and fixup counts (measured on the planner's predecessor)
  const struct { int w, h, filter; size_t variants; } counts[] = {
      {1920, 1080, MIP_FILTER_NONE, 2}, {1920, 1080, MIP_FILTER_1D_INT, 4}, {1920, 1080, MIP_FILTER_1D_FLOAT_5x5, 2},
      {416, 240, MIP_FILTER_NONE, 5},   {416, 240, MIP_FILTER_1D_INT, 8},   {416, 240, MIP_FILTER_1D_FLOAT_5x5, 6}};
  for (const auto &c : counts) {
    const CtuVariants cv = ctu_variants(c.w, c.h, c.filter);
    CHECK(cv.pattern.size() == c.variants, "%dx%d filter %d: %zu variants", c.w, c.h, c.filter, cv.pattern.size());
    CHECK(cv.fixup[kMapOrig].empty(), "%dx%d: fixup CUs with original references", c.w, c.h);
    if (c.w == 416) {
      CHECK(cv.fixup[kMapAltCaller].size() == 1088, "416x240 filter %d: %zu caller-reference fixup CUs", c.filter,
            cv.fixup[kMapAltCaller].size());
      if (c.filter == MIP_FILTER_1D_INT)
        CHECK(cv.fixup[kMapAltEngine].size() == 1076, "416x240 1D_INT: %zu engine-reference fixup CUs", cv.fixup[kMapAltEngine].size());
    }
  }

  // a single slice count: non-wide, then wide
  {
    const EnginePlan p = plan_engine(416, 240, MIP_FILTER_NONE, {2});
    CHECK(p.work.size() == 2 && p.work[0].slices == 2 && !p.work[0].wide && p.work[1].slices == 2 && p.work[1].wide, "slice set {2}");
    CHECK(closest_slices(p.work, 1) == 0 && closest_slices(p.work, 4) == 0, "closest_slices of one list set");
  }

  // c. lpt_makespan against a brute-force simulation, and the choices among the lists
  {
    uint32_t rng = 12345;
    auto next = [&] { return (rng = rng * 1664525u + 1013904223u) >> 8; };
    for (int trial = 0; trial < 200; trial++) {
      std::vector<double> cost(1 + next() % 12);
      for (double &c : cost) c = 1 + next() % 1000;
      std::sort(cost.rbegin(), cost.rend());
      const int nframes = 1 + next() % 3, groups = 1 + next() % 5;
      CHECK(lpt_makespan(cost, nframes, groups) == brute_makespan(cost, nframes, groups), "lpt_makespan trial %d", trial);
    }
    CHECK(lpt_makespan({5, 3, 3, 2}, 1, 2) == 7 && lpt_makespan({5, 3, 3, 2}, 2, 2) == 13 && lpt_makespan({4}, 3, 8) == 4,
          "lpt_makespan by hand");
    const EnginePlan p = plan_engine(1920, 1080, MIP_FILTER_NONE, {1, 2, 4});
    CHECK(closest_slices(p.work, 1) == 0 && closest_slices(p.work, 2) == 1 && closest_slices(p.work, 3) == 1 &&
              closest_slices(p.work, 8) == 2,
          "closest_slices");
    CHECK(closest_slices({}, 1) == -1 && shortest_makespan({}, false, 1, 1) == -1, "no lists");
    for (int wide = 0; wide < 2; wide++)
      for (int nframes : {1, 2, 7})
        for (int groups : {256, 512}) {
          int want = -1;
          for (int i = 0; i < 6; i++)
            if (p.work[i].wide == (wide != 0) && (want < 0 || lpt_makespan(p.work[i].order_cost, nframes, groups) <
                                                                 lpt_makespan(p.work[want].order_cost, nframes, groups)))
              want = i;
          CHECK(shortest_makespan(p.work, wide != 0, nframes, groups) == want, "shortest_makespan wide %d frames %d groups %d", wide,
                nframes, groups);
        }
    CHECK(few_items_per_cu(767, 256) && !few_items_per_cu(768, 256), "few_items_per_cu");
  }

  if (fails) {
    std::printf("work_plan: %d FAILED\n", fails);
    return 1;
  }
  std::printf("work_plan: ok\n");
  return 0;
}
