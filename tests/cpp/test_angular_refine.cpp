// Host walk of the coarse-to-fine angular search (vvc-mip-gpu_amd/csrc/angular_plan.h,
// angular_refine_frames_host) as a stand-alone program: tests/test_angular_refine_cpu.py writes
// frames and a set of (list, seeds) jobs to a file, this program runs the walk for every job on
// exactly frame-sized arrays and writes every output back; the test compares them with
// tests/angular_refine_ref.py.  Built with -fsanitize=address,undefined.
//
//   test_angular_refine run IN OUT
//   IN : int32 width, height, nframes, bias, njobs; uint16 frames[nframes][H][W];
//        uint16 refs[nframes][H][W]; uint8 unavail[nctus*5380];
//        uint8 best_mode[nframes][nctus*5380]; int32 best_cost[nframes][nctus*5380];
//        per job: int32 seeds, nmodes (0: all); uint8 modes[nmodes]
//   OUT: per job int32 cost, sad, satd [nframes][nctus*5380][65]; uint8 ang_mode; int32 ang_cost;
//        uint8 tried; uint8 best_mode; int32 best_cost (merged)
//   test_angular_refine rules
//   the candidate step against a straightforward set computation, for every seed tuple of up to
//   three modes and five list masks; the running top three against a stable sort; the argument
//   rules of the walk (seeds 0 and 4, a bad list, a bad bias, no output, half a pair).
#include <algorithm>
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

static bool candidates_ok() {
  std::vector<std::vector<uint8_t>> lists(5);
  for (int m = 2; m <= 66; m += 2) lists[0].push_back((uint8_t)m);
  for (int m = 3; m <= 65; m += 2) lists[1].push_back((uint8_t)m);
  lists[2] = {2, 34, 66};
  for (int m = 2; m <= 66; m++) lists[3].push_back((uint8_t)m);
  lists[4] = {2};
  long long checked = 0;
  for (const auto &l : lists) {
    AngList list;
    if (!ang_list(l.data(), (int)l.size(), &list)) return false;
    for (int n = 1; n <= 3; n++)
      for (int s0 = 2; s0 <= 66; s0++)
        for (int s1 = n > 1 ? 2 : 66; s1 <= 66; s1++)
          for (int s2 = n > 2 ? 2 : 66; s2 <= 66; s2++) {
            const int seed[3] = {s0, s1, s2};
            bool in[68] = {};
            for (int q = 0; q < n; q++)
              for (int step = -1; step <= 1; step += 2) {
                const int m = seed[q] + step;
                if (m >= 2 && m <= 66 && std::find(l.begin(), l.end(), (uint8_t)m) == l.end()) in[m] = true;
              }
            AngTop top = ang_top_none();
            top.m0 = s0, top.c0 = 1;
            if (n > 1) top.m1 = s1, top.c1 = 2;
            if (n > 2) top.m2 = s2, top.c2 = 3;
            for (int given = n; given <= 3; given++) {  // (seeds above the entries the top list holds change nothing)
              AngSet set = ang_candidates(top, given, list.listed);
              int want = 0;
              for (int m = 2; m <= 66; m++) want += in[m];
              if (ang_set_count(set) != want) return false;
              for (int m = 2; m <= 66; m++)
                if (in[m] && ang_set_pop(set) != m) return false;  // increasing order, each once
              if (ang_set_pop(set) != 0 || ang_set_count(set) != 0) return false;
            }
            // fewer seeds asked for than entries held: only the first count
            if (n == 3) {
              AngSet one = ang_candidates(top, 1, list.listed);
              AngTop first = ang_top_none();
              first.m0 = s0, first.c0 = 1;
              AngSet same = ang_candidates(first, 3, list.listed);
              if (one.w0 != same.w0 || one.w1 != same.w1 || one.w2 != same.w2) return false;
            }
            checked++;
          }
  }
  return checked == 5LL * (65 + 65 * 65 + 65 * 65 * 65);
}

static bool top_ok() {
  unsigned state = 12345u;
  auto next = [&]() { return state = state * 1664525u + 1013904223u, state >> 8; };
  for (int round = 0; round < 20000; round++) {
    const int n = 1 + (int)(next() % 9), spread = 1 + (int)(next() % 4);  // few values: many ties
    std::vector<std::pair<int32_t, int>> all;
    AngTop top = ang_top_none();
    int m = 2;
    for (int q = 0; q < n; q++) {
      m += (int)(next() % 6);
      if (m > 66) break;
      const int32_t c = (int32_t)(next() % spread);
      all.push_back({c, m});
      ang_top_step(top, m, c);
      m++;
    }
    std::stable_sort(all.begin(), all.end());  // (cost, mode)
    const int got_m[3] = {top.m0, top.m1, top.m2};
    const int32_t got_c[3] = {top.c0, top.c1, top.c2};
    for (int q = 0; q < 3; q++) {
      const bool has = q < (int)all.size();
      if (got_m[q] != (has ? all[q].second : 0) || got_c[q] != (has ? all[q].first : MIP_COST_UNAVAILABLE)) return false;
    }
  }
  uint8_t mode = 0xff;
  int32_t cost = MIP_COST_UNAVAILABLE;
  ang_best_step_any(mode, cost, 40, 7);
  ang_best_step_any(mode, cost, 30, 7);  // a tie goes to the lower mode, whatever the order
  ang_best_step_any(mode, cost, 35, 7);
  ang_best_step_any(mode, cost, 2, 8);
  if (mode != MIP_MODE_ANGULAR(30) || cost != 7) return false;
  ang_best_step_any(mode, cost, 66, 6);
  return mode == MIP_MODE_ANGULAR(66) && cost == 6;
}

static bool arguments_ok() {
  const int w = 8, h = 8;
  const size_t ncu = MIP_CUS_PER_CTU;
  std::vector<uint16_t> frame((size_t)w * h, 500);
  std::vector<uint8_t> unavail(ncu, 1), am(ncu, 0x5a), tried(ncu, 0x5a), bm(ncu, 3);
  std::vector<int32_t> ac(ncu, -7), bc(ncu, 9), cost(ncu * 65, -7);
  const uint8_t good[2] = {10, 20}, twice[2] = {30, 30};
#define WALK(m, n, seeds, c, mo, co, tr, b, bmo, bco) \
  angular_refine_frames_host(frame.data(), frame.data(), unavail.data(), w, h, 1, m, n, seeds, c, nullptr, nullptr, mo, co, tr, b, bmo, bco)
  if (WALK(good, 2, 0, cost.data(), am.data(), ac.data(), tried.data(), 0, bm.data(), bc.data()) == 0) return false;
  if (WALK(good, 2, 4, cost.data(), am.data(), ac.data(), tried.data(), 0, bm.data(), bc.data()) == 0) return false;
  if (WALK(good, 2, -1, cost.data(), am.data(), ac.data(), tried.data(), 0, bm.data(), bc.data()) == 0) return false;
  if (WALK(twice, 2, 1, cost.data(), am.data(), ac.data(), tried.data(), 0, bm.data(), bc.data()) == 0) return false;
  if (WALK(good, 66, 1, cost.data(), am.data(), ac.data(), tried.data(), 0, bm.data(), bc.data()) == 0) return false;
  if (WALK(good, 2, 1, cost.data(), am.data(), ac.data(), tried.data(), -1, bm.data(), bc.data()) == 0) return false;
  if (WALK(good, 2, 1, cost.data(), am.data(), ac.data(), tried.data(), (1 << 20) + 1, bm.data(), bc.data()) == 0) return false;
  if (WALK(good, 2, 1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == 0) return false;
  if (WALK(good, 2, 1, cost.data(), am.data(), nullptr, nullptr, 0, nullptr, nullptr) == 0) return false;
  if (WALK(good, 2, 1, cost.data(), nullptr, nullptr, nullptr, 0, nullptr, bc.data()) == 0) return false;
  if (cost[0] != -7 || am[0] != 0x5a || ac[0] != -7 || tried[0] != 0x5a || bm[0] != 3 || bc[0] != 9) return false;  // nothing written
  // tried alone is an output; every CU here is unavailable
  if (WALK(good, 2, 3, nullptr, nullptr, nullptr, tried.data(), 0, nullptr, nullptr) != 0) return false;
#undef WALK
  return std::all_of(tried.begin(), tried.end(), [](uint8_t v) { return v == 0; }) && ang_seeds_ok(1) && ang_seeds_ok(3) &&
         !ang_seeds_ok(0) && !ang_seeds_ok(4);
}

int main(int argc, char **argv) {
  if (argc == 2 && std::string(argv[1]) == "rules") {
    if (!candidates_ok()) return 3;
    if (!top_ok()) return 4;
    if (!arguments_ok()) return 5;
    printf("angular_refine rules: ok\n");
    return 0;
  }
  if (argc != 4 || std::string(argv[1]) != "run") return 2;
  FILE *in = fopen(argv[2], "rb");
  if (!in) return 2;
  int32_t hdr[5];
  if (!rd(in, hdr, 5)) return 2;
  const int w = hdr[0], h = hdr[1], nf = hdr[2], bias = hdr[3], njobs = hdr[4];
  const size_t fs = (size_t)w * h, ncu = (size_t)((w + 127) / 128) * ((h + 127) / 128) * MIP_CUS_PER_CTU;
  // (exact-size heap arrays: a read past a frame's end is an AddressSanitizer report)
  std::vector<uint16_t> frames(nf * fs), refs(nf * fs);
  std::vector<uint8_t> unavail(ncu), mode0(nf * ncu);
  std::vector<int32_t> best0(nf * ncu);
  if (!rd(in, frames.data(), frames.size()) || !rd(in, refs.data(), refs.size()) || !rd(in, unavail.data(), ncu) ||
      !rd(in, mode0.data(), mode0.size()) || !rd(in, best0.data(), best0.size()))
    return 2;
  FILE *out = fopen(argv[3], "wb");
  if (!out) return 2;
  for (int job = 0; job < njobs; job++) {
    int32_t js[2];
    if (!rd(in, js, 2) || js[1] < 0 || js[1] > 65) return 2;
    std::vector<uint8_t> list(js[1]);
    if (!rd(in, list.data(), list.size())) return 2;
    std::vector<int32_t> cost(nf * ncu * 65, -7), sad(cost), satd(cost), ang_cost(nf * ncu, -7), best(best0);
    std::vector<uint8_t> ang_mode(nf * ncu, 0x5a), tried(nf * ncu, 0x5a), mode(mode0);
    if (angular_refine_frames_host(frames.data(), refs.data(), unavail.data(), w, h, nf, js[1] ? list.data() : nullptr, js[1], js[0],
                                   cost.data(), sad.data(), satd.data(), ang_mode.data(), ang_cost.data(), tried.data(), bias,
                                   mode.data(), best.data()) != 0)
      return 4;
    if (!(wr(out, cost.data(), cost.size()) && wr(out, sad.data(), sad.size()) && wr(out, satd.data(), satd.size()) &&
          wr(out, ang_mode.data(), ang_mode.size()) && wr(out, ang_cost.data(), ang_cost.size()) && wr(out, tried.data(), tried.size()) &&
          wr(out, mode.data(), mode.size()) && wr(out, best.data(), best.size())))
      return 2;
  }
  fclose(in);
  fclose(out);
  printf("angular_refine: ok\n");
  return 0;
}
