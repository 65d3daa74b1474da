// Stand-alone host program over csrc/convT_stack_plan.h (built with -fsanitize=address,undefined by
// tests/test_convT_stack_cpu.py): the (class, offset) tables, the pack index map into a real buffer, and the plan
// over a sweep of shapes.  Prints "ok <plans>" and returns 0, or prints what failed and returns 1.
#include <cstdio>
#include <vector>

#include "convT_stack_plan.h"

namespace cts = tb::cts;

static int fail(const char* what, long a = 0, long b = 0, long c = 0) {
  std::printf("FAIL %s %ld %ld %ld\n", what, a, b, c);
  return 1;
}

int main() {
  // tables: 27 pairs, each tap once, ranks dense per offset
  int pairs = 0;
  bool seen[27] = {};
  for (int o = 0; o < 8; ++o) {
    bool rk[8] = {};
    int n = 0;
    for (int cls = 0; cls < 8; ++cls) {
      if (!cts::uses(cls, o)) continue;
      const int r = cts::rank_of(cls, o), t = cts::tap_index(cls, o);
      if (r < 0 || r >= cts::ncls_of(o) || rk[r]) return fail("rank", cls, o, r);
      rk[r] = true;
      if (t < 0 || t >= 27 || seen[t]) return fail("tap", cls, o, t);
      seen[t] = true;
      int c2, o2;
      cts::pair_of_tap(t, c2, o2);
      if (c2 != cls || o2 != o) return fail("pair_of_tap", t, c2, o2);
      ++n, ++pairs;
    }
    if (n != cts::ncls_of(o) || cts::pair_base(o) != pairs - n) return fail("ncls", o, n, pairs);
  }
  if (pairs != 27) return fail("pairs", pairs);
  // the pack index is a bijection onto [0, 27 Cin Cout)
  for (int Cout : {32, 64})
    for (int Cin : {32, 128, 384}) {
      const long total = 27L * Cin * Cout;
      std::vector<unsigned char> hit((size_t)total, 0);
      for (int c = 0; c < Cin; ++c)
        for (int m = 0; m < Cout; ++m)
          for (int t = 0; t < 27; ++t) {
            const long i = (long)cts::pack_index(Cin, c, m, t);
            if (i < 0 || i >= total) return fail("pack range", c, m, t);
            if (hit[(size_t)i]++) return fail("pack twice", c, m, t);
          }
    }
  // plans
  long plans = 0;
  for (int N : {1, 2, 3})
    for (int Cin : {32, 64, 128, 256, 384, 1024})
      for (int Cout : {32, 64})
        for (int D : {1, 2, 15, 30, 61})
          for (int W : {1, 5, 20, 97})
            for (int cu : {1, 64, 256, 304})
              for (int force : {0, 1, 3, 100}) {
                cts::Plan pl;
                const int rc = cts::make_plan(N, Cin, Cout, D, D, W, cu, force, pl);
                if (rc == 2) continue;
                if (rc != 0) return fail("rc", rc);
                if (pl.nsplit < 1 || pl.cper < 1 || (pl.nsplit - 1) * pl.cper >= pl.CB || pl.nsplit * pl.cper < pl.CB)
                  return fail("slices", pl.nsplit, pl.cper, pl.CB);
                if ((long)pl.ptiles * cts::BP < pl.P || (long)(pl.ptiles - 1) * cts::BP >= pl.P) return fail("ptiles");
                if (pl.ws_bytes() < pl.pack_bytes() + 4 * (size_t)pl.part_floats) return fail("ws");
                if (pl.nsplit > 1 && pl.part_floats != (long)pl.nsplit * 8 * Cout * pl.P) return fail("part");
                ++plans;
              }
  cts::Plan pl;
  if (cts::make_plan(1, 40, 32, 2, 2, 2, 256, 0, pl) != 2 || cts::make_plan(1, 64, 16, 2, 2, 2, 256, 0, pl) != 2 ||
      cts::make_plan(0, 64, 32, 2, 2, 2, 256, 0, pl) != 1 || cts::make_plan(4, 1024, 64, 64, 64, 64, 256, 0, pl) != 2)
    return fail("refusals");
  std::printf("ok %ld\n", plans);
  return 0;
}
