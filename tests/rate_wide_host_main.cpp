/* Stand-alone host check of the edge-record rate planner
 * (opengemini_amd/csrc/gemx_ratewide.hpp). Built with sanitizers by
 * test_rate_wide_host.py; exits 0 when every invariant holds.
 *
 * Each case on the command line is
 *   start end range step nseg min_0 max_0 ... min_{n-1} max_{n-1}
 * (one series, segments in time order). For every case the program plans
 * the series and checks, against the ownership rule applied edge by edge:
 *  - every left / right edge lies in the run of at most one segment, and
 *    that segment is the rule's owner (first max_time >= L_o, last
 *    min_time <= R_o);
 *  - an ordinal has a row exactly when both its edges have an owner;
 *  - owners are monotone in o, the runs tile the row range in segment order;
 *  - record bases are contiguous and records <= 2 * grid steps.
 * It prints "grid n_ord s_min n_steps records" and one
 * "seg k l0 nl r0 nr" line per segment, which the test compares with numpy. */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gemx_ratewide.hpp"

static int fail(const char *what, long long a, long long b) {
  printf("invariant: %s (%lld, %lld)\n", what, a, b);
  return 1;
}

static int run_case(int64_t start, int64_t end, int64_t range, int64_t step,
                    const std::vector<int64_t> &mn,
                    const std::vector<int64_t> &mx) {
  const uint32_t n = (uint32_t)mn.size();
  RateWideGrid g;
  if (ratew_grid(start, end, range, step, &g)) return fail("grid refused", 0, 0);
  std::vector<RateWideSeg> seg(n);
  RateWideSeries ser;
  ser.sid = 1;
  ser.seg_start = 0;
  ser.seg_count = n;
  ser.out_base = 0;
  ser._pad = 0;
  uint64_t recs = 1000; /* a non-zero base: bases must be relative to it */
  ratew_plan_series(mn.data(), mx.data(), n, start, g, seg.data(), &ser, &recs);
  recs -= 1000;
  printf("grid %lld %lld %u %llu\n", (long long)g.n_ord, (long long)ser.s_min,
         ser.n_steps, (unsigned long long)recs);
  for (uint32_t k = 0; k < n; k++)
    printf("seg %u %lld %u %lld %u\n", k, (long long)seg[k].l0, seg[k].nl,
           (long long)seg[k].r0, seg[k].nr);

  if (recs > 2 * (uint64_t)g.n_ord) return fail("records > 2*steps", recs, g.n_ord);
  if (recs != 2 * (uint64_t)ser.n_steps) return fail("records != 2*rows", recs, ser.n_steps);
  const int64_t s_lo = ser.s_min, s_hi = ser.s_min + (int64_t)ser.n_steps;
  if (s_lo < 0 || s_hi > g.n_ord) return fail("rows off the grid", s_lo, s_hi);
  uint64_t base = 1000;
  int64_t la = s_lo, ra = s_lo;
  for (uint32_t k = 0; k < n; k++) {
    if (seg[k].rec_base != base) return fail("record base", k, (long long)base);
    base += (uint64_t)seg[k].nl + seg[k].nr;
    if (seg[k].l0 != la) return fail("left runs do not tile", k, la);
    if (seg[k].r0 != ra) return fail("right runs do not tile", k, ra);
    la += seg[k].nl;
    ra += seg[k].nr;
  }
  if (la != s_hi || ra != s_hi) return fail("runs do not end at s_hi", la, ra);

  int64_t prev_lo = -1, prev_ro = -1;
  for (int64_t o = 0; o < g.n_ord; o++) {
    const int64_t R = g.start_sample + o * g.eff_step, L = R - range;
    int64_t lo = -1, ro = -1; /* the rule's owners */
    for (uint32_t k = 0; k < n; k++)
      if (mx[k] >= L) { lo = k; break; }
    for (uint32_t k = n; k-- > 0;)
      if (mn[k] <= R) { ro = k; break; }
    int64_t nlo = 0, nro = 0, got_lo = -1, got_ro = -1;
    for (uint32_t k = 0; k < n; k++) {
      if (o >= seg[k].l0 && o < seg[k].l0 + (int64_t)seg[k].nl) { nlo++; got_lo = k; }
      if (o >= seg[k].r0 && o < seg[k].r0 + (int64_t)seg[k].nr) { nro++; got_ro = k; }
    }
    if (nlo > 1 || nro > 1) return fail("edge with two owners", o, nlo + nro);
    const bool row = o >= s_lo && o < s_hi;
    if (row != (lo >= 0 && ro >= 0)) return fail("row without both owners", o, row);
    if (row) {
      if (got_lo != lo) return fail("left owner", o, got_lo);
      if (got_ro != ro) return fail("right owner", o, got_ro);
      if (lo < prev_lo || ro < prev_ro) return fail("owners not monotone", o, lo);
      prev_lo = lo;
      prev_ro = ro;
    } else if (nlo || nro) {
      return fail("record outside the rows", o, nlo + nro);
    }
  }
  return 0;
}

int main(int argc, char **argv) {
  int a = 1, cases = 0;
  while (a + 4 < argc) {
    const int64_t start = atoll(argv[a]), end = atoll(argv[a + 1]),
                  range = atoll(argv[a + 2]), step = atoll(argv[a + 3]);
    const int n = atoi(argv[a + 4]);
    a += 5;
    if (n < 1 || a + 2 * n > argc) {
      printf("bad arguments\n");
      return 2;
    }
    std::vector<int64_t> mn(n), mx(n);
    for (int k = 0; k < n; k++) {
      mn[k] = atoll(argv[a + 2 * k]);
      mx[k] = atoll(argv[a + 2 * k + 1]);
    }
    a += 2 * n;
    if (run_case(start, end, range, step, mn, mx)) return 1;
    cases++;
  }
  /* a grid too long for a plan is refused, not wrapped */
  RateWideGrid g;
  if (ratew_grid(0, INT64_MAX - 1, 1, 1, &g) == 0) return fail("long grid accepted", 0, 0);
  if (ratew_grid(10, 5, 1, 1, &g) != 0 || g.n_ord != 0) return fail("empty grid", 0, 0);
  printf("ok %d\n", cases);
  return 0;
}
