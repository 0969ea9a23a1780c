/* Stand-alone host check of the per-cell *_over_time planner and folds
 * (opengemini_amd/csrc/gemx_otwide.hpp). Built with sanitizers by
 * test_ot_wide_host.py; exits 0 when every invariant holds.
 *
 * Each case on the command line is
 *   start end range step nseg min_0 max_0 ... min_{n-1} max_{n-1}
 * (one series, segments in descriptor order). For every case the program
 * plans the series and checks:
 *  - otw_cell and otw_row_cells equal the formulas over ratew_left_le /
 *    ratew_right_lt, and otw_cell_next names the first time of another cell;
 *  - a_o and b_o are monotone, widths never exceed W, and a row folds its
 *    cells directly only when it is narrower than W;
 *  - slot, state and block bases are relative to the caller's, a segment's
 *    cell range holds the cell of each of its bounds, every cell index the
 *    folds form lies inside the buffers;
 *  - with one point per second inside every segment, the block scheme
 *    (cells, C, P, Q, row join: the functions the kernels call) gives for
 *    count, min, max, last, changes and resets exactly what a walk over the
 *    window's points gives.
 * It prints "grid n_ord W B slots states blocks s_min n_steps cmin ncell",
 * one "seg k c0 ncells" per segment, one "ord o a b kind" per ordinal and
 * one "probe t cell" per probe time (every edge, every edge +- 1, every
 * segment bound), which the test checks with numpy. */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gemx_otwide.hpp"

static int fail(const char *what, long long a, long long b) {
  printf("invariant: %s (%lld, %lld)\n", what, a, b);
  return 1;
}

static const char *KIND[4] = {"join", "prefix", "suffix", "fold"};

struct Pt {
  int64_t t;
  double v;
};

/* the window's value by a plain walk over its points; false: no point */
static bool direct(const std::vector<Pt> &pts, int64_t L, int64_t R, int func,
                   double *out) {
  OtRun run;
  otw_run_reset(run);
  int64_t n = 0, hits = 0;
  double mn = 0, mx = 0, last = 0;
  for (const Pt &p : pts) {
    if (p.t < L || p.t > R) continue;
    if (n == 0) mn = mx = p.v;
    if (p.v < mn) mn = p.v;
    if (p.v > mx) mx = p.v;
    if (n > 0) {
      if (func == OTW_F_CHANGES && p.v != last) hits++;
      if (func == OTW_F_RESETS && p.v < last) hits++;
    }
    last = p.v;
    n++;
  }
  if (func == OTW_F_ABSENT) {
    *out = 1.0;
    return n == 0;
  }
  if (n == 0) return false;
  switch (func) {
  case OTW_F_COUNT: *out = (double)n; break;
  case OTW_F_MIN: *out = mn; break;
  case OTW_F_MAX: *out = mx; break;
  case OTW_F_LAST: *out = last; break;
  case OTW_F_PRESENT: *out = 1.0; break;
  default: *out = (double)hits; break;
  }
  return true;
}

template <int CLS>
static int emulate(int func, int64_t start, int64_t range,
                   const RateWideGrid &g, const std::vector<int64_t> &mn,
                   const std::vector<int64_t> &mx,
                   const std::vector<OtWideSeg> &seg, const OtWideSeries &ser,
                   uint64_t slot0, uint64_t nslots, uint64_t nstates) {
  const uint32_t n = (uint32_t)mn.size();
  const int64_t k = otw_ratio(range, g.eff_step, g.n_ord);
  const int64_t blk = otw_block_len(k, g.n_ord);
  /* stage 1: one state per (segment, cell), the scan's flush rule */
  std::vector<OtState> slots(nslots, otw_identity());
  std::vector<Pt> all;
  uint32_t lcg = 12345u + (uint32_t)func;
  for (uint32_t s = 0; s < n; s++) {
    /* at most 600 points a segment: both bounds, then a fixed stride */
    int64_t span = mx[s] - mn[s];
    int64_t dt = span / 600 + 1;
    if (dt < 1000000000ll && span >= 1000000000ll) dt = 1000000000ll;
    OtRun run;
    otw_run_reset(run);
    int64_t cur = -1;
    for (int64_t t = mn[s];; t += dt) {
      if (t > mx[s]) t = mx[s];
      lcg = lcg * 1664525u + 1013904223u;
      const double v = (double)((lcg >> 16) % 3);
      all.push_back({t, v});
      int64_t c = otw_cell(t, start, g.start_sample, g.eff_step, g.n_ord) - seg[s].c0;
      if (c < 0 || c >= (int64_t)seg[s].ncells) return fail("cell off the segment's slots", s, c);
      if (c < cur) return fail("cell steps back", s, c);
      if (c > cur) {
        if (cur >= 0) slots[seg[s].slot_base - slot0 + (uint64_t)cur] = otw_flush<CLS>(run);
        otw_run_reset(run);
        cur = c;
      }
      otw_update<CLS>(run, v, func);
      if (t == mx[s]) break;
    }
    if (cur >= 0) slots[seg[s].slot_base - slot0 + (uint64_t)cur] = otw_flush<CLS>(run);
  }
  /* stages 2-4 with the kernels' own functions, on exactly sized buffers
   * so that the sanitizer sees any index off them */
  std::vector<OtWideSeg> sg(seg);
  for (auto &q : sg) q.slot_base -= slot0;
  OtWideSeries s = ser;
  s.state_base = 0;
  s.seg_start = 0;
  std::vector<OtState> C(nstates), P(nstates), Q(nstates);
  const int64_t cmax = s.cmin + (int64_t)s.ncell - 1;
  for (int64_t b = s.cmin / blk; b <= cmax / blk; b++)
    otw_fold_block<CLS>(s, sg.data(), slots.data(), C.data(), P.data(), Q.data(),
                        b, blk, func);
  for (int64_t o = 0; o < g.n_ord; o++) {
    int64_t a, b;
    otw_row_cells(o, k, g.n_ord, &a, &b);
    int kind;
    const OtState st = otw_row_state<CLS>(s, C.data(), P.data(), Q.data(), a, b,
                                          blk, func, &kind);
    double got = 0, want = 0;
    const bool hg = otw_finalise(st, func, &got);
    const int64_t L = start + o * g.eff_step;
    const bool hw = direct(all, L, L + range, func, &want);
    if (hg != hw) return fail("row presence", o, func);
    if (hg && got != want) return fail("row value", o, func);
  }
  return 0;
}

static int run_case(int64_t start, int64_t end, int64_t range, int64_t step,
                    const std::vector<int64_t> &mn,
                    const std::vector<int64_t> &mx) {
  const uint32_t n = (uint32_t)mn.size();
  RateWideGrid g;
  if (ratew_grid(start, end, range, step, &g)) return fail("grid refused", 0, 0);
  if (g.n_ord == 0) {
    printf("grid 0 0 0 0 0 0 0 0 0 0\n");
    return 0;
  }
  std::vector<OtWideSeg> seg(n);
  OtWideSeries ser;
  ser.sid = 1;
  ser.seg_start = 0;
  ser.seg_count = n;
  ser.out_base = 0;
  /* non-zero bases: everything planned must be relative to them */
  uint64_t slots = 1000, states = 2000, blocks = 3000;
  otw_plan_series(mn.data(), mx.data(), n, start, range, g, seg.data(), &ser,
                  &slots, &states, &blocks);
  slots -= 1000;
  states -= 2000;
  blocks -= 3000;
  const int64_t k = otw_ratio(range, g.eff_step, g.n_ord);
  const int64_t W = 2 * (range / g.eff_step) + 1;
  const int64_t blk = otw_block_len(k, g.n_ord);
  printf("grid %lld %lld %lld %llu %llu %llu %lld %u %lld %u\n",
         (long long)g.n_ord, (long long)W, (long long)blk,
         (unsigned long long)slots, (unsigned long long)states,
         (unsigned long long)blocks, (long long)ser.s_min, ser.n_steps,
         (long long)ser.cmin, ser.ncell);
  if (ser.state_base != 2000 || ser.blk_base != 3000) return fail("series bases", 0, 0);
  if (states != ser.ncell) return fail("states != ncell", states, ser.ncell);
  const int64_t cmax = ser.cmin + (int64_t)ser.ncell - 1;
  if (ser.cmin < 0 || cmax > 2 * g.n_ord) return fail("series cells off the axis", ser.cmin, cmax);
  if (blocks != (uint64_t)(cmax / blk - ser.cmin / blk + 1)) return fail("block count", blocks, blk);
  uint64_t base = 1000;
  for (uint32_t s = 0; s < n; s++) {
    printf("seg %u %lld %u\n", s, (long long)seg[s].c0, seg[s].ncells);
    if (seg[s].slot_base != base) return fail("slot base", s, (long long)base);
    base += seg[s].ncells;
    const int64_t c0 = otw_cell(mn[s], start, g.start_sample, g.eff_step, g.n_ord);
    const int64_t c1 = otw_cell(mx[s], start, g.start_sample, g.eff_step, g.n_ord);
    if (c0 != seg[s].c0 || c1 != seg[s].c0 + (int64_t)seg[s].ncells - 1)
      return fail("segment cells", s, c0);
    if (seg[s].c0 < ser.cmin || c1 > cmax) return fail("segment off the series", s, c1);
  }

  int64_t pa = -1, pb = -1;
  for (int64_t o = 0; o < g.n_ord; o++) {
    int64_t a, b;
    otw_row_cells(o, k, g.n_ord, &a, &b);
    const int64_t L = start + o * g.eff_step, R = L + range;
    const int64_t a2 = o + 1 + ratew_right_lt(L, g);
    const int64_t b2 = o + ratew_left_le(R, start, g);
    if (a != a2 || b != b2) return fail("row cells differ from the edge counts", a, a2);
    if (a < pa || b < pb) return fail("row cells not monotone", o, a);
    if (a > b) return fail("empty cell range", a, b);
    if (a < 1 || b > 2 * g.n_ord - 1) return fail("row cells off the axis", a, b);
    if (b - a + 1 > W) return fail("wider than W", o, b - a + 1);
    pa = a;
    pb = b;
    const int kind = otw_row_kind(a, b, blk);
    if (kind == OTW_FOLD && b - a + 1 >= W) return fail("full-width row folds", o, kind);
    if (kind == OTW_JOIN && b / blk != a / blk + 1) return fail("join not adjacent", a, b);
    printf("ord %lld %lld %lld %s\n", (long long)o, (long long)a, (long long)b, KIND[kind]);
  }

  std::vector<int64_t> probes;
  for (int64_t o = 0; o < g.n_ord; o++) {
    const int64_t L = start + o * g.eff_step, R = L + range;
    for (int64_t d = -1; d <= 1; d++) {
      probes.push_back(L + d);
      probes.push_back(R + d);
    }
  }
  for (uint32_t s = 0; s < n; s++) {
    probes.push_back(mn[s]);
    probes.push_back(mx[s]);
  }
  for (int64_t t : probes) {
    int64_t cut;
    const int64_t c = otw_cell_next(t, start, g.start_sample, g.eff_step, g.n_ord, &cut);
    if (c != ratew_left_le(t, start, g) + ratew_right_lt(t, g))
      return fail("cell differs from the edge counts", t, c);
    if (c < 0 || c > 2 * g.n_ord) return fail("cell off the axis", t, c);
    if (cut <= t) return fail("next cut not after t", t, cut);
    if (cut != INT64_MAX) {
      if (otw_cell(cut, start, g.start_sample, g.eff_step, g.n_ord) == c)
        return fail("no new cell at the cut", t, cut);
      if (otw_cell(cut - 1, start, g.start_sample, g.eff_step, g.n_ord) != c)
        return fail("new cell before the cut", t, cut);
    } else if (c != 2 * g.n_ord) {
      return fail("no cut before the last cell", t, c);
    }
    printf("probe %lld %lld\n", (long long)t, (long long)c);
  }
  printf("end\n");

  int rc = 0;
  rc = rc || emulate<OTW_C_LAST>(OTW_F_COUNT, start, range, g, mn, mx, seg, ser, 1000, slots, states);
  rc = rc || emulate<OTW_C_LAST>(OTW_F_LAST, start, range, g, mn, mx, seg, ser, 1000, slots, states);
  rc = rc || emulate<OTW_C_LAST>(OTW_F_ABSENT, start, range, g, mn, mx, seg, ser, 1000, slots, states);
  rc = rc || emulate<OTW_C_MINMAX>(OTW_F_MIN, start, range, g, mn, mx, seg, ser, 1000, slots, states);
  rc = rc || emulate<OTW_C_MINMAX>(OTW_F_MAX, start, range, g, mn, mx, seg, ser, 1000, slots, states);
  rc = rc || emulate<OTW_C_CHG>(OTW_F_CHANGES, start, range, g, mn, mx, seg, ser, 1000, slots, states);
  rc = rc || emulate<OTW_C_CHG>(OTW_F_RESETS, start, range, g, mn, mx, seg, ser, 1000, slots, states);
  return rc;
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
  /* a ratio far beyond the grid clamps instead of overflowing */
  if (otw_ratio(INT64_MAX, 1, 5) != 5 || otw_block_len(5, 5) != 11)
    return fail("ratio clamp", 0, 0);
  /* unsupported codes have no class */
  const int bad[] = {0, 1, 13, 14, 16, 17, 18, -1, 19};
  for (int f : bad)
    if (otw_class_of(f) != OTW_C_NONE) return fail("class for a refused func", f, 0);
  printf("ok %d\n", cases);
  return 0;
}
