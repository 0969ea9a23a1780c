/* rate()/irate() for any range/step ratio: per-segment edge records.
 *
 * A window [ts-range, ts] over a series' time-sorted point stream is a
 * prefix difference: its count and counter-reset sum are (stream state at
 * the right edge) - (stream state at the left edge), its first point is the
 * first point at or after the left edge, its last two points are the stream
 * tail at the right edge. So a window needs two records, one per edge, and
 * nothing per (segment, step it touches): storage and merge work follow the
 * number of steps, never the range.
 *
 *   step o:  L_o = ts_o - range (left edge),  R_o = ts_o (right edge)
 *   left  owner: the first segment of the series with max_time >= L_o
 *   right owner: the last  segment of the series with min_time <= R_o
 *
 * Both owners are monotone in o, so each segment owns one contiguous run of
 * left ordinals and one of right ordinals. k_rate_edges decodes a segment
 * once, advancing two cursors over its runs; k_rate_edge_merge joins a left
 * and a right record per output row and adds the whole-segment summaries
 * strictly between the two owners.
 *
 * The planner (first part of this file) is plain C++ with no engine state,
 * so it can be compiled into a stand-alone host program; the kernels and the
 * query entry points need hipcc and the engine's decoders. */
#pragma once
#include <cstdint>
#include <vector>

/* ---------------- host planner (descriptors only) ---------------- */

struct RateWideSeg {
  int64_t l0, r0;    /* first left / right ordinal this segment owns */
  uint64_t rec_base; /* nl left records, then nr right records */
  uint32_t nl, nr;
};

struct RateWideSeries {
  uint64_t sid;
  int64_t s_min;     /* first ordinal that has both owners */
  uint64_t out_base; /* dense output row of s_min */
  uint32_t n_steps;
  uint32_t seg_start, seg_count;
  uint32_t _pad;
};

struct RateWideGrid {
  int64_t start_sample; /* ts of ordinal 0 */
  int64_t eff_step;     /* step, or 1 for the single sample of step == 0 */
  int64_t n_ord;        /* samples on the grid; 0 when end < start + range */
};

/* Sampling grid of the RangeVectorCursor (prom_range_vector_cursor.go:55-68).
 * Returns 0, or -1 when the grid holds more steps than a plan can index. */
static inline int ratew_grid(int64_t start_time, int64_t end_time,
                             int64_t range_ns, int64_t step_ns,
                             RateWideGrid *g) {
  g->start_sample = start_time + range_ns;
  g->eff_step = step_ns ? step_ns : 1;
  g->n_ord = 0;
  if (end_time < g->start_sample) return 0;
  const uint64_t span = (uint64_t)end_time - (uint64_t)g->start_sample;
  const uint64_t last = step_ns ? span / (uint64_t)step_ns : 0;
  if (last >= 0x7fffffffull) return -1;
  g->n_ord = (int64_t)last + 1;
  return 0;
}

/* ordinals o in [0, n_ord) with left edge start_time + o*step <= x */
static inline int64_t ratew_left_le(int64_t x, int64_t start_time,
                                    const RateWideGrid &g) {
  if (x < start_time) return 0;
  const uint64_t k =
      ((uint64_t)x - (uint64_t)start_time) / (uint64_t)g.eff_step;
  return k >= (uint64_t)g.n_ord ? g.n_ord : (int64_t)k + 1;
}

/* ordinals o in [0, n_ord) with right edge start_sample + o*step < x */
static inline int64_t ratew_right_lt(int64_t x, const RateWideGrid &g) {
  if (x <= g.start_sample) return 0;
  const uint64_t k =
      ((uint64_t)x - (uint64_t)g.start_sample - 1) / (uint64_t)g.eff_step;
  return k >= (uint64_t)g.n_ord ? g.n_ord : (int64_t)k + 1;
}

static inline int64_t ratew_clamp(int64_t v, int64_t lo, int64_t hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

/* One series: segments [0, n) in descriptor (time) order with their
 * min_time / max_time. Fills seg[0..n) and *ser (sid, seg_start, seg_count
 * and out_base are the caller's); record bases start at *rec_base, which
 * advances by the records allocated. Only ordinals with both owners get
 * rows and records, so records = 2 * n_steps <= 2 * grid steps.
 *
 * max_time is taken as a running maximum and min_time as a running minimum
 * from the right, so that the owners stay monotone (and every index the
 * kernels form stays in bounds) for segments that overlap in time. */
static inline void ratew_plan_series(const int64_t *min_time,
                                     const int64_t *max_time, uint32_t n,
                                     int64_t start_time, const RateWideGrid &g,
                                     RateWideSeg *seg, RateWideSeries *ser,
                                     uint64_t *rec_base) {
  std::vector<int64_t> rmin(n);
  for (uint32_t k = n; k-- > 0;)
    rmin[k] = (k + 1 < n && rmin[k + 1] < min_time[k]) ? rmin[k + 1]
                                                       : min_time[k];
  int64_t rmax = max_time[0];
  for (uint32_t k = 1; k < n; k++)
    if (max_time[k] > rmax) rmax = max_time[k];
  /* rows: right edge at or after the first point, left edge at or before
   * the last one */
  const int64_t s_lo = ratew_right_lt(rmin[0], g);
  int64_t s_hi = ratew_left_le(rmax, start_time, g);
  if (s_hi < s_lo) s_hi = s_lo;
  ser->s_min = s_lo;
  ser->n_steps = (uint32_t)(s_hi - s_lo);
  int64_t la = s_lo; /* left ordinals below la belong to earlier segments */
  int64_t run_max = max_time[0];
  for (uint32_t k = 0; k < n; k++) {
    if (max_time[k] > run_max) run_max = max_time[k];
    const int64_t lb =
        ratew_clamp(ratew_left_le(run_max, start_time, g), la, s_hi);
    const int64_t ra = ratew_clamp(ratew_right_lt(rmin[k], g), s_lo, s_hi);
    const int64_t rb =
        k + 1 < n ? ratew_clamp(ratew_right_lt(rmin[k + 1], g), ra, s_hi)
                  : s_hi;
    seg[k].l0 = la;
    seg[k].nl = (uint32_t)(lb - la);
    seg[k].r0 = ra;
    seg[k].nr = (uint32_t)(rb - ra);
    seg[k].rec_base = *rec_base;
    *rec_base += (uint64_t)seg[k].nl + seg[k].nr;
    la = lb;
  }
}

#ifdef __HIPCC__

/* ---------------- device ---------------- */

/* One edge record. Left edge: (t, v) = first point with t >= L_o, count =
 * segment point count after it (1-based position), reset = segment reset sum
 * after its pair. Right edge: (t, v) = last point with t <= R_o, (t2, v2) =
 * the point before it (valid when count >= 2), count / reset = segment
 * totals up to and including it. count == 0: the segment holds no usable
 * point on the wanted side of the edge. */
struct RateEdgeRec {
  int64_t t;
  double v;
  int64_t t2;
  double v2;
  int64_t count;
  double reset;
};

/* Whole-segment summary: first usable point, last two, totals. */
struct RateSegSum {
  int64_t first_t, last_t, prev_t;
  double first_v, last_v, prev_v;
  int64_t count;
  double reset;
};

template <int FAST>
__global__ void __launch_bounds__(256) k_rate_edges(
    const uint8_t *__restrict__ blob, const uint64_t *__restrict__ arena,
    const GorDesc *__restrict__ gors, const gemx_seg_desc *__restrict__ descs,
    const RateWideSeg *__restrict__ wseg, const uint32_t *__restrict__ seg_ids,
    uint32_t nseg_ids, RateEdgeRec *__restrict__ recs,
    RateSegSum *__restrict__ sums, int64_t start_time, int64_t start_sample,
    int64_t step_ns, uint8_t *__restrict__ scratch, uint64_t scratch_per_lane,
    uint32_t nlanes, unsigned long long *__restrict__ points, DevErr *err) {
  uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t stride = FAST ? gridDim.x * blockDim.x : nlanes;
  if (!FAST && gid >= nlanes) return;

  for (uint32_t li = gid; li < nseg_ids; li += stride) {
    uint32_t si = seg_ids[li];
    const gemx_seg_desc d = descs[si];
    const RateWideSeg wq = wseg[si];
    int rows = (int)d.rows;
    RateEdgeRec *lrec = recs + wq.rec_base;
    RateEdgeRec *rrec = lrec + wq.nl;

    /* fast: streaming reader; general: buffered into per-lane scratch
     * (gemx_segdecode.hpp) */
    SegStream<GEMX_TYPE_FLOAT> st;
    SegBuffered<GEMX_TYPE_FLOAT> sb;
    if (int rc = FAST ? st.open(blob, arena, gors, si, d)
                      : sb.decode(blob, d, scratch + (uint64_t)gid * scratch_per_lane)) {
      set_err(err, rc);
      return;
    }

    /* stream state of this segment (the sh_* state of k_rate_scan) */
    int64_t cnt = 0;
    double reset = 0;
    int64_t first_t = 0, last_t = 0, prev_t = 0;
    double first_v = 0, last_v = 0, prev_v = 0;
    /* the two cursors: next unanswered left / right edge of this segment */
    uint32_t lcur = 0, rcur = 0;
    int64_t next_L = wq.nl ? start_time + wq.l0 * step_ns : 0;
    int64_t next_R = wq.nr ? start_sample + wq.r0 * step_ns : 0;

    for (int i = 0; i < rows; i++) {
      int64_t t, bits = 0;
      int valid = 1;
      if (int rc = FAST ? st.next(i, &t, &bits) : sb.row(i, &t, &bits, &valid)) {
        set_err(err, rc);
        return;
      }
      if (!valid) continue;
      const double fv = d_bits_f(bits);
      if (fv != fv) continue; /* FilterRangeNANPoint */

      /* right edges this point lies beyond: the stream before it is their
       * answer (count 0: nothing at or before the edge in this segment) */
      while (rcur < wq.nr && t > next_R) {
        RateEdgeRec r;
        r.t = last_t;
        r.v = last_v;
        r.t2 = prev_t;
        r.v2 = prev_v;
        r.count = cnt;
        r.reset = reset;
        rrec[rcur] = r;
        if (++rcur < wq.nr) next_R += step_ns; /* stays on the grid */
      }
      /* stream update */
      if (cnt > 0 && fv < last_v) reset += last_v; /* agg_func_prom.go:236-250 */
      prev_t = last_t;
      prev_v = last_v;
      last_t = t;
      last_v = fv;
      if (cnt == 0) {
        first_t = t;
        first_v = fv;
      }
      cnt++;
      /* left edges this point is the first to reach */
      while (lcur < wq.nl && t >= next_L) {
        RateEdgeRec r;
        r.t = t;
        r.v = fv;
        r.t2 = 0;
        r.v2 = 0;
        r.count = cnt;   /* position of the first in-window point */
        r.reset = reset; /* the pair (previous, this) is not in the window */
        lrec[lcur] = r;
        if (++lcur < wq.nl) next_L += step_ns;
      }
    }
    /* edges beyond the last point: right edges see the whole segment, left
     * edges found nothing here */
    for (; rcur < wq.nr; rcur++) {
      RateEdgeRec r;
      r.t = last_t;
      r.v = last_v;
      r.t2 = prev_t;
      r.v2 = prev_v;
      r.count = cnt;
      r.reset = reset;
      rrec[rcur] = r;
    }
    for (; lcur < wq.nl; lcur++) {
      RateEdgeRec r;
      r.t = 0;
      r.v = 0;
      r.t2 = 0;
      r.v2 = 0;
      r.count = 0;
      r.reset = 0;
      lrec[lcur] = r;
    }
    RateSegSum sm;
    sm.first_t = first_t;
    sm.first_v = first_v;
    sm.last_t = last_t;
    sm.last_v = last_v;
    sm.prev_t = prev_t;
    sm.prev_v = prev_v;
    sm.count = cnt;
    sm.reset = reset;
    sums[si] = sm;
    if (cnt) atomicAdd(points, (unsigned long long)cnt);
  }
}

/* rate()/increase()/delta() from a window's first/last point, count and
 * reset sum: the finalise arithmetic of k_rate_merge (CalcReduceResult +
 * floatPromRateMerge, clamp order as in oracle/agg.c prom_rate_value).
 * Returns false for a nil row. */
__device__ __forceinline__ bool ratew_finalise_rate(
    int64_t first_t, double first_v, int64_t last_t, double last_v,
    int64_t count, double reset_adj, int64_t ts, int64_t range_ns, int is_rate,
    int is_counter, double *value) {
  if (!(count > 1 && last_t != first_t && range_ns != 0)) return false;
  double reduce = (last_v - first_v) + (is_counter ? reset_adj : 0.0);
  int64_t range_start = ts - range_ns;
  double dur_to_start = (double)(first_t - range_start) / 1e9;
  double dur_to_end = (double)(ts - last_t) / 1e9;
  double sampled = (double)(last_t - first_t) / 1e9;
  double avg_dur = sampled / (double)(count - 1);
  if (is_counter && reduce > 0 && first_v >= 0) {
    double dz = sampled * (first_v / reduce);
    if (dz < dur_to_start) dur_to_start = dz;
  }
  double thresh = avg_dur * 1.1;
  double extrap = sampled;
  if (dur_to_start >= thresh) dur_to_start = avg_dur / 2;
  extrap += dur_to_start;
  if (dur_to_end >= thresh) dur_to_end = avg_dur / 2;
  extrap += dur_to_end;
  double result = reduce * (extrap / sampled);
  if (is_rate) result = result / ((double)range_ns / 1e9);
  *value = result;
  return true;
}

/* irate/idelta from the window's last two points (prom_functions.go:479-506),
 * as k_rate_merge's func == 1 branch. */
__device__ __forceinline__ bool ratew_finalise_irate(
    int64_t prev_t, double prev_v, int64_t last_t, double last_v,
    int64_t count, int64_t range_ns, int is_rate, double *value) {
  if (!(count >= 2 && last_t != prev_t && range_ns != 0)) return false;
  double rv;
  if (is_rate && last_v < prev_v)
    rv = last_v;
  else
    rv = last_v - prev_v;
  if (is_rate) rv /= (double)(last_t - prev_t) / 1e9;
  *value = rv;
  return true;
}

/* one thread per (series, step) row: join the left and the right record */
__global__ void __launch_bounds__(256) k_rate_edge_merge(
    const RateWideSeries *__restrict__ series, uint32_t nseries,
    const RateWideSeg *__restrict__ wseg, const RateEdgeRec *__restrict__ recs,
    const RateSegSum *__restrict__ sums, gemx_rate_row *__restrict__ rows,
    uint64_t total_rows, int64_t start_sample, int64_t step_ns,
    int64_t range_ns, int is_rate, int is_counter, int func,
    DevErr *__restrict__ err) {
  uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  for (uint64_t r = gid; r < total_rows; r += gridDim.x * (uint64_t)blockDim.x) {
    uint32_t lo = 0, hi = nseries - 1;
    while (lo < hi) {
      uint32_t mid = (lo + hi + 1) >> 1;
      if (series[mid].out_base <= r) lo = mid;
      else hi = mid - 1;
    }
    const RateWideSeries s = series[lo];
    const int64_t o = s.s_min + (int64_t)(r - s.out_base);
    const int64_t ts = start_sample + o * step_ns;
    const uint32_t sa = s.seg_start, sb = s.seg_start + s.seg_count;

    gemx_rate_row out;
    out.sid = s.sid;
    out.ts = ts;
    out.value = 0;
    out.isnil = 1;
    memset(out._pad, 0, sizeof(out._pad));

    /* owners: the runs tile [s_min, s_min + n_steps) in segment order, so
     * the owner is the first segment whose run ends beyond o */
    uint32_t a = sa, b = sa;
    {
      uint32_t flo = sa, fhi = sb - 1;
      while (flo < fhi) {
        uint32_t mid = (flo + fhi) >> 1;
        if (wseg[mid].l0 + (int64_t)wseg[mid].nl > o) fhi = mid;
        else flo = mid + 1;
      }
      a = flo;
      flo = sa;
      fhi = sb - 1;
      while (flo < fhi) {
        uint32_t mid = (flo + fhi) >> 1;
        if (wseg[mid].r0 + (int64_t)wseg[mid].nr > o) fhi = mid;
        else flo = mid + 1;
      }
      b = flo;
    }
    const RateWideSeg wa = wseg[a], wb = wseg[b];
    bool ok = o >= wa.l0 && o < wa.l0 + (int64_t)wa.nl && o >= wb.r0 &&
              o < wb.r0 + (int64_t)wb.nr;

    /* left end: first in-window point, its position and reset prefix */
    int64_t first_t = 0, lcount = 0;
    double first_v = 0, lreset = 0;
    if (ok) {
      const RateEdgeRec L = recs[wa.rec_base + (uint64_t)(o - wa.l0)];
      if (L.count > 0) {
        first_t = L.t;
        first_v = L.v;
        lcount = L.count;
        lreset = L.reset;
      } else {
        /* nothing at or after the edge in the owner: the window starts at
         * the first point of the next segment that has one */
        for (a++; a < sb && sums[a].count == 0; a++) {}
        if (a < sb) {
          first_t = sums[a].first_t;
          first_v = sums[a].first_v;
          lcount = 1;
          lreset = 0;
        } else {
          ok = false;
        }
      }
    }
    /* right end: last two in-window points, count and reset prefix */
    int64_t last_t = 0, prev_t = 0, rcount = 0;
    double last_v = 0, prev_v = 0, rreset = 0;
    if (ok) {
      const RateEdgeRec R = recs[wb.rec_base + wb.nl + (uint64_t)(o - wb.r0)];
      if (R.count > 0) {
        last_t = R.t;
        last_v = R.v;
        prev_t = R.t2;
        prev_v = R.v2;
        rcount = R.count;
        rreset = R.reset;
      } else {
        /* nothing at or before the edge in the owner: the window ends at
         * the tail of the previous segment that has points */
        int64_t bb = (int64_t)b - 1;
        for (; bb >= (int64_t)sa && sums[bb].count == 0; bb--) {}
        if (bb >= (int64_t)sa) {
          b = (uint32_t)bb;
          const RateSegSum sm = sums[b];
          last_t = sm.last_t;
          last_v = sm.last_v;
          prev_t = sm.prev_t;
          prev_v = sm.prev_v;
          rcount = sm.count;
          rreset = sm.reset;
        } else {
          ok = false;
        }
      }
    }
    int64_t count = 0;
    double reset_adj = 0;
    if (ok && a <= b) {
      if (a == b) {
        count = rcount - lcount + 1;
        reset_adj = rreset - lreset;
      } else {
        /* segment-local prefix differences at the two ends, the totals of
         * the segments strictly between one by one, and the reset across
         * every boundary between segments that have points */
        const RateSegSum sm_a = sums[a];
        count = sm_a.count - lcount + 1;
        reset_adj = sm_a.reset - lreset;
        double tail_v = sm_a.last_v;
        int64_t tail_t = sm_a.last_t;
        for (uint32_t k = a + 1; k < b; k++) {
          const RateSegSum sm = sums[k];
          if (sm.count == 0) continue;
          if (sm.first_v < tail_v) reset_adj += tail_v;
          reset_adj += sm.reset;
          count += sm.count;
          tail_v = sm.last_v;
          tail_t = sm.last_t;
        }
        if (sums[b].first_v < tail_v) reset_adj += tail_v;
        reset_adj += rreset;
        count += rcount;
        if (rcount < 2) { /* the point before the last is the previous tail */
          prev_t = tail_t;
          prev_v = tail_v;
        }
      }
    }
    if (count > 0) {
      double v;
      bool have =
          func == 1 ? ratew_finalise_irate(prev_t, prev_v, last_t, last_v, count,
                                           range_ns, is_rate, &v)
                    : ratew_finalise_rate(first_t, first_v, last_t, last_v,
                                          count, reset_adj, ts, range_ns,
                                          is_rate, is_counter, &v);
      if (have) {
        out.value = v;
        out.isnil = 0;
      }
    }
    if (out.isnil) __hip_atomic_fetch_add(&err->gaps, 1ull, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_SYSTEM);
    rows[r] = out;
  }
}

/* ---------------- host ---------------- */

/* Device state of the wide rate queries, separate from RatePlan: a wide
 * call never rebuilds or frees a buffer of the ring path. */
struct RateWidePlan {
  bool valid = false;
  int64_t start = 0, end = 0, range_ns = 0, step_ns = 0;
  RateWideGrid grid = {0, 1, 0};
  std::vector<RateWideSeg> wseg;
  std::vector<RateWideSeries> wser;
  uint64_t edge_records = 0, total_rows = 0;
  RateWideSeg *d_wseg = nullptr;
  RateWideSeries *d_wser = nullptr;
  RateEdgeRec *d_recs = nullptr;
  RateSegSum *d_sums = nullptr;
  gemx_rate_row *d_rows = nullptr;
  uint8_t *d_scratch = nullptr;
  uint32_t gen_lanes = 0;
  DevErr *d_err = nullptr, *h_err = nullptr;
  unsigned long long *d_points = nullptr, *h_points = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  /* last wide query (gemx_prom_wide_stats) */
  uint64_t last_edge_records = 0, last_points = 0;
};

static void free_rate_wide_bufs(RateWidePlan &p) {
  if (p.d_wseg) (void)hipFree(p.d_wseg);
  if (p.d_wser) (void)hipFree(p.d_wser);
  if (p.d_recs) (void)hipFree(p.d_recs);
  if (p.d_sums) (void)hipFree(p.d_sums);
  if (p.d_rows) (void)hipFree(p.d_rows);
  if (p.d_scratch) (void)hipFree(p.d_scratch);
  if (p.d_err) (void)hipFree(p.d_err);
  if (p.h_err) (void)hipHostFree(p.h_err);
  if (p.d_points) (void)hipFree(p.d_points);
  if (p.h_points) (void)hipHostFree(p.h_points);
  for (int e = 0; e < 3; e++)
    if (p.ev[e]) (void)hipEventDestroy(p.ev[e]);
  const uint64_t er = p.last_edge_records, pt = p.last_points;
  p = RateWidePlan();
  p.last_edge_records = er;
  p.last_points = pt;
}

static void free_rate_wide_plan(gemx_shard *s) {
  if (!s->rate_wide_plan) return;
  free_rate_wide_bufs(*s->rate_wide_plan);
  delete s->rate_wide_plan;
  s->rate_wide_plan = nullptr;
}

/* edge runs, output ranges and buffers for one (start, end, range, step) */
static int rate_wide_build_plan(gemx_shard *s, RateWidePlan &P,
                                int64_t start_time, int64_t end_time,
                                int64_t range_ns, int64_t step_ns,
                                const RateWideGrid &g,
                                uint64_t scratch_per_lane) {
  const uint64_t nsegs = s->nsegs;
  free_rate_wide_bufs(P);
  P.grid = g;
  P.wseg.resize(nsegs);
  P.wser.resize(s->series_ranges.size());
  std::vector<int64_t> tmin, tmax;
  for (size_t gi = 0; gi < s->series_ranges.size(); gi++) {
    auto &r = s->series_ranges[gi];
    tmin.resize(r.count);
    tmax.resize(r.count);
    for (uint32_t k = 0; k < r.count; k++) {
      tmin[k] = s->h_descs[r.start + k].min_time;
      tmax[k] = s->h_descs[r.start + k].max_time;
    }
    RateWideSeries &q = P.wser[gi];
    q.sid = r.sid;
    q.seg_start = r.start;
    q.seg_count = r.count;
    q.out_base = P.total_rows;
    q._pad = 0;
    ratew_plan_series(tmin.data(), tmax.data(), r.count, start_time, g,
                      &P.wseg[r.start], &q, &P.edge_records);
    P.total_rows += q.n_steps;
  }
  HIP_CHECK(hipMalloc(&P.d_wseg, sizeof(RateWideSeg) * (nsegs ? nsegs : 1)));
  HIP_CHECK(hipMemcpyAsync(P.d_wseg, P.wseg.data(), sizeof(RateWideSeg) * nsegs,
                           hipMemcpyHostToDevice, s->stream));
  HIP_CHECK(hipMalloc(&P.d_wser, sizeof(RateWideSeries) *
                                     (P.wser.empty() ? 1 : P.wser.size())));
  HIP_CHECK(hipMemcpyAsync(P.d_wser, P.wser.data(),
                           sizeof(RateWideSeries) * P.wser.size(),
                           hipMemcpyHostToDevice, s->stream));
  HIP_CHECK(hipMalloc(&P.d_recs, sizeof(RateEdgeRec) *
                                     (P.edge_records ? P.edge_records : 1)));
  HIP_CHECK(hipMalloc(&P.d_sums, sizeof(RateSegSum) * (nsegs ? nsegs : 1)));
  HIP_CHECK(hipMalloc(&P.d_rows,
                      sizeof(gemx_rate_row) * (P.total_rows ? P.total_rows : 1)));
  HIP_CHECK(hipMalloc(&P.d_err, sizeof(DevErr)));
  HIP_CHECK(hipHostMalloc(&P.h_err, sizeof(DevErr)));
  HIP_CHECK(hipMalloc(&P.d_points, sizeof(unsigned long long)));
  HIP_CHECK(hipHostMalloc(&P.h_points, sizeof(unsigned long long)));
  if (!s->general_ids.empty()) {
    P.gen_lanes = (uint32_t)std::min<uint64_t>(s->general_ids.size(), 16384);
    HIP_CHECK(hipMalloc(&P.d_scratch, scratch_per_lane * P.gen_lanes));
  }
  for (int e = 0; e < 3; e++) HIP_CHECK(hipEventCreate(&P.ev[e]));
  /* the uploads read P.wseg / P.wser, which live as long as the plan */
  P.start = start_time;
  P.end = end_time;
  P.range_ns = range_ns;
  P.step_ns = step_ns;
  P.valid = true;
  return GEMX_OK;
}

static int prom_wide_impl(gemx_shard *s, int64_t start_time, int64_t end_time,
                          int64_t range_ns, int64_t step_ns, int is_rate,
                          int is_counter, int func, gemx_rate_row *out_host,
                          uint64_t cap, uint64_t *n_out,
                          gemx_query_stats *stats) {
  if (!s) {
    seterr("prom_rate_wide: NULL shard handle");
    return GEMX_E_INVALID;
  }
  if (!n_out || (!out_host && cap)) {
    seterr("prom_rate_wide: bad arguments");
    return GEMX_E_INVALID;
  }
  if (s->rpend_count > 0) {
    seterr("async rate queries in flight: call gemx_prom_finish first");
    return GEMX_E_INVALID;
  }
  if (s->col_type != GEMX_TYPE_FLOAT) {
    seterr("prom rate needs a float column");
    return GEMX_E_INVALID;
  }
  if (range_ns <= 0 || step_ns < 0) {
    seterr("invalid range/step");
    return GEMX_E_INVALID;
  }
  RateWideGrid g;
  if (ratew_grid(start_time, end_time, range_ns, step_ns, &g)) {
    seterr("prom_rate_wide: more than 2^31 sample steps");
    return GEMX_E_INVALID;
  }
  HIP_CHECK(hipSetDevice(s->device));
  if (!s->rate_wide_plan) s->rate_wide_plan = new RateWidePlan();
  RateWidePlan &P = *s->rate_wide_plan;
  if (g.n_ord == 0) { /* end < start + range: no sample on the grid */
    P.last_edge_records = 0;
    P.last_points = 0;
    *n_out = 0;
    return GEMX_OK;
  }
  const uint64_t scratch_per_lane = seg_scratch_bytes(SEG_SPARE_PAGE);
  if (!P.valid || P.start != start_time || P.end != end_time ||
      P.range_ns != range_ns || P.step_ns != step_ns) {
    int rc = rate_wide_build_plan(s, P, start_time, end_time, range_ns, step_ns,
                                  g, scratch_per_lane);
    if (rc != GEMX_OK) {
      free_rate_wide_bufs(P);
      return rc;
    }
  }
  if (P.total_rows > cap) {
    seterr("output capacity too small");
    return GEMX_E_CAP;
  }
  HIP_CHECK(hipMemsetAsync(P.d_err, 0, sizeof(DevErr), s->stream));
  HIP_CHECK(hipMemsetAsync(P.d_points, 0, sizeof(unsigned long long), s->stream));
  HIP_CHECK(hipEventRecord(P.ev[0], s->stream));
  const int TPB = 256;
  if (!s->fast_ids.empty()) {
    uint32_t n = (uint32_t)s->fast_ids.size();
    uint32_t blocks = std::min<uint32_t>((n + TPB - 1) / TPB, 65535);
    hipLaunchKernelGGL((k_rate_edges<1>), dim3(blocks), dim3(TPB), 0, s->stream,
                       s->d_blob, s->d_arena, s->d_gor, s->d_descs, P.d_wseg,
                       s->d_fast_ids, n, P.d_recs, P.d_sums, start_time,
                       g.start_sample, g.eff_step, nullptr, 0, 0, P.d_points,
                       P.d_err);
  }
  if (!s->general_ids.empty()) {
    uint32_t n = (uint32_t)s->general_ids.size();
    uint32_t blocks = (P.gen_lanes + TPB - 1) / TPB;
    hipLaunchKernelGGL((k_rate_edges<0>), dim3(blocks), dim3(TPB), 0, s->stream,
                       s->d_blob, s->d_arena, s->d_gor, s->d_descs, P.d_wseg,
                       s->d_general_ids, n, P.d_recs, P.d_sums, start_time,
                       g.start_sample, g.eff_step, P.d_scratch, scratch_per_lane,
                       P.gen_lanes, P.d_points, P.d_err);
  }
  HIP_CHECK(hipEventRecord(P.ev[1], s->stream));
  if (P.total_rows > 0) {
    uint32_t blocks =
        (uint32_t)std::min<uint64_t>((P.total_rows + TPB - 1) / TPB, 65535);
    hipLaunchKernelGGL(k_rate_edge_merge, dim3(blocks), dim3(TPB), 0, s->stream,
                       P.d_wser, (uint32_t)P.wser.size(), P.d_wseg, P.d_recs,
                       P.d_sums, P.d_rows, P.total_rows, g.start_sample,
                       g.eff_step, range_ns, is_rate, is_counter, func, P.d_err);
  }
  HIP_CHECK(hipEventRecord(P.ev[2], s->stream));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(P.h_err, P.d_err, sizeof(DevErr), hipMemcpyDeviceToHost,
                           s->stream));
  HIP_CHECK(hipMemcpyAsync(P.h_points, P.d_points, sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, s->stream));
  if (P.total_rows)
    HIP_CHECK(hipMemcpyAsync(out_host, P.d_rows,
                             sizeof(gemx_rate_row) * P.total_rows,
                             hipMemcpyDeviceToHost, s->stream));
  HIP_CHECK(hipStreamSynchronize(s->stream));
  const DevErr herr = *P.h_err;
  if (herr.code != 0) {
    seterr(herr.code == GEMX_E_UNSUPPORTED ? "unsupported codec on device"
                                           : "segment decode failed on device");
    return herr.code;
  }
  P.last_edge_records = P.edge_records;
  P.last_points = *P.h_points;

  /* only non-nil rows leave, as in the ring path's delivery */
  uint64_t n = 0;
  if (herr.gaps == 0) {
    n = P.total_rows;
  } else {
    uint64_t i = 0;
    while (i < P.total_rows && !out_host[i].isnil) i++;
    n = i;
    for (; i < P.total_rows; i++) {
      if (out_host[i].isnil) continue;
      out_host[n] = out_host[i];
      n++;
    }
  }
  *n_out = n;
  if (stats) {
    float ms_scan = 0, ms_merge = 0, ms_total = 0;
    (void)hipEventElapsedTime(&ms_scan, P.ev[0], P.ev[1]);
    (void)hipEventElapsedTime(&ms_merge, P.ev[1], P.ev[2]);
    (void)hipEventElapsedTime(&ms_total, P.ev[0], P.ev[2]);
    stats->h2d_ms = 0;
    stats->decode_ms = ms_scan;
    stats->merge_ms = ms_merge;
    stats->total_ms = ms_total;
    stats->points = s->total_rows_scanned;
    stats->compressed_bytes = s->total_compressed_bytes;
    stats->n_rows = n;
  }
  return GEMX_OK;
}

extern "C" int gemx_prom_rate_wide(gemx_shard *s, int64_t start_time,
                                   int64_t end_time, int64_t range_ns,
                                   int64_t step_ns, int is_rate, int is_counter,
                                   gemx_rate_row *out_host, uint64_t cap,
                                   uint64_t *n_out, gemx_query_stats *stats) {
  return prom_wide_impl(s, start_time, end_time, range_ns, step_ns, is_rate,
                        is_counter, 0, out_host, cap, n_out, stats);
}

extern "C" int gemx_prom_irate_wide(gemx_shard *s, int64_t start_time,
                                    int64_t end_time, int64_t range_ns,
                                    int64_t step_ns, int is_rate,
                                    gemx_rate_row *out_host, uint64_t cap,
                                    uint64_t *n_out, gemx_query_stats *stats) {
  return prom_wide_impl(s, start_time, end_time, range_ns, step_ns, is_rate, 0,
                        1, out_host, cap, n_out, stats);
}

extern "C" int gemx_prom_wide_stats(gemx_shard *s, uint64_t *edge_records,
                                    uint64_t *points) {
  if (!s) {
    seterr("prom_wide_stats: NULL shard handle");
    return GEMX_E_INVALID;
  }
  const RateWidePlan *P = s->rate_wide_plan;
  if (edge_records) *edge_records = P ? P->last_edge_records : 0;
  if (points) *points = P ? P->last_points : 0;
  return GEMX_OK;
}

#endif /* __HIPCC__ */
