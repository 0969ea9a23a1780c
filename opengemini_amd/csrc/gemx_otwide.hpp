/* The *_over_time family for any range/step ratio: per-cell states.
 *
 * sum/count/avg/min/max/last/stdvar/stddev/present/absent/changes/resets
 * all have an associative combine (the one k_rate_merge folds segment
 * partials with), and an associative operator over a partition of the time
 * axis needs no inverse. Windows are closed, [L_o, R_o] with
 * L_o = start + o*step and R_o = L_o + range, so the axis is cut just before
 * every L_o and just after every R_o:
 *
 *   cell(t) = #{o : L_o <= t} + #{o : R_o < t}              0 .. 2*n_ord
 *   window o = cells [a_o, b_o],  a_o = o + 1 + #{j : R_j < L_o}
 *                                 b_o = o + #{j : L_j <= R_o}
 *
 * Both are monotone, the width b_o - a_o + 1 is W = 2*floor(range/step) + 1
 * for every interior ordinal and smaller only where the grid's ends clamp
 * it. k_ot_cells decodes a segment once and leaves one state per cell it
 * spans; k_ot_blocks folds the segment states of a (series, cell) in
 * descriptor order and computes, per block of B = W cells, the inclusive
 * prefix P and suffix Q (van Herk / Gil-Werman); k_ot_rows answers a window
 * as Q[a_o] (+) P[b_o]. Storage and work follow the number of steps, never
 * the range. Every fold goes left = earlier: the combine is associative but
 * not commutative (last, changes, resets).
 *
 * The first part of this file (geometry, states, planner and the folds
 * over stored states) is plain C++ with no engine state, so it compiles
 * into a stand-alone host program; the kernels and the entry points need
 * hipcc and the engine's decoders. */
#pragma once
#include <cstdint>
#include <vector>

#include "gemx_ratewide.hpp"

#ifdef __HIPCC__
#define OTW_HD __host__ __device__ __forceinline__
#else
#define OTW_HD static inline
#endif

/* ---------------- geometry (host and device) ---------------- */

/* cell(t) in closed form, the sum of ratew_left_le and ratew_right_lt, and
 * the first time at or after which the cell differs (INT64_MAX: never). The
 * two divisions are why the scan calls this only at a cell change. */
OTW_HD int64_t otw_cell_next(int64_t t, int64_t start_time,
                             int64_t start_sample, int64_t step, int64_t n_ord,
                             int64_t *next_cut) {
  int64_t nl = 0, nr = 0;
  if (t >= start_time) {
    const uint64_t k = ((uint64_t)t - (uint64_t)start_time) / (uint64_t)step;
    nl = k >= (uint64_t)n_ord ? n_ord : (int64_t)k + 1;
  }
  if (t > start_sample) {
    const uint64_t k =
        ((uint64_t)t - (uint64_t)start_sample - 1) / (uint64_t)step;
    nr = k >= (uint64_t)n_ord ? n_ord : (int64_t)k + 1;
  }
  /* the next left cut is L_nl itself, the next right cut lies one past R_nr */
  int64_t cut = INT64_MAX;
  if (nl < n_ord) cut = start_time + nl * step;
  if (nr < n_ord) {
    const int64_t rc = start_sample + nr * step + 1;
    if (rc < cut) cut = rc;
  }
  *next_cut = cut;
  return nl + nr;
}

OTW_HD int64_t otw_cell(int64_t t, int64_t start_time, int64_t start_sample,
                        int64_t step, int64_t n_ord) {
  int64_t cut;
  return otw_cell_next(t, start_time, start_sample, step, n_ord, &cut);
}

/* floor(range/step), clamped to n_ord: beyond that every count below clamps
 * anyway, and the sums stay far from overflow */
OTW_HD int64_t otw_ratio(int64_t range_ns, int64_t step, int64_t n_ord) {
  const int64_t k = range_ns / step;
  return k > n_ord ? n_ord : k;
}

/* cells of window o: R_j < L_o <=> j < o - range/step, L_j <= R_o <=>
 * j <= o + range/step, both counted over j in [0, n_ord) */
OTW_HD void otw_row_cells(int64_t o, int64_t k, int64_t n_ord, int64_t *a,
                          int64_t *b) {
  const int64_t below = o > k ? o - k : 0;
  const int64_t upto = o + k + 1 < n_ord ? o + k + 1 : n_ord;
  *a = o + 1 + below;
  *b = o + upto;
}

/* block length: W, or the whole cell axis where that is shorter */
OTW_HD int64_t otw_block_len(int64_t k, int64_t n_ord) {
  const int64_t w = 2 * k + 1, all = 2 * n_ord + 1;
  return w < all ? w : all;
}

enum { OTW_JOIN = 0, OTW_PREFIX = 1, OTW_SUFFIX = 2, OTW_FOLD = 3 };

/* how window [a, b] is answered from the stored states; blocks are aligned
 * to cell 0. A full-width window is a join or a whole block; only windows
 * narrower than the block (clamped end rows, range < step) can fall inside
 * a block and fold their cells directly. */
OTW_HD int otw_row_kind(int64_t a, int64_t b, int64_t blk) {
  const int64_t ba = a / blk, bb = b / blk;
  if (bb == ba + 1) return OTW_JOIN;
  if (bb != ba) return OTW_FOLD;
  if (a == ba * blk) return OTW_PREFIX;
  if (b == ba * blk + blk - 1) return OTW_SUFFIX;
  return OTW_FOLD;
}

/* ---------------- states and their combine (host and device) ------------ */

/* state classes: one scan / fold instantiation each */
enum {
  OTW_C_SUM = 0,
  OTW_C_AVG = 1,
  OTW_C_MINMAX = 2,
  OTW_C_LAST = 3, /* last, count, present, absent */
  OTW_C_STDVAR = 4,
  OTW_C_CHG = 5, /* changes, resets */
  OTW_C_NONE = -1
};

/* the GEMX_PF_* codes this path takes (gemx_engine.hip) */
enum {
  OTW_F_SUM = 2, OTW_F_COUNT = 3, OTW_F_AVG = 4, OTW_F_MIN = 5, OTW_F_MAX = 6,
  OTW_F_LAST = 7, OTW_F_STDVAR = 8, OTW_F_STDDEV = 9, OTW_F_PRESENT = 10,
  OTW_F_CHANGES = 11, OTW_F_RESETS = 12, OTW_F_ABSENT = 15
};

OTW_HD int otw_class_of(int func) {
  switch (func) {
  case OTW_F_SUM: return OTW_C_SUM;
  case OTW_F_AVG: return OTW_C_AVG;
  case OTW_F_MIN:
  case OTW_F_MAX: return OTW_C_MINMAX;
  case OTW_F_COUNT:
  case OTW_F_LAST:
  case OTW_F_PRESENT:
  case OTW_F_ABSENT: return OTW_C_LAST;
  case OTW_F_STDVAR:
  case OTW_F_STDDEV: return OTW_C_STDVAR;
  case OTW_F_CHANGES:
  case OTW_F_RESETS: return OTW_C_CHG;
  default: return OTW_C_NONE;
  }
}

/* Stored state of a cell, a prefix or a suffix: 32 bytes, tails applied.
 *   sum      a = sum + c            avg     a = mean + c
 *   min/max  a = extreme            last    a = last value
 *   stdvar   a = mean, b = M2       changes a = counter, b = first value,
 *                                           c = last value
 * count == 0 is the identity. */
struct alignas(16) OtState {
  int64_t count;
  double a, b, c;
};

/* States move between memory and registers field by field: a whole-struct
 * copy goes through a private stack slot in some instantiations. */
OTW_HD OtState otw_load(const OtState *p) {
  OtState s;
  s.count = p->count;
  s.a = p->a;
  s.b = p->b;
  s.c = p->c;
  return s;
}

OTW_HD void otw_store(OtState *p, const OtState &s) {
  p->count = s.count;
  p->a = s.a;
  p->b = s.b;
  p->c = s.c;
}

/* Running state of the cell a lane is in: the sequential state of the
 * reference, compensation terms apart (r1, r3). */
struct OtRun {
  int64_t count;
  double r0, r1, r2, r3;
};

OTW_HD void otw_kahan_inc(double inc, double &sum, double &c) {
  /* executor.KahanSumInc */
  double t = sum + inc;
  if (__builtin_fabs(sum) >= __builtin_fabs(inc))
    c += (sum - t) + inc;
  else
    c += (inc - t) + sum;
  sum = t;
}

OTW_HD void otw_run_reset(OtRun &p) {
  p.count = 0;
  p.r0 = p.r1 = p.r2 = p.r3 = 0;
}

/* one point into the running state: the per-point body of ot_slot_update */
template <int CLS>
OTW_HD void otw_update(OtRun &p, double v, int func) {
  if (CLS == OTW_C_SUM) {
    otw_kahan_inc(v, p.r0, p.r1); /* floatPromSumReduce Kahan */
  } else if (CLS == OTW_C_AVG) {
    /* floatAvgReduce: streaming Kahan mean with Inf carve-outs */
    double count = (double)(p.count + 1);
    double mean = p.r0;
    bool skip = false;
    if (__builtin_isinf(mean)) {
      if (__builtin_isinf(v) && (mean > 0) == (v > 0)) skip = true;
      else if (!__builtin_isinf(v) && !__builtin_isnan(v)) skip = true;
    }
    if (!skip) otw_kahan_inc(v / count - mean / count, p.r0, p.r1);
  } else if (CLS == OTW_C_MINMAX) {
    if (func == OTW_F_MIN) {
      if (p.count == 0 || v < p.r0 || __builtin_isnan(p.r0)) p.r0 = v;
    } else {
      if (p.count == 0 || v > p.r0 || __builtin_isnan(p.r0)) p.r0 = v;
    }
  } else if (CLS == OTW_C_LAST) {
    p.r0 = v;
  } else if (CLS == OTW_C_STDVAR) {
    /* sequential Kahan-Welford as floatStdVarOverTimeMerger: mean in
     * (r0, r1), M2 in (r2, r3); the product must not fuse into the add */
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double c = (double)(p.count + 1);
    double delta = v - (p.r0 + p.r1);
    otw_kahan_inc(delta / c, p.r0, p.r1);
    double inc = delta * (v - (p.r0 + p.r1));
    otw_kahan_inc(inc, p.r2, p.r3);
  } else if (CLS == OTW_C_CHG) {
    /* executor.CalcChange / CalcResets streamed: counter r0, first value
     * r1, last value r2 */
    if (p.count == 0) {
      p.r1 = v;
    } else {
      bool hit = (func == OTW_F_CHANGES)
                     ? (v != p.r2 && !(__builtin_isnan(v) && __builtin_isnan(p.r2)))
                     : (v < p.r2);
      if (hit) p.r0 += 1.0;
    }
    p.r2 = v;
  }
  p.count++;
}

/* the running state as a stored one: tails applied, as the reduce returns
 * sum + c / mean + c before any merge */
template <int CLS>
OTW_HD OtState otw_flush(const OtRun &p) {
  OtState s;
  s.count = p.count;
  s.a = p.r0;
  s.b = 0;
  s.c = 0;
  if (CLS == OTW_C_SUM || CLS == OTW_C_AVG) {
    if (!__builtin_isinf(p.r0)) s.a = p.r0 + p.r1;
  } else if (CLS == OTW_C_STDVAR) {
    s.a = p.r0 + p.r1;
    s.b = p.r2 + p.r3;
  } else if (CLS == OTW_C_CHG) {
    s.b = p.r1;
    s.c = p.r2;
  }
  return s;
}

OTW_HD OtState otw_identity() {
  OtState s;
  s.count = 0;
  s.a = s.b = s.c = 0;
  return s;
}

/* l (+) r, l the earlier: the combine of k_rate_merge on stored states */
template <int CLS>
OTW_HD OtState otw_combine(const OtState &l, const OtState &r, int func) {
  /* the identity on either side is picked field by field at the end, so
   * that no state has its address taken */
  OtState s;
  s.count = l.count + r.count;
  s.a = l.a;
  s.b = l.b;
  s.c = l.c;
  if (CLS == OTW_C_SUM) {
    s.a = l.a + r.a;
  } else if (CLS == OTW_C_AVG) {
    double pc = (double)l.count, cc = (double)r.count;
    s.a = (l.a * pc + r.a * cc) / (pc + cc);
  } else if (CLS == OTW_C_MINMAX) {
    if (func == OTW_F_MIN) {
      if (__builtin_isnan(l.a) || (!__builtin_isnan(r.a) && r.a < l.a)) s.a = r.a;
    } else {
      if (__builtin_isnan(l.a) || (!__builtin_isnan(r.a) && r.a > l.a)) s.a = r.a;
    }
  } else if (CLS == OTW_C_LAST) {
    s.a = r.a;
  } else if (CLS == OTW_C_STDVAR) {
    /* Chan's parallel formula */
    double na = (double)l.count, nb = (double)r.count;
    double n = na + nb;
    double d2 = r.a - l.a;
    s.b = l.b + (r.b + d2 * d2 * na * nb / n);
    s.a = l.a + d2 * nb / n;
  } else if (CLS == OTW_C_CHG) {
    /* the boundary pair (l's last, r's first) counts by the same rule,
     * then r's own counter adds on */
    bool hit = (func == OTW_F_CHANGES)
                   ? (r.b != l.c && !(__builtin_isnan(l.c) && __builtin_isnan(r.b)))
                   : (r.b < l.c);
    s.a = l.a + (r.a + (hit ? 1.0 : 0.0));
    s.b = l.b;
    s.c = r.c;
  }
  if (l.count == 0) {
    s.a = r.a;
    s.b = r.b;
    s.c = r.c;
  } else if (r.count == 0) {
    s.a = l.a;
    s.b = l.b;
    s.c = l.c;
  }
  return s;
}

/* the row value of a folded window; false for a nil row */
OTW_HD bool otw_finalise(const OtState &s, int func, double *value) {
  if (func == OTW_F_ABSENT) { /* inverse emit: 1 for windows with no samples */
    *value = 1.0;
    return s.count == 0;
  }
  if (s.count == 0) return false;
  switch (func) {
  case OTW_F_COUNT: *value = (double)s.count; break;
  case OTW_F_PRESENT: *value = 1.0; break;
  case OTW_F_STDVAR: *value = s.b / (double)s.count; break;
  case OTW_F_STDDEV: *value = __builtin_sqrt(s.b / (double)s.count); break;
  default: *value = s.a; break;
  }
  return true;
}

/* ---------------- host planner (descriptors only) ---------------- */

struct OtWideSeg {
  uint64_t slot_base; /* ncells states, one per cell from c0 on */
  int64_t c0;         /* cell(min_time) */
  uint32_t ncells;    /* cell(max_time) - c0 + 1 */
  uint32_t _pad;
};

struct OtWideSeries {
  uint64_t sid;
  int64_t s_min;       /* first ordinal with a row */
  uint64_t out_base;   /* dense output row of s_min */
  uint64_t state_base; /* ncell series states from cmin on (C, P and Q) */
  uint64_t blk_base;   /* first (series, block) work item */
  int64_t cmin;        /* cells [cmin, cmin + ncell) can hold data */
  uint32_t ncell;
  uint32_t n_steps;
  uint32_t seg_start, seg_count;
};

/* One series: segments [0, n) in descriptor order with their min_time /
 * max_time. Fills seg[0..n) and the geometry of *ser (sid, seg_start,
 * seg_count and out_base are the caller's); the bases start at *slots,
 * *states and *blocks, which advance by what the series takes. A segment's
 * cell range comes from its own bounds only, so segments that overlap in
 * time stay in bounds without a running maximum. */
static inline void otw_plan_series(const int64_t *min_time,
                                   const int64_t *max_time, uint32_t n,
                                   int64_t start_time, int64_t range_ns,
                                   const RateWideGrid &g, OtWideSeg *seg,
                                   OtWideSeries *ser, uint64_t *slots,
                                   uint64_t *states, uint64_t *blocks) {
  int64_t tmin = min_time[0], tmax = max_time[0];
  int64_t cmin = INT64_MAX, cmax = INT64_MIN;
  for (uint32_t k = 0; k < n; k++) {
    if (min_time[k] < tmin) tmin = min_time[k];
    if (max_time[k] > tmax) tmax = max_time[k];
    const int64_t c0 =
        ratew_left_le(min_time[k], start_time, g) + ratew_right_lt(min_time[k], g);
    int64_t c1 =
        ratew_left_le(max_time[k], start_time, g) + ratew_right_lt(max_time[k], g);
    if (c1 < c0) c1 = c0; /* bounds out of order: one cell, still in bounds */
    seg[k].c0 = c0;
    seg[k].ncells = (uint32_t)(c1 - c0 + 1);
    seg[k]._pad = 0;
    seg[k].slot_base = *slots;
    *slots += seg[k].ncells;
    if (c0 < cmin) cmin = c0;
    if (c1 > cmax) cmax = c1;
  }
  ser->cmin = cmin;
  ser->ncell = (uint32_t)(cmax - cmin + 1);
  ser->state_base = *states;
  *states += ser->ncell;
  const int64_t blk = otw_block_len(otw_ratio(range_ns, g.eff_step, g.n_ord), g.n_ord);
  ser->blk_base = *blocks;
  *blocks += (uint64_t)(cmax / blk - cmin / blk + 1);
  /* rows: right edge at or after the first point, left edge at or before
   * the last one (the rows of the ring path and of the edge-record path) */
  const int64_t s_lo = ratew_right_lt(tmin, g);
  int64_t s_hi = ratew_left_le(tmax, start_time, g);
  if (s_hi < s_lo) s_hi = s_lo;
  ser->s_min = s_lo;
  ser->n_steps = (uint32_t)(s_hi - s_lo);
}

/* ---------------- folds over the stored states (host and device) -------- */

/* Block b of series s (blocks are aligned to cell 0 and clipped to the
 * cells the series has data in): the segment states of each cell folded in
 * descriptor order into C, then the inclusive prefix P (left to right) and
 * suffix Q (right to left). C, P and Q are indexed by state_base + cell -
 * cmin. */
template <int CLS>
OTW_HD void otw_fold_block(const OtWideSeries &s, const OtWideSeg *wseg,
                           const OtState *slots, OtState *C, OtState *P,
                           OtState *Q, int64_t b, int64_t blk, int func) {
  const int64_t cmax = s.cmin + (int64_t)s.ncell - 1;
  int64_t c_lo = b * blk, c_hi = b * blk + blk - 1;
  if (c_lo < s.cmin) c_lo = s.cmin;
  if (c_hi > cmax) c_hi = cmax;
  if (c_hi < c_lo) return;
  const uint64_t off = s.state_base - (uint64_t)s.cmin; /* wraps back below */
  for (int64_t c = c_lo; c <= c_hi; c++)
    otw_store(&C[off + (uint64_t)c], otw_identity());
  for (uint32_t k = s.seg_start; k < s.seg_start + s.seg_count; k++) {
    const OtWideSeg q = wseg[k];
    int64_t x0 = q.c0, x1 = q.c0 + (int64_t)q.ncells - 1;
    if (x0 < c_lo) x0 = c_lo;
    if (x1 > c_hi) x1 = c_hi;
    for (int64_t c = x0; c <= x1; c++) {
      const OtState st = otw_load(&slots[q.slot_base + (uint64_t)(c - q.c0)]);
      if (st.count == 0) continue;
      otw_store(&C[off + (uint64_t)c],
                otw_combine<CLS>(otw_load(&C[off + (uint64_t)c]), st, func));
    }
  }
  OtState acc = otw_identity();
  for (int64_t c = c_lo; c <= c_hi; c++) {
    acc = otw_combine<CLS>(acc, otw_load(&C[off + (uint64_t)c]), func);
    otw_store(&P[off + (uint64_t)c], acc);
  }
  acc = otw_identity();
  for (int64_t c = c_hi; c >= c_lo; c--) {
    acc = otw_combine<CLS>(otw_load(&C[off + (uint64_t)c]), acc, func);
    otw_store(&Q[off + (uint64_t)c], acc);
  }
}

/* The state of window [a, b] of series s, and how it was answered. Cells
 * outside [cmin, cmin + ncell) hold the identity and have no storage. */
template <int CLS>
OTW_HD OtState otw_row_state(const OtWideSeries &s, const OtState *C,
                             const OtState *P, const OtState *Q, int64_t a,
                             int64_t b, int64_t blk, int func, int *kind_out) {
  const int64_t cmax = s.cmin + (int64_t)s.ncell - 1;
  const uint64_t off = s.state_base - (uint64_t)s.cmin;
  const int kind = otw_row_kind(a, b, blk);
  *kind_out = kind;
  const int64_t ac = a < s.cmin ? s.cmin : a;
  const int64_t bc = b > cmax ? cmax : b;
  OtState acc = otw_identity();
  if (ac > bc) return acc;
  if (kind == OTW_FOLD) {
    for (int64_t c = ac; c <= bc; c++)
      acc = otw_combine<CLS>(acc, otw_load(&C[off + (uint64_t)c]), func);
    return acc;
  }
  /* Q[ac] is the fold of [a, end of a's block], P[bc] that of [start of
   * b's block, b], where the clipped cell is still in that block */
  const int64_t a_end = a / blk * blk + blk - 1;
  const int64_t b_start = b / blk * blk;
  if (kind != OTW_PREFIX && ac <= a_end) acc = otw_load(&Q[off + (uint64_t)ac]);
  if (kind != OTW_SUFFIX && bc >= b_start)
    acc = otw_combine<CLS>(acc, otw_load(&P[off + (uint64_t)bc]), func);
  return acc;
}

#ifdef __HIPCC__

/* ---------------- device ---------------- */

/* One lane per segment: decode it once, keep one running state for the cell
 * the stream is in, and at every cell change store it to the lane's own slot
 * c - c0 (identity states into the cells skipped). No ring, no indexed
 * private array, no atomics on the states. */
template <int FAST, int CLS>
__global__ void __launch_bounds__(256) k_ot_cells(
    const uint8_t *__restrict__ blob, const uint64_t *__restrict__ arena,
    const GorDesc *__restrict__ gors, const gemx_seg_desc *__restrict__ descs,
    const OtWideSeg *__restrict__ wseg, const uint32_t *__restrict__ seg_ids,
    uint32_t nseg_ids, OtState *__restrict__ slots, int64_t start_time,
    int64_t start_sample, int64_t step_ns, int64_t n_ord, int func,
    uint8_t *__restrict__ scratch, uint64_t scratch_per_lane, uint32_t nlanes,
    unsigned long long *__restrict__ points, DevErr *err) {
  uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t stride = FAST ? gridDim.x * blockDim.x : nlanes;
  if (!FAST && gid >= nlanes) return;

  for (uint32_t li = gid; li < nseg_ids; li += stride) {
    uint32_t si = seg_ids[li];
    const gemx_seg_desc d = descs[si];
    const OtWideSeg wq = wseg[si];
    int rows = (int)d.rows;
    OtState *my_slots = slots + wq.slot_base;

    /* fast: streaming reader; general: buffered into per-lane scratch
     * (gemx_segdecode.hpp) */
    SegStream<GEMX_TYPE_FLOAT> st;
    SegBuffered<GEMX_TYPE_FLOAT> sb;
    if (int rc = FAST ? st.open(blob, arena, gors, si, d)
                      : sb.decode(blob, d, scratch + (uint64_t)gid * scratch_per_lane)) {
      set_err(err, rc);
      return;
    }

    /* the cell the stream is in (relative to c0; -1 before the first
     * usable point), its running state, and the time of the next cut */
    OtRun run;
    otw_run_reset(run);
    int64_t cur = -1;
    int64_t next_cut = INT64_MIN;
    const int64_t last_cell = (int64_t)wq.ncells - 1;
    int64_t cnt = 0;

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

      if (t >= next_cut) {
        /* a cut lies between the previous point and this one. The cell is
         * clamped to this lane's slots and never steps back, whatever the
         * times are, so every store below stays inside [0, ncells). */
        int64_t c = otw_cell_next(t, start_time, start_sample, step_ns, n_ord,
                                  &next_cut) - wq.c0;
        if (c > last_cell) c = last_cell;
        if (c < 0) c = 0;
        if (c > cur) {
          if (cur >= 0) otw_store(&my_slots[cur], otw_flush<CLS>(run));
          for (int64_t z = cur + 1; z < c; z++) otw_store(&my_slots[z], otw_identity());
          otw_run_reset(run);
          cur = c;
        }
      }
      otw_update<CLS>(run, fv, func);
      cnt++;
    }
    if (cur >= 0) otw_store(&my_slots[cur], otw_flush<CLS>(run));
    for (int64_t z = cur + 1; z <= last_cell; z++)
      otw_store(&my_slots[z], otw_identity());
    if (cnt) atomicAdd(points, (unsigned long long)cnt);
  }
}

/* One thread per (series, block): the segment states of each cell of the
 * block folded in descriptor order into C, then the inclusive prefix P
 * (left to right) and suffix Q (right to left) within the block. Blocks are
 * aligned to cell 0 and clipped to the cells the series has data in. */
template <int CLS>
__global__ void __launch_bounds__(256) k_ot_blocks(
    const OtWideSeries *__restrict__ series, uint32_t nseries,
    const OtWideSeg *__restrict__ wseg, const OtState *__restrict__ slots,
    OtState *__restrict__ cst, OtState *__restrict__ pst,
    OtState *__restrict__ qst, uint64_t total_blocks, int64_t blk, int func) {
  uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  for (uint64_t w = gid; w < total_blocks; w += gridDim.x * (uint64_t)blockDim.x) {
    uint32_t lo = 0, hi = nseries - 1;
    while (lo < hi) {
      uint32_t mid = (lo + hi + 1) >> 1;
      if (series[mid].blk_base <= w) lo = mid;
      else hi = mid - 1;
    }
    const OtWideSeries s = series[lo];
    otw_fold_block<CLS>(s, wseg, slots, cst, pst, qst,
                        s.cmin / blk + (int64_t)(w - s.blk_base), blk, func);
  }
}

/* One thread per (series, step) row. whole_grid: every series has a row at
 * every ordinal (absent), otherwise the rows of the plan. */
template <int CLS>
__global__ void __launch_bounds__(256) k_ot_rows(
    const OtWideSeries *__restrict__ series, uint32_t nseries,
    const OtState *__restrict__ cst, const OtState *__restrict__ pst,
    const OtState *__restrict__ qst, gemx_rate_row *__restrict__ rows,
    uint64_t total_rows, int64_t start_sample, int64_t step_ns, int64_t n_ord,
    int64_t ratio, int64_t blk, int func, int whole_grid,
    unsigned long long *__restrict__ kinds, DevErr *__restrict__ err) {
  __shared__ unsigned int sh_kind[2];
  if (threadIdx.x < 2) sh_kind[threadIdx.x] = 0;
  __syncthreads();
  unsigned int n_join = 0, n_fold = 0;
  uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  for (uint64_t r = gid; r < total_rows; r += gridDim.x * (uint64_t)blockDim.x) {
    uint32_t lo;
    int64_t o;
    if (whole_grid) {
      lo = (uint32_t)(r / (uint64_t)n_ord);
      o = (int64_t)(r % (uint64_t)n_ord);
    } else {
      uint32_t hi = nseries - 1;
      lo = 0;
      while (lo < hi) {
        uint32_t mid = (lo + hi + 1) >> 1;
        if (series[mid].out_base <= r) lo = mid;
        else hi = mid - 1;
      }
      o = series[lo].s_min + (int64_t)(r - series[lo].out_base);
    }
    const OtWideSeries s = series[lo];
    int64_t a, b;
    otw_row_cells(o, ratio, n_ord, &a, &b);
    int kind;
    const OtState acc =
        otw_row_state<CLS>(s, cst, pst, qst, a, b, blk, func, &kind);
    if (kind == OTW_FOLD) n_fold++;
    else n_join++;

    gemx_rate_row out;
    out.sid = s.sid;
    out.ts = start_sample + o * step_ns;
    out.value = 0;
    out.isnil = 1;
    memset(out._pad, 0, sizeof(out._pad));
    double v;
    if (otw_finalise(acc, func, &v)) {
      out.value = v;
      out.isnil = 0;
    }
    if (out.isnil) __hip_atomic_fetch_add(&err->gaps, 1ull, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_SYSTEM);
    rows[r] = out;
  }
  if (n_join) atomicAdd(&sh_kind[0], n_join);
  if (n_fold) atomicAdd(&sh_kind[1], n_fold);
  __syncthreads();
  if (threadIdx.x < 2 && sh_kind[threadIdx.x])
    atomicAdd(&kinds[threadIdx.x], (unsigned long long)sh_kind[threadIdx.x]);
}

/* ---------------- host ---------------- */

/* Device state of the wide over_time queries, separate from RatePlan and
 * RateWidePlan. Geometry and buffers are shared by all functions; the
 * states are recomputed per call. */
struct OtWidePlan {
  bool valid = false;
  int64_t start = 0, end = 0, range_ns = 0, step_ns = 0;
  RateWideGrid grid = {0, 1, 0};
  int64_t ratio = 0, blk = 1;
  std::vector<OtWideSeg> wseg;
  std::vector<OtWideSeries> wser;
  uint64_t cell_slots = 0, series_states = 0, total_blocks = 0, total_rows = 0;
  uint64_t rows_cap = 0; /* rows d_rows holds: grows for absent's whole grid */
  OtWideSeg *d_wseg = nullptr;
  OtWideSeries *d_wser = nullptr;
  OtState *d_slots = nullptr;
  OtState *d_cpq = nullptr; /* C, P and Q, series_states each */
  gemx_rate_row *d_rows = nullptr;
  uint8_t *d_scratch = nullptr;
  uint32_t gen_lanes = 0;
  DevErr *d_err = nullptr, *h_err = nullptr;
  unsigned long long *d_cnt = nullptr, *h_cnt = nullptr; /* points, joined, folded */
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  /* last wide over_time query (gemx_prom_wide_ot_stats) */
  uint64_t last[4] = {0, 0, 0, 0};
};

static void free_ot_wide_bufs(OtWidePlan &p) {
  if (p.d_wseg) (void)hipFree(p.d_wseg);
  if (p.d_wser) (void)hipFree(p.d_wser);
  if (p.d_slots) (void)hipFree(p.d_slots);
  if (p.d_cpq) (void)hipFree(p.d_cpq);
  if (p.d_rows) (void)hipFree(p.d_rows);
  if (p.d_scratch) (void)hipFree(p.d_scratch);
  if (p.d_err) (void)hipFree(p.d_err);
  if (p.h_err) (void)hipHostFree(p.h_err);
  if (p.d_cnt) (void)hipFree(p.d_cnt);
  if (p.h_cnt) (void)hipHostFree(p.h_cnt);
  for (int e = 0; e < 3; e++)
    if (p.ev[e]) (void)hipEventDestroy(p.ev[e]);
  uint64_t keep[4];
  for (int i = 0; i < 4; i++) keep[i] = p.last[i];
  p = OtWidePlan();
  for (int i = 0; i < 4; i++) p.last[i] = keep[i];
}

static void free_ot_wide_plan(gemx_shard *s) {
  if (!s->ot_wide_plan) return;
  free_ot_wide_bufs(*s->ot_wide_plan);
  delete s->ot_wide_plan;
  s->ot_wide_plan = nullptr;
}

/* cell ranges, state bases, output ranges and buffers for one
 * (start, end, range, step) */
static int ot_wide_build_plan(gemx_shard *s, OtWidePlan &P, int64_t start_time,
                              int64_t end_time, int64_t range_ns,
                              int64_t step_ns, const RateWideGrid &g,
                              uint64_t scratch_per_lane) {
  const uint64_t nsegs = s->nsegs;
  free_ot_wide_bufs(P);
  P.grid = g;
  P.ratio = otw_ratio(range_ns, g.eff_step, g.n_ord);
  P.blk = otw_block_len(P.ratio, g.n_ord);
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
    OtWideSeries &q = P.wser[gi];
    q.sid = r.sid;
    q.seg_start = r.start;
    q.seg_count = r.count;
    q.out_base = P.total_rows;
    otw_plan_series(tmin.data(), tmax.data(), r.count, start_time, range_ns, g,
                    &P.wseg[r.start], &q, &P.cell_slots, &P.series_states,
                    &P.total_blocks);
    P.total_rows += q.n_steps;
  }
  HIP_CHECK(hipMalloc(&P.d_wseg, sizeof(OtWideSeg) * (nsegs ? nsegs : 1)));
  HIP_CHECK(hipMemcpyAsync(P.d_wseg, P.wseg.data(), sizeof(OtWideSeg) * nsegs,
                           hipMemcpyHostToDevice, s->stream));
  HIP_CHECK(hipMalloc(&P.d_wser, sizeof(OtWideSeries) *
                                     (P.wser.empty() ? 1 : P.wser.size())));
  HIP_CHECK(hipMemcpyAsync(P.d_wser, P.wser.data(),
                           sizeof(OtWideSeries) * P.wser.size(),
                           hipMemcpyHostToDevice, s->stream));
  HIP_CHECK(hipMalloc(&P.d_slots,
                      sizeof(OtState) * (P.cell_slots ? P.cell_slots : 1)));
  HIP_CHECK(hipMalloc(&P.d_cpq, sizeof(OtState) * 3 *
                                    (P.series_states ? P.series_states : 1)));
  P.rows_cap = P.total_rows ? P.total_rows : 1;
  HIP_CHECK(hipMalloc(&P.d_rows, sizeof(gemx_rate_row) * P.rows_cap));
  HIP_CHECK(hipMalloc(&P.d_err, sizeof(DevErr)));
  HIP_CHECK(hipHostMalloc(&P.h_err, sizeof(DevErr)));
  HIP_CHECK(hipMalloc(&P.d_cnt, sizeof(unsigned long long) * 3));
  HIP_CHECK(hipHostMalloc(&P.h_cnt, sizeof(unsigned long long) * 3));
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

template <int CLS>
static void ot_wide_launch(gemx_shard *s, OtWidePlan &P, int64_t start_time,
                           int func, int whole_grid, uint64_t total_rows,
                           uint64_t scratch_per_lane) {
  const int TPB = 256;
  const RateWideGrid &g = P.grid;
  if (!s->fast_ids.empty()) {
    uint32_t n = (uint32_t)s->fast_ids.size();
    uint32_t blocks = std::min<uint32_t>((n + TPB - 1) / TPB, 65535);
    hipLaunchKernelGGL((k_ot_cells<1, CLS>), dim3(blocks), dim3(TPB), 0,
                       s->stream, s->d_blob, s->d_arena, s->d_gor, s->d_descs,
                       P.d_wseg, s->d_fast_ids, n, P.d_slots, start_time,
                       g.start_sample, g.eff_step, g.n_ord, func, nullptr, 0, 0,
                       P.d_cnt, P.d_err);
  }
  if (!s->general_ids.empty()) {
    uint32_t n = (uint32_t)s->general_ids.size();
    uint32_t blocks = (P.gen_lanes + TPB - 1) / TPB;
    hipLaunchKernelGGL((k_ot_cells<0, CLS>), dim3(blocks), dim3(TPB), 0,
                       s->stream, s->d_blob, s->d_arena, s->d_gor, s->d_descs,
                       P.d_wseg, s->d_general_ids, n, P.d_slots, start_time,
                       g.start_sample, g.eff_step, g.n_ord, func, P.d_scratch,
                       scratch_per_lane, P.gen_lanes, P.d_cnt, P.d_err);
  }
  (void)hipEventRecord(P.ev[1], s->stream);
  OtState *C = P.d_cpq;
  OtState *Pp = C + P.series_states, *Q = Pp + P.series_states;
  if (P.total_blocks > 0) {
    uint32_t blocks =
        (uint32_t)std::min<uint64_t>((P.total_blocks + TPB - 1) / TPB, 65535);
    hipLaunchKernelGGL((k_ot_blocks<CLS>), dim3(blocks), dim3(TPB), 0, s->stream,
                       P.d_wser, (uint32_t)P.wser.size(), P.d_wseg, P.d_slots, C,
                       Pp, Q, P.total_blocks, P.blk, func);
  }
  if (total_rows > 0) {
    uint32_t blocks =
        (uint32_t)std::min<uint64_t>((total_rows + TPB - 1) / TPB, 65535);
    hipLaunchKernelGGL((k_ot_rows<CLS>), dim3(blocks), dim3(TPB), 0, s->stream,
                       P.d_wser, (uint32_t)P.wser.size(), C, Pp, Q, P.d_rows,
                       total_rows, g.start_sample, g.eff_step, g.n_ord, P.ratio,
                       P.blk, func, whole_grid, P.d_cnt + 1, P.d_err);
  }
}

extern "C" int gemx_prom_over_time_wide(gemx_shard *s, int64_t start_time,
                                        int64_t end_time, int64_t range_ns,
                                        int64_t step_ns, int func,
                                        gemx_rate_row *out_host, uint64_t cap,
                                        uint64_t *n_out,
                                        gemx_query_stats *stats) {
  if (!s) {
    seterr("prom_over_time_wide: NULL shard handle");
    return GEMX_E_INVALID;
  }
  if (!n_out || (!out_host && cap)) {
    seterr("prom_over_time_wide: bad arguments");
    return GEMX_E_INVALID;
  }
  const int cls = otw_class_of(func);
  if (cls == OTW_C_NONE) {
    seterr("prom_over_time_wide: func has no per-cell state (takes sum, count, "
           "avg, min, max, last, stdvar, stddev, present, changes, resets, "
           "absent)");
    return GEMX_E_INVALID;
  }
  if (s->rpend_count > 0) {
    seterr("async rate queries in flight: call gemx_prom_finish first");
    return GEMX_E_INVALID;
  }
  if (s->col_type != GEMX_TYPE_FLOAT) {
    seterr("prom over_time needs a float column");
    return GEMX_E_INVALID;
  }
  if (range_ns <= 0 || step_ns < 0) {
    seterr("invalid range/step");
    return GEMX_E_INVALID;
  }
  RateWideGrid g;
  if (ratew_grid(start_time, end_time, range_ns, step_ns, &g)) {
    seterr("prom_over_time_wide: more than 2^31 sample steps");
    return GEMX_E_INVALID;
  }
  HIP_CHECK(hipSetDevice(s->device));
  if (!s->ot_wide_plan) s->ot_wide_plan = new OtWidePlan();
  OtWidePlan &P = *s->ot_wide_plan;
  if (g.n_ord == 0) { /* end < start + range: no sample on the grid */
    for (int i = 0; i < 4; i++) P.last[i] = 0;
    *n_out = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    return GEMX_OK;
  }
  const uint64_t scratch_per_lane = seg_scratch_bytes(SEG_SPARE_PAGE);
  if (!P.valid || P.start != start_time || P.end != end_time ||
      P.range_ns != range_ns || P.step_ns != step_ns) {
    int rc = ot_wide_build_plan(s, P, start_time, end_time, range_ns, step_ns, g,
                                scratch_per_lane);
    if (rc != GEMX_OK) {
      free_ot_wide_bufs(P);
      return rc;
    }
  }
  /* absent answers every ordinal of every series, as the reference's
   * sample loop does; the others only where the series can have points */
  const int whole_grid = func == OTW_F_ABSENT;
  const uint64_t total_rows =
      whole_grid ? (uint64_t)P.wser.size() * (uint64_t)g.n_ord : P.total_rows;
  if (total_rows > cap) {
    seterr("output capacity too small");
    return GEMX_E_CAP;
  }
  if (total_rows > P.rows_cap) {
    HIP_CHECK(hipStreamSynchronize(s->stream));
    (void)hipFree(P.d_rows);
    P.d_rows = nullptr;
    P.rows_cap = 0;
    HIP_CHECK(hipMalloc(&P.d_rows, sizeof(gemx_rate_row) * total_rows));
    P.rows_cap = total_rows;
  }
  HIP_CHECK(hipMemsetAsync(P.d_err, 0, sizeof(DevErr), s->stream));
  HIP_CHECK(hipMemsetAsync(P.d_cnt, 0, sizeof(unsigned long long) * 3, s->stream));
  HIP_CHECK(hipEventRecord(P.ev[0], s->stream));
  switch (cls) {
  case OTW_C_SUM:
    ot_wide_launch<OTW_C_SUM>(s, P, start_time, func, whole_grid, total_rows,
                              scratch_per_lane);
    break;
  case OTW_C_AVG:
    ot_wide_launch<OTW_C_AVG>(s, P, start_time, func, whole_grid, total_rows,
                              scratch_per_lane);
    break;
  case OTW_C_MINMAX:
    ot_wide_launch<OTW_C_MINMAX>(s, P, start_time, func, whole_grid, total_rows,
                                 scratch_per_lane);
    break;
  case OTW_C_LAST:
    ot_wide_launch<OTW_C_LAST>(s, P, start_time, func, whole_grid, total_rows,
                               scratch_per_lane);
    break;
  case OTW_C_STDVAR:
    ot_wide_launch<OTW_C_STDVAR>(s, P, start_time, func, whole_grid, total_rows,
                                 scratch_per_lane);
    break;
  default:
    ot_wide_launch<OTW_C_CHG>(s, P, start_time, func, whole_grid, total_rows,
                              scratch_per_lane);
    break;
  }
  HIP_CHECK(hipEventRecord(P.ev[2], s->stream));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(P.h_err, P.d_err, sizeof(DevErr), hipMemcpyDeviceToHost,
                           s->stream));
  HIP_CHECK(hipMemcpyAsync(P.h_cnt, P.d_cnt, sizeof(unsigned long long) * 3,
                           hipMemcpyDeviceToHost, s->stream));
  if (total_rows)
    HIP_CHECK(hipMemcpyAsync(out_host, P.d_rows,
                             sizeof(gemx_rate_row) * total_rows,
                             hipMemcpyDeviceToHost, s->stream));
  HIP_CHECK(hipStreamSynchronize(s->stream));
  const DevErr herr = *P.h_err;
  if (herr.code != 0) {
    seterr(herr.code == GEMX_E_UNSUPPORTED ? "unsupported codec on device"
                                           : "segment decode failed on device");
    return herr.code;
  }
  P.last[0] = P.cell_slots;
  P.last[1] = P.h_cnt[0];
  P.last[2] = P.h_cnt[1];
  P.last[3] = P.h_cnt[2];

  /* only non-nil rows leave, as in the ring path's delivery */
  uint64_t n = 0;
  if (herr.gaps == 0) {
    n = total_rows;
  } else {
    uint64_t i = 0;
    while (i < total_rows && !out_host[i].isnil) i++;
    n = i;
    for (; i < total_rows; i++) {
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

extern "C" int gemx_prom_wide_ot_stats(gemx_shard *s, uint64_t *cell_slots,
                                       uint64_t *points, uint64_t *rows_joined,
                                       uint64_t *rows_folded) {
  if (!s) {
    seterr("prom_wide_ot_stats: NULL shard handle");
    return GEMX_E_INVALID;
  }
  const OtWidePlan *P = s->ot_wide_plan;
  if (cell_slots) *cell_slots = P ? P->last[0] : 0;
  if (points) *points = P ? P->last[1] : 0;
  if (rows_joined) *rows_joined = P ? P->last[2] : 0;
  if (rows_folded) *rows_folded = P ? P->last[3] : 0;
  return GEMX_OK;
}

#endif /* __HIPCC__ */
