/*
 * gemx_distinct.hpp — distinct(field) selector scans: the ninth series-level
 * call of the aggregate cursor (engine/series_call_processor.go:56-78).
 *
 * Replaces floatDistinctItem / integerDistinctItem / booleanDistinctItem and
 * the …DistinctReducer.Aggregate loops (engine/series_agg_reducer.gen.go:
 * 1583-1920) and the executor twin DistinctItem[T]
 * (engine/executor/agg_iterator.go:284-332): per (series, window) every
 * distinct value once, with the time of its first occurrence, emitted by
 * (time, value) — the Less of the reference item. A window's result is a
 * pure function of its set of (value, time) points, so it decomposes like
 * top/bottom: per-segment lanes -> lane-owned per-(segment, window)
 * candidate runs -> a tree of sort-and-unique nodes -> emit.
 *
 * Values travel as an order-preserving int64 key (distinct_key): equal keys
 * are equal values and signed key order is value order. Floats are
 * canonicalised first (-0.0 -> +0.0, NaN dropped), so the node
 * kernels are type-agnostic: they sort (key, time) pairs.
 *
 * Included by gemx_engine.hip (single translation unit) after gemx_topn.hpp.
 * No atomics on the data path; the DevErr fields are the exception.
 */

#define DISTINCT_TILE 4096  /* entries of the LDS sort tile (64 KB) */
#define DISTINCT_SMALL 64   /* small node class: one wave, registers only */
#ifndef DISTINCT_SET
#define DISTINCT_SET 4      /* recent-value set of the scan lane */
#endif
#define DISTINCT_TPB 256

/* one candidate / list entry */
struct DItem {
  int64_t k; /* distinct_key of the value */
  int64_t t;
};

/* one child list of a node; off = position of its first entry in the
 * node's tile (host prefix sum over the node's children) */
struct DList {
  const DItem *p;
  uint32_t cnt;
  uint32_t off;
};

/* one tree node: children [child0, child0 + nchild) of the level's list
 * table, `total` entries in all, output at out[out_off ..] */
struct DNode {
  uint32_t child0, nchild;
  uint32_t total, _pad;
  uint64_t out_off;
};

/* one root list and where its rows go */
struct DRoot {
  const DItem *p;
  uint32_t cnt, _pad;
  uint64_t row_off;
  uint64_t bucket; /* per series: SeriesQ.out_base + window; grouped: window - W0 */
};

/* float order as a monotone integer transform of the bits (an involution) */
template <int COLTYPE>
__device__ __forceinline__ int64_t distinct_key(int64_t bits) {
  if (COLTYPE == GEMX_TYPE_FLOAT) return bits ^ ((bits >> 63) & INT64_MAX);
  return bits;
}

__device__ __forceinline__ bool dpair_less(int64_t a0, int64_t a1, int64_t b0,
                                           int64_t b1) {
  return a0 < b0 || (a0 == b0 && a1 < b1);
}

/* The window's most recent distinct values, in registers: statically
 * indexed, fully unrolled (a runtime-indexed private array would live in
 * scratch). A row whose value is here is later in time than the entry that
 * put it here, so it can never be a first occurrence. */
template <int N>
struct DSet {
  int64_t v[N];
  uint32_t n;

  __device__ __forceinline__ void clear() {
    n = 0;
#pragma unroll
    for (int j = 0; j < N; j++) v[j] = 0;
  }
  __device__ __forceinline__ bool has(int64_t x) const {
    bool hit = false;
#pragma unroll
    for (int j = 0; j < N; j++) hit |= ((uint32_t)j < n) & (v[j] == x);
    return hit;
  }
  __device__ __forceinline__ void push(int64_t x) { /* oldest falls out */
#pragma unroll
    for (int j = N - 1; j >= 1; j--) v[j] = v[j - 1];
    v[0] = x;
    if (n < (uint32_t)N) n++;
  }
};

/* One lane per in-range segment. The lane owns cand[cbase[si] .. + rows) and
 * appends one (key, time) candidate per row that is not in its recent-value
 * set; slot (segment, window) records where its run starts and how long it
 * is. FAST = 1: nil-free segments inside the query range, streaming decode
 * (SegStream, gemx_segdecode.hpp). FAST = 0: everything else (and every
 * boolean segment), decoded into per-lane scratch (SegBuffered, which owns
 * the layout, the bounds / length checks and the error codes); nil rows and
 * rows outside the range are skipped. seg_pts / seg_cand receive the lane's non-nil
 * in-range row count and its appended candidate count. */
template <int COLTYPE, int FAST>
__global__ void __launch_bounds__(256) k_distinct_scan(
    const uint8_t *__restrict__ blob, const uint64_t *__restrict__ arena,
    const GorDesc *__restrict__ gors, const gemx_seg_desc *__restrict__ descs,
    const SegQ *__restrict__ segq, const uint64_t *__restrict__ cbase,
    const uint32_t *__restrict__ seg_ids, uint32_t nseg_ids,
    DItem *__restrict__ cand, uint64_t *__restrict__ rstart,
    uint32_t *__restrict__ rcnt, uint32_t *__restrict__ seg_pts,
    uint32_t *__restrict__ seg_cand, int64_t interval, int64_t offset,
    int64_t q_start, int64_t q_end, uint8_t *__restrict__ scratch,
    uint64_t scratch_per_lane, uint32_t nlanes, DevErr *err) {
  uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t stride = FAST ? gridDim.x * blockDim.x : nlanes;
  if (!FAST && gid >= nlanes) return;

  for (uint32_t li = gid; li < nseg_ids; li += stride) {
    uint32_t si = seg_ids[li];
    const gemx_seg_desc d = descs[si];
    const SegQ sq = segq[si];
    if (sq.n_wins == 0) continue; /* segment outside the query range */
    const int rows = (int)d.rows;

    /* a window can hold no usable point (time gaps, nils, NaNs, clipping) */
    for (uint32_t k = 0; k < sq.n_wins; k++) rcnt[sq.partial_base + k] = 0;

    SegStream<COLTYPE> st;
    SegBuffered<COLTYPE> sb;
    if (int rc = FAST ? st.open(blob, arena, gors, si, d)
                      : sb.decode(blob, d, scratch + (uint64_t)gid * scratch_per_lane)) {
      set_err(err, rc);
      return;
    }

    /* current window by range compare; the 64-bit floored division runs
     * only at a window change (as in k_scan_fast) */
    int64_t cur_ord = INT64_MIN;
    int64_t ws_cur = 1, we_cur = 0; /* empty range forces the first window */
    DSet<DISTINCT_SET> set;
    set.clear();
    const uint64_t base = cbase[si];
    uint32_t pos = 0;      /* candidates appended, <= rows seen so far */
    uint32_t run0 = 0;     /* pos at the current window's first candidate */
    uint32_t npts = 0;

    for (int i = 0; i < rows; i++) {
      int64_t t;
      int64_t xv = 0;
      int valid = 1;
      if (int rc = FAST ? st.next(i, &t, &xv) : sb.row(i, &t, &xv, &valid)) {
        set_err(err, rc);
        return;
      }
      if (!valid) continue;
      if (!FAST && (t < q_start || t > q_end)) continue;
      npts++;
      if (COLTYPE == GEMX_TYPE_FLOAT) {
        const double fv = d_bits_f(xv);
        if (fv != fv) continue;   /* NaN is never a key */
        if (fv == 0.0) xv = 0;    /* -0.0 and +0.0 are one key */
      }
      const int64_t key = distinct_key<COLTYPE>(xv);

      if (t >= we_cur || t < ws_cur) {
        if (cur_ord != INT64_MIN) {
          const uint64_t slot = sq.partial_base + (uint64_t)(cur_ord - sq.w_first);
          rstart[slot] = base + run0;
          rcnt[slot] = pos - run0;
        }
        if (interval) {
          cur_ord = win_ordinal(t, interval, offset);
          ws_cur = cur_ord * interval + offset;
          we_cur = ws_cur + interval;
        } else {
          cur_ord = 0;
          ws_cur = INT64_MIN;
          we_cur = INT64_MAX;
        }
        if (cur_ord < sq.w_first || cur_ord >= sq.w_first + (int64_t)sq.n_wins) {
          set_err(err, GEMX_E_INVALID); /* descriptor min/max_time lied */
          return;
        }
        run0 = pos;
        set.n = 0;
      }
      if (set.has(key)) continue;
      set.push(key);
      /* pos < rows: at most one append per row, and this row is not counted yet */
      DItem it;
      it.k = key;
      it.t = t;
      cand[base + pos] = it;
      pos++;
    }
    if (cur_ord != INT64_MIN) {
      const uint64_t slot = sq.partial_base + (uint64_t)(cur_ord - sq.w_first);
      rstart[slot] = base + run0;
      rcnt[slot] = pos - run0;
    }
    seg_pts[si] = npts;
    seg_cand[si] = pos;
  }
}

/* ---- node core: sort by (key, time), keep the head of every key run ---- */

/* Small class, one wave per node, <= 64 entries, in registers: a bitonic
 * network over cross-lane exchanges, then a ballot with popcount for the
 * output positions. Every lane of the wave must be active. Returns the
 * number of distinct keys; lanes with `head` hold an output entry for
 * position `pos`. */
__device__ __forceinline__ uint32_t dnode_wave(int64_t &a, int64_t &b, bool valid,
                                               uint32_t lane, bool *head,
                                               uint32_t *pos) {
  if (!valid) { /* pads sort last; a real entry equal to the pad is the same entry */
    a = INT64_MAX;
    b = INT64_MAX;
  }
  const uint64_t nvalid = __popcll(__ballot(valid));
#pragma unroll
  for (uint32_t k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      const int64_t pa = (int64_t)__shfl_xor((long long)a, (int)j, 64);
      const int64_t pb = (int64_t)__shfl_xor((long long)b, (int)j, 64);
      const bool up = (lane & k) == 0;
      const bool lower = (lane & j) == 0;
      const bool take = (lower == up) ? dpair_less(pa, pb, a, b)
                                      : dpair_less(a, b, pa, pb);
      a = take ? pa : a;
      b = take ? pb : b;
    }
  }
  const int64_t prev = (int64_t)__shfl_up((long long)a, 1, 64);
  const bool hd = lane < nvalid && (lane == 0 || a != prev);
  const uint64_t m = __ballot(hd);
  *head = hd;
  *pos = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  return (uint32_t)__popcll(m);
}

/* Full-tile class, one block per node: bitonic network in LDS over the next
 * power of two >= total (<= DISTINCT_TILE); pads sort last. */
__device__ __forceinline__ void dtile_sort(int64_t *sa, int64_t *sb, uint32_t n2,
                                           uint32_t tid) {
  for (uint32_t k = 2; k <= n2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = tid; i < (n2 >> 1); i += DISTINCT_TPB) {
        /* i-th pair of this step: lo has bit j clear */
        const uint32_t lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        const uint32_t hi = lo | j;
        const bool up = (lo & k) == 0;
        const int64_t a0 = sa[lo], b0 = sb[lo], a1 = sa[hi], b1 = sb[hi];
        const bool sw = up ? dpair_less(a1, b1, a0, b0) : dpair_less(a0, b0, a1, b1);
        if (sw) {
          sa[lo] = a1;
          sb[lo] = b1;
          sa[hi] = a0;
          sb[hi] = b0;
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ uint32_t dtile_pow2(uint32_t total) {
  uint32_t n2 = 2;
  while (n2 < total) n2 <<= 1;
  return n2;
}

/* the tile is sorted by (key, time): write the head of every key run to
 * out[0..), return the number written (uniform over the block). sscan:
 * DISTINCT_TPB words of LDS. */
__device__ __forceinline__ uint32_t dtile_unique(const int64_t *sa, const int64_t *sb,
                                                 uint32_t *sscan, uint32_t total,
                                                 uint32_t n2, uint32_t tid,
                                                 DItem *__restrict__ out) {
  const uint32_t per = n2 >= DISTINCT_TPB ? n2 / DISTINCT_TPB : 1;
  const uint32_t e0 = tid * per;
  uint32_t mine = 0;
  for (uint32_t e = e0; e < e0 + per && e < total; e++)
    mine += (uint32_t)(e == 0 || sa[e] != sa[e - 1]);
  sscan[tid] = mine;
  __syncthreads();
  for (uint32_t st = 1; st < DISTINCT_TPB; st <<= 1) { /* inclusive scan */
    const uint32_t add = tid >= st ? sscan[tid - st] : 0;
    __syncthreads();
    sscan[tid] += add;
    __syncthreads();
  }
  uint32_t w = sscan[tid] - mine;
  const uint32_t uniq = sscan[DISTINCT_TPB - 1];
  for (uint32_t e = e0; e < e0 + per && e < total; e++)
    if (e == 0 || sa[e] != sa[e - 1]) {
      DItem it;
      it.k = sa[e];
      it.t = sb[e];
      out[w++] = it; /* w < uniq <= total: the output holds `total` entries */
    }
  __syncthreads(); /* sscan and the tile are reused by the caller's next node */
  return uniq;
}

/* entry e of a node's concatenated children (children sorted by off) */
__device__ __forceinline__ DItem dnode_entry(const DList *__restrict__ ch,
                                             uint32_t nchild, uint32_t e) {
  uint32_t lo = 0, hi = nchild - 1;
  while (lo < hi) { /* last child with off <= e */
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (ch[mid].off <= e) lo = mid;
    else hi = mid - 1;
  }
  return ch[lo].p[e - ch[lo].off];
}

/* Level 0, small class: one wave per (segment, window) slot whose run holds
 * 2..64 candidates; unique in place, the slot's count is rewritten. */
__global__ void __launch_bounds__(DISTINCT_TPB) k_distinct_node0_small(
    DItem *__restrict__ cand, const uint64_t *__restrict__ rstart,
    uint32_t *__restrict__ rcnt, uint64_t nslots) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wv = (blockIdx.x * (uint64_t)DISTINCT_TPB + threadIdx.x) >> 6;
  const uint64_t nwv = (gridDim.x * (uint64_t)DISTINCT_TPB) >> 6;
  for (uint64_t slot = wv; slot < nslots; slot += nwv) {
    const uint32_t c = rcnt[slot];
    if (c < 2 || c > DISTINCT_SMALL) continue; /* wave-uniform */
    DItem *run = cand + rstart[slot];
    int64_t a = 0, b = 0;
    const bool valid = lane < c;
    if (valid) {
      const DItem it = run[lane];
      a = it.k;
      b = it.t;
    }
    bool head;
    uint32_t pos;
    const uint32_t uniq = dnode_wave(a, b, valid, lane, &head, &pos);
    /* every load of the run precedes the exchanges these stores depend on */
    if (head) {
      DItem it;
      it.k = a;
      it.t = b;
      run[pos] = it; /* pos < uniq <= c */
    }
    if (lane == 0) rcnt[slot] = uniq;
  }
}

/* Level 0, full-tile class: one block per in-range segment walks its
 * window slots and handles the runs of more than 64 candidates (a run is
 * at most one segment, <= 4096 rows). */
__global__ void __launch_bounds__(DISTINCT_TPB) k_distinct_node0_tile(
    DItem *__restrict__ cand, const uint64_t *__restrict__ rstart,
    uint32_t *__restrict__ rcnt, const SegQ *__restrict__ segq,
    const uint32_t *__restrict__ seg_ids, uint32_t nseg_ids, DevErr *err) {
  __shared__ int64_t sa[DISTINCT_TILE];
  __shared__ int64_t sb[DISTINCT_TILE];
  __shared__ uint32_t sscan[DISTINCT_TPB];
  const uint32_t tid = threadIdx.x;
  for (uint32_t li = blockIdx.x; li < nseg_ids; li += gridDim.x) {
    const SegQ sq = segq[seg_ids[li]];
    for (uint32_t k = 0; k < sq.n_wins; k++) {
      const uint64_t slot = sq.partial_base + k;
      const uint32_t c = rcnt[slot]; /* block-uniform; rewritten only after
                                        the barriers every thread passes */
      if (c <= DISTINCT_SMALL) continue;
      if (c > DISTINCT_TILE) { set_err(err, GEMX_E_INVALID); return; }
      DItem *run = cand + rstart[slot];
      const uint32_t n2 = dtile_pow2(c);
      for (uint32_t e = tid; e < n2; e += DISTINCT_TPB) {
        DItem it;
        it.k = INT64_MAX;
        it.t = INT64_MAX;
        if (e < c) it = run[e];
        sa[e] = it.k;
        sb[e] = it.t;
      }
      __syncthreads();
      dtile_sort(sa, sb, n2, tid);
      const uint32_t uniq = dtile_unique(sa, sb, sscan, c, n2, tid, run);
      if (tid == 0) {
        rcnt[slot] = uniq;
        if (uniq > GEMX_DISTINCT_MAX) atomicExch(&err->distinct_over, 1u);
      }
    }
  }
}

/* Level >= 1, small class: one wave per node of <= 64 entries. */
__global__ void __launch_bounds__(DISTINCT_TPB) k_distinct_node_small(
    const DNode *__restrict__ nodes, uint32_t n_nodes,
    const DList *__restrict__ lists, DItem *__restrict__ out,
    uint32_t *__restrict__ ncnt) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wv = (blockIdx.x * (uint64_t)DISTINCT_TPB + threadIdx.x) >> 6;
  const uint64_t nwv = (gridDim.x * (uint64_t)DISTINCT_TPB) >> 6;
  for (uint64_t ni = wv; ni < n_nodes; ni += nwv) {
    const DNode nd = nodes[ni];
    if (nd.total > DISTINCT_SMALL || nd.nchild == 0) continue; /* host invariant */
    int64_t a = 0, b = 0;
    const bool valid = lane < nd.total;
    if (valid) {
      const DItem it = dnode_entry(lists + nd.child0, nd.nchild, lane);
      a = it.k;
      b = it.t;
    }
    bool head;
    uint32_t pos;
    const uint32_t uniq = dnode_wave(a, b, valid, lane, &head, &pos);
    if (head) {
      DItem it;
      it.k = a;
      it.t = b;
      out[nd.out_off + pos] = it;
    }
    if (lane == 0) ncnt[ni] = uniq;
  }
}

/* Level >= 1, full-tile class: one block per node of <= 4096 entries. */
__global__ void __launch_bounds__(DISTINCT_TPB) k_distinct_node_tile(
    const DNode *__restrict__ nodes, uint32_t n_nodes,
    const DList *__restrict__ lists, DItem *__restrict__ out,
    uint32_t *__restrict__ ncnt, DevErr *err) {
  __shared__ int64_t sa[DISTINCT_TILE];
  __shared__ int64_t sb[DISTINCT_TILE];
  __shared__ uint32_t sscan[DISTINCT_TPB];
  const uint32_t tid = threadIdx.x;
  for (uint32_t ni = blockIdx.x; ni < n_nodes; ni += gridDim.x) {
    const DNode nd = nodes[ni];
    if (nd.total > DISTINCT_TILE || nd.nchild == 0) { /* host invariant */
      set_err(err, GEMX_E_INVALID);
      return;
    }
    const uint32_t n2 = dtile_pow2(nd.total);
    for (uint32_t e = tid; e < n2; e += DISTINCT_TPB) {
      DItem it;
      it.k = INT64_MAX;
      it.t = INT64_MAX;
      if (e < nd.total) it = dnode_entry(lists + nd.child0, nd.nchild, e);
      sa[e] = it.k;
      sb[e] = it.t;
    }
    __syncthreads();
    dtile_sort(sa, sb, n2, tid);
    const uint32_t uniq =
        dtile_unique(sa, sb, sscan, nd.total, n2, tid, out + nd.out_off);
    if (tid == 0) {
      ncnt[ni] = uniq;
      if (uniq > GEMX_DISTINCT_MAX) atomicExch(&err->distinct_over, 1u);
    }
  }
}

/* ---- emit: a root list ordered by (time, value) -> gemx_point_rows ---- */

template <int COLTYPE>
__device__ __forceinline__ void distinct_row(gemx_point_row *__restrict__ dst,
                                             const SeriesQ *__restrict__ series,
                                             uint32_t nseries, int group_all,
                                             uint64_t bucket, int64_t W0,
                                             int64_t interval, int64_t offset,
                                             int64_t q_start, int64_t t, int64_t key) {
  gemx_point_row r;
  int64_t w;
  if (group_all) {
    r.sid = 0;
    w = W0 + (int64_t)bucket;
  } else {
    uint32_t lo = 0, hi = nseries - 1;
    while (lo < hi) {
      uint32_t mid = (lo + hi + 1) >> 1;
      if (series[mid].out_base <= bucket) lo = mid;
      else hi = mid - 1;
    }
    r.sid = series[lo].sid;
    w = series[lo].w_min + (int64_t)(bucket - series[lo].out_base);
  }
  r.win_start = interval ? win_start_of(w, interval, offset) : q_start;
  r.time = t;
  r.v.i = distinct_key<COLTYPE>(key); /* the key transform is an involution */
  *dst = r;
}

/* roots of <= 64 entries: one wave each, sorted in registers */
template <int COLTYPE>
__global__ void __launch_bounds__(DISTINCT_TPB) k_distinct_emit_small(
    const DRoot *__restrict__ roots, uint32_t n_roots,
    const SeriesQ *__restrict__ series, uint32_t nseries, int group_all,
    int64_t W0, int64_t interval, int64_t offset, int64_t q_start,
    gemx_point_row *__restrict__ rows) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wv = (blockIdx.x * (uint64_t)DISTINCT_TPB + threadIdx.x) >> 6;
  const uint64_t nwv = (gridDim.x * (uint64_t)DISTINCT_TPB) >> 6;
  for (uint64_t ri = wv; ri < n_roots; ri += nwv) {
    const DRoot rt = roots[ri];
    if (rt.cnt > DISTINCT_SMALL) continue; /* host invariant */
    int64_t a = 0, b = 0; /* (time, key): the emission order */
    const bool valid = lane < rt.cnt;
    if (valid) {
      const DItem it = rt.p[lane];
      a = it.t;
      b = it.k;
    }
    bool head;
    uint32_t pos;
    (void)dnode_wave(a, b, valid, lane, &head, &pos);
    /* keys are unique in a root, so after the sort lane i holds row i */
    if (valid)
      distinct_row<COLTYPE>(rows + rt.row_off + lane, series, nseries, group_all,
                            rt.bucket, W0, interval, offset, q_start, a, b);
  }
}

/* roots of 65..GEMX_DISTINCT_MAX entries: one block each, half a tile */
template <int COLTYPE>
__global__ void __launch_bounds__(DISTINCT_TPB) k_distinct_emit_tile(
    const DRoot *__restrict__ roots, uint32_t n_roots,
    const SeriesQ *__restrict__ series, uint32_t nseries, int group_all,
    int64_t W0, int64_t interval, int64_t offset, int64_t q_start,
    gemx_point_row *__restrict__ rows, DevErr *err) {
  __shared__ int64_t sa[GEMX_DISTINCT_MAX];
  __shared__ int64_t sb[GEMX_DISTINCT_MAX];
  const uint32_t tid = threadIdx.x;
  for (uint32_t ri = blockIdx.x; ri < n_roots; ri += gridDim.x) {
    const DRoot rt = roots[ri];
    if (rt.cnt > GEMX_DISTINCT_MAX) { set_err(err, GEMX_E_INVALID); return; }
    const uint32_t n2 = dtile_pow2(rt.cnt);
    for (uint32_t e = tid; e < n2; e += DISTINCT_TPB) {
      DItem it;
      it.k = INT64_MAX;
      it.t = INT64_MAX;
      if (e < rt.cnt) it = rt.p[e];
      sa[e] = it.t;
      sb[e] = it.k;
    }
    __syncthreads();
    dtile_sort(sa, sb, n2, tid);
    for (uint32_t e = tid; e < rt.cnt; e += DISTINCT_TPB)
      distinct_row<COLTYPE>(rows + rt.row_off + e, series, nseries, group_all,
                            rt.bucket, W0, interval, offset, q_start, sa[e], sb[e]);
    __syncthreads(); /* the tile is reloaded for the next root */
  }
}

/* ---------------- host ---------------- */

/* Device state of distinct queries, separate from QueryPlan and TopPlan:
 * gemx_scan_distinct never rebuilds or frees a buffer that an in-flight
 * begin/finish aggregate query or a top/bottom query uses. */
struct DistinctPlan {
  bool valid = false;
  int64_t start = 0, end = 0, interval = 0, offset = 0;
  std::vector<SegQ> segq;
  std::vector<SeriesQ> sq;
  std::vector<uint32_t> in_q; /* in-range segments, descriptor order */
  uint64_t slots = 0, total_wins = 0, n_gwins = 0, cand_cap = 0;
  int64_t W0 = 0;
  /* slots in bucket order, [0] per (series, window), [1] per window; a
   * bucket's slots keep (series, segment) order. Built on first use. */
  std::vector<uint64_t> order[2], bucket_off[2];
  SegQ *d_segq = nullptr;
  SeriesQ *d_sq = nullptr;
  uint64_t *d_cbase = nullptr;
  uint32_t *d_fast_q = nullptr, *d_gen_q = nullptr, *d_in_q = nullptr;
  uint32_t n_fast_q = 0, n_gen_q = 0, gen_lanes = 0;
  uint8_t *d_scratch = nullptr;
  DItem *d_cand = nullptr; /* 16 B per in-range row, allocated when first needed */
  uint64_t *d_rstart = nullptr, *h_rstart = nullptr;
  uint32_t *d_rcnt = nullptr, *h_rcnt = nullptr;
  uint32_t *d_seg_pts = nullptr, *d_seg_cand = nullptr;
  /* per level >= 1: output lists; kept so that later queries reuse them */
  std::vector<DItem *> d_level;
  std::vector<uint64_t> level_cap;
  /* grow-only upload / result buffers */
  DList *d_lists = nullptr;
  DNode *d_nodes = nullptr;
  uint32_t *d_ncnt = nullptr;
  DRoot *d_roots = nullptr;
  gemx_point_row *d_rows = nullptr;
  uint64_t lists_cap = 0, nodes_cap = 0, ncnt_cap = 0, roots_cap = 0, rows_cap = 0;
  DevErr *d_err = nullptr, *h_err = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  /* gemx_distinct_stats: the last query */
  uint64_t last_candidates = 0, last_points = 0;
  uint32_t last_levels = 0;
};

static void free_distinct_plan_bufs(DistinctPlan &p) {
  void *dev[] = {p.d_segq,   p.d_sq,      p.d_cbase,    p.d_fast_q, p.d_gen_q,
                 p.d_in_q,   p.d_scratch, p.d_cand,     p.d_rstart, p.d_rcnt,
                 p.d_seg_pts, p.d_seg_cand, p.d_lists,  p.d_nodes,  p.d_ncnt,
                 p.d_roots,  p.d_rows,    p.d_err};
  for (void *q : dev)
    if (q) (void)hipFree(q);
  for (DItem *q : p.d_level)
    if (q) (void)hipFree(q);
  if (p.h_rstart) (void)hipHostFree(p.h_rstart);
  if (p.h_rcnt) (void)hipHostFree(p.h_rcnt);
  if (p.h_err) (void)hipHostFree(p.h_err);
  for (int e = 0; e < 3; e++)
    if (p.ev[e]) (void)hipEventDestroy(p.ev[e]);
  p = DistinctPlan();
}

static void free_distinct_plan(gemx_shard *s) {
  if (!s->distinct_plan) return;
  free_distinct_plan_bufs(*s->distinct_plan);
  delete s->distinct_plan;
  s->distinct_plan = nullptr;
}

/* grow-only device buffer of COUNT elements */
template <typename T>
static hipError_t distinct_grow(T *&ptr, uint64_t &cap, uint64_t count) {
  if (count <= cap && ptr) return hipSuccess;
  if (ptr) (void)hipFree(ptr);
  ptr = nullptr;
  cap = 0;
  hipError_t e = hipMalloc(&ptr, sizeof(T) * (count ? count : 1));
  if (e == hipSuccess) cap = count ? count : 1;
  return e;
}

/* window spans, output ranges, launch lists, the candidate layout and the
 * fixed buffers for one (start, end, interval, offset) */
static int distinct_build_plan(gemx_shard *s, DistinctPlan &P, int64_t start_time,
                               int64_t end_time, int64_t interval, int64_t offset,
                               uint64_t scratch_per_lane) {
  const uint64_t nsegs = s->nsegs;
  free_distinct_plan_bufs(P);
  P.segq.resize(nsegs);
  P.sq.resize(s->series_ranges.size());
  std::vector<uint32_t> fast_q, gen_q;
  std::vector<uint64_t> cbase(nsegs ? nsegs : 1, 0);
  std::vector<char> is_gen(nsegs, 0);
  for (auto id : s->general_ids) is_gen[id] = 1;
  const bool all_gen = (s->col_type == GEMX_TYPE_BOOL); /* bits unpack in scratch */
  for (size_t g = 0; g < s->series_ranges.size(); g++) {
    auto &r = s->series_ranges[g];
    int64_t wmin = INT64_MAX, wmax = INT64_MIN;
    /* running max of (w_first + n_wins), clamped sentinels for out-of-range
     * segments: the aggregate plan's invariant (see topn_build_plan) */
    int64_t run = INT64_MIN;
    for (uint32_t i = r.start; i < r.start + r.count; i++) {
      const gemx_seg_desc &d = s->h_descs[i];
      P.segq[i].partial_base = P.slots;
      P.segq[i].series_idx = (uint32_t)g;
      cbase[i] = P.cand_cap;
      if (d.max_time < start_time || d.min_time > end_time) {
        int64_t cand;
        if (interval) {
          int64_t ct = std::min(std::max(d.min_time, start_time), end_time);
          cand = win_ordinal(ct, interval, offset) + (d.min_time > end_time ? 1 : 0);
        } else {
          cand = (d.min_time > end_time) ? 1 : 0;
        }
        P.segq[i].w_first = std::max(cand, run);
        P.segq[i].n_wins = 0;
        run = P.segq[i].w_first;
        continue;
      }
      int64_t mt = std::max(d.min_time, start_time);
      int64_t xt = std::min(d.max_time, end_time);
      int64_t w0 = interval ? win_ordinal(mt, interval, offset) : 0;
      int64_t w1 = interval ? win_ordinal(xt, interval, offset) : 0;
      P.segq[i].w_first = w0;
      P.segq[i].n_wins = (uint32_t)(w1 - w0 + 1);
      run = std::max(run, w1 + 1);
      P.slots += P.segq[i].n_wins;
      P.cand_cap += d.rows; /* the lane's region: one entry per row */
      wmin = std::min(wmin, w0);
      wmax = std::max(wmax, w1);
      const bool clip = (d.min_time < start_time || d.max_time > end_time);
      if (clip || is_gen[i] || all_gen) gen_q.push_back(i);
      else fast_q.push_back(i);
      P.in_q.push_back(i);
    }
    if (wmin == INT64_MAX) { /* series entirely out of range */
      wmin = 0;
      wmax = -1;
    }
    P.sq[g].sid = r.sid;
    P.sq[g].w_min = wmin;
    P.sq[g].out_base = P.total_wins;
    P.sq[g].n_wins = (uint32_t)(wmax - wmin + 1);
    P.sq[g].seg_start = r.start;
    P.sq[g].seg_count = r.count;
    P.total_wins += P.sq[g].n_wins;
  }
  /* arena-mode gorilla lanes in arena slot order */
  if (!s->h_gor.empty())
    std::stable_sort(fast_q.begin(), fast_q.end(), [&](uint32_t x, uint32_t y) {
      return s->h_gor[x].arena_base < s->h_gor[y].arena_base;
    });
  {
    int64_t W0 = INT64_MAX, W1 = INT64_MIN;
    for (auto &g : P.sq) {
      if (g.n_wins == 0) continue;
      W0 = std::min(W0, g.w_min);
      W1 = std::max(W1, g.w_min + (int64_t)g.n_wins - 1);
    }
    P.W0 = (W0 == INT64_MAX) ? 0 : W0;
    P.n_gwins = (W0 == INT64_MAX) ? 0 : (uint64_t)(W1 - W0 + 1);
  }
#define DIST_ALLOC(PTR, TYPE, COUNT)                                           \
  HIP_CHECK(hipMalloc(&PTR, sizeof(TYPE) * ((COUNT) ? (COUNT) : 1)))
#define DIST_UPLOAD(PTR, TYPE, VEC)                                            \
  do {                                                                         \
    DIST_ALLOC(PTR, TYPE, (VEC).size());                                       \
    if (!(VEC).empty())                                                        \
      HIP_CHECK(hipMemcpyAsync(PTR, (VEC).data(), sizeof(TYPE) * (VEC).size(), \
                               hipMemcpyHostToDevice, s->stream));             \
  } while (0)
  DIST_UPLOAD(P.d_segq, SegQ, P.segq);
  DIST_UPLOAD(P.d_sq, SeriesQ, P.sq);
  DIST_UPLOAD(P.d_cbase, uint64_t, cbase);
  DIST_UPLOAD(P.d_fast_q, uint32_t, fast_q);
  DIST_UPLOAD(P.d_gen_q, uint32_t, gen_q);
  DIST_UPLOAD(P.d_in_q, uint32_t, P.in_q);
  P.n_fast_q = (uint32_t)fast_q.size();
  P.n_gen_q = (uint32_t)gen_q.size();
  DIST_ALLOC(P.d_cand, DItem, P.cand_cap);
  DIST_ALLOC(P.d_rstart, uint64_t, P.slots);
  DIST_ALLOC(P.d_rcnt, uint32_t, P.slots);
  DIST_ALLOC(P.d_seg_pts, uint32_t, nsegs);
  DIST_ALLOC(P.d_seg_cand, uint32_t, nsegs);
  /* a lane that stops on a decode error leaves its slots unwritten: they
   * must read as empty runs, never as whatever the allocation held */
  HIP_CHECK(hipMemsetAsync(P.d_rcnt, 0, sizeof(uint32_t) * (P.slots ? P.slots : 1),
                           s->stream));
  HIP_CHECK(hipMemsetAsync(P.d_rstart, 0, sizeof(uint64_t) * (P.slots ? P.slots : 1),
                           s->stream));
  /* out-of-range segments are never written: their counts stay zero */
  HIP_CHECK(hipMemsetAsync(P.d_seg_pts, 0, sizeof(uint32_t) * (nsegs ? nsegs : 1),
                           s->stream));
  HIP_CHECK(hipMemsetAsync(P.d_seg_cand, 0, sizeof(uint32_t) * (nsegs ? nsegs : 1),
                           s->stream));
  HIP_CHECK(hipHostMalloc(&P.h_rstart, sizeof(uint64_t) * (P.slots ? P.slots : 1)));
  HIP_CHECK(hipHostMalloc(&P.h_rcnt, sizeof(uint32_t) * (P.slots ? P.slots : 1)));
  if (P.n_gen_q) {
    P.gen_lanes = std::min<uint32_t>(P.n_gen_q, 16384);
    HIP_CHECK(hipMalloc(&P.d_scratch, scratch_per_lane * P.gen_lanes));
  }
  HIP_CHECK(hipMalloc(&P.d_err, sizeof(DevErr)));
  HIP_CHECK(hipHostMalloc(&P.h_err, sizeof(DevErr)));
  for (int e = 0; e < 3; e++) HIP_CHECK(hipEventCreate(&P.ev[e]));
#undef DIST_UPLOAD
#undef DIST_ALLOC
  HIP_CHECK(hipStreamSynchronize(s->stream)); /* the uploads read locals */
  P.start = start_time;
  P.end = end_time;
  P.interval = interval;
  P.offset = offset;
  P.valid = true;
  return GEMX_OK;
}

/* slots in bucket order (stable counting sort of the series-major walk) */
static void distinct_build_order(DistinctPlan &P, int mode) {
  const uint64_t nb = mode ? P.n_gwins : P.total_wins;
  std::vector<uint64_t> &off = P.bucket_off[mode];
  std::vector<uint64_t> &ord = P.order[mode];
  off.assign(nb + 1, 0);
  ord.assign(P.slots, 0);
  auto bucket_of = [&](const SegQ &q, uint32_t k) -> uint64_t {
    const int64_t w = q.w_first + (int64_t)k;
    if (mode) return (uint64_t)(w - P.W0);
    const SeriesQ &g = P.sq[q.series_idx];
    return g.out_base + (uint64_t)(w - g.w_min);
  };
  for (uint32_t i : P.in_q)
    for (uint32_t k = 0; k < P.segq[i].n_wins; k++) off[bucket_of(P.segq[i], k) + 1]++;
  for (uint64_t b = 0; b < nb; b++) off[b + 1] += off[b];
  std::vector<uint64_t> fill(off.begin(), off.end() - 1);
  for (uint32_t i : P.in_q)
    for (uint32_t k = 0; k < P.segq[i].n_wins; k++)
      ord[fill[bucket_of(P.segq[i], k)]++] = P.segq[i].partial_base + k;
}

/* a list on the host side of the tree */
struct DHostList {
  const DItem *p;
  uint32_t cnt;
  uint64_t bucket;
};

template <int COLTYPE>
static void distinct_launch_scan(gemx_shard *s, DistinctPlan &P) {
  const int TPB = 256;
  const uint64_t scratch_per_lane = seg_scratch_bytes(SEG_SPARE_SCAN);
  if constexpr (COLTYPE != GEMX_TYPE_BOOL) { /* boolean shards: FAST = 0 only */
    if (P.n_fast_q) {
      uint32_t blocks = std::min<uint32_t>((P.n_fast_q + TPB - 1) / TPB, 65535);
      hipLaunchKernelGGL((k_distinct_scan<COLTYPE, 1>), dim3(blocks), dim3(TPB), 0,
                         s->stream, s->d_blob, s->d_arena, s->d_gor, s->d_descs,
                         P.d_segq, P.d_cbase, P.d_fast_q, P.n_fast_q, P.d_cand,
                         P.d_rstart, P.d_rcnt, P.d_seg_pts, P.d_seg_cand, P.interval,
                         P.offset, P.start, P.end, nullptr, 0, 0, P.d_err);
    }
  }
  if (P.n_gen_q) {
    uint32_t blocks = (P.gen_lanes + TPB - 1) / TPB;
    hipLaunchKernelGGL((k_distinct_scan<COLTYPE, 0>), dim3(blocks), dim3(TPB), 0,
                       s->stream, s->d_blob, s->d_arena, s->d_gor, s->d_descs,
                       P.d_segq, P.d_cbase, P.d_gen_q, P.n_gen_q, P.d_cand,
                       P.d_rstart, P.d_rcnt, P.d_seg_pts, P.d_seg_cand, P.interval,
                       P.offset, P.start, P.end, P.d_scratch, scratch_per_lane,
                       P.gen_lanes, P.d_err);
  }
}

template <int COLTYPE>
static void distinct_launch_emit(gemx_shard *s, DistinctPlan &P, int group_all,
                                 uint32_t n_small, uint32_t n_tile) {
  if (n_small) {
    uint32_t blocks = std::min<uint32_t>((n_small + 3) / 4, 65535);
    hipLaunchKernelGGL((k_distinct_emit_small<COLTYPE>), dim3(blocks),
                       dim3(DISTINCT_TPB), 0, s->stream, P.d_roots, n_small, P.d_sq,
                       (uint32_t)P.sq.size(), group_all, P.W0, P.interval, P.offset,
                       P.start, P.d_rows);
  }
  if (n_tile) {
    uint32_t blocks = std::min<uint32_t>(n_tile, 65535);
    hipLaunchKernelGGL((k_distinct_emit_tile<COLTYPE>), dim3(blocks),
                       dim3(DISTINCT_TPB), 0, s->stream, P.d_roots + n_small, n_tile,
                       P.d_sq, (uint32_t)P.sq.size(), group_all, P.W0, P.interval,
                       P.offset, P.start, P.d_rows, P.d_err);
  }
}

static int distinct_dev_error(const DevErr &e) {
  if (e.code != 0) {
    seterr(e.code == GEMX_E_UNSUPPORTED ? "unsupported codec on device"
           : e.code == GEMX_E_INVALID
               ? "segment descriptor inconsistent with its data"
               : "segment decode failed on device");
    return e.code;
  }
  if (e.distinct_over) {
    seterr("scan_distinct: a window holds more than GEMX_DISTINCT_MAX (2048) "
           "distinct values");
    return GEMX_E_UNSUPPORTED;
  }
  return GEMX_OK;
}

extern "C" int gemx_scan_distinct(gemx_shard *s, int64_t start_time,
                                  int64_t end_time, int64_t interval,
                                  int64_t offset, int group_all,
                                  gemx_point_row *out_host, uint64_t cap,
                                  uint64_t *n_out, gemx_query_stats *stats) {
  if (!s) {
    seterr("scan_distinct: NULL shard handle");
    return GEMX_E_INVALID;
  }
  if (interval < 0 || !n_out || (!out_host && cap)) {
    seterr("scan_distinct: bad arguments");
    return GEMX_E_INVALID;
  }
  if (interval > 0 && s->nsegs) {
    const double lo = (double)std::max(start_time, s->shard_min_t);
    const double hi = (double)std::min(end_time, s->shard_max_t);
    if (hi > lo && (hi - lo) / (double)interval > 1e9) {
      seterr("scan_distinct: more than 1e9 windows in the query range");
      return GEMX_E_INVALID;
    }
  }
  HIP_CHECK(hipSetDevice(s->device));
  const uint64_t scratch_per_lane = seg_scratch_bytes(SEG_SPARE_SCAN);
  if (!s->distinct_plan) s->distinct_plan = new DistinctPlan();
  DistinctPlan &P = *s->distinct_plan;
  if (!P.valid || P.start != start_time || P.end != end_time ||
      P.interval != interval || P.offset != offset) {
    int rc = distinct_build_plan(s, P, start_time, end_time, interval, offset,
                                 scratch_per_lane);
    if (rc != GEMX_OK) {
      free_distinct_plan_bufs(P);
      return rc;
    }
  }
  const int mode = group_all ? 1 : 0;
  if (P.bucket_off[mode].empty()) distinct_build_order(P, mode);
  P.last_candidates = P.last_points = 0;
  P.last_levels = 0;
  *n_out = 0;

  /* ---- scan, then level 0: every candidate run unique in place ---- */
  HIP_CHECK(hipMemsetAsync(P.d_err, 0, sizeof(DevErr), s->stream));
  (void)hipEventRecord(P.ev[0], s->stream);
  if (s->col_type == GEMX_TYPE_FLOAT) distinct_launch_scan<GEMX_TYPE_FLOAT>(s, P);
  else if (s->col_type == GEMX_TYPE_BOOL) distinct_launch_scan<GEMX_TYPE_BOOL>(s, P);
  else distinct_launch_scan<GEMX_TYPE_INT>(s, P);
  (void)hipEventRecord(P.ev[1], s->stream);
  if (P.slots) {
    uint32_t blocks = (uint32_t)std::min<uint64_t>((P.slots + 3) / 4, 65535);
    hipLaunchKernelGGL(k_distinct_node0_small, dim3(blocks), dim3(DISTINCT_TPB), 0,
                       s->stream, P.d_cand, P.d_rstart, P.d_rcnt, P.slots);
    blocks = (uint32_t)std::min<uint64_t>(P.in_q.size(), 65535);
    hipLaunchKernelGGL(k_distinct_node0_tile, dim3(blocks), dim3(DISTINCT_TPB), 0,
                       s->stream, P.d_cand, P.d_rstart, P.d_rcnt, P.d_segq, P.d_in_q,
                       (uint32_t)P.in_q.size(), P.d_err);
  }
  HIP_CHECK(hipGetLastError());
  std::vector<uint32_t> seg_pts(s->nsegs), seg_cand(s->nsegs);
  if (P.slots) {
    HIP_CHECK(hipMemcpyAsync(P.h_rstart, P.d_rstart, sizeof(uint64_t) * P.slots,
                             hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipMemcpyAsync(P.h_rcnt, P.d_rcnt, sizeof(uint32_t) * P.slots,
                             hipMemcpyDeviceToHost, s->stream));
  }
  if (s->nsegs) {
    HIP_CHECK(hipMemcpyAsync(seg_pts.data(), P.d_seg_pts, sizeof(uint32_t) * s->nsegs,
                             hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipMemcpyAsync(seg_cand.data(), P.d_seg_cand,
                             sizeof(uint32_t) * s->nsegs, hipMemcpyDeviceToHost,
                             s->stream));
  }
  HIP_CHECK(hipMemcpyAsync(P.h_err, P.d_err, sizeof(DevErr), hipMemcpyDeviceToHost,
                           s->stream));
  HIP_CHECK(hipStreamSynchronize(s->stream));
  {
    int rc = distinct_dev_error(*P.h_err);
    if (rc != GEMX_OK) return rc;
  }
  for (uint32_t i : P.in_q) {
    P.last_points += seg_pts[i];
    P.last_candidates += seg_cand[i];
  }
  uint32_t levels = 1;

  /* ---- the lists of every bucket, bucket order ---- */
  const std::vector<uint64_t> &boff = P.bucket_off[mode];
  const std::vector<uint64_t> &bord = P.order[mode];
  const uint64_t nb = boff.size() - 1;
  std::vector<DHostList> cur, nxt;
  cur.reserve(P.slots);
  for (uint64_t b = 0; b < nb; b++)
    for (uint64_t j = boff[b]; j < boff[b + 1]; j++) {
      const uint64_t slot = bord[j];
      if (P.h_rcnt[slot] == 0) continue;
      cur.push_back({P.d_cand + P.h_rstart[slot], P.h_rcnt[slot], b});
    }

  /* ---- levels >= 1: greedy packing of consecutive lists of a bucket into
   * nodes of <= DISTINCT_TILE entries. Every list holds <= 2048 entries, so
   * a node with a second child available takes it: the list count of a
   * bucket at least halves (rounded up) per level. ---- */
  std::vector<DList> lists;
  std::vector<DNode> nodes_small, nodes_tile;
  std::vector<uint32_t> ncnt;
  /* where a node's output goes in nxt */
  std::vector<uint64_t> small_at, tile_at;
  for (;;) {
    lists.clear();
    nodes_small.clear();
    nodes_tile.clear();
    small_at.clear();
    tile_at.clear();
    nxt.clear();
    uint64_t out_total = 0;
    size_t i = 0;
    while (i < cur.size()) {
      size_t e = i + 1;
      while (e < cur.size() && cur[e].bucket == cur[i].bucket) e++;
      size_t a = i;
      while (a < e) {
        uint32_t total = cur[a].cnt;
        size_t z = a + 1;
        while (z < e && total + cur[z].cnt <= DISTINCT_TILE) total += cur[z++].cnt;
        if (z - a == 1) {
          nxt.push_back(cur[a]); /* a unique list already: carried as it is */
        } else {
          DNode nd;
          nd.child0 = (uint32_t)lists.size();
          nd.nchild = (uint32_t)(z - a);
          nd.total = total;
          nd._pad = 0;
          nd.out_off = out_total;
          uint32_t off = 0;
          for (size_t c = a; c < z; c++) {
            lists.push_back({cur[c].p, cur[c].cnt, off});
            off += cur[c].cnt;
          }
          out_total += total;
          if (total <= DISTINCT_SMALL) {
            nodes_small.push_back(nd);
            small_at.push_back(nxt.size());
          } else {
            nodes_tile.push_back(nd);
            tile_at.push_back(nxt.size());
          }
          nxt.push_back({nullptr, 0, cur[a].bucket});
        }
        a = z;
      }
      i = e;
    }
    const uint64_t n_small = nodes_small.size(), n_tile = nodes_tile.size();
    if (n_small + n_tile == 0) break; /* one list per bucket: the roots */
    if (lists.size() > 0xffffffffull || n_small + n_tile > 0xffffffffull) {
      seterr("scan_distinct: too many lists in one tree level");
      return GEMX_E_INVALID;
    }
    const uint32_t lv = levels - 1;
    if (P.d_level.size() <= lv) {
      P.d_level.resize(lv + 1, nullptr);
      P.level_cap.resize(lv + 1, 0);
    }
    HIP_CHECK(distinct_grow(P.d_level[lv], P.level_cap[lv], out_total));
    HIP_CHECK(distinct_grow(P.d_lists, P.lists_cap, lists.size()));
    HIP_CHECK(distinct_grow(P.d_nodes, P.nodes_cap, n_small + n_tile));
    HIP_CHECK(distinct_grow(P.d_ncnt, P.ncnt_cap, n_small + n_tile));
    HIP_CHECK(hipMemcpyAsync(P.d_lists, lists.data(), sizeof(DList) * lists.size(),
                             hipMemcpyHostToDevice, s->stream));
    if (n_small)
      HIP_CHECK(hipMemcpyAsync(P.d_nodes, nodes_small.data(), sizeof(DNode) * n_small,
                               hipMemcpyHostToDevice, s->stream));
    if (n_tile)
      HIP_CHECK(hipMemcpyAsync(P.d_nodes + n_small, nodes_tile.data(),
                               sizeof(DNode) * n_tile, hipMemcpyHostToDevice,
                               s->stream));
    if (n_small) {
      uint32_t blocks = (uint32_t)std::min<uint64_t>((n_small + 3) / 4, 65535);
      hipLaunchKernelGGL(k_distinct_node_small, dim3(blocks), dim3(DISTINCT_TPB), 0,
                         s->stream, P.d_nodes, (uint32_t)n_small, P.d_lists,
                         P.d_level[lv], P.d_ncnt);
    }
    if (n_tile) {
      uint32_t blocks = (uint32_t)std::min<uint64_t>(n_tile, 65535);
      hipLaunchKernelGGL(k_distinct_node_tile, dim3(blocks), dim3(DISTINCT_TPB), 0,
                         s->stream, P.d_nodes + n_small, (uint32_t)n_tile, P.d_lists,
                         P.d_level[lv], P.d_ncnt + n_small, P.d_err);
    }
    HIP_CHECK(hipGetLastError());
    ncnt.resize(n_small + n_tile);
    HIP_CHECK(hipMemcpyAsync(ncnt.data(), P.d_ncnt, sizeof(uint32_t) * ncnt.size(),
                             hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipMemcpyAsync(P.h_err, P.d_err, sizeof(DevErr), hipMemcpyDeviceToHost,
                             s->stream));
    HIP_CHECK(hipStreamSynchronize(s->stream));
    levels++;
    P.last_levels = levels;
    {
      int rc = distinct_dev_error(*P.h_err);
      if (rc != GEMX_OK) return rc;
    }
    for (uint64_t k = 0; k < n_small; k++) {
      nxt[small_at[k]].p = P.d_level[lv] + nodes_small[k].out_off;
      nxt[small_at[k]].cnt = ncnt[k];
    }
    for (uint64_t k = 0; k < n_tile; k++) {
      nxt[tile_at[k]].p = P.d_level[lv] + nodes_tile[k].out_off;
      nxt[tile_at[k]].cnt = ncnt[n_small + k];
    }
    cur.swap(nxt);
  }
  P.last_levels = levels;

  /* ---- roots -> rows at the prefix sum of their counts ---- */
  std::vector<DRoot> roots_small, roots_tile;
  uint64_t m = 0;
  for (const DHostList &l : cur) {
    if (l.cnt > GEMX_DISTINCT_MAX) { /* a carried level-0 list: checked on device too */
      seterr("scan_distinct: a window holds more than GEMX_DISTINCT_MAX (2048) "
             "distinct values");
      return GEMX_E_UNSUPPORTED;
    }
    DRoot r;
    r.p = l.p;
    r.cnt = l.cnt;
    r._pad = 0;
    r.row_off = m;
    r.bucket = l.bucket;
    (l.cnt <= DISTINCT_SMALL ? roots_small : roots_tile).push_back(r);
    m += l.cnt;
  }
  *n_out = m;
  if (m > cap) {
    seterr("scan_distinct: output capacity too small (n_out holds the row count)");
    return GEMX_E_CAP;
  }
  const uint64_t n_rs = roots_small.size(), n_rt = roots_tile.size();
  if (n_rs + n_rt > 0xffffffffull) {
    seterr("scan_distinct: too many output buckets");
    return GEMX_E_INVALID;
  }
  if (m) {
    HIP_CHECK(distinct_grow(P.d_roots, P.roots_cap, n_rs + n_rt));
    HIP_CHECK(distinct_grow(P.d_rows, P.rows_cap, m));
    if (n_rs)
      HIP_CHECK(hipMemcpyAsync(P.d_roots, roots_small.data(), sizeof(DRoot) * n_rs,
                               hipMemcpyHostToDevice, s->stream));
    if (n_rt)
      HIP_CHECK(hipMemcpyAsync(P.d_roots + n_rs, roots_tile.data(),
                               sizeof(DRoot) * n_rt, hipMemcpyHostToDevice,
                               s->stream));
    if (s->col_type == GEMX_TYPE_FLOAT)
      distinct_launch_emit<GEMX_TYPE_FLOAT>(s, P, group_all, (uint32_t)n_rs,
                                            (uint32_t)n_rt);
    else
      distinct_launch_emit<GEMX_TYPE_INT>(s, P, group_all, (uint32_t)n_rs,
                                          (uint32_t)n_rt);
    HIP_CHECK(hipGetLastError());
  }
  (void)hipEventRecord(P.ev[2], s->stream);
  if (m)
    HIP_CHECK(hipMemcpyAsync(out_host, P.d_rows, sizeof(gemx_point_row) * m,
                             hipMemcpyDeviceToHost, s->stream));
  HIP_CHECK(hipMemcpyAsync(P.h_err, P.d_err, sizeof(DevErr), hipMemcpyDeviceToHost,
                           s->stream));
  HIP_CHECK(hipStreamSynchronize(s->stream));
  {
    int rc = distinct_dev_error(*P.h_err);
    if (rc != GEMX_OK) {
      *n_out = 0;
      return rc;
    }
  }
  if (stats) {
    float ms_scan = 0, ms_merge = 0, ms_total = 0;
    (void)hipEventElapsedTime(&ms_scan, P.ev[0], P.ev[1]);
    (void)hipEventElapsedTime(&ms_merge, P.ev[1], P.ev[2]);
    (void)hipEventElapsedTime(&ms_total, P.ev[0], P.ev[2]);
    stats->h2d_ms = 0;
    stats->decode_ms = ms_scan;
    stats->merge_ms = ms_merge; /* node levels (host table building between
                                   them included) and the emit */
    stats->total_ms = ms_total;
    stats->points = s->total_rows_scanned;
    stats->compressed_bytes = s->total_compressed_bytes;
    stats->n_rows = m;
  }
  return GEMX_OK;
}

extern "C" int gemx_distinct_stats(gemx_shard *s, uint64_t *candidates,
                                   uint64_t *points, uint32_t *levels) {
  if (!s) {
    seterr("distinct_stats: NULL shard handle");
    return GEMX_E_INVALID;
  }
  const DistinctPlan *p = s->distinct_plan;
  if (candidates) *candidates = p ? p->last_candidates : 0;
  if (points) *points = p ? p->last_points : 0;
  if (levels) *levels = p ? p->last_levels : 0;
  return GEMX_OK;
}
