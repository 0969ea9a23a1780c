/*
 * gemx_topn.hpp — top(field, N) / bottom(field, N) selector scans.
 *
 * Replaces the reference's series-level heap reducers
 * (engine/series_agg_reducer.gen.go:1969-2146, 2327-2600:
 * newTopRoutineImpl / newBottomRoutineImpl over FloatHeapItem /
 * IntegerHeapItem) and the executor-side merge with the same comparators
 * (engine/executor/agg_func.go:44-70). The heap keeps, per window, the N
 * best points under "better value first, earlier time on equal value"
 * (series_agg_func.gen.go:276-326 …CmpByValueTop/Bottom) and emits them
 * time-ascending (…CmpByTimeTop/Bottom). That is a pure function of the
 * window's multiset of points, so it decomposes exactly like Partial:
 * per-segment lanes -> lane-owned per-(segment, window) lists -> merge.
 *
 * Included by gemx_engine.hip (single translation unit) after the scan,
 * merge and host plumbing it builds on.
 *
 * List storage: a compile-time capacity K in registers, every access
 * statically indexed in fully unrolled loops (a runtime-indexed private
 * array would live in scratch). Two capacity classes are instantiated,
 * K = 4 (n <= 4) and K = 16 (n <= GEMX_TOPN_MAX), so small-N queries keep
 * the register budget of the neighbouring streaming kernels.
 */

#define TOPN_GAP_TIME INT64_MIN /* below INFLUX_MIN_TIME: never a point's time */
#define TOPN_GROUP_TPB 128

/* one kept point; v holds the value's bits (double or int64) */
struct TopItem {
  int64_t v;
  int64_t t;
};

/* series chunk of the grouped stage: positions [start, start+count) of the
 * series order array (identity when the order pointer is NULL) */
struct TopChunk {
  uint32_t start, count;
};

/* a is kept in preference to b (…CmpByValueTop/Bottom, operands swapped:
 * the reference's comparator says "a is worse") */
template <int COLTYPE, int SEL>
__device__ __forceinline__ bool top_better(int64_t av, int64_t at, int64_t bv,
                                           int64_t bt) {
  if (COLTYPE == GEMX_TYPE_FLOAT) {
    const double a = d_bits_f(av), b = d_bits_f(bv);
    if (a != b) return SEL == GEMX_SEL_TOP ? (a > b) : (a < b);
    return at < bt;
  }
  if (av != bv) return SEL == GEMX_SEL_TOP ? (av > bv) : (av < bv);
  return at < bt;
}

/* a is emitted before b (…CmpByTimeTop/Bottom) */
template <int COLTYPE, int SEL>
__device__ __forceinline__ bool top_before(int64_t av, int64_t at, int64_t bv,
                                           int64_t bt) {
  if (at != bt) return at < bt;
  if (COLTYPE == GEMX_TYPE_FLOAT) {
    const double a = d_bits_f(av), b = d_bits_f(bv);
    return SEL == GEMX_SEL_TOP ? (a > b) : (a < b);
  }
  return SEL == GEMX_SEL_TOP ? (av > bv) : (av < bv);
}

/* rank-ordered candidate list (best first), capacity K, bound n <= K */
template <int COLTYPE, int SEL, int K>
struct TopList {
  int64_t v[K], t[K];
  int64_t wv, wt; /* worst kept point, valid once cnt == n */
  uint32_t cnt;

  __device__ __forceinline__ void clear() {
    cnt = 0;
    wv = 0;
    wt = 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
      v[j] = 0;
      t[j] = 0;
    }
  }

  /* hot path: a full list rejects with one predicated compare */
  __device__ __forceinline__ bool rejects(uint32_t n, int64_t xv, int64_t xt) const {
    return cnt >= n && !top_better<COLTYPE, SEL>(xv, xt, wv, wt);
  }

  __device__ __forceinline__ void insert(uint32_t n, int64_t xv, int64_t xt) {
    /* the list is rank-sorted, so the kept points x does not beat form a
     * prefix; p is x's rank. p <= n-1: either the list is not full
     * (p <= cnt < n) or x beats the worst (p < cnt == n). */
    uint32_t p = 0;
#pragma unroll
    for (int j = 0; j < K; j++)
      p += (uint32_t)((uint32_t)j < cnt &&
                      !top_better<COLTYPE, SEL>(xv, xt, v[j], t[j]));
#pragma unroll
    for (int j = K - 1; j >= 1; j--) {
      const bool sh = (uint32_t)j > p;
      v[j] = sh ? v[j - 1] : v[j];
      t[j] = sh ? t[j - 1] : t[j];
    }
#pragma unroll
    for (int j = 0; j < K; j++) {
      const bool at = (uint32_t)j == p;
      v[j] = at ? xv : v[j];
      t[j] = at ? xt : t[j];
    }
    if (cnt < n) cnt++;
    if (cnt >= n) {
#pragma unroll
      for (int j = 0; j < K; j++) {
        const bool last = (uint32_t)j == n - 1;
        wv = last ? v[j] : wv;
        wt = last ? t[j] : wt;
      }
    }
  }

  __device__ __forceinline__ void offer(uint32_t n, int64_t xv, int64_t xt) {
    if (rejects(n, xv, xt)) return;
    insert(n, xv, xt);
  }

  /* emission order: odd-even transposition over the valid prefix */
  __device__ __forceinline__ void sort_by_time() {
#pragma unroll
    for (int pass = 0; pass < K; pass++) {
#pragma unroll
      for (int j = (pass & 1); j + 1 < K; j += 2) {
        const bool sw = (uint32_t)(j + 1) < cnt &&
                        top_before<COLTYPE, SEL>(v[j + 1], t[j + 1], v[j], t[j]);
        const int64_t av = v[j], at = t[j];
        v[j] = sw ? v[j + 1] : av;
        t[j] = sw ? t[j + 1] : at;
        v[j + 1] = sw ? av : v[j + 1];
        t[j + 1] = sw ? at : t[j + 1];
      }
    }
  }

  __device__ __forceinline__ void store(TopItem *__restrict__ dst,
                                        uint32_t *__restrict__ cntp) const {
#pragma unroll
    for (int j = 0; j < K; j++)
      if ((uint32_t)j < cnt) {
        TopItem it;
        it.v = v[j];
        it.t = t[j];
        dst[j] = it;
      }
    *cntp = cnt;
  }

  /* n-row output slot: kept points, then gap markers; returns gap rows */
  __device__ __forceinline__ uint32_t emit(gemx_point_row *__restrict__ dst,
                                           uint32_t n, uint64_t sid,
                                           int64_t win_start) const {
#pragma unroll
    for (int j = 0; j < K; j++)
      if ((uint32_t)j < n) {
        gemx_point_row r;
        r.sid = sid;
        r.win_start = win_start;
        r.time = (uint32_t)j < cnt ? t[j] : TOPN_GAP_TIME;
        r.v.i = (uint32_t)j < cnt ? v[j] : 0;
        dst[j] = r;
      }
    return n - cnt;
  }
};

/* One lane per in-range segment; lane-owned per-(segment, window) lists:
 * pcnt[slot] kept points, pitems[slot * n + rank]. No atomics on the data
 * path. FAST = 1: nil-free segments inside the query range, streaming
 * decode (SegStream, gemx_segdecode.hpp). FAST = 0: everything else,
 * decoded into per-lane scratch (SegBuffered, which owns the layout, the
 * bounds / length checks and the error codes); nil rows and rows outside
 * [q_start, q_end] are skipped. */
template <int COLTYPE, int SEL, int FAST, int K>
__global__ void __launch_bounds__(256) k_topn_scan(
    const uint8_t *__restrict__ blob, const uint64_t *__restrict__ arena,
    const GorDesc *__restrict__ gors, const gemx_seg_desc *__restrict__ descs,
    const SegQ *__restrict__ segq, const uint32_t *__restrict__ seg_ids,
    uint32_t nseg_ids, uint32_t *__restrict__ pcnt, TopItem *__restrict__ pitems,
    uint32_t n, int64_t interval, int64_t offset, int64_t q_start, int64_t q_end,
    uint8_t *__restrict__ scratch, uint64_t scratch_per_lane, uint32_t nlanes,
    DevErr *err) {
  uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t stride = FAST ? gridDim.x * blockDim.x : nlanes;
  if (!FAST && gid >= nlanes) return;

  for (uint32_t li = gid; li < nseg_ids; li += stride) {
    uint32_t si = seg_ids[li];
    const gemx_seg_desc d = descs[si];
    const SegQ sq = segq[si];
    if (sq.n_wins == 0) continue; /* segment outside the query range */
    const int rows = (int)d.rows;

    /* clear this lane's slots: a window can hold no usable point (time
     * gaps, nils, NaNs, rows clipped by the range) */
    for (uint32_t k = 0; k < sq.n_wins; k++) pcnt[sq.partial_base + k] = 0;

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
    TopList<COLTYPE, SEL, K> L;
    L.clear();

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
      if (COLTYPE == GEMX_TYPE_FLOAT) {
        const double fv = d_bits_f(xv);
        if (fv != fv) continue; /* NaN never selected */
      }

      if (t >= we_cur || t < ws_cur) {
        if (cur_ord != INT64_MIN) {
          const uint64_t slot = sq.partial_base + (uint64_t)(cur_ord - sq.w_first);
          L.store(pitems + slot * n, pcnt + slot);
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
        L.cnt = 0;
      }
      if (L.rejects(n, xv, t)) continue;
      L.insert(n, xv, t);
    }
    if (cur_ord != INT64_MIN) {
      const uint64_t slot = sq.partial_base + (uint64_t)(cur_ord - sq.w_first);
      L.store(pitems + slot * n, pcnt + slot);
    }
  }
}

/* One lane per (series, window): merge the lists of the series' segments
 * whose span covers the window (the SeriesQ/SegQ walk of
 * merge_series_window), keep the best n, order by time, write the fixed
 * n-row slot. Unused rows carry the gap marker and are counted. */
template <int COLTYPE, int SEL, int K>
__global__ void __launch_bounds__(256) k_topn_merge(
    const SeriesQ *__restrict__ series, uint32_t nseries,
    const SegQ *__restrict__ segq, const uint32_t *__restrict__ pcnt,
    const TopItem *__restrict__ pitems, uint32_t n,
    gemx_point_row *__restrict__ rows, uint64_t total_wins, int64_t interval,
    int64_t offset, int64_t q_start, DevErr *__restrict__ err) {
  uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  for (uint64_t r = gid; r < total_wins; r += gridDim.x * (uint64_t)blockDim.x) {
    uint32_t lo = 0, hi = nseries - 1;
    while (lo < hi) {
      uint32_t mid = (lo + hi + 1) >> 1;
      if (series[mid].out_base <= r) lo = mid;
      else hi = mid - 1;
    }
    const SeriesQ s = series[lo];
    const int64_t w = s.w_min + (int64_t)(r - s.out_base);
    TopList<COLTYPE, SEL, K> L;
    L.clear();
    uint32_t a = s.seg_start, b = s.seg_start + s.seg_count;
    /* first segment with w_first + n_wins > w (spans are time-sorted) */
    uint32_t flo = a, fhi = b;
    while (flo < fhi) {
      uint32_t mid = (flo + fhi) >> 1;
      if (segq[mid].w_first + (int64_t)segq[mid].n_wins > w) fhi = mid;
      else flo = mid + 1;
    }
    for (uint32_t si = flo; si < b && segq[si].w_first <= w; si++) {
      const SegQ q = segq[si];
      if (w < q.w_first || w >= q.w_first + (int64_t)q.n_wins) continue;
      const uint64_t slot = q.partial_base + (uint64_t)(w - q.w_first);
      uint32_t c = pcnt[slot];
      if (c > n) c = n;
      const TopItem *it = pitems + slot * n;
      for (uint32_t j = 0; j < c; j++) {
        const TopItem x = it[j];
        if (L.rejects(n, x.v, x.t)) break; /* rank order: the rest is worse */
        L.insert(n, x.v, x.t);
      }
    }
    L.sort_by_time();
    const uint32_t g = L.emit(rows + r * n, n, s.sid,
                              interval ? win_start_of(w, interval, offset) : q_start);
    if (g)
      __hip_atomic_fetch_add(&err->gaps, (unsigned long long)g, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

/* Grouped stage 1: one block per (window, series chunk). Each thread folds
 * a deterministic stride of the chunk's series' winner rows (the merge
 * kernel's output slots) into its own list; an LDS tree then merges the
 * lists pairwise. The best n of the union are a subset of the per-series
 * winners. `order` maps chunk positions to series (NULL = identity), so a
 * hash GROUP BY tag can reuse the kernel with a sid->group permutation. */
template <int COLTYPE, int SEL, int K>
__global__ void __launch_bounds__(TOPN_GROUP_TPB) k_topn_group_p1(
    const SeriesQ *__restrict__ series, const uint32_t *__restrict__ order,
    const TopChunk *__restrict__ chunks, uint32_t nchunks,
    const gemx_point_row *__restrict__ rows, uint32_t n, int64_t W0,
    uint32_t *__restrict__ gcnt, TopItem *__restrict__ gitems) {
  __shared__ int64_t sv[K][TOPN_GROUP_TPB];
  __shared__ int64_t st[K][TOPN_GROUP_TPB];
  __shared__ uint32_t sc[TOPN_GROUP_TPB];
  const uint32_t tid = threadIdx.x;
  const uint64_t gw = blockIdx.x;
  const int64_t w = W0 + (int64_t)gw;
  const TopChunk ch = chunks[blockIdx.y];
  TopList<COLTYPE, SEL, K> L;
  L.clear();
  for (uint32_t i = tid; i < ch.count; i += TOPN_GROUP_TPB) {
    const uint32_t g = order ? order[ch.start + i] : ch.start + i;
    const SeriesQ s = series[g];
    if (w < s.w_min || w >= s.w_min + (int64_t)s.n_wins) continue;
    const gemx_point_row *src = rows + (s.out_base + (uint64_t)(w - s.w_min)) * n;
    for (uint32_t j = 0; j < n; j++) {
      const gemx_point_row x = src[j];
      if (x.time == TOPN_GAP_TIME) break;
      L.offer(n, x.v.i, x.time);
    }
  }
#pragma unroll
  for (int j = 0; j < K; j++) {
    sv[j][tid] = L.v[j];
    st[j][tid] = L.t[j];
  }
  sc[tid] = L.cnt;
  __syncthreads();
  for (uint32_t stride = TOPN_GROUP_TPB / 2; stride >= 1; stride >>= 1) {
    if (tid < stride) {
      const uint32_t pc = sc[tid + stride];
#pragma unroll
      for (int j = 0; j < K; j++)
        if ((uint32_t)j < pc) L.offer(n, sv[j][tid + stride], st[j][tid + stride]);
#pragma unroll
      for (int j = 0; j < K; j++) {
        sv[j][tid] = L.v[j];
        st[j][tid] = L.t[j];
      }
      sc[tid] = L.cnt;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const uint64_t slot = gw * nchunks + blockIdx.y;
    L.store(gitems + slot * n, gcnt + slot);
  }
}

/* Grouped stage 2: one lane per window merges the chunk lists, orders by
 * time and emits rows with sid = 0. */
template <int COLTYPE, int SEL, int K>
__global__ void __launch_bounds__(256) k_topn_group_p2(
    const uint32_t *__restrict__ gcnt, const TopItem *__restrict__ gitems,
    uint32_t nchunks, uint32_t n, gemx_point_row *__restrict__ grows,
    uint64_t n_gwins, int64_t W0, int64_t interval, int64_t offset,
    int64_t q_start, DevErr *__restrict__ err) {
  uint64_t gid = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  for (uint64_t gw = gid; gw < n_gwins; gw += gridDim.x * (uint64_t)blockDim.x) {
    TopList<COLTYPE, SEL, K> L;
    L.clear();
    for (uint32_t c = 0; c < nchunks; c++) {
      const uint64_t slot = gw * nchunks + c;
      uint32_t pc = gcnt[slot];
      if (pc > n) pc = n;
      const TopItem *it = gitems + slot * n;
      for (uint32_t j = 0; j < pc; j++) {
        const TopItem x = it[j];
        if (L.rejects(n, x.v, x.t)) break;
        L.insert(n, x.v, x.t);
      }
    }
    L.sort_by_time();
    const int64_t w = W0 + (int64_t)gw;
    const uint32_t g = L.emit(grows + gw * n, n, 0,
                              interval ? win_start_of(w, interval, offset) : q_start);
    if (g)
      __hip_atomic_fetch_add(&err->gaps, (unsigned long long)g, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

/* ---------------- host ---------------- */

/* Device state of the selector queries, separate from the aggregate
 * QueryPlan (as RatePlan is): gemx_scan_topn never rebuilds or frees a
 * buffer that an in-flight begin/finish aggregate query uses. */
struct TopPlan {
  bool valid = false;
  int64_t start = 0, end = 0, interval = 0, offset = 0;
  uint32_t n = 0;
  std::vector<SegQ> segq;
  std::vector<SeriesQ> sq;
  uint64_t slots = 0, total_wins = 0, n_gwins = 0;
  int64_t W0 = 0;
  SegQ *d_segq = nullptr;
  SeriesQ *d_sq = nullptr;
  uint32_t *d_pcnt = nullptr;
  TopItem *d_pitems = nullptr;
  gemx_point_row *d_rows = nullptr, *d_grows = nullptr;
  uint32_t *d_fast_q = nullptr, *d_gen_q = nullptr;
  uint32_t n_fast_q = 0, n_gen_q = 0, gen_lanes = 0;
  uint8_t *d_scratch = nullptr;
  TopChunk *d_chunks = nullptr;
  uint32_t nchunks = 0;
  uint32_t *d_gcnt = nullptr;
  TopItem *d_gitems = nullptr;
  DevErr *d_err = nullptr, *h_err = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
};

static void free_top_plan_bufs(TopPlan &p) {
  if (p.d_segq) (void)hipFree(p.d_segq);
  if (p.d_sq) (void)hipFree(p.d_sq);
  if (p.d_pcnt) (void)hipFree(p.d_pcnt);
  if (p.d_pitems) (void)hipFree(p.d_pitems);
  if (p.d_rows) (void)hipFree(p.d_rows);
  if (p.d_grows) (void)hipFree(p.d_grows);
  if (p.d_fast_q) (void)hipFree(p.d_fast_q);
  if (p.d_gen_q) (void)hipFree(p.d_gen_q);
  if (p.d_scratch) (void)hipFree(p.d_scratch);
  if (p.d_chunks) (void)hipFree(p.d_chunks);
  if (p.d_gcnt) (void)hipFree(p.d_gcnt);
  if (p.d_gitems) (void)hipFree(p.d_gitems);
  if (p.d_err) (void)hipFree(p.d_err);
  if (p.h_err) (void)hipHostFree(p.h_err);
  for (int e = 0; e < 4; e++)
    if (p.ev[e]) (void)hipEventDestroy(p.ev[e]);
  p = TopPlan();
}

static void free_top_plan(gemx_shard *s) {
  if (!s->top_plan) return;
  free_top_plan_bufs(*s->top_plan);
  delete s->top_plan;
  s->top_plan = nullptr;
}

/* window spans, output ranges, launch lists and buffers for one
 * (start, end, interval, offset, n) */
static int topn_build_plan(gemx_shard *s, TopPlan &P, int64_t start_time,
                           int64_t end_time, int64_t interval, int64_t offset,
                           uint32_t n, uint64_t scratch_per_lane) {
  const uint64_t nsegs = s->nsegs;
  free_top_plan_bufs(P);
  P.segq.resize(nsegs);
  P.sq.resize(s->series_ranges.size());
  std::vector<uint32_t> fast_q, gen_q;
  std::vector<char> is_gen(nsegs, 0);
  for (auto id : s->general_ids) is_gen[id] = 1;
  for (size_t g = 0; g < s->series_ranges.size(); g++) {
    auto &r = s->series_ranges[g];
    int64_t wmin = INT64_MAX, wmax = INT64_MIN;
    /* running max of (w_first + n_wins): the merge's binary search needs
     * it non-decreasing, so out-of-range segments get a clamped sentinel
     * (the aggregate plan's invariant) */
    int64_t run = INT64_MIN;
    for (uint32_t i = r.start; i < r.start + r.count; i++) {
      const gemx_seg_desc &d = s->h_descs[i];
      P.segq[i].partial_base = P.slots;
      P.segq[i].series_idx = (uint32_t)g;
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
      wmin = std::min(wmin, w0);
      wmax = std::max(wmax, w1);
      const bool clip = (d.min_time < start_time || d.max_time > end_time);
      if (clip || is_gen[i]) gen_q.push_back(i);
      else fast_q.push_back(i);
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
  /* arena-mode gorilla lanes first, in arena slot order: in descriptor
   * order the interleaved arena does not coalesce */
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
  /* chunk table of the grouped stage: aim for >= 2048 blocks in all,
   * at least one series per thread of a block */
  std::vector<TopChunk> chunks;
  {
    uint64_t nser = P.sq.size() ? P.sq.size() : 1;
    uint64_t want = P.n_gwins ? (2048 + P.n_gwins - 1) / P.n_gwins : 1;
    uint64_t per_chunk = (nser + want - 1) / want;
    if (per_chunk < TOPN_GROUP_TPB) per_chunk = TOPN_GROUP_TPB;
    if (per_chunk > nser) per_chunk = nser;
    for (uint64_t c0 = 0; c0 < P.sq.size(); c0 += per_chunk) {
      TopChunk c;
      c.start = (uint32_t)c0;
      c.count = (uint32_t)std::min<uint64_t>(per_chunk, P.sq.size() - c0);
      chunks.push_back(c);
    }
    P.nchunks = (uint32_t)chunks.size();
  }
#define TOPN_ALLOC(PTR, TYPE, COUNT)                                           \
  HIP_CHECK(hipMalloc(&PTR, sizeof(TYPE) * ((COUNT) ? (COUNT) : 1)))
#define TOPN_UPLOAD(PTR, TYPE, VEC)                                            \
  do {                                                                         \
    TOPN_ALLOC(PTR, TYPE, (VEC).size());                                       \
    if (!(VEC).empty())                                                        \
      HIP_CHECK(hipMemcpyAsync(PTR, (VEC).data(), sizeof(TYPE) * (VEC).size(), \
                               hipMemcpyHostToDevice, s->stream));             \
  } while (0)
  TOPN_UPLOAD(P.d_segq, SegQ, P.segq);
  TOPN_UPLOAD(P.d_sq, SeriesQ, P.sq);
  TOPN_UPLOAD(P.d_fast_q, uint32_t, fast_q);
  TOPN_UPLOAD(P.d_gen_q, uint32_t, gen_q);
  TOPN_UPLOAD(P.d_chunks, TopChunk, chunks);
  P.n_fast_q = (uint32_t)fast_q.size();
  P.n_gen_q = (uint32_t)gen_q.size();
  TOPN_ALLOC(P.d_pcnt, uint32_t, P.slots);
  TOPN_ALLOC(P.d_pitems, TopItem, P.slots * n);
  TOPN_ALLOC(P.d_rows, gemx_point_row, P.total_wins * n);
  TOPN_ALLOC(P.d_grows, gemx_point_row, P.n_gwins * n);
  TOPN_ALLOC(P.d_gcnt, uint32_t, P.n_gwins * P.nchunks);
  TOPN_ALLOC(P.d_gitems, TopItem, P.n_gwins * P.nchunks * n);
  if (P.n_gen_q) {
    P.gen_lanes = std::min<uint32_t>(P.n_gen_q, 16384);
    HIP_CHECK(hipMalloc(&P.d_scratch, scratch_per_lane * P.gen_lanes));
  }
  HIP_CHECK(hipMalloc(&P.d_err, sizeof(DevErr)));
  HIP_CHECK(hipHostMalloc(&P.h_err, sizeof(DevErr)));
  for (int e = 0; e < 4; e++) HIP_CHECK(hipEventCreate(&P.ev[e]));
#undef TOPN_UPLOAD
#undef TOPN_ALLOC
  /* the launch lists and chunk table are locals */
  HIP_CHECK(hipStreamSynchronize(s->stream));
  P.start = start_time;
  P.end = end_time;
  P.interval = interval;
  P.offset = offset;
  P.n = n;
  P.valid = true;
  return GEMX_OK;
}

template <int COLTYPE, int SEL, int K>
static void topn_launch(gemx_shard *s, TopPlan &P, int group_all) {
  const int TPB = 256;
  const uint64_t scratch_per_lane = seg_scratch_bytes(SEG_SPARE_SCAN);
  (void)hipEventRecord(P.ev[0], s->stream);
  if (P.n_fast_q) {
    uint32_t blocks = std::min<uint32_t>((P.n_fast_q + TPB - 1) / TPB, 65535);
    hipLaunchKernelGGL((k_topn_scan<COLTYPE, SEL, 1, K>), dim3(blocks), dim3(TPB),
                       0, s->stream, s->d_blob, s->d_arena, s->d_gor, s->d_descs,
                       P.d_segq, P.d_fast_q, P.n_fast_q, P.d_pcnt, P.d_pitems, P.n,
                       P.interval, P.offset, P.start, P.end, nullptr, 0, 0, P.d_err);
  }
  if (P.n_gen_q) {
    uint32_t blocks = (P.gen_lanes + TPB - 1) / TPB;
    hipLaunchKernelGGL((k_topn_scan<COLTYPE, SEL, 0, K>), dim3(blocks), dim3(TPB),
                       0, s->stream, s->d_blob, s->d_arena, s->d_gor, s->d_descs,
                       P.d_segq, P.d_gen_q, P.n_gen_q, P.d_pcnt, P.d_pitems, P.n,
                       P.interval, P.offset, P.start, P.end, P.d_scratch,
                       scratch_per_lane, P.gen_lanes, P.d_err);
  }
  (void)hipEventRecord(P.ev[1], s->stream);
  if (P.total_wins) {
    uint32_t blocks =
        (uint32_t)std::min<uint64_t>((P.total_wins + TPB - 1) / TPB, 65535);
    hipLaunchKernelGGL((k_topn_merge<COLTYPE, SEL, K>), dim3(blocks), dim3(TPB), 0,
                       s->stream, P.d_sq, (uint32_t)P.sq.size(), P.d_segq, P.d_pcnt,
                       P.d_pitems, P.n, P.d_rows, P.total_wins, P.interval, P.offset,
                       P.start, P.d_err);
  }
  (void)hipEventRecord(P.ev[2], s->stream);
  if (group_all && P.n_gwins) {
    /* the per-series gap count is not part of the grouped result */
    (void)hipMemsetAsync(&P.d_err->gaps, 0, sizeof(P.d_err->gaps), s->stream);
    hipLaunchKernelGGL((k_topn_group_p1<COLTYPE, SEL, K>),
                       dim3((uint32_t)P.n_gwins, P.nchunks), dim3(TOPN_GROUP_TPB), 0,
                       s->stream, P.d_sq, (const uint32_t *)nullptr, P.d_chunks,
                       P.nchunks, P.d_rows, P.n, P.W0, P.d_gcnt, P.d_gitems);
    uint32_t blocks =
        (uint32_t)std::min<uint64_t>((P.n_gwins + TPB - 1) / TPB, 65535);
    hipLaunchKernelGGL((k_topn_group_p2<COLTYPE, SEL, K>), dim3(blocks), dim3(TPB), 0,
                       s->stream, P.d_gcnt, P.d_gitems, P.nchunks, P.n, P.d_grows,
                       P.n_gwins, P.W0, P.interval, P.offset, P.start, P.d_err);
  }
  (void)hipEventRecord(P.ev[3], s->stream);
}

extern "C" int gemx_scan_topn(gemx_shard *s, int64_t start_time, int64_t end_time,
                              int64_t interval, int64_t offset, int group_all,
                              int sel, uint32_t n, gemx_point_row *out_host,
                              uint64_t cap, uint64_t *n_out,
                              gemx_query_stats *stats) {
  if (!s) {
    seterr("scan_topn: NULL shard handle");
    return GEMX_E_INVALID;
  }
  if (n == 0 || n > GEMX_TOPN_MAX) {
    seterr("scan_topn: n must be in 1..GEMX_TOPN_MAX (16)");
    return GEMX_E_INVALID;
  }
  if (sel != GEMX_SEL_TOP && sel != GEMX_SEL_BOTTOM) {
    seterr("scan_topn: sel must be GEMX_SEL_TOP (0) or GEMX_SEL_BOTTOM (1)");
    return GEMX_E_INVALID;
  }
  if (s->col_type != GEMX_TYPE_FLOAT && s->col_type != GEMX_TYPE_INT) {
    seterr("scan_topn: top/bottom need a float or integer column "
           "(no boolean reducer in the reference)");
    return GEMX_E_INVALID;
  }
  if (interval < 0 || !n_out || (!out_host && cap)) {
    seterr("scan_topn: bad arguments");
    return GEMX_E_INVALID;
  }
  if (interval > 0 && s->nsegs) {
    /* the part of the query range that holds data bounds the window count */
    const double lo = (double)std::max(start_time, s->shard_min_t);
    const double hi = (double)std::min(end_time, s->shard_max_t);
    if (hi > lo && (hi - lo) / (double)interval > 1e9) {
      seterr("scan_topn: more than 1e9 windows in the query range");
      return GEMX_E_INVALID;
    }
  }
  HIP_CHECK(hipSetDevice(s->device));
  const uint64_t scratch_per_lane = seg_scratch_bytes(SEG_SPARE_SCAN);
  if (!s->top_plan) s->top_plan = new TopPlan();
  TopPlan &P = *s->top_plan;
  if (!P.valid || P.start != start_time || P.end != end_time ||
      P.interval != interval || P.offset != offset || P.n != n) {
    int rc = topn_build_plan(s, P, start_time, end_time, interval, offset, n,
                             scratch_per_lane);
    if (rc != GEMX_OK) {
      free_top_plan_bufs(P);
      return rc;
    }
  }
  if (group_all && P.n_gwins > 0x7fffffffull) {
    seterr("scan_topn: window count too large");
    return GEMX_E_INVALID;
  }
  HIP_CHECK(hipMemsetAsync(P.d_err, 0, sizeof(DevErr), s->stream));
  const bool fl = (s->col_type == GEMX_TYPE_FLOAT);
  const bool top = (sel == GEMX_SEL_TOP);
#define TOPN_GO(CT, SL)                                                        \
  do {                                                                         \
    if (n <= 4) topn_launch<CT, SL, 4>(s, P, group_all);                       \
    else topn_launch<CT, SL, 16>(s, P, group_all);                             \
  } while (0)
  if (fl && top) TOPN_GO(GEMX_TYPE_FLOAT, GEMX_SEL_TOP);
  else if (fl) TOPN_GO(GEMX_TYPE_FLOAT, GEMX_SEL_BOTTOM);
  else if (top) TOPN_GO(GEMX_TYPE_INT, GEMX_SEL_TOP);
  else TOPN_GO(GEMX_TYPE_INT, GEMX_SEL_BOTTOM);
#undef TOPN_GO
  HIP_CHECK(hipGetLastError());

  const uint64_t bound = (group_all ? P.n_gwins : P.total_wins) * n;
  const gemx_point_row *d_src = group_all ? P.d_grows : P.d_rows;
  HIP_CHECK(hipMemcpyAsync(P.h_err, P.d_err, sizeof(DevErr), hipMemcpyDeviceToHost,
                           s->stream));
  /* rows land in the caller's buffer when it holds the whole slot array;
   * otherwise in a staging copy that is compacted into it */
  std::vector<gemx_point_row> stage;
  gemx_point_row *dst = out_host;
  if (cap < bound) {
    stage.resize(bound);
    dst = stage.data();
  }
  if (bound)
    HIP_CHECK(hipMemcpyAsync(dst, d_src, sizeof(gemx_point_row) * bound,
                             hipMemcpyDeviceToHost, s->stream));
  HIP_CHECK(hipStreamSynchronize(s->stream));
  const DevErr herr = *P.h_err;
  if (herr.code != 0) {
    seterr(herr.code == GEMX_E_UNSUPPORTED ? "unsupported codec on device"
           : herr.code == GEMX_E_INVALID
               ? "segment descriptor inconsistent with its data"
               : "segment decode failed on device");
    return herr.code;
  }
  uint64_t m = 0;
  if (dst == out_host) {
    if (herr.gaps == 0) {
      m = bound;
    } else { /* in-place compaction, only when the kernels wrote gap rows */
      for (uint64_t i = 0; i < bound; i++) {
        if (dst[i].time == TOPN_GAP_TIME) continue;
        if (m != i) out_host[m] = dst[i];
        m++;
      }
    }
  } else {
    for (uint64_t i = 0; i < bound; i++) m += (dst[i].time != TOPN_GAP_TIME);
    if (m > cap) {
      seterr("scan_topn: output capacity too small");
      return GEMX_E_CAP;
    }
    m = 0;
    for (uint64_t i = 0; i < bound; i++)
      if (dst[i].time != TOPN_GAP_TIME) out_host[m++] = dst[i];
  }
  *n_out = m;
  if (stats) {
    float ms_scan = 0, ms_merge = 0, ms_total = 0;
    (void)hipEventElapsedTime(&ms_scan, P.ev[0], P.ev[1]);
    (void)hipEventElapsedTime(&ms_merge, P.ev[1], P.ev[3]);
    (void)hipEventElapsedTime(&ms_total, P.ev[0], P.ev[3]);
    stats->h2d_ms = 0;
    stats->decode_ms = ms_scan;
    stats->merge_ms = ms_merge; /* per-series merge + grouped stages */
    stats->total_ms = ms_total;
    stats->points = s->total_rows_scanned;
    stats->compressed_bytes = s->total_compressed_bytes;
    stats->n_rows = m;
  }
  return GEMX_OK;
}

/* point rows -> record.ColVal wire layout (the cgo cursor's record
 * assembly for top/bottom; appendCurrItem emits one dense value and the
 * point's own time per kept point) */
extern "C" int gemx_rec_from_points(const gemx_point_row *rows, uint64_t n_rows,
                                    int col_type, void *val_buf, uint8_t *bitmap,
                                    int64_t *time_out, gemx_colval *col_out) {
  if ((!rows && n_rows) || !val_buf || !bitmap || !time_out || !col_out) {
    seterr("rec_from_points: bad arguments");
    return GEMX_E_INVALID;
  }
  if (col_type != GEMX_TYPE_FLOAT && col_type != GEMX_TYPE_INT) {
    seterr("rec_from_points: col_type must be float or integer");
    return GEMX_E_INVALID;
  }
  if (n_rows > 0x7fffffffull) {
    seterr("rec_from_points: too many rows for one record");
    return GEMX_E_INVALID;
  }
  const uint64_t bm_bytes = (n_rows + 7) / 8;
  memset(bitmap, 0, bm_bytes);
  gemx_val *dst = (gemx_val *)val_buf;
  for (uint64_t r = 0; r < n_rows; r++) {
    dst[r] = rows[r].v;
    time_out[r] = rows[r].time;
    bitmap[r >> 3] |= (uint8_t)(1u << (r & 7));
  }
  col_out->val = val_buf;
  col_out->bitmap = bitmap;
  col_out->bitmap_offset = 0;
  col_out->len = (int32_t)n_rows;
  col_out->nil_count = 0;
  return GEMX_OK;
}
