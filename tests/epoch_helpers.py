"""Production-like time axes, an exact scan-aggregate reference and the
PromQL numpy restatements shared by test_oracle_epoch.py (CPU) and
test_gpu_epoch.py (GPU).

Every other test builds its data within about +-1000 s of time zero, on
whole seconds, 1 s apart. Real TSSP data sits near 1.7e18 ns (above 2^53)
with a nanosecond remainder and sub-second sampling, so the axes here are a
base (EPOCH, FAR) plus a spacing, each with intervals chosen so that 300
rows give 5-40 windows.

ref_scan is written from the query semantics alone: times and window
starts are Python int, float sums math.fsum, int sums Python int. It calls
neither the oracle nor the engine.
"""

import functools
import math

import numpy as np

S = 10**9
EPOCH = 1_700_000_000 * S + 123_456_789    # production-like, odd remainder
FAR = 4_102_444_800 * S + 999_999_999      # year 2100, still below 2**62
BASES = {"EPOCH": EPOCH, "FAR": FAR}

# spacing -> [(interval, offset), ...]
QUERIES = {
    "1s": [(60 * S, 0), (60 * S, 13 * 10**6 + 1), (7 * S + 1, 0)],
    "100ms": [(S, 0), (S, S // 3)],
    "1ms": [(10**7, 0), (3 * 10**6 + 1, 0)],
    "7ns": [(100, 0), (100, 37)],
    "jit_ns": [(60 * S, 0)],
    "jit_ms": [(60 * S, S // 2)],
    "dt0": [(60 * S, 0)],
}
STEP = {"1s": S, "100ms": 10**8, "1ms": 10**6, "7ns": 7}
REGULAR = tuple(STEP)
# (base name, spacing): EPOCH runs every spacing, FAR three of them
AXES = [("EPOCH", k) for k in QUERIES] + [("FAR", k)
                                          for k in ("1s", "1ms", "jit_ns")]
# the axes every route has to reach
CORE_AXES = [("EPOCH", "1s"), ("EPOCH", "100ms"), ("EPOCH", "7ns"),
             ("FAR", "1s")]

N_SERIES = 70       # one full 64-lane wave plus a partial one
ROWS0 = 300         # + sid % 7 rows per series
QUIET_ROWS = 64     # see values(): rows with short gorilla records


def axis_id(axis):
    return f"{axis[0]}-{axis[1]}"


def series_rows(sid):
    return ROWS0 + sid % 7


def times_of(axis, sid, rows):
    """int64 times of one series. Regular spacings are the same grid for
    every series (the shape aligned waves need); the jittered ones differ
    per series; dt0 puts every row of a series on one timestamp."""
    base = BASES[axis[0]]
    kind = axis[1]
    if kind in STEP:
        return base + np.arange(rows, dtype=np.int64) * STEP[kind]
    if kind == "dt0":
        return np.full(rows, base + sid * 11 * S, dtype=np.int64)
    rng = np.random.default_rng(9000 + sid)
    if kind == "jit_ns":   # simple8b time codec with scale 1
        return base + np.cumsum(rng.integers(1, 2 * S, rows)).astype(np.int64)
    assert kind == "jit_ms"  # simple8b x 10^6
    return base + np.cumsum(rng.integers(1, 4000, rows)).astype(np.int64) * 10**6


def values(kind, rng, rows, salt=0):
    """One series' values. `walk` starts with QUIET_ROWS rows that cycle
    through three neighbouring integers: their gorilla records are a few
    bits, so with seg_rows 64 or 65 the first segment of every series is
    shorter than every other segment and those segments fill the first
    launch wave on their own, and with seg_rows 257 they are longer than
    the tails and fill the last one (waves are cut from the launch list in
    stream-length order, and only a wave of same-shaped segments folds).
    `salt` differs per series."""
    if kind == "walk":
        q = min(QUIET_ROWS, rows)
        quiet = 4096.0 + salt + (np.arange(q) * 7 + salt) % 3
        rest = np.round(np.cumsum(rng.normal(0, 1, rows - q)) * 128) / 128
        return np.concatenate([quiet, rest]) + 0.0
    if kind == "rle":
        n = rows // 150 + 1
        return np.repeat(np.round(rng.normal(0, 10, n), 1), 150)[:rows] + 0.0
    if kind == "const":
        return np.full(rows, 3.25)
    if kind == "raw":      # random mantissae: uncompressed blocks
        return rng.random(rows) * 1e6 + rng.random(rows)
    if kind == "counter":  # monotone, for the rate family
        return np.cumsum(np.abs(rng.normal(1, 0.3, rows)))
    if kind == "steps":    # repeats and decreases, for changes/resets
        return rng.integers(0, 4, rows).astype(np.float64)
    if kind == "int":
        return rng.integers(0, 1000, rows).astype(np.int64)
    assert kind == "bool"
    return rng.integers(0, 2, rows).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def make_points(axis, kind, nil_frac=0.0, n_series=N_SERIES):
    """{sid: (times, values, valid)}, sids ascending from 1. Read-only."""
    pts = {}
    for sid in range(1, n_series + 1):
        rows = series_rows(sid)
        rng = np.random.default_rng(7000 + sid)
        t = times_of(axis, sid, rows)
        v = values(kind, rng, rows, sid)
        valid = (rng.random(rows) >= nil_frac) if nil_frac else np.ones(
            rows, dtype=bool)
        for a in (t, v, valid):
            a.setflags(write=False)
        pts[sid] = (t, v, valid)
    return pts


def flat(pts):
    """(sids, times, values, valid uint8) in the writer's row order."""
    sids = np.concatenate([np.full(len(t), s, dtype=np.uint64)
                           for s, (t, _, _) in pts.items()])
    times = np.concatenate([t for t, _, _ in pts.values()])
    vals = np.concatenate([v for _, v, _ in pts.values()])
    valid = np.concatenate([x for _, _, x in pts.values()]).astype(np.uint8)
    return sids, times, vals, valid


def col_type_of(vals):
    k = np.asarray(vals).dtype
    return 5 if k == np.uint8 else (1 if k.kind in "iu" else 3)


def writer_shard(pts, seg_rows):
    """Shard through the engine's own writer, which picks the codecs.
    Returns (blob, descs, col_type); nil-free points pass no bitmap."""
    import opengemini_amd as gx

    sids, times, vals, valid = flat(pts)
    ct = col_type_of(vals)
    blob, descs = gx.encode_shard(ct, sids, times, vals,
                                  None if valid.all() else valid, seg_rows)
    return blob, np.ascontiguousarray(descs), ct


def clip_range(pts):
    """A [start, end] at nanosecond granularity that cuts inside segments:
    one past a row's time and one before another's (on dt0, where a
    series has one timestamp, one past series 5's and one before series
    60's)."""
    t = pts[1][0]
    if t[0] == t[-1]:
        return int(pts[5][0][0]) + 1, int(pts[60][0][0]) - 1
    return int(t[37]) + 1, int(t[230]) - 1


def full_range(axis):
    return BASES[axis[0]] - 10**15, 2**62


# ------------------------------------------------------------ the reference

REF_DTYPE_F = np.dtype([
    ("sid", "<u8"), ("win_start", "<i8"), ("first_row_time", "<i8"),
    ("count", "<i8"), ("sum", "<f8"), ("min", "<f8"), ("min_time", "<i8"),
    ("max", "<f8"), ("max_time", "<i8"), ("first", "<f8"),
    ("first_time", "<i8"), ("last", "<f8"), ("last_time", "<i8"),
    ("isnil", "u1")])
REF_DTYPE_I = np.dtype([(n, "<i8" if n in ("sum", "min", "max", "first",
                                           "last") else REF_DTYPE_F[n])
                        for n in REF_DTYPE_F.names])
VALUE_FIELDS = ("min", "max", "first", "last")


def window_starts(times, interval, offset):
    """Floored window starts, in Python int arithmetic."""
    return np.array([(t - offset) // interval * interval + offset
                     for t in times.tolist()], dtype=np.int64)


def _first_where(mask, starts):
    """Per run (starts: reduceat boundaries), the first index whose mask
    is set."""
    idx = np.where(mask, np.arange(len(mask)), len(mask))
    return np.minimum.reduceat(idx, starts)


def _exact_sum(v):
    if v.dtype.kind == "f":
        return math.fsum(v.tolist())
    return sum(v.tolist())


def _series_ref(sid, t, v, valid, start, end, interval, offset, seg_rows, dt):
    seg = np.arange(len(t)) // seg_rows     # the writer cuts every seg_rows
    m = (t >= start) & (t <= end)
    t, v, valid, seg = t[m], v[m], valid[m], seg[m]
    if len(t) == 0:
        return np.zeros(0, dtype=dt)
    ws = window_starts(t, interval, offset)
    # rows are time-ordered, so a window is one run of rows
    b = np.flatnonzero(np.diff(ws) != 0) + 1
    starts = np.concatenate([[0], b])
    out = np.zeros(len(starts), dtype=dt)
    out["sid"] = sid
    out["win_start"] = ws[starts]
    out["count"] = np.add.reduceat(valid.astype(np.int64), starts)
    out["isnil"] = out["count"] == 0
    # first_row_time: every contributing segment overwrites it with the
    # time of its first row in the window, so the last segment's stays
    rb = np.flatnonzero((np.diff(ws) != 0) | (np.diff(seg) != 0)) + 1
    rstarts = np.concatenate([[0], rb])
    last_run = np.searchsorted(ws[rstarts], ws[starts], side="right") - 1
    out["first_row_time"] = t[rstarts[last_run]]
    win = np.repeat(np.arange(len(starts)), np.diff(np.append(starts, len(t))))
    tv, vv, wv = t[valid], v[valid], win[valid]
    if len(tv) == 0:
        return out
    have = np.flatnonzero(out["count"] > 0)
    vs = np.searchsorted(wv, have)          # run starts in the valid rows
    ve = np.append(vs[1:], len(tv))
    run = np.repeat(np.arange(len(vs)), ve - vs)
    mn = np.minimum.reduceat(vv, vs)
    mx = np.maximum.reduceat(vv, vs)
    imn = _first_where(vv == mn[run], vs)   # first occurrence wins
    imx = _first_where(vv == mx[run], vs)
    out["min"][have], out["min_time"][have] = vv[imn], tv[imn]
    out["max"][have], out["max_time"][have] = vv[imx], tv[imx]
    out["first"][have], out["first_time"][have] = vv[vs], tv[vs]
    out["last"][have], out["last_time"][have] = vv[ve - 1], tv[ve - 1]
    out["sum"][have] = [_exact_sum(vv[a:e]) for a, e in zip(vs, ve)]
    return out


def _group_ref(per, pts, start, end, interval, offset, dt):
    """Merge per-series rows in ascending sid order: a smaller (larger)
    value wins min (max), then the earlier time, then the lower sid; first
    is the earliest time, last the latest, ties to the lower sid. Sums are
    taken over the points again, not over per-series sums."""
    if len(per) == 0:
        return np.zeros(0, dtype=dt)
    wins, inv = np.unique(per["win_start"], return_inverse=True)
    out = np.zeros(len(wins), dtype=dt)
    out["win_start"] = wins
    out["first_row_time"] = wins
    np.add.at(out["count"], inv, per["count"])
    out["isnil"] = out["count"] == 0
    live = np.flatnonzero(per["count"] > 0)
    r, w = per[live], inv[live]
    pos = np.arange(len(r))                 # rows are in ascending sid order
    for f, keys in (("min", (pos, r["min_time"], r["min"], w)),
                    ("max", (pos, r["max_time"], -r["max"], w)),
                    ("first", (pos, r["first_time"], w)),
                    ("last", (pos, -r["last_time"], w))):
        o = np.lexsort(keys)
        head = o[np.concatenate([[True], w[o][1:] != w[o][:-1]])]
        out[f][w[head]] = r[f][head]
        out[f + "_time"][w[head]] = r[f + "_time"][head]
    acc = {int(x): [] for x in wins}
    for sid in sorted(pts):
        t, v, valid = pts[sid]
        m = valid & (t >= start) & (t <= end)
        if not m.any():
            continue
        ws = window_starts(t[m], interval, offset)
        vm = v[m]
        cut = np.flatnonzero(np.diff(ws) != 0) + 1
        for a, e in zip(np.concatenate([[0], cut]), np.append(cut, len(ws))):
            acc[int(ws[a])].extend(vm[a:e].tolist())
    for k, x in enumerate(wins):
        vals = acc[int(x)]
        if vals:
            out["sum"][k] = (math.fsum(vals) if isinstance(vals[0], float)
                             else sum(vals))
    return out


def ref_scan(pts, start, end, interval, offset, grouped, seg_rows=10**9):
    """The gemx_agg_row content of scan_agg over {sid: (times, values,
    valid)}: count, sum, min/max/first/last with their times, the nil flag
    (one for all five: a window has values or it has none) and
    first_row_time, which depends on where the writer cut the segments
    (seg_rows). Rows in (sid, window) order; grouped rows carry sid 0 and
    first_row_time = win_start."""
    assert interval > 0
    v0 = next(iter(pts.values()))[1]
    dt = REF_DTYPE_F if v0.dtype.kind == "f" else REF_DTYPE_I
    conv = (lambda v: v) if v0.dtype.kind == "f" else (
        lambda v: v.astype(np.int64))
    cp = {s: (t, conv(v), x) for s, (t, v, x) in pts.items()}
    per = [_series_ref(sid, *cp[sid], start, end, interval, offset, seg_rows,
                       dt) for sid in sorted(cp)]
    per = np.concatenate(per) if per else np.zeros(0, dtype=dt)
    if not grouped:
        return per
    return _group_ref(per, cp, start, end, interval, offset, dt)


def assert_matches_ref(rows, ref, grouped=False, with_sum=True,
                       row_time=True, ctx=""):
    """Engine or oracle rows (AGG_ROW_DTYPE) against ref_scan: everything
    bit-exact but float sums, which hold the project's contract
    1e-9 * max(1, |ref|). Value times are compared where the aggregate is
    not nil. with_sum=False is for boolean columns, which have no sum;
    row_time=False leaves first_row_time out (predicate scans, whose
    reference sees the passing rows only, not the segment cuts)."""
    assert len(rows) == len(ref), (ctx, len(rows), len(ref))
    is_f = ref.dtype == REF_DTYPE_F
    ids = ("win_start", "count") if grouped else (
        "sid", "win_start", "first_row_time", "count")
    if not row_time:
        ids = tuple(f for f in ids if f != "first_row_time")
    for f in ids:
        assert np.array_equal(rows[f], ref[f]), (ctx, f)
    for f in VALUE_FIELDS:
        assert np.array_equal(rows[f + "_isnil"], ref["isnil"]), (ctx, f)
    if with_sum:
        assert np.array_equal(rows["sum_isnil"], ref["isnil"]), (ctx, "sum")
    live = ref["isnil"] == 0
    for f in VALUE_FIELDS:
        got = rows[f][live].view(np.uint64)
        assert np.array_equal(got, ref[f][live].view(np.uint64)), (ctx, f)
        assert np.array_equal(rows[f + "_time"][live],
                              ref[f + "_time"][live]), (ctx, f + "_time")
    if not with_sum:
        return
    if is_f:
        g, r = rows["sum"][live], ref["sum"][live]
        tol = 1e-9 * np.maximum(1.0, np.abs(r))
        assert np.all(np.abs(g - r) <= tol), (ctx, "sum")
    else:
        assert np.array_equal(rows["sum"][live].view(np.int64),
                              ref["sum"][live]), (ctx, "sum")


def assert_grouped_parity(gpu_rows, ref, is_float):
    """Grouped engine rows against oracle scan_agg + group_merge, by the
    fields and rules of test_gpu_parity.TestGroupedParity."""
    assert len(gpu_rows) == len(ref), (len(gpu_rows), len(ref))
    for f in ("win_start", "count", "min_time", "max_time", "first_time",
              "last_time", "min_isnil", "max_isnil", "first_isnil",
              "last_isnil", "sum_isnil"):
        assert np.array_equal(gpu_rows[f], ref[f]), f
    for f in VALUE_FIELDS:
        assert np.array_equal(gpu_rows[f].view(np.uint64),
                              ref[f].view(np.uint64)), f
    if is_float:
        tol = 1e-9 * np.maximum(1.0, np.abs(ref["sum"]))
        both_nan = np.isnan(gpu_rows["sum"]) & np.isnan(ref["sum"])
        assert np.all(both_nan | (np.abs(gpu_rows["sum"] - ref["sum"]) <= tol))
    else:
        assert np.array_equal(gpu_rows["sum"].view(np.int64),
                              ref["sum"].view(np.int64))


def has_multi_row_window(ref):
    return len(ref) > 0 and int(ref["count"].max()) > 1


# ------------------------------------------------- PromQL numpy restatements
# the restatements test_oracle_rate.py carries inline, as functions of one
# window's non-nil, non-NaN points (time-ordered)

def prom_grid(start, end, range_ns, step):
    """Sample steps: start + range, then every step up to end."""
    ss = start + range_ns
    if end < ss:
        return []
    es = ss + (end - ss) // step * step
    return list(range(ss, es + 1, step))


def prom_windows(pts, start, end, range_ns, step):
    """Yields (sid, ts, times, values) of every non-empty window
    [ts - range, ts], sids ascending, in step order."""
    grid = prom_grid(start, end, range_ns, step)
    for sid in sorted(pts):
        t, v, valid = pts[sid]
        keep = valid & ~np.isnan(v)
        t, v = t[keep], v[keep]
        for ts in grid:
            m = (t >= ts - range_ns) & (t <= ts)
            if m.any():
                yield sid, ts, t[m], v[m]


def np_stdvar(v):
    """population variance (the reference divides by n)"""
    return float(np.mean((v - v.mean()) ** 2))


def np_changes(v):
    return float(np.count_nonzero(v[1:] != v[:-1]))


def np_resets(v):
    return float(np.count_nonzero(v[1:] < v[:-1]))


def np_linear(t, v, ts, scalar=None):
    """least-squares slope over x = (t - ts) seconds; with scalar, the
    prediction slope * scalar + intercept"""
    x = (t - ts) / 1e9
    n = len(x)
    vx = np.sum(x * x) - np.sum(x) ** 2 / n
    cov = np.sum(x * v) - np.sum(x) * np.sum(v) / n
    slope = cov / vx
    if scalar is None:
        return slope
    return slope * scalar + (np.mean(v) - slope * np.mean(x))


def np_quantile(v, q):
    x = np.sort(v)
    n = len(x)
    rank = q * (n - 1)
    lo = int(np.floor(rank))
    hi = min(n - 1, lo + 1)
    w = rank - np.floor(rank)
    return x[lo] * (1 - w) + x[hi] * w


def np_mad(v):
    return np_quantile(np.abs(v - np_quantile(v, 0.5)), 0.5)


def np_holt(v, sf, tf):
    s0, s1, b = 0.0, v[0], v[1] - v[0]
    for i in range(1, len(v)):
        x = sf * v[i]
        if i - 1 != 0:
            b = tf * (s1 - s0) + (1 - tf) * b
        y = (1 - sf) * (s1 + b)
        s0, s1 = s1, x + y
    return s1


def np_rate(t, v, ts, range_ns, is_rate=True, is_counter=True):
    """Prometheus extrapolated rate / increase / delta; None when the
    window has fewer than two points or no time span."""
    n = len(t)
    if n < 2 or t[-1] == t[0]:
        return None
    reduce = v[-1] - v[0]
    if is_counter:
        reduce += float(np.sum(v[:-1][v[1:] < v[:-1]]))
    to_start = int(t[0] - (ts - range_ns)) / 1e9
    to_end = int(ts - t[-1]) / 1e9
    sampled = int(t[-1] - t[0]) / 1e9
    avg = sampled / (n - 1)
    if is_counter and reduce > 0 and v[0] >= 0:
        to_start = min(to_start, sampled * (v[0] / reduce))
    thresh = avg * 1.1
    extrap = sampled
    extrap += avg / 2 if to_start >= thresh else to_start
    extrap += avg / 2 if to_end >= thresh else to_end
    res = reduce * (extrap / sampled)
    return res / (range_ns / 1e9) if is_rate else res


def np_irate(t, v, is_rate=True):
    if len(t) < 2 or t[-1] == t[-2]:
        return None
    if is_rate and v[-1] < v[-2]:
        res = v[-1]
    else:
        res = v[-1] - v[-2]
    return res / (int(t[-1] - t[-2]) / 1e9) if is_rate else res


OVER_TIME = {
    "sum": np.sum, "count": len, "avg": np.mean, "min": np.min,
    "max": np.max, "last": lambda x: x[-1], "stdvar": np_stdvar,
    "stddev": lambda x: np_stdvar(x) ** 0.5, "present": lambda x: 1.0,
    "changes": np_changes, "resets": np_resets,
}
OVER_TIME_EXACT = ("count", "min", "max", "last", "present", "changes",
                   "resets")

# (range, step) grids per spacing; start = base - 17 ns
PROM_AXES = [("EPOCH", "1s"), ("EPOCH", "100ms"), ("EPOCH", "jit_ns"),
             ("FAR", "1s")]
PROM_GRIDS = {"1s": [(300 * S, 60 * S)], "jit_ns": [(300 * S, 60 * S)],
              "100ms": [(300 * S, 60 * S), (5 * S, S)]}


def prom_query(axis, range_ns, step):
    """(start, end): the grid starts 17 ns before the first row and has
    six steps, so windows empty out one step at a time."""
    start = BASES[axis[0]] - 17
    return start, start + range_ns + 5 * step + step // 2


def check_prom(call, pts, start, end, range_ns, step):
    """Every Prom call against its restatement. call(name, **kw) returns
    the rows of one function. Tolerances are test_oracle_rate.py's for the
    same pairs: 1e-9, 1e-12 for quantile/mad, 1e-6 for deriv/predict; the
    counting and selecting functions are exact. Returns the number of rows
    compared."""
    wins = list(prom_windows(pts, start, end, range_ns, step))
    n = 0

    def compare(rows, fn, rel, min_pts=1, ctx=""):
        exp = []
        for sid, ts, t, v in wins:
            if len(t) < min_pts:
                continue
            r = fn(ts, t, v)
            if r is not None:
                exp.append((sid, ts, float(r)))
        assert len(rows) == len(exp), (ctx, len(rows), len(exp))
        assert len(exp) > 0, ctx
        assert rows["sid"].tolist() == [e[0] for e in exp], ctx
        assert rows["ts"].tolist() == [e[1] for e in exp], ctx
        ref = np.array([e[2] for e in exp])
        if rel == 0:
            assert np.array_equal(rows["value"], ref), ctx
        else:
            err = np.abs(rows["value"] - ref)
            assert np.all(err <= rel * np.maximum(1.0, np.abs(ref))), (
                ctx, float(err.max()))
        return len(exp)

    for fn, f in OVER_TIME.items():
        n += compare(call("over_time", func=fn), lambda ts, t, v: f(v),
                     0 if fn in OVER_TIME_EXACT else 1e-9, ctx=fn)
    for kw in (dict(is_rate=True, is_counter=True),
               dict(is_rate=False, is_counter=True),
               dict(is_rate=False, is_counter=False)):
        n += compare(call("rate", **kw),
                     lambda ts, t, v: np_rate(t, v, ts, range_ns, **kw),
                     1e-9, ctx=("rate", kw))
    for is_rate in (True, False):
        n += compare(call("irate", is_rate=is_rate),
                     lambda ts, t, v: np_irate(t, v, is_rate), 1e-9,
                     ctx=("irate", is_rate))
    n += compare(call("linear"), lambda ts, t, v: np_linear(t, v, ts), 1e-6,
                 min_pts=2, ctx="deriv")
    n += compare(call("linear", is_predict=True, scalar=300.0),
                 lambda ts, t, v: np_linear(t, v, ts, 300.0), 1e-6,
                 min_pts=2, ctx="predict")
    for q in (0.0, 0.5, 0.95):
        n += compare(call("quantile", q=q),
                     lambda ts, t, v: np_quantile(v, q), 1e-12, ctx=("q", q))
    n += compare(call("quantile", is_mad=True), lambda ts, t, v: np_mad(v),
                 1e-12, ctx="mad")
    n += compare(call("holt", sf=0.3, tf=0.6),
                 lambda ts, t, v: np_holt(v, 0.3, 0.6), 1e-9, min_pts=2,
                 ctx="holt")
    # quantile has to see a window whose point count is no power of two
    assert any(len(t) & (len(t) - 1) for _, _, t, _ in wins)
    return n


# every Prom call of check_prom, for engine-vs-oracle parity
PROM_CALLS = ([("over_time", dict(func=f)) for f in OVER_TIME]
              + [("rate", dict(is_rate=True, is_counter=True)),
                 ("rate", dict(is_rate=False, is_counter=True)),
                 ("rate", dict(is_rate=False, is_counter=False)),
                 ("irate", dict(is_rate=True)), ("irate", dict(is_rate=False)),
                 ("linear", dict()),
                 ("linear", dict(is_predict=True, scalar=300.0)),
                 ("quantile", dict(q=0.0)), ("quantile", dict(q=0.5)),
                 ("quantile", dict(q=0.95)), ("quantile", dict(is_mad=True)),
                 ("holt", dict(sf=0.3, tf=0.6))])


# ------------------------------------------------- what the writer produced

def seg_codes(blob, descs, col_type):
    """Per segment (data block kind, data codec tag, time codec tag), read
    from the block headers the way the engine's attach classifies them:
    kind full / one / empty / bitmap; time tag 1 const-delta, 2 simple8b,
    4 uncompressed, "one" for a one-row block."""
    out = []
    for d in descs:
        ds = blob[int(d["data_offset"]):int(d["data_offset"] + d["data_size"])]
        ts = blob[int(d["time_offset"]):int(d["time_offset"] + d["time_size"])]
        k = ds[0]
        if 30 <= k < 35:
            data = ("full", ds[5] >> 4)
        elif 16 < k < 21:
            data = ("one", None)
        elif 40 <= k < 45:
            data = ("empty", None)
        else:
            assert k == col_type, k
            data = ("bitmap", None)
        out.append(data + ((ts[5] >> 4) if ts[0] == 32 else "one",))
    return out


def foldable_segments(blob, descs):
    """How many segments of an all-gorilla, regular-grid shard sit in a
    launch wave the grouped scan can fold: the launch list is ordered by
    (stream words, segment id) and cut into waves of 64; a wave folds when
    its members share first time and row count."""
    words = (descs["data_size"].astype(np.int64) - 15 + 7) // 8
    order = sorted(range(len(descs)), key=lambda i: (int(words[i]), i))
    n = 0
    for a in range(0, len(order), 64):
        wave = order[a:a + 64]
        if len({(int(descs[i]["min_time"]), int(descs[i]["rows"]))
                for i in wave}) == 1:
            n += len(wave)
    return n
