"""prom_over_time_wide (per-cell path, any range/step) against the CPU
oracle's orc_prom_over_time. Every comparison needs equal length, sid and
ts; every wide query runs twice on its handle and must repeat bit for bit.

Bars: count, min, max, last, present, absent, changes and resets are exact
(value equal bit for bit). sum, avg, stdvar and stddev combine states across
cells and segments, so they hold np.isclose(rtol=1e-9, atol=1e-12), the bar
TestPromFamilyFuzz and TestStdVarOverTimeGPU hold these functions to when
states combine across segments."""

import numpy as np
import pytest

import binding as orc
import epoch_helpers as eh
from test_gpu_rate_wide import (BUILDERS, NEG, Case, S, SWEEP, pack, query)

pytestmark = pytest.mark.gpu

F = orc.ORC_TYPE_FLOAT
I = orc.ORC_TYPE_INT

EXACT = ["count", "min", "max", "last", "present", "absent", "changes",
         "resets"]
FLOAT = ["sum", "avg", "stdvar", "stddev"]
ALL = EXACT + FLOAT
assert sorted(ALL) == sorted(orc.OT_FUNCS)


# ------------------------------------------------------------------ helpers

def wide(sh, fn, q, **kw):
    rows, _ = sh.prom_over_time_wide(*q, fn, **kw)
    return rows.copy()  # the rows live in a pooled buffer


def ring(sh, fn, q, **kw):
    rows, _ = sh.prom_over_time(*q, fn, **kw)
    return rows.copy()


def same_rows(got, ref, fn, ctx):
    assert len(got) == len(ref), (ctx, len(got), len(ref))
    assert np.array_equal(got["sid"], ref["sid"]), ctx
    assert np.array_equal(got["ts"], ref["ts"]), ctx
    assert not got["isnil"].any(), ctx
    if fn in EXACT:
        assert got["value"].tobytes() == ref["value"].tobytes(), ctx
    else:
        err = np.abs(got["value"] - ref["value"])
        worst = float((err / np.maximum(1e-300, np.abs(ref["value"]))).max()
                      ) if len(ref) else 0.0
        print(ctx, "rows", len(ref), "worst rel err", worst)
        assert np.all(np.isclose(got["value"], ref["value"], rtol=1e-9,
                                 atol=1e-12)), (ctx, worst)


def check(c, q, funcs=ALL, min_rows=1):
    """every function at one query, twice; returns the rows compared"""
    n = 0
    for fn in funcs:
        a = wide(c.sh, fn, q)
        b = wide(c.sh, fn, q)
        assert a.tobytes() == b.tobytes(), (fn, q)
        same_rows(a, orc.prom_over_time(c.blob, c.descs, *q, fn), fn, (fn, q))
        n += len(a)
    assert n >= min_rows, (q, n)
    return n


def flat_series(sid, segs):
    """[(first second, values)] -> one series with a point every second"""
    return sid, [((t0 + np.arange(len(v), dtype=np.int64)) * S,
                  np.asarray(v, dtype=np.float64), None) for t0, v in segs]


def _steps():
    """changes/resets whose only hit lies on a seam. query(600, 10) cuts the
    axis just before every multiple of 10 s and just after it."""
    rng = np.random.default_rng(41)
    one = np.ones
    series = [
        # between the last point of one cell (99 s) and the first of the
        # next (100 s)
        flat_series(1, [(0, np.r_[one(100) * 5, one(100) * 3])]),
        # between 100 s (a cell of its own, on an edge) and 101 s
        flat_series(2, [(0, np.r_[one(101) * 5, one(99) * 7])]),
        # between two segments, inside a cell (154 s | 155 s)
        flat_series(3, [(0, one(155) * 5), (155, one(145) * 3)]),
        # between two segments, on a cut (149 s | 150 s), and nowhere else
        flat_series(4, [(0, one(150) * 2), (150, one(150) * 9)]),
        # no hit at all across a segment seam
        flat_series(5, [(0, one(155) * 4), (155, one(145) * 4)]),
    ]
    for sid in range(6, 12):
        segs, t = [], int(rng.integers(0, 40))
        for _ in range(int(rng.integers(2, 6))):
            n = int(rng.integers(50, 301))
            segs.append((t, rng.integers(0, 3, n).astype(float)))
            t += n
        series.append(flat_series(sid, segs))
    return Case(*pack(series))


MY_BUILDERS = dict(BUILDERS, steps=_steps)


@pytest.fixture(scope="module")
def shards():
    made = {}

    def get(name):
        if name not in made:
            made[name] = MY_BUILDERS[name]()
        return made[name]

    yield get
    for c in made.values():
        c.close()


def dense_rows(c, q):
    """(series, step) rows the plan spans: first right edge at or after the
    series' first descriptor time to the last left edge at or before its
    last one"""
    start, end, rng_ns, step = q
    n_ord = 1 if step == 0 else (end - start - rng_ns) // step + 1
    L = start + np.arange(n_ord, dtype=np.int64) * (step or 1)
    R = L + rng_ns
    total = 0
    for sid in np.unique(c.descs["sid"]):
        d = c.descs[c.descs["sid"] == sid]
        lo = int((R < d["min_time"].min()).sum())
        hi = int((L <= d["max_time"].max()).sum())
        total += max(hi - lo, 0)
    return total, int(n_ord)


# -------------------------------------------------------------------- tests

@pytest.mark.parametrize("rs", SWEEP, ids=lambda x: f"{x[0]}-{x[1]}")
@pytest.mark.parametrize("data", ["exact", "mono_full", "resets_full"])
def test_sweep(shards, data, rs):
    """(600,10) has interior rows (joins), (3600,60) only clamped end rows
    (folds), (5,20) width-1 windows and cells of no window, (300,0) the
    single sample"""
    check(shards(data), query(*rs))


@pytest.mark.parametrize("data", ["exact", "mono_full", "resets_full"])
def test_edges_off_the_grid(shards, data):
    """(600, 10) with start and end half a second off: no point lies on an
    edge, where the unshifted sweep puts one on every edge (and the point
    must count in both windows that share the edge)"""
    check(shards(data), query(600, 10, shift=S // 2))


@pytest.mark.parametrize("rs", [(600, 10), (120, 30), (5, 20), (300, 0)],
                         ids=lambda x: f"{x[0]}-{x[1]}")
@pytest.mark.parametrize("data", ["gor", "irregular", "nils", "shapes"])
def test_decode_routes(shards, data, rs):
    """gorilla arena over 3 segments per series, simple8b times, the
    general route (bitmap + NaN), one-row / constant / 2-point segments"""
    c = shards(data)
    t1 = 3100 * S if data == "gor" else 2000 * S
    check(c, query(*rs, t1=t1))


@pytest.mark.parametrize("rs", [(600, 10), (120, 30), (60, 1), (5, 20),
                                (300, 0), (3600, 60)],
                         ids=lambda x: f"{x[0]}-{x[1]}")
def test_ownership_shapes(shards, rs):
    """all-nil head/tail/middle segments, gaps longer than the range,
    segments sharing a boundary timestamp, series outside the query, a
    series with nothing usable; absent emits what the oracle emits"""
    c = shards("ownership")
    q = query(*rs)
    check(c, q)
    if rs == (120, 30):
        for fn in ("present", "count"):
            rows = wide(c.sh, fn, q)
            got = rows[rows["sid"] == 4]["ts"]
            # nothing inside the long gaps of series 4 (points at 0-79 s,
            # 800 s, 1500-1629 s; windows reach 120 s back)
            assert len(got) > 0
            assert not ((got > 200 * S) & (got < 800 * S)).any(), fn
            assert not ((got > 920 * S) & (got < 1500 * S)).any(), fn
            assert set(rows["sid"].tolist()) == {1, 2, 3, 4, 5, 6}
        ab = wide(c.sh, "absent", q)
        # series 7-9 have no usable point in the query: absent everywhere
        n_steps = (q[1] - q[0] - q[2]) // q[3] + 1
        for sid in (7, 8, 9):
            assert (ab["sid"] == sid).sum() == n_steps, sid


@pytest.mark.parametrize("rs", [(600, 10), (601, 7), (120, 30), (5, 20),
                                (3600, 60)],
                         ids=lambda x: f"{x[0]}-{x[1]}")
def test_changes_resets_across_seams(shards, rs):
    """values of rng.integers(0, 3, n), and hand-built series whose only
    change lies between two cells or between two segments"""
    c = shards("steps")
    q = query(*rs, t1=400 * S)
    check(c, q, funcs=["changes", "resets", "last", "count"])
    if rs == (600, 10):
        ch = wide(c.sh, "changes", q)
        rs_ = wide(c.sh, "resets", q)
        for sid, n_ch, n_rs in ((1, 1, 1), (2, 1, 0), (3, 1, 1), (4, 1, 0),
                                (5, 0, 0)):
            # the last window holds the whole series
            assert ch[ch["sid"] == sid]["value"].max() == n_ch, sid
            assert rs_[rs_["sid"] == sid]["value"].max() == n_rs, sid


@pytest.mark.parametrize("rs", [(600, 10), (120, 30), (5, 20)],
                         ids=lambda x: f"{x[0]}-{x[1]}")
@pytest.mark.parametrize("data,t0", [("negative", NEG), ("epoch", eh.EPOCH),
                                     ("ownership_epoch", eh.EPOCH)])
def test_shifted_times(shards, data, t0, rs):
    """negative times and a production epoch with a nanosecond remainder"""
    check(shards(data), query(*rs, t0=t0, t1=t0 + 2000 * S))


@pytest.mark.parametrize("rs", [(600, 10), (120, 30)],
                         ids=lambda x: f"{x[0]}-{x[1]}")
def test_many_segments(shards, rs):
    c = shards("many")
    assert len(c.descs) >= 300
    check(c, query(*rs, t1=300 * S), min_rows=1000)


@pytest.mark.parametrize("rs", [(300, 60), (120, 30)],
                         ids=lambda x: f"{x[0]}-{x[1]}")
@pytest.mark.parametrize("data", ["exact", "nils", "ownership"])
def test_agrees_with_ring_path(shards, data, rs):
    """Same rows, exact functions equal, float functions within the bar.
    absent is the one function whose rows differ by design: the ring path
    answers a series only between its first and last descriptor time, the
    wide path (and the oracle) over the whole grid. There the ring's rows
    must all be among the wide ones."""
    c = shards(data)
    q = query(*rs)
    for fn in ALL:
        a, b = wide(c.sh, fn, q), ring(c.sh, fn, q)
        if fn == "absent":
            wa = set(zip(a["sid"].tolist(), a["ts"].tolist()))
            rb = set(zip(b["sid"].tolist(), b["ts"].tolist()))
            assert rb <= wa and np.all(a["value"] == 1.0), fn
            continue
        assert len(b) > 0, fn
        same_rows(a, b, fn, (fn, "ring", rs))


def test_the_bound_is_gone(shards):
    """(3600, 60): the ring path still refuses, the wide path answers"""
    import opengemini_amd as gx

    c = shards("exact")
    q = query(3600, 60)
    for fn in ALL:
        with pytest.raises(gx.GemxError):
            c.sh.prom_over_time(*q, fn)
        got = wide(c.sh, fn, q)
        same_rows(got, orc.prom_over_time(c.blob, c.descs, *q, fn), fn, fn)
        if fn != "absent":
            assert len(got) > 0, fn


@pytest.mark.parametrize("data", ["exact", "nils", "gor"])
def test_cost_does_not_follow_the_range(shards, data):
    c = shards(data)
    n_series = len(np.unique(c.descs["sid"]))
    n_segs = len(c.descs)
    seen = []
    for rng_s in (60, 3600):
        q = query(rng_s, 10, t1=3100 * S)
        dense, n_ord = dense_rows(c, q)
        for fn in ("sum", "max", "absent"):
            rows = wide(c.sh, fn, q)
            slots, pts, joined, folded = c.sh.prom_wide_ot_stats()
            print(data, rng_s, fn, "steps", n_ord, "slots", slots, "points",
                  pts, "joined", joined, "folded", folded)
            assert 0 < slots <= n_series * (2 * n_ord + 1) + (n_segs - n_series)
            assert pts == c.points
            want = n_series * n_ord if fn == "absent" else dense
            assert joined + folded == want, fn
            assert len(rows) <= want
        seen.append(n_ord)
    # the same grid length at both ranges: the slot bound did not move
    assert seen[0] == seen[1]
    # interior rows join stored states; a grid shorter than the ratio has
    # only clamped end rows, which fold their cells
    wide(c.sh, "sum", query(600, 10))
    assert c.sh.prom_wide_ot_stats()[2] > 0
    wide(c.sh, "sum", query(3600, 60))
    _, _, joined, folded = c.sh.prom_wide_ot_stats()
    assert joined == 0 and folded == dense_rows(c, query(3600, 60))[0]


def test_contract_arguments(shards):
    import opengemini_amd as gx

    blob, descs = orc.gen_shard(47, 4, 200, mode=orc.GEN_INT_SMALL)
    ci = Case(blob, descs, col_type=I)
    try:
        with pytest.raises(gx.GemxError):
            ci.sh.prom_over_time_wide(0, 199 * S, 60 * S, 10 * S, "sum")
    finally:
        ci.close()
    sh = shards("exact").sh
    for rng_ns, step in ((0, 10 * S), (-S, 10 * S), (60 * S, -1)):
        with pytest.raises(gx.GemxError):
            sh.prom_over_time_wide(0, 2000 * S, rng_ns, step, "sum")
    # deriv/predict, quantile/mad, holt, rate/irate: no per-cell state
    for code in (13, 14, 16, 17, 18, 0, 1):
        with pytest.raises(gx.GemxError) as ei:
            sh.prom_over_time_wide(0, 2000 * S, 600 * S, 10 * S, code)
        assert str(ei.value)
    # end < start + range: no sample on the grid
    for fn in ("sum", "absent"):
        rows, st = sh.prom_over_time_wide(0, 100 * S, 600 * S, 10 * S, fn)
        assert len(rows) == 0
        assert st["n_rows"] == 0 and st["total_ms"] == 0 and st["points"] == 0
    assert sh.prom_wide_ot_stats() == (0, 0, 0, 0)


def test_contract_out_cap(shards):
    """out_cap below the row count: whatever prom_over_time does, on a
    shape both paths take"""
    import opengemini_amd as gx

    sh = shards("exact").sh
    q = query(300, 60)
    full = len(ring(sh, "sum", q))

    def outcome(call, fn, cap):
        try:
            rows, _ = call(*q, fn, out_cap=cap)
            return len(rows)
        except gx.GemxError:
            return "error"

    for cap in (1, full // 2, full - 1, full, full + 64, 4 * full):
        for fn in ("sum", "max", "count", "changes"):
            assert outcome(sh.prom_over_time_wide, fn, cap) == outcome(
                sh.prom_over_time, fn, cap), (fn, cap)
    assert outcome(sh.prom_over_time_wide, "sum", 1) == "error"
    assert outcome(sh.prom_over_time_wide, "sum", 4 * full) == full


def test_contract_refused_while_async_in_flight(shards):
    import opengemini_amd as gx

    c = shards("exact")
    q = query(300, 60)
    out = c.sh.prom_rate_begin(*q)
    try:
        with pytest.raises(gx.GemxError):
            c.sh.prom_over_time_wide(*q, "sum")
        with pytest.raises(gx.GemxError):
            c.sh.prom_over_time_wide(*query(600, 10), "max")
    finally:
        rows, _ = c.sh.prom_rate_finish(out)
    ref = orc.prom_rate(c.blob, c.descs, *q)
    assert len(rows) == len(ref) and np.array_equal(rows["ts"], ref["ts"])
    check(c, query(600, 10))  # and the wide path works again


def test_plan_cache_reuse_and_rebuild(shards):
    """the same query around a different (range, step): reuse, rebuild,
    rebuild back — all three agree bit for bit and with the oracle; the
    functions share one plan, so alternating them must not disturb it"""
    c = shards("exact")
    qa, qb = query(600, 10), query(3600, 60)
    for fn in ALL:
        a1 = wide(c.sh, fn, qa)
        a2 = wide(c.sh, fn, qa)
        b = wide(c.sh, fn, qb)
        a3 = wide(c.sh, fn, qa)
        assert a1.tobytes() == a2.tobytes() == a3.tobytes(), fn
        same_rows(a3, orc.prom_over_time(c.blob, c.descs, *qa, fn), fn, (fn, "a"))
        same_rows(b, orc.prom_over_time(c.blob, c.descs, *qb, fn), fn, (fn, "b"))
    first = {fn: wide(c.sh, fn, qa) for fn in ALL}
    for fn in reversed(ALL):
        assert wide(c.sh, fn, qa).tobytes() == first[fn].tobytes(), fn
