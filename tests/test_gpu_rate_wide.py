"""prom_rate_wide / prom_irate_wide (edge-record path, any range/step)
against the CPU oracle's orc_prom_rate / orc_prom_irate. Every comparison
needs equal length, sid and ts; every wide query runs twice on its handle
and must repeat bit for bit.

Bars: 1e-12 * max(1, |ref|) where the reset sums are exact in any order
(values are multiples of 1/128 below 2^40) or absent (monotone counters),
the bar of TestRateParity; 1e-9 * max(1, |ref|), the project's bar for float
sums whose order differs, on full-mantissa data with resets."""

import numpy as np
import pytest

import binding as orc
import epoch_helpers as eh
from shard_helpers import build_shard

pytestmark = pytest.mark.gpu

S = 10**9
F = orc.ORC_TYPE_FLOAT
I = orc.ORC_TYPE_INT

# (range, step) seconds
SWEEP = [(600, 10), (601, 7), (3600, 60), (300, 60), (120, 30), (5, 20),
         (300, 0)]
# rate, increase, delta, irate, idelta
FUNCS = [("rate", dict(is_rate=True, is_counter=True)),
         ("rate", dict(is_rate=False, is_counter=True)),
         ("rate", dict(is_rate=False, is_counter=False)),
         ("irate", dict(is_rate=True)),
         ("irate", dict(is_rate=False))]


# ------------------------------------------------------------------ helpers

def exact_resets(rng, rows):
    """counter in multiples of 1/128 that resets: cumsum % 97"""
    return np.cumsum(rng.integers(0, 2560, rows) / 128.0) % 97


def mono_full():
    """reset-free, full mantissa: one counter that keeps rising through
    every segment it is asked for"""
    last = [0.0]

    def fn(rng, rows):
        v = last[0] + np.cumsum(np.abs(rng.normal(1, 0.3, rows)))
        last[0] = float(v[-1])
        return v

    return fn


def resets_full(rng, rows):
    return np.cumsum(np.abs(rng.normal(1, 0.3, rows))) % 97.0


def pack(series):
    """[(sid, [(times, values, valid or None), ...])] -> blob, descs,
    usable point count. Segments in the order given."""
    blob, descs, pts = bytearray(), [], 0
    for sid, segs in series:
        for t, v, valid in segs:
            t = np.asarray(t, dtype=np.int64)
            v = np.asarray(v, dtype=np.float64)
            rows = len(t)
            if valid is None:
                ds = orc.encode_data_segment(F, v, None, rows, 0)
                pts += int((~np.isnan(v)).sum())
            else:
                valid = np.asarray(valid, dtype=bool)
                bm = np.packbits(valid.astype(np.uint8), bitorder="little")
                ds = orc.encode_data_segment(F, v[valid], bm, rows,
                                             int((~valid).sum()))
                pts += int((valid & ~np.isnan(v)).sum())
            ts = orc.encode_time_segment(t)
            descs.append((sid, len(blob), len(ds), rows, len(blob) + len(ds),
                          len(ts), 0, t[0], t[-1]))
            blob += ds + ts
    d = np.zeros(len(descs), dtype=orc.SEG_DESC_DTYPE)
    for i, x in enumerate(descs):
        d[i] = x
    return bytes(blob), d, pts


def grid_series(rng, sid, t0, seg_rows, value_fn, gap=S, dt=S):
    """one series: segments of seg_rows rows, dt apart, `gap` between the
    last row of a segment and the first of the next"""
    segs, t = [], t0
    for rows in seg_rows:
        times = t + np.arange(rows, dtype=np.int64) * dt
        segs.append((times, value_fn(rng, rows), None))
        t = int(times[-1]) + gap
    return sid, segs


class Case:
    """an attached shard with its encoded form, closed by the fixture"""

    def __init__(self, blob, descs, points=None, col_type=F):
        import opengemini_amd as gx

        self.blob, self.descs, self.points = blob, descs, points
        self.sh = gx.Shard(blob, descs, col_type)

    def close(self):
        self.sh.close()


def wide(sh, fn, kw, q):
    call = sh.prom_rate_wide if fn == "rate" else sh.prom_irate_wide
    rows, _ = call(*q, **kw)
    return rows.copy()  # the rows live in a pooled buffer


def ring(sh, fn, kw, q):
    call = sh.prom_rate if fn == "rate" else sh.prom_irate
    rows, _ = call(*q, **kw)
    return rows.copy()


def oracle(c, fn, kw, q):
    call = orc.prom_rate if fn == "rate" else orc.prom_irate
    return call(c.blob, c.descs, *q, **kw)


def same_rows(got, ref, rel, ctx):
    assert len(got) == len(ref), (ctx, len(got), len(ref))
    assert np.array_equal(got["sid"], ref["sid"]), ctx
    assert np.array_equal(got["ts"], ref["ts"]), ctx
    err = np.abs(got["value"] - ref["value"])
    tol = rel * np.maximum(1.0, np.abs(ref["value"]))
    worst = float((err / np.maximum(1.0, np.abs(ref["value"]))).max()) if len(
        ref) else 0.0
    print(ctx, "rows", len(ref), "worst rel err", worst)
    assert np.all(err <= tol), (ctx, worst)


def check(c, q, rel, funcs=FUNCS, min_rows=1):
    """every function of the family at one query, twice; returns the rows
    compared"""
    n = 0
    for fn, kw in funcs:
        a = wide(c.sh, fn, kw, q)
        b = wide(c.sh, fn, kw, q)
        assert a.tobytes() == b.tobytes(), (fn, kw, q)
        ref = oracle(c, fn, kw, q)
        same_rows(a, ref, rel, (fn, kw, q))
        n += len(ref)
    assert n >= min_rows, (q, n)
    return n


def query(rng_s, step_s, t0=0, t1=2000 * S, shift=0):
    """windows from 20 s after t0 (so the first ones are partly before the
    data) to t1; the single window of step 0 ends 250 s after t0"""
    first = t0 + (20 if step_s else 250) * S
    return (first - rng_s * S + shift, t1 + shift, rng_s * S, step_s * S)


# ------------------------------------------------------------------- shards

@pytest.fixture(scope="module")
def shards():
    made = {}

    def get(name):
        if name not in made:
            made[name] = BUILDERS[name]()
        return made[name]

    yield get
    for c in made.values():
        c.close()


def _built(value_fn, seed, null_frac=0.0, nan_at=None):
    rng = np.random.default_rng(seed)

    def vf(r, rows):
        v = value_fn(r, rows)
        if nan_at is not None and rows > nan_at:
            v[nan_at] = np.nan
        return v

    blob, d, truth = build_shard(rng, F, list(range(1, 9)), seg_range=(2, 7),
                                 row_range=(50, 301), null_frac=null_frac,
                                 value_fn=vf)
    pts = sum(int((x & ~np.isnan(v)).sum()) for _, v, x in truth.values())
    return Case(blob, d, pts)


def _gor():
    blob, descs = orc.gen_shard(5, 10, 3000)
    return Case(blob, descs, 10 * 3000)


def _irregular():
    rng = np.random.default_rng(31)
    series = []
    for sid in range(1, 7):
        t, segs = int(rng.integers(0, 50)) * S, []
        for _ in range(int(rng.integers(2, 5))):
            rows = int(rng.integers(50, 301))
            times = t + np.cumsum(rng.integers(1, 4000, rows)).astype(
                np.int64) * 10**6
            segs.append((times, exact_resets(rng, rows), None))
            t = int(times[-1]) + int(rng.integers(1, 4000)) * 10**6
        series.append((sid, segs))
    return Case(*pack(series))


def _shapes():
    """one-row segments, a constant series, a 2-point series"""
    rng = np.random.default_rng(32)
    s1 = grid_series(rng, 1, 5 * S, [120, 1, 1, 90, 1], exact_resets)
    s2 = grid_series(rng, 2, 0, [100, 150, 70], lambda r, n: np.full(n, 3.25))
    s3 = (3, [(np.array([400, 430]) * S, np.array([1.5, 4.25]), None)])
    s4 = (4, [(np.array([77 * S]), np.array([2.0]), None)])
    return Case(*pack([s1, s2, s3, s4]))


def _ownership(t0=0):
    """segments whose descriptor bounds hold no usable point where an edge
    falls; gaps; a shared boundary timestamp; series off the query"""
    rng = np.random.default_rng(33)

    def seg(start_s, rows, nil=None):
        t = t0 + (start_s + np.arange(rows, dtype=np.int64)) * S
        v = exact_resets(rng, rows)
        if nil is None:
            return (t, v, None)
        valid = np.ones(rows, dtype=bool)
        valid[nil] = False
        return (t, v, valid)

    series = [
        # tail rows all nil, then head rows all nil
        (1, [seg(0, 100, slice(60, None)), seg(100, 100, slice(0, 45)),
             seg(200, 80)]),
        # a wholly nil middle segment (and one at each end)
        (2, [seg(0, 90), seg(90, 60, slice(None)), seg(150, 90)]),
        (3, [seg(10, 40, slice(None)), seg(50, 120), seg(170, 40, slice(None))]),
        # gaps longer than the range inside the series
        (4, [seg(0, 80), seg(800, 1), seg(1500, 60), seg(1560, 70)]),
        # two segments sharing a boundary timestamp (and a third on it)
        (5, [seg(0, 101), seg(100, 100), seg(199, 1), seg(199, 90)]),
        # starts after start + range
        (6, [seg(900, 100), seg(1000, 100)]),
        # entirely outside the query
        (7, [seg(5000, 100), seg(5100, 50)]),
        (8, [seg(-9000, 100), seg(-8900, 50)]),
        # nothing usable at all
        (9, [seg(0, 50, slice(None)), seg(50, 50, slice(None))]),
    ]
    return Case(*pack(series))


def _many():
    """340 segments: more than one wave, more than one 256-thread block"""
    rng = np.random.default_rng(34)
    series = [grid_series(rng, sid, int(rng.integers(0, 30)) * S, [50] * 4,
                          exact_resets) for sid in range(1, 86)]
    return Case(*pack(series))


def _placed(t0):
    rng = np.random.default_rng(35)
    series = [grid_series(rng, sid, t0 + int(rng.integers(0, 60)) * S,
                          rng.integers(50, 301, int(rng.integers(2, 7))),
                          exact_resets) for sid in range(1, 7)]
    return Case(*pack(series))


NEG = -3_000 * S - 1
BUILDERS = {
    "exact": lambda: _built(exact_resets, 21),
    "mono_full": lambda: _built(mono_full(), 22),
    "resets_full": lambda: _built(resets_full, 23),
    "nils": lambda: _built(exact_resets, 24, null_frac=0.2, nan_at=17),
    "gor": _gor,
    "irregular": _irregular,
    "shapes": _shapes,
    "ownership": _ownership,
    "ownership_epoch": lambda: _ownership(eh.EPOCH),
    "many": _many,
    "negative": lambda: _placed(NEG),
    "epoch": lambda: _placed(eh.EPOCH),
}


# -------------------------------------------------------------------- tests

@pytest.mark.parametrize("rs", SWEEP, ids=lambda x: f"{x[0]}-{x[1]}")
@pytest.mark.parametrize("data,rel", [("exact", 1e-12), ("mono_full", 1e-12),
                                      ("resets_full", 1e-9)])
def test_sweep(shards, data, rel, rs):
    check(shards(data), query(*rs), rel)


@pytest.mark.parametrize("data,rel", [("exact", 1e-12), ("mono_full", 1e-12),
                                      ("resets_full", 1e-9)])
def test_edges_off_the_grid(shards, data, rel):
    """(600, 10) with start and end half a second off: no point lies on an
    edge, where the unshifted sweep puts one on every edge"""
    check(shards(data), query(600, 10, shift=S // 2), rel)


@pytest.mark.parametrize("rs", [(600, 10), (120, 30), (5, 20), (300, 0)],
                         ids=lambda x: f"{x[0]}-{x[1]}")
@pytest.mark.parametrize("data", ["gor", "irregular", "nils", "shapes"])
def test_decode_routes(shards, data, rs):
    """gorilla arena over 3 segments per series, simple8b times, the
    general route (bitmap + NaN), one-row / constant / 2-point segments"""
    c = shards(data)
    t1 = 3100 * S if data == "gor" else 2000 * S
    check(c, query(*rs, t1=t1), 1e-12)


@pytest.mark.parametrize("rs", [(600, 10), (120, 30), (60, 1), (5, 20),
                                (300, 0), (3600, 60)],
                         ids=lambda x: f"{x[0]}-{x[1]}")
def test_edge_ownership(shards, rs):
    c = shards("ownership")
    q = query(*rs)
    check(c, q, 1e-12)
    if rs == (120, 30):
        # the gap rows of series 4 are absent, not nil; series 7-9 give none
        rows = wide(c.sh, "rate", {}, q)
        assert not rows["isnil"].any()
        got = rows[rows["sid"] == 4]["ts"]
        assert len(got) > 0 and not ((got > 300 * S) & (got < 1500 * S)).any()
        assert set(rows["sid"].tolist()) == {1, 2, 3, 4, 5, 6}


@pytest.mark.parametrize("rs", [(600, 10), (120, 30), (5, 20)],
                         ids=lambda x: f"{x[0]}-{x[1]}")
@pytest.mark.parametrize("data,t0", [("negative", NEG), ("epoch", eh.EPOCH),
                                     ("ownership_epoch", eh.EPOCH)])
def test_shifted_times(shards, data, t0, rs):
    """negative times and a production epoch with a nanosecond remainder"""
    check(shards(data), query(*rs, t0=t0, t1=t0 + 2000 * S), 1e-12)


@pytest.mark.parametrize("rs", [(600, 10), (120, 30)],
                         ids=lambda x: f"{x[0]}-{x[1]}")
def test_many_segments(shards, rs):
    c = shards("many")
    assert len(c.descs) >= 300
    check(c, query(*rs, t1=300 * S), 1e-12, min_rows=1000)


@pytest.mark.parametrize("rs", [(300, 60), (120, 30)],
                         ids=lambda x: f"{x[0]}-{x[1]}")
@pytest.mark.parametrize("data", ["exact", "nils", "ownership"])
def test_agrees_with_ring_path(shards, data, rs):
    c = shards(data)
    q = query(*rs)
    for fn, kw in FUNCS:
        a, b = wide(c.sh, fn, kw, q), ring(c.sh, fn, kw, q)
        assert len(a) == len(b) > 0, (fn, kw)
        assert np.array_equal(a["sid"], b["sid"])
        assert np.array_equal(a["ts"], b["ts"])
        tol = 1e-12 * np.maximum(1.0, np.abs(b["value"]))
        assert np.all(np.abs(a["value"] - b["value"]) <= tol), (fn, kw)


@pytest.mark.parametrize("data", ["exact", "nils", "gor"])
def test_cost_does_not_follow_the_range(shards, data):
    c = shards(data)
    n_series = len(np.unique(c.descs["sid"]))
    seen = []
    for rng_s in (60, 3600):
        q = query(rng_s, 10, t1=3100 * S)
        start, end, rng_ns, step = q
        n_steps = (end - start - rng_ns) // step + 1
        rows = wide(c.sh, "rate", {}, q)
        assert len(rows) > 0
        recs, pts = c.sh.prom_wide_stats()
        print(data, rng_s, "steps", n_steps, "edge records", recs, "points", pts)
        assert 0 < recs <= 2 * n_series * n_steps
        assert pts == c.points
        seen.append((recs, n_steps))
    # the same grid length at both ranges: the record bound did not move
    assert seen[0][1] == seen[1][1]


def test_contract_arguments(shards):
    import opengemini_amd as gx

    blob, descs = orc.gen_shard(47, 4, 200, mode=orc.GEN_INT_SMALL)
    ci = Case(blob, descs, col_type=I)
    try:
        with pytest.raises(gx.GemxError):
            ci.sh.prom_rate_wide(0, 199 * S, 60 * S, 10 * S)
        with pytest.raises(gx.GemxError):
            ci.sh.prom_irate_wide(0, 199 * S, 60 * S, 10 * S)
    finally:
        ci.close()
    sh = shards("exact").sh
    for rng_ns, step in ((0, 10 * S), (-S, 10 * S), (60 * S, -1)):
        with pytest.raises(gx.GemxError):
            sh.prom_rate_wide(0, 2000 * S, rng_ns, step)
        with pytest.raises(gx.GemxError):
            sh.prom_irate_wide(0, 2000 * S, rng_ns, step)
    # end < start + range: no sample on the grid
    for call in (sh.prom_rate_wide, sh.prom_irate_wide):
        rows, _ = call(0, 100 * S, 600 * S, 10 * S)
        assert len(rows) == 0
    assert sh.prom_wide_stats() == (0, 0)


def test_contract_out_cap(shards):
    """out_cap below the row count: whatever prom_rate does, on a shape
    both paths take"""
    import opengemini_amd as gx

    sh = shards("exact").sh
    q = query(300, 60)
    full = len(ring(sh, "rate", {}, q))

    def outcome(call, cap):
        try:
            rows, _ = call(*q, out_cap=cap)
            return len(rows)
        except gx.GemxError:
            return "error"

    for cap in (1, full // 2, full - 1, full, full + 64, 4 * full):
        assert outcome(sh.prom_rate_wide, cap) == outcome(sh.prom_rate, cap), cap
        assert outcome(sh.prom_irate_wide, cap) == outcome(sh.prom_irate, cap), cap
    assert outcome(sh.prom_rate_wide, 1) == "error"
    assert outcome(sh.prom_rate_wide, 4 * full) == full


def test_contract_refused_while_async_in_flight(shards):
    import opengemini_amd as gx

    c = shards("exact")
    q = query(300, 60)
    out = c.sh.prom_rate_begin(*q)
    try:
        with pytest.raises(gx.GemxError):
            c.sh.prom_rate_wide(*q)
        with pytest.raises(gx.GemxError):
            c.sh.prom_irate_wide(*query(600, 10))
    finally:
        rows, _ = c.sh.prom_rate_finish(out)
    same_rows(rows, oracle(c, "rate", {}, q), 1e-12, "finish after refusal")
    check(c, query(600, 10), 1e-12)  # and the wide path works again


def test_plan_cache_reuse_and_rebuild(shards):
    """the same query around a different (range, step): reuse, rebuild,
    rebuild back — all three agree bit for bit and with the oracle"""
    c = shards("exact")
    qa, qb = query(600, 10), query(3600, 60)
    for fn, kw in FUNCS:
        a1 = wide(c.sh, fn, kw, qa)
        a2 = wide(c.sh, fn, kw, qa)
        b = wide(c.sh, fn, kw, qb)
        a3 = wide(c.sh, fn, kw, qa)
        assert a1.tobytes() == a2.tobytes() == a3.tobytes(), (fn, kw)
        same_rows(a3, oracle(c, fn, kw, qa), 1e-12, (fn, kw, "a"))
        same_rows(b, oracle(c, fn, kw, qb), 1e-12, (fn, kw, "b"))
    # rate and irate share one plan: alternating them must not disturb it
    r = wide(c.sh, "rate", {}, qa)
    i = wide(c.sh, "irate", {}, qa)
    same_rows(r, oracle(c, "rate", {}, qa), 1e-12, "rate after irate")
    same_rows(i, oracle(c, "irate", {}, qa), 1e-12, "irate after rate")
