"""Every consumer of the per-segment decode over every decode route.

One tiny shard per column type holds one series per route a segment can
take through the decoders: the block kinds (full, nil bitmap, one-value,
empty), the value codecs (gorilla, constant, snappy, bit-packed booleans)
and the time forms (const-delta grid, simple8b, one raw timestamp).
Segments have 1, 9 and 70 rows (70 crosses a bitmap byte and a bitmap
word), two or three to a series. Every scan call that decodes segments
runs over that shard and is compared with the CPU oracle, or with the
numpy reference its own test uses where the oracle has no such call, under
the bar that test holds it to.

Snappy-compressed time blocks are not covered: the oracle's time encoder
keeps its all-literal snappy stream only below a ratio it never reaches, so
no helper produces one.
"""

import numpy as np
import pytest

import binding as orc
import epoch_helpers as eh
from bool_helpers import assert_bool_rows, py_encode_bool_segment
from distinct_helpers import ref_distinct
from test_gpu_parity import assert_parity
from topn_helpers import (assert_rows_equal, oracle_shard, points_of_segments,
                          ref_topn, snappy_float_segment)

pytestmark = pytest.mark.gpu

S = 10**9
F = orc.ORC_TYPE_FLOAT
I = orc.ORC_TYPE_INT
BOOL = 5
T0 = eh.EPOCH
INTERVAL = 60 * S
FULL = (T0 - 10 * S, T0 + 10**6 * S)
CLIP = (T0 + 20 * S + 1, T0 + 100 * S - 1)   # cuts inside segments
PROM = (T0 - 17, T0 + 170 * S, 60 * S, 20 * S)  # start, end, range, step


# ------------------------------------------------------------------- shards

def _series(sid, seg_rows, value_fn, nil_fn=None, jitter=False, dseg_fn=None):
    """[(sid, times, values, valid[, data segment])]: consecutive segments
    of one series, 1 s apart (or a few ms to 4 s apart when jitter)."""
    rng = np.random.default_rng(4000 + sid)
    segs, t = [], T0 + sid * 3 * S
    for k, rows in enumerate(seg_rows):
        if jitter:
            times = t + np.cumsum(rng.integers(1, 4000, rows)).astype(
                np.int64) * 10**6
        else:
            times = t + np.arange(rows, dtype=np.int64) * S
        vals = value_fn(rng, rows)
        valid = (np.ones(rows, dtype=bool) if nil_fn is None
                 else nil_fn(rng, k, rows))
        seg = (sid, times, vals, valid)
        if dseg_fn is not None:
            seg += (dseg_fn(vals, valid),)
        segs.append(seg)
        t = int(times[-1]) + S
    return segs


def _counter(rng, rows):
    """multiples of 1/128 that reset: sums are exact in any order"""
    return np.cumsum(rng.integers(0, 2560, rows) / 128.0) % 97


def _some_nil(rng, k, rows):
    return rng.random(rows) > 0.25


def _float_segments():
    def with_nan(rng, rows):
        v = _counter(rng, rows)
        if rows > 17:
            v[17] = np.nan
        return v

    def blocks_nil(rng, k, rows):       # all-nil block, full, one-value nil
        return np.full(rows, k == 1, dtype=bool)

    return (
        _series(1, (70, 9, 70), _counter)                  # gorilla on a grid
        + _series(2, (70, 9), _counter, jitter=True)       # irregular times
        + _series(3, (1, 70, 1), _counter)                 # one-row segments
        + _series(4, (70, 9), lambda r, n: np.full(n, 3.25))   # one value
        + _series(5, (70, 9, 70), with_nan, _some_nil)     # nil bitmap, a NaN
        + _series(6, (9, 70, 1), _counter, blocks_nil)     # empty blocks
        + _series(7, (70, 9), _counter,                    # snappy values
                  dseg_fn=lambda v, x: snappy_float_segment(v)))


def _int_segments():
    def ints(rng, rows):
        return rng.integers(0, 1000, rows).astype(np.int64)

    return (_series(1, (70, 9, 70), ints)
            + _series(2, (70, 9, 70), ints, _some_nil)
            + _series(3, (1, 70, 1), ints)
            + _series(4, (9, 70), ints, jitter=True)
            + _series(5, (70, 9), lambda r, n: np.full(n, 7, dtype=np.int64)))


def _bool_segments(as_int=False):
    def bits(rng, rows):
        v = rng.integers(0, 2, rows)
        return v.astype(np.int64 if as_int else np.uint8)

    enc = None if as_int else py_encode_bool_segment
    return (_series(1, (70, 9, 70), bits, dseg_fn=enc)
            + _series(2, (70, 9, 70), bits, _some_nil, dseg_fn=enc)
            + _series(3, (1, 70, 1), bits, dseg_fn=enc))


def _filter_segments(segs, col):
    """The same rows with other values and other nils: the filter column of
    the cross-field predicate."""
    rng = np.random.default_rng(77)
    out = []
    for sid, times, _, _ in (s[:4] for s in segs):
        rows = len(times)
        valid = rng.random(rows) > 0.2
        if col == F:
            seg = (sid, times, rng.normal(0, 10, rows), valid)
        elif col == I:
            seg = (sid, times, rng.integers(0, 100, rows).astype(np.int64),
                   valid)
        else:
            v = rng.integers(0, 2, rows).astype(np.uint8)
            seg = (sid, times, v, valid, py_encode_bool_segment(v, valid))
        out.append(seg)
    return out


class Case:
    def __init__(self, col, segs, twin=None):
        import opengemini_amd as gx

        self.col, self.segs = col, segs
        self.blob, self.descs = oracle_shard(col, segs)
        self.descs = np.ascontiguousarray(self.descs)
        self.odescs = np.frombuffer(self.descs.tobytes(),
                                    dtype=orc.SEG_DESC_DTYPE)
        # what the oracle reads: a boolean shard's int64 0/1 twin
        self.ref_col = I if col == BOOL else col
        self.ref_blob, self.ref_descs = self.blob, self.odescs
        if twin is not None:
            b, d = oracle_shard(I, twin)
            self.ref_blob = b
            self.ref_descs = np.frombuffer(
                np.ascontiguousarray(d).tobytes(), dtype=orc.SEG_DESC_DTYPE)
        self.points = points_of_segments(segs)
        self.fsegs = _filter_segments(segs, col)
        fblob, fdescs = oracle_shard(col, self.fsegs)
        self.sh = gx.Shard(self.blob, self.descs, col)
        self.fsh = gx.Shard(fblob, np.ascontiguousarray(fdescs), col)

    def close(self):
        self.sh.close()
        self.fsh.close()


BUILDERS = {
    "float": lambda: Case(F, _float_segments()),
    "int": lambda: Case(I, _int_segments()),
    "bool": lambda: Case(BOOL, _bool_segments(),
                         twin=_bool_segments(as_int=True)),
}
FILTER = {"float": ("gt", 40.0), "int": ("gt", 500), "bool": ("eq", 1)}
XFILTER = {"float": ("gt", 0.0), "int": ("lt", 50), "bool": ("eq", True)}


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = BUILDERS[name]()
        return made[name]

    yield get
    for c in made.values():
        c.close()


def test_shards_reach_the_routes(cases):
    """The encoders picked the block kinds and codecs the cases are named
    after (data kind, value codec tag, time codec tag per segment)."""
    c = cases("float")
    codes = eh.seg_codes(c.blob, c.descs, F)
    by_sid = {}
    for d, code in zip(c.descs, codes):
        by_sid.setdefault(int(d["sid"]), []).append(code)
    assert by_sid[1][0] == ("full", 3, 1)            # gorilla, const-delta
    assert by_sid[2][0] == ("full", 3, 2)            # gorilla, simple8b times
    assert by_sid[3][0] == ("one", None, "one")
    assert by_sid[4][0][0] == "full" and by_sid[4][0][1] not in (2, 3)
    assert {x[0] for x in by_sid[5]} == {"bitmap"}
    assert [x[0] for x in by_sid[6]] == ["empty", "full", "empty"]
    assert by_sid[7][0] == ("full", 2, 1)            # snappy values
    ci = cases("int")
    kinds = [x[0] for x in eh.seg_codes(ci.blob, ci.descs, I)]
    assert {"full", "bitmap", "one"} <= set(kinds)
    cb = cases("bool")
    kinds = [x[0] for x in eh.seg_codes(cb.blob, cb.descs, BOOL)]
    assert {"full", "bitmap", "one"} <= set(kinds)


# ------------------------------------------------------------------ scan_agg

def _agg_same(c, got, ref):
    if c.col == BOOL:
        assert_bool_rows(got, ref)
    else:
        assert_parity(got, ref, c.col)
    assert len(ref) > 0


def _xfield_expect(c, op, operand, start, end):
    """(sid, window, count, sum, min, max) of the value rows whose filter
    row is non-nil and passes, from the authored inputs."""
    cmp = {"gt": np.greater, "lt": np.less, "eq": np.equal}[op]
    rows = []
    sids = sorted({s[0] for s in c.segs})
    for sid in sids:
        t = np.concatenate([s[1] for s in c.segs if s[0] == sid])
        v = np.concatenate([s[2] for s in c.segs if s[0] == sid])
        x = np.concatenate([s[3] for s in c.segs if s[0] == sid])
        fv = np.concatenate([s[2] for s in c.fsegs if s[0] == sid])
        fx = np.concatenate([s[3] for s in c.fsegs if s[0] == sid])
        keep = fx & cmp(fv, operand) & (t >= start) & (t <= end)
        t, v, x = t[keep], v[keep], x[keep]
        wins = t // INTERVAL * INTERVAL
        for w in np.unique(wins):
            vv = v[(wins == w) & x]
            rows.append((sid, int(w), vv))
    return rows


SCANS = ["plain", "clip", "filter", "xfield"]


@pytest.mark.parametrize("col", ["float", "int", "bool"])
@pytest.mark.parametrize("scan", SCANS)
def test_scan_agg(cases, scan, col):
    c = cases(col)
    if scan in ("plain", "clip"):
        q = FULL if scan == "plain" else CLIP
        for interval in (INTERVAL, 0):
            got = c.sh.scan_agg(*q, interval)[0].copy()
            ref = orc.scan_agg(c.ref_blob, c.ref_descs, c.ref_col, *q,
                               interval)
            _agg_same(c, got, ref)
    elif scan == "filter":
        op, operand = FILTER[col]
        for q in (FULL, CLIP):
            got = c.sh.scan_agg(*q, INTERVAL, filter=(op, operand))[0].copy()
            ref = orc.scan_agg_filtered(c.ref_blob, c.ref_descs, c.ref_col,
                                        *q, INTERVAL, op, operand)
            _agg_same(c, got, ref)
    else:
        op, operand = XFILTER[col]
        for q in (FULL, CLIP):
            got = c.sh.scan_agg_xfield(c.fsh, (op, operand), *q,
                                       INTERVAL)[0].copy()
            exp = _xfield_expect(c, op, operand, *q)
            assert len(got) == len(exp) > 0, (len(got), len(exp))
            for r, (sid, w, vv) in zip(got, exp):
                assert (int(r["sid"]), int(r["win_start"])) == (sid, w)
                assert int(r["count"]) == len(vv)
                if len(vv) == 0:
                    assert r["min_isnil"] and r["max_isnil"]
                    continue
                if c.col == F and np.isnan(vv).any():
                    continue    # numpy's NaN rules are not the engine's
                if c.col == F:
                    sm = float(vv.sum())
                    assert abs(r["sum"] - sm) <= 1e-9 * max(1.0, abs(sm))
                    assert r["min"] == vv.min() and r["max"] == vv.max()
                else:
                    iv = lambda f: int(np.array(r[f]).view(np.int64))
                    assert iv("min") == vv.min() and iv("max") == vv.max()
                    if c.col == I:
                        assert iv("sum") == int(vv.sum())


# ---------------------------------------------------------- the Prom family

def _prom_same(got, ref, how, ctx):
    assert len(got) == len(ref) > 0, (ctx, len(got), len(ref))
    assert np.array_equal(got["sid"], ref["sid"]), ctx
    assert np.array_equal(got["ts"], ref["ts"]), ctx
    g, r = got["value"], ref["value"]
    if how == "bits":
        assert g.tobytes() == r.tobytes(), ctx
    elif how == "isclose":
        assert np.all(np.isclose(g, r, rtol=1e-9, atol=1e-12)), ctx
    else:
        assert np.all(np.abs(g - r) <= how * np.maximum(1.0, np.abs(r))), ctx


# consumer -> [(engine call, oracle call, keywords, bar)]; the bars are
# those of TestRateParity, TestIrateParity, TestStdVarOverTimeGPU,
# test_quantile_mad_parity, test_gpu_rate_wide and test_gpu_ot_wide
PROM_CONSUMERS = {
    "rate": [("prom_rate", "prom_rate", kw, 1e-12) for kw in (
        dict(), dict(is_rate=False), dict(is_rate=False, is_counter=False))],
    "irate": [("prom_irate", "prom_irate", dict(), "bits"),
              ("prom_irate", "prom_irate", dict(is_rate=False), "bits")],
    "stdvar": [("prom_over_time", "prom_over_time", dict(func="stdvar"),
                "isclose"),
               ("prom_over_time", "prom_over_time", dict(func="count"),
                "bits")],
    "quantile": [("prom_quantile", "prom_quantile", dict(q=0.5), "bits"),
                 ("prom_quantile", "prom_quantile", dict(is_mad=True),
                  "bits")],
    "rate_wide": [("prom_rate_wide", "prom_rate", kw, 1e-12) for kw in (
        dict(), dict(is_rate=False), dict(is_rate=False, is_counter=False))],
    "irate_wide": [("prom_irate_wide", "prom_irate", dict(), 1e-12),
                   ("prom_irate_wide", "prom_irate", dict(is_rate=False),
                    1e-12)],
    "over_time_wide": [("prom_over_time_wide", "prom_over_time",
                        dict(func=f), "bits" if f in (
                            "min", "last", "changes") else "isclose")
                       for f in ("sum", "avg", "min", "last", "stdvar",
                                 "changes")],
}


@pytest.mark.parametrize("consumer", list(PROM_CONSUMERS))
def test_prom(cases, consumer):
    c = cases("float")
    for call, ref_call, kw, how in PROM_CONSUMERS[consumer]:
        got = getattr(c.sh, call)(*PROM, **kw)[0].copy()
        ref = getattr(orc, ref_call)(c.blob, c.odescs, *PROM, **kw)
        _prom_same(got, ref, how, (call, kw))


# ------------------------------------------------------ selectors, distinct

@pytest.mark.parametrize("col", ["float", "int"])
@pytest.mark.parametrize("sel", ["top", "bottom"])
def test_topn(cases, sel, col):
    c = cases(col)
    for q in (FULL, CLIP):
        for interval, n in ((INTERVAL, 3), (0, 5)):
            got = c.sh.scan_topn(*q, interval, n, sel=sel)[0].copy()
            exp = ref_topn(c.points, *q, interval, 0, n, sel, False)
            assert len(exp) > 0
            assert_rows_equal(got, exp, (sel, q, interval))


@pytest.mark.parametrize("col", ["float", "int", "bool"])
def test_distinct(cases, col):
    c = cases(col)
    for q in (FULL, CLIP):
        for interval in (INTERVAL, 0):
            got = c.sh.scan_distinct(*q, interval)[0].copy()
            exp = ref_distinct(c.points, *q, interval, 0, False)
            assert len(exp) > 0
            assert_rows_equal(got, exp, (q, interval))
