"""distinct() selector scans on the GPU against the numpy reference
(distinct_helpers.ref_distinct, itself checked against the reference's
golden records in test_distinct_host.py). Every comparison is exact."""

import ctypes as C

import numpy as np
import pytest

import opengemini_amd as gx
from opengemini_amd.engine import (GEMX_TYPE_BOOL, GEMX_TYPE_FLOAT,
                                   GEMX_TYPE_INT)

import bool_helpers as bh
import distinct_helpers as dh
import topn_helpers as th
from test_gpu_topn import _times, _values

pytestmark = pytest.mark.gpu

S = dh.S
NSER = 8
E_UNSUPPORTED = -4
E_CAP = -6


def _grid_series(nser, nrows, value_fn, t0_fn=lambda sid: 0):
    return {sid: ((t0_fn(sid) + np.arange(nrows, dtype=np.int64)) * S,
                  value_fn(sid, np.arange(nrows)))
            for sid in range(1, nser + 1)}


# ---- 1. the reference's golden records ----

@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("case", dh.load_golden(), ids=lambda c: c["name"])
def test_golden_records(case, kind):
    """One segment per reference record, so windows of time(2ns) span
    segments."""
    vtype, ct = ((np.int64, GEMX_TYPE_INT) if kind == "int"
                 else (np.float64, GEMX_TYPE_FLOAT))
    segs = dh.golden_segments(case, vtype)
    blob, descs = th.oracle_shard(ct, segs)
    pts = th.points_of_segments(segs)
    sh = gx.Shard(blob, descs, ct)
    try:
        for q in case["queries"]:
            rows, _ = sh.scan_distinct(case["start"], case["end"],
                                       q["interval"],
                                       group_all=q["group_all"])
            dh.assert_golden_query(rows, q, (case["name"], q["interval"]))
            assert rows["value"].dtype == np.dtype(vtype)
        dh.sweep(sh, pts, case["start"], case["end"],
                 ((2, 0), (3, 1), (0, 0)), ctx=case["name"])
    finally:
        sh.close()


# ---- 2. codec and path sweep ----

# (values, times, rows per segment, rows per series): every value kind over
# every time kind; segment sizes 1, 3, 64, 65, 1000; walks of <= 1500 rows
SWEEP = [
    ("rle", "grid", 1000, 1500),
    ("rle", "gaps", 3, 40),
    ("rle", "dt0", 64, 150),
    ("rle", "neg", 65, 200),
    ("const", "grid", 64, 150),
    ("const", "gaps", 1000, 1200),
    ("const", "dt0", 3, 20),
    ("const", "neg", 1, 30),
    ("small", "grid", 1000, 1200),
    ("small", "gaps", 64, 200),
    ("small", "dt0", 3, 25),
    ("small", "neg", 65, 200),
    ("walk", "grid", 65, 200),
    ("walk", "gaps", 1, 30),
    ("walk", "dt0", 65, 140),
    ("walk", "neg", 1000, 1490),
]


@pytest.mark.parametrize("vk,tk,seg_rows,nrows", SWEEP,
                         ids=["%s-%s-%d" % c[:3] for c in SWEEP])
def test_codec_and_path_sweep(vk, tk, seg_rows, nrows):
    rng = np.random.default_rng(2000 + SWEEP.index((vk, tk, seg_rows, nrows)))
    pts = {}
    for sid in range(1, NSER + 1):
        n = nrows + int(rng.integers(0, 7))
        pts[sid] = (_times(rng, tk, n, sid), _values(rng, vk, n))
    blob, descs, ct = th.writer_shard(pts, seg_rows)
    sh = gx.Shard(blob, descs, ct)
    try:
        assert dh.sweep(sh, pts, -(2**62), 2**62, ctx=(vk, tk, seg_rows)) > 0
    finally:
        sh.close()


# ---- 3. more series than a wave, windows straddling segment boundaries ----

def test_seventy_series_three_segments():
    rng = np.random.default_rng(303)
    codes = np.array([200, 301, 404, 500, 503], dtype=np.int64)
    pts = _grid_series(70, 2500, lambda sid, r: codes[rng.integers(0, 5, len(r))])
    sids = np.concatenate([np.full(2500, s, dtype=np.uint64) for s in pts])
    times = np.concatenate([t for t, _ in pts.values()])
    vals = np.concatenate([v for _, v in pts.values()])
    # segments of 1000 + 1000 + 500 rows; 60 s windows straddle both cuts
    blob, descs = gx.encode_shard(GEMX_TYPE_INT, sids, times, vals, seg_rows=1000)
    assert descs["rows"][:3].tolist() == [1000, 1000, 500]
    assert 1000 % 60 and 2000 % 60
    sh = gx.Shard(blob, descs, GEMX_TYPE_INT)
    try:
        dh.sweep(sh, pts, 0, 2**62, ctx="70x3")
        rows, _ = sh.scan_distinct(0, 2**62, 0)
        assert len(rows) == 70 * 5
        assert sh.distinct_stats()["levels"] >= 2
    finally:
        sh.close()


# ---- 4. the register set in front of the append ----

def _slots_with_rows(pts, seg_rows, interval, offset):
    n = 0
    for t, _ in pts.values():
        for a in range(0, len(t), seg_rows):
            seg = t[a:a + seg_rows]
            n += len(np.unique((seg - offset) // interval)) if interval else 1
    return n


def test_register_set_const_column():
    pts = _grid_series(NSER, 500, lambda sid, r: np.full(len(r), 7 * sid,
                                                         dtype=np.int64),
                       t0_fn=lambda sid: sid)
    blob, descs, ct = th.writer_shard(pts, 128)
    sh = gx.Shard(blob, descs, ct)
    try:
        dh.sweep(sh, pts, 0, 2**62, ctx="const")
        for interval, offset in dh.QUERIES:
            sh.scan_distinct(0, 2**62, interval, offset=offset)
            st = sh.distinct_stats()
            assert st["points"] == NSER * 500
            # exactly one candidate per (segment, window) that holds a row
            assert st["candidates"] == _slots_with_rows(pts, 128, interval, offset), \
                (interval, offset)
    finally:
        sh.close()


def test_register_set_overflowing_cycle():
    """40 codes in rotation: more than any allowed set size, so every row
    is appended; results are unchanged."""
    pts = _grid_series(NSER, 500, lambda sid, r: ((r + sid) % 40).astype(np.int64))
    blob, descs, ct = th.writer_shard(pts, 128)
    sh = gx.Shard(blob, descs, ct)
    try:
        dh.sweep(sh, pts, 0, 2**62, ctx="cycle40")
        sh.scan_distinct(0, 2**62, 60 * S)
        st = sh.distinct_stats()
        assert st["points"] == NSER * 500
        assert 0 < st["candidates"] <= st["points"]
    finally:
        sh.close()


# ---- 5. general-path segments ----

@pytest.mark.parametrize("ct", [GEMX_TYPE_FLOAT, GEMX_TYPE_INT], ids=["float", "int"])
def test_general_path_segments(ct):
    """Nil bitmaps, an all-nil segment, an empty block, one-value blocks, a
    snappy float block, and a query range that clips the first and last
    segment in mid-window."""
    rng = np.random.default_rng(505)
    is_f = ct == GEMX_TYPE_FLOAT
    empty_tag = 41 if is_f else 42  # BlockFloatEmpty / BlockIntegerEmpty

    def vals(n):
        v = rng.integers(0, 9, n)
        return v.astype(np.float64) * 0.5 if is_f else v.astype(np.int64)

    segs = []
    for sid in range(1, NSER + 1):
        t0 = sid * S
        plan = [("nil", 90), ("allnil", 40), ("full", 100), ("one", 1),
                ("empty", 30), ("onenil", 1), ("snappy" if is_f else "full", 70),
                ("nil", 65)]
        for kind, n in plan:
            times = t0 + np.arange(n, dtype=np.int64) * S
            t0 = int(times[-1]) + S
            v = vals(n)
            if kind == "nil":
                segs.append((sid, times, v, rng.random(n) > 0.3))
            elif kind in ("allnil", "onenil"):
                segs.append((sid, times, v, np.zeros(n, dtype=bool)))
            elif kind == "empty":
                segs.append((sid, times, v, np.zeros(n, dtype=bool),
                             bytes([empty_tag]) + n.to_bytes(4, "big")))
            elif kind == "snappy":
                segs.append((sid, times, v, np.ones(n, dtype=bool),
                             th.snappy_float_segment(v)))
            else:
                segs.append((sid, times, v, np.ones(n, dtype=bool)))
    blob, descs = th.oracle_shard(ct, segs)
    pts = th.points_of_segments(segs)
    sh = gx.Shard(blob, descs, ct)
    try:
        dh.sweep(sh, pts, 0, 2**62, ctx="general")
        # first and last segment clipped in the middle of a 60 s window
        dh.sweep(sh, pts, 31 * S + 1, 371 * S, ((60 * S, 0), (0, 0)),
                 ctx="general-clip")
    finally:
        sh.close()


# ---- 6. float edge values ----

def test_float_edge_values():
    edge = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 5e-324, -5e-324,
                     2.2250738585072014e-308, 1.5, -1.5, 0.0, -0.0])
    rng = np.random.default_rng(606)
    segs = []
    for sid in range(1, NSER + 1):
        for k in range(3):
            n = 80
            times = (k * n + np.arange(n, dtype=np.int64)) * S
            v = edge[rng.integers(0, len(edge), n)]
            if sid == 1 and k == 0:
                v[:60] = np.where(np.arange(60) % 2, -0.0, 0.0)  # window [0, 60 s)
            if sid == 2 and k == 0:
                v[:60] = np.nan                                 # an all-NaN window
            segs.append((sid, times, v, np.ones(n, dtype=bool)))
    blob, descs = th.oracle_shard(GEMX_TYPE_FLOAT, segs)
    pts = th.points_of_segments(segs)
    sh = gx.Shard(blob, descs, GEMX_TYPE_FLOAT)
    try:
        dh.sweep(sh, pts, 0, 2**62, ctx="edges")
        rows, _ = sh.scan_distinct(0, 2**62, 60 * S)
        w0 = rows[(rows["sid"] == 1) & (rows["win_start"] == 0)]
        assert len(w0) == 1 and w0["value"][0] == 0.0 and w0["time"][0] == 0
        assert not np.signbit(rows["value"][rows["value"] == 0.0]).any()
        assert not np.isnan(rows["value"]).any()
        assert not ((rows["sid"] == 2) & (rows["win_start"] == 0)).any()
        got = set(rows["value"].tolist())
        assert {np.inf, -np.inf, 5e-324, -5e-324} <= got
    finally:
        sh.close()


# ---- 7. boolean shards ----

def test_boolean_shard_equals_int_twin():
    rng = np.random.default_rng(707)
    specs = []
    for sid in range(1, NSER + 1):
        n = 400
        t = np.arange(n, dtype=np.int64) * S
        v = rng.integers(0, 2, n).astype(np.uint8)
        v[0:60] = 1         # an all-true window
        v[60:120] = 0       # an all-false window
        x = np.ones(n, dtype=np.uint8)
        x[200:300] = rng.random(100) > 0.4   # nil-bitmap segments
        if sid == 3:
            x[120:180] = 0                   # a window of nils only
        specs.append((sid, t, v, x))
    sids, times, vals, valid = bh.series_rows(specs)
    (bblob, bdescs), (iblob, idescs) = bh.build_twin(sids, times, vals, valid, 100)
    pts = {sid: (t[x.astype(bool)], v[x.astype(bool)].astype(np.int64))
           for sid, t, v, x in specs}
    bsh = gx.Shard(bblob, bdescs, GEMX_TYPE_BOOL)
    ish = gx.Shard(iblob, idescs, GEMX_TYPE_INT)
    try:
        dh.sweep(bsh, pts, 0, 2**62, ctx="bool")
        for interval, offset in dh.QUERIES:
            for grouped in (False, True):
                b, _ = bsh.scan_distinct(0, 2**62, interval, offset=offset,
                                         group_all=grouped)
                i, _ = ish.scan_distinct(0, 2**62, interval, offset=offset,
                                         group_all=grouped)
                assert b.dtype == gx.POINT_ROW_INT_DTYPE
                assert b.tobytes() == i.tobytes(), (interval, offset, grouped)
        rows, _ = bsh.scan_distinct(0, 2**62, 60 * S)
        s1 = rows[rows["sid"] == 1]
        assert s1[s1["win_start"] == 0]["value"].tolist() == [1]
        assert s1[s1["win_start"] == 60 * S]["value"].tolist() == [0]
        assert not ((rows["sid"] == 3) & (rows["win_start"] == 120 * S)).any()
    finally:
        bsh.close()
        ish.close()


# ---- 8. the grouped tree ----

def test_grouped_tree_shared_values():
    """300 series x 200 rows, values sid % 7 + row % 3: at most 9 distinct
    values per window, each shared by many series that reach it at
    different times."""
    pts = _grid_series(300, 200,
                       lambda sid, r: (sid % 7 + r % 3).astype(np.int64),
                       t0_fn=lambda sid: sid % 11)
    blob, descs, ct = th.writer_shard(pts, 100)
    sh = gx.Shard(blob, descs, ct)
    try:
        dh.sweep(sh, pts, 0, 2**62, ctx="tree")
        rows, _ = sh.scan_distinct(0, 2**62, 60 * S, group_all=True)
        assert sh.distinct_stats()["levels"] >= 2
        assert dh.max_per_output(rows) <= 9
        # the earliest-time rule, checked from the points directly
        allt = np.concatenate([t for t, _ in pts.values()])
        allv = np.concatenate([v for _, v in pts.values()])
        for r in rows[rows["win_start"] == 60 * S]:
            m = (allv == r["value"]) & (allt >= 60 * S) & (allt < 120 * S)
            assert r["time"] == allt[m].min()
            assert r["sid"] == 0
    finally:
        sh.close()


# ---- 9. the cap ----

def _ramp(first, n):
    return (np.arange(n, dtype=np.int64) * S,
            first + np.arange(n, dtype=np.int64))


def test_cap_per_series():
    for n, ok in ((2048, True), (2049, False)):
        pts = {1: _ramp(0, n)}
        blob, descs, ct = th.writer_shard(pts, 1000)
        sh = gx.Shard(blob, descs, ct)
        try:
            if ok:
                rows, _ = sh.scan_distinct(0, 2**62, 0)
                assert len(rows) == 2048
                th.assert_rows_equal(rows, dh.ref_distinct(pts, 0, 2**62, 0, 0,
                                                           False))
            else:
                with pytest.raises(gx.GemxError) as ei:
                    sh.scan_distinct(0, 2**62, 0)
                assert th.err_code(ei) == E_UNSUPPORTED
                assert "2048" in str(ei.value)
                # the same handle still answers a small query
                rows, _ = sh.scan_distinct(0, 99 * S, 60 * S)
                th.assert_rows_equal(rows, dh.ref_distinct(pts, 0, 99 * S,
                                                           60 * S, 0, False))
        finally:
            sh.close()


def test_cap_at_the_group_level():
    pts = {1: _ramp(0, 683), 2: _ramp(10000, 683), 3: _ramp(20000, 683)}
    assert sum(len(v) for _, v in pts.values()) == 2049
    blob, descs, ct = th.writer_shard(pts, 1000)
    sh = gx.Shard(blob, descs, ct)
    try:
        rows, _ = sh.scan_distinct(0, 2**62, 0)
        th.assert_rows_equal(rows, dh.ref_distinct(pts, 0, 2**62, 0, 0, False))
        with pytest.raises(gx.GemxError) as ei:
            sh.scan_distinct(0, 2**62, 0, group_all=True)
        assert th.err_code(ei) == E_UNSUPPORTED
        rows, _ = sh.scan_distinct(0, 2**62, 60 * S, group_all=True)
        th.assert_rows_equal(rows, dh.ref_distinct(pts, 0, 2**62, 60 * S, 0, True))
    finally:
        sh.close()


# ---- 10. output capacity ----

def test_out_cap_and_retry():
    pts = {1: (np.arange(300, dtype=np.int64) * S,
               (np.arange(300, dtype=np.int64) * 7) % 100)}
    blob, descs, ct = th.writer_shard(pts, 64)
    exp = dh.ref_distinct(pts, 0, 2**62, 0, 0, False)
    assert len(exp) == 100
    sh = gx.Shard(blob, descs, ct)
    try:
        with pytest.raises(gx.GemxError) as ei:
            sh.scan_distinct(0, 2**62, 0, out_cap=99)
        assert th.err_code(ei) == E_CAP
        # the raw call reports the row count a retry needs
        out = np.zeros(99, dtype=gx.POINT_ROW_DTYPE)
        n = C.c_uint64(0)
        rc = sh._lib.gemx_scan_distinct(sh._h, 0, 2**62, 0, 0, 0,
                                        out.ctypes.data_as(C.c_void_p), 99,
                                        C.byref(n), None)
        assert rc == E_CAP and n.value == 100
        exact, _ = sh.scan_distinct(0, 2**62, 0, out_cap=100)
        th.assert_rows_equal(exact, exp)
        # the default bound (8 x the aggregate row bound = 40) is too small
        # here: one retry with the reported count returns everything
        assert 8 * sh._rows_bound(0, 0, False) < 100
        rows, stats = sh.scan_distinct(0, 2**62, 0)
        th.assert_rows_equal(rows, exp)
        assert stats["n_rows"] == 100
    finally:
        sh.close()


# ---- 11. plan independence ----

def test_plan_independence():
    rng = np.random.default_rng(1111)
    pts = {sid: (np.arange(300, dtype=np.int64) * S,
                 rng.integers(0, 6, 300).astype(np.float64) * 1.5)
           for sid in range(1, NSER + 1)}
    blob, descs, ct = th.writer_shard(pts, 100)
    exp = dh.ref_distinct(pts, 0, 2**62, 60 * S, 0, False)
    expg = dh.ref_distinct(pts, 0, 2**62, 60 * S, 0, True)
    sh = gx.Shard(blob, descs, ct)
    try:
        a0 = sh.scan_agg(0, 2**62, 60 * S)[0].copy()
        g0 = sh.scan_agg(0, 2**62, 60 * S, group_all=True)[0].copy()
        # distinct queries while aggregate queries are in flight
        o1 = sh.scan_agg_begin(0, 2**62, 60 * S, buf_id=0)
        o2 = sh.scan_agg_begin(0, 2**62, 60 * S, group_all=True, buf_id=1)
        rows, _ = sh.scan_distinct(0, 2**62, 60 * S)
        th.assert_rows_equal(rows, exp)
        rows, _ = sh.scan_distinct(0, 2**62, 60 * S, group_all=True)
        th.assert_rows_equal(rows, expg)
        f1, _ = sh.scan_agg_finish(o1)
        assert f1.tobytes() == a0.tobytes()
        f2, _ = sh.scan_agg_finish(o2)
        assert f2.tobytes() == g0.tobytes()
        # a top/bottom query between two distinct queries disturbs neither
        top0 = sh.scan_topn(0, 2**62, 60 * S, 3)[0].copy()
        d1 = sh.scan_distinct(0, 2**62, 60 * S)[0].copy()
        top1 = sh.scan_topn(0, 2**62, 60 * S, 3)[0].copy()
        d2 = sh.scan_distinct(0, 2**62, 60 * S)[0].copy()
        th.assert_rows_equal(d1, exp)
        assert d1.tobytes() == d2.tobytes()
        assert top0.tobytes() == top1.tobytes()
        th.assert_rows_equal(top1, th.ref_topn(pts, 0, 2**62, 60 * S, 0, 3,
                                               "top", False))
    finally:
        sh.close()
