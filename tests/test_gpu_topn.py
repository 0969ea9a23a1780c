"""top()/bottom() selector scans on the GPU against the numpy reference
(topn_helpers.ref_topn, itself checked against the reference's golden
records in test_topn_host.py)."""

import numpy as np
import pytest

import binding as orc

import opengemini_amd as gx
from opengemini_amd.engine import (GEMX_TYPE_BOOL, GEMX_TYPE_FLOAT,
                                   GEMX_TYPE_INT)

import topn_helpers as th
from shard_helpers import build_shard

pytestmark = pytest.mark.gpu

S = th.S
NS = (1, 2, 4, 5, 16)  # both capacity classes, their edges, the maximum
NSER = 8
BIG = 2**62


def _sweep(sh, pts, start, end, queries, ns=NS, ctx=""):
    """Every (interval, offset) x n x top/bottom x per-series/grouped."""
    for interval, offset in queries:
        for n in ns:
            for sel in ("top", "bottom"):
                for grouped in (False, True):
                    rows, _ = sh.scan_topn(start, end, interval, n, sel=sel,
                                           offset=offset, group_all=grouped)
                    exp = th.ref_topn(pts, start, end, interval, offset, n,
                                      sel, grouped)
                    th.assert_rows_equal(
                        rows, exp, (ctx, interval, offset, n, sel, grouped))


QUERIES = ((60 * S, 0), (60 * S, S // 2), (7 * S, S // 2), (0, 0))


def _values(rng, kind, n):
    if kind == "walk":       # gorilla
        return np.round(np.cumsum(rng.normal(0, 1, n)) * 128) / 128
    if kind == "raw":        # full random mantissae
        return rng.random(n) * 1e6 - 5e5
    if kind == "rle":        # <= 8 distinct values
        return rng.integers(0, 6, n).astype(np.float64) * 1.5
    if kind == "const":
        return np.full(n, 42.25)
    if kind == "small":      # simple8b
        return rng.integers(0, 1000, n).astype(np.int64)
    if kind == "big":        # near-2**62 magnitudes, both signs
        return (rng.integers(0, 2**40, n).astype(np.int64) + BIG - 2**41) * \
            rng.choice(np.array([-1, 1], dtype=np.int64), n)
    raise AssertionError(kind)


def _times(rng, kind, n, sid):
    t0 = int(rng.integers(0, 50)) * S
    if kind == "grid":
        return t0 + np.arange(n, dtype=np.int64) * S
    if kind == "gaps":       # irregular: simple8b-coded deltas
        return t0 + np.cumsum(rng.integers(1, 4000, n).astype(np.int64)) * (S // 1000)
    if kind == "dt0":        # the whole series on one timestamp
        return np.full(n, t0 + sid * 11 * S, dtype=np.int64)
    if kind == "neg":
        return -400 * S + t0 + np.arange(n, dtype=np.int64) * S
    raise AssertionError(kind)


# (values, times, rows per segment, rows per series)
SWEEP = [
    ("walk", "grid", 64, 200),
    ("walk", "grid", 1, 30),        # one-row segments
    ("walk", "neg", 1000, 1300),
    ("raw", "gaps", 65, 200),
    ("raw", "grid", 1000, 1100),
    ("rle", "grid", 1000, 1500),
    ("rle", "gaps", 3, 40),
    ("const", "dt0", 3, 20),
    ("const", "grid", 64, 150),
    ("walk", "dt0", 65, 140),
    ("small", "gaps", 64, 200),
    ("small", "dt0", 3, 25),
    ("small", "grid", 1000, 1200),
    ("big", "grid", 65, 200),
    ("big", "neg", 1, 20),
]


@pytest.mark.parametrize("vk,tk,seg_rows,nrows", SWEEP,
                         ids=["%s-%s-%d" % c[:3] for c in SWEEP])
def test_codec_and_path_sweep(vk, tk, seg_rows, nrows):
    rng = np.random.default_rng(1000 + SWEEP.index((vk, tk, seg_rows, nrows)))
    pts = {}
    for sid in range(1, NSER + 1):
        n = nrows + int(rng.integers(0, 7))
        pts[sid] = (_times(rng, tk, n, sid), _values(rng, vk, n))
    blob, descs, ct = th.writer_shard(pts, seg_rows)
    sh = gx.Shard(blob, descs, ct)
    try:
        _sweep(sh, pts, -(2**62), 2**62, QUERIES, ctx=(vk, tk, seg_rows))
    finally:
        sh.close()


@pytest.mark.parametrize("case", th.load_golden(), ids=lambda c: c["name"])
def test_golden_records(case):
    """The reference's four aggregate-cursor tests, one segment per
    reference record (windows of time(4ns) span segments)."""
    for q in case["queries"]:
        ct = GEMX_TYPE_INT if q["column"] == "int" else GEMX_TYPE_FLOAT
        segs = []
        for rec in case["records"]:
            col = rec[q["column"]]
            valid = [c is not None for c in col]
            vals = np.array([0 if c is None else c for c in col],
                            dtype=np.int64 if ct == GEMX_TYPE_INT else np.float64)
            segs.append((1, rec["time"], vals, valid))
        blob, descs = th.oracle_shard(ct, segs)
        sh = gx.Shard(blob, descs, ct)
        try:
            rows, _ = sh.scan_topn(0, 100, q["interval"], case["n"],
                                   sel=case["sel"])
        finally:
            sh.close()
        assert rows["time"].tolist() == q["times"], (case["name"], q)
        assert rows["value"].tolist() == q["values"], (case["name"], q)
        assert (rows["sid"] == 1).all()
        if q["interval"]:
            assert (rows["win_start"] == rows["time"] // 4 * 4).all()
        else:
            assert (rows["win_start"] == 0).all()


@pytest.mark.parametrize("ct", [GEMX_TYPE_FLOAT, GEMX_TYPE_INT], ids=["float", "int"])
def test_nil_shard(ct):
    """20 % nil rows (bitmap segments, the scratch kernel): nil rows are
    never selected and all-nil windows emit nothing."""
    rng = np.random.default_rng(5)
    oct_ = orc.ORC_TYPE_FLOAT if ct == GEMX_TYPE_FLOAT else orc.ORC_TYPE_INT
    blob, descs, truth = build_shard(rng, oct_, list(range(1, NSER + 1)),
                                     seg_range=(2, 4), row_range=(50, 150))
    pts = {sid: (t[x], v[x]) for sid, (t, v, x) in truth.items()}
    sh = gx.Shard(blob, descs, ct)
    try:
        _sweep(sh, pts, 0, 2**62, QUERIES, ns=(1, 4, 16), ctx="nil")
        rows, _ = sh.scan_topn(0, 2**62, 2 * S, 2)
    finally:
        sh.close()
    # with 2 s windows some windows hold only nil rows: they are absent
    n_allnil = 0
    for sid, (t, v, x) in truth.items():
        w = t // (2 * S)
        for u in np.unique(w):
            n_allnil += not x[w == u].any()
    assert n_allnil > 0
    exp = th.ref_topn(pts, 0, 2**62, 2 * S, 0, 2, "top", False)
    th.assert_rows_equal(rows, exp, "all-nil windows")


def test_snappy_blocks():
    """Snappy-coded float blocks (and, on every other segment, a 10 % nil
    bitmap block beside them) decode through the scratch kernel."""
    rng = np.random.default_rng(9)
    segs = []
    for sid in range(1, NSER + 1):
        t0 = 0
        for k in range(3):
            n = int(rng.integers(60, 130))
            times = t0 + np.arange(n, dtype=np.int64) * S
            t0 = int(times[-1]) + S
            vals = _values(rng, "walk", n)
            if k == 1:
                segs.append((sid, times, vals, rng.random(n) > 0.1))
            else:
                segs.append((sid, times, vals, np.ones(n, dtype=bool),
                             th.snappy_float_segment(vals)))
    blob, descs = th.oracle_shard(GEMX_TYPE_FLOAT, segs)
    # the framed block is what the reference's reader sees as snappy floats
    d0 = descs[0]
    seg0 = blob[d0["data_offset"]: d0["data_offset"] + d0["data_size"]]
    assert seg0[0] == 31 and seg0[5] >> 4 == 2
    assert np.array_equal(orc.decode_data_segment(orc.ORC_TYPE_FLOAT, seg0)[0],
                          segs[0][2])
    pts = th.points_of_segments(segs)
    sh = gx.Shard(blob, descs, GEMX_TYPE_FLOAT)
    try:
        _sweep(sh, pts, 0, 2**62, ((60 * S, 0), (0, 0)), ns=(2, 5),
               ctx="snappy")
    finally:
        sh.close()


@pytest.fixture(scope="module")
def ties_shard():
    """Values from {0,1,2,3}: almost every selection is decided by the
    earlier-time rule; every series shares one time grid, so grouped
    selections see identical (value, time) points in different series."""
    rng = np.random.default_rng(21)
    pts_f, pts_i = {}, {}
    for sid in range(1, NSER + 1):
        t = np.arange(300, dtype=np.int64) * S
        v = rng.integers(0, 4, 300)
        pts_f[sid] = (t, v.astype(np.float64))
        pts_i[sid] = (t, v.astype(np.int64))
    return pts_f, pts_i


@pytest.mark.parametrize("kind", ["float", "int"])
def test_ties(ties_shard, kind):
    pts = ties_shard[0 if kind == "float" else 1]
    blob, descs, ct = th.writer_shard(pts, 64)
    sh = gx.Shard(blob, descs, ct)
    try:
        _sweep(sh, pts, 0, 2**62, ((60 * S, 0), (0, 0)), ctx="ties")
    finally:
        sh.close()


def test_clipping():
    """start/end strictly inside a segment and on a window boundary."""
    rng = np.random.default_rng(33)
    pts = {}
    for sid in range(1, NSER + 1):
        n = 400
        pts[sid] = (np.arange(n, dtype=np.int64) * S + (sid % 3) * S,
                    _values(rng, "walk", n))
    blob, descs, ct = th.writer_shard(pts, 100)
    sh = gx.Shard(blob, descs, ct)
    try:
        for start, end in ((37 * S + 1, 251 * S), (60 * S, 240 * S - 1),
                           (60 * S, 240 * S), (130 * S, 140 * S),
                           (1000 * S, 2000 * S)):
            _sweep(sh, pts, start, end, ((60 * S, 0), (0, 0)), ns=(1, 4, 5),
                   ctx=("clip", start, end))
            rows, _ = sh.scan_topn(start, end, 60 * S, 16)
            assert ((rows["time"] >= start) & (rows["time"] <= end)).all()
    finally:
        sh.close()


@pytest.mark.parametrize("ct", [GEMX_TYPE_FLOAT, GEMX_TYPE_INT], ids=["float", "int"])
def test_overlapping_segments(ct):
    """Two segments of a series interleaved in time."""
    rng = np.random.default_rng(44)
    segs = []
    for sid in range(1, NSER + 1):
        for rep in range(2):
            base = rep * 400 * S
            for phase in (0, 1):
                n = 90
                times = base + (np.arange(n, dtype=np.int64) * 2 + phase) * S
                vals = (_values(rng, "walk", n) if ct == GEMX_TYPE_FLOAT
                        else _values(rng, "small", n) % 7)
                segs.append((sid, times, vals, np.ones(n, dtype=bool)))
    blob, descs = th.oracle_shard(ct, segs)
    pts = th.points_of_segments(segs)
    sh = gx.Shard(blob, descs, ct)
    try:
        _sweep(sh, pts, 0, 2**62, ((60 * S, 0), (0, 0)), ns=(1, 3, 16),
               ctx="overlap")
    finally:
        sh.close()


@pytest.mark.parametrize("vk", ["walk", "small", "rle"])
def test_top1_equals_scan_agg_extrema(vk):
    """top(1)/bottom(1) are max/min with their times: bit-exact against the
    aggregate scan on the same handle, per-series and grouped."""
    rng = np.random.default_rng(55)
    pts = {}
    for sid in range(1, NSER + 1):
        n = 500
        pts[sid] = (np.arange(n, dtype=np.int64) * S, _values(rng, vk, n))
    blob, descs, ct = th.writer_shard(pts, 128)
    sh = gx.Shard(blob, descs, ct)
    try:
        for grouped in (False, True):
            agg, _ = sh.scan_agg(0, 2**62, 60 * S, group_all=grouped)
            agg = agg.copy()
            for sel, vf, tf in (("top", "max", "max_time"),
                                ("bottom", "min", "min_time")):
                rows, _ = sh.scan_topn(0, 2**62, 60 * S, 1, sel=sel,
                                       group_all=grouped)
                assert len(rows) == len(agg)
                assert np.array_equal(rows["sid"], agg["sid"])
                assert np.array_equal(rows["win_start"], agg["win_start"])
                assert np.array_equal(rows["time"], agg[tf])
                assert np.array_equal(
                    np.ascontiguousarray(rows["value"]).view(np.int64),
                    np.ascontiguousarray(agg[vf]).view(np.int64))
    finally:
        sh.close()


def test_nan_points_are_dropped():
    rng = np.random.default_rng(66)
    segs = []
    for sid in range(1, NSER + 1):
        for k in range(2):
            n = 120
            times = (k * n + np.arange(n, dtype=np.int64)) * S
            vals = _values(rng, "walk", n)
            vals[rng.integers(0, n, 6)] = np.nan
            if sid == 1 and k == 0:
                vals[60:120] = np.nan  # the whole window [60 s, 120 s)
            valid = rng.random(n) > (0.1 if sid % 2 else 0.0)
            segs.append((sid, times, vals, valid))
    blob, descs = th.oracle_shard(GEMX_TYPE_FLOAT, segs)
    pts = th.points_of_segments(segs)
    sh = gx.Shard(blob, descs, GEMX_TYPE_FLOAT)
    try:
        _sweep(sh, pts, 0, 2**62, ((60 * S, 0), (0, 0)), ns=(1, 4, 16),
               ctx="nan")
        rows, _ = sh.scan_topn(0, 2**62, 60 * S, 16)
        assert not np.isnan(rows["value"]).any()
        assert not ((rows["sid"] == 1) & (rows["win_start"] == 60 * S)).any()
    finally:
        sh.close()


def test_surface_and_plan_isolation():
    rng = np.random.default_rng(77)
    pts = {}
    for sid in range(1, NSER + 1):
        pts[sid] = (np.arange(300, dtype=np.int64) * S, _values(rng, "walk", 300))
    blob, descs, ct = th.writer_shard(pts, 100)
    sh = gx.Shard(blob, descs, ct)
    try:
        for kw in (dict(n=0), dict(n=17), dict(n=2, sel=2)):
            with pytest.raises(gx.GemxError) as ei:
                sh.scan_topn(0, 2**62, 60 * S, **kw)
            assert th.err_code(ei) == -2, kw
        rows, _ = sh.scan_topn(0, 2**62, 60 * S, 3)
        assert len(rows) == NSER * 5 * 3
        with pytest.raises(gx.GemxError) as ei:
            sh.scan_topn(0, 2**62, 60 * S, 3, out_cap=len(rows) - 1)
        assert th.err_code(ei) == -6
        exact, _ = sh.scan_topn(0, 2**62, 60 * S, 3, out_cap=len(rows))
        th.assert_rows_equal(exact, th.ref_topn(pts, 0, 2**62, 60 * S, 0, 3,
                                                "top", False))

        # the aggregate plan is not disturbed by selector queries
        a0 = sh.scan_agg(0, 2**62, 60 * S)[0].copy()
        g0 = sh.scan_agg(0, 2**62, 60 * S, group_all=True)[0].copy()
        sh.scan_topn(0, 2**62, 60 * S, 5, sel="bottom")
        sh.scan_topn(10 * S, 200 * S, 7 * S, 16, group_all=True)
        a1 = sh.scan_agg(0, 2**62, 60 * S)[0].copy()
        g1 = sh.scan_agg(0, 2**62, 60 * S, group_all=True)[0].copy()
        assert a0.tobytes() == a1.tobytes()
        assert g0.tobytes() == g1.tobytes()

        # a selector query while an async aggregate query is in flight:
        # works (or is refused with -2); the pending finish stays correct
        out = sh.scan_agg_begin(0, 2**62, 60 * S)
        try:
            rows, _ = sh.scan_topn(0, 2**62, 60 * S, 2)
            th.assert_rows_equal(rows, th.ref_topn(pts, 0, 2**62, 60 * S, 0, 2,
                                                   "top", False))
        except gx.GemxError as e:
            assert "gemx error -2" in str(e)
        fin, _ = sh.scan_agg_finish(out)
        assert fin.tobytes() == a0.tobytes()
    finally:
        sh.close()

    bt = np.arange(40, dtype=np.int64) * S
    bblob, bdescs = gx.encode_shard(GEMX_TYPE_BOOL, np.ones(40, dtype=np.uint64),
                                    bt, (bt // S) % 2)
    bsh = gx.Shard(bblob, bdescs, GEMX_TYPE_BOOL)
    try:
        with pytest.raises(gx.GemxError) as ei:
            bsh.scan_topn(0, 2**62, 60 * S, 2)
        assert th.err_code(ei) == -2
    finally:
        bsh.close()
