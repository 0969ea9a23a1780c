"""Numpy reference and golden loader for the distinct() selector tests.

ref_distinct is checked against the reference's own expected records
(tests/golden/distinct_cases.json, test_distinct_host.py) and then serves
as the reference for the GPU tests."""

import json
import os

import numpy as np

from topn_helpers import (S, assert_rows_equal, err_code, oracle_shard,  # noqa: F401
                          point_dtype, points_of_segments,
                          snappy_float_segment, writer_shard)

HERE = os.path.dirname(os.path.abspath(__file__))

QUERIES = ((60 * S, 0), (60 * S, S // 2), (7 * S, S // 2), (0, 0))


def ref_distinct(points_by_sid, start, end, interval, offset, group_all):
    """points_by_sid: {sid: (times, values)} in descriptor order, non-nil
    rows only. Float NaN rows are dropped and -0.0 reads as 0.0 (the
    engine's documented deviations). Per (series, window) — or per window
    over all series, sid 0 — every distinct value with its minimum time,
    ordered by (time, value). Boolean values travel as int64 0/1."""
    sids = list(points_by_sid)

    def vals_of(s):
        v = np.asarray(points_by_sid[s][1])
        return v.astype(np.int64) if v.dtype.kind == "b" else v

    dt = point_dtype(vals_of(sids[0])) if sids else point_dtype(np.zeros(0))
    if group_all:
        ts = np.concatenate([np.asarray(points_by_sid[s][0], dtype=np.int64)
                             for s in sids])
        vs = np.concatenate([vals_of(s) for s in sids])
        groups = [(0, ts, vs)]
    else:
        groups = [(s, np.asarray(points_by_sid[s][0], dtype=np.int64),
                   vals_of(s)) for s in sids]
    out = []
    for sid, t, v in groups:
        m = (t >= start) & (t <= end)
        if v.dtype.kind == "f":
            m &= ~np.isnan(v)
        t, v = t[m], v[m]
        if v.dtype.kind == "f":
            v = v + 0.0
        if len(t) == 0:
            continue
        if interval:
            ws = (t - offset) // interval * interval + offset
        else:
            ws = np.full(len(t), start, dtype=np.int64)
        # all windows of the group at once: by (window, value, time), keep
        # the head of every (window, value) run — its minimum time
        o = np.lexsort((t, v, ws))
        t, v, ws = t[o], v[o], ws[o]
        head = np.concatenate([[True], (ws[1:] != ws[:-1]) | (v[1:] != v[:-1])])
        t, v, ws = t[head], v[head], ws[head]
        e = np.lexsort((v, t, ws))                # emission: (time, value)
        rows = np.zeros(len(e), dtype=dt)
        rows["sid"] = sid
        rows["win_start"] = ws[e]
        rows["time"] = t[e]
        rows["value"] = v[e]
        out.append(rows)
    return np.concatenate(out) if out else np.zeros(0, dtype=dt)


def max_per_output(rows):
    """Largest number of rows one (sid, window) output holds."""
    if len(rows) == 0:
        return 0
    key = np.stack([rows["sid"].astype(np.int64), rows["win_start"]], axis=1)
    return int(np.unique(key, axis=0, return_counts=True)[1].max())


def load_golden():
    with open(os.path.join(HERE, "golden", "distinct_cases.json")) as f:
        return json.load(f)["cases"]


def golden_points(case, vtype=np.int64):
    """{sid: (times, values)} over all records of every series."""
    pts = {}
    for ser in case["series"]:
        t = np.concatenate([np.asarray(r["time"], dtype=np.int64)
                            for r in ser["records"]])
        v = np.concatenate([np.asarray(r["int"], dtype=vtype)
                            for r in ser["records"]])
        pts[ser["sid"]] = (t, v)
    return pts


def golden_segments(case, vtype=np.int64):
    """One segment per reference record: [(sid, times, values, valid)]."""
    segs = []
    for ser in case["series"]:
        for r in ser["records"]:
            n = len(r["time"])
            segs.append((ser["sid"], np.asarray(r["time"], dtype=np.int64),
                         np.asarray(r["int"], dtype=vtype),
                         np.ones(n, dtype=bool)))
    return segs


def assert_golden_query(rows, q, ctx=""):
    assert rows["sid"].tolist() == q["sids"], (ctx, "sid")
    assert rows["win_start"].tolist() == q["win_starts"], (ctx, "win_start")
    assert rows["time"].tolist() == q["times"], (ctx, "time")
    assert rows["value"].tolist() == q["values"], (ctx, "value")


def sweep(sh, pts, start, end, queries=QUERIES, ctx=""):
    """Every (interval, offset), per series and grouped, against
    ref_distinct; returns the number of rows compared."""
    import pytest

    import opengemini_amd as gx

    n = 0
    for interval, offset in queries:
        for grouped in (False, True):
            exp = ref_distinct(pts, start, end, interval, offset, grouped)
            if max_per_output(exp) > gx.GEMX_DISTINCT_MAX:
                # the documented cap: refused loudly, never truncated
                with pytest.raises(gx.GemxError) as ei:
                    sh.scan_distinct(start, end, interval, offset=offset,
                                     group_all=grouped)
                assert err_code(ei) == -4, (ctx, interval, offset, grouped)
                continue
            rows, _ = sh.scan_distinct(start, end, interval, offset=offset,
                                       group_all=grouped)
            assert_rows_equal(rows, exp, (ctx, interval, offset, grouped))
            n += len(exp)
    return n
