"""top()/bottom() selector scans — host-side checks (no GPU): the numpy
reference against the reference's golden records, the C ABI surface, the
record assembly and the cross-shard merge."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import opengemini_amd as gx
from opengemini_amd import dist as gdist
from opengemini_amd import engine as ge

import topn_helpers as th

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", th.load_golden(), ids=lambda c: c["name"])
def test_ref_topn_reproduces_golden(case):
    """ref_topn equals the reference's expected records on all four
    aggregate-cursor tests (int and float, no interval and time(4ns))."""
    assert len(case["queries"]) == 4
    for q in case["queries"]:
        t, v, x = th.golden_points(case, q["column"])
        got = th.ref_topn({1: (t[x], v[x])}, 0, 100, q["interval"], 0,
                          case["n"], case["sel"], False)
        assert got["time"].tolist() == q["times"], (case["name"], q)
        assert got["value"].tolist() == q["values"], (case["name"], q)
        # one series: the grouped result holds the same points
        grp = th.ref_topn({1: (t[x], v[x])}, 0, 100, q["interval"], 0,
                          case["n"], case["sel"], True)
        assert grp["time"].tolist() == q["times"]
        assert grp["value"].tolist() == q["values"]
        assert not grp["sid"].any()


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(REPO, "include", "gemx.h")).read()
    assert re.search(r"\bint gemx_scan_topn\(", hdr)
    assert re.search(r"\bint gemx_rec_from_points\(", hdr)
    for name, val in (("GEMX_SEL_TOP", 0), ("GEMX_SEL_BOTTOM", 1),
                      ("GEMX_TOPN_MAX", 16)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr), name
    assert "gemx_point_row" in hdr
    assert re.search(r"#define GEMX_ABI_VERSION 1\b", hdr)
    lib = ge._load()
    assert lib.gemx_scan_topn is not None
    assert lib.gemx_rec_from_points is not None
    assert ge.POINT_ROW_DTYPE.itemsize == 32
    assert ge.POINT_ROW_INT_DTYPE.itemsize == 32


def test_scan_topn_null_handle_is_invalid():
    lib = ge._load()
    out = np.zeros(4, dtype=ge.POINT_ROW_DTYPE)
    n = C.c_uint64(0)
    rc = lib.gemx_scan_topn(None, 0, 10, 0, 0, 0, 0, 2,
                            out.ctypes.data_as(C.c_void_p), 4, C.byref(n), None)
    assert rc == -2
    assert lib.gemx_last_error()


@pytest.mark.parametrize("col_type", [ge.GEMX_TYPE_INT, ge.GEMX_TYPE_FLOAT])
def test_rec_from_points_packs_record(col_type):
    lib = ge._load()
    n = 11  # not a multiple of 8: the bitmap's last byte is partial
    is_int = col_type == ge.GEMX_TYPE_INT
    rows = np.zeros(n, dtype=ge.POINT_ROW_INT_DTYPE if is_int
                    else ge.POINT_ROW_DTYPE)
    rows["sid"] = 7
    rows["win_start"] = np.arange(n) // 3 * 60
    rows["time"] = 1000 + np.arange(n) * 5
    if is_int:
        rows["value"] = np.arange(n, dtype=np.int64) * -(2**40) + 3
    else:
        rows["value"] = np.arange(n) * 0.25 - 1.0
    vals = np.full(n + 2, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)  # poisoned
    bm = np.full((n + 7) // 8 + 1, 0xA5, dtype=np.uint8)
    times = np.full(n + 2, -77, dtype=np.int64)
    cv = ge._ColVal()
    rc = lib.gemx_rec_from_points(
        rows.ctypes.data_as(C.c_void_p), n, col_type,
        vals.ctypes.data_as(C.c_void_p), bm.ctypes.data_as(C.c_void_p),
        times.ctypes.data_as(C.c_void_p), C.byref(cv))
    assert rc == 0
    got = vals[:n].view(np.int64 if is_int else np.float64)
    assert np.array_equal(got, rows["value"])
    assert np.array_equal(times[:n], rows["time"])
    # nothing written past the n rows
    assert (vals[n:] == 0x5A5A5A5A5A5A5A5A).all()
    assert (times[n:] == -77).all()
    assert bm[-1] == 0xA5
    bits = np.unpackbits(bm[: (n + 7) // 8], bitorder="little")
    assert bits[:n].all() and not bits[n:].any()
    assert cv.len == n and cv.nil_count == 0 and cv.bitmap_offset == 0
    assert cv.val == vals.ctypes.data and cv.bitmap == bm.ctypes.data
    # boolean columns have no top/bottom
    assert lib.gemx_rec_from_points(
        rows.ctypes.data_as(C.c_void_p), n, ge.GEMX_TYPE_BOOL,
        vals.ctypes.data_as(C.c_void_p), bm.ctypes.data_as(C.c_void_p),
        times.ctypes.data_as(C.c_void_p), C.byref(cv)) == -2


def test_python_surface_exists():
    assert callable(gx.Shard.scan_topn)
    assert callable(gdist.merge_topn)
    assert gx.POINT_ROW_DTYPE.names == ("sid", "win_start", "time", "value")


def _synthetic_shards(rng, n_shards, kind):
    """Per-shard point sets over shared windows: values from a tiny alphabet
    (selections decided by the earlier-time rule), one sparse window."""
    shards = []
    for k in range(n_shards):
        pts = {}
        for sid in range(3):
            t = np.sort(rng.integers(0, 300, 40)).astype(np.int64) * th.S
            # window [300 s, 360 s): fewer than n points over all shards
            if k < 2 and sid == 0:
                t = np.concatenate([t, [310 * th.S + k]])
            if kind == "int":
                v = rng.integers(0, 4, len(t)).astype(np.int64)
            else:
                v = rng.integers(0, 4, len(t)).astype(np.float64) / 2
            pts[100 * k + sid] = (t, v)
        shards.append(pts)
    return shards


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("n_shards", [2, 8])
@pytest.mark.parametrize("sel", ["top", "bottom"])
def test_merge_topn_equals_ref_over_union(kind, n_shards, sel):
    rng = np.random.default_rng(11 + n_shards)
    shards = _synthetic_shards(rng, n_shards, kind)
    union = {}
    for pts in shards:
        union.update(pts)
    for n in (1, 3, 5):
        for interval in (60 * th.S, 0):
            per_shard = [th.ref_topn(pts, 0, 400 * th.S, interval, 0, n, sel, True)
                         for pts in shards]
            got = gdist.merge_topn(per_shard, n, sel)
            exp = th.ref_topn(union, 0, 400 * th.S, interval, 0, n, sel, True)
            th.assert_rows_equal(got, exp, (kind, n_shards, sel, n, interval))
            if interval:
                sparse = exp[exp["win_start"] == 300 * th.S]
                assert len(sparse) == min(n, 2)  # fewer than n points
    # value ties are resolved by time: the kept points of a tied value are
    # its earliest ones
    exp = th.ref_topn(union, 0, 400 * th.S, 60 * th.S, 0, 3, sel, True)
    w0 = exp[exp["win_start"] == 0]
    assert len(np.unique(w0["value"])) == 1
    allt = np.concatenate([t[(t < 60 * th.S)] for t, _ in union.values()])
    allv = np.concatenate([v[(t < 60 * th.S)] for t, v in union.values()])
    best = allv.max() if sel == "top" else allv.min()
    assert w0["value"][0] == best
    assert w0["time"].tolist() == np.sort(allt[allv == best])[:3].tolist()
