"""distinct() selector scans — host-side checks (no GPU): the numpy
reference against the reference's golden records, the cross-shard merge and
the C ABI surface."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import opengemini_amd as gx
from opengemini_amd import dist as gdist

import distinct_helpers as dh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "opengemini_amd", "libgemx.so")
S = dh.S


@pytest.mark.parametrize("case", dh.load_golden(), ids=lambda c: c["name"])
def test_ref_distinct_reproduces_golden(case):
    """ref_distinct equals the reference's expected records: values, times
    and window starts, as int and as the same values in float."""
    for vtype in (np.int64, np.float64):
        pts = dh.golden_points(case, vtype)
        for q in case["queries"]:
            got = dh.ref_distinct(pts, case["start"], case["end"],
                                  q["interval"], 0, q["group_all"])
            dh.assert_golden_query(got, q, (case["name"], q["interval"]))
            assert got["value"].dtype == np.dtype(vtype)


def _shards(rng, kind, with_empty):
    """Three shards' point sets over shared windows: a tiny value alphabet
    every shard uses, so equal (window, value) pairs meet with different
    times across shards."""
    shards = []
    for k in range(3):
        pts = {}
        for sid in range(3):
            n = 0 if (with_empty and k == 1) else 50
            t = np.sort(rng.integers(0, 300, n)).astype(np.int64) * S + k
            if kind == "int":
                v = rng.integers(-2, 4, n).astype(np.int64)
            elif kind == "bool":
                v = rng.integers(0, 2, n).astype(np.int64)
            else:
                v = rng.integers(-2, 3, n).astype(np.float64) / 2
                v[v == 0.0] = np.where(rng.random((v == 0.0).sum()) < 0.5,
                                       -0.0, 0.0)
            pts[100 * k + sid] = (t, v)
        shards.append(pts)
    return shards


@pytest.mark.parametrize("with_empty", [False, True], ids=["full", "empty-shard"])
@pytest.mark.parametrize("kind", ["int", "float", "bool"])
def test_merge_distinct_equals_ref_over_union(kind, with_empty):
    rng = np.random.default_rng(17)
    shards = _shards(rng, kind, with_empty)
    union = {}
    for pts in shards:
        union.update(pts)
    if kind == "float":
        allv = np.concatenate([v for _, v in union.values()])
        assert np.signbit(allv[allv == 0.0]).any()      # -0.0 is in play
        assert (~np.signbit(allv[allv == 0.0])).any()
    for interval in (60 * S, 0):
        per_shard = [dh.ref_distinct(pts, 0, 400 * S, interval, 0, True)
                     for pts in shards]
        if with_empty:
            assert len(per_shard[1]) == 0
        got = gdist.merge_distinct(per_shard)
        exp = dh.ref_distinct(union, 0, 400 * S, interval, 0, True)
        dh.assert_rows_equal(got, exp, (kind, interval))
        assert got.dtype == per_shard[0].dtype
        assert not got["sid"].any()
        if kind == "float":
            assert not np.signbit(got["value"][got["value"] == 0.0]).any()
        # shared values: the union has fewer rows than the shards together
        assert len(got) < sum(len(r) for r in per_shard)
    # the same (window, value) with different times: the earliest wins
    a = np.zeros(2, dtype=per_shard[0].dtype)
    a["win_start"], a["time"], a["value"] = 0, [7, 9], [1, 2]
    b = a.copy()
    b["time"] = [8, 3]
    got = gdist.merge_distinct([a, b])
    assert got["time"].tolist() == [3, 7] and got["value"].tolist() == [2, 1]


def test_merge_distinct_edge_inputs():
    with pytest.raises(ValueError):
        gdist.merge_distinct([])
    empty = np.zeros(0, dtype=gx.POINT_ROW_INT_DTYPE)
    got = gdist.merge_distinct([empty, empty])
    assert len(got) == 0 and got.dtype == gx.POINT_ROW_INT_DTYPE
    nan = np.zeros(1, dtype=gx.POINT_ROW_DTYPE)
    nan["value"] = np.nan
    with pytest.raises(ValueError):
        gdist.merge_distinct([nan])


def test_header_and_python_surface():
    hdr = open(os.path.join(REPO, "include", "gemx.h")).read()
    assert re.search(r"\bint gemx_scan_distinct\(", hdr)
    assert re.search(r"\bint gemx_distinct_stats\(", hdr)
    assert re.search(r"#define GEMX_DISTINCT_MAX 2048\b", hdr)
    assert re.search(r"#define GEMX_ABI_VERSION 1\b", hdr)
    assert gx.GEMX_DISTINCT_MAX == 2048
    assert callable(gx.Shard.scan_distinct)
    assert callable(gx.Shard.distinct_stats)
    assert callable(gdist.merge_distinct)


def test_library_exports_distinct_symbols():
    if not os.path.exists(SO):
        pytest.skip("libgemx.so not built in this checkout")
    lib = C.CDLL(SO)
    assert hasattr(lib, "gemx_scan_distinct")
    assert hasattr(lib, "gemx_distinct_stats")
    # a NULL handle is refused before any device work
    lib.gemx_scan_distinct.restype = C.c_int
    lib.gemx_scan_distinct.argtypes = [
        C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int,
        C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
    out = np.zeros(4, dtype=gx.POINT_ROW_DTYPE)
    n = C.c_uint64(0)
    rc = lib.gemx_scan_distinct(None, 0, 10, 0, 0, 0,
                                out.ctypes.data_as(C.c_void_p), 4,
                                C.byref(n), None)
    assert rc == -2
    lib.gemx_distinct_stats.restype = C.c_int
    lib.gemx_distinct_stats.argtypes = [C.c_void_p] * 4
    assert lib.gemx_distinct_stats(None, None, None, None) == -2
