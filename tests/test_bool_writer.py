"""Boolean columns on the host-side surface (CPU): writer rejects,
write-side pre-agg rows, gemx_rec_from_rows packing, gemx_chunkmeta_to_descs
and the cross-shard fold."""

import ctypes as C
import os

import numpy as np
import pytest

import binding as orc
from bool_helpers import (BOOL, I, S, assert_bool_rows, build_twin, odescs,
                          pack_chunkmeta, py_decode_bool_segment,
                          py_encode_bool_segment, series_rows)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "opengemini_amd", "libgemx.so")
GEMX_E_INVALID = -2
OP_COUNT, OP_SUM, OP_MIN, OP_MAX, OP_FIRST, OP_LAST = range(6)


class ColVal(C.Structure):
    _fields_ = [("val", C.c_void_p), ("bitmap", C.c_void_p),
                ("bitmap_offset", C.c_int32), ("len", C.c_int32),
                ("nil_count", C.c_int32)]


def _lib():
    if not os.path.exists(SO):
        pytest.skip("libgemx.so not built")
    lib = C.CDLL(SO)
    lib.gemx_rec_from_rows.restype = C.c_int
    lib.gemx_chunkmeta_to_descs.restype = C.c_int
    lib.gemx_encode_shard.restype = C.c_int
    return lib


def rec_from_rows(lib, rows, ops, col_type):
    r = np.ascontiguousarray(rows, dtype=orc.AGG_ROW_DTYPE)
    n, n_ops = len(r), len(ops)
    # poison the buffers: packing must not depend on their old contents
    vals = [np.full(max(n, 1) * 8, 0xEE, dtype=np.uint8) for _ in ops]
    bms = [np.full(max((n + 7) // 8, 1), 0xEE, dtype=np.uint8) for _ in ops]
    times = np.zeros(max(n, 1), dtype=np.int64)
    cols = (ColVal * n_ops)()
    vptrs = (C.c_void_p * n_ops)(*[v.ctypes.data for v in vals])
    bptrs = (C.c_void_p * n_ops)(*[b.ctypes.data for b in bms])
    opsa = (C.c_int * n_ops)(*ops)
    rc = lib.gemx_rec_from_rows(
        r.ctypes.data_as(C.c_void_p), C.c_uint64(n), opsa, n_ops,
        C.c_int(col_type), vptrs, bptrs,
        times.ctypes.data_as(C.POINTER(C.c_int64)), cols)
    return rc, vals, bms, times[:n], cols


def _twin_rows(seed=5, n=700, nil_frac=0.3):
    """Oracle rows of an int 0/1 column with nils, made boolean-shaped
    (sum blank) — what a boolean scan returns."""
    rng = np.random.default_rng(seed)
    specs = []
    for sid in (1, 2, 7):
        t = np.arange(n, dtype=np.int64) * S
        specs.append((sid, t, rng.integers(0, 2, n), rng.random(n) > nil_frac))
    # one series with an all-nil window (rows 60..119)
    x = np.ones(n, bool)
    x[60:120] = False
    specs.append((9, np.arange(n, dtype=np.int64) * S,
                  rng.integers(0, 2, n), x))
    sids, times, vals, valid = series_rows(specs)
    _, (iblob, idescs) = build_twin(sids, times, vals, valid, 250)
    rows = orc.scan_agg(iblob, odescs(idescs), I, 0, 2**62, 60 * S)
    rows["sum"] = 0
    rows["sum_isnil"] = 1
    return rows


class TestWriterRejects:
    def test_value_byte_two_is_invalid(self):
        import opengemini_amd as gx

        sids = np.ones(10, dtype=np.uint64)
        times = np.arange(10, dtype=np.int64) * S
        vals = np.zeros(10, dtype=np.uint8)
        vals[4] = 2
        with pytest.raises(gx.GemxError, match="gemx error -2"):
            gx.encode_shard(BOOL, sids, times, vals)
        with pytest.raises(gx.GemxError, match="gemx error -2"):
            gx.encode_shard(BOOL, sids, times, vals, with_preagg=True)
        # the same byte on a nil row is not a value
        valid = np.ones(10, dtype=np.uint8)
        valid[4] = 0
        gx.encode_shard(BOOL, sids, times, vals, valid)

    def test_rec_from_rows_sum_is_invalid(self):
        lib = _lib()
        rows = _twin_rows()
        rc, *_ = rec_from_rows(lib, rows, [OP_COUNT, OP_SUM], BOOL)
        assert rc == GEMX_E_INVALID
        rc, *_ = rec_from_rows(lib, rows, [OP_SUM], BOOL)
        assert rc == GEMX_E_INVALID


class TestIntTwinWriter:
    """The int64 0/1 twin is the reference for every boolean query, so the
    int writer must round-trip long runs of equal values: a run of >= 120
    zero deltas must not take simple8b selectors 0/1, which encode runs of
    the VALUE 1 (simple8b encoding.go:454-462)."""

    @pytest.mark.parametrize("run", [119, 120, 240, 500])
    def test_long_equal_runs_round_trip(self, run):
        import opengemini_amd as gx

        vals = np.concatenate([[1, 0], np.ones(run + 1), [0], np.ones(run + 1),
                               [0, 1]]).astype(np.int64)
        n = len(vals)
        sids = np.ones(n, dtype=np.uint64)
        times = np.arange(n, dtype=np.int64) * S
        blob, descs = gx.encode_shard(I, sids, times, vals, seg_rows=4096)
        seg = blob[int(descs["data_offset"][0]):
                   int(descs["data_offset"][0]) + int(descs["data_size"][0])]
        dense, _, rows, nil = orc.decode_data_segment(I, seg)
        assert rows == n and nil == 0
        assert np.array_equal(np.asarray(dense).view(np.int64)[:n], vals)


class TestWriterPreagg:
    @pytest.mark.parametrize("seg_rows", [1, 64, 400])
    def test_preagg_rows_equal_twin_scan(self, seg_rows):
        import opengemini_amd as gx

        rng = np.random.default_rng(40 + seg_rows)
        specs = []
        for sid, n in ((1, 900), (2, 65), (5, 1), (6, 130)):
            t = np.arange(n, dtype=np.int64) * S
            specs.append((sid, t, rng.integers(0, 2, n),
                          rng.random(n) > 0.3))
        specs.append((8, np.arange(70, dtype=np.int64) * S,
                      np.ones(70, np.uint8), np.zeros(70, bool)))  # all nil
        sids, times, vals, valid = series_rows(specs)
        _, (iblob, idescs) = build_twin(sids, times, vals, valid, seg_rows)
        _, _, pre = gx.encode_shard(BOOL, sids, times, vals, valid, seg_rows,
                                    with_preagg=True)
        ref = orc.scan_agg(iblob, odescs(idescs), I, -2**62, 2**62, 0)
        # win_start is rewritten when the rows are served
        fields = ("sid", "first_row_time", "count", "count_time", "sum_time",
                  "min_time", "max_time", "first_time", "last_time",
                  "min_isnil", "max_isnil", "first_isnil", "last_isnil")
        assert_bool_rows(pre, ref, fields)


class TestRecFromRowsBool:
    def test_byte_packing_bitmap_and_nil_counts(self):
        lib = _lib()
        rows = _twin_rows()
        ops = [OP_MIN, OP_MAX, OP_FIRST, OP_LAST, OP_COUNT]
        rc, vals, bms, times, cols = rec_from_rows(lib, rows, ops, BOOL)
        assert rc == 0
        n = len(rows)
        fields = {OP_MIN: "min", OP_MAX: "max", OP_FIRST: "first",
                  OP_LAST: "last"}
        assert (rows["min_isnil"] == 1).any(), "need a nil window"
        for k, op in enumerate(ops):
            if op == OP_COUNT:
                nil = rows["count"] == 0
                dense = rows["count"][~nil].astype(np.int64)
                got = vals[k].view(np.int64)[: len(dense)]  # stays int64
            else:
                nil = rows[fields[op] + "_isnil"] == 1
                dense = np.asarray(rows[fields[op]]).view(np.int64)[~nil]
                assert set(np.unique(dense)) <= {0, 1}
                got = vals[k][: len(dense)]  # ONE byte per value
                # nothing written past the dense bytes
                assert np.all(vals[k][len(dense):] == 0xEE)
            assert np.array_equal(got, dense), op
            assert cols[k].len == n and cols[k].bitmap_offset == 0
            assert cols[k].nil_count == int(nil.sum())
            bm = np.packbits((~nil).astype(np.uint8), bitorder="little")
            assert bytes(bms[k][: len(bm)]) == bm.tobytes()
        assert np.array_equal(times, rows["first_row_time"])

    def test_single_call_time(self):
        lib = _lib()
        rows = _twin_rows(seed=6)
        rc, _, _, times, _ = rec_from_rows(lib, rows, [OP_MAX], BOOL)
        assert rc == 0
        assert np.array_equal(times, rows["max_time"])


class TestChunkMetaBool:
    def test_bool_column_descs(self):
        lib = _lib()
        rng = np.random.default_rng(77)
        blob = bytearray()
        bcol, fcol, tcol, ranges, truth = [], [], [], [], []
        t0 = 0
        for rows in (200, 200, 1):
            times = t0 + np.arange(rows, dtype=np.int64) * S
            t0 = int(times[-1]) + S
            v = rng.integers(0, 2, rows).astype(np.uint8)
            x = rng.random(rows) > 0.2 if rows > 1 else np.ones(1, bool)
            bseg = py_encode_bool_segment(v, x)
            fseg = orc.encode_data_segment(
                orc.ORC_TYPE_FLOAT, rng.normal(0, 1, rows), None, rows, 0)
            tseg = orc.encode_time_segment(times)
            for col, seg in ((bcol, bseg), (fcol, fseg), (tcol, tseg)):
                col.append((len(blob), len(seg)))
                blob += seg
            ranges.append((int(times[0]), int(times[-1])))
            truth.append((v, x))
        meta = pack_chunkmeta(11, 0, len(blob), ranges,
                              [("ok", 5, b"", bcol),
                               ("value", 3, b"\x00" * 16, fcol),
                               ("time", 1, b"", tcol)])
        blob = bytes(blob)

        def parse(column, col_type):
            descs = np.zeros(8, dtype=orc.SEG_DESC_DTYPE)
            n, used = C.c_uint64(0), C.c_uint64(0)
            b = np.frombuffer(blob, dtype=np.uint8)
            m = np.frombuffer(meta, dtype=np.uint8)
            rc = lib.gemx_chunkmeta_to_descs(
                m.ctypes.data_as(C.c_void_p), len(m),
                b.ctypes.data_as(C.c_void_p), len(b), column.encode(),
                col_type, descs.ctypes.data_as(C.c_void_p), 8, C.byref(n),
                C.byref(used))
            return rc, descs[: n.value].copy(), used.value

        rc, d, used = parse("ok", BOOL)
        assert rc == 0 and used == len(meta) and len(d) == 3
        assert np.array_equal(d["rows"], [200, 200, 1])
        assert all(d["sid"] == 11)
        for k in range(3):
            assert (int(d["data_offset"][k]), int(d["data_size"][k])) == bcol[k]
            assert (int(d["time_offset"][k]), int(d["time_size"][k])) == tcol[k]
            assert (int(d["min_time"][k]), int(d["max_time"][k])) == ranges[k]
            seg = blob[bcol[k][0]: bcol[k][0] + bcol[k][1]]
            v, x = py_decode_bool_segment(seg, int(d["rows"][k]))
            assert np.array_equal(x, truth[k][1])
            assert np.array_equal(v[x], truth[k][0][truth[k][1]])
        # a boolean column is not an int or float column
        assert parse("ok", 1)[0] != 0
        assert parse("value", BOOL)[0] != 0


class TestDistFoldBool:
    def _rows(self, spec):
        """spec: list of (win_start, count, (min, t), (max, t), (first, t),
        (last, t)) -> grouped boolean rows (sum blank)."""
        rows = np.zeros(len(spec), dtype=orc.AGG_ROW_DTYPE)
        for k, (w, cnt, mn, mx, fi, la) in enumerate(spec):
            rows["win_start"][k] = w
            rows["count"][k] = cnt
            for f, (v, t) in (("min", mn), ("max", mx), ("first", fi),
                              ("last", la)):
                rows[f].view(np.int64)[k] = v  # int64 bits in the union slot
                rows[f + "_time"][k] = t
        rows["sum_isnil"] = 1
        return rows

    def test_fold_two_shards(self):
        from opengemini_amd import dist as gd

        W = 60
        # window 0: min tie on value, shard B's is earlier -> B's time wins
        # window 1: full ties (value AND time) -> rank order: shard A stays;
        #           first/last tie on time with different values shows it
        # window 2: only shard B has rows
        a = self._rows([
            (0, 10, (0, 50), (1, 5), (1, 5), (0, 59)),
            (W, 4, (0, 70), (1, 61), (1, 61), (0, 100)),
        ])
        b = self._rows([
            (0, 7, (0, 30), (1, 9), (0, 2), (1, 40)),
            (W, 6, (0, 70), (1, 61), (0, 61), (1, 100)),
            (2 * W, 3, (1, 130), (1, 130), (1, 130), (1, 140)),
        ])
        pa = gd.window_partials(a, W, 0, 0, 3, col_type=gd.TYPE_BOOL)
        pb = gd.window_partials(b, W, 0, 0, 3, col_type=gd.TYPE_BOOL)
        acc = gd._fold(pa.copy(), pb, col_type=gd.TYPE_BOOL)
        ai = acc.view(np.int64)
        assert list(acc[:, gd.C_COUNT]) == [17, 10, 3]
        assert not ai[:, gd.C_SUM].any()  # sum stays nil/zero
        # window 0
        assert (ai[0, gd.C_MIN], ai[0, gd.C_MINT]) == (0, 30)
        assert (ai[0, gd.C_MAX], ai[0, gd.C_MAXT]) == (1, 5)
        assert (ai[0, gd.C_FIRST], ai[0, gd.C_FIRSTT]) == (0, 2)
        assert (ai[0, gd.C_LAST], ai[0, gd.C_LASTT]) == (0, 59)
        # window 1: every candidate ties on time; shard A (rank 0) stays
        assert (ai[1, gd.C_MIN], ai[1, gd.C_MINT]) == (0, 70)
        assert (ai[1, gd.C_MAX], ai[1, gd.C_MAXT]) == (1, 61)
        assert (ai[1, gd.C_FIRST], ai[1, gd.C_FIRSTT]) == (1, 61)
        assert (ai[1, gd.C_LAST], ai[1, gd.C_LASTT]) == (0, 100)
        # window 2: taken from shard B, payloads bit-exact
        assert (ai[2, gd.C_MIN], ai[2, gd.C_MINT]) == (1, 130)
        assert (ai[2, gd.C_LAST], ai[2, gd.C_LASTT]) == (1, 140)
        # true must beat false in max even though 1 is a denormal as float
        c = self._rows([(0, 1, (0, 10), (0, 10), (0, 10), (0, 10))])
        d = self._rows([(0, 1, (1, 20), (1, 20), (1, 20), (1, 20))])
        acc2 = gd._fold(
            gd.window_partials(c, W, 0, 0, 1, col_type=gd.TYPE_BOOL),
            gd.window_partials(d, W, 0, 0, 1, col_type=gd.TYPE_BOOL),
            col_type=gd.TYPE_BOOL).view(np.int64)
        assert (acc2[0, gd.C_MAX], acc2[0, gd.C_MAXT]) == (1, 20)
        assert (acc2[0, gd.C_MIN], acc2[0, gd.C_MINT]) == (0, 10)
