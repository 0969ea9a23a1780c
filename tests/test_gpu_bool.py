"""Boolean field columns on the GPU: bit-parallel scan, general path,
predicates, the scan surface, downsample and malformed-input rejection.

Reference: the CPU oracle on the int twin — the same rows written as an
int64 0/1 column with identical segment cuts (bool_helpers.build_twin).
The boolean reducers are instances of the integer templates, so a boolean
query returns the int twin's rows field by field, with sum blank (0, nil).
Cross-field and CNF cases use numpy ground truth from the authored inputs.
"""

import functools

import numpy as np
import pytest

import binding as orc
from bool_helpers import (BOOL, GROUP_FIELDS, I, INT, S, assert_bool_rows,
                          build_twin, odescs, series_rows)

pytestmark = pytest.mark.gpu

F = orc.ORC_TYPE_FLOAT
FAR = 2**62
PATTERNS = ["all_true", "all_false", "false_at_window_end", "true_at_row0",
            "random"]


def gx():
    import opengemini_amd

    return opengemini_amd


def pattern(name, t, rng, interval=INT):
    n = len(t)
    if name == "all_true":
        return np.ones(n, np.uint8)
    if name == "all_false":
        return np.zeros(n, np.uint8)
    if name == "true_at_row0":
        v = np.zeros(n, np.uint8)
        v[0] = 1
        return v
    if name == "false_at_window_end":
        # the single false sits on the last row of the first window that
        # ends inside the series (else on the last row)
        v = np.ones(n, np.uint8)
        w = t // interval
        ends = np.nonzero(w[1:] != w[:-1])[0]
        v[ends[0] if len(ends) else n - 1] = 0
        return v
    return rng.integers(0, 2, n).astype(np.uint8)


def scan_both(sh, iblob, idescs, start, end, interval, offset=0):
    """per-series and grouped rows of one query, checked against the twin."""
    ref = orc.scan_agg(iblob, odescs(idescs), I, start, end, interval, offset)
    got, _ = sh.scan_agg(start, end, interval, offset)
    assert_bool_rows(got.copy(), ref)
    stats = sh.bool_stats()
    if interval:
        grp, _ = sh.scan_agg(start, end, interval, offset, group_all=True)
        assert_bool_rows(grp.copy(), orc.group_merge(ref, I, interval),
                         GROUP_FIELDS)
        assert sh.bool_stats() == stats
    return ref, stats


# ---------------------------------------------------------------- 6 ------

SEG_ROWS = [1, 7, 8, 9, 63, 64, 65, 128, 1000]


def grid_shard(seg_rows, t0_s, dt=S):
    """8 all-valid const-delta series, every segment exactly seg_rows rows:
    the five patterns plus three random series on shifted starts."""
    rng = np.random.default_rng(seg_rows * 7 + t0_s)
    n = 5 if seg_rows == 1 else 3 * seg_rows
    specs = []
    for k in range(8):
        t0 = t0_s * S + (k - 4) * 64 * S * (k >= 5)
        t = t0 + np.arange(n, dtype=np.int64) * dt
        specs.append((k + 1, t, pattern(PATTERNS[k % 5] if k < 5 else "random",
                                        t, rng), None))
    return series_rows(specs)


@pytest.mark.parametrize("t0_s", [0, 56])  # 56 s: row 64 opens a window
@pytest.mark.parametrize("seg_rows", SEG_ROWS)
def test_bitparallel_parity(seg_rows, t0_s):
    """t0 = 0 puts the 60 s window boundaries mid-word (rows 60, 120, ...);
    t0 = 56 s puts one exactly on the word boundary at row 64. interval
    200 s gives windows wider than three words; offset 0.5 s is not a
    multiple of dt. Every segment is eligible, so bool_stats must report
    all of them as bit-parallel."""
    sids, times, vals, valid = grid_shard(seg_rows, t0_s)
    (bblob, bdescs), (iblob, idescs) = build_twin(sids, times, vals, valid,
                                                  seg_rows)
    sh = gx().Shard(bblob, bdescs, BOOL)
    try:
        for interval, offset in ((INT, 0), (200 * S, 0), (INT, S // 2)):
            _, stats = scan_both(sh, iblob, idescs, 0, FAR, interval, offset)
            assert stats == (len(bdescs), 0), (interval, offset)
    finally:
        sh.close()


@pytest.mark.parametrize("seg_rows", [9, 65, 130])
def test_bitparallel_all_rows_one_timestamp(seg_rows):
    """dt = 0: every row of a series shares one timestamp."""
    rng = np.random.default_rng(600 + seg_rows)
    specs = []
    for k in range(8):
        t = np.full(130, (1000 + 61 * k) * S, dtype=np.int64)
        specs.append((k + 1, t, pattern(PATTERNS[k % 5], t, rng), None))
    sids, times, vals, valid = series_rows(specs)
    (bblob, bdescs), (iblob, idescs) = build_twin(sids, times, vals, valid,
                                                  seg_rows)
    sh = gx().Shard(bblob, bdescs, BOOL)
    try:
        _, stats = scan_both(sh, iblob, idescs, 0, FAR, INT)
        assert stats == (len(bdescs), 0)
    finally:
        sh.close()


# ---------------------------------------------------------------- 7 ------

@functools.lru_cache(maxsize=None)
def nil_shard(jitter):
    """30 % nils, an all-nil segment, an all-nil series, one-row series
    (valid and nil), windows spanning segment boundaries (seg_rows 250 vs
    60 s windows); jitter=True makes the timestamps irregular."""
    rng = np.random.default_rng(700 + jitter)
    specs = []
    for k in range(5):
        n = 700
        t = (k * 17 * S) + np.arange(n, dtype=np.int64) * S
        if jitter:
            t = t + np.sort(rng.integers(0, 900_000_000, n))
        x = rng.random(n) > 0.3
        if k == 1:
            x[250:500] = False  # an all-nil segment
        specs.append((k + 1, t, rng.integers(0, 2, n), x))
    t = np.arange(300, dtype=np.int64) * S
    specs.append((10, t, rng.integers(0, 2, 300), np.zeros(300, bool)))
    specs.append((11, np.array([90 * S]), [1], [True]))   # one row, valid
    specs.append((12, np.array([95 * S]), [1], [False]))  # one row, nil
    specs.append((13, np.array([30 * S, 40 * S]), [0, 1], None))  # raw times
    rows = series_rows(specs)
    return rows, build_twin(*rows, 250)


@pytest.mark.parametrize("jitter", [False, True])
def test_general_path_parity(jitter):
    _, ((bblob, bdescs), (iblob, idescs)) = nil_shard(jitter)
    sh = gx().Shard(bblob, bdescs, BOOL)
    try:
        _, stats = scan_both(sh, iblob, idescs, 0, FAR, INT)
        assert sum(stats) == len(bdescs) and stats[1] > 0
        # interval 0: one window per series, nothing bit-parallel
        _, stats = scan_both(sh, iblob, idescs, 0, FAR, 0)
        assert stats == (0, len(bdescs))
        # a range cutting segments mid-way (and mid-second)
        lo, hi = 100 * S + 300_000_000, 500 * S
        _, stats = scan_both(sh, iblob, idescs, lo, hi, INT)
        in_range = int(((bdescs["max_time"] >= lo) &
                        (bdescs["min_time"] <= hi)).sum())
        assert sum(stats) == in_range
        scan_both(sh, iblob, idescs, lo, hi, 0)
    finally:
        sh.close()


# ---------------------------------------------------------------- 8 ------

@functools.lru_cache(maxsize=None)
def surface_shard():
    """64 all-valid series, 3 segments x 400 rows (every eighth series has
    one), staggered starts, a gap before the third segment that leaves the
    windows 900..1080 s empty in every series."""
    rng = np.random.default_rng(800)
    specs = []
    for k in range(64):
        t0 = (k % 4) * 30 * S
        t = t0 + np.arange(1200, dtype=np.int64) * S
        t[800:] += 300 * S
        if k % 8 == 7:
            t = t[:400]
        v = rng.integers(0, 2, len(t)).astype(np.uint8)
        if k % 3 == 0:
            v[:] = rng.random(len(t)) < 0.02  # mostly false: min ties abound
        specs.append((k + 1, t, v, None))
    rows = series_rows(specs)
    twin = build_twin(*rows, 400)
    (iblob, idescs) = twin[1]
    base = orc.scan_agg(iblob, odescs(idescs), I, 0, FAR, INT)
    return rows, twin, base


class TestSurface:
    def test_tags_with_empty_group_and_ties(self):
        _, ((bblob, bdescs), _), base = surface_shard()
        order = np.arange(1, 65)
        gmap = np.array([0, 1, 2, 4], dtype=np.uint32)[(order - 1) % 4]
        sh = gx().Shard(bblob, bdescs, BOOL)
        try:
            rows, _ = sh.scan_agg_tags(gmap, 5, 0, FAR, INT)
            rows = rows.copy()
        finally:
            sh.close()
        assert not (rows["sid"] == 3).any()  # the empty group emits nothing
        tie = False
        for g in (0, 1, 2, 4):
            sub = base[np.isin(base["sid"], order[gmap == g])]
            ref = orc.group_merge(sub, I, INT)
            assert_bool_rows(rows[rows["sid"] == g], ref, GROUP_FIELDS)
            # a cross-series min tie: the winning (value, time) occurs in
            # more than one series of the group
            for r in ref[:3]:
                m = sub[(sub["win_start"] == r["win_start"]) &
                        (sub["min"].view(np.int64) == r["min"].view(np.int64))
                        & (sub["min_time"] == r["min_time"])]
                tie |= len(m) > 1
        assert tie

    def test_series_subset(self):
        _, ((bblob, bdescs), _), base = surface_shard()
        mask = (np.arange(64) % 3 == 1).astype(np.uint8)
        keep = np.arange(1, 65)[mask == 1]
        sh = gx().Shard(bblob, bdescs, BOOL)
        try:
            rows, _ = sh.scan_agg_series(mask, 0, FAR, INT)
            rows = rows.copy()
            grp, _ = sh.scan_agg_series(mask, 0, FAR, INT, group_all=True)
            grp = grp.copy()
        finally:
            sh.close()
        ref = base[np.isin(base["sid"], keep)]
        assert_bool_rows(rows, ref)
        assert_bool_rows(grp, orc.group_merge(ref, I, INT), GROUP_FIELDS)

    def test_grouped_fill_and_async(self):
        _, ((bblob, bdescs), _), base = surface_shard()
        sh = gx().Shard(bblob, bdescs, BOOL)
        try:
            dense, _ = sh.scan_agg_grouped_fill(0, FAR, INT)
            dense = dense.copy()
            compact, _ = sh.scan_agg(0, FAR, INT, group_all=True)
            compact = compact.copy()
            per, _ = sh.scan_agg(0, FAR, INT)
            per = per.copy()
            # begin/finish equals the sync result, two in flight
            b0 = sh.scan_agg_begin(0, FAR, INT, buf_id=0)
            b1 = sh.scan_agg_begin(0, FAR, INT, group_all=True, buf_id=1)
            a0 = sh.scan_agg_finish(b0)[0].copy()
            a1 = sh.scan_agg_finish(b1)[0].copy()
            with pytest.raises(gx().GemxError, match="float column"):
                sh.prom_rate(0, 2000 * S, 300 * S, 60 * S)
        finally:
            sh.close()
        raw = lambda r: r.view(np.uint8).reshape(len(r), -1)
        assert np.array_equal(raw(a0), raw(per))
        assert np.array_equal(raw(a1), raw(compact))
        assert_bool_rows(per, base)
        assert_bool_rows(compact, orc.group_merge(base, I, INT), GROUP_FIELDS)
        empt = dense[dense["count"] == 0]
        assert np.array_equal(empt["win_start"], np.array([15, 16, 17]) * INT)
        for f in ("min_isnil", "max_isnil", "first_isnil", "last_isnil",
                  "sum_isnil"):
            assert np.all(empt[f] == 1), f
        assert np.array_equal(raw(dense[dense["count"] > 0]), raw(compact))

    def test_preagg_mixed_coverage(self):
        _, ((bblob, bdescs), (iblob, idescs)), _ = surface_shard()
        sh = gx().Shard(bblob, bdescs, BOOL)
        try:
            for lo, hi in ((-10**15, 1000 * S), (50 * S, 10**15)):
                pre, st = sh.scan_preagg(lo, hi)
                pre = pre.copy()
                ref = orc.scan_agg(iblob, odescs(idescs), I, lo, hi, 0)
                assert_bool_rows(pre, ref)
                assert 0 < st["meta_rows"] < 64, (lo, hi)
        finally:
            sh.close()

    def test_write_side_preagg_serves_without_scan(self):
        (sids, times, vals, valid), (_, (iblob, idescs)), _ = surface_shard()
        blob, descs, pre = gx().encode_shard(BOOL, sids, times, vals, valid,
                                             400, with_preagg=True)
        sh = gx().Shard(blob, np.ascontiguousarray(descs), BOOL)
        try:
            sh.set_preagg(pre)
            rows, st = sh.scan_preagg(-FAR, FAR)
            rows = rows.copy()
        finally:
            sh.close()
        assert st["meta_rows"] == 64 and st["decode_ms"] == 0.0
        assert_bool_rows(rows,
                         orc.scan_agg(iblob, odescs(idescs), I, -FAR, FAR, 0))


# ---------------------------------------------------------------- 9 ------

class TestPredicates:
    @pytest.mark.parametrize("which", ["nils", "grid"])
    def test_own_column(self, which):
        if which == "nils":
            _, ((bblob, bdescs), (iblob, idescs)) = nil_shard(False)
        else:
            _, ((bblob, bdescs), (iblob, idescs)), _ = surface_shard()
        sh = gx().Shard(bblob, bdescs, BOOL)
        try:
            for op, operand, ival in (("eq", 1, 1), ("neq", 1, 1),
                                      ("eq", True, 1), ("eq", False, 0)):
                got, _ = sh.scan_agg(0, FAR, INT, filter=(op, operand))
                ref = orc.scan_agg_filtered(iblob, odescs(idescs), I, 0, FAR,
                                            INT, op, ival)
                assert_bool_rows(got.copy(), ref)
                assert sh.bool_stats()[0] == 0  # predicate: nothing bit-parallel
            mask = np.ones(len(np.unique(bdescs["sid"])), np.uint8)
            got, _ = sh.scan_agg_series(mask, 0, FAR, INT, filter=("neq", 0))
            ref = orc.scan_agg_filtered(iblob, odescs(idescs), I, 0, FAR, INT,
                                        "neq", 0)
            assert_bool_rows(got.copy(), ref)
            with pytest.raises(gx().GemxError, match="gemx error -2"):
                sh.scan_agg(0, FAR, INT, filter=("gt", 1))
            for op, operand in (("gt", 1), ("le", 0), ("eq", 2)):
                with pytest.raises(gx().GemxError, match="gemx error -2"):
                    _raw_filter(sh, op, operand)
        finally:
            sh.close()

    def _build_fields(self, seed, n_series=24, pts=900):
        rng = np.random.default_rng(seed)
        n = n_series * pts
        sids = np.repeat(np.arange(1, n_series + 1, dtype=np.uint64), pts)
        times = np.tile(np.arange(pts, dtype=np.int64) * S, n_series)
        cols = dict(
            vals=np.round(np.cumsum(rng.normal(0, 1, n)) * 128) / 128,
            vvalid=(rng.random(n) > 0.2).astype(np.uint8),
            ok=rng.integers(0, 2, n).astype(np.uint8),
            okvalid=(rng.random(n) > 0.2).astype(np.uint8),
            lvl=rng.integers(0, 6, n).astype(np.int64),
            lvlvalid=(rng.random(n) > 0.2).astype(np.uint8),
        )
        enc = gx().encode_shard
        shards = dict(
            v=enc(F, sids, times, cols["vals"], cols["vvalid"], 400),
            ok=enc(BOOL, sids, times, cols["ok"], cols["okvalid"], 400),
            lvl=enc(I, sids, times, cols["lvl"], cols["lvlvalid"], 400),
        )
        return sids, times, cols, shards

    @staticmethod
    def _expect(sids, times, vals, vvalid, passmask):
        rows = []
        for sid in np.unique(sids):
            m = (sids == sid) & passmask
            st, sv, sx = times[m], vals[m], vvalid[m].astype(bool)
            wins = (st // INT) * INT
            for w in np.unique(wins):
                vv = sv[(wins == w) & sx]
                rows.append((int(sid), int(w), vv))
        return rows

    @staticmethod
    def _check(got, exp):
        assert len(got) == len(exp), (len(got), len(exp))
        for r, (sid, w, vv) in zip(got, exp):
            assert int(r["sid"]) == sid and int(r["win_start"]) == w
            assert int(r["count"]) == len(vv)
            if len(vv):
                assert abs(r["sum"] - vv.sum()) <= 1e-9 * max(1, abs(vv.sum()))
                assert r["min"] == vv.min() and r["max"] == vv.max()
                assert r["first"] == vv[0] and r["last"] == vv[-1]
            else:
                assert r["min_isnil"] and r["max_isnil"]

    def test_bool_filter_shard_xfield(self):
        sids, times, c, shards = self._build_fields(901)
        vsh = gx().Shard(shards["v"][0], np.ascontiguousarray(shards["v"][1]), F)
        osh = gx().Shard(shards["ok"][0], np.ascontiguousarray(shards["ok"][1]),
                         BOOL)
        try:
            g1 = vsh.scan_agg_xfield(osh, ("eq", True), 0, FAR, INT)[0].copy()
            g2 = vsh.scan_agg_xfield(osh, ("eq", True), 0, FAR, INT)[0].copy()
            g3 = vsh.scan_agg_xfield(osh, ("neq", True), 0, FAR, INT)[0].copy()
            with pytest.raises(gx().GemxError, match="gemx error -2"):
                vsh.scan_agg_xfield(osh, ("ge", True), 0, FAR, INT)
        finally:
            vsh.close()
            osh.close()
        okv = c["okvalid"].astype(bool)
        self._check(g1, self._expect(sids, times, c["vals"], c["vvalid"],
                                     okv & (c["ok"] == 1)))
        raw = lambda r: r.view(np.uint8).reshape(len(r), -1)
        assert np.array_equal(raw(g1), raw(g2))  # cached bitmap
        self._check(g3, self._expect(sids, times, c["vals"], c["vvalid"],
                                     okv & (c["ok"] != 1)))

    def test_cnf_mixing_bool_float_int(self):
        """(ok == true) AND (value > 0 OR level == 3)"""
        sids, times, c, shards = self._build_fields(902)
        mk = lambda k, ct: gx().Shard(shards[k][0],
                                      np.ascontiguousarray(shards[k][1]), ct)
        vsh, osh, lsh = mk("v", F), mk("ok", BOOL), mk("lvl", I)
        try:
            got = vsh.scan_agg_cnf(
                [(osh, "eq", True, 0), (None, "gt", 0.0, 1),
                 (lsh, "eq", 3, 1)], 0, FAR, INT)[0].copy()
        finally:
            for s in (vsh, osh, lsh):
                s.close()
        pm = (c["okvalid"].astype(bool) & (c["ok"] == 1)) & (
            (c["vvalid"].astype(bool) & (c["vals"] > 0)) |
            (c["lvlvalid"].astype(bool) & (c["lvl"] == 3)))
        self._check(got, self._expect(sids, times, c["vals"], c["vvalid"], pm))


def _raw_filter(sh, op, operand):
    """scan_agg_ex with the operand passed through unconverted (the Python
    layer maps any truthy operand to 1; the C ABI must refuse 2 itself)."""
    import ctypes as C

    out = np.zeros(4096, dtype=gx().engine.AGG_ROW_DTYPE)
    n = C.c_uint64(0)
    rc = sh._lib.gemx_scan_agg_ex(
        sh._h, 0, FAR, INT, 0, 0, sh.FILTER_OPS[op], 0.0, int(operand),
        out.ctypes.data_as(C.c_void_p), len(out), C.byref(n), None)
    gx().engine._check(rc, sh._lib)


# --------------------------------------------------------------- 10 ------

class TestDownsample:
    W5 = 300 * S

    def _pair(self):
        _, ((bblob, bdescs), (iblob, idescs)) = nil_shard(False)
        return (gx().Shard(bblob, bdescs, BOOL),
                gx().Shard(iblob, idescs, gx().engine.GEMX_TYPE_INT))

    def test_max_writes_a_boolean_column(self):
        bsh, ish = self._pair()
        try:
            oblob, od = bsh.downsample_write(0, FAR, INT, op="max")
            tblob, td = ish.downsample_write(0, FAR, INT, op="max")
        finally:
            bsh.close()
            ish.close()
        assert np.array_equal(od["rows"], td["rows"])
        out = gx().Shard(oblob, np.ascontiguousarray(od), BOOL)
        try:
            got = out.scan_agg(0, FAR, self.W5)[0].copy()
        finally:
            out.close()
        assert_bool_rows(got, orc.scan_agg(tblob, odescs(td), I, 0, FAR,
                                           self.W5))

    def test_count_writes_an_int_column(self):
        bsh, ish = self._pair()
        try:
            oblob, od, _, out_type = bsh.downsample_write(
                0, FAR, INT, op="count", with_preagg=True)
            tblob, td = ish.downsample_write(0, FAR, INT, op="count")
            with pytest.raises(gx().GemxError, match="gemx error -2"):
                bsh.downsample_write(0, FAR, INT, op="sum")
        finally:
            bsh.close()
            ish.close()
        assert out_type == gx().engine.GEMX_TYPE_INT
        out = gx().Shard(oblob, np.ascontiguousarray(od), out_type)
        try:
            got = out.scan_agg(0, FAR, self.W5)[0].copy()
        finally:
            out.close()
        ref = orc.scan_agg(tblob, odescs(td), I, 0, FAR, self.W5)
        assert len(got) == len(ref)
        for f in got.dtype.names:
            if f != "_pad":
                assert np.array_equal(np.asarray(got[f]).view(np.int64)
                                      if got[f].dtype.kind == "f" else got[f],
                                      np.asarray(ref[f]).view(np.int64)
                                      if ref[f].dtype.kind == "f" else ref[f]), f


# --------------------------------------------------------------- 11 ------

class TestMalformedRejectedAtAttach:
    """Host-side validation: nothing malformed reaches a kernel."""

    def _valid(self):
        rng = np.random.default_rng(1100)
        sids = np.ones(100, dtype=np.uint64)
        times = np.arange(100, dtype=np.int64) * S
        blob, descs = gx().encode_shard(BOOL, sids, times,
                                        rng.integers(0, 2, 100))
        descs = np.ascontiguousarray(descs)
        assert len(descs) == 1 and blob[int(descs["data_offset"][0])] == 33
        return bytearray(blob), descs

    def _refused(self, blob, descs):
        with pytest.raises(gx().GemxError, match="gemx error -2"):
            gx().Shard(bytes(blob), descs, BOOL).close()

    def test_valid_baseline_attaches(self):
        blob, descs = self._valid()
        gx().Shard(bytes(blob), descs, BOOL).close()

    def test_encoding_nibble_two(self):
        blob, descs = self._valid()
        blob[int(descs["data_offset"][0]) + 5] = 0x20
        self._refused(blob, descs)

    def test_full_block_count_differs_from_rows(self):
        blob, descs = self._valid()
        blob[int(descs["data_offset"][0]) + 9] = 99  # count u32be low byte
        self._refused(blob, descs)

    def test_payload_one_byte_short(self):
        blob, descs = self._valid()
        descs["data_size"][0] -= 1
        self._refused(blob, descs)

    def test_float_type_byte(self):
        blob, descs = self._valid()
        blob[int(descs["data_offset"][0])] = 31
        self._refused(blob, descs)
