"""Hand-written wide gorilla streams through every user of the arena reader
other than the folded scan.

The reader reloads its word in flight only in the lanes whose cursor left
the first window word. test_gpu_gor_reader.py drives that through the folded
kernel; its shard of 128 series x 130 rows (a wave mixing j one-bit repeats
followed by 77-bit records, j = 0..63, and a wave mixing all-repeat, all-wide
and in-window 66-bit streams: lanes that never advance next to lanes that
advance every record and twice at word boundaries) is sent here through

- the per-series scan: unclipped, which on a shard this small runs one lane
  per sub-segment (k_scan_gor_sub), and with one extra series cut by the
  query's end, which makes the plan clipped and sends the 128 whole segments
  through k_scan_grid_gor<false>;
- scan_agg_tags with 4 groups;
- the grouped scan without GEMX_FOLD_UNDERFILLED: nothing folds
  (fold_stats()), the 130-row segments are split in runs of 64 rows and
  resumed (k_scan_gor_sub);
- prom_rate, scan_topn (N = 3) and scan_distinct (FloatIter: the same
  reader with the reload left in every lane, the form its callers are
  faster with).

The aggregate and rate references are the oracle's; top/bottom and distinct
use the numpy references of their own test files over the points the oracle
decodes from the streams. Counts, times, min/max/first/last and the selected
points are bit-exact, float sums within 1e-9 relative, rates within 1e-12
relative (test_gpu_parity.py's bounds). test_reference_side runs every
reference without a GPU.
"""

import functools

import numpy as np
import pytest

import binding as orc
import distinct_helpers as dh
import topn_helpers as th
from shard_helpers import F
from test_gpu_gor_reader import (END, ROWS, S, _build, _is_gorilla, _two_word,
                                 _walk, assert_grouped)
from test_gpu_parity import assert_parity

INTERVAL = 13 * S
N_GROUPS = 4
CLIP_END = (ROWS - 1) * S  # last row of the 128 series
RATE = (0, (ROWS - 1) * S, 30 * S, 10 * S)  # start, end, range, step


@functools.lru_cache(maxsize=None)
def _shard():
    blob, d, _, _ = _two_word()
    assert len(d) == 128 and np.all(d["rows"] == ROWS)
    assert all(_is_gorilla(blob, x) for x in d)
    return blob, d


@functools.lru_cache(maxsize=None)
def _shard_clipped():
    """the same 128 segments and a 129th series from t = 100 s on, which a
    query ending at CLIP_END cuts: a clipped plan with 128 whole gorilla
    segments"""
    blob, d = _shard()
    eblob, e = _build([(1000, 100 * S, _walk(np.random.default_rng(810), ROWS),
                        None)])
    e = e.copy()
    e["data_offset"] += len(blob)
    e["time_offset"] += len(blob)
    both = np.concatenate([d, e])
    assert all(_is_gorilla(blob + eblob, x) for x in both)
    return blob + eblob, both


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _points():
    """{sid: (times, values)} as the oracle decodes them"""
    blob, d = _shard()
    pts = {}
    for x in d:
        o, n = int(x["data_offset"]), int(x["data_size"])
        vals, _, rows, nils = orc.decode_data_segment(F, blob[o:o + n])
        assert rows == ROWS and nils == 0
        o, n = int(x["time_offset"]), int(x["time_size"])
        pts[int(x["sid"])] = (_frozen(orc.decode_time_segment(blob[o:o + n])),
                              _frozen(vals))
    return pts


@functools.lru_cache(maxsize=None)
def _ref(what):
    blob, d = _shard()
    if what == "series":
        return _frozen(orc.scan_agg(blob, d, F, 0, END, INTERVAL))
    if what == "clipped":
        cb, cd = _shard_clipped()
        return _frozen(orc.scan_agg(cb, cd, F, 0, CLIP_END, INTERVAL))
    if what == "grouped":
        return _frozen(orc.group_merge(_ref("series"), F, INTERVAL))
    if what == "rate":
        return _frozen(orc.prom_rate(blob, d, *RATE))
    kind, sel = what
    if kind == "topn":
        return _frozen(th.ref_topn(_points(), 0, END, INTERVAL, 0, 3, sel,
                                   False))
    assert kind == "distinct"
    return _frozen(dh.ref_distinct(_points(), 0, END, sel, 0, False))


def _gmap(d):
    return (np.arange(len(d)) % N_GROUPS).astype(np.uint32)


def _tag_refs():
    """per group: group_merge over the per-series rows of its series"""
    _, d = _shard()
    base, gmap = _ref("series"), _gmap(d)
    return [orc.group_merge(base[np.isin(base["sid"], d["sid"][gmap == g])],
                            F, INTERVAL) for g in range(N_GROUPS)]


REFS = ["series", "clipped", "grouped", "rate", ("topn", "top"),
        ("topn", "bottom"), ("distinct", INTERVAL), ("distinct", 0)]


def test_reference_side():
    pts = _points()
    assert len(pts) == 128
    wide = sum(len(np.unique(v)) == ROWS for _, v in pts.values())
    flat = sum(len(np.unique(v)) == 1 for _, v in pts.values())
    assert wide == 33 and flat == 32  # j = 0 and the 32 all-wide; all-repeat
    for what in REFS:
        assert len(_ref(what)) > 0, what
    assert len(_ref("series")) == 128 * 10
    assert np.all(_ref("grouped")["count"] == 128 * 13)
    clipped = _ref("clipped")
    assert np.sum(clipped["sid"] == 1000) == 3  # rows 100..129 s of 100..229
    assert len(clipped) == 128 * 10 + 3
    for ref in _tag_refs():
        assert len(ref) == 10 and np.all(ref["count"] == 32 * 13)
    assert np.all(np.isfinite(_ref("rate")["value"]))


def _open(blob, d):
    import opengemini_amd as gx

    return gx.Shard(blob, d, F)


@pytest.fixture
def shard(monkeypatch):
    monkeypatch.delenv("GEMX_FOLD_UNDERFILLED", raising=False)
    sh = _open(*_shard())
    yield sh
    sh.close()


@pytest.mark.gpu
def test_per_series_scan(shard):
    rows, _ = shard.scan_agg(0, END, INTERVAL)
    assert_parity(rows, _ref("series"), F)


@pytest.mark.gpu
def test_per_series_scan_clipped_plan(monkeypatch):
    monkeypatch.delenv("GEMX_FOLD_UNDERFILLED", raising=False)
    sh = _open(*_shard_clipped())
    try:
        rows, _ = sh.scan_agg(0, CLIP_END, INTERVAL)
        assert_parity(rows, _ref("clipped"), F)
    finally:
        sh.close()


@pytest.mark.gpu
def test_tags(shard):
    _, d = _shard()
    rows, _ = shard.scan_agg_tags(_gmap(d), N_GROUPS, 0, END, INTERVAL)
    rows = rows.copy()
    for g, ref in enumerate(_tag_refs()):
        assert_grouped(rows[rows["sid"] == g], ref)


@pytest.mark.gpu
def test_grouped_scan_takes_the_sub_segment_split(shard):
    rows, _ = shard.scan_agg(0, END, INTERVAL, group_all=True)
    fs = shard.fold_stats()
    assert fs["folded"] == 0 and fs["scanned"] == 128 and not fs["redone"], fs
    assert_grouped(rows, _ref("grouped"))


@pytest.mark.gpu
def test_rate(shard):
    gpu, _ = shard.prom_rate(*RATE)
    ref = _ref("rate")
    assert len(gpu) == len(ref), (len(gpu), len(ref))
    assert np.array_equal(gpu["sid"], ref["sid"])
    assert np.array_equal(gpu["ts"], ref["ts"])
    tol = 1e-12 * np.maximum(1.0, np.abs(ref["value"]))
    assert np.all(np.abs(gpu["value"] - ref["value"]) <= tol)


@pytest.mark.gpu
@pytest.mark.parametrize("sel", ["top", "bottom"])
def test_topn(shard, sel):
    rows, _ = shard.scan_topn(0, END, INTERVAL, 3, sel=sel)
    th.assert_rows_equal(rows, _ref(("topn", sel)), sel)


@pytest.mark.gpu
@pytest.mark.parametrize("interval", [INTERVAL, 0])
def test_distinct(shard, interval):
    rows, _ = shard.scan_distinct(0, END, interval)
    dh.assert_rows_equal(rows, _ref(("distinct", interval)), str(interval))
