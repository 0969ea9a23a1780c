"""k_group_p2, the cross-series merge of a grouped scan: per window, thread t
of one 256-thread block folds entries t, t + 256, ... (the p1 split entries,
then one entry per folded wave) and a 256 -> 1 tree merges the threads. The
tree's top two levels go through shared memory, the rest are shuffles inside
the first wave, so the cases put entries below one wave, past one wave, one
past the block and on no multiple of 256: 1, 65, 257 and 321 folding waves,
the last one partial.

Every GPU case compares with the oracle (scan_agg + group_merge) by
TestGroupedParity's bounds: counts, times, nil flags and min/max/first/last
bit-exact, float sums within 1e-9 relative, int sums exact. The folded
cases also assert through Shard.fold_stats() that the segments did fold.

Shards hold 26 rows at 1 s per series and are queried at 5 s: six windows,
the last one a single row. They are far below the size at which a shard
folds by default, so the folded cases attach with GEMX_FOLD_UNDERFILLED set
(as test_gpu_fold does).
"""

import numpy as np
import pytest

import binding as orc
from group_merge_helpers import (
    S, END, IV, ROWS, WAVES, LAST_LANES, BIG, SMALL, TIE_WAVES,
    TIE_MAX_TIME, TIE_MIN_TIME, _nseries, _gorilla_mask, _walk_shard,
    _int_shard, _overlap_shard, _tie_shard, _gap_shard, launch_waves, _ref,
    assert_grouped, _grouped,
)
from shard_helpers import F, I


@pytest.fixture
def fold_small(monkeypatch):
    monkeypatch.setenv("GEMX_FOLD_UNDERFILLED", "1")


# --------------------------------------------------------- reference side

def test_reference_side():
    """every builder and oracle call of this file, without a GPU"""
    for w in WAVES:
        blob, d = _walk_shard(w)
        assert len(d) == _nseries(w) and _gorilla_mask(blob, d).all()
        ref = _ref("walk", w)
        assert list(ref["count"]) == [5 * len(d)] * 5 + [len(d)]
        assert launch_waves(blob, d).max() == w - 1
        blob, d = _int_shard(w)
        ref = _ref("int", w)
        assert len(d) == _nseries(w) and int(ref["count"].sum()) == ROWS * len(d)
    blob, d = _overlap_shard()
    assert len(d) == _nseries(257) + 1
    assert int(_ref("overlap")["count"].sum()) == ROWS * len(d)
    blob, d = _walk_shard(257, False)
    assert 0 < (~_gorilla_mask(blob, d)).sum() < 64 * 4
    assert len(_ref("mixed", 257)) == 6

    blob, d = _tie_shard()
    assert len(d) == _nseries(321)
    assert len(set(((d["data_size"].astype(np.int64) - 15 + 7) // 8).tolist())) == 1
    wave = launch_waves(blob, d)
    assert np.array_equal(wave, np.arange(len(d)) // 64)
    ref = _ref("tie")
    # the planted values are the extremes and the tie goes to the earlier
    # row, not to the smaller series (waves 0 and 63 hold them one row later)
    assert ref["max"][1] == BIG and ref["max_time"][1] == TIE_MAX_TIME
    assert ref["min"][2] == SMALL and ref["min_time"][2] == TIE_MIN_TIME
    # the other windows tie as well: the planted series share their values
    base = orc.scan_agg(blob, d, F, 0, END, IV)
    for wnd in (0, 3, 4, 5):
        rows = base[base["win_start"] == wnd * IV]
        assert (rows["min"] == ref["min"][wnd]).sum() == len(TIE_WAVES)

    blob, d = _gap_shard()
    ref = _ref("gap")
    assert list(ref["win_start"] // IV) == [0, 1, 4, 5]
    assert list(ref["count"]) == [5 * _nseries(65)] * 4


# ------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
def test_folded(fold_small, waves):
    blob, d = _walk_shard(waves)
    rows, fs = _grouped(blob, d)
    assert_grouped(rows, _ref("walk", waves))
    assert fs == dict(folded=len(d), scanned=len(d), redone=False)


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
def test_unfolded_float(waves):
    """no fold switch: shards this small keep the per-segment path, and the
    merge reads p1 split entries only"""
    blob, d = _walk_shard(waves)
    rows, fs = _grouped(blob, d)
    assert_grouped(rows, _ref("walk", waves))
    assert fs == dict(folded=0, scanned=len(d), redone=False)


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
def test_unfolded_int(fold_small, waves):
    """int columns never fold, with the fold switch set as well: p1 split
    entries only, through the int instantiation of the merge"""
    blob, d = _int_shard(waves)
    rows, fs = _grouped(blob, d, I)
    assert_grouped(rows, _ref("int", waves), I)
    assert fs["folded"] == 0


@pytest.mark.gpu
def test_overlap_wave_goes_through_p1(fold_small):
    blob, d = _overlap_shard()
    rows, fs = _grouped(blob, d)
    assert_grouped(rows, _ref("overlap"))
    assert fs["scanned"] == len(d)
    # the wave that holds the overlapping series cannot fold
    assert 0 < fs["folded"] <= len(d) - LAST_LANES
    assert not fs["redone"]


@pytest.mark.gpu
def test_split_and_fold_entries(fold_small):
    blob, d = _walk_shard(257, False)
    n_gor = int(_gorilla_mask(blob, d).sum())
    rows, fs = _grouped(blob, d)
    assert_grouped(rows, _ref("mixed", 257))
    assert fs == dict(folded=n_gor, scanned=len(d), redone=False)
    assert n_gor < len(d)  # the rest reached the merge through p1


@pytest.mark.gpu
def test_ties(fold_small):
    blob, d = _tie_shard()
    ref = _ref("tie")
    rows, fs = _grouped(blob, d)
    assert_grouped(rows, ref)
    assert fs == dict(folded=len(d), scanned=len(d), redone=False)
    assert rows["max_time"][1] == TIE_MAX_TIME
    assert rows["min_time"][2] == TIE_MIN_TIME


@pytest.mark.gpu
def test_ties_unfolded():
    blob, d = _tie_shard()
    rows, fs = _grouped(blob, d)
    assert_grouped(rows, _ref("tie"))
    assert fs["folded"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("fold", [True, False])
def test_uncovered_window(monkeypatch, fold):
    if fold:
        monkeypatch.setenv("GEMX_FOLD_UNDERFILLED", "1")
    blob, d = _gap_shard()
    ref = _ref("gap")
    compact, fs = _grouped(blob, d)
    # the early segments end inside a wave; that wave holds both kinds
    assert fs["folded"] == (len(d) - 64 if fold else 0)
    assert_grouped(compact, ref)  # gaps dropped: four rows
    dense, _ = _grouped(blob, d, fill=True)
    assert list(dense["win_start"] // IV) == [0, 1, 2, 3, 4, 5]
    empty = dense[2:4]
    assert np.all(empty["count"] == 0)
    for f in ("min_isnil", "max_isnil", "first_isnil", "last_isnil", "sum_isnil"):
        assert np.all(empty[f] == 1), f
    assert_grouped(dense[[0, 1, 4, 5]], ref)
