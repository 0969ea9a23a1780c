"""Delivery of a synchronous scan next to the pipelined one.

A synchronous call fetches its error word and rows on the compute stream;
the begin/finish pair fetches them on the copy stream so the copy can
overlap the next scan. Both use the same two result slots of a shard, so
the cases interleave them on one shard, in every order the API allows, and
require each result to equal the same call made alone on a fresh shard.
The other cases run a synchronous call right after a query whose error
word was not clean (a NaN redo, dropped gap rows): nothing of it may show
in the next result.

The error return itself is not exercised: no test sends a corrupt segment
as far as the GPU (the attach-time walk refuses them first).
"""

import functools

import numpy as np
import pytest

import binding as orc
import test_gpu_fold as tgf  # its NaN shard (_nan) and reference
from group_merge_helpers import _gap_shard, _ref as _merge_ref, assert_grouped
from shard_helpers import F

pytestmark = pytest.mark.gpu

S = 10**9
END = 2**62
IV = 60 * S
N_GROUPS = 4


def _same(a, b):
    assert a.dtype == b.dtype and len(a) == len(b), (len(a), len(b))
    for f in a.dtype.names:
        assert a[f].tobytes() == b[f].tobytes(), f


@functools.lru_cache(maxsize=None)
def _data():
    return orc.gen_shard(811, 300, 300)


def _gmap(d):
    sids = np.unique(d["sid"])
    return (np.arange(len(sids)) % N_GROUPS).astype(np.uint32)


def _shard(blob, d):
    import opengemini_amd as gx

    return gx.Shard(blob, d, F)


CALLS = {
    "grouped": lambda sh, d: sh.scan_agg(0, END, IV, group_all=True),
    "series": lambda sh, d: sh.scan_agg(0, END, IV),
    "tags": lambda sh, d: sh.scan_agg_tags(_gmap(d), N_GROUPS, 0, END, IV),
}


def _alone(blob, d, call):
    sh = _shard(blob, d)
    try:
        rows, _ = CALLS[call](sh, d)
        rows = rows.copy()
    finally:
        sh.close()
    rows.setflags(write=False)
    return rows


@pytest.fixture(params=[False, True], ids=["split", "fold"])
def fold(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("GEMX_FOLD_UNDERFILLED", "1")
    return request.param


def test_alone_calls_match_the_oracle(fold):
    blob, d = _data()
    base = orc.scan_agg(blob, d, F, 0, END, IV)
    assert_grouped(_alone(blob, d, "grouped"), orc.group_merge(base, F, IV))
    series = _alone(blob, d, "series")
    assert np.array_equal(series["sid"], base["sid"])
    assert_grouped(series, base)


def test_interleaved_with_pipelined(fold):
    blob, d = _data()
    alone = {c: _alone(blob, d, c) for c in ("grouped", "series", "tags")}
    sh = _shard(blob, d)

    def sync(call):
        rows, _ = CALLS[call](sh, d)
        _same(rows, alone[call])

    def begin(call, buf_id):
        return call, sh.scan_agg_begin(0, END, IV, group_all=call == "grouped",
                                       buf_id=buf_id)

    def finish(pending):
        call, out = pending
        rows, _ = sh.scan_agg_finish(out)
        _same(rows, alone[call])

    try:
        sync("grouped")
        b0, b1 = begin("grouped", 0), begin("series", 1)
        finish(b0)
        finish(b1)
        sync("series")
        b0 = begin("series", 0)
        finish(b0)
        sync("tags")
        b1, b0 = begin("grouped", 1), begin("grouped", 0)
        finish(b1)
        b1 = begin("series", 1)  # one still in flight: slots alternate
        finish(b0)
        finish(b1)
        sync("grouped")
        sync("tags")
        b0 = begin("grouped", 0)
        finish(b0)
        sync("series")
        sync("grouped")
    finally:
        sh.close()


def test_sync_after_nan_redo(monkeypatch):
    monkeypatch.setenv("GEMX_FOLD_UNDERFILLED", "1")
    blob, d = tgf._nan()
    ref = tgf._ref(tgf._nan)
    alone = {c: _alone(blob, d, c) for c in ("series", "tags")}  # neither folds
    sh = _shard(blob, d)
    try:
        rows, _ = sh.scan_agg(0, END, tgf.INT, group_all=True)
        assert_grouped(rows, ref)
        assert sh.fold_stats()["redone"]
        for call in ("series", "tags"):
            rows, _ = CALLS[call](sh, d)
            _same(rows, alone[call])
        rows, _ = sh.scan_agg(0, END, tgf.INT, group_all=True)
        assert_grouped(rows, ref)
        assert not sh.fold_stats()["redone"]
    finally:
        sh.close()


def test_sync_after_gaps(fold):
    blob, d = _gap_shard()
    iv = 5 * S
    ref = _merge_ref("gap")
    sh = _shard(blob, d)
    try:
        compact, _ = sh.scan_agg(0, END, iv, group_all=True)  # drops 2 gap rows
        assert_grouped(compact, ref)
        dense, _ = sh.scan_agg_grouped_fill(0, END, iv)  # same slot pair, no gaps
        assert list(dense["win_start"] // iv) == [0, 1, 2, 3, 4, 5]
        assert_grouped(dense[[0, 1, 4, 5]], ref)
        compact, _ = sh.scan_agg(0, END, iv, group_all=True)
        assert_grouped(compact, ref)
        # a range without gaps right after one with: every row is delivered
        head, _ = sh.scan_agg(0, 9 * S, iv, group_all=True)
        base = orc.scan_agg(blob, d, F, 0, 9 * S, iv)
        assert len(base) == 2 * len(np.unique(d["sid"]))
        assert_grouped(head, orc.group_merge(base, F, iv))
        series, _ = sh.scan_agg(0, 9 * S, iv)
        assert_grouped(series, base)
    finally:
        sh.close()
