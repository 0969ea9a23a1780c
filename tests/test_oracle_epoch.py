"""The CPU oracle at production timestamps: orc.scan_agg (+ group_merge)
and the Prom family against the exact reference and the numpy restatements
of epoch_helpers, on every time axis (base 1.7e18 ns and year 2100, spacings
from 1 s down to 7 ns, jittered and all-equal timestamps).

The GPU tests compare the engine with this oracle, so it has to hold here
first: everything bit-exact except float sums, which hold the project's
contract 1e-9 * max(1, |ref|).
"""

import numpy as np
import pytest

import binding as orc
import epoch_helpers as eh

SEG_ROWS = 64


def _ids(axes):
    return [eh.axis_id(a) for a in axes]


@pytest.mark.parametrize("nil_frac", [0.0, 0.2], ids=["full", "nils"])
@pytest.mark.parametrize("kind", ["walk", "int"])
@pytest.mark.parametrize("axis", eh.AXES, ids=_ids(eh.AXES))
def test_scan_agg_matches_exact_reference(axis, kind, nil_frac):
    pts = eh.make_points(axis, kind, nil_frac)
    blob, descs, ct = eh.writer_shard(pts, SEG_ROWS)
    multi = False
    for start, end in (eh.full_range(axis), eh.clip_range(pts)):
        for interval, offset in eh.QUERIES[axis[1]]:
            ctx = (start, end, interval, offset)
            rows = orc.scan_agg(blob, descs, ct, start, end, interval, offset)
            ref = eh.ref_scan(pts, start, end, interval, offset, False,
                              SEG_ROWS)
            assert len(ref) > 0
            multi |= eh.has_multi_row_window(ref)
            eh.assert_matches_ref(rows, ref, ctx=ctx)
            grows = orc.group_merge(rows, ct, interval)
            gref = eh.ref_scan(pts, start, end, interval, offset, True)
            eh.assert_matches_ref(grows, gref, grouped=True, ctx=ctx)
    assert multi


def _oracle_call(blob, descs, start, end, range_ns, step):
    def call(name, **kw):
        if name == "over_time":
            return orc.prom_over_time(blob, descs, start, end, range_ns, step,
                                      kw["func"])
        fn = {"rate": orc.prom_rate, "irate": orc.prom_irate,
              "linear": orc.prom_linear, "quantile": orc.prom_quantile,
              "holt": orc.prom_holt}[name]
        return fn(blob, descs, start, end, range_ns, step, **kw)
    return call


@pytest.mark.parametrize("kind,nil_frac", [("counter", 0.0), ("steps", 0.1)])
@pytest.mark.parametrize("axis", eh.PROM_AXES, ids=_ids(eh.PROM_AXES))
def test_prom_family_matches_restatements(axis, kind, nil_frac):
    pts = eh.make_points(axis, kind, nil_frac)
    blob, descs, _ = eh.writer_shard(pts, SEG_ROWS)
    for range_ns, step in eh.PROM_GRIDS[axis[1]]:
        start, end = eh.prom_query(axis, range_ns, step)
        n = eh.check_prom(_oracle_call(blob, descs, start, end, range_ns,
                                       step), pts, start, end, range_ns, step)
        assert n > 0


def test_prom_rows_sit_on_the_expected_grid():
    axis = ("EPOCH", "1s")
    pts = eh.make_points(axis, "counter")
    blob, descs, _ = eh.writer_shard(pts, SEG_ROWS)
    start, end = eh.prom_query(axis, 300 * eh.S, 60 * eh.S)
    rows = orc.prom_rate(blob, descs, start, end, 300 * eh.S, 60 * eh.S)
    grid = eh.prom_grid(start, end, 300 * eh.S, 60 * eh.S)
    assert grid[0] == eh.EPOCH - 17 + 300 * eh.S and len(grid) == 6
    assert set(rows["ts"].tolist()) <= set(grid)
    assert rows["ts"][0] == grid[0]


@pytest.mark.parametrize("axis", eh.CORE_AXES, ids=_ids(eh.CORE_AXES))
def test_written_shards_have_the_shapes_the_gpu_routes_need(axis):
    """What test_gpu_epoch.py relies on, checked where no GPU is needed:
    the writer's codec choice per value kind, and that the walk shards hold
    a launch wave the grouped scan can fold."""
    want = {"walk": {("full", 3, 1)}, "raw": {("full", 0, 1)},
            "int": {("full", 2, 1)}, "bool": {("full", 1, 1)}}
    for kind, codes in want.items():
        blob, descs, ct = eh.writer_shard(eh.make_points(axis, kind), 64)
        assert set(eh.seg_codes(blob, descs, ct)) == codes, kind
    for seg_rows, n in ((64, 64), (65, 64), (257, 12)):
        blob, descs, _ = eh.writer_shard(eh.make_points(axis, "walk"),
                                         seg_rows)
        assert eh.foldable_segments(blob, descs) == n, seg_rows
