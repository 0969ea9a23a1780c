"""The engine at production timestamps: every scan path on the time axes of
epoch_helpers (base 1.7e18 ns with a nanosecond remainder, and year 2100;
spacings from 1 s down to 7 ns, jittered, and all-equal), against both the
exact Python reference (epoch_helpers.ref_scan) and the CPU oracle, which
test_oracle_epoch.py holds to the same reference on the same axes.

Shards are 70 series (one full 64-lane wave plus a partial one) of
300 + sid % 7 rows, written by the engine's own writer. Each route case
first checks, from the block headers, that the shard holds the codecs the
route needs, and asserts the route's stat where the engine has one, so a
case cannot pass on a fallback path. Every case runs per series and
grouped, at each (interval, offset) of its spacing, over the whole shard
and over a range clipped one nanosecond inside two rows.
"""

import functools

import numpy as np
import pytest

import binding as orc
import bool_helpers as bh
import distinct_helpers as dh
import epoch_helpers as eh
import topn_helpers as th
from epoch_helpers import CORE_AXES, S
from test_gpu_fold_split import _bounds, _cuts
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

F, I, BOOL = 3, 1, 5
REG_AXES = [a for a in eh.AXES if a[1] in eh.REGULAR]
JIT_AXES = [a for a in eh.AXES if a[1].startswith("jit")]


def _ids(axes):
    return [eh.axis_id(a) for a in axes]


# -------------------------------------------------- shards and expectations

@functools.lru_cache(maxsize=None)
def _built(axis, kind, nil_frac, seg_rows):
    pts = eh.make_points(axis, kind, nil_frac)
    blob, descs, ct = eh.writer_shard(pts, seg_rows)
    return pts, blob, descs, ct


@functools.lru_cache(maxsize=None)
def _twin(axis, nil_frac, seg_rows):
    """the int64 0/1 twin of a boolean shard, for the oracle"""
    import opengemini_amd as gx

    pts = eh.make_points(axis, "bool", nil_frac)
    sids, times, vals, valid = eh.flat(pts)
    blob, descs = gx.encode_shard(I, sids, times, vals.astype(np.int64),
                                  None if valid.all() else valid, seg_rows)
    return blob, np.ascontiguousarray(descs)


@functools.lru_cache(maxsize=None)
def _expected(axis, kind, nil_frac, seg_rows, start, end, interval, offset):
    """(ref rows, ref grouped, oracle rows, oracle grouped), read-only"""
    pts, blob, descs, ct = _built(axis, kind, nil_frac, seg_rows)
    oct_ = ct
    if ct == BOOL:
        blob, descs = _twin(axis, nil_frac, seg_rows)
        oct_ = I
    ref = eh.ref_scan(pts, start, end, interval, offset, False, seg_rows)
    gref = eh.ref_scan(pts, start, end, interval, offset, True)
    orows = orc.scan_agg(blob, descs, oct_, start, end, interval, offset)
    ogrp = orc.group_merge(orows, oct_, interval)
    for a in (ref, gref, orows, ogrp):
        a.setflags(write=False)
    return ref, gref, orows, ogrp


def _ranges(axis, pts):
    return (eh.full_range(axis), eh.clip_range(pts))


def _check_rows(rows, ref, orows, ct, grouped, ctx):
    if ct == BOOL:
        eh.assert_matches_ref(rows, ref, grouped, with_sum=False, ctx=ctx)
        bh.assert_bool_rows(rows, orows, bh.GROUP_FIELDS if grouped
                            else bh.SERIES_FIELDS)
        return
    eh.assert_matches_ref(rows, ref, grouped, ctx=ctx)
    if grouped:
        eh.assert_grouped_parity(rows, orows, ct == F)
    else:
        assert_parity(rows, orows, ct)


def _sweep(sh, axis, kind, nil_frac, seg_rows, per_series=True, after=None):
    """Every (interval, offset) of the axis over the whole shard and the
    clipped range, per series and grouped. after(sh, clipped) runs behind
    each grouped scan (route stats)."""
    pts, _, _, ct = _built(axis, kind, nil_frac, seg_rows)
    multi = False
    for clipped, (start, end) in enumerate(_ranges(axis, pts)):
        for interval, offset in eh.QUERIES[axis[1]]:
            ref, gref, orows, ogrp = _expected(axis, kind, nil_frac, seg_rows,
                                               start, end, interval, offset)
            ctx = (eh.axis_id(axis), kind, seg_rows, start, end, interval,
                   offset)
            assert len(ref) > 0, ctx
            multi |= eh.has_multi_row_window(ref)
            if per_series:
                rows, _ = sh.scan_agg(start, end, interval, offset=offset)
                _check_rows(rows.copy(), ref, orows, ct, False, ctx)
            rows, _ = sh.scan_agg(start, end, interval, offset=offset,
                                  group_all=True)
            _check_rows(rows.copy(), gref, ogrp, ct, True, ctx)
            if after is not None:
                after(sh, bool(clipped), interval, offset)
    assert multi


def _attach(axis, kind, nil_frac, seg_rows):
    import opengemini_amd as gx

    _, blob, descs, ct = _built(axis, kind, nil_frac, seg_rows)
    return gx.Shard(blob, descs, ct)


def _run_route(axis, kind, nil_frac, seg_rows, want, **kw):
    """want(codes) states what the route needs of the written blocks."""
    _, blob, descs, ct = _built(axis, kind, nil_frac, seg_rows)
    codes = set(eh.seg_codes(blob, descs, ct))
    assert want(codes), codes
    sh = _attach(axis, kind, nil_frac, seg_rows)
    try:
        _sweep(sh, axis, kind, nil_frac, seg_rows, **kw)
    finally:
        sh.close()


GOR = {("full", 3, 1)}      # gorilla values on a const-delta grid


# ------------------------------------------------------------------- routes

# seg_rows 64 on every regular axis, 65 and 257 on the four core axes
GOR_CASES = [(a, 64) for a in REG_AXES] + [(a, r) for a in CORE_AXES
                                            for r in (65, 257)]


@pytest.mark.parametrize("axis,seg_rows", GOR_CASES,
                         ids=[f"{eh.axis_id(a)}-{r}" for a, r in GOR_CASES])
def test_gorilla_grid_and_sub_segment_split(axis, seg_rows):
    """k_scan_grid_gor per series; grouped, a shard this small takes the
    sub-segment split (default environment)."""
    _run_route(axis, "walk", 0.0, seg_rows, lambda c: c == GOR)


@pytest.mark.parametrize("split", [None, 1, 4])
@pytest.mark.parametrize("seg_rows", [64, 65, 257])
@pytest.mark.parametrize("axis", CORE_AXES, ids=_ids(CORE_AXES))
def test_folded_waves_and_fold_split(monkeypatch, axis, seg_rows, split):
    """Grouped scans with the wave fold forced on for a small shard, unsplit
    by policy (None) and with GEMX_FOLD_SPLIT 1 and 4."""
    monkeypatch.setenv("GEMX_FOLD_UNDERFILLED", "1")
    if split is not None:
        monkeypatch.setenv("GEMX_FOLD_SPLIT", str(split))
    _, blob, descs, _ = _built(axis, "walk", 0.0, seg_rows)
    can_fold = eh.foldable_segments(blob, descs)
    assert can_fold > 0
    seen = []

    def stats(sh, clipped, interval, offset):
        fs, ss = sh.fold_stats(), sh.fold_split_stats()
        if clipped:
            return   # boundary segments are sliced: fewer waves can fold
        seen.append((fs, ss))
        assert fs["folded"] >= can_fold and not fs["redone"], fs
        assert ss["tasks"] > 0 and ss["k_max"] >= 1, ss
        if split == 1:
            assert ss["k_max"] == 1 and ss["skipped_rows"] == 0, ss
        if split == 4 and seg_rows == 257:
            # the folding wave is the series' first segments: 257 rows
            # from the base, cut by the rule of gemx_foldsplit.hpp
            b = _bounds(eh.BASES[axis[0]], eh.STEP[axis[1]], 257, interval,
                        offset)
            assert ss["k_max"] == len(_cuts(b, 4)) - 1, ss

    _run_route(axis, "walk", 0.0, seg_rows, lambda c: c == GOR,
               per_series=False, after=stats)
    assert seen
    if split == 4 and seg_rows == 257:
        assert max(ss["k_max"] for _, ss in seen) > 1   # some wave was cut


@pytest.mark.parametrize("axis", CORE_AXES, ids=_ids(CORE_AXES))
def test_generic_grid_kernel_on_gorilla(monkeypatch, axis):
    """GEMX_DISABLE_GORK (read at attach) sends gorilla grid segments
    through the generic grid kernel."""
    monkeypatch.setenv("GEMX_DISABLE_GORK", "1")
    _run_route(axis, "walk", 0.0, 64, lambda c: c == GOR)


@pytest.mark.parametrize("kind", ["rle", "const"])
@pytest.mark.parametrize("axis", CORE_AXES, ids=_ids(CORE_AXES))
def test_generic_grid_kernel_on_rle_and_const(axis, kind):
    """Float blocks that are neither gorilla nor raw, on a const-delta
    grid: the generic grid kernel without any switch."""
    _run_route(axis, kind, 0.0, 64, lambda c: all(
        k == "full" and tag in (4, 5) and tt == 1 for k, tag, tt in c))


@pytest.mark.parametrize("axis", CORE_AXES, ids=_ids(CORE_AXES))
def test_raw_blocks(axis):
    _run_route(axis, "raw", 0.0, 64, lambda c: c == {("full", 0, 1)})


@pytest.mark.parametrize("axis", REG_AXES, ids=_ids(REG_AXES))
def test_simple8b_int_grid(axis):
    """k_scan_grid_s8b: small ints on a regular grid."""
    _run_route(axis, "int", 0.0, 64, lambda c: c == {("full", 2, 1)})


@pytest.mark.parametrize("axis", CORE_AXES, ids=_ids(CORE_AXES))
def test_bool_bit_parallel_grid(axis):
    """k_scan_bool_grid: boolean column, full blocks."""
    seen = []

    def stats(sh, clipped, interval, offset):
        seen.append(sh.bool_stats())
        assert seen[-1][0] > 0, seen[-1]

    _run_route(axis, "bool", 0.0, 64, lambda c: c == {("full", 1, 1)},
               after=stats)
    assert (350, 0) in seen   # unclipped: every segment bit-parallel


@pytest.mark.parametrize("kind", ["walk", "int"])
@pytest.mark.parametrize("axis", JIT_AXES, ids=_ids(JIT_AXES))
def test_stream_path(axis, kind):
    """Jittered times are simple8b-coded (scale 1 and 10^6): no grid."""
    _run_route(axis, kind, 0.0, 64,
               lambda c: all(k == "full" and tt == 2 for k, _, tt in c))


NIL_CASES = ([(a, k) for a in CORE_AXES + JIT_AXES for k in ("walk", "int")]
             + [(a, "bool") for a in CORE_AXES])


@pytest.mark.parametrize("axis,kind", NIL_CASES,
                         ids=[f"{eh.axis_id(a)}-{k}" for a, k in NIL_CASES])
def test_general_path_with_nils(axis, kind):
    _run_route(axis, kind, 0.2, 64,
               lambda c: all(k == "bitmap" for k, _, _ in c))


@pytest.mark.parametrize("kind,nil_frac", [("walk", 0.0), ("int", 0.0),
                                           ("walk", 0.2)])
def test_all_rows_on_one_timestamp(kind, nil_frac):
    """dt0: every row of a series at base + sid * 11 s (a const-delta grid
    of step zero; segments of a series overlap in time)."""
    _run_route(("EPOCH", "dt0"), kind, nil_frac, 64, lambda c: True)


@pytest.mark.parametrize("axis", [("EPOCH", "1s"), ("EPOCH", "7ns")],
                         ids=["EPOCH-1s", "EPOCH-7ns"])
def test_one_row_segments(axis):
    _run_route(axis, "walk", 0.0, 1, lambda c: c == {("one", None, "one")})


# ----------------------------------------------------------- other surfaces

SURFACES = [(("EPOCH", "100ms"), S), (("EPOCH", "1s"), 60 * S)]
SURF_IDS = ["EPOCH-100ms", "EPOCH-1s"]


def _bytes(a):
    return a.view(np.uint8).reshape(len(a), -1)


@pytest.mark.parametrize("axis,interval", SURFACES, ids=SURF_IDS)
def test_pipelined_equals_sync(axis, interval):
    start, end = eh.full_range(axis)
    sh = _attach(axis, "walk", 0.0, 64)
    try:
        for grouped in (False, True):
            ref, _ = sh.scan_agg(start, end, interval, group_all=grouped)
            ref = ref.copy()
            b0 = sh.scan_agg_begin(start, end, interval, group_all=grouped,
                                   buf_id=0)
            b1 = sh.scan_agg_begin(start, end, interval, group_all=grouped,
                                   buf_id=1)
            r0, _ = sh.scan_agg_finish(b0)
            r1, _ = sh.scan_agg_finish(b1)
            assert len(ref) > 0
            for r in (r0, r1):
                assert np.array_equal(_bytes(r), _bytes(ref))
    finally:
        sh.close()


def _filtered_ref(pts, passed, start, end, interval):
    fp = {s: (t[passed[s]], v[passed[s]], x[passed[s]])
          for s, (t, v, x) in pts.items()}
    return eh.ref_scan(fp, start, end, interval, 0, False)


@pytest.mark.parametrize("axis,interval", SURFACES, ids=SURF_IDS)
def test_predicates(axis, interval):
    """filter=, scan_agg_xfield with a boolean shard, scan_agg_cnf."""
    import opengemini_amd as gx

    start, end = eh.full_range(axis)
    pts, blob, descs, _ = _built(axis, "walk", 0.2, 64)
    bpts, bblob, bdescs, _ = _built(axis, "bool", 0.1, 64)
    fpts, fblob, fdescs, _ = _built(axis, "walk", 0.0, 64)
    b2pts, b2blob, b2descs, _ = _built(axis, "bool", 0.0, 64)
    vsh = gx.Shard(blob, descs, F)
    bsh = gx.Shard(bblob, bdescs, BOOL)
    fsh = gx.Shard(fblob, fdescs, F)
    b2sh = gx.Shard(b2blob, b2descs, BOOL)
    try:
        got, _ = vsh.scan_agg(start, end, interval, filter=("gt", 0.0))
        got = got.copy()
        xf, _ = vsh.scan_agg_xfield(bsh, ("eq", True), start, end, interval)
        xf = xf.copy()
        conds = [(b2sh, "eq", True, 0), (None, "gt", 0.0, 1)]
        cnf, _ = fsh.scan_agg_cnf(conds, start, end, interval)
        cnf = cnf.copy()
    finally:
        for h in (vsh, bsh, fsh, b2sh):
            h.close()
    oref = orc.scan_agg_filtered(blob, descs, F, start, end, interval, "gt",
                                 0.0)
    assert len(oref) > 0
    assert_parity(got, oref, F)
    # failing and nil rows leave the record before aggregation
    ref = _filtered_ref(pts, {s: x & (v > 0.0) for s, (t, v, x) in pts.items()},
                        start, end, interval)
    eh.assert_matches_ref(got, ref, row_time=False, ctx="filter")
    ref = _filtered_ref(
        pts, {s: bpts[s][2] & (bpts[s][1] == 1) for s in pts}, start, end,
        interval)
    assert len(ref) > 0
    eh.assert_matches_ref(xf, ref, row_time=False, ctx="xfield")
    ref = _filtered_ref(
        fpts, {s: (b2pts[s][1] == 1) & (fpts[s][1] > 0.0) for s in fpts},
        start, end, interval)
    assert len(ref) > 0
    eh.assert_matches_ref(cnf, ref, row_time=False, ctx="cnf")


@pytest.mark.parametrize("axis,interval", SURFACES, ids=SURF_IDS)
def test_series_mask_tags_and_fill(axis, interval):
    start, end = eh.full_range(axis)
    pts, blob, descs, ct = _built(axis, "walk", 0.0, 64)
    order = np.array(sorted(pts), dtype=np.uint64)
    mask = (np.arange(len(order)) % 5 < 2).astype(np.uint8)
    n_groups = 7
    gmap = (order % n_groups).astype(np.uint32)
    sh = _attach(axis, "walk", 0.0, 64)
    try:
        rows, _ = sh.scan_agg_series(mask, start, end, interval)
        rows = rows.copy()
        grows, _ = sh.scan_agg_series(mask, start, end, interval,
                                      group_all=True)
        grows = grows.copy()
        trows, _ = sh.scan_agg_tags(gmap, n_groups, start, end, interval)
        trows = trows.copy()
    finally:
        sh.close()
    base = orc.scan_agg(blob, descs, ct, start, end, interval)
    sel = base[np.isin(base["sid"], order[mask == 1])]
    assert len(sel) > 0
    assert_parity(rows, sel, F)
    eh.assert_grouped_parity(grows, orc.group_merge(sel, F, interval), True)
    mpts = {s: pts[s] for s in order[mask == 1].tolist()}
    eh.assert_matches_ref(rows, eh.ref_scan(mpts, start, end, interval, 0,
                                            False, 64), ctx="mask")
    eh.assert_matches_ref(grows, eh.ref_scan(mpts, start, end, interval, 0,
                                             True), grouped=True, ctx="mask")
    for g in range(n_groups):
        sub = base[np.isin(base["sid"], order[gmap == g])]
        got = trows[trows["sid"] == g]
        assert len(got) > 0
        eh.assert_grouped_parity(got, orc.group_merge(sub, F, interval), True)
        gpts = {s: pts[s] for s in order[gmap == g].tolist()}
        eh.assert_matches_ref(got, eh.ref_scan(gpts, start, end, interval, 0,
                                               True), grouped=True, ctx=g)
    # fill: rows 80..239 of every series removed leave windows without rows
    import opengemini_amd as gx

    keep = np.r_[0:80, 240:300]
    hpts = {s: (t[keep], v[keep], x[keep]) for s, (t, v, x) in pts.items()}
    hblob, hdescs, _ = eh.writer_shard(hpts, 64)
    sh = gx.Shard(hblob, hdescs, F)
    try:
        dense, _ = sh.scan_agg_grouped_fill(start, end, interval)
        dense = dense.copy()
        compact, _ = sh.scan_agg(start, end, interval, group_all=True)
        compact = compact.copy()
    finally:
        sh.close()
    gref = eh.ref_scan(hpts, start, end, interval, 0, True)
    eh.assert_matches_ref(compact, gref, grouped=True, ctx="fill")
    w0, w1 = int(gref["win_start"][0]), int(gref["win_start"][-1])
    assert dense["win_start"].tolist() == list(range(w0, w1 + 1, interval))
    empty = dense[dense["count"] == 0]
    assert len(empty) == len(dense) - len(compact) > 0
    assert np.all(empty["min_isnil"] == 1) and np.all(empty["sum_isnil"] == 1)
    pop = dense[dense["count"] > 0]
    assert np.array_equal(_bytes(pop), _bytes(compact))


@pytest.mark.parametrize("kind", ["walk", "int"])
@pytest.mark.parametrize("axis,interval", SURFACES, ids=SURF_IDS)
def test_preagg(axis, interval, kind):
    pts, blob, descs, ct = _built(axis, kind, 0.2, 64)
    sh = _attach(axis, kind, 0.2, 64)
    try:
        sh.preagg_build()
        for n, (start, end) in enumerate(_ranges(axis, pts)):
            pre, st = sh.scan_preagg(start, end)
            pre = pre.copy()
            ref, _ = sh.scan_agg(start, end, 0)
            assert len(pre) > 0
            assert_parity(pre, ref.copy(), ct)
            assert_parity(pre, orc.scan_agg(blob, descs, ct, start, end, 0),
                          ct)
            if n == 0:
                assert st["meta_rows"] == len(pts)   # covering: metadata only
    finally:
        sh.close()


@pytest.mark.parametrize("kind", ["walk", "int"])
@pytest.mark.parametrize("axis,interval", SURFACES, ids=SURF_IDS)
def test_topn_and_distinct(axis, interval, kind):
    pts, _, _, _ = _built(axis, kind, 0.0, 64)
    sel_pts = {s: (t, v) for s, (t, v, _) in pts.items()}
    sh = _attach(axis, kind, 0.0, 64)
    try:
        for start, end in _ranges(axis, pts):
            for n in (1, 3, 16):
                for sel in ("top", "bottom"):
                    for grouped in (False, True):
                        exp = th.ref_topn(sel_pts, start, end, interval, 0, n,
                                          sel, grouped)
                        assert len(exp) > 0
                        rows, _ = sh.scan_topn(start, end, interval, n, sel,
                                               group_all=grouped)
                        th.assert_rows_equal(rows, exp, (n, sel, grouped))
            if kind == "int":
                nrows = dh.sweep(sh, sel_pts, start, end,
                                 queries=((interval, 0), (interval, 37)))
                assert nrows > 0
    finally:
        sh.close()


@pytest.mark.parametrize("axis,interval", SURFACES, ids=SURF_IDS)
def test_downsample_write_with_preagg(axis, interval):
    """The written time column holds each window's first row time (the
    writer's documented multi-call time), so it has to equal the scan's
    first_row_time exactly and floor to the scan's window start exactly."""
    import opengemini_amd as gx

    start, end = eh.full_range(axis)
    pts, blob, descs, ct = _built(axis, "walk", 0.0, 64)
    ref = eh.ref_scan(pts, start, end, interval, 0, False, 64)
    src = _attach(axis, "walk", 0.0, 64)
    try:
        oblob, odescs, pre, out_type = src.downsample_write(
            start, end, interval, op="sum", seg_rows=16, with_preagg=True)
    finally:
        src.close()
    assert out_type == F and len(pre) == len(pts)
    odescs = np.ascontiguousarray(odescs)
    times = np.concatenate([orc.decode_time_segment(
        oblob[int(d["time_offset"]):int(d["time_offset"] + d["time_size"])])
        for d in odescs])
    sids = np.repeat(odescs["sid"], odescs["rows"])
    assert np.array_equal(sids, ref["sid"])
    assert np.array_equal(times, ref["first_row_time"])
    assert np.array_equal(eh.window_starts(times, interval, 0),
                          ref["win_start"])
    dst = gx.Shard(oblob, odescs, out_type)
    try:
        dst.set_preagg(pre)
        rows, st = dst.scan_preagg(start, end)
        rows = rows.copy()
        assert st["meta_rows"] == len(pts) and st["decode_ms"] == 0.0
        scan, _ = dst.scan_agg(start, end, 0)
        scan = scan.copy()
        again, _ = dst.scan_agg(start, end, 4 * interval)
        again = again.copy()
    finally:
        dst.close()
    assert_parity(rows, scan, F)
    assert_parity(rows, orc.scan_agg(oblob, odescs, F, start, end, 0), F)
    assert_parity(again, orc.scan_agg(oblob, odescs, F, start, end,
                                      4 * interval), F)


# --------------------------------------------------------------------- Prom

def _prom_calls(target, blob, descs, start, end, range_ns, step):
    """target: a Shard, or orc for the oracle"""
    def call(name, **kw):
        if target is orc:
            args = (blob, descs, start, end, range_ns, step)
        else:
            args = (start, end, range_ns, step)
        if name == "over_time":
            r = target.prom_over_time(*args, kw["func"])
        else:
            r = getattr(target, "prom_" + name)(*args, **kw)
        r = r[0] if isinstance(r, tuple) else r
        return r.copy()
    return call


def _prom_tolerance(name, kw, single_segment):
    """Engine against oracle, as the near-zero tests of test_gpu_parity
    have it: rate 1e-12, the Kahan sums of sum/avg 1e-9, and everything
    else bit-exact on one segment per series; where windows span segments
    stdvar/stddev and deriv/predict get 1e-9 (partial states are combined),
    and the counting, selecting, sorting and sequential functions (irate,
    quantile, mad, holt_winters) stay bit-exact."""
    if name == "rate":
        return 1e-12
    if name == "over_time":
        if kw["func"] in eh.OVER_TIME_EXACT:
            return 0
        if kw["func"] in ("sum", "avg"):
            return 1e-9
    if name in ("irate", "quantile", "holt"):
        return 0
    return 0 if single_segment else 1e-9


# one segment per series (bit-exact parity) is stated for nil-free data
PROM_DATA = [("counter", 0.0, 1000), ("counter", 0.0, 64), ("steps", 0.1, 64)]


@pytest.mark.parametrize("kind,nil_frac,seg_rows", PROM_DATA,
                         ids=["one_seg", "seg64", "seg64_nils"])
@pytest.mark.parametrize("axis", eh.PROM_AXES, ids=_ids(eh.PROM_AXES))
def test_prom_family(axis, kind, nil_frac, seg_rows):
    pts, blob, descs, _ = _built(axis, kind, nil_frac, seg_rows)
    sh = _attach(axis, kind, nil_frac, seg_rows)
    try:
        for range_ns, step in eh.PROM_GRIDS[axis[1]]:
            start, end = eh.prom_query(axis, range_ns, step)
            gpu = _prom_calls(sh, None, None, start, end, range_ns, step)
            ora = _prom_calls(orc, blob, descs, start, end, range_ns, step)
            got = {}
            for name, kw in eh.PROM_CALLS:
                key = (name, tuple(sorted(kw.items())))
                g, o = gpu(name, **kw), ora(name, **kw)
                got[key] = g
                assert len(g) == len(o) > 0, key
                assert np.array_equal(g["sid"], o["sid"]), key
                assert np.array_equal(g["ts"], o["ts"]), key
                tol = _prom_tolerance(name, kw, seg_rows >= 307)
                if tol == 0:
                    assert np.array_equal(g["value"].view(np.uint64),
                                          o["value"].view(np.uint64)), key
                elif name == "over_time" and kw["func"] in ("sum", "avg") \
                        or name == "rate":
                    err = np.abs(g["value"] - o["value"])
                    assert np.all(err <= tol * np.maximum(
                        1.0, np.abs(o["value"]))), (key, float(err.max()))
                else:   # the bar DESIGN.md states for combined states
                    assert np.all(np.isclose(g["value"], o["value"], rtol=tol,
                                             atol=1e-12)), key
            n = eh.check_prom(
                lambda name, **kw: got[(name, tuple(sorted(kw.items())))],
                pts, start, end, range_ns, step)
            assert n > 0
    finally:
        sh.close()


# ------------------------------------------------------------ stated limits

def test_refusals_are_loud():
    """What the host validates before a plan is built (time axis
    limits): each refusal is a GemxError with a message, through the
    wrapper's own sizing and, with out_cap given, from the engine."""
    import opengemini_amd as gx

    axis = ("EPOCH", "1s")
    start, end = eh.full_range(axis)
    sh = _attach(axis, "int", 0.0, 64)
    try:
        # 306 s of data in 1 ns windows: 3e11 of them
        with pytest.raises(gx.GemxError, match="1e9 windows"):
            sh.scan_agg(start, end, 1)
        for grouped in (False, True):
            with pytest.raises(gx.GemxError, match="1e9 windows"):
                sh.scan_agg(start, end, 1, group_all=grouped, out_cap=16)
        with pytest.raises(gx.GemxError, match="interval must be >= 0"):
            sh.scan_agg(start, end, -60 * S, out_cap=16)
        with pytest.raises(gx.GemxError, match="offset out of range"):
            sh.scan_agg(start, end, 60 * S, offset=2**62, out_cap=16)
        # the same interval over a range that holds 2 s of data is fine
        pts = eh.make_points(axis, "int")
        t = pts[1][0]
        rows, _ = sh.scan_agg(int(t[10]), int(t[12]), 10**7, out_cap=20000)
        ref = eh.ref_scan(pts, int(t[10]), int(t[12]), 10**7, 0, False, 64)
        eh.assert_matches_ref(rows.copy(), ref, ctx="narrow")
        # and the shard still answers an ordinary query afterwards
        rows, _ = sh.scan_agg(start, end, 60 * S)
        assert len(rows) > 0
    finally:
        sh.close()
