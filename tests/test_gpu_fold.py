"""Grouped wave fold: aligned gorilla waves reduced inside the scan kernel
must give the rows of the per-segment partial path.

Every case compares gemx_scan_agg_grouped with oracle scan_agg +
group_merge using TestGroupedParity's comparator (count, times, nil flags,
min/max/first/last bit-exact; float sum within 1e-9 relative), and the
cases that say so also assert fold coverage through Shard.fold_stats() —
without it they could pass with the fold path never running.

Shapes are the smallest that still reach every path: more than one wave, a
partial last wave, waves that do not fold, windows that straddle a segment
boundary, and the NaN redo. Shards this small normally run the sub-segment
split instead of folding (it fills the chip better below 65536 gorilla
segments), so the cases attach with GEMX_FOLD_UNDERFILLED set; the kernel
path is the one large shards take by default, which
TestFullScaleParity covers at the benchmark's size.
"""

import functools
import struct

import numpy as np
import pytest

import binding as orc
from shard_helpers import INT, F

pytestmark = pytest.mark.gpu

S = 10**9
END = 2**62
GORILLA_TAG = 3  # outer float codec tag (high nibble of the codec byte)


@pytest.fixture(autouse=True)
def _fold_small_shards(monkeypatch):
    monkeypatch.setenv("GEMX_FOLD_UNDERFILLED", "1")


# ---------------------------------------------------------------- builders

def _walk(rng, n):
    return np.round(np.cumsum(rng.normal(0, 1, n)) * 128) / 128


def _py_gorilla(vals):
    """Minimal tsm1 gorilla stream writer for the one input the reference
    writer refuses (a NaN value): every changed value is written with the
    `new window` control bits. Same layout as orc.gorilla_encode."""
    uvnan = 0x7FF8000000000001
    bits = []

    def put(v, n):
        bits.extend((v >> (n - 1 - i)) & 1 for i in range(n))

    words = [struct.unpack("<Q", struct.pack("<d", float(v)))[0] for v in vals]
    prev = words[0]
    for cur in words[1:] + [uvnan]:
        x = cur ^ prev
        prev = cur
        if x == 0:
            put(0, 1)
            continue
        lead = min(64 - x.bit_length(), 31)
        trail = (x & -x).bit_length() - 1
        sig = 64 - lead - trail
        put(0b11, 2)
        put(lead, 5)
        put(sig & 0x3F, 6)  # 64 significant bits are written as 0
        put(x >> trail, sig)
    bits.extend([0] * (-len(bits) % 8))
    body = bytes(
        int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8)
    )
    return bytes([1 << 4]) + struct.pack(">Q", words[0]) + body


def _data_segment(vals, valid=None):
    rows = len(vals)
    if valid is None:
        if np.isnan(vals).any():
            # full-block header of an ordinary segment of the same length,
            # then the gorilla codec byte and the hand-written stream
            head = orc.encode_data_segment(
                F, np.arange(rows, dtype=np.float64) * 0.5 + 0.25, None, rows, 0
            )[:5]
            return head + bytes([GORILLA_TAG << 4]) + _py_gorilla(vals)
        return orc.encode_data_segment(F, vals, None, rows, 0)
    bm = np.packbits(valid.astype(np.uint8), bitorder="little")
    return orc.encode_data_segment(F, vals[valid], bm, rows, int((~valid).sum()))


def _build(series):
    """series: list of (sid, [(t0_ns, dt_ns, vals, valid|None), ...])"""
    blob = bytearray()
    descs = []
    for sid, segs in series:
        for t0, dt, vals, valid in segs:
            rows = len(vals)
            times = t0 + np.arange(rows, dtype=np.int64) * dt
            dseg = _data_segment(np.asarray(vals, dtype=np.float64), valid)
            tseg = orc.encode_time_segment(times)
            descs.append((sid, len(blob), len(dseg), rows, len(blob) + len(dseg),
                          len(tseg), 0, int(times[0]), int(times[-1])))
            blob += dseg + tseg
    d = np.zeros(len(descs), dtype=orc.SEG_DESC_DTYPE)
    for i, tup in enumerate(descs):
        d[i] = tup
    return bytes(blob), d


def _is_gorilla(blob, desc):
    return blob[int(desc["data_offset"]) + 5] >> 4 == GORILLA_TAG


@functools.lru_cache(maxsize=None)
def _aligned(t0=0):
    """case-1 shape: 200 series x 1 segment x 300 rows, same t0, 1 s step:
    3 full waves plus one of 8 lanes."""
    rng = np.random.default_rng(700)
    return _build([(sid, [(t0, S, _walk(rng, 300), None)])
                   for sid in range(1, 201)])


@functools.lru_cache(maxsize=None)
def _ties():
    rng = np.random.default_rng(701)
    series = []
    for sid in range(1, 151):
        run = int(rng.integers(4, 11))   # run length differs per series, so
        n = 300 // run + 1              # stream lengths (arena order) do too
        vals = np.repeat(rng.integers(0, 3, n).astype(np.float64), run)[:300]
        series.append((sid, [(0, S, vals, None)]))
    return _build(series)


def _iwalk(rng, n):
    """integer-valued walk: still gorilla-coded, but its XORs carry long
    zero tails, so its streams are shorter than _walk's"""
    return np.round(np.cumsum(rng.normal(0, 3, n)))


@functools.lru_cache(maxsize=None)
def _mixed():
    """The stream arena (= launch order) is sorted by stream length, so the
    100 aligned series get the longest streams: they then fill the end of
    the launch list and its last wave holds aligned segments only."""
    rng = np.random.default_rng(702)
    series = []
    sid = 1
    for _ in range(100):  # aligned
        series.append((sid, [(0, S, _walk(rng, 300), None)]))
        sid += 1
    for k in range(40):  # shifted by 7 s, or 250 rows: waves not aligned
        if k % 2:
            series.append((sid, [(7 * S, S, _iwalk(rng, 300), None)]))
        else:
            series.append((sid, [(0, S, _iwalk(rng, 250), None)]))
        sid += 1
    for _ in range(20):  # two disjoint 90-row segments; window 1 straddles
        series.append((sid, [(0, S, _iwalk(rng, 90), None),
                             (90 * S, S, _iwalk(rng, 90), None)]))
        sid += 1
    for _ in range(10):  # nulls: general kernel
        valid = rng.random(300) > 0.2
        series.append((sid, [(0, S, _walk(rng, 300), valid)]))
        sid += 1
    blob, d = _build(series)
    assert d["data_size"][:100].min() > d["data_size"][100:180].max() + 8
    return blob, d


@functools.lru_cache(maxsize=None)
def _overlap():
    rng = np.random.default_rng(703)
    series = []
    for sid in range(1, 71):
        if sid == 30:  # second segment starts inside the first one's span
            series.append((sid, [(0, S, _walk(rng, 300), None),
                                 (100 * S + S // 2, S, _walk(rng, 300), None)]))
        else:
            series.append((sid, [(0, S, _walk(rng, 300), None)]))
    return _build(series)


@functools.lru_cache(maxsize=None)
def _nan():
    """130 aligned series; the last one (series index 129) has NaN as the
    first value of its third window. The oracle folds series in order, so a
    NaN minimum arriving last never replaces the running one; the unfolded
    device merge has one lane per series here and drops that lane's NaN at
    its first tree step in the same way."""
    rng = np.random.default_rng(704)
    series = []
    for sid in range(1, 131):
        vals = _walk(rng, 300)
        if sid == 130:
            vals[120] = np.nan
        series.append((sid, [(0, S, vals, None)]))
    return _build(series)


@functools.lru_cache(maxsize=None)
def _ref(builder, t0=None, start=0, end=END, offset=0):
    blob, d = builder() if t0 is None else builder(t0)
    base = orc.scan_agg(blob, d, F, start, end, INT, offset)
    ref = orc.group_merge(base, F, INT)
    ref.setflags(write=False)
    return ref


# ---------------------------------------------------------------- compare

def assert_grouped(gpu_rows, ref):
    assert len(gpu_rows) == len(ref), (len(gpu_rows), len(ref))
    for f in ("win_start", "count", "min_time", "max_time", "first_time",
              "last_time", "min_isnil", "max_isnil", "first_isnil",
              "last_isnil", "sum_isnil"):
        assert np.array_equal(gpu_rows[f], ref[f]), f
    for f in ("min", "max", "first", "last"):
        assert np.array_equal(
            gpu_rows[f].view(np.uint64), ref[f].view(np.uint64)
        ), f
    tol = 1e-9 * np.maximum(1.0, np.abs(ref["sum"]))
    both_nan = np.isnan(gpu_rows["sum"]) & np.isnan(ref["sum"])
    assert np.all(both_nan | (np.abs(gpu_rows["sum"] - ref["sum"]) <= tol))


def _shard(blob, d):
    import opengemini_amd as gx

    return gx.Shard(blob, d, F)


def _grouped(blob, d, start=0, end=END, offset=0):
    sh = _shard(blob, d)
    try:
        rows, _ = sh.scan_agg(start, end, INT, offset=offset, group_all=True)
        return rows.copy(), sh.fold_stats()
    finally:
        sh.close()


# ------------------------------------------------------------------- cases

def test_aligned_with_tail():
    blob, d = _aligned()
    assert all(_is_gorilla(blob, x) for x in d)
    rows, fs = _grouped(blob, d)
    assert_grouped(rows, _ref(_aligned))
    assert fs == dict(folded=200, scanned=200, redone=False)


def test_ties():
    blob, d = _ties()
    assert all(_is_gorilla(blob, x) for x in d)
    assert len({int(x["data_size"]) for x in d}) > 10  # arena != series order
    ref = _ref(_ties)
    # the input really has cross-series and in-series ties to resolve
    assert np.all(ref["min"] == 0.0) and np.all(ref["max"] == 2.0)
    rows, fs = _grouped(blob, d)
    assert_grouped(rows, ref)
    assert fs["folded"] == 150 and not fs["redone"]


def test_mixed():
    blob, d = _mixed()
    rows, fs = _grouped(blob, d)
    assert_grouped(rows, _ref(_mixed))
    assert fs["scanned"] == len(d) == 190
    assert sum(_is_gorilla(blob, x) for x in d[:180]) == 180
    # 180 gorilla segments = waves of 64, 64 and 52; only the last holds
    # aligned segments alone
    assert fs["folded"] == 52
    assert not fs["redone"]


def test_overlap_is_never_folded():
    blob, d = _overlap()
    rows, fs = _grouped(blob, d)
    assert_grouped(rows, _ref(_overlap))
    # 71 segments in two waves; the overlapping series sits in one of them
    # (which therefore cannot fold), so at most the other wave folds and
    # never a segment of that series
    assert fs["scanned"] == 71
    assert fs["folded"] in (0, 71 - 64, 64)
    assert not fs["redone"]


def test_nan_redo(monkeypatch):
    blob, d = _nan()
    assert all(_is_gorilla(blob, x) for x in d)
    ref = _ref(_nan)
    assert np.isnan(ref["sum"][2]) and not np.isnan(ref["min"]).any()
    sh = _shard(blob, d)
    try:
        rows, _ = sh.scan_agg(0, END, INT, group_all=True)
        rows = rows.copy()
        first = sh.fold_stats()
        again, _ = sh.scan_agg(0, END, INT, group_all=True)
        again = again.copy()
        second = sh.fold_stats()
    finally:
        sh.close()
    monkeypatch.setenv("GEMX_DISABLE_FOLD", "1")
    sh = _shard(blob, d)
    try:
        plain, _ = sh.scan_agg(0, END, INT, group_all=True)
        plain = plain.copy()
        off = sh.fold_stats()
    finally:
        sh.close()
    assert first["redone"] and first["folded"] == 0
    assert not second["redone"] and second["folded"] == 0  # plan stays unfolded
    assert off == dict(folded=0, scanned=130, redone=False)
    for got in (rows, again):
        assert_grouped(got, plain)  # the contract: same rows as unfolded
        for f in ("count", "min", "max", "first", "last", "min_time",
                  "max_time", "first_time", "last_time"):
            assert np.array_equal(got[f].view(np.uint64),
                                  plain[f].view(np.uint64)), f
    assert_grouped(rows, ref)


def test_plan_sharing():
    blob, d = _aligned()
    ref = _ref(_aligned)
    sh = _shard(blob, d)
    try:
        g1, _ = sh.scan_agg(0, END, INT, group_all=True)
        g1 = g1.copy()
        assert sh.fold_stats()["folded"] == 200
        per, _ = sh.scan_agg(0, END, INT)  # same plan, must write partials
        per = per.copy()
        g2, _ = sh.scan_agg(0, END, INT, group_all=True)
        g2 = g2.copy()
        assert sh.fold_stats()["folded"] == 200
        # pipelined, both buffers in flight
        b0 = sh.scan_agg_begin(0, END, INT, group_all=True, buf_id=0)
        b1 = sh.scan_agg_begin(0, END, INT, group_all=True, buf_id=1)
        a0, _ = sh.scan_agg_finish(b0)
        a0 = a0.copy()
        a1, _ = sh.scan_agg_finish(b1)
        a1 = a1.copy()
        # clipped range on the same shard: boundary segments are sliced by
        # the general kernel, nothing may fold
        clip, _ = sh.scan_agg(100 * S, 199 * S, INT, group_all=True)
        clip = clip.copy()
        clip_fs = sh.fold_stats()
    finally:
        sh.close()
    assert_grouped(g1, ref)
    assert_grouped(g2, ref)
    for f in g1.dtype.names:  # fixed reduce order: identical run to run
        assert np.array_equal(g1[f], g2[f]), f
        assert np.array_equal(g1[f], a0[f]), f
        assert np.array_equal(g1[f], a1[f]), f
    base = orc.scan_agg(blob, d, F, 0, END, INT)
    assert len(per) == len(base)
    for f in ("sid", "win_start", "count", "min_time", "max_time",
              "first_time", "last_time"):
        assert np.array_equal(per[f], base[f]), f
    for f in ("min", "max", "first", "last"):
        assert np.array_equal(per[f].view(np.uint64), base[f].view(np.uint64)), f
    assert np.all(np.abs(per["sum"] - base["sum"])
                  <= 1e-9 * np.maximum(1.0, np.abs(base["sum"])))
    assert_grouped(clip, _ref(_aligned, None, 100 * S, 199 * S))
    assert clip_fs["folded"] == 0 and clip_fs["scanned"] == 200


def test_pipelined_nan_redo():
    """Both in-flight queries hit the NaN counter; each finish redoes its
    own slot."""
    blob, d = _nan()
    sh = _shard(blob, d)
    try:
        b0 = sh.scan_agg_begin(0, END, INT, group_all=True, buf_id=0)
        b1 = sh.scan_agg_begin(0, END, INT, group_all=True, buf_id=1)
        a0, _ = sh.scan_agg_finish(b0)
        a0 = a0.copy()
        r0 = sh.fold_stats()["redone"]
        a1, _ = sh.scan_agg_finish(b1)
        a1 = a1.copy()
    finally:
        sh.close()
    assert r0
    assert_grouped(a0, _ref(_nan))
    assert_grouped(a1, _ref(_nan))


@pytest.mark.parametrize("offset", [0, 7 * S])
def test_offset_and_negative_time(offset):
    blob, d = _aligned(-150 * S)
    rows, fs = _grouped(blob, d, start=-(2**62), offset=offset)
    assert_grouped(rows, _ref(_aligned, -150 * S, -(2**62), END, offset))
    assert fs == dict(folded=200, scanned=200, redone=False)


def test_split_sized_shard_keeps_the_split_by_default(monkeypatch):
    monkeypatch.delenv("GEMX_FOLD_UNDERFILLED")
    blob, d = _aligned()
    rows, fs = _grouped(blob, d)
    assert_grouped(rows, _ref(_aligned))
    assert fs == dict(folded=0, scanned=200, redone=False)


def test_default_folds_a_full_grid(monkeypatch):
    """No switch set: from 65536 gorilla segments up there is no
    sub-segment split and aligned waves fold by default (66,000 one-segment
    series x 120 rows: 1031 full waves and one of 16 lanes)."""
    monkeypatch.delenv("GEMX_FOLD_UNDERFILLED")
    blob, d = orc.gen_shard(49, 66_000, 120)
    rows, fs = _grouped(blob, d)
    base = orc.scan_agg(blob, d, F, 0, END, INT, nthreads=16)
    assert_grouped(rows, orc.group_merge(base, F, INT))
    assert fs == dict(folded=66_000, scanned=66_000, redone=False)
