"""Arena gorilla reader and folded wave reduce, at the shapes where they
can go wrong.

The record loop of the gorilla grid kernels keeps a four-word window per
lane, rotates it by one word per record behind predicated moves and takes
the second word of a two-word advance (a record wider than 64 bits that
crosses a word boundary) on a wave-uniform cold path. The folded path then
reduces every window across the wave: a full-wave form without presence
predicates, a general form for the partial wave, first/last read from the
one lane that holds the smallest series index, and min/max ties broken on
a packed (row, series) key.

Every case attaches with GEMX_FOLD_UNDERFILLED (shards this small would
otherwise run the sub-segment split), compares the grouped rows with the
oracle (scan_agg + group_merge; count, times, min/max/first/last bit-exact,
float sum within 1e-9 relative), compares them bit for bit, sum included,
with the same build at GEMX_FOLD_SPLIT=1, and asserts through fold_stats()
that the segments really folded. Each case runs unsplit (GEMX_FOLD_SPLIT=1)
and cut into runs that resume from decoder checkpoints (GEMX_FOLD_SPLIT=4);
fold_split_stats() must report the cut. A run keeps at least 64 rows, so a
130-row wave is cut in two, and only where a window starts at row 64..66:
hence the 13 s windows (row 65, one record past a checkpoint) next to the
1 s ones (row 64, on a checkpoint).

The reference writer stores incompressible values as raw blocks, so the
streams with wide records are written by the local gorilla writer below;
every case asserts the codec tag of its segments.
"""

import functools
import struct

import numpy as np
import pytest

import binding as orc
from shard_helpers import F

pytestmark = pytest.mark.gpu

S = 10**9
END = 2**62
GORILLA_TAG = 3  # outer float codec tag (high nibble of the codec byte)
ROWS = 130
SPLITS = [1, 4]


@pytest.fixture(autouse=True)
def _fold_small_shards(monkeypatch):
    monkeypatch.setenv("GEMX_FOLD_UNDERFILLED", "1")


# ---------------------------------------------------------------- builders

def _py_gorilla(words, reuse=False):
    """tsm1 gorilla stream of the given uint64 value bits. A changed value
    is written with the `new window` control bits (13-bit header), or, with
    reuse=True, inside the previous window where it fits (2-bit header).
    Same layout as orc.gorilla_encode."""
    uvnan = 0x7FF8000000000001
    acc, nbits = 0, 0
    win = None  # (lead, trail) of the current window
    words = [int(w) for w in words]
    prev = words[0]
    for cur in words[1:] + [uvnan]:
        x = cur ^ prev
        prev = cur
        if x == 0:
            acc, nbits = acc << 1, nbits + 1
            continue
        lead = min(64 - x.bit_length(), 31)
        trail = (x & -x).bit_length() - 1
        if reuse and win is not None and lead >= win[0] and trail >= win[1]:
            sig = 64 - win[0] - win[1]
            acc = (((acc << 2) | 0b10) << sig) | (x >> win[1])
            nbits += 2 + sig
            continue
        win = (lead, trail)
        sig = 64 - lead - trail
        hdr = (0b11 << 11) | (lead << 6) | (sig & 0x3F)  # 64 is written as 0
        acc = (((acc << 13) | hdr) << sig) | (x >> trail)
        nbits += 13 + sig
    pad = -nbits % 8
    body = (acc << pad).to_bytes((nbits + pad) // 8, "big")
    return bytes([1 << 4]) + struct.pack(">Q", words[0]) + body


def _bits(vals):
    return np.asarray(vals, dtype=np.float64).view(np.uint64)


def _data_segment(vals, writer):
    rows = len(vals)
    if writer is None:
        return orc.encode_data_segment(F, vals, None, rows, 0)
    # full-block header of an ordinary segment of the same length, then the
    # gorilla codec byte and the hand-written stream
    head = orc.encode_data_segment(
        F, np.arange(rows, dtype=np.float64) * 0.5 + 0.25, None, rows, 0
    )[:5]
    return head + bytes([GORILLA_TAG << 4]) + _py_gorilla(
        _bits(vals), reuse=(writer == "reuse"))


def _build(series):
    """series: list of (sid, t0_ns, vals, writer) — one segment each, 1 s
    step; writer None = reference writer, "new" / "reuse" = local writer"""
    blob = bytearray()
    descs = []
    for sid, t0, vals, writer in series:
        vals = np.asarray(vals, dtype=np.float64)
        rows = len(vals)
        times = t0 + np.arange(rows, dtype=np.int64) * S
        dseg = _data_segment(vals, writer)
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


def _walk(rng, n):
    return np.round(np.cumsum(rng.normal(0, 1, n)) * 128) / 128


def _wide(rng, n, start):
    """n values from `start` on; every XOR between neighbours has bit 63
    and bit 0 set (64 significant bits) and leaves the exponent alone, so
    the values stay finite"""
    x = (rng.integers(0, 1 << 51, n - 1, dtype=np.uint64) << np.uint64(1)) \
        | np.uint64(0x8000000000000001)
    w = np.empty(n, dtype=np.uint64)
    w[0] = _bits([start])[0]
    w[1:] = w[0] ^ np.bitwise_xor.accumulate(x)
    return w.view(np.float64)


# A case is (blob, descs, interval, number of segments that must fold).
RUNS_AT_4 = 2  # runs per 130-row wave at GEMX_FOLD_SPLIT=4


@functools.lru_cache(maxsize=None)
def _two_word():
    """128 series x 130 rows, two waves. 64 series: j one-bit repeat
    records, then 77-bit records (13-bit header + 64 significant bits) back
    to back, j = 0..63, so the wide records start at 64 different bit
    offsets and cross word boundaries at every one. 32 series repeat one
    value throughout; 32 are wide from the first record, half of them
    inside the previous window (66-bit records). The arena orders lanes by
    stream length: the all-repeat lanes share a wave with the j >= 32
    streams, the all-wide lanes with the j < 32 ones."""
    rng = np.random.default_rng(800)
    series = []
    sid = 1
    for j in range(64):
        start = 1.5 + j / 128
        vals = np.concatenate([np.full(j, start), _wide(rng, ROWS - j, start)])
        series.append((sid, 0, vals, "new"))
        sid += 1
    for k in range(32):
        series.append((sid, 0, np.full(ROWS, 3.0 + k / 64), "new"))
        sid += 1
    for k in range(32):
        series.append((sid, 0, _wide(rng, ROWS, 1.25 + k / 256),
                       "reuse" if k % 2 else "new"))
        sid += 1
    blob, d = _build(series)
    # 129 records of 77 bits in the j = 0 stream, one bit each in a repeat
    assert d["data_size"].max() > 129 * 77 // 8
    assert d["data_size"].min() < 64
    return blob, d, 13 * S, 128


@functools.lru_cache(maxsize=None)
def _window_lengths(interval_s):
    """70 series (a full wave and 6 lanes) x 130 rows from t = 5 s: the
    first window of the 2 s, 3 s and 7 s intervals is partial, the 1 s
    interval makes every window a single row (the record loop runs zero
    times), 2 s / 3 s / 7 s give even and odd lengths."""
    rng = np.random.default_rng(801)
    blob, d = _build([(sid, 5 * S, _walk(rng, ROWS), None)
                      for sid in range(1, 71)])
    return blob, d, interval_s * S, 70


@functools.lru_cache(maxsize=None)
def _population(n):
    """n aligned series x 130 rows: 64 and 128 are full waves only, 63 is
    one partial wave, 65 a full wave and a lone lane. The plan folds only
    shards of more than 32 series, so n = 1 gets 64 shorter, mutually
    unaligned streams in front: they fill the first wave (the arena orders
    by stream length) and leave the aligned series alone in the second."""
    rng = np.random.default_rng(802)
    series = []
    sid = 1
    if n == 1:
        for k in range(64):
            vals = np.round(np.cumsum(rng.normal(0, 3, 60 + k % 2)))
            series.append((sid, 0, vals, None))
            sid += 1
    for _ in range(n):
        series.append((sid, 0, _walk(rng, ROWS), None))
        sid += 1
    blob, d = _build(series)
    if n == 1:
        assert d["data_size"][64] > d["data_size"][:64].max() + 8
    return blob, d, 13 * S, n


@functools.lru_cache(maxsize=None)
def _first_last():
    """70 series whose stream length falls with the series id: series k
    repeats its first value k times (one bit each) and then changes in
    77-bit records, so launch order is the reverse of series order and in
    both waves the smallest series index sits in the last valid lane. The
    values are random mantissas: every series has its own first and last
    value in every window."""
    rng = np.random.default_rng(803)
    series = []
    for k in range(70):
        start = 1.5 + k / 128
        w = np.concatenate([np.full(k, start), _wide(rng, ROWS - k, start)])
        series.append((k + 1, 0, w, "new"))
    blob, d = _build(series)
    assert np.all(np.diff(d["data_size"].astype(np.int64)) < 0)
    return blob, d, 13 * S, 70


@functools.lru_cache(maxsize=None)
def _ties_small():
    """70 series of values in {0, 1, 2} held for runs of 2..6 rows: the
    window minimum and maximum occur in many lanes, at the same row and at
    different rows."""
    rng = np.random.default_rng(804)
    series = []
    for sid in range(1, 71):
        run = int(rng.integers(2, 7))
        n = ROWS // run + 1
        vals = np.repeat(rng.integers(0, 3, n).astype(np.float64), run)[:ROWS]
        series.append((sid, 0, vals, None))
    return _build(series) + (13 * S, 70)


@functools.lru_cache(maxsize=None)
def _ties_4096():
    """40 series x 4096 rows, the largest segment an attach accepts, with
    the extremes planted late so the row half of the tie key is large: in
    window 66 the same minimum / maximum at the same row in two series
    (the smaller series index wins), in window 67 at an earlier row in a
    third series as well (the earlier row wins)."""
    rng = np.random.default_rng(805)
    vals = [_walk(rng, 4096) for _ in range(40)]
    for sidx, row in ((5, 3990), (9, 3990)):
        vals[sidx][row] = -4096.0
        vals[sidx][row + 3] = 4096.0
    for sidx, row in ((30, 4050), (12, 4050), (20, 4041)):
        vals[sidx][row] = -4096.0
        vals[sidx][row + 4] = 4096.0
    blob, d = _build([(k + 1, 0, v, None) for k, v in enumerate(vals)])
    return blob, d, 60 * S, 40


# ---------------------------------------------------------------- compare

def _oracle(blob, d, interval):
    base = orc.scan_agg(blob, d, F, 0, END, interval)
    return orc.group_merge(base, F, interval)


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


def assert_same_bits(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for f in a.dtype.names:
        x, y = a[f], b[f]
        if x.dtype.kind == "f":
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), f


def _grouped(monkeypatch, blob, d, interval, split):
    import opengemini_amd as gx

    monkeypatch.setenv("GEMX_FOLD_SPLIT", str(split))
    sh = gx.Shard(blob, d, F)
    try:
        rows, _ = sh.scan_agg(0, END, interval, group_all=True)
        return rows.copy(), dict(sh.fold_stats(), **sh.fold_split_stats())
    finally:
        sh.close()


_REFS = {}


def _check(monkeypatch, key, case, split, runs_at_4=RUNS_AT_4):
    blob, d, interval, nfold = case
    if key not in _REFS:  # oracle rows and the unsplit rows, once per case
        ref = _oracle(blob, d, interval)
        ref.setflags(write=False)
        unsplit, _ = _grouped(monkeypatch, blob, d, interval, 1)
        unsplit.setflags(write=False)
        _REFS[key] = (ref, unsplit)
    ref, unsplit = _REFS[key]
    assert len(ref) > 0 and np.all(ref["count"] > 0)
    rows, fs = _grouped(monkeypatch, blob, d, interval, split)
    assert fs["folded"] == nfold and fs["scanned"] == len(d), fs
    assert not fs["redone"]
    assert fs["k_max"] == (1 if split == 1 else runs_at_4), fs
    assert_grouped(rows, ref)
    assert_same_bits(rows, unsplit)
    return ref


# ------------------------------------------------------------------- cases

@pytest.mark.parametrize("split", SPLITS)
def test_two_word_advance_at_every_bit_offset(monkeypatch, split):
    case = _two_word()
    assert all(_is_gorilla(case[0], x) for x in case[1])
    _check(monkeypatch, "two_word", case, split)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("interval_s", [1, 2, 3, 7])
def test_window_lengths(monkeypatch, interval_s, split):
    case = _window_lengths(interval_s)
    assert all(_is_gorilla(case[0], x) for x in case[1])
    ref = _check(monkeypatch, ("lengths", interval_s), case, split)
    per = ref["count"] // 70  # rows per window: every lane covers the same
    assert per[0] == {1: 1, 2: 1, 3: 1, 7: 2}[interval_s]
    assert set(per[1:-1]) == {interval_s}


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 128])
def test_wave_population(monkeypatch, n, split):
    case = _population(n)
    assert all(_is_gorilla(case[0], x) for x in case[1])
    _check(monkeypatch, ("population", n), case, split)


@pytest.mark.parametrize("split", SPLITS)
def test_first_last_winner_is_not_lane_0(monkeypatch, split):
    case = _first_last()
    blob, d, interval, _ = case
    assert all(_is_gorilla(blob, x) for x in d)
    ref = _check(monkeypatch, "first_last", case, split)
    # the rows report series 1 (index 0), and no other series would do
    base = orc.scan_agg(blob, d, F, 0, END, interval)
    for f in ("first", "last"):
        for w, v in zip(ref["win_start"], ref[f]):
            hit = base[(base["win_start"] == w) & (base[f] == v)]
            assert list(hit["sid"]) == [1], (f, w)


@pytest.mark.parametrize("split", SPLITS)
def test_tie_key_small_rows(monkeypatch, split):
    case = _ties_small()
    assert all(_is_gorilla(case[0], x) for x in case[1])
    ref = _check(monkeypatch, "ties_small", case, split)
    assert np.all(ref["min"] == 0.0) and np.all(ref["max"] == 2.0)


@pytest.mark.parametrize("split", SPLITS)
def test_tie_key_largest_segment(monkeypatch, split):
    case = _ties_4096()
    assert all(_is_gorilla(case[0], x) for x in case[1])
    assert np.all(case[1]["rows"] == 4096)
    ref = _check(monkeypatch, "ties_4096", case, split, runs_at_4=4)
    assert ref["min"][66] == -4096.0 and ref["min_time"][66] == 3990 * S
    assert ref["max"][66] == 4096.0 and ref["max_time"][66] == 3993 * S
    assert ref["min"][67] == -4096.0 and ref["min_time"][67] == 4041 * S
    assert ref["max"][67] == 4096.0 and ref["max_time"][67] == 4045 * S
