"""Row split of folded gorilla waves: a folding wave cut into K runs of
windows, each resumed from an attach-time decoder checkpoint, must return
the rows of the unsplit fold bit for bit.

Every case runs K = 1, 2, 3, 4 through GEMX_FOLD_SPLIT (read at attach) and
checks, per K: all row fields equal the K = 1 rows as raw bits, the rows
match the oracle's scan_agg + group_merge (test_gpu_fold's comparator),
fold_stats() is what K = 1 reports, and fold_split_stats() shows the number
of runs the shape allows, so a case cannot pass with the split never
running. The expected run counts come from `_cuts`, a transcription of the
plan's cut rule (csrc/gemx_foldsplit.hpp): a run keeps at least 2 windows
and 64 rows, starts within one window of the even cut and, among those,
where its first row is closest above a checkpoint row (every CKPT rows;
the earliest window wins ties).

Shapes are the smallest that reach each path: several waves and a partial
one, a first window that is cut short, windows without rows, decoder states
that are awkward to resume (1-bit records, records wider than a word), waves
that do not fold beside waves that do, and the NaN redo. Small shards only
fold with GEMX_FOLD_UNDERFILLED set; two cases at the end cover the default
policy on shards of 66,000 segments.
"""

import functools

import numpy as np
import pytest

import binding as orc
from shard_helpers import INT, F
from test_gpu_fold import (END, GORILLA_TAG, S, _aligned, _build, _is_gorilla,
                           _mixed, _nan, _py_gorilla, _shard, _walk,
                           assert_grouped)

pytestmark = pytest.mark.gpu

CKPT = 32      # GEMX_GOR_CKPT_ROWS of the default build
MIN_ROWS = 64  # GEMX_SUB_MIN_ROWS
KS = (1, 2, 3, 4)


@pytest.fixture(autouse=True)
def _fold_small_shards(monkeypatch):
    monkeypatch.setenv("GEMX_FOLD_UNDERFILLED", "1")


# ------------------------------------------------------------ the cut rule

def _bounds(t0, dt, rows, interval=INT, offset=0):
    """row boundaries of the windows a (t0, dt, rows) segment covers"""
    wf = (t0 - offset) // interval
    wl = (t0 + (rows - 1) * dt - offset) // interval
    b = [0]
    for k in range(wl - wf + 1):
        we = (wf + k + 1) * interval + offset
        b.append(min((we - t0 + dt - 1) // dt, rows))
    return b


def _cuts(b, k, ckpt=CKPT):
    """first window of each run, plus the window count"""
    nw = len(b) - 1
    rows = b[nw]
    runs = max(1, min(k, nw // 2, rows // MIN_ROWS))
    while runs > 1:
        cut = [0]
        for j in range(1, runs):
            e = (j * nw + runs // 2) // runs
            best = None
            for w in (e - 1, e, e + 1):
                if w < cut[-1] + 2 or w + 2 * (runs - j) > nw:
                    continue
                if (b[w] - b[cut[-1]] < MIN_ROWS
                        or rows - b[w] < MIN_ROWS * (runs - j)):
                    continue
                d = b[w] % ckpt
                if best is None or d < best[1]:
                    best = (w, d)
            if best is None:
                break
            cut.append(best[0])
        else:
            return cut + [nw]
        runs -= 1
    return [0, nw]


def _expect(b, k, fold_waves, other_waves=0):
    c = _cuts(b, k)
    runs = len(c) - 1
    skipped = sum(b[w] % CKPT for w in c[1:-1]) * fold_waves
    return dict(k_max=runs, tasks=fold_waves * runs + other_waves,
                skipped_rows=skipped)


# ------------------------------------------------------------------ runner

def _scan(blob, d, interval, start, end, offset):
    sh = _shard(blob, d)
    try:
        rows, _ = sh.scan_agg(start, end, interval, offset=offset,
                              group_all=True)
        return rows.copy(), sh.fold_stats(), sh.fold_split_stats()
    finally:
        sh.close()


def _same_bits(a, b):
    assert len(a) == len(b)
    for f in a.dtype.names:
        if f.startswith("_"):
            continue
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.dtype.itemsize == 8:
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), f


def _oracle(blob, d, interval=INT, start=0, end=END, offset=0):
    base = orc.scan_agg(blob, d, F, start, end, interval, offset)
    return orc.group_merge(base, F, interval)


def _check_all_k(monkeypatch, blob, d, expect, fold_stats, interval=INT,
                 start=0, end=END, offset=0):
    """expect(k) -> fold_split_stats() dict; returns {k: split stats}"""
    ref = _oracle(blob, d, interval, start, end, offset)
    first = None
    seen = {}
    for k in KS:
        monkeypatch.setenv("GEMX_FOLD_SPLIT", str(k))
        rows, fs, ss = _scan(blob, d, interval, start, end, offset)
        assert_grouped(rows, ref)
        assert fs == fold_stats, (k, fs)
        assert ss == expect(k), (k, ss)
        if first is None:
            first = rows
            assert ss["k_max"] == 1 and ss["skipped_rows"] == 0
        else:
            _same_bits(rows, first)
        seen[k] = ss
    return seen


# ------------------------------------------------------------------- cases

def test_aligned_with_tail(monkeypatch):
    """200 x 300 rows, 5 windows: 3 full waves and one of 8 lanes; 5 windows
    allow 2 runs, so K = 3 and 4 clamp to 2."""
    blob, d = _aligned()
    b = _bounds(0, S, 300)
    assert len(b) - 1 == 5
    seen = _check_all_k(monkeypatch, blob, d, lambda k: _expect(b, k, 4),
                        dict(folded=200, scanned=200, redone=False))
    assert [seen[k]["k_max"] for k in KS] == [1, 2, 2, 2]


def test_negative_time_and_offset(monkeypatch):
    blob, d = _aligned(-150 * S)
    b = _bounds(-150 * S, S, 300, offset=7 * S)
    assert len(b) - 1 == 6 and b[1] < 60  # partial first window
    seen = _check_all_k(monkeypatch, blob, d, lambda k: _expect(b, k, 4),
                        dict(folded=200, scanned=200, redone=False),
                        start=-(2**62), offset=7 * S)
    assert [seen[k]["k_max"] for k in KS] == [1, 2, 3, 3]


@functools.lru_cache(maxsize=None)
def _partial_first():
    rng = np.random.default_rng(710)
    return _build([(sid, [(7 * S, S, _walk(rng, 333), None)])
                   for sid in range(1, 71)])


def test_partial_first_window(monkeypatch):
    """70 x 333 rows from t0 = 7 s under 45 s windows: the first window holds
    38 rows, so later window starts (83, 128, 173, ...) are no multiples of
    the checkpoint stride and runs begin mid-stride."""
    blob, d = _partial_first()
    assert all(_is_gorilla(blob, x) for x in d)
    b = _bounds(7 * S, S, 333, interval=45 * S)
    assert b[:3] == [0, 38, 83] and len(b) - 1 == 8
    seen = _check_all_k(monkeypatch, blob, d, lambda k: _expect(b, k, 2),
                        dict(folded=70, scanned=70, redone=False),
                        interval=45 * S)
    assert max(seen[k]["k_max"] for k in KS) >= 3
    assert max(seen[k]["skipped_rows"] for k in KS) > 0


@functools.lru_cache(maxsize=None)
def _sparse():
    rng = np.random.default_rng(711)
    return _build([(sid, [(0, 90 * S, _walk(rng, 200), None)])
                   for sid in range(1, 131)])


def test_empty_windows_in_the_table(monkeypatch):
    """dt = 90 s under 1-minute windows: every third window has no row. A
    run whose first window is empty must skip it (gend <= i) and start its
    first real window without a leading decode."""
    blob, d = _sparse()
    b = _bounds(0, 90 * S, 200)
    nw = len(b) - 1
    assert sum(b[k + 1] <= b[k] for k in range(nw)) > nw // 4
    for ckpt in (16, 32, 64):  # whatever stride the library was built with
        assert any(b[w + 1] <= b[w]
                   for k in KS for w in _cuts(b, k, ckpt)[1:-1]), ckpt
    seen = _check_all_k(monkeypatch, blob, d, lambda k: _expect(b, k, 3),
                        dict(folded=130, scanned=130, redone=False))
    assert [seen[k]["k_max"] for k in KS] == [1, 2, 3, 3]


def _forced_gorilla(vals):
    """A gorilla block for values the adaptive writer would store another
    way (RLE for long runs, raw for incompressible doubles): an ordinary
    full-block header, then the gorilla codec byte and test_gpu_fold's
    hand-written stream."""
    rows = len(vals)
    head = orc.encode_data_segment(
        F, np.arange(rows, dtype=np.float64) * 0.5 + 0.25, None, rows, 0)[:5]
    return head + bytes([GORILLA_TAG << 4]) + _py_gorilla(vals)


@functools.lru_cache(maxsize=None)
def _awkward():
    """128 x 256 rows, three kinds of series: constant runs (1-bit records
    around each checkpoint), sign-random full-mantissa doubles (records
    wider than 64 bits, two-word advances, 64 meaningful bits) and a walk
    from the reference writer (which also reuses the previous bit window)."""
    rng = np.random.default_rng(712)
    times = np.arange(256, dtype=np.int64) * S
    tseg = orc.encode_time_segment(times)
    blob = bytearray()
    descs = []
    for sid in range(1, 129):
        kind = sid % 3
        if kind == 0:
            run = int(rng.integers(30, 50))
            dseg = _forced_gorilla(
                np.repeat(_walk(rng, 256 // run + 1), run)[:256])
        elif kind == 1:
            dseg = _forced_gorilla(
                rng.random(256) * rng.choice([-1.0, 1.0], 256))
        else:
            dseg = orc.encode_data_segment(F, _walk(rng, 256), None, 256, 0)
        descs.append((sid, len(blob), len(dseg), 256, len(blob) + len(dseg),
                      len(tseg), 0, 0, int(times[-1])))
        blob += dseg + tseg
    d = np.zeros(len(descs), dtype=orc.SEG_DESC_DTYPE)
    for i, tup in enumerate(descs):
        d[i] = tup
    return bytes(blob), d


def test_checkpoints_at_awkward_decoder_states(monkeypatch):
    blob, d = _awkward()
    assert all(_is_gorilla(blob, x) for x in d)
    # the random series really are wider than a word per record, the
    # constant ones far below one byte per record
    sizes = d["data_size"].astype(np.int64)
    assert sizes.max() > 256 * 8 and sizes.min() < 256
    b = _bounds(0, S, 256)
    seen = _check_all_k(monkeypatch, blob, d, lambda k: _expect(b, k, 2),
                        dict(folded=128, scanned=128, redone=False))
    assert [seen[k]["k_max"] for k in KS] == [1, 2, 2, 2]


def test_mixed_folding_and_plain_waves(monkeypatch):
    """Waves of 64, 64 and 52 gorilla segments; only the last folds. The two
    others stay one task each at every K: their segments are scanned once."""
    blob, d = _mixed()
    b = _bounds(0, S, 300)
    seen = _check_all_k(monkeypatch, blob, d,
                        lambda k: _expect(b, k, 1, other_waves=2),
                        dict(folded=52, scanned=190, redone=False))
    assert [seen[k]["tasks"] for k in KS] == [3, 4, 4, 4]


def test_nan_redo_at_k4(monkeypatch):
    blob, d = _nan()
    monkeypatch.setenv("GEMX_FOLD_SPLIT", "4")
    rows, fs, ss = _scan(blob, d, INT, 0, END, 0)
    assert fs == dict(folded=0, scanned=130, redone=True)
    assert ss["k_max"] == 0  # the rows come from the unfolded re-run
    monkeypatch.setenv("GEMX_DISABLE_FOLD", "1")
    plain, pfs, _ = _scan(blob, d, INT, 0, END, 0)
    assert pfs == dict(folded=0, scanned=130, redone=False)
    _same_bits(rows, plain)
    assert_grouped(rows, _oracle(blob, d))


# ------------------------------------------------- default policy, no switch

def _default_policy(monkeypatch, pts):
    monkeypatch.delenv("GEMX_FOLD_UNDERFILLED")
    monkeypatch.delenv("GEMX_FOLD_SPLIT", raising=False)
    blob, d = orc.gen_shard(49, 66_000, pts)
    rows, fs, ss = _scan(blob, d, INT, 0, END, 0)
    base = orc.scan_agg(blob, d, F, 0, END, INT, nthreads=16)
    assert_grouped(rows, orc.group_merge(base, F, INT))
    assert fs == dict(folded=66_000, scanned=66_000, redone=False)
    return ss


def test_default_policy_on_120_rows(monkeypatch):
    """test_default_folds_a_full_grid's shard: the policy asks for 8 runs
    of its 1032 waves, but 120 rows in 2 windows are below two runs' floor (2 windows and 64
    rows each), so the policy must leave these waves whole."""
    ss = _default_policy(monkeypatch, 120)
    assert ss == dict(k_max=1, tasks=1032, skipped_rows=0)


def test_default_policy_splits_a_full_grid(monkeypatch):
    """Same 66,000 series with 240 rows (4 windows): the smallest shard of
    that width the floors let the default policy cut, into 2 runs."""
    ss = _default_policy(monkeypatch, 240)
    assert ss["k_max"] == 2 and ss["tasks"] == 2 * 1032
