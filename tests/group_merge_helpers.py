"""Shards, oracle references and the comparator shared by
test_gpu_group_merge and test_gpu_sync_delivery (see the former for what
the shapes are for)."""


import functools

import numpy as np

import binding as orc
from shard_helpers import F, I

S = 10**9
END = 2**62
IV = 5 * S
ROWS = 26
GORILLA_TAG = 3
WAVES = (1, 65, 257, 321)
LAST_LANES = 64 - 37  # lanes of the partial last wave


def _nseries(waves):
    """last wave partial. A single wave keeps 47 lanes: grouped scans of 32
    series or fewer take k_group_small and never reach the merge kernel."""
    return waves * 64 - (37 if waves > 1 else 17)


# ---------------------------------------------------------------- builders

def _gorilla_mask(blob, d):
    b = np.frombuffer(blob, dtype=np.uint8)
    return (b[d["data_offset"].astype(np.int64) + 5] >> 4) == GORILLA_TAG


@functools.lru_cache(maxsize=None)
def _walk_shard(waves, gorilla_only=True):
    """Random-walk series, one aligned segment each. The float writer codes
    a few of them with another codec than gorilla; gorilla_only drops those,
    so exactly `waves` waves fold and nothing else reaches the merge.
    Without it the others stay: they never fold and arrive as p1 split
    entries next to the fold entries."""
    n = _nseries(waves)
    blob, d = orc.gen_shard(900 + waves, n + n // 40 + 64, ROWS)
    gor = _gorilla_mask(blob, d)
    if gorilla_only:
        d = d[gor][:n]
        assert len(d) == n
    else:
        d = d[: n + 5]
        assert 0 < (~gor[: n + 5]).sum()
    return blob, np.ascontiguousarray(d)


@functools.lru_cache(maxsize=None)
def _int_shard(waves):
    return orc.gen_shard(950 + waves, _nseries(waves), ROWS,
                         mode=orc.GEN_INT_SMALL)


def _desc_array(tuples):
    d = np.zeros(len(tuples), dtype=orc.SEG_DESC_DTYPE)
    for i, t in enumerate(tuples):
        d[i] = t
    return d


def _append_series(blob, tuples, sid, t0, vals):
    times = t0 + np.arange(len(vals), dtype=np.int64) * S
    dseg = orc.encode_data_segment(F, np.asarray(vals, dtype=np.float64), None,
                                   len(vals), 0)
    tseg = orc.encode_time_segment(times)
    tuples.append((sid, len(blob), len(dseg), len(vals), len(blob) + len(dseg),
                   len(tseg), 0, int(times[0]), int(times[-1])))
    blob += dseg + tseg


@functools.lru_cache(maxsize=None)
def _overlap_shard():
    """test_gpu_fold's overlap shape at 257 waves: one series owns a second
    segment that starts inside the first one's span, so its wave cannot fold
    and its series go through p1. The merge then sees split entries and
    fold entries in the same window."""
    blob, d = _walk_shard(257)
    blob = bytearray(blob)
    k = len(d) // 2
    tuples = [tuple(x) for x in d[: k + 1]]
    rng = np.random.default_rng(977)
    vals = np.round(np.cumsum(rng.normal(0, 1, ROWS)) * 128) / 128
    _append_series(blob, tuples, int(d["sid"][k]), 10 * S + S // 2, vals)
    tuples += [tuple(x) for x in d[k + 1:]]
    return bytes(blob), _desc_array(tuples)


# Ties. Every series is the same 26-value template XORed with a per-series
# constant in the low mantissa bits: consecutive values then XOR to the same
# bits in every series, all gorilla streams have one length, and the launch
# order (sorted by stream length, then segment) is the series order, so
# series w * 64 + lane sits in wave w. The constant only raises a value by a
# few ulps, so the ordinary series stay strictly inside (SMALL, BIG) and the
# planted series, written without a constant, hold every extreme exactly.
BIG, SMALL = 1000.0, 1.0
TIE_WAVES = (0, 63, 64, 255, 256, 320)
TIE_LANE = 5  # < LAST_LANES
# (row of BIG in window 1 = rows 5..9, row of SMALL in window 2 = rows 10..14)
TIE_ROWS = {0: (7, 12), 63: (7, 11), 64: (7, 12), 255: (6, 12), 256: (6, 12),
            320: (7, 11)}
# expected winners: the earlier row first, then the smaller series
TIE_MAX_TIME, TIE_MIN_TIME = 6 * S, 11 * S


def _tie_template(seed):
    rng = np.random.default_rng(seed)
    t = 100.0 + np.round(np.cumsum(rng.normal(0, 1, ROWS)) * 128) / 128
    assert t.min() > 50 and t.max() < 150
    return t


def _tie_variants(seed):
    base = _tie_template(seed)
    out = {}
    ordinary = base.copy()
    ordinary[7], ordinary[12] = 900.0, 2.0  # decoys: same record widths
    out[None] = ordinary
    for rows in set(TIE_ROWS.values()):
        v = base.copy()
        v[rows[0]], v[rows[1]] = BIG, SMALL
        out[rows] = v
    return out


def _stream_words(vals):
    seg = orc.encode_data_segment(F, vals, None, len(vals), 0)
    assert seg[5] >> 4 == GORILLA_TAG
    return (len(seg) - 15 + 7) // 8


@functools.lru_cache(maxsize=None)
def _tie_seed():
    """first template whose four variants code to streams of one length"""
    for seed in range(3000, 3400):
        if len({_stream_words(v) for v in _tie_variants(seed).values()}) == 1:
            return seed
    raise AssertionError("no template with equal stream lengths")


@functools.lru_cache(maxsize=None)
def _tie_shard():
    variants = _tie_variants(_tie_seed())
    n = _nseries(321)
    planted = {w * 64 + TIE_LANE: TIE_ROWS[w] for w in TIE_WAVES}
    times = np.arange(ROWS, dtype=np.int64) * S
    tseg = orc.encode_time_segment(times)
    ordinary = variants[None].view(np.uint64)
    blob = bytearray()
    tuples = []
    for k in range(n):
        if k in planted:
            vals = variants[planted[k]]
        else:
            vals = (ordinary ^ np.uint64((k + 1) << 4)).view(np.float64)
        dseg = orc.encode_data_segment(F, vals, None, ROWS, 0)
        tuples.append((k + 1, len(blob), len(dseg), ROWS, len(blob) + len(dseg),
                       len(tseg), 0, 0, int(times[-1])))
        blob += dseg + tseg
    return bytes(blob), _desc_array(tuples)


def launch_waves(blob, d):
    """wave of each segment in the gorilla launch order: segments sorted by
    stream length in 8-byte words, then by segment index"""
    assert _gorilla_mask(blob, d).all()
    words = (d["data_size"].astype(np.int64) - 15 + 7) // 8
    order = np.lexsort((np.arange(len(d)), words))
    wave = np.empty(len(d), dtype=np.int64)
    wave[order] = np.arange(len(d)) // 64
    return wave


@functools.lru_cache(maxsize=None)
def _gap_shard():
    """65 waves of series with rows at 0..9 s and 20..29 s: windows 2 and 3
    are covered by nobody. Two aligned segments per series, each a template
    XORed with a per-series constant (as in the tie shard), the later one
    with finer values and so a longer stream. The launch order (by stream
    length) then keeps the two kinds apart, every wave but the one where
    they meet folds, and the empty windows reach the merge as unused
    entries."""
    n = _nseries(65)
    rng = np.random.default_rng(978)
    t_a = orc.encode_time_segment(np.arange(10, dtype=np.int64) * S)
    t_b = orc.encode_time_segment((20 + np.arange(10, dtype=np.int64)) * S)
    early = 100.0 + np.round(np.cumsum(rng.normal(0, 1, 10)) * 128) / 128
    late = 100.0 + np.round(np.cumsum(rng.normal(0, 1, 10)) * 2**16) / 2**16
    blob = bytearray()
    tuples = []
    for k in range(n):
        c = np.uint64((k + 1) << 4)
        for tmpl, tseg, t0 in ((early, t_a, 0), (late, t_b, 20 * S)):
            vals = (tmpl.view(np.uint64) ^ c).view(np.float64)
            dseg = orc.encode_data_segment(F, vals, None, 10, 0)
            tuples.append((k + 1, len(blob), len(dseg), 10, len(blob) + len(dseg),
                           len(tseg), 0, t0, t0 + 9 * S))
            blob += dseg + tseg
    d = _desc_array(tuples)
    assert _gorilla_mask(bytes(blob), d).all()
    words = (d["data_size"].astype(np.int64) - 15 + 7) // 8
    assert words[0::2].max() < words[1::2].min()
    return bytes(blob), d


_SHARDS = {
    "walk": (_walk_shard, F),
    "int": (_int_shard, I),
    "overlap": (_overlap_shard, F),
    "mixed": (lambda waves: _walk_shard(waves, False), F),
    "tie": (_tie_shard, F),
    "gap": (_gap_shard, F),
}


@functools.lru_cache(maxsize=None)
def _ref(kind, *args):
    """oracle rows of a shard, computed once and shared read-only"""
    build, col_type = _SHARDS[kind]
    blob, d = build(*args)
    base = orc.scan_agg(blob, d, col_type, 0, END, IV)
    ref = orc.group_merge(base, col_type, IV)
    ref.setflags(write=False)
    return ref


# ---------------------------------------------------------------- compare

def assert_grouped(gpu_rows, ref, col_type=F):
    assert len(gpu_rows) == len(ref), (len(gpu_rows), len(ref))
    for f in ("win_start", "count", "min_time", "max_time", "first_time",
              "last_time", "min_isnil", "max_isnil", "first_isnil",
              "last_isnil", "sum_isnil"):
        assert np.array_equal(gpu_rows[f], ref[f]), f
    for f in ("min", "max", "first", "last"):
        assert np.array_equal(
            gpu_rows[f].view(np.uint64), ref[f].view(np.uint64)
        ), f
    if col_type == F:
        tol = 1e-9 * np.maximum(1.0, np.abs(ref["sum"]))
        both_nan = np.isnan(gpu_rows["sum"]) & np.isnan(ref["sum"])
        assert np.all(both_nan | (np.abs(gpu_rows["sum"] - ref["sum"]) <= tol))
    else:
        assert np.array_equal(gpu_rows["sum"].view(np.int64),
                              ref["sum"].view(np.int64))


def _grouped(blob, d, col_type=F, fill=False):
    import opengemini_amd as gx

    sh = gx.Shard(blob, d, col_type)
    try:
        if fill:
            rows, _ = sh.scan_agg_grouped_fill(0, END, IV)
        else:
            rows, _ = sh.scan_agg(0, END, IV, group_all=True)
        return rows.copy(), sh.fold_stats()
    finally:
        sh.close()
