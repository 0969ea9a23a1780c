"""Boolean segment writer vs a from-spec Python codec (CPU).

gemx_encode_shard(GEMX_TYPE_BOOL) must emit, per data segment, exactly the
bytes the format description yields (bool_helpers.py restates it from
lib/encoding/bool.go + encoding.go's block tags, independently of the
writer), and the Python decoder must recover values and nils from the
writer's segments."""

import numpy as np
import pytest

from bool_helpers import (BOOL, S, py_decode_bool_segment,
                          py_encode_bool_segment, segment_cuts)

ROW_COUNTS = [1, 7, 8, 9, 63, 64, 65, 1000]
SEG_ROWS = [1, 64, 400]
PATTERNS = ["all_true", "all_false", "alternating",
            "random_nil0", "random_nil30", "random_nil100"]


def make_column(pattern, n, seed):
    rng = np.random.default_rng(seed)
    valid = np.ones(n, dtype=np.uint8)
    if pattern == "all_true":
        vals = np.ones(n, dtype=np.uint8)
    elif pattern == "all_false":
        vals = np.zeros(n, dtype=np.uint8)
    elif pattern == "alternating":
        vals = (np.arange(n) & 1).astype(np.uint8)
    else:
        vals = rng.integers(0, 2, n).astype(np.uint8)
        frac = {"random_nil0": 0.0, "random_nil30": 0.3,
                "random_nil100": 1.0}[pattern]
        valid = (rng.random(n) >= frac).astype(np.uint8)
    return vals, valid


@pytest.mark.parametrize("seg_rows", SEG_ROWS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_writer_matches_spec_codec(n, pattern, seg_rows):
    import opengemini_amd as gx

    # two series so a sid change cuts a segment too
    vals, valid = make_column(pattern, 2 * n, seed=n * 131 + seg_rows)
    sids = np.repeat(np.array([3, 9], dtype=np.uint64), n)
    times = np.tile(np.arange(n, dtype=np.int64) * S, 2)
    blob, descs = gx.encode_shard(BOOL, sids, times, vals, valid, seg_rows)
    cuts = segment_cuts(sids, seg_rows)
    assert len(descs) == len(cuts)
    for d, (a, b) in zip(descs, cuts):
        assert int(d["rows"]) == b - a and int(d["sid"]) == int(sids[a])
        seg = blob[int(d["data_offset"]):
                   int(d["data_offset"]) + int(d["data_size"])]
        v, x = vals[a:b], valid[a:b].astype(bool)
        assert seg == py_encode_bool_segment(v, x), (a, b)
        dv, dx = py_decode_bool_segment(seg, b - a)
        assert np.array_equal(dx, x)
        assert np.array_equal(dv[x], v[x])


def test_layout_tags():
    """One of each layout, spelled out byte by byte."""
    t, f = 1, 0
    assert py_encode_bool_segment([t], [1]) == bytes([19, 1])
    assert py_encode_bool_segment([t, f], [0, 0]) == bytes([43, 0, 0, 0, 2])
    # 9 rows T F T T F F F F T -> 0b10110000, 0b10000000
    full = py_encode_bool_segment([t, f, t, t, f, f, f, f, t], [1] * 9)
    assert full == bytes([33, 0, 0, 0, 9, 0x10, 0, 0, 0, 9, 0xB0, 0x80])
    # rows: T nil F -> bitmap 0b101 (LSB-first), dense T F -> 0b10000000
    mixed = py_encode_bool_segment([t, t, f], [1, 0, 1])
    assert mixed == bytes([5, 0, 0, 0, 1, 0x05, 0, 0, 0, 0, 0, 0, 0, 1,
                           0x10, 0, 0, 0, 2, 0x80])
    # the nil one-row form is decodable even though the writer emits the
    # empty form for an all-nil row
    v, x = py_decode_bool_segment(bytes([19]), 1)
    assert not x[0]
