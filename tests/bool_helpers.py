"""Shared helpers for the boolean-column tests.

* A pure-Python encoder/decoder of the four boolean data-segment layouts,
  written from the format description (lib/encoding/bool.go, encoding.go
  block tags, column_builder.go), independent of the writer under test:

      full, no nils   [33][rows u32be][0x10][count u32be][ceil(count/8) B]
      nil bitmap      [5][bmlen u32be][bitmap][bm_off u32be][nilcount u32be]
                      [0x10][count u32be][bits]
      one row         [19][value byte]   ([19] alone = a nil row)
      empty           [43][rows u32be]

  Bits are MSB-first (value k at bit 7-(k&7) of byte k>>3, pad bits zero);
  the validity bitmap is LSB-first over rows.

* Twin shards: the same rows written once as a boolean column and once as
  the int64 column holding them as 0/1, with identical segment cuts. The
  boolean reducers are instances of the integer templates
  (series_agg_func.gen.go), so the expected rows of any boolean query are
  the oracle's rows for the int twin, minus sum.
"""

import struct

import numpy as np

import binding as orc

BOOL = 5
I = orc.ORC_TYPE_INT
S = 10**9
INT = 60 * S

VALUE_FIELDS = ("min", "max", "first", "last")
# every row field but sum / sum_isnil (per-series rows)
SERIES_FIELDS = ("sid", "win_start", "first_row_time", "count", "count_time",
                 "sum_time", "min_time", "max_time", "first_time", "last_time",
                 "min_isnil", "max_isnil", "first_isnil", "last_isnil")
# orc.group_merge synthesizes sid / first_row_time / count_time / sum_time
# (it sets them to the window start), so merged rows compare on the fields
# the cross-series merge defines
GROUP_FIELDS = ("win_start", "count", "min_time", "max_time", "first_time",
                "last_time", "min_isnil", "max_isnil", "first_isnil",
                "last_isnil")


def u32be(v):
    return struct.pack(">I", v)


def py_encode_bool_segment(values, valid):
    """values, valid: one entry per row. Returns the data segment bytes."""
    values = np.asarray(values, dtype=np.uint8)
    valid = np.asarray(valid, dtype=bool)
    rows = len(values)
    dense = values[valid]
    nil = rows - len(dense)
    if rows == 1 and nil == 0:
        return bytes([19, int(dense[0])])
    if nil == rows:
        return bytes([43]) + u32be(rows)
    bits = np.packbits(dense, bitorder="big").tobytes()
    enc = bytes([0x10]) + u32be(len(dense)) + bits
    if nil == 0:
        return bytes([33]) + u32be(rows) + enc
    bm = np.packbits(valid.astype(np.uint8), bitorder="little").tobytes()
    return bytes([5]) + u32be(len(bm)) + bm + u32be(0) + u32be(nil) + enc


def _decode_bits(enc):
    assert enc[0] >> 4 == 1, "boolCompressedBitpack"
    count = struct.unpack(">I", enc[1:5])[0]
    nbytes = (count + 7) // 8
    assert len(enc) == 5 + nbytes
    bits = np.unpackbits(np.frombuffer(enc[5:], dtype=np.uint8),
                         bitorder="big")
    assert not bits[count:].any(), "pad bits must be zero"
    return bits[:count]


def py_decode_bool_segment(seg, rows):
    """Returns (values uint8[rows] with 0 at nil rows, valid bool[rows])."""
    typ = seg[0]
    if typ == 19:
        assert rows == 1
        if len(seg) == 1:
            return np.zeros(1, np.uint8), np.zeros(1, bool)
        assert len(seg) == 2
        return np.array([seg[1]], np.uint8), np.ones(1, bool)
    if typ == 43:
        assert struct.unpack(">I", seg[1:5])[0] == rows and len(seg) == 5
        return np.zeros(rows, np.uint8), np.zeros(rows, bool)
    if typ == 33:
        assert struct.unpack(">I", seg[1:5])[0] == rows
        dense = _decode_bits(seg[5:])
        assert len(dense) == rows
        return dense.astype(np.uint8), np.ones(rows, bool)
    assert typ == 5
    bmlen = struct.unpack(">I", seg[1:5])[0]
    bm = np.frombuffer(seg[5:5 + bmlen], dtype=np.uint8)
    bm_off, nil = struct.unpack(">II", seg[5 + bmlen:13 + bmlen])
    valid = np.unpackbits(bm, bitorder="little")[bm_off:bm_off + rows]
    valid = valid.astype(bool)
    dense = _decode_bits(seg[13 + bmlen:])
    assert len(dense) == rows - nil == int(valid.sum())
    out = np.zeros(rows, np.uint8)
    out[valid] = dense
    return out, valid


def segment_cuts(sids, seg_rows):
    """(start, end) row ranges: cut at sid changes and every seg_rows rows."""
    cuts = []
    pos, n = 0, len(sids)
    while pos < n:
        end = pos
        while end < n and sids[end] == sids[pos] and end - pos < seg_rows:
            end += 1
        cuts.append((pos, end))
        pos = end
    return cuts


def series_rows(specs):
    """specs: list of (sid, times int64[], values 0/1[], valid bool[] or
    None). Returns flat (sids, times, values uint8, valid uint8)."""
    sids, times, vals, valid = [], [], [], []
    for sid, t, v, x in specs:
        n = len(t)
        sids.append(np.full(n, sid, dtype=np.uint64))
        times.append(np.asarray(t, dtype=np.int64))
        vals.append(np.asarray(v, dtype=np.uint8))
        valid.append(np.ones(n, np.uint8) if x is None
                     else np.asarray(x, dtype=np.uint8))
    return (np.concatenate(sids), np.concatenate(times), np.concatenate(vals),
            np.concatenate(valid))


def build_twin(sids, times, vals, valid, seg_rows):
    """The same rows as a boolean shard and as its int64 0/1 twin.
    Returns ((bblob, bdescs), (iblob, idescs))."""
    import opengemini_amd as gx

    bblob, bdescs = gx.encode_shard(BOOL, sids, times, vals, valid, seg_rows)
    iblob, idescs = gx.encode_shard(I, sids, times, vals.astype(np.int64),
                                    valid, seg_rows)
    bdescs = np.ascontiguousarray(bdescs)
    idescs = np.ascontiguousarray(idescs)
    # identical segment cuts
    for f in ("sid", "rows", "min_time", "max_time", "time_size"):
        assert np.array_equal(bdescs[f], idescs[f]), f
    return (bblob, bdescs), (iblob, idescs)


def odescs(descs):
    return np.frombuffer(np.asarray(descs).tobytes(),
                         dtype=orc.SEG_DESC_DTYPE)


def assert_bool_rows(got, exp, fields=SERIES_FIELDS):
    """got: rows of a boolean query; exp: oracle rows of the int twin.
    Bit-exact on every compared field; sum must be blank."""
    assert len(got) == len(exp), (len(got), len(exp))
    for f in fields:
        assert np.array_equal(got[f], exp[f]), f
    for f in VALUE_FIELDS:
        assert np.array_equal(np.asarray(got[f]).view(np.int64),
                              np.asarray(exp[f]).view(np.int64)), f
    assert not np.asarray(got["sum"]).view(np.int64).any(), "sum must be 0"
    assert np.all(got["sum_isnil"] == 1), "sum must be nil"


def pack_chunkmeta(sid, chunk_off, chunk_size, seg_ranges, cols):
    """Independent ChunkMeta marshal (tssp_file_meta.go:566-581; numberenc
    big-endian, int64 zigzag). cols: (name, ty, preagg_bytes,
    [(off, size), ...])."""
    def zz64(v):
        return struct.pack(">Q", ((v << 1) ^ (v >> 63)) & (2**64 - 1))

    out = bytearray()
    out += struct.pack(">Q", sid) + zz64(chunk_off)
    out += struct.pack(">III", chunk_size, len(cols), len(seg_ranges))
    for mn, mx in seg_ranges:
        out += zz64(mn) + zz64(mx)
    for name, ty, preagg, entries in cols:
        nb = name.encode()
        out += struct.pack(">H", len(nb)) + nb + bytes([ty])
        out += struct.pack(">H", len(preagg)) + preagg
        assert len(entries) == len(seg_ranges)
        for off, size in entries:
            out += zz64(off) + struct.pack(">I", size)
    return bytes(out)
