"""Numpy reference and shard builders for the top()/bottom() selector tests.

ref_topn is checked against the reference's own golden records
(tests/golden/topn_cases.json, test_topn_host.py) and then serves as the
reference for the GPU tests."""

import json
import os

import numpy as np

import binding as orc

import opengemini_amd as gx
from opengemini_amd.engine import GEMX_TYPE_FLOAT, GEMX_TYPE_INT

S = 10**9
HERE = os.path.dirname(os.path.abspath(__file__))


def point_dtype(values):
    vt = "<i8" if np.asarray(values).dtype.kind in "iu" else "<f8"
    return np.dtype([("sid", "<u8"), ("win_start", "<i8"), ("time", "<i8"),
                     ("value", vt)])


def _select(times, vals, n, sel):
    """Best n points under (better value, then earlier time), returned in
    emission order: time ascending, on equal time the better value first."""
    # rank of the value instead of the value: negating a rank is exact for
    # int64 too, and -0.0 / 0.0 share a rank as they compare equal
    _, rank = np.unique(vals, return_inverse=True)
    key = -rank if sel == "top" else rank
    best = np.lexsort((times, key))[:n]
    t, v, k = times[best], vals[best], key[best]
    emit = np.lexsort((k, t))
    return t[emit], v[emit]


def ref_topn(points_by_sid, start, end, interval, offset, n, sel, group_all):
    """points_by_sid: {sid: (times, values)} in descriptor order, non-nil
    rows only (NaN allowed: dropped here, as the engine drops them).
    Returns the expected rows as a structured array (point_dtype)."""
    assert sel in ("top", "bottom")
    sids = list(points_by_sid)
    dt = point_dtype(points_by_sid[sids[0]][1]) if sids else point_dtype(
        np.zeros(0))
    if group_all:
        ts = np.concatenate([np.asarray(points_by_sid[s][0], dtype=np.int64)
                             for s in sids])
        vs = np.concatenate([np.asarray(points_by_sid[s][1]) for s in sids])
        groups = [(0, ts, vs)]
    else:
        groups = [(s, np.asarray(points_by_sid[s][0], dtype=np.int64),
                   np.asarray(points_by_sid[s][1])) for s in sids]
    out = []
    for sid, t, v in groups:
        m = (t >= start) & (t <= end)
        if v.dtype.kind == "f":
            m &= ~np.isnan(v)
        t, v = t[m], v[m]
        if len(t) == 0:
            continue
        if interval:
            ws = (t - offset) // interval * interval + offset
        else:
            ws = np.full(len(t), start, dtype=np.int64)
        for w in np.unique(ws):
            wm = ws == w
            et, ev = _select(t[wm], v[wm], n, sel)
            rows = np.zeros(len(et), dtype=dt)
            rows["sid"] = sid
            rows["win_start"] = w
            rows["time"] = et
            rows["value"] = ev
            out.append(rows)
    return np.concatenate(out) if out else np.zeros(0, dtype=dt)


def assert_rows_equal(got, exp, ctx=""):
    assert len(got) == len(exp), (ctx, len(got), len(exp))
    for f in ("sid", "win_start", "time"):
        assert np.array_equal(got[f], exp[f]), (ctx, f)
    assert got["value"].dtype == exp["value"].dtype, (ctx, got["value"].dtype)
    assert np.array_equal(got["value"], exp["value"]), (ctx, "value")


def load_golden():
    with open(os.path.join(HERE, "golden", "topn_cases.json")) as f:
        return json.load(f)["cases"]


def golden_points(case, column):
    """(times, values, valid) of one column of a golden case, all records."""
    t, v, x = [], [], []
    for rec in case["records"]:
        for ti, vi in zip(rec["time"], rec[column]):
            t.append(ti)
            x.append(vi is not None)
            v.append(0 if vi is None else vi)
    vt = np.int64 if column == "int" else np.float64
    return (np.array(t, dtype=np.int64), np.array(v, dtype=vt),
            np.array(x, dtype=bool))


def col_type_of(values):
    return GEMX_TYPE_INT if np.asarray(values).dtype.kind in "iu" \
        else GEMX_TYPE_FLOAT


def writer_shard(points_by_sid, seg_rows):
    """Nil-free shard through the engine's own writer (gx.encode_shard)."""
    sids = np.concatenate([np.full(len(t), s, dtype=np.uint64)
                           for s, (t, _) in points_by_sid.items()])
    times = np.concatenate([np.asarray(t, dtype=np.int64)
                            for t, _ in points_by_sid.values()])
    vals = np.concatenate([np.asarray(v) for _, v in points_by_sid.values()])
    ct = col_type_of(vals)
    blob, descs = gx.encode_shard(ct, sids, times, vals, seg_rows=seg_rows)
    return blob, descs, ct


def oracle_shard(col_type, segments):
    """Shard through the oracle's segment encoders (nil bitmaps, snappy,
    empty blocks). segments: [(sid, times, values, valid)] in descriptor
    order; values has one entry per row (nil rows' entries are ignored).
    A fifth tuple element replaces the encoded data segment."""
    ot = orc.ORC_TYPE_FLOAT if col_type == GEMX_TYPE_FLOAT else orc.ORC_TYPE_INT
    blob = bytearray()
    descs = []
    for seg in segments:
        sid, times, vals, valid = seg[:4]
        times = np.asarray(times, dtype=np.int64)
        vals = np.asarray(vals)
        valid = np.asarray(valid, dtype=bool)
        rows = len(times)
        nil = int((~valid).sum())
        bm = np.packbits(valid.astype(np.uint8), bitorder="little")
        if len(seg) > 4:
            dseg = seg[4]
        else:
            dseg = orc.encode_data_segment(ot, vals[valid], bm, rows, nil)
        tseg = orc.encode_time_segment(times)
        descs.append((sid, len(blob), len(dseg), rows, len(blob) + len(dseg),
                      len(tseg), 0, times.min(), times.max()))
        blob += dseg + tseg
    d = np.zeros(len(descs), dtype=gx.SEG_DESC_DTYPE)
    for i, tup in enumerate(descs):
        d[i] = tup
    return bytes(blob), d


def snappy_float_segment(vals):
    """Nil-free float data segment in the snappy form of the float codec
    (lib/compress/float.go: tag 2 over the raw little-endian values). The
    oracle's adaptive encoder never keeps it — its all-literal snappy
    stream always trips the 90 % ratio fallback — so the block is framed
    here around the oracle's snappy stream: [BlockFloatFull][rows u32be]
    [2 << 4][snappy]."""
    raw = np.frombuffer(np.asarray(vals, dtype="<f8").tobytes(), dtype=np.uint8)
    enc = bytes(orc.snappy_encode(raw))
    return bytes([31]) + len(vals).to_bytes(4, "big") + bytes([2 << 4]) + enc


def points_of_segments(segments):
    """{sid: (times, values)} of the non-nil rows, descriptor order."""
    acc = {}
    for sid, times, vals, valid in (s[:4] for s in segments):
        valid = np.asarray(valid, dtype=bool)
        a = acc.setdefault(sid, ([], []))
        a[0].append(np.asarray(times, dtype=np.int64)[valid])
        a[1].append(np.asarray(vals)[valid])
    return {s: (np.concatenate(t), np.concatenate(v)) for s, (t, v) in acc.items()}


def err_code(excinfo):
    """GEMX_E_* code out of a GemxError ("gemx error <rc>: ...")."""
    return int(str(excinfo.value).split("gemx error ")[1].split(":")[0])
