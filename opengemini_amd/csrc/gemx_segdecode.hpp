/* gemx_segdecode.hpp — the one place a segment is decoded for the
 * per-segment scan kernels (k_scan_fast, k_eval_filter, k_scan_general,
 * k_rate_scan, k_topn_scan, k_distinct_scan, k_rate_edges, k_ot_cells).
 *
 * Two readers, both plain structs a kernel keeps in registers:
 *   SegStream<COLTYPE>    nil-free segments, decoded row by row
 *   SegBuffered<COLTYPE>  everything else, decoded into per-lane scratch
 * and the layout of that scratch, shared by the host code that sizes it.
 *
 * Included by gemx_engine.hip after the byte readers, the iterators,
 * SegHeader / parse_data_header / bm_valid and the GEMX_E_* codes. Errors
 * come back as codes; the kernel does its own set_err(err, rc); return;. */
#ifndef GEMX_SEGDECODE_HPP
#define GEMX_SEGDECODE_HPP

/* ---------------- per-lane scratch layout ----------------
 *
 *   SEG_OFF_T       int64 times, one per row            SEG_COL_BYTES
 *   SEG_OFF_V       int64 value bits, dense (no nils)   SEG_COL_BYTES
 *   SEG_OFF_SNAPPY  snappy output before it is copied   SEG_SNAPPY_BYTES
 *   SEG_OFF_SPARE   the kernel's own (k_scan_general: two row bitmaps)
 *
 * The values-only form k_eval_filter uses drops the time column. */
constexpr int SEG_MAX_ROWS = 4096; /* gemx_shard_attach refuses more */
constexpr uint64_t SEG_COL_BYTES = 4096 * 8;
constexpr uint64_t SEG_SNAPPY_BYTES = 40960;
constexpr uint64_t SEG_BM_BYTES = SEG_MAX_ROWS / 8; /* one bit per row */
constexpr uint64_t SEG_OFF_T = 0;
constexpr uint64_t SEG_OFF_V = SEG_COL_BYTES;
constexpr uint64_t SEG_OFF_SNAPPY = 2 * SEG_COL_BYTES;
constexpr uint64_t SEG_OFF_SPARE = SEG_OFF_SNAPPY + SEG_SNAPPY_BYTES;
constexpr uint64_t seg_scratch_bytes(uint64_t spare) { return SEG_OFF_SPARE + spare; }
constexpr uint64_t SEGV_OFF_V = 0;
constexpr uint64_t SEGV_OFF_SNAPPY = SEG_COL_BYTES;
constexpr uint64_t SEGV_SCRATCH_BYTES = SEG_COL_BYTES + SEG_SNAPPY_BYTES;
/* k_scan_general's spare: the bitmap its time clip rebuilds, then the one
 * its cross-field predicate rebuilds */
constexpr uint64_t SEG_OFF_CLIP_BM = SEG_OFF_SPARE;
constexpr uint64_t SEG_OFF_XROW_BM = SEG_OFF_SPARE + SEG_BM_BYTES;
constexpr uint64_t SEG_SPARE_SCAN = 2 * SEG_BM_BYTES;
constexpr uint64_t SEG_SPARE_PAGE = 4096; /* unused pad of the rate family */

#ifdef __HIPCC__

/* a time segment that holds one raw little-endian timestamp
 * ([BlockIntegerOne][8B], chunkdata_builder.go:91-95) */
__host__ __device__ __forceinline__ bool seg_time_is_one(const uint8_t *tseg) {
  return tseg[0] == 18;
}

__device__ __forceinline__ int seg_iter_rc(int rc) {
  return rc == -2 ? GEMX_E_UNSUPPORTED : GEMX_E_DECODE;
}

/* ---------------- streaming reader ----------------
 *
 * For segments the host routed as nil-free and inside the query range.
 * open() once, then next(i, ...) for i = 0 .. rows-1 in order. Values come
 * back as int64 bits for every column type (d_bits_f for a float). */
template <int COLTYPE>
struct SegStream {
  TimeIter ti;
  SegHeader h;
  typename std::conditional<COLTYPE == GEMX_TYPE_FLOAT, FloatIter, IntIter>::type vit;
  /* const-delta timestamps (the regular-grid case, timestamp.go:190):
   * closed form, no per-row iterator dispatch */
  int t_const;
  int64_t t0c, dtc;

  /* gors != nullptr: a gorilla block with an arena slot is read from the
   * arena, anything else from the blob */
  __device__ __forceinline__ int open(const uint8_t *__restrict__ blob,
                                      const uint64_t *__restrict__ arena,
                                      const GorDesc *__restrict__ gors,
                                      uint32_t si, const gemx_seg_desc &d) {
    if (d.rows > (uint32_t)SEG_MAX_ROWS) return GEMX_E_INVALID;
    /* time segment: [BlockIntegerFull][rows u32][Time enc] or
     * [BlockIntegerOne][8B raw LE] (chunkdata_builder.go:91-95) */
    const uint8_t *tseg = blob + d.time_offset;
    if (seg_time_is_one(tseg)) {
      ti.kind = 1;
      ti.cur = (int64_t)d_u64le(tseg + 1);
      ti.delta = 0;
      ti.left = 1;
    } else if (tseg[0] == 32 && d.time_size > 5) {
      if (ti.init(tseg + 5, d.time_size - 5)) return GEMX_E_DECODE;
    } else {
      return GEMX_E_DECODE;
    }
    if (parse_data_header(blob + d.data_offset, d.data_size, COLTYPE, &h))
      return GEMX_E_DECODE;
    if (h.one_value) {
      if (h.enc_len < 8) return GEMX_E_DECODE; /* next() reads 8 raw bytes */
    } else {
      int vrc;
      if constexpr (COLTYPE == GEMX_TYPE_FLOAT) {
        if (gors && (h.enc[0] >> 4) == 3 && gors[si].arena_base != ~0ull)
          vrc = vit.init_gor_arena(arena, &gors[si]);
        else
          vrc = vit.init(h.enc, h.enc_len);
      } else {
        vrc = vit.init(h.enc, h.enc_len);
      }
      if (vrc) return seg_iter_rc(vrc);
    }
    t_const = (ti.kind == 1);
    t0c = t_const ? ti.cur : 0;
    dtc = t_const ? ti.delta : 0;
    if (t_const && ti.left < (int64_t)d.rows) return GEMX_E_DECODE;
    return 0;
  }

  __device__ __forceinline__ int next(int i, int64_t *t, int64_t *bits) {
    if (t_const) *t = t0c + (int64_t)i * dtc;
    else if (ti.next(t)) return GEMX_E_DECODE;
    if (h.one_value) {
      memcpy(bits, h.enc, 8);
    } else if constexpr (COLTYPE == GEMX_TYPE_FLOAT) {
      double fv;
      if (vit.next(&fv)) return GEMX_E_DECODE;
      *bits = d_f_bits(fv);
    } else {
      if (vit.next(bits)) return GEMX_E_DECODE;
    }
    return 0;
  }
};

/* ---------------- buffered reader ----------------
 *
 * Nil bitmaps, empty blocks, snappy, booleans, segments the query range
 * cuts. decode() fills tbuf (rows times) and vbuf (dense value bits: the
 * non-nil rows only) in the lane's scratch; row(i, ...) then walks the rows
 * in order. The members are plain: k_scan_general compacts tbuf / vbuf and
 * rewrites rows / dense / nilcount / h.bitmap in its clip and filter stages.
 *
 * After decode(): dense + nilcount == rows, and h.bitmap is non-null
 * whenever a row is nil (d_zero_bm for blocks that carry no bitmap bytes),
 * so bm_valid(&h, i) alone tells whether row i has a value. */
template <int COLTYPE>
struct SegBuffered {
  int64_t *tbuf, *vbuf;
  int rows, dense, nilcount;
  SegHeader h;
  int vIdx; /* next dense value row() hands out */

  /* the value half alone (k_eval_filter): vb takes SEG_COL_BYTES, sbuf
   * SEG_SNAPPY_BYTES */
  __device__ __forceinline__ int decode_values(const uint8_t *__restrict__ blob,
                                               const gemx_seg_desc &d,
                                               int64_t *vb, uint8_t *sbuf) {
    vbuf = vb;
    vIdx = 0;
    rows = (int)d.rows;
    if (d.rows > (uint32_t)SEG_MAX_ROWS) return GEMX_E_INVALID;
    if (parse_data_header(blob + d.data_offset, d.data_size, COLTYPE, &h))
      return GEMX_E_DECODE;
    if (h.one_value) {
      nilcount = h.nilcount;
      dense = 1 - nilcount;
      if (dense) {
        if (COLTYPE == GEMX_TYPE_BOOL) {
          vbuf[0] = h.enc[0] & 1; /* one byte */
        } else {
          if (h.enc_len < 8) return GEMX_E_DECODE;
          memcpy(&vbuf[0], h.enc, 8);
        }
      }
    } else if (h.enc_len == 0) { /* empty block */
      nilcount = h.nilcount;
      dense = 0;
    } else if (COLTYPE == GEMX_TYPE_BOOL) {
      /* bit-packed booleans unpack to int64 0/1 */
      dense = d_bool_decode(h.enc, h.enc_len, vbuf);
      if (dense < 0) return GEMX_E_DECODE;
      nilcount = h.bitmap ? h.nilcount : 0;
    } else if (COLTYPE == GEMX_TYPE_FLOAT) {
      if ((h.enc[0] >> 4) == 2) { /* snappy floats (compress.go:81-84,149) */
        int64_t dl = d_snappy_decode(h.enc + 1, h.enc_len - 1, sbuf, SEG_COL_BYTES);
        if (dl < 0 || dl % 8) return GEMX_E_DECODE;
        dense = (int)(dl / 8);
        for (int i = 0; i < dense; i++) vbuf[i] = (int64_t)d_u64le(sbuf + i * 8);
      } else {
        FloatIter fit;
        int rc = fit.init(h.enc, h.enc_len);
        if (rc) return seg_iter_rc(rc);
        dense = 0;
        double x;
        while (dense < SEG_MAX_ROWS && fit.next(&x) == 0) {
          memcpy(&vbuf[dense], &x, 8);
          dense++;
        }
      }
      nilcount = h.bitmap ? h.nilcount : 0;
    } else {
      IntIter iit;
      int rc = iit.init(h.enc, h.enc_len);
      if (rc) return seg_iter_rc(rc);
      dense = 0;
      int64_t x;
      while (dense < SEG_MAX_ROWS && iit.next(&x) == 0) {
        vbuf[dense] = x;
        dense++;
      }
      nilcount = h.bitmap ? h.nilcount : 0;
    }
    if (h.bitmap == nullptr && !h.one_value && h.enc_len > 0 && dense != rows &&
        h.nilcount == 0)
      return GEMX_E_DECODE;
    if (h.bitmap && dense + nilcount != rows) return GEMX_E_DECODE;
    if (!h.bitmap && nilcount == rows && rows > 0) {
      /* empty block / one-value null: no bitmap bytes, all rows nil */
      h.bitmap = d_zero_bm;
      h.bm_off = 0;
    }
    return 0;
  }

  /* lane_scratch: this lane's seg_scratch_bytes(spare) bytes */
  __device__ __forceinline__ int decode(const uint8_t *__restrict__ blob,
                                        const gemx_seg_desc &d,
                                        uint8_t *lane_scratch) {
    tbuf = (int64_t *)(lane_scratch + SEG_OFF_T);
    uint8_t *sbuf = lane_scratch + SEG_OFF_SNAPPY;
    if (d.rows > (uint32_t)SEG_MAX_ROWS) return GEMX_E_INVALID;
    const int n = (int)d.rows;
    const uint8_t *tseg = blob + d.time_offset;
    const int64_t tlen = d.time_size;
    if (tlen < 5) return GEMX_E_DECODE;
    if (seg_time_is_one(tseg)) {
      memcpy(&tbuf[0], tseg + 1, 8);
    } else {
      const uint8_t *enc = tseg + 5;
      const int64_t elen = tlen - 5;
      if ((enc[0] >> 4) == 3) { /* snappy: raw LE bytes (timestamp.go:274-297) */
        if (elen < 9) return GEMX_E_DECODE;
        int64_t comp_len = (int64_t)d_u32be(enc + 5);
        int64_t dl = d_snappy_decode(enc + 9, comp_len, sbuf, SEG_COL_BYTES);
        if (dl != n * 8) return GEMX_E_DECODE;
        for (int i = 0; i < n; i++) tbuf[i] = (int64_t)d_u64le(sbuf + i * 8);
      } else {
        TimeIter ti;
        int rc = ti.init(enc, elen);
        if (rc) return seg_iter_rc(rc);
        for (int i = 0; i < n; i++)
          if (ti.next(&tbuf[i])) return GEMX_E_DECODE;
      }
    }
    return decode_values(blob, d, (int64_t *)(lane_scratch + SEG_OFF_V), sbuf);
  }

  /* rows in order, i = 0 .. rows-1: *valid = 0 for a nil row (bits untouched) */
  __device__ __forceinline__ int value(int i, int64_t *bits, int *valid) {
    *valid = bm_valid(&h, i);
    if (*valid) {
      if (vIdx >= dense) return GEMX_E_DECODE;
      *bits = vbuf[vIdx++];
    }
    return 0;
  }
  __device__ __forceinline__ int row(int i, int64_t *t, int64_t *bits, int *valid) {
    *t = tbuf[i];
    return value(i, bits, valid);
  }
};

#endif /* __HIPCC__ */
#endif /* GEMX_SEGDECODE_HPP */
