/* Row split of folded gorilla waves: host-side plan arithmetic.
 *
 * A folding wave covers nw windows whose row boundaries are b[0..nw]
 * (b[0] = 0, b[nw] = rows, non-decreasing; an empty window has
 * b[k] == b[k + 1]). The plan cuts the window list into K contiguous runs
 * that run as separate wave-tasks, each resuming the decode from the
 * attach-time checkpoint below its first row. Plain functions with no
 * engine state, so they can be compiled into a stand-alone host program. */
#pragma once
#include <cstdint>

/* Runs per folding wave, 1..8. The scan kernel's registers allow 4 waves
 * per SIMD, 4096 wave-tasks resident on 256 CUs x 4 SIMDs. Measured
 * (DESIGN.md section 5 note 7), a launch is fastest either as one resident
 * round that nearly fills those slots, where nothing waits for a tail, or
 * with tasks small and many enough that the dispatcher evens the tail out;
 * a little over one round is the worst place to be (the K = 3 that
 * ceil(4096 / n_waves) gives the 1563-wave headline shard measured slower
 * than every K from 4 to 8). So: the largest K that fits one round if that
 * round is at least 7/8 full, else about 2 1/4 rounds. forced > 0
 * (GEMX_FOLD_SPLIT) overrides the policy. */
static inline uint32_t fold_split_k(uint64_t n_waves, uint32_t forced) {
  if (forced > 0) return forced > 8 ? 8 : forced;
  if (n_waves == 0) return 1;
  const uint64_t slots = 4 * 1024;
  uint64_t k = slots / n_waves;
  if (k > 8) k = 8;
  if (k >= 1 && k * n_waves * 8 >= slots * 7) return (uint32_t)k;
  k = (slots * 9 / 4 + n_waves - 1) / n_waves;
  return (uint32_t)(k < 1 ? 1 : (k > 8 ? 8 : k));
}

/* Cut windows [0, nw) into at most K runs; cut[j] is the first window of
 * run j and cut[runs] = nw (cut must hold K + 1 entries). Every run keeps
 * at least 2 windows and min_rows rows. Run j starts within one window of
 * the even cut round(j * nw / runs), at the candidate whose first row
 * b[w] lies closest above a checkpoint row (multiple of ckpt_rows): those
 * are the records the run decodes only to throw away. The earliest
 * candidate wins ties (an empty window and its successor start on the same
 * row). When a cut has no valid candidate the wave gets one run fewer.
 * Returns the number of runs (>= 1). */
static inline uint32_t fold_split_cuts(const uint32_t *b, uint32_t nw,
                                       uint32_t K, uint32_t ckpt_rows,
                                       uint32_t min_rows, uint32_t *cut) {
  const uint32_t rows = b[nw];
  uint32_t runs = K < 1 ? 1 : K;
  if (runs > nw / 2) runs = nw / 2;
  if (min_rows > 0 && runs > rows / min_rows) runs = rows / min_rows;
  if (runs < 1) runs = 1;
  for (; runs > 1; runs--) {
    bool ok = true;
    cut[0] = 0;
    for (uint32_t j = 1; j < runs && ok; j++) {
      const uint32_t e = (uint32_t)(((uint64_t)j * nw + runs / 2) / runs);
      const int64_t cand[3] = {(int64_t)e - 1, (int64_t)e, (int64_t)e + 1};
      int64_t best = -1;
      uint32_t best_d = 0;
      for (int64_t w : cand) {
        if (w < (int64_t)cut[j - 1] + 2) continue;
        if (w + 2 * (int64_t)(runs - j) > (int64_t)nw) continue;
        const uint32_t r0 = b[w];
        if (r0 - b[cut[j - 1]] < min_rows) continue;
        if ((uint64_t)(rows - r0) < (uint64_t)min_rows * (runs - j)) continue;
        const uint32_t d = r0 % ckpt_rows;
        if (best < 0 || d < best_d) {
          best = w;
          best_d = d;
        }
      }
      if (best < 0)
        ok = false;
      else
        cut[j] = (uint32_t)best;
    }
    if (ok) break;
  }
  cut[0] = 0;
  cut[runs] = nw;
  return runs;
}
