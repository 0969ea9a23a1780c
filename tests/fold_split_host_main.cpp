/* Stand-alone host check of the fold plan's cut arithmetic
 * (opengemini_amd/csrc/gemx_foldsplit.hpp). Built with sanitizers by
 * test_fold_split_host.py; exits 0 when every invariant holds.
 *
 * Sweeps (t0, dt, rows, interval, K, checkpoint stride) over small and
 * awkward values, builds the row-boundary table the plan builds, cuts it,
 * and checks: cuts are increasing from 0 to nw; every run keeps >= 2
 * windows and >= min_rows rows when there is more than one run; each cut
 * lies within one window of the even cut; the resume checkpoint lies at or
 * below the run's first row, inside the segment, with skip < stride.
 * Prints "runs=<n>" lines for the shapes named on the command line
 * (t0_s dt_s rows interval_s K stride), which the test compares with its
 * own transcription of the rule. */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gemx_foldsplit.hpp"

static std::vector<uint32_t> bounds(int64_t t0, int64_t dt, uint32_t rows,
                                    int64_t interval) {
  auto ord = [&](int64_t t) {
    int64_t q = t / interval;
    if (t % interval < 0) q--;
    return q;
  };
  const int64_t wf = ord(t0), wl = ord(t0 + (int64_t)(rows - 1) * dt);
  std::vector<uint32_t> b;
  b.push_back(0);
  for (int64_t k = 0; k <= wl - wf; k++) {
    const int64_t we = (wf + k + 1) * interval;
    int64_t nb = (we - t0 + dt - 1) / dt;
    if (nb > rows) nb = rows;
    b.push_back((uint32_t)nb);
  }
  return b;
}

static int check(const std::vector<uint32_t> &b, uint32_t K, uint32_t S,
                 uint32_t min_rows, uint32_t *runs_out) {
  const uint32_t nw = (uint32_t)b.size() - 1, rows = b[nw];
  std::vector<uint32_t> cut(K + 1, 0xdeadbeef);
  const uint32_t runs = fold_split_cuts(b.data(), nw, K, S, min_rows, cut.data());
  *runs_out = runs;
  if (runs < 1 || runs > K) return 1;
  if (cut[0] != 0 || cut[runs] != nw) return 2;
  for (uint32_t j = 0; j < runs; j++) {
    if (cut[j + 1] <= cut[j]) return 3;
    if (runs > 1) {
      if (cut[j + 1] - cut[j] < 2) return 4;
      if (b[cut[j + 1]] - b[cut[j]] < min_rows) return 5;
    }
    if (j > 0) {
      const int64_t e = ((int64_t)j * nw + runs / 2) / runs;
      if ((int64_t)cut[j] < e - 1 || (int64_t)cut[j] > e + 1) return 6;
      const uint32_t r0 = b[cut[j]], c = r0 / S, skip = r0 % S;
      if (r0 >= rows || c * S + skip != r0 || c > (rows - 1) / S) return 7;
    }
  }
  return 0;
}

int main(int argc, char **argv) {
  /* one nearly full round where it exists, else 2 1/4 rounds */
  if (fold_split_k(1024, 0) != 4 || fold_split_k(1250, 0) != 3 ||
      fold_split_k(2048, 0) != 2 || fold_split_k(1563, 0) != 6 ||
      fold_split_k(3125, 0) != 3 || fold_split_k(4096, 0) != 1 ||
      fold_split_k(9216, 0) != 1 || fold_split_k(100000, 0) != 1 ||
      fold_split_k(1, 0) != 8 || fold_split_k(0, 0) != 1 ||
      fold_split_k(99, 5) != 5 || fold_split_k(99, 100) != 8) {
    printf("fold_split_k\n");
    return 1;
  }
  uint64_t n = 0;
  const int64_t dts[] = {1, 7, 59, 60, 90, 1000};
  const uint32_t rowss[] = {1, 2, 63, 64, 127, 128, 129, 200, 333, 1000, 4096};
  const int64_t ints[] = {1, 45, 60, 300, 100000};
  const uint32_t strides[] = {16, 32, 64};
  for (int64_t t0 = -150; t0 <= 150; t0 += 37)
    for (int64_t dt : dts)
      for (uint32_t rows : rowss)
        for (int64_t iv : ints) {
          if ((int64_t)rows * dt / iv > 20000) continue; /* table size */
          const std::vector<uint32_t> b = bounds(t0, dt, rows, iv);
          for (uint32_t K = 1; K <= 8; K++)
            for (uint32_t S : strides) {
              uint32_t runs;
              const int rc = check(b, K, S, 64, &runs);
              if (rc) {
                printf("invariant %d: t0=%lld dt=%lld rows=%u iv=%lld K=%u S=%u\n",
                       rc, (long long)t0, (long long)dt, rows, (long long)iv, K, S);
                return 1;
              }
              n++;
            }
        }
  for (int a = 1; a + 5 < argc; a += 6) {
    const std::vector<uint32_t> b = bounds(atoll(argv[a]), atoll(argv[a + 1]),
                                           (uint32_t)atoi(argv[a + 2]),
                                           atoll(argv[a + 3]));
    uint32_t runs;
    if (check(b, (uint32_t)atoi(argv[a + 4]), (uint32_t)atoi(argv[a + 5]), 64,
              &runs))
      return 1;
    printf("runs=%u\n", runs);
  }
  printf("ok %llu\n", (unsigned long long)n);
  return 0;
}
