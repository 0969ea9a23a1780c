"""Per-cell *_over_time planner and folds on the host (no GPU): the header
the engine includes (csrc/gemx_otwide.hpp) is compiled into a stand-alone
program with AddressSanitizer and UBSan. The program checks its own
invariants and runs the block scheme on small point sets with the functions
the kernels call; this test checks what it prints with numpy:

 - for every probe time (each edge, each edge +- 1 ns, each segment bound)
   cell(t) lies in [a_o, b_o] exactly when L_o <= t <= R_o;
 - a segment's cell range holds the cell of each of its bounds, and the
   slots obey  slots <= (2 * n_ord + 1) + (segments - 1)  for the
   time-disjoint cases;
 - a row folds its cells directly only when it is narrower than W."""

import os
import shutil
import subprocess

import numpy as np

from test_rate_wide_host import CASES, S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _disjoint(segs):
    return all(segs[i][1] < segs[i + 1][0] for i in range(len(segs) - 1))


def test_cells_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ot_wide_host")
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all",
         "-I", os.path.join(REPO, "opengemini_amd", "csrc"),
         os.path.join(REPO, "tests", "ot_wide_host_main.cpp"), "-o", exe],
        check=True)
    args = []
    for _, start, end, rng, step, segs in CASES:
        args += [start, end, rng, step, len(segs)]
        for a, b in segs:
            args += [a, b]
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == f"ok {len(CASES)}"
    it = iter(lines)
    kinds_seen = set()
    for name, start, end, rng, step, segs in CASES:
        g = next(it).split()
        assert g[0] == "grid", name
        n_ord, W, B, slots, states, blocks, s_min, n_steps, cmin, ncell = (
            int(x) for x in g[1:])
        ss = start + rng
        want_ord = 0 if end < ss else (1 if step == 0 else (end - ss) // step + 1)
        assert n_ord == want_ord, name
        if n_ord == 0:
            continue
        est = step or 1
        assert W == 2 * (rng // est) + 1, name
        assert B == min(W, 2 * n_ord + 1), name
        o = np.arange(n_ord, dtype=np.int64)
        L = start + o * est
        R = L + rng

        def cell(t):
            return int((L <= t).sum() + (R < t).sum())

        # segments: the cell of each bound, and the slot bound
        total = 0
        for k, (mn, mx) in enumerate(segs):
            f = next(it).split()
            assert f[0] == "seg" and int(f[1]) == k, name
            c0, ncells = int(f[2]), int(f[3])
            assert c0 == cell(mn), (name, k)
            assert c0 + ncells - 1 == cell(mx), (name, k)
            assert cmin <= c0 and c0 + ncells <= cmin + ncell, (name, k)
            total += ncells
        assert total == slots, name
        if _disjoint(segs):
            assert 0 < slots <= (2 * n_ord + 1) + (len(segs) - 1), name
        assert states == ncell <= 2 * n_ord + 1, name
        # rows of the ring path: first R >= first point, last L <= last point
        tmin = min(a for a, _ in segs)
        tmax = max(b for _, b in segs)
        lo, hi = int((R < tmin).sum()), int((L <= tmax).sum())
        assert (s_min, n_steps) == (lo, max(hi - lo, 0)), name

        a_o = np.zeros(n_ord, dtype=np.int64)
        b_o = np.zeros(n_ord, dtype=np.int64)
        for i in range(n_ord):
            f = next(it).split()
            assert f[0] == "ord" and int(f[1]) == i, name
            a_o[i], b_o[i] = int(f[2]), int(f[3])
            width = b_o[i] - a_o[i] + 1
            assert 1 <= width <= W, (name, i)
            if f[4] == "fold":
                assert width < W, (name, i, "a full-width row folds")
            else:
                assert f[4] in ("join", "prefix", "suffix"), name
            kinds_seen.add(f[4])
        # interior ordinals have the full width
        k = rng // est
        inner = (o >= k) & (o + k + 1 <= n_ord)
        assert np.all((b_o - a_o + 1)[inner] == W), name

        probes = set()
        for d in (-1, 0, 1):
            probes |= set((L + d).tolist()) | set((R + d).tolist())
        for mn, mx in segs:
            probes |= {mn, mx}
        seen = set()
        for f in it:
            f = f.split()
            if f[0] == "end":
                break
            assert f[0] == "probe", name
            t, c = int(f[1]), int(f[2])
            seen.add(t)
            assert c == cell(t), (name, t)
            inside = (L <= t) & (t <= R)
            in_cells = (a_o <= c) & (c <= b_o)
            assert np.array_equal(inside, in_cells), (name, t)
        assert seen == probes, name
    # the cases reach every way of answering a row
    assert kinds_seen == {"join", "prefix", "suffix", "fold"}, kinds_seen
    assert S == 10**9
