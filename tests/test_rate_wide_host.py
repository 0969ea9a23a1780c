"""Edge-record rate planner on the host (no GPU): the header the engine
includes (csrc/gemx_ratewide.hpp) is compiled into a stand-alone program
with AddressSanitizer and UBSan. The program checks the ownership
invariants edge by edge; this test compares the left/right ordinal runs it
prints with numpy's searchsorted over max_time / min_time."""

import os
import shutil
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 10**9
E = 1_700_000_000 * S  # a production epoch, ~1.7e18 ns


def _segs(t0, spans):
    """[(min, max)] from (gap_before, length) pairs starting at t0."""
    out, t = [], t0
    for gap, ln in spans:
        t += gap
        out.append((t, t + ln))
        t += ln
    return out


# (name, start, end, range, step, [(min_time, max_time)])
CASES = [
    ("adjoining", 0, 900 * S, 300 * S, 60 * S,
     _segs(0, [(0, 299 * S), (S, 299 * S), (S, 299 * S)])),
    ("wide ratio", 0, 900 * S, 600 * S, 10 * S,
     _segs(0, [(0, 299 * S), (S, 299 * S), (S, 299 * S)])),
    ("gaps longer than the range", 0, 2000 * S, 120 * S, 30 * S,
     _segs(50 * S, [(0, 100 * S), (500 * S, 80 * S), (700 * S, 60 * S)])),
    ("shared boundary", 0, 600 * S, 120 * S, 30 * S,
     [(0, 150 * S), (150 * S, 300 * S), (300 * S, 300 * S), (300 * S, 450 * S)]),
    ("one-row segments", 0, 400 * S, 60 * S, 10 * S,
     [(100 * S, 100 * S), (130 * S, 130 * S), (131 * S, 131 * S),
      (200 * S, 260 * S)]),
    ("negative times", -1000 * S, -100 * S, 300 * S, 60 * S,
     _segs(-950 * S, [(0, 200 * S), (S, 250 * S), (40 * S, 300 * S)])),
    ("production epoch", E - 7, E + 900 * S, 601 * S, 7 * S,
     _segs(E, [(0, 299 * S), (S, 299 * S), (S, 299 * S)])),
    ("range < step", 0, 900 * S, 5 * S, 20 * S,
     _segs(3 * S, [(0, 250 * S), (S, 299 * S), (17 * S, 200 * S)])),
    ("range not a multiple of step", 0, 900 * S, 601 * S, 7 * S,
     _segs(0, [(0, 299 * S), (S, 299 * S), (S, 299 * S)])),
    ("off-grid edges", S // 2, 900 * S + S // 2, 600 * S, 10 * S,
     _segs(0, [(0, 299 * S), (S, 299 * S), (S, 299 * S)])),
    ("step == 0", 0, 900 * S, 300 * S, 0,
     _segs(0, [(0, 299 * S), (S, 299 * S), (S, 299 * S)])),
    ("step == 0 in a gap", 0, 900 * S, 100 * S, 0,
     [(0, 50 * S), (400 * S, 500 * S)]),
    ("series after start+range", 0, 900 * S, 120 * S, 30 * S,
     _segs(400 * S, [(0, 100 * S), (S, 100 * S)])),
    ("series outside the query", 5000 * S, 6000 * S, 120 * S, 30 * S,
     _segs(0, [(0, 100 * S), (S, 100 * S)])),
    ("series beyond the query", 0, 600 * S, 120 * S, 30 * S,
     _segs(5000 * S, [(0, 100 * S), (S, 100 * S)])),
    ("end before start+range", 0, 100 * S, 300 * S, 60 * S,
     _segs(0, [(0, 299 * S)])),
    ("single segment", 0, 900 * S, 3600 * S, 60 * S, [(0, 299 * S)]),
]


def _expected(start, end, rng, step, segs):
    """Runs by the ownership rule, with searchsorted."""
    mn = np.array([a for a, _ in segs], dtype=np.int64)
    mx = np.array([b for _, b in segs], dtype=np.int64)
    ss = start + rng
    if end < ss:
        return 0, [(set(), set()) for _ in segs], 0
    n_ord = 1 if step == 0 else (end - ss) // step + 1
    o = np.arange(n_ord, dtype=np.int64)
    R = ss + o * (step or 1)
    L = R - rng
    lown = np.searchsorted(mx, L, side="left")        # first max_time >= L
    rown = np.searchsorted(mn, R, side="right") - 1   # last min_time <= R
    row = (lown < len(segs)) & (rown >= 0)
    runs = []
    for k in range(len(segs)):
        runs.append((set(o[row & (lown == k)].tolist()),
                     set(o[row & (rown == k)].tolist())))
    return int(n_ord), runs, int(row.sum())


def test_planner_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rate_wide_host")
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all",
         "-I", os.path.join(REPO, "opengemini_amd", "csrc"),
         os.path.join(REPO, "tests", "rate_wide_host_main.cpp"), "-o", exe],
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
    for name, start, end, rng, step, segs in CASES:
        exp = _expected(start, end, rng, step, segs)
        g = next(it).split()
        assert g[0] == "grid", name
        n_ord, s_min, n_steps, recs = (int(x) for x in g[1:])
        assert n_ord == exp[0], name
        rows = exp[2] if n_ord else 0
        assert n_steps == rows, name
        assert recs == 2 * rows <= 2 * max(n_ord, 0), name
        for k in range(len(segs)):
            f = next(it).split()
            assert f[0] == "seg" and int(f[1]) == k, name
            l0, nl, r0, nr = (int(x) for x in f[2:])
            want_l, want_r = exp[1][k]
            assert set(range(l0, l0 + nl)) == want_l, (name, k, "left")
            assert set(range(r0, r0 + nr)) == want_r, (name, k, "right")
        if rows:
            lo = min(min(a | b) for a, b in exp[1] if a | b)
            assert s_min == lo, name
