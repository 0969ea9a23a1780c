"""Fold plan cut arithmetic on the host (no GPU): the header the engine
includes (csrc/gemx_foldsplit.hpp) is compiled into a stand-alone program
with AddressSanitizer and UBSan and swept over awkward shapes; the run
counts it prints for the GPU tests' shapes must equal test_gpu_fold_split's
transcription of the rule, which those tests' expectations rest on."""

import os
import shutil
import subprocess

import test_gpu_fold_split as fs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (t0 s, dt s, rows, interval s) of the GPU cases (offset folded into t0)
SHAPES = [(0, 1, 300, 60), (-157, 1, 300, 60), (7, 1, 333, 45),
          (0, 90, 200, 60), (0, 1, 256, 60), (0, 1, 120, 60), (0, 1, 240, 60)]


def test_cut_rule_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fold_split_host")
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all",
         "-I", os.path.join(REPO, "opengemini_amd", "csrc"),
         os.path.join(REPO, "tests", "fold_split_host_main.cpp"), "-o", exe],
        check=True)
    args, want = [], []
    for t0, dt, rows, iv in SHAPES:
        b = fs._bounds(t0 * fs.S, dt * fs.S, rows, interval=iv * fs.S)
        for k in range(1, 9):
            for stride in (16, 32, 64):
                args += [t0, dt, rows, iv, k, stride]
                want.append(len(fs._cuts(b, k, stride)) - 1)
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split()
    assert lines[-2] == "ok" and int(lines[-1]) > 10_000
    assert [int(x[5:]) for x in lines if x.startswith("runs=")] == want
