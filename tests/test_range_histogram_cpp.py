"""Builds and runs tests/cpp/test_range_histogram.cpp: the C++ mirror's shift_report (kzero_amd/csrc/host/hip_network.hpp) on the
crafted histograms of tests/range_hist_ref.py, with the numbers the numpy restatement gives — the tables and numbers of
tests/test_range_histogram.py —, built the way tests/test_stream_shift_cpp.py builds its program.  Needs no GPU."""
import os
import subprocess

from tests import range_hist_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BUILD = os.path.join(CPP, "build")
GOLDEN = os.path.join(REPO, "tests", "golden")


def test_cpp_mirror_shift_report(tmp_path):
    os.makedirs(BUILD, exist_ok=True)
    lib = os.path.join(REPO, "kzero_amd")
    exe = os.path.join(BUILD, "test_range_histogram")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-pthread", os.path.join(CPP, "test_range_histogram.cpp"),
                           "-o", exe, f"-L{lib}", "-lkzhip", f"-Wl,-rpath,{lib}"])
    lines, cases = [], 0
    for name, hist in sorted(R.crafted_tables().items()):
        for k in R.REPORT_KS:
            want = R.shift_report_ref(hist, k)
            lines.append(f"case {name} {hist.shape[0]} {k}")
            lines += [" ".join(str(int(v)) for v in row) for row in hist]
            lines += [" ".join(str(int(want[f][site])) for f in R.FIELDS) for site in range(hist.shape[0])]
            cases += 1
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path), os.path.join(GOLDEN, "ataxx7_4x64.kzm")], capture_output=True, text=True, timeout=100)
    assert out.returncode == 0 and f"range histogram tests ok: {cases} cases" in out.stdout, out.stdout + out.stderr
