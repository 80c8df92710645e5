"""Neighbour lists of a chained streaming launch (csrc/tb_chain.hpp): tests/cpp/tb_chain_lists.cpp, a stand-alone program with
its own main, built with AddressSanitizer + UBSan and run on the CPU.  It draws random tile tables (1-12 strips, ragged nx, both
strip placements, 1-3 images, random cuts of at least T rows, waves without a tile), checks every tile's list against a
cell-by-cell brute force of  own(n) & window(t)  and  window(n) & own(t),  and checks that tables whose lists do not fit are
reported as such."""
import os
import subprocess

from conftest import ROOT


def test_lists_equal_brute_force_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tb_chain_lists")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "tb_chain_lists.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for seed in ("20260", "7"):
        r = subprocess.run([exe, "300", seed], capture_output=True, text=True, timeout=300)
        print(r.stdout.strip())
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert "equal to the brute force" in r.stdout and "correctly refused" in r.stdout
