"""The flood fill on bitmaps and the 3-phase row numbering on the CPU: tests/cpp/fill_bits.cpp, a stand-alone program with its
own main, built with AddressSanitizer + UBSan.  Part one runs csrc/fill_step.hpp -- the word step the fill kernels run -- as a
whole fill, in the single-workgroup form and in row tiles of 1..8 rows, against deff::flood_fill (Grid and PathFlag) on random
masks (widths 2 .. 258 around the word boundaries, heights 2 .. 40, solid fractions 0.2 .. 0.9, a third with the top-left
cell solid) and on designed ones (serpentines, a pore reachable only through the wrap between the first and last row, a solid
left column, all open, all solid, solid cells in the last column under the reference's quirk), and checks every round count
against the cap formula.  Part two checks csrc/row_index3.hpp: dense, injective, 451 at most, blind to neighbours without a
link, every table row fvm_row of its tuple byte for byte."""
import os
import subprocess

from conftest import ROOT


def test_fill_and_row_index_under_sanitizers(tmp_path):
    exe = str(tmp_path / "fill_bits")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tests", "cpp", "shim"),
                        "-I", os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "fill_bits.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for seed in ("20260", "7"):
        r = subprocess.run([exe, "400", seed], capture_output=True, text=True, timeout=300)
        print(r.stdout.strip())
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert "fills equal to flood_fill" in r.stdout and "dense and injective" in r.stdout and "all checks passed" in r.stdout
