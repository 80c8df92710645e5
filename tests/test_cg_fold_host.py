"""The folded conjugate-gradient launches (kernels_cg_fold.hpp, tuning key "cg_fold") and the driver's --cg-fold, host side:
the register, scratch and LDS figures of the new kernels on the ISA hipcc emits for gfx950, the names the older tests find
their kernels by, the header's words and the option's refusals.  No GPU needed."""
import os
import subprocess

from conftest import ROOT
from test_cg_onchip_host import EXE, cg_usage
from test_cg_planes_host import PLANE_KERNELS
from test_cg_stream_host import OLD_KERNELS, kernels_by_name

TABLE_FOLD = ("k_cgf_dir", "k_cgf_dir2", "k_cgf_update")
PLANE_FOLD = ("k_cgpf_dir", "k_cgpf_update")
TABLE_LDS = 29120                                                    # the 7-plane row table (kernels_cg.hpp)


def test_fold_kernels_resources():
    """Each new kernel is one symbol; nothing spills, no AGPR.  The table form stays in its parents' class (<= 96 VGPRs, the
    table's LDS plus at most 512 bytes for the tail, 5 waves per SIMD) -- k_cgf_dir2 with its two rows of loads in flight
    included --; the plane form has no table: <= 96 VGPRs, 5 waves per SIMD, at most 512 bytes of LDS."""
    got = kernels_by_name(TABLE_FOLD + PLANE_FOLD)
    assert set(got) == set(TABLE_FOLD + PLANE_FOLD), sorted(got)
    for k, u in got.items():
        print(k, u)
        assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, (k, u)
        assert u["VGPRs"] <= 96 and u["Occupancy"] >= 5, (k, u)
    for k in TABLE_FOLD:
        assert TABLE_LDS <= got[k]["LDS"] <= TABLE_LDS + 512, (k, got[k])
    for k in PLANE_FOLD:
        assert got[k]["LDS"] <= 512, (k, got[k])


def test_fold_kernels_do_not_shadow_the_pinned_names():
    """The older host tests find kernels by length-prefixed pieces of their mangled names: each of those is still exactly one
    symbol."""
    usage = cg_usage()
    for k in OLD_KERNELS + PLANE_KERNELS:
        tag = f"{len(k)}{k}"
        assert len([s for s in usage if tag in s]) == 1, (k, [s for s in usage if tag in s])


def test_header_documents_cg_fold():
    text = open(os.path.join(ROOT, "include", "deff_amd.h")).read()
    assert '"cg_fold"' in text
    doc = " ".join(text[text.index('Tuning key "cg_fold"'):].split("*/")[0].replace("\n *", "\n").split())
    for words in ("two launches", "last workgroup", "bit for bit", "deff_solve_cg_stream", "on-chip", "row slabs",
                  'deff_get_plan "cg_fold"'):
        assert words in doc, words
    from effectivediffusivityfvm_amd.solver import Solver
    assert "cg_fold" in Solver.solve_cg.__doc__ and "cg_fold" in Solver.solve_cg_stream.__doc__


def test_help_names_cg_fold():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--cg-fold" in r.stdout


def test_cg_fold_refusals(tmp_path):
    """Exit 2 with a message, before the input file is read or a device touched (there is no input.txt here, and no GPU)."""
    for args, word in ((["input.txt", "--cg-fold", "1"], "--solver cg"),
                       (["input.txt", "--cg-fold", "1", "--solver", "jacobi"], "--solver cg"),
                       (["input.txt", "--solver", "cg", "--cg-fold", "3"], "--cg-fold"),
                       (["input.txt", "--cg-fold", "-1", "--solver", "cg"], "--cg-fold"),
                       (["input.txt", "--solver", "cg", "--cg-fold", "one"], "--cg-fold"),
                       (["input.txt", "--solver", "cg", "--cg-fold", "1x"], "--cg-fold")):
        r = subprocess.run([EXE] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert word in r.stderr and not r.stdout, (args, r.stderr, r.stdout)
    assert not os.listdir(tmp_path)
