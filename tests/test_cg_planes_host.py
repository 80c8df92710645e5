"""Conjugate gradients on the coefficient planes (kernels_cg_planes.hpp, tuning key "cg_planes"), host side: the register,
scratch and LDS figures of the new kernels on the ISA hipcc emits for gfx950, the names the older tests find their kernels
by, and the header's words.  No GPU needed."""
import os

from conftest import ROOT
from test_cg_onchip_host import cg_usage
from test_cg_stream_host import OLD_KERNELS

PLANE_KERNELS = ("k_cgp_prepare", "k_cgp_dir", "k_cgp_update", "k_cgp_resid")


def plane_kernels():
    got = {}
    for sym, u in cg_usage().items():
        for k in PLANE_KERNELS:
            if sym.startswith(f"_ZN4deff{len(k)}{k}E"):
                assert k not in got, (k, sym)
                got[k] = u
    return got


def test_plane_kernels_resources():
    """Nothing spills, no AGPR, no LDS at all (there is no row table; the wave sums go through DPP) and at least the table
    form's 5 waves per SIMD -- here registers alone bound the occupancy, so that is <= 96 VGPRs.  (The counts of the build
    are in DESIGN.md section 9, "Planes".)"""
    got = plane_kernels()
    assert set(got) == set(PLANE_KERNELS), sorted(got)
    for k, u in got.items():
        print(k, u)
        assert u["ScratchSize"] == 0 and u["AGPRs"] == 0 and u["LDS"] == 0, (k, u)
        assert u["Occupancy"] >= 5 and u["VGPRs"] <= 96, (k, u)


def test_plane_kernels_do_not_shadow_the_pinned_names():
    """test_cg_host.py, test_cg_onchip_host.py and test_cg_stream_host.py find kernels by length-prefixed pieces of their
    mangled names: each of those is still exactly one symbol."""
    usage = cg_usage()
    for k in OLD_KERNELS:
        tag = f"{len(k)}{k}"
        assert len([s for s in usage if tag in s]) == 1, (k, [s for s in usage if tag in s])


def test_header_documents_the_key():
    text = open(os.path.join(ROOT, "include", "deff_amd.h")).read()
    assert '"cg_planes"' in text
    assert "3 = on the coefficient planes" in text                  # deff_get_plan "cg_impl"
    doc = " ".join(text[text.index('Tuning key "cg_planes"'):].split("*/")[0].split())
    for words in ("no dictionary", '"cg_impl" = 3', "row-slab", "explicit-only", "deff_solve_cg_stream"):
        assert words in doc, words
    from effectivediffusivityfvm_amd.solver import Solver
    assert "cg_planes" in Solver.solve_cg.__doc__
