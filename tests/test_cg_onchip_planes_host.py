"""The on-chip conjugate-gradient kernel on coefficient planes (kernels_cg_image_planes.hpp, tuning key "cg_onchip_planes"), host
side: the kernel's scratch / LDS / occupancy on the ISA hipcc emits for gfx950, the names the older tests find their kernels by,
and the words of the header and the Python layer.  No GPU needed."""
import inspect
import os

from conftest import ROOT
from test_cg_onchip_host import cg_usage
from test_cg_stream_host import OLD_KERNELS


def test_plane_image_kernel_resources():
    """k_cgp_image: one workgroup of 1024 threads per compute unit has to be resident, which takes 4 waves per SIMD (128 VGPRs a
    lane at most); nothing may spill -- x, r and a pair's row live in registers, and scratch would be a second stream of
    memory traffic in a kernel that is bound by its loads --, no AGPR, and p (128 KiB) + the wave sums fit the CU's 160 KiB of
    LDS (no table: less than k_cg_image takes)."""
    got = {k: v for k, v in cg_usage().items() if k.startswith("_ZN4deff11k_cgp_imageE")}
    assert len(got) == 1, list(got)
    (name, u), = got.items()
    print(name, u)
    assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, u
    assert u["Occupancy"] >= 4 and u["VGPRs"] <= 128, u
    assert 128 * 1024 <= u["LDS"] <= 163840, u
    table = [v for k, v in cg_usage().items() if "10k_cg_image" in k]
    assert len(table) == 1 and u["LDS"] < table[0]["LDS"], (u, table)


def test_plane_image_kernel_does_not_shadow_the_pinned_names():
    """The older host tests find kernels by length-prefixed pieces of their mangled names ("10k_cg_image", ...): each of those
    is still exactly one symbol."""
    usage = cg_usage()
    for k in OLD_KERNELS:
        tag = f"{len(k)}{k}"
        assert len([s for s in usage if tag in s]) == 1, (k, [s for s in usage if tag in s])


def test_header_and_python_document_the_key():
    text = open(os.path.join(ROOT, "include", "deff_amd.h")).read()
    assert '"cg_onchip_planes"' in text
    assert "4 = on chip on the coefficient planes" in text           # deff_get_plan "cg_impl"
    doc = " ".join(text[text.index('Tuning key "cg_onchip_planes"'):].split("*/")[0].replace(" * ", " ").split())
    for words in ('"cg_impl" = 4', '"cg_fold" = 0', "16 384 cells", "deff_solve_adjoint", "deff_solve_tangent",
                  "deff_solve_adjoint_tangent", "DEFF_EINVAL", "deff_solve_cg_stream", "row slabs"):
        assert words in doc, words
    from effectivediffusivityfvm_amd import autograd
    from effectivediffusivityfvm_amd.solver import Solver
    assert "cg_onchip_planes" in Solver.solve_cg.__doc__ and "cg_onchip_planes" in Solver.plan.__doc__
    assert "4 one image per compute unit on the coefficient" in " ".join(Solver.plan.__doc__.split())
    for fn in (autograd.effective_diffusivity, autograd.concentration_field):
        assert inspect.signature(fn).parameters["onchip"].default is False
        assert "cg_onchip_planes" in fn.__doc__ and "overwritten" in fn.__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "cg_onchip_planes" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "On chip, planes" in design and "k_cgp_image" in design
