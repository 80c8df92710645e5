"""deff_solve_cg_stream (api_cg.hip, kernels_cg_stream.hpp) and the driver's --cg-stream, host side: the symbol and its
argument checks, the slot-list kernels' register / scratch / LDS figures on the ISA hipcc emits for gfx950, and the option's
refusals, which come before any file or device is touched.  No GPU needed.  (The figures of the kernels the stream iterates
with are pinned by test_cg_host.py and test_cg_onchip_host.py, which this change leaves as they are.)"""
import ctypes as C
import os
import subprocess

from conftest import ROOT
from test_cg_onchip_host import EXE, cg_usage

NEW_KERNELS = ("k_cgs_resid", "k_cgs_check", "k_cgs_enter", "k_cgs_admissible", "k_cgs_flux")
OLD_KERNELS = ("k_cg_image", "k_cg_dir", "k_cg_update", "k_cg_resid", "k_cg_alpha", "k_cg_beta", "k_cg_check", "k_cg_admissible")


def test_library_exports_solve_cg_stream():
    lib = os.path.join(ROOT, "effectivediffusivityfvm_amd", "libdeff_amd.so")
    assert os.path.exists(lib), "libdeff_amd.so is not built"
    L = C.CDLL(lib)
    assert hasattr(L, "deff_solve_cg_stream")
    from effectivediffusivityfvm_amd import _capi
    assert "deff_solve_cg_stream" in _capi.SYMBOLS
    # argument checks come before any device work: no context, then no callbacks
    nxt = _capi.NEXT_IMAGE_FN(lambda *a: 0)
    dn = _capi.CG_IMAGE_DONE_FN(lambda *a: None)
    d = C.c_double
    args = (C.c_int(8), C.c_int(8), C.c_int(1), C.c_int(1), d(1e-3), d(1.0), d(0.0), d(1.0), d(1e-10), C.c_int64(10), C.c_int64(1))
    assert L.deff_solve_cg_stream(None, *args, nxt, dn, None) == -1
    assert L.deff_solve_cg_stream(C.c_void_p(1), *args, None, None, None) == -1


def kernels_by_name(names):
    got = {}
    for sym, u in cg_usage().items():
        for k in names:
            if sym.startswith(f"_ZN4deff{len(k)}{k}E"):
                assert k not in got, (k, sym)
                got[k] = u
    return got


def test_slot_list_kernels_resources():
    """Nothing spills and no AGPR is used; k_cgs_resid stays in its parent's class (<= 96 VGPRs, the 7-plane table's 28.4 KiB
    of LDS, 5 waves per SIMD), as does k_cgs_admissible; k_cgs_check stays with the per-image reductions (<= 32 VGPRs)."""
    got = kernels_by_name(NEW_KERNELS)
    assert set(got) == set(NEW_KERNELS), sorted(got)
    for k, u in got.items():
        print(k, u)
        assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, (k, u)
    for k in ("k_cgs_resid", "k_cgs_admissible"):
        assert got[k]["VGPRs"] <= 96 and got[k]["LDS"] <= 29184 and got[k]["Occupancy"] >= 5, (k, got[k])
    assert got["k_cgs_check"]["VGPRs"] <= 32 and got["k_cgs_check"]["LDS"] <= 64, got["k_cgs_check"]
    for k in ("k_cgs_enter", "k_cgs_flux"):
        assert got[k]["VGPRs"] <= 64 and got[k]["LDS"] == 0, (k, got[k])


def test_new_kernels_do_not_shadow_the_pinned_names():
    """test_cg_host.py and test_cg_onchip_host.py find the iteration kernels by their length-prefixed mangled names: no new
    symbol may contain one, and each old kernel is still exactly one symbol."""
    usage = cg_usage()
    for k in OLD_KERNELS:
        tag = f"{len(k)}{k}"
        assert len([s for s in usage if tag in s]) == 1, (k, [s for s in usage if tag in s])


def test_help_names_cg_stream():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--cg-stream" in r.stdout and "--cg-batch" in r.stdout


def test_cg_stream_refusals(tmp_path):
    """Exit 2 with a message, before the input file is read or a device touched (there is no input.txt here, and no GPU)."""
    for args, word in ((["input.txt", "--cg-stream", "8"], "--solver cg"),
                       (["input.txt", "--solver", "cg", "--cg-stream", "-1"], "--cg-stream"),
                       (["input.txt", "--cg-stream", "-1", "--solver", "cg"], "--cg-stream"),
                       (["input.txt", "--solver", "cg", "--cg-stream", "many"], "--cg-stream"),
                       (["input.txt", "--solver", "cg", "--cg-stream", "8x"], "--cg-stream"),
                       (["input.txt", "--solver", "cg", "--cg-stream", "8", "--cg-batch", "8"], "exclude"),
                       (["input.txt", "--solver", "cg", "--cg-batch", "8", "--cg-stream", "8"], "exclude")):
        r = subprocess.run([EXE] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert word in r.stderr and not r.stdout, (args, r.stderr, r.stdout)
    assert not os.listdir(tmp_path)
