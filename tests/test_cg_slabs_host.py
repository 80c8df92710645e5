"""Conjugate gradients over row slabs (deff_slab_group_solve_cg, deff_slab_rank_solve_cg), host side: the library's exports
and argument checks, the slab kernels' register / LDS budget on the ISA hipcc emits for gfx950 (the bars of
test_cg_host.py::test_cg_kernels_resources), and the driver's usage errors around --cg-slabs.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc")
EXE = os.path.join(ROOT, "effectivediffusivityfvm_amd", "deff2d")


def test_library_exports_slab_solve_cg():
    from effectivediffusivityfvm_amd import _capi
    lib = os.path.join(ROOT, "effectivediffusivityfvm_amd", "libdeff_amd.so")
    assert os.path.exists(lib), "libdeff_amd.so is not built"
    L = C.CDLL(lib)
    out = (C.c_byte * 64)()
    for name in ("deff_slab_group_solve_cg", "deff_slab_rank_solve_cg"):
        assert hasattr(L, name) and name in _capi.SYMBOLS
        fn = getattr(L, name)
        # NULL arguments: refused before any device work
        assert fn(None, C.c_double(1e-10), C.c_int64(10), C.c_int64(1), out, None, None) == -1
        assert fn(C.c_void_p(1), C.c_double(1e-10), C.c_int64(10), C.c_int64(1), None, None, None) == -1
        # ... and so are the numbers, before the handle is looked at
        assert fn(C.c_void_p(1), C.c_double(-1.0), C.c_int64(10), C.c_int64(1), out, None, None) == -1
        assert fn(C.c_void_p(1), C.c_double(1e-10), C.c_int64(-1), C.c_int64(1), out, None, None) == -1
        assert fn(C.c_void_p(1), C.c_double(1e-10), C.c_int64(10), C.c_int64(0), out, None, None) == -1


def test_slab_cg_kernels_resources():
    """The slab forms spill nothing and keep the existing kernels' bars: k_slcg_dir / _update / _resid / _admissible <= 96
    VGPRs, no AGPR, 28.4 KiB of LDS, 5 waves per SIMD; the one-workgroup reductions <= 32 VGPRs."""
    path = os.path.join(CSRC, "build", "api_cg.usage.txt")
    assert os.path.exists(path), "build/api_cg.usage.txt missing: api_cg.hip is not part of the build"
    usage, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    streaming = ("k_slcg_dir", "k_slcg_update", "k_slcg_resid", "k_slcg_admissible")
    small = ("k_slcg_sum", "k_slcg_alpha", "k_slcg_beta", "k_slcg_check", "k_slcg_verdict")
    seen = set()
    for name, u in usage.items():
        for k in streaming:
            if f"{len(k)}{k}" in name:
                seen.add(k)
                assert u["ScratchSize"] == 0 and u["VGPRs"] <= 96 and u["AGPRs"] == 0, (name, u)
                assert u["LDS"] <= 29184 and u["Occupancy"] >= 5, (name, u)
        for k in small:
            if f"{len(k)}{k}" in name:
                seen.add(k)
                assert u["ScratchSize"] == 0 and u["VGPRs"] <= 32, (name, u)
    assert seen == set(streaming) | set(small)


def test_deff2d_cg_slabs_usage_errors(tmp_path):
    from test_frontend import _write_input
    assert os.path.exists(EXE), "deff2d is not built"
    _write_input(tmp_path / "single.txt", Phases=2, Ds="1e-3", Df=1, MeshAmpX=1, MeshAmpY=1, CR=1, CL=0,
                 InputName="00000.jpg", OutputName="single.csv", printCMap=0, Convergence="1e-6", MaxIter="5e5", Verbose=0,
                 RunBatch=0, NumImages=1)
    _write_input(tmp_path / "batch.txt", Phases=2, Ds="1e-3", Df=1, MeshAmpX=1, MeshAmpY=1, CR=1, CL=0,
                 OutputName="out.csv", printCMap=0, Convergence="1e-6", MaxIter="5e5", Verbose=0, RunBatch=1, NumImages=1)

    def run(*args):
        return subprocess.run([EXE, *args], cwd=tmp_path, capture_output=True, text=True, timeout=60)

    r = run("single.txt", "--devices", "0,0", "--cg-slabs")                      # without --solver cg
    assert r.returncode == 2 and "--cg-slabs needs --solver cg" in r.stderr, r.stderr
    r = run("single.txt", "--solver", "cg", "--cg-slabs")                        # no slab run: one device
    assert r.returncode == 2 and "row-slab run" in r.stderr, r.stderr
    r = run("batch.txt", "--solver", "cg", "--devices", "0,0", "--cg-slabs")     # no slab run: batch mode
    assert r.returncode == 2 and "row-slab run" in r.stderr, r.stderr
    r = run("single.txt", "--solver", "cg", "--devices", "0,0")                  # the default keeps refusing, and names the flag
    assert r.returncode == 2 and "row slabs" in r.stderr and "--cg-slabs" in r.stderr, r.stderr
    assert "--cg-slabs" in run("--help").stdout
