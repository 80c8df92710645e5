"""Host-side checks of the native 3-phase assembly (no GPU): the two new entry points are exported and wrapped, the driver
knows --fill and gives its refusals, the new kernels keep to their resource budget on the ISA hipcc emits for gfx950, and the
figures of the sweep and residual kernels pinned by test_kernel_resources.py are what they were before the fill was added
(tests/golden/kernel_usage_before_fill.json: the compiler's remarks for those kernels in the parent commit's build)."""
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_kernel_resources import SWEEP_UNITS, remarks_of

EXE = os.path.join(ROOT, "effectivediffusivityfvm_amd", "deff2d")


@pytest.fixture(scope="module")
def built():
    pkg_dir = os.path.join(ROOT, "effectivediffusivityfvm_amd")
    if not (os.path.exists(os.path.join(pkg_dir, "libdeff_amd.so")) and os.path.exists(EXE)):
        subprocess.run(["make", "-s", "-C", os.path.join(pkg_dir, "csrc")], check=True)
    return EXE


def usage_of(units):
    import re
    out, cur = {}, None
    for line in "\n".join(remarks_of(u) for u in units).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def test_exports_and_wrappers(built):
    from effectivediffusivityfvm_amd import _capi
    import effectivediffusivityfvm_amd as pkg
    L = _capi.load()
    for name in ("deff_assemble_3phase_native", "deff_get_grid"):
        assert name in _capi.SYMBOLS and hasattr(L, name)
    assert callable(pkg.Solver.assemble_3phase_native) and callable(pkg.Solver.grid)
    assert L.deff_assemble_3phase_native(None, 0.0, 1.0, 10.0, 0.0, 1.0) == -1       # EINVAL before any HIP call
    assert L.deff_get_grid(None, None, None) == -1
    header = open(os.path.join(ROOT, "include", "deff_amd.h")).read()
    for key in ("fill_impl", "fill_tile_rows", "fill_launches", "fill_runs", "fill_fallbacks", "native3_rows"):
        assert f'"{key}"' in header, key


def _write_input(path, **kv):
    open(path, "w").write("\n".join(["Input File:"] + [f"{k}: {v}" for k, v in kv.items()]) + "\n")


def test_driver_knows_fill_and_refuses_what_it_cannot_do(built, tmp_path):
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--fill host|device" in r.stdout and "deff_assemble_3phase_native" in r.stdout
    r = subprocess.run([EXE, "--fill", "gpu"], capture_output=True, text=True)
    assert r.returncode == 2 and "--fill host|device" in r.stderr
    _write_input(tmp_path / "two.txt", Phases=2, InputName="nothere.jpg", RunBatch=0)
    r = subprocess.run([EXE, str(tmp_path / "two.txt"), "--fill", "device"], capture_output=True, text=True)
    assert r.returncode == 2 and "--fill device applies to 3 phases" in r.stderr
    r = subprocess.run([EXE, str(tmp_path / "two.txt"), "--fill", "host"], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot open" in r.stderr                            # the default, spelled out: goes on to the image
    _write_input(tmp_path / "three.txt", Phases=3, InputName="nothere.jpg", RunBatch=0)
    r = subprocess.run([EXE, str(tmp_path / "three.txt"), "--fill", "device", "--devices", "0,1"], capture_output=True, text=True)
    assert r.returncode == 2 and "row slabs" in r.stderr
    r = subprocess.run([EXE, str(tmp_path / "three.txt"), "--fill", "device", "--devices", "0,1", "--solver", "cg", "--cg-slabs"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "row slabs" in r.stderr and "--cg-slabs" in r.stderr


def test_fill_kernels_are_within_their_budget():
    """No scratch, at most the compute unit's 160 KiB of LDS; the one-workgroup form for small images leaves room for several
    images per compute unit; the streaming kernels around the fill stay at full occupancy."""
    u = usage_of(("api_fill",))
    fill = {k: v for k, v in u.items() if any(n in k for n in ("k_fill_", "k_phase_codes3", "k_wall_D_3phase"))}
    names = " ".join(fill)
    for want in ("k_fill_imageILi1024ELi256E", "k_fill_imageILi8192ELi1024E", "k_fill_tilesILi8192ELi1024E", "k_fill_open", "k_fill_path",
                 "k_fill_grid", "k_phase_codes3", "k_wall_D_3phase"):
        assert want in names, want
    for name, v in fill.items():
        assert v["ScratchSize"] == 0 and v["LDS"] <= 163840 and v["AGPRs"] == 0, (name, v)
        if "k_fill_imageILi1024E" in name:
            assert v["LDS"] <= 17 * 1024 and v["Occupancy"] >= 8, (name, v)
        elif "k_fill_image" in name or "k_fill_tiles" in name:
            assert 128 * 1024 <= v["LDS"] and v["Occupancy"] >= 4, (name, v)             # 1024 threads = 4 waves per SIMD
        else:
            assert v["LDS"] <= 512 and v["Occupancy"] >= 8, (name, v)


def test_existing_kernels_keep_their_figures():
    before = json.load(open(os.path.join(GOLDEN, "kernel_usage_before_fill.json")))
    now = usage_of(SWEEP_UNITS + ("api_residual",))
    assert len(before) > 200
    for name, v in before.items():
        assert now.get(name) == v, (name, now.get(name), v)
