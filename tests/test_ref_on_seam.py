"""The reference's own program on the seam, executed (VERDICT's first open item).

oracle/_ref/ref_on_seam is Deff2D.cu / Deff2D.cuh with section A's patch applied by oracle/Makefile -- main, readInputFile, the
four drivers, FloodFill, the CSV and CMAP writers are the reference's text, unchanged; structs, kernels, assemblies,
initializeGPU / unInitializeGPU and the two Jacobi loops are reference_seam.hpp on libdeff_amd.so.  tests/test_integration_patch.py
only LINKS that program; here it RUNS, in all four modes, next to deff2d on the same directory contents:

  * the reference's real call order goes through the seam: initializeGPU, DiscretizeMatrix2D[_ImpSolid] on the thread's scratch
    context (re-created when the image size changes inside a batch), JacobiGPU[PreCond] with deff_set_system per stage, warm
    starts, deff /= DCF, unInitializeGPU per image;
  * every column of the CSV files but Time, the CMAP files and the verbose stage lines of the two programs are equal as text;
  * both are pinned to the record and to the CPU oracle, printed with the reference's own format strings (cuh:182-230).

The reference's program is the authority for file names, column order and number formats, the oracle for the numbers.  No
tolerance appears: everything compared is text or bit-equal doubles.  Time (device milliseconds of different loops in the two
programs) is only required to parse as a finite number >= 0; tests/test_gpu_timing.py owns it.

Without a GPU the program must still end by itself: the reference waits on getchar() after a failed initializeGPU (cuh:914),
the seam must not, and whatever a driver does after a failed call must not crash in the seam.
"""
import glob
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from conftest import GOLDEN, ROOT
from test_integration_patch import DELETED, REF

LIBDIR = os.path.join(ROOT, "effectivediffusivityfvm_amd")
EXE = os.path.join(LIBDIR, "deff2d")
SEAM_ENTRY_POINTS = ("deff_create", "deff_destroy", "deff_assemble_from_D", "deff_get_system", "deff_set_system", "deff_set_field",
                     "deff_solve", "deff_get_field")          # what test_section_A_patch_compiles_and_links lists


def _write_input(path, **kv):
    lines = ["Input File:"] + [f"{k}: {v}" for k, v in kv.items()]
    open(path, "w").write("\n".join(lines) + "\n")


# ------------------------------------------------------------------ CPU: the recipe and the program without a GPU ----------

def test_makefile_cut_ranges_are_the_link_tests_ranges():
    """oracle/Makefile states the deleted ranges once (SEAM_CUT); the test that only links applies its own list: the binary
    that runs and the test that links must not drift apart."""
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    m = re.findall(r"^SEAM_CUT\s*:?=\s*(.+)$", text, flags=re.M)
    assert len(m) == 1, "SEAM_CUT must be defined exactly once"
    cut = [tuple(int(v) for v in r.split("-")) for r in m[0].split()]
    assert cut == DELETED
    assert text.count("$(SEAM_CUT)") == 1 and "_ref/ref_on_seam" in re.search(r"^ref:(.*)$", text, flags=re.M).group(1)


@pytest.fixture(scope="module")
def binary():
    """The program as the committed recipe builds it: made here where the reference is mounted and the library is built
    (a no-op when build() already did), taken as it travelled otherwise."""
    if os.path.exists(os.path.join(REF, "Deff2D.cuh")) and os.path.exists(os.path.join(LIBDIR, "libdeff_amd.so")):
        r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/ref_on_seam"], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert ob.have_ref_on_seam()
    elif not ob.have_ref_on_seam():
        pytest.skip("oracle/_ref/ref_on_seam absent and the reference is not mounted (or libdeff_amd.so is not built)")
    return ob.REF_ON_SEAM


def test_ref_on_seam_is_built_and_calls_the_seam(binary):
    syms = subprocess.run(["nm", "-u", binary], capture_output=True, text=True).stdout
    for name in SEAM_ENTRY_POINTS:
        assert f" U {name}" in syms, name
    assert "cuda" not in syms.lower()
    # it finds the library relative to itself, wherever the tree lies
    dyn = subprocess.run(["readelf", "-d", binary], capture_output=True, text=True).stdout
    assert "$ORIGIN/../../effectivediffusivityfvm_amd" in dyn


def test_missing_library_is_reported_by_the_recipe(tmp_path):
    """`make _ref/ref_on_seam` without libdeff_amd.so fails with a message that says so (dry tree: only the recipe is copied)."""
    if not os.path.exists(os.path.join(REF, "Deff2D.cuh")):
        pytest.skip("reference not mounted")
    os.makedirs(tmp_path / "oracle")
    os.makedirs(tmp_path / "effectivediffusivityfvm_amd" / "csrc")
    os.makedirs(tmp_path / "include")
    shutil.copy(os.path.join(ROOT, "oracle", "Makefile"), tmp_path / "oracle" / "Makefile")
    shutil.copy(os.path.join(LIBDIR, "csrc", "reference_seam.hpp"), tmp_path / "effectivediffusivityfvm_amd" / "csrc")
    shutil.copy(os.path.join(ROOT, "include", "deff_amd.h"), tmp_path / "include")
    r = subprocess.run(["make", "-C", str(tmp_path / "oracle"), "_ref/ref_on_seam"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "libdeff_amd.so is missing" in r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "oracle" / "_ref" / "ref_on_seam")


@pytest.mark.parametrize("run_batch", [1, 0])
def test_without_a_gpu_the_program_ends_by_itself(binary, tmp_path, run_batch):
    """No GPU: initializeGPU fails.  The reference's own initializeGPU would now sit in getchar() (cuh:914); the seam reports
    the failed call on stderr and returns 0, the driver prints its message and returns (cuh:1750-1755, :1975-1980) -- no
    signal, no wait, and no CSV row with a solved value."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present: the gpu-marked tests run the program there")
    shutil.copy(os.path.join(GOLDEN, "00000.jpg"), tmp_path / "00000.jpg")
    _write_input(tmp_path / "input.txt", Phases=2, Ds="1e-3", Df=100, Dg=1, MeshAmpX=1, MeshAmpY=1, InputName="00000.jpg", CR=1, CL=0,
                 OutputName="out.csv", printCMap=0, CMapName="CMAP.csv", Convergence="1e-6", MaxIter="2e4", Verbose=1,
                 RunBatch=run_batch, NumImages=1)
    r = ob.run_ref_on_seam(tmp_path, timeout=120)               # TimeoutExpired = it waited: a failure
    assert r.returncode >= 0, (r.returncode, r.stderr[-2000:])  # no signal
    assert "initializeGPU: " in r.stderr, r.stderr[-2000:]      # the seam's report names the failed call
    assert "Error when allocating space in GPU" in r.stdout
    if os.path.exists(tmp_path / "out.csv"):
        rows = open(tmp_path / "out.csv").read().splitlines()
        assert all(row.startswith("imgNum,") for row in rows), rows


# ------------------------------------------------------------------ GPU: the two programs side by side ---------------------

needs_binary = pytest.mark.skipif(not ob.have_ref_on_seam(), reason="oracle/_ref/ref_on_seam not built (the reference was not mounted at build time)")

COMMON = dict(MeshAmpX=1, MeshAmpY=1, CR=1, CL=0, OutputName="out.csv", CMapName="CMAP.csv")
MODES = {
    # name: (input.txt, timeout in s)
    "batch2": (dict(Phases=2, Ds="1e-3", Df=1, Dg=1, InputName="00000.jpg", printCMap=0, Convergence="1e-6", MaxIter="5e5", Verbose=1,
                    RunBatch=1, NumImages=3), 300),
    "single2": (dict(Phases=2, Ds="1e-3", Df="1e4", Dg=1, InputName="00000.jpg", printCMap=1, Convergence="1e-6", MaxIter="3e5",
                     Verbose=1, RunBatch=0, NumImages=1), 300),
    "single3": (dict(Phases=3, Ds=0, Df=1, Dg=1237500, InputName="00000.jpg", printCMap=1, Convergence="1e-5", MaxIter="5e5", Verbose=1,
                     RunBatch=0, NumImages=1), 600),
    "batch3": (dict(Phases=3, Ds=0, Df=1, Dg=1237500, InputName="00000.jpg", printCMap=1, Convergence="1e-5", MaxIter="5e5", Verbose=1,
                    RunBatch=1, NumImages=2), 600),
}


def _blobs(rng, W, H, cell, levels, cuts):
    """Thresholded random blobs: a coarse random field blown up by `cell`, cut at `cuts` into the grey `levels`."""
    coarse = rng.random(((H + cell - 1) // cell, (W + cell - 1) // cell))
    f = np.kron(coarse, np.ones((cell, cell)))[:H, :W]
    return np.asarray(levels, dtype=np.uint8)[np.searchsorted(np.asarray(cuts), f)]


def _fill_directory(mode, d):
    """The directory contents of a mode (the same bytes for both programs): 00000.jpg of the reference, and the written images
    -- another size than 128 x 128 (the seam's scratch context is re-created between the images of a batch), one odd width."""
    from PIL import Image
    shutil.copy(os.path.join(GOLDEN, "00000.jpg"), os.path.join(d, "00000.jpg"))
    if mode == "batch2":
        rng = np.random.default_rng(20240)
        Image.fromarray(_blobs(rng, 96, 64, 8, [0, 255], [0.45])).save(os.path.join(d, "00001.jpg"), quality=95)
        Image.fromarray(_blobs(rng, 97, 41, 6, [0, 255], [0.5])).save(os.path.join(d, "00002.jpg"), quality=95)
    if mode == "batch3":
        rng = np.random.default_rng(20241)
        Image.fromarray(_blobs(rng, 72, 56, 8, [0, 150, 255], [0.3, 0.65])).save(os.path.join(d, "00001.jpg"), quality=100)
    cfg = dict(COMMON)
    cfg.update(MODES[mode][0])
    _write_input(os.path.join(d, "input.txt"), **cfg)


class Run:
    def __init__(self, d, returncode, stdout, stderr):
        self.dir, self.returncode, self.stdout, self.stderr = d, returncode, stdout, stderr

    def csv(self):
        return open(os.path.join(self.dir, "out.csv")).read().splitlines()

    def cmaps(self):
        return sorted(os.path.basename(p) for p in glob.glob(os.path.join(self.dir, "CMAP*.csv")))

    def lines(self, prefix):
        return [ln for ln in self.stdout.splitlines() if ln.startswith(prefix)]


class Runner:
    """Each mode runs once per program, each in a fresh directory (the reference opens its CSV with a+), each process under
    its own timeout.  After a run that ended by signal or timeout nothing more is started: later requests fail from the
    recorded status.  Nothing is retried."""

    def __init__(self, base):
        self.base, self.done, self.dead = base, {}, None

    def _one(self, mode, who):
        d = self.base / f"{mode}_{who}"
        os.makedirs(d)
        _fill_directory(mode, d)
        timeout = MODES[mode][1]
        try:
            if who == "ref":
                r = ob.run_ref_on_seam(d, timeout)
            else:
                r = subprocess.run([EXE], cwd=d, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            self.dead = f"{who} in mode {mode} did not end within {timeout} s (killed)"
            pytest.fail(self.dead)
        if r.returncode < 0:
            self.dead = f"{who} in mode {mode} ended by signal {-r.returncode}: {r.stderr[-1500:]}"
            pytest.fail(self.dead)
        return Run(str(d), r.returncode, r.stdout, r.stderr)

    def get(self, mode):
        if mode not in self.done:
            if self.dead:
                pytest.fail(f"not started: an earlier GPU process died ({self.dead})")
            ref = self._one(mode, "ref")
            ours = self._one(mode, "ours")
            self.done[mode] = (ref, ours)
        ref, ours = self.done[mode]
        assert ref.returncode == 0, (ref.returncode, ref.stderr[-2000:])
        for call in ("initializeGPU", "DiscretizeMatrix2D", "JacobiGPU"):                      # the seam reported nothing
            assert call not in ref.stderr, ref.stderr[-2000:]
        assert ours.returncode == 0, ours.stderr[-2000:]
        return ref, ours


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    assert os.access(EXE, os.X_OK), "deff2d is not built"
    return Runner(tmp_path_factory.mktemp("ref_on_seam"))


def _time_column(header):
    return header.split(",").index("Time")


def _assert_same_outputs(ref, ours, want_cmaps):
    """CSV: header and every row equal field by field as text, except Time (finite, >= 0 in both).  CMAP files: same names,
    same bytes.  Verbose: the same sequences of `Iterations taken = N` and `Pre-Cond Stage k: DCG = ...` lines."""
    a, b = ref.csv(), ours.csv()
    assert a[0] == b[0] and len(a) == len(b) and len(a) >= 2
    t = _time_column(a[0])
    for ra, rb in zip(a[1:], b[1:]):
        fa, fb = ra.split(","), rb.split(",")
        assert len(fa) == len(fb) == len(a[0].split(","))
        for who, f in (("ref", fa), ("ours", fb)):
            v = float(f[t])
            assert math.isfinite(v) and v >= 0, (who, f[t])
        assert fa[:t] + fa[t + 1:] == fb[:t] + fb[t + 1:], (ra, rb)
    assert ref.cmaps() == ours.cmaps() == want_cmaps
    for name in want_cmaps:
        assert open(os.path.join(ref.dir, name), "rb").read() == open(os.path.join(ours.dir, name), "rb").read(), name
    for prefix in ("Iterations taken = ", "Pre-Cond Stage "):
        assert ref.lines(prefix) == ours.lines(prefix), prefix


def _without_time(row, header):
    f = row.split(",")
    t = _time_column(header)
    return f[:t] + f[t + 1:]


def _iterations(run):
    return [int(ln.split("=")[1]) for ln in run.lines("Iterations taken = ")]


@needs_binary
@pytest.mark.gpu
def test_batch_sim_three_images_of_three_sizes(runner, recorded, oracle, img00000):
    """BatchSim (cuh:1843-2054): 00000.jpg, then 96 x 64 and 97 x 41 written by the test."""
    import effectivediffusivityfvm_amd as pkg
    ref, ours = runner.get("batch2")
    _assert_same_outputs(ref, ours, [])                            # BatchSim writes no concentration map
    rows = ref.csv()
    assert rows[0] == "imgNum,porosity,PathFlag,Deff,Time,nElements,converge,ds,df" and len(rows) == 4
    # image 0: the record
    rec = recorded["img00000_2phase_batch"]
    assert _iterations(ref)[0] == rec["iters"] == 110001
    f0 = rows[1].split(",")
    assert f0[0] == "0" and f0[1] == "0.346069" and f0[3] == "0.182862" and f0[5] == "16384"
    # every image: the oracle's one-image result, printed as outputBatch prints it (cuh:212)
    pixs = [img00000] + [pkg.load_jpeg_gray(os.path.join(ref.dir, f"{k:05d}.jpg")) for k in (1, 2)]
    assert [p.shape for p in pixs] == [(128, 128), (64, 96), (41, 97)]
    for k, pix in enumerate(pixs):
        H, W = pix.shape
        D = oracle.fill_D_2phase(pix, 1.0, 1e-3)
        A, b = oracle.discretize(D, 0.0, 1.0)
        it, deff, conv, _, _, _ = oracle.jacobi(A, b, oracle.linear_guess(W, H, 0.0, 1.0), D, 0.0, 1.0, 1e-6, 500000)
        path = int(oracle.floodfill((pix > 150).astype(np.uint32))[1])
        want = "%d,%f,%d,%f,%f,%d,%f,%f,%f" % (k, oracle.porosity(pix), path, deff / 1.0, 0.0, W * H, conv, 1e-3, 1.0)
        for run in (ref, ours):
            assert _without_time(run.csv()[1 + k], rows[0]) == _without_time(want, rows[0]), (k, run.dir)
            assert _iterations(run)[k] == it, (k, run.dir)


@needs_binary
@pytest.mark.gpu
def test_single_sim_ramp_with_warm_start(runner, oracle, img00000):
    """SingleSim (cuh:1635-1841), Df = 1e4: two ramp stages (DCF = 100, 1e4), the second warm-started from the first through
    x_vec in/out of JacobiGPU."""
    ref, ours = runner.get("single2")
    _assert_same_outputs(ref, ours, ["CMAP.csv"])
    want = oracle.solve_single_2phase_ramp(img00000, 1e-3, 1e4, 0.0, 1.0, 1e-6, 300000)
    assert [st[0] for st in want["stages"]] == [100.0, 1e4]
    dcf, it, deff, conv = want["stages"][-1]
    path = int(oracle.floodfill((img00000 > 150).astype(np.uint32))[1])
    row = "%s,%f,%d,%f,%f,%d,%f,%f,%f" % ("00000.jpg", oracle.porosity(img00000), path, deff, 0.0, 128 * 128, conv, 1e-3, 1e4)   # cuh:184
    header = "imgNum,porosity,PathFlag,Deff,Time,nElements,converge,ds,df"
    for run in (ref, ours):
        assert _iterations(run) == [st[1] for st in want["stages"]], run.dir
        rows = run.csv()
        assert rows[0] == header and len(rows) == 2
        assert _without_time(rows[1], header) == _without_time(row, header), run.dir
    # the map is createCMAP's (cuh:516-520) of the oracle's final field
    cmap = open(os.path.join(ref.dir, "CMAP.csv")).read().splitlines()
    x = want["field"]
    assert cmap[0] == "X,Y,C" and len(cmap) == 1 + 128 * 128
    assert cmap[1:] == ["%d,%d,%1.3e" % (j, i, x[i, j]) for i in range(128) for j in range(128)]


@needs_binary
@pytest.mark.gpu
def test_single_sim_3phase_as_shipped(runner, recorded):
    """SingleSim3Phase (cuh:1316-1633) with the shipped options on 00000.jpg: six JacobiGPUPreCond stages and the final solve."""
    ref, ours = runner.get("single3")
    _assert_same_outputs(ref, ours, ["CMAP.csv"])
    rec = recorded["img00000_3phase_as_shipped"]
    assert rec["stage_sweeps"] == [80001, 10001, 10001, 10001, 10001, 10001, 10001]
    for run in (ref, ours):
        assert _iterations(run) == rec["stage_sweeps"], run.dir
        assert [ln.split(":")[0] for ln in run.lines("Pre-Cond Stage ")] == [f"Pre-Cond Stage {k}" for k in range(1, 7)]
        rows = run.csv()
        assert rows[0] == "imgNum,SVF,LVF,PathFlag,Deff,Time,nElements,converge,ds,df,dg" and len(rows) == 2
        assert rows[1].startswith("00000.jpg,0.653931,0.000000,1,2.247e+05,"), rows[1]
        f = rows[1].split(",")
        assert f[4] == "%1.3e" % rec["deff"] and f[7] == "%1.3e" % rec["conv"] and f[6] == "16384"
        assert f[8:] == ["%1.3e" % 0.0, "%1.3e" % 1.0, "%1.3e" % 1237500.0]


@needs_binary
@pytest.mark.gpu
def test_batch_sim_3phase_two_sizes(runner, recorded, oracle, img00000):
    """BatchSim3Phase (cuh:2056-2419): 00000.jpg and a written 72 x 56 image of three grey levels; CMAP_%05d.csv per image."""
    import effectivediffusivityfvm_amd as pkg
    ref, ours = runner.get("batch3")
    _assert_same_outputs(ref, ours, ["CMAP_00000.csv", "CMAP_00001.csv"])
    header = "imgNum,SVF,LVF,PathFlag,Deff,Time,nElements,converge,ds,df,dg"
    pixs = [img00000, pkg.load_jpeg_gray(os.path.join(ref.dir, "00001.jpg"))]
    assert pixs[1].shape == (56, 72) and len(np.unique(pixs[1])) >= 3
    stages, fields = [], []
    for k, pix in enumerate(pixs):
        with np.errstate(all="ignore"):
            want = oracle.solve_3phase(pix, 0.0, 1.0, 1237500.0, 0.0, 1.0, 1e-5, 500000)
        stages += want["stage_sweeps"]
        fields.append(want["field"])
        row = "%d,%f,%f,%d,%1.5e,%f,%d,%1.5e,%1.5e,%1.5e,%1.5e" % (k, want["SVF"], want["LVF"], int(want["path"]), want["deff"], 0.0,
                                                                  pix.size, want["conv"], 0.0, 1.0, 1237500.0)   # cuh:227
        for run in (ref, ours):
            rows = run.csv()
            assert rows[0] == header and len(rows) == 3
            assert _without_time(rows[1 + k], header) == _without_time(row, header), (k, run.dir)
    assert stages[:7] == recorded["img00000_3phase_as_shipped"]["stage_sweeps"]
    for run in (ref, ours):
        assert _iterations(run) == stages, run.dir                 # image after image, stage after stage
        assert len(run.lines("Pre-Cond Stage ")) == 12
    for k, x in enumerate(fields):                                 # createCMAPBatch (cuh:546-550) of the oracle's field
        H, W = x.shape
        cmap = open(os.path.join(ref.dir, f"CMAP_{k:05d}.csv")).read().splitlines()
        assert cmap[0] == "X,Y,C" and cmap[1:] == ["%d,%d,%1.3e" % (j, i, x[i, j]) for i in range(H) for j in range(W)]
