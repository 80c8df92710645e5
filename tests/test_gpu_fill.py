"""The native 3-phase assembly on the GPU (deff_assemble_3phase_native): the flood fill on the device against the host fill
(deff_flood_fill, and the reference's own FloodFill where oracle/_ref is built), the system it assembles against the explicit
path (deff_assemble_3phase with the host-filled Grid) bit for bit through every consumer, the continuation stages, the
refusals and the driver's --fill device.  Every fill test asserts from deff_get_plan which form ran and that no image went to
the host fill, except the one test that is about that fallback."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "effectivediffusivityfvm_amd", "deff2d")
WORDS_ONE_WORKGROUP = 8192          # csrc/kernels_fill.hpp: FILL_LARGE_WORDS


def pkg():
    import torch  # noqa: F401  (first, so one HIP runtime serves torch and libdeff_amd)
    import effectivediffusivityfvm_amd as p
    return p


def three_levels(rng, H, W, solid, gas=0.25):
    """pixels 255 (solid, > 200), 20 (gas, < 50), 150 (fluid)"""
    f = rng.random((H, W))
    return np.where(f < solid, 255, np.where(f < solid + gas, 20, 150)).astype(np.uint8)


def host_fill(pix, nimg=1, ampX=1, ampY=1):
    """deff_flood_fill of every image of a stack on `pixel > 200` at mesh resolution: (grid[nimg*ny, nx], path[nimg])"""
    P = pkg()
    mesh = np.repeat(np.repeat(pix, ampY, axis=0), ampX, axis=1)
    ny = mesh.shape[0] // nimg
    grids, paths = [], []
    for k in range(nimg):
        g, p = P.flood_fill((mesh[k * ny:(k + 1) * ny] > 200).astype(np.uint32))
        grids.append(g)
        paths.append(p)
    return np.concatenate(grids), np.array(paths, dtype=bool)


def planner_form(nx, ny):
    return 1 if ny * ((nx + 63) // 64) <= WORDS_ONE_WORKGROUP else 2


def device_fill(pix, nimg=1, ampX=1, ampY=1, impl=0, tile_rows=0, fallbacks=0):
    """Solver.grid() after a native assembly; asserts the form that ran and the fallback count"""
    P = pkg()
    H, W = pix.shape[0] // nimg, pix.shape[1]
    nx, ny = W * ampX, H * ampY
    with P.Solver(nx, ny, nimg=nimg) as s:
        s.set_tuning("fill_impl", impl)
        s.set_tuning("fill_tile_rows", tile_rows)
        s.set_image(pix, ampX, ampY)
        s.assemble_3phase_native(1e-3, 1.0, 10.0, 0.0, 1.0)
        want_impl = impl if impl else planner_form(nx, ny)
        assert s.plan_value("fill_impl") == want_impl, (s.plan_value("fill_impl"), want_impl)
        assert s.plan_value("fill_runs") == 1 and s.plan_value("native3_rows") == 452
        assert s.plan_value("fill_launches") >= (1 if want_impl == 1 else 3)
        if fallbacks is not None:
            assert s.plan_value("fill_fallbacks") == fallbacks, s.plan_value("fill_fallbacks")
        g, p = s.grid()
        print(f"{nx} x {ny} x {nimg}: form {want_impl}, tile rows {tile_rows}, launches {s.plan_value('fill_launches')}, "
              f"rounds {s.plan_value('fill_rounds')}, fallbacks {s.plan_value('fill_fallbacks')}")
        return g, p


def check_fill(pix, nimg=1, ampX=1, ampY=1, forms=((0, 0), (2, 8), (2, 5)), ref=False):
    want_g, want_p = host_fill(pix, nimg, ampX, ampY)
    if ref and ob.have_ref_host() and nimg == 1:
        mesh = np.repeat(np.repeat(pix, ampY, axis=0), ampX, axis=1)
        assert np.array_equal(ob.ref_floodfill((mesh > 200).astype(np.uint32)), want_g)
    for impl, tr in forms:
        g, p = device_fill(pix, nimg, ampX, ampY, impl, tr)
        assert np.array_equal(g, want_g), (impl, tr, int((g != want_g).sum()))
        assert np.array_equal(p, want_p), (impl, tr, p, want_p)


SHAPES = [(2, 2), (3, 5), (64, 2), (65, 3), (127, 9), (128, 128), (130, 71), (258, 9), (2, 300), (1030, 517)]


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_fill_equals_host_fill(nx, ny):
    """Random three-level images, the top-left cell open and solid (the quirk): the planner's form, row tiles of 8 rows and
    of 5 (a ragged last tile at most heights; 130 x 71: seams, halo rows and the wrap between the first and the last tile)."""
    rng = np.random.default_rng(nx * 1000 + ny)
    for k, solid in enumerate((0.3, 0.42)):
        pix = three_levels(rng, ny, nx, solid)
        pix[0, 0] = 255 if k else 150
        check_fill(pix, ref=(nx, ny) in ((3, 5), (65, 3), (130, 71), (128, 128)))


def designed_masks(nx, ny):
    out = {}
    a = np.full((ny, nx), 255, np.uint8)                  # serpentine by rows: one seed, a path of about ny nx / 2 cells
    a[0, 0] = 150
    a[0::2, 1:] = 150
    for i in range(1, ny, 2):
        a[i, 1 if (i // 2) & 1 else nx - 1] = 20
    out["serpentine"] = a
    a = np.full((ny, nx), 255, np.uint8)                  # a pore reachable only through the wrap between rows 0 and ny - 1
    a[ny - 1, :] = 150
    a[0, nx - 1] = 20
    a[1, nx - 1] = 150
    a[0, 0] = 150
    a[0, 1] = 255
    out["wrap_only"] = a
    a = np.full((ny, nx), 150, np.uint8)                  # solid left column but for the top-left cell, which is walled in
    a[1:, 0] = 255
    a[0, 1] = 255
    out["solid_left"] = a                                 # every other pore is 2, PathFlag 0
    out["all_open"] = np.full((ny, nx), 150, np.uint8)
    out["all_solid"] = np.full((ny, nx), 255, np.uint8)
    a = np.full((ny, nx), 255, np.uint8)                  # the quirk (top-left solid) with solid cells in the last column
    a[0::2, 1:nx - 1] = 150
    a[1::3, nx - 1] = 20
    out["quirk_last_column"] = a
    return out


@pytest.mark.parametrize("nx,ny", [(130, 71), (65, 3), (258, 9)])
def test_fill_designed_masks(nx, ny):
    masks = designed_masks(nx, ny)
    g, p = host_fill(masks["solid_left"])
    assert not p[0] and g[0, 0] == 0 and (g[g != 1][1:] == 2).all()
    g, p = host_fill(masks["wrap_only"])
    assert g[0, nx - 1] == 0 and g[1, nx - 1] == 0 and p[0]
    for name, pix in masks.items():
        check_fill(pix, ref=name in ("wrap_only", "quirk_last_column"))


def test_fill_amplified_and_odd_widths():
    rng = np.random.default_rng(5)
    check_fill(three_levels(rng, 9, 21, 0.35), ampX=2, ampY=3)          # 42 x 27 cells
    check_fill(three_levels(rng, 24, 43, 0.4), ampX=3, ampY=2)          # 129 x 48 cells: odd width, the pad column
    check_fill(three_levels(rng, 40, 131, 0.38))


@pytest.mark.parametrize("nimg", [3, 5])
def test_fill_stacks_do_not_leak_between_images(nimg):
    """Different images per slot; one whose only connection is the wrap between its own first and last row sits between two
    fully open images: nothing leaks across images, in either form."""
    nx, ny = 130, 24
    rng = np.random.default_rng(nimg)
    imgs = [three_levels(rng, ny, nx, 0.3 + 0.04 * k) for k in range(nimg)]
    imgs[0] = np.full((ny, nx), 150, np.uint8)
    imgs[1] = designed_masks(nx, ny)["wrap_only"]
    imgs[2] = np.full((ny, nx), 150, np.uint8)
    check_fill(np.concatenate(imgs), nimg=nimg)


def test_fill_out_of_launches_goes_to_the_host():
    """A serpentine by columns crosses every seam of one-row tiles nx / 2 times: more launches than the tiled form is given.
    The image is then filled on the host, counted, and the result is the same."""
    nx, ny = 130, 71
    a = np.full((ny, nx), 255, np.uint8)
    a[1:ny - 1, 0::2] = 150
    for j in range(1, nx, 2):
        a[1 if (j // 2) & 1 else ny - 2, j] = 150
    want_g, want_p = host_fill(a)
    g, p = device_fill(a, impl=2, tile_rows=1, fallbacks=1)
    assert np.array_equal(g, want_g) and np.array_equal(p, want_p)
    g, p = device_fill(a)                                               # one workgroup: no launches to run out of
    assert np.array_equal(g, want_g) and np.array_equal(p, want_p)


# ---------------------------------------------------------------- the system ---

def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def results_equal(ra, rb, fields):
    ra = ra if isinstance(ra, list) else [ra]
    rb = rb if isinstance(rb, list) else [rb]
    for x, y in zip(ra, rb):
        for f in fields:
            assert same(getattr(x, f), getattr(y, f)), (f, getattr(x, f), getattr(y, f))


def both(native, explicit, fn):
    """fn on both contexts: the same outcome, be it a result or a refusal"""
    P = pkg()
    out = []
    for s in (native, explicit):
        try:
            out.append(("ok", fn(s)))
        except P.DeffError as e:
            out.append(("refused", e.code))
    assert out[0][0] == out[1][0], out
    if out[0][0] == "refused":
        assert out[0][1] == out[1][1], out
        return None
    return out[0][1], out[1][1]


SYSTEM_SHAPES = [(40, 32, 1), (33, 21, 1), (130, 71, 1), (33, 20, 3)]


@pytest.mark.parametrize("nx,ny,nimg", SYSTEM_SHAPES)
@pytest.mark.parametrize("Ds", [1e-3, 0.0])
@pytest.mark.parametrize("Dg", [10.0, 1e6])
@pytest.mark.parametrize("CL,CR", [(0.0, 1.0), (2.0, -1.0)])
def test_system_equals_explicit_path(nx, ny, nimg, Ds, Dg, CL, CR):
    P = pkg()
    rng = np.random.default_rng(nx * 100 + ny)
    pix = three_levels(rng, ny * nimg, nx, 0.36)
    grid, path = host_fill(pix, nimg)
    with P.Solver(nx, ny, nimg=nimg) as a, P.Solver(nx, ny, nimg=nimg) as b, np.errstate(all="ignore"):
        for s in (a, b):
            s.set_image(pix)
        a.assemble_3phase_native(Ds, 1.0, Dg, CL, CR)
        b.assemble_3phase(Ds, 1.0, Dg, CL, CR, grid=grid)
        assert a.plan_value("native3_rows") == 452 and a.plan_value("fill_fallbacks") == 0
        g, p = a.grid()
        assert np.array_equal(g, grid) and np.array_equal(p, path)
        Aa, ba = a.get_system()
        Ab, bb = b.get_system()
        assert np.array_equal(Aa, Ab) and np.array_equal(ba, bb)
        for s in (a, b):
            s.init_linear(CL, CR)
        fa, fb = a.flux(), b.flux()
        for x, y in zip(fa, fb):
            assert same(x, y)
        for kernel in ("explicit", "scalar", "matfree", "matfree_tb"):
            for s in (a, b):
                s.set_kernel(kernel)
                s.init_linear(CL, CR)
                s.sweeps(27)
            assert same(a.get_field(), b.get_field()), kernel
        assert a.kernel_in_use() == b.kernel_in_use()
        for s in (a, b):
            s.set_kernel("auto")
            s.init_linear(CL, CR)
        ra, rb = a.solve(1e-4, 3000, check_every=100), b.solve(1e-4, 3000, check_every=100)
        results_equal(ra, rb, ("iters", "deff_raw", "conv"))
        assert same(a.get_field(), b.get_field())
        assert same(a.residual(), b.residual())
        for onchip in (0, 1):
            for s in (a, b):
                s.set_tuning("cg_onchip", onchip)
                s.init_linear(CL, CR)
            got = both(a, b, lambda s: s.solve_cg(1e-9, 400, check_every=32))
            if got is not None:
                results_equal(got[0], got[1], ("iters", "rel_residual", "deff_raw"))
                assert a.plan_value("cg_impl") == b.plan_value("cg_impl") == (2 if onchip else 1)
                assert same(a.get_field(), b.get_field())
        assert a.plan_value("fill_runs") == 1


def test_system_against_the_oracle():
    """The oracle's own chain: floodfill -> fill_D_3phase -> discretize (ImpSolid) -> 27 sweeps."""
    P = pkg()
    nx, ny = 130, 71
    pix = three_levels(np.random.default_rng(99), ny, nx, 0.36)
    grid, path = ob.floodfill((pix > 200).astype(np.uint32))
    D = ob.fill_D_3phase(pix, 1.0, 1e-3, 100.0)
    A, b = ob.discretize(D, 0.0, 1.0, grid=grid)
    want = ob.sweeps(A, b, ob.linear_guess(nx, ny, 0.0, 1.0), 27)
    with P.Solver(nx, ny) as s:
        s.set_image(pix)
        s.assemble_3phase_native(1e-3, 1.0, 100.0, 0.0, 1.0)
        g, p = s.grid()
        assert np.array_equal(g, grid) and bool(p[0]) == path
        Ag, bg = s.get_system()
        assert np.array_equal(Ag, A) and np.array_equal(bg, b)
        s.init_linear(0.0, 1.0)
        s.sweeps(27)
        assert np.array_equal(s.get_field(), want)


def test_stages_reuse_the_fill():
    P = pkg()
    nx, ny = 130, 71
    rng = np.random.default_rng(3)
    pix = three_levels(rng, ny, nx, 0.36)
    grid, _ = host_fill(pix)
    with P.Solver(nx, ny) as a, P.Solver(nx, ny) as b:
        a.set_image(pix)
        b.set_image(pix)
        for k in range(7):
            Dg = 10.0 ** (k + 1)
            a.assemble_3phase_native(0.0, 1.0, Dg, 0.0, 1.0)
            b.assemble_3phase(0.0, 1.0, Dg, 0.0, 1.0, grid=grid)
            assert a.plan_value("fill_runs") == 1
            Aa, ba = a.get_system()
            Ab, bb = b.get_system()
            assert np.array_equal(Aa, Ab) and np.array_equal(ba, bb), Dg
        pix2 = three_levels(rng, ny, nx, 0.4)
        a.set_image(pix2)
        a.assemble_3phase_native(0.0, 1.0, 10.0, 0.0, 1.0)
        assert a.plan_value("fill_runs") == 2
        assert np.array_equal(a.grid()[0], host_fill(pix2)[0])


def test_refusals_leave_field_and_system_alone():
    P = pkg()
    nx, ny = 40, 32
    pix = three_levels(np.random.default_rng(8), ny, nx, 0.3)
    with P.Solver(nx, ny) as s:
        with pytest.raises(P.DeffError) as e:                          # no image
            s.assemble_3phase_native(1e-3, 1.0, 10.0, 0.0, 1.0)
        assert e.value.code == -5                                   # DEFF_ESTATE
        s.set_image(pix)
        with pytest.raises(P.DeffError) as e:                          # no fill yet
            s.grid()
        assert e.value.code == -5                                   # DEFF_ESTATE
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        s.sweeps(9)
        A0, b0 = s.get_system()
        x0 = s.get_field()
        with pytest.raises(P.DeffError):
            s.set_tuning("fill_impl", 3)
        with pytest.raises(P.DeffError):
            s.grid()
        A1, b1 = s.get_system()
        assert np.array_equal(A0, A1) and np.array_equal(b0, b1) and np.array_equal(x0, s.get_field())
    nx, ny = 1030, 517                                                 # 17 words x 517 rows: more than one workgroup holds
    with P.Solver(nx, ny) as s:
        s.synth_image(1, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        A0, b0 = s.get_system()
        x0 = s.get_field()
        s.set_tuning("fill_impl", 1)
        with pytest.raises(P.DeffError) as e:
            s.assemble_3phase_native(1e-3, 1.0, 10.0, 0.0, 1.0)
        assert e.value.code == -1 and "fill_impl" in str(e.value)
        A1, b1 = s.get_system()
        assert np.array_equal(A0, A1) and np.array_equal(b0, b1) and np.array_equal(x0, s.get_field())
        assert s.plan_value("fill_runs") == 0 and s.plan_value("native3_rows") == 0
    from effectivediffusivityfvm_amd import _capi
    L = _capi.load()
    with P.SlabRank(64, 64, 0, 1, P.rccl_unique_id()) as r:            # a row slab's context
        r.synth_image(1, 0)
        r.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        r.init_linear(0.0, 1.0)
        r.sweeps(8)
        x0 = r.get_field()
        assert L.deff_assemble_3phase_native(r._ctx, 1e-3, 1.0, 10.0, 0.0, 1.0) == -1
        assert b"slab" in L.deff_last_error()
        r.sweeps(8)
        x1 = r.get_field()
    with P.SlabRank(64, 64, 0, 1, P.rccl_unique_id()) as r:            # the same 16 sweeps without the refused call
        r.synth_image(1, 0)
        r.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        r.init_linear(0.0, 1.0)
        r.sweeps(8)
        assert np.array_equal(x0, r.get_field())
        r.sweeps(8)
        assert np.array_equal(x1, r.get_field())


# ---------------------------------------------------------------- the driver ---

def _write_input(path, **kv):
    open(path, "w").write("\n".join(["Input File:"] + [f"{k}: {v}" for k, v in kv.items()]) + "\n")


def _run_both_fills(tmp_path, extra, count):
    out = {}
    for fill in ("host", "device"):
        r = subprocess.run([EXE, "input.txt", "--json", f"res_{fill}.json", "--field-bin", f"field_{fill}", "--fill", fill,
                            "--precond-maxiter", "12000"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + r.stdout
        res = json.load(open(tmp_path / f"res_{fill}.json"))["results"]
        assert len(res) == count
        out[fill] = [{k: v for k, v in row.items() if k != "Time"} for row in res]
        shutil.move(tmp_path / "out.csv", tmp_path / f"out_{fill}.csv")
    assert out["host"] == out["device"]
    strip = lambda text: [",".join(c for i, c in enumerate(line.split(",")) if i != 5) for line in text.splitlines()]   # Time
    assert strip(open(tmp_path / "out_host.csv").read()) == strip(open(tmp_path / "out_device.csv").read())
    fields = sorted(f for f in os.listdir(tmp_path) if f.startswith("field_host"))
    assert len(fields) == count
    for f in fields:
        assert open(tmp_path / f, "rb").read() == open(tmp_path / f.replace("field_host", "field_device"), "rb").read(), f
    return out["device"]


def test_driver_fill_device_single_image(tmp_path):
    """The shipped 3-phase options on 00000.jpg (every stage capped at 12 000 sweeps): --fill device gives the numbers and the
    field of --fill host."""
    shutil.copy(os.path.join(GOLDEN, "00000.jpg"), tmp_path / "00000.jpg")
    _write_input(tmp_path / "input.txt", Phases=3, Ds=0, Df=1, Dg=1237500, MeshAmpX=1, MeshAmpY=1, InputName="00000.jpg", CR=1,
                 CL=0, OutputName="out.csv", printCMap=0, Convergence="1e-5", MaxIter=12000, Verbose=0, RunBatch=0, NumImages=1)
    res = _run_both_fills(tmp_path, [], 1)
    assert res[0]["PathFlag"] == 1 and len(res[0]["stage_iterations"]) == 7


def test_driver_fill_device_batch(tmp_path):
    """A numbered batch of four small three-level JPEGs through the stacked 3-phase continuation, groups of 3."""
    from PIL import Image
    rng = np.random.default_rng(77)
    for k in range(4):
        f = np.kron(rng.random((6, 8)), np.ones((8, 8)))
        a = np.where(f < 0.3, 0, np.where(f < 0.65, 150, 255)).astype(np.uint8)
        Image.fromarray(a).save(tmp_path / f"{k:05d}.jpg", quality=100)
    _write_input(tmp_path / "input.txt", Phases=3, Ds=0, Df=1, Dg=2500, MeshAmpX=1, MeshAmpY=1, CR=1, CL=0,
                 OutputName="out.csv", printCMap=0, Convergence="1e-4", MaxIter="3e5", Verbose=0, RunBatch=1, NumImages=4)
    _run_both_fills(tmp_path, ["--batch-size", "3"], 4)
