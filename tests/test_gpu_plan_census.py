"""What the sweep planner decides, context by context, against a census recorded on the MI355X
(tests/golden/plan_census.json): a change to the planner that is meant to keep every plan is held to that here.  Per
context: every tb_* key of deff_get_plan after a deff_sweeps(c, 0, omega) -- which plans and launches nothing --, the
sweeps per pass deff_last_launches reports and, for contexts of at most 1 Mi cells, the launches of 2 T + 1 sweeps.
All of it is compared for equality: the planner is deterministic for a given compute-unit count, so the test skips only
on a device with another count.

Record again (on the commit whose plans are the reference) with `python tests/test_gpu_plan_census.py --record [FILE]`."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "plan_census.json")
PLAN_KEYS = ("tb_T", "tb_LY", "tb_strips", "tb_chunks_per_image", "tb_blocks", "tb_impl", "tb_R", "tb_NW", "tb_resident", "tb_sym",
             "tb_fallbacks", "tb_ranked", "tb_aged", "tb_rank_misses", "tb_rank_lost")
SYM_ONLY_MESSAGE = "tb_T = 6 on 12-wave tiles: the tiles are not co-resident or the system is not link-symmetric"


def case(nx, ny, nimg=1, system="native", **tunings):
    name = f"{nimg}x{nx}x{ny}" if nimg > 1 else f"{nx}x{ny}"
    if system != "native":
        name += "-" + system
    for k, v in tunings.items():
        name += f"-{k}={v}"
    return dict(name=name, nx=nx, ny=ny, nimg=nimg, system=system, tunings=tunings)


def sq(n, **tunings):
    return case(n, n, **tunings)


CASES = (
    # one image, the planner's own choice: below, at and above every size where the form changes
    [sq(n) for n in (128, 512, 640, 768, 1024, 1100, 1101, 1152, 1172, 1200, 1208, 1209, 1280, 1536, 2048, 2304, 2560, 3072)]
    + [case(1030, 37), case(2, 64), case(97, 241), case(1001, 333)]
    # stacks (300 x 128^2: whole images beyond one per compute unit)
    + [case(128, 128, 16), case(128, 128, 64), case(128, 128, 200), case(128, 128, 256), case(256, 256, 16), case(512, 512, 16),
       case(1024, 1024, 2), case(1024, 1024, 4), case(128, 128, 300)]
    # one launch per pass
    + [sq(640, tb_launch=1), sq(1024, tb_launch=1), sq(1536, tb_launch=1), case(128, 128, 64, tb_launch=1)]
    # the form
    + [sq(512, tb_impl=1), sq(1024, tb_impl=1), sq(2560, tb_impl=2), sq(3072, tb_impl=2), case(1024, 1024, 4, tb_impl=2)]
    + [sq(1024, tb_NW=8), sq(1536, tb_NW=8), case(128, 128, 16, tb_NW=8), sq(640, tb_NW=12), sq(1152, tb_NW=12), sq(1536, tb_NW=12),
       sq(640, tb_NW=16), sq(1024, tb_NW=16), sq(2560, tb_NW=16)]
    # sweeps per pass, alone and on 12-wave tiles
    + [sq(n, tb_T=T) for n in (1024, 1152, 3072) for T in (4, 6, 8)]
    + [sq(n, tb_NW=12, tb_T=T) for n in (1024, 1152, 1200) for T in (4, 6, 8)]
    # the caller's tile shape
    + [sq(1024, tb_R=4), sq(1024, tb_R=6), sq(1024, tb_R=7), sq(1536, tb_R=6), sq(1536, tb_NW=16, tb_R=8), sq(1024, tb_NW=12, tb_R=5),
       sq(1024, tb_LY=11), sq(1536, tb_LY=20), sq(3072, tb_LY=64), sq(1024, tb_wg=128), sq(3072, tb_wg=256)]
    # the short-cuts and the rows by age
    + [sq(768, tb_sym=2), sq(1024, tb_sym=2), sq(1152, tb_sym=2), sq(1536, tb_sym=2), case(128, 128, 64, tb_sym=2),
       sq(1536, tb_tall_deal=0), sq(2048, tb_tall_deal=0), sq(768, tb_sym_age=0), sq(1024, tb_sym_age=0),
       sq(768, tb_sym_shape=1), sq(1024, tb_sym_shape=2), sq(1024, tb_sym_shape=5), sq(1100, tb_sym_shape=3)]
    # streaming: dealt tiles, strip placement; the contracted arithmetic's kernels
    + [sq(3072, tb_ranked=0), sq(2560, tb_ranked=0), sq(1024, tb_wall_halo=0), sq(1024, tb_wall_halo=1), sq(3072, tb_wall_halo=0),
       sq(3072, tb_wall_halo=1), case(128, 128, 64, tb_wall_halo=1), sq(1024, fma=1), sq(1536, fma=1), sq(3072, fma=1)]
    # systems: guarded (a phase of zero diffusivity), three phases (harvested dictionary), dictionaries harvested from a
    # link-symmetric matrix and from one that is not, a system that stays explicit
    + [case(256, 256, system="guard"), case(1024, 1024, system="guard"), case(1536, 1536, system="guard"),
       case(128, 128, system="three_phase"), case(512, 512, system="three_phase"),
       case(700, 600, system="dict_sym"), case(700, 600, system="dict_asym"), case(700, 600, system="dict_asym", tb_NW=12, tb_R=4),
       case(1536, 600, system="dict_asym"), case(64, 40, system="explicit")]
)
assert len({c["name"] for c in CASES}) == len(CASES)


def img00000():
    return np.load(os.path.join(HERE, "golden", "img00000_pix_stb.npy"))


def set_system(s, ob, c):
    """The image or system of case c and a linear field."""
    nx, ny, system = c["nx"], c["ny"], c["system"]
    if system == "native":
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
    elif system == "guard":
        s.set_image(np.tile(img00000(), (ny // 128, nx // 128)))
        s.assemble_2phase(0.0, 1.0, 0.0, 1.0)
    elif system == "three_phase":
        pix = np.tile(img00000(), (ny // 128, nx // 128))
        grid, _ = ob.floodfill((pix > 200).astype(np.uint32))
        s.set_image(pix)
        s.assemble_3phase(0.0, 1.0, 1237500.0, 0.0, 1.0, grid)
    else:
        rng = np.random.default_rng(2718)
        if system == "explicit":
            D = rng.uniform(0.5, 2.0, size=(ny, nx))                 # every cell its own diffusivity: no dictionary
        else:
            D = ob.fill_D_2phase(np.where(rng.random((ny, nx)) < 0.5, 0, 255).astype(np.uint8), 1.0, 1e-2)
        A, b = ob.discretize(D, 0.0, 1.0)
        if system == "dict_asym":
            A = A.copy().reshape(ny, nx, 5)
            A[:, :, 2] *= 1.0 + 2.0 ** -10                           # E links that differ from their partners' W links
            A = A.reshape(-1, 5)
        s.set_system(A, b, D, 0.0, 1.0)
    s.init_linear(0.0, 1.0)


def census(pkg, ob, c):
    """What the planner decides for case c (see the module's docstring)."""
    with pkg.Solver(c["nx"], c["ny"], nimg=c["nimg"]) as s:
        set_system(s, ob, c)
        for k, v in c["tunings"].items():
            s.set_tuning(k, v)
        try:
            s.sweeps(0)
        except pkg.DeffError as e:                                   # (a caller's form that does not fit: part of the census)
            return {"error": str(e)}
        out = {"kernel": s.kernel_in_use()}
        out.update({k: s.plan_value(k) for k in PLAN_KEYS})
        out["sweeps_per_pass"] = s.last_launches()[1]
        if c["nx"] * c["ny"] * c["nimg"] <= 1 << 20:
            s.sweeps(2 * out["sweeps_per_pass"] + 1)
            out["launches"] = s.last_launches()[0]
        return out


def compute_units():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


@pytest.fixture(scope="module")
def census_recorded():
    with open(FIXTURE) as f:
        rec = json.load(f)
    if rec["compute_units"] != compute_units():
        pytest.skip(f"the census was recorded on {rec['compute_units']} compute units, this device has {compute_units()}")
    return rec["cases"]


def test_the_census_holds_every_case(census_recorded):
    assert set(census_recorded) == {c["name"] for c in CASES}


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_plan_is_the_recorded_one(pkg, oracle, census_recorded, c):
    got = census(pkg, oracle, c)
    print(c["name"], got)
    assert got == census_recorded[c["name"]]


def test_twelve_wave_tiles_at_a_callers_T_that_do_not_fit_are_an_error(pkg):
    """tb_NW = 12 with tb_T = 6: 12-wave tiles or nothing; at T = 6 the tiles of a 1200^2 image are not co-resident (1172
    columns are the most that fit)."""
    with pkg.Solver(1200, 1200) as s:
        s.synth_image(12345, 0)
        s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
        s.init_linear(0.0, 1.0)
        s.set_tuning("tb_NW", 12)
        s.set_tuning("tb_T", 6)
        with pytest.raises(pkg.DeffError) as e:
            s.sweeps(0)
        assert SYM_ONLY_MESSAGE in str(e.value)


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"] or len(sys.argv) > 3:
        sys.exit("usage: python tests/test_gpu_plan_census.py --record [FILE]")
    target = sys.argv[2] if len(sys.argv) == 3 else FIXTURE
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import torch  # noqa: F401  (first, so one HIP runtime serves torch and the library)
    import oracle_binding
    import effectivediffusivityfvm_amd
    oracle_binding.build()
    rec = {"compute_units": compute_units(), "cases": {c["name"]: census(effectivediffusivityfvm_amd, oracle_binding, c) for c in CASES}}
    with open(target, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} cases on {rec['compute_units']} compute units -> {target}")
