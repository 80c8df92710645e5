"""What every entry point of the face passes, the flux field, the side solves and the side vectors answers in every state of a
context: (code, message), or "ok", against tests/golden/pass_refusals.json -- recorded once from the library as it was before
these entry points were moved onto one host path (`python tests/test_gpu_pass_refusals.py` writes the file from whatever
DEFF_AMD_LIB names).  The order of an entry point's refusals shows in which message a state gets, so the table pins it per entry
point.  After every refused call the field, the side vectors and the device maps that were valid read back with the same bits.

A context of 5 x 4 cells (odd width: a pad column) with a stack of 2 images; the row-slab state is a one-rank SlabRank's context
of 5 x 8 cells (a slab has at least 8 rows), its transport never asked for anything."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_gpu_sequences import device_rows

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pass_refusals.json")
NX, NY, NIMG = 5, 4, 2
SLAB_NY = 8
WALLS = (0.0, 1.0)
EQUAL = (1.0, 1.0)                                       # CR == CL

# what a state is made of, in this order; "slab" and the assemblies with a Grid replace "system"
STEPS = ("system", "field", "lambda", "tangent", "all")
STATES = {
    "fresh": (),
    "system": STEPS[:1],
    "field": STEPS[:2],
    "lambda": STEPS[:3],
    "tangent": STEPS[:4],
    "all": STEPS,
    "all, then set_image": STEPS + ("set_image",),
    "all, then set_adjoint": STEPS + ("set_adjoint",),
    "grid": ("grid", "field", "vectors set"),
    "native3": ("native3", "field", "vectors set"),
    "slab": ("slab", "field"),
}
STATES.update({f"{name}, CR == CL": STATES[name] + ("equal",) for name in ("fresh", "system", "field", "lambda", "tangent")})


@pytest.fixture(scope="module")
def pkg():
    import torch  # noqa: F401  (first, so one HIP runtime serves torch and libdeff_amd)
    import effectivediffusivityfvm_amd as p
    return p


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Case:
    """One context in one state, and the planes the calls are given."""

    def __init__(self, pkg, state):
        from effectivediffusivityfvm_amd import _capi
        self.L = _capi.load()
        steps = STATES[state]
        self.walls = EQUAL if "equal" in steps else WALLS
        CL, CR = self.walls
        rng = np.random.default_rng(7)
        nimg, self.ny = (1, SLAB_NY) if "slab" in steps else (NIMG, NY)
        self.rows = rows = nimg * self.ny
        pix = rng.integers(0, 256, (rows, NX), dtype=np.uint8)
        self.D = np.exp(rng.standard_normal((rows, NX)))
        self.dD = rng.standard_normal((rows, NX))
        self.w = rng.standard_normal((rows, NX))
        self.nimg = nimg
        if "slab" in steps:
            self.owner = s = pkg.SlabRank(NX, SLAB_NY, 0, 1, transport=object())
        else:
            self.owner = s = pkg.Solver(NX, NY, nimg=nimg)
        self.ctx = s._ctx
        for step in steps:
            if step in ("system", "slab"):
                s.set_image(pix)
                s.assemble_2phase(1e-3, 1.0, CL, CR)
            elif step == "grid":
                s.set_image(pix)
                s.assemble_3phase(1e-3, 1.0, 10.0, CL, CR, grid=np.zeros((rows, NX), dtype=np.uint32))
            elif step == "native3":
                s.set_image(pix)
                s.assemble_3phase_native(1e-3, 1.0, 10.0, CL, CR)
            elif step == "field":
                s.init_linear(CL, CR)
            elif step == "lambda":
                s.solve_adjoint(self.w)
            elif step == "tangent":
                s.tangent_rhs(self.D, self.dD, CL, CR)
                s.solve_tangent()
            elif step == "all":
                s.adjoint_tangent_rhs(self.D, self.dD)
                s.solve_adjoint_tangent()
                s.sensitivity(self.D, CL, CR)
                s.flux_field(self.D, CL, CR)
                s.field_vjp(self.D, CL, CR)
                s.sens_hvp(self.D, self.dD, CL, CR)
                s.field_vjp_hvp(self.D, self.dD, CL, CR)
            elif step == "vectors set":
                s.set_adjoint(self.w)
                s.set_tangent(self.dD)
                s.set_adjoint_tangent(self.D)
            elif step == "set_image":
                s.set_image(pix[::-1].copy())
            elif step == "set_adjoint":
                s.set_adjoint(self.w[::-1].copy())

    def close(self):
        self.owner.close()

    # ---- the entry points: name -> (call, changes the context when it succeeds) ------------------------------------------
    def entries(self):
        L, c, (CL, CR) = self.L, self.ctx, self.walls
        D, dD, w = vp(self.D), vp(self.dD), vp(self.w)
        out = np.empty((self.rows, NX))
        sums = (C.c_double * self.nimg)()
        left, sec = np.empty((self.nimg, self.ny)), np.empty((self.nimg, NX + 1))
        res = (_cg_result() * self.nimg)()
        p, p2, pitch = C.c_void_p(), C.c_void_p(), C.c_size_t()
        table = {
            "deff_sensitivity": (lambda: L.deff_sensitivity(c, vp(out), sums, None), True),
            "deff_sensitivity_D": (lambda: L.deff_sensitivity_D(c, D, CL, CR, vp(out), sums, None), True),
            "deff_flux_field": (lambda: L.deff_flux_field(c, vp(out), vp(out), vp(left), vp(sec), None), True),
            "deff_flux_field_D": (lambda: L.deff_flux_field_D(c, D, CL, CR, vp(out), vp(out), vp(left), vp(sec), None), True),
            "deff_field_vjp_D": (lambda: L.deff_field_vjp_D(c, D, CL, CR, vp(out), sums, None), True),
            "deff_tangent_rhs_D": (lambda: L.deff_tangent_rhs_D(c, D, dD, CL, CR, vp(out), sums, None), True),
            "deff_adjoint_tangent_rhs_D": (lambda: L.deff_adjoint_tangent_rhs_D(c, D, dD, vp(out), sums, None), True),
            "deff_sensitivity_hvp_D": (lambda: L.deff_sensitivity_hvp_D(c, D, dD, CL, CR, vp(out), sums, None), True),
            "deff_field_vjp_hvp_D": (lambda: L.deff_field_vjp_hvp_D(c, D, dD, CL, CR, vp(out), sums, None), True),
            "deff_solve_adjoint": (lambda: L.deff_solve_adjoint(c, w, 1e-10, 1000, 64, res), True),
            "deff_solve_tangent": (lambda: L.deff_solve_tangent(c, 1e-10, 1000, 64, res), True),
            "deff_solve_adjoint_tangent": (lambda: L.deff_solve_adjoint_tangent(c, 1e-10, 1000, 64, res), True),
            "deff_set_adjoint": (lambda: L.deff_set_adjoint(c, w), True),
            "deff_set_tangent": (lambda: L.deff_set_tangent(c, w), True),
            "deff_set_adjoint_tangent": (lambda: L.deff_set_adjoint_tangent(c, w), True),
            "deff_get_adjoint": (lambda: L.deff_get_adjoint(c, vp(out)), False),
            "deff_get_tangent": (lambda: L.deff_get_tangent(c, vp(out)), False),
            "deff_get_adjoint_tangent": (lambda: L.deff_get_adjoint_tangent(c, vp(out)), False),
            "deff_device_flux_field": (lambda: L.deff_device_flux_field(c, C.byref(p), C.byref(p2), C.byref(pitch)), False),
        }
        for name in DEVICE_GETTERS:
            table[name] = (lambda fn=getattr(L, name): fn(c, C.byref(p), C.byref(pitch)), False)
        return table

    def snapshot(self):
        """Everything a refused call has to leave alone: the field, the three vectors, the device maps -- each as bytes, or the
        code that says there is none."""
        L, c = self.L, self.ctx
        snap = {}
        out = np.empty((self.rows, NX))
        for name in ("deff_get_adjoint", "deff_get_tangent", "deff_get_adjoint_tangent"):
            rc = getattr(L, name)(c, vp(out))
            snap[name] = out.tobytes() if rc == 0 else rc
        try:
            snap["field"] = self.owner.get_field().tobytes()
        except RuntimeError as e:                            # DeffError: no field yet
            snap["field"] = str(e)
        p, p2, pitch = C.c_void_p(), C.c_void_p(), C.c_size_t()
        for name in DEVICE_GETTERS:
            rc = getattr(L, name)(c, C.byref(p), C.byref(pitch))
            snap[name] = (p.value, device_rows(p.value, self.rows, pitch.value).tobytes()) if rc == 0 else rc
        rc = L.deff_device_flux_field(c, C.byref(p), C.byref(p2), C.byref(pitch))
        snap["deff_device_flux_field"] = rc if rc else (p.value, p2.value, device_rows(p.value, self.rows, pitch.value).tobytes(),
                                                        device_rows(p2.value, self.rows, pitch.value).tobytes())
        return snap


DEVICE_GETTERS = ("deff_device_adjoint", "deff_device_tangent", "deff_device_adjoint_tangent", "deff_device_sensitivity",
                  "deff_device_field_vjp", "deff_device_tangent_rhs", "deff_device_sensitivity_hvp", "deff_device_field_vjp_hvp")
ENTRY_POINTS = ("deff_sensitivity", "deff_sensitivity_D", "deff_flux_field", "deff_flux_field_D", "deff_field_vjp_D",
                "deff_tangent_rhs_D", "deff_adjoint_tangent_rhs_D", "deff_sensitivity_hvp_D", "deff_field_vjp_hvp_D",
                "deff_solve_adjoint", "deff_solve_tangent", "deff_solve_adjoint_tangent", "deff_set_adjoint", "deff_set_tangent",
                "deff_set_adjoint_tangent", "deff_get_adjoint", "deff_get_tangent", "deff_get_adjoint_tangent",
                "deff_device_flux_field") + DEVICE_GETTERS


def _cg_result():
    from effectivediffusivityfvm_amd._capi import CGResultC
    return CGResultC


def walk(pkg, state):
    """Every entry point in `state` -> {name: "ok" | [code, message]}.  The context is built anew after a call that went through
    and may have changed it."""
    answers = {}
    case = Case(pkg, state)
    try:
        assert set(case.entries()) == set(ENTRY_POINTS)
        for name in ENTRY_POINTS:
            call, changes = case.entries()[name]
            before = case.snapshot()
            rc = call()
            if rc == 0:
                answers[name] = "ok"
            else:
                answers[name] = [rc, case.L.deff_last_error().decode()]
            if rc != 0 or not changes:
                assert case.snapshot() == before, f"{state}: {name} changed what it had to leave alone"
            else:
                case.close()
                case = Case(pkg, state)
    finally:
        case.close()
    return answers


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_is_complete(golden):
    """Every state x every entry point is in the file, and nothing else."""
    assert set(golden) == set(STATES)
    for state, answers in golden.items():
        assert set(answers) == set(ENTRY_POINTS), state
    # the table is about refusals: each entry point is refused somewhere and goes through somewhere
    for name in ENTRY_POINTS:
        got = [golden[state][name] for state in STATES]
        assert "ok" in got and any(g != "ok" for g in got), name


@pytest.mark.parametrize("state", sorted(STATES))
def test_answers(pkg, golden, state):
    got = walk(pkg, state)
    for name in ENTRY_POINTS:
        print(f"{state}: {name}: {got[name]}")
    assert got == golden[state]


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch  # noqa: F401
    import effectivediffusivityfvm_amd as package
    table = {state: walk(package, state) for state in sorted(STATES)}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
