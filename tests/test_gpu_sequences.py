"""Random sequences of C-ABI calls on one context against a model made of the CPU oracle.

The parity tests elsewhere each exercise one flow (image -> assembly -> guess -> sweeps / solve -> read).  A context is a
state machine -- field ping-pong, frozen images of a stack, resident intervals and their restart copy, a row dictionary that
belongs to one assembly, plans that depend on tuning -- and the bug ADVICE r03 found by reading (an unchecked resident interval
outliving the field it ran under) lives BETWEEN calls.  Here every seed draws ~30 calls at random from: new image, assembly
(2-phase with changing Ds / Df / walls, 3 pixel classes, from a D plane), linear guess, a caller's field, sweeps (omega 2/3 and
1), solve (small MAX_ITER / check interval: stops by tolerance, by MAX_ITER on and between checks), wall fluxes, residual,
field read-back, and changes of kernel / sweeps per pass / tile form / launch mode in between.  After every call that returns
numbers they are compared with the oracle's: fields, sweep counts, Deff and conv bit for bit, the residual as
oracle_binding.assert_residual does.

With `with_cg` the draw also holds deff_solve_cg (small and large max_iter, two tolerances, two check intervals).  CG is not
the reference's algorithm, so its field is not the oracle's: it is checked by its own residual, its Deff and wall fluxes bit
for bit against the oracle's flux evaluation of the field read back, and then the model ADOPTS that field -- every later
sweep, solve, flux and residual has to match the oracle bit for bit from there, which is what shows that CG left the Jacobi
tables, the plans, the frozen-image bookkeeping and the field ping-pong as it found them."""
import numpy as np
import pytest

from test_cg_host import residual_np

pytestmark = pytest.mark.gpu

SHAPES = [(64, 48), (130, 70), (97, 41), (256, 130), (40, 300), (512, 512)]


@pytest.fixture(scope="module")
def pkg():
    import effectivediffusivityfvm_amd as p
    return p


class Model:
    """The oracle's side of one stack of B images."""

    def __init__(self, ob, nx, ny, B, rng):
        self.ob, self.nx, self.ny, self.B, self.rng = ob, nx, ny, B, rng
        self.pix = None
        self.D = self.A = self.b = None
        self.x = None
        self.CL, self.CR = 0.0, 1.0
        self.kind = None                                     # "2p" / "3p" / "D": how the current system was assembled

    def new_image(self):
        self.pix = draw_images(self.rng, self.nx, self.ny, self.B)
        self.kind = None

    def assemble(self, kind, Ds, Df, Dg, CL, CR, D=None, base=None):
        """kind "3n" / "3g": three pixel classes with the flood-filled Grid (ImpSolid rows); "S" / "Sw": a caller's system, the
        oracle's of the plane `base` names, "Sw" with the wall-column links of wrap_system()."""
        ob = self.ob
        self.CL, self.CR, self.kind = CL, CR, kind
        plane = base if kind in ("S", "Sw") else kind
        if plane == "2p":
            self.D = [ob.fill_D_2phase(p, Df, Ds) for p in self.pix]
        elif plane in ("3p", "3n", "3g"):
            self.D = [ob.fill_D_3phase(p, Df, Ds, Dg) for p in self.pix]
        else:
            self.D = D if D is not None else draw_D_planes(self.rng, self.nx, self.ny, self.B, Ds, Df, Dg)
        self.grid = [ob.floodfill((p > 200).astype(np.uint32))[0] for p in self.pix] if kind in ("3n", "3g") else None
        sys_ = [ob.discretize(D, CL, CR, grid=self.grid[k] if self.grid else None) for k, D in enumerate(self.D)]
        self.A, self.b = [s[0] for s in sys_], [s[1] for s in sys_]
        if kind == "Sw":
            for A in self.A:
                A.reshape(self.ny, self.nx, 5)[1:, 0, 1] = -0.125

    def stacked(self, arrs):
        return np.concatenate(arrs, axis=0)


def draw_images(rng, nx, ny, count):
    p = rng.uniform(0.3, 0.7)
    vals = np.array([0, 30, 120, 199, 201, 255], dtype=np.uint8)
    if rng.random() < 0.5:
        return [np.where(rng.random((ny, nx)) < p, 0, 255).astype(np.uint8) for _ in range(count)]
    return [rng.choice(vals, size=(ny, nx)) for _ in range(count)]


def draw_D_planes(rng, nx, ny, count, Ds, Df, Dg):
    levels = np.array([Ds, Df, Dg, 0.5 * (Ds + Df)])
    return [levels[rng.integers(0, 4, size=(ny, nx))] for _ in range(count)]


# ---------------------------------------------------------------------------------------------------------------------------
# The draw.  It depends on the generator and on three facts of the model's state (how the system was assembled, whether there
# is a field, the stack size) -- never on what the GPU returns -- so it is separate from the execution: run_sequence() below
# executes it against a context and the oracle, tests/test_sequences_host.py replays it without a GPU and counts what the
# seeds reach.  Every option defaults to off, and with all of them off the generator is consumed exactly as before they
# existed: the seeds 1000-1039 and 2000-2023 draw the sequences they always drew.
#
#   onchip   the tune draw may set "cg_onchip"; after every cg the form that ran (deff_get_plan "cg_impl") is asserted
#   stream   deff_solve_stream of B ... 3B+1 images on a stack (B >= 2); the model becomes what deff_amd.h says the context holds
#   ptr      deff_synchronize + deff_device_field, read with the HIP runtime's own hipMemcpy: pitch, pad column, every cell
#   slot     deff_get_slot_field of a random slot outside any callback
#   stamps   deff_debug_tb_stamps: sizing call, real call, the field advances by T (3 T on a resident plan) sweeps
#   fma      the tuning key "fma" as a per-context choice, drawn once per seed before the first guess

ONCHIP_LIMIT = 16384                                         # cells (row pitch x ny) one compute unit holds: deff_amd.h, "cg_onchip"
SOLVE_TOL, SOLVE_MAX_ITER, SOLVE_CE = [1e-2, 1e-4, 1e-12], [1, 7, 100, 101, 130, 301], [7, 50, 100]
ASSEMBLE_D = [(1e-3, 1.0, 10.0), (1e-2, 1.0, 50.0), (0.1, 2.0, 7.0)]
ASSEMBLE_C = [(0.0, 1.0), (0.25, 0.75)]


# The options below draw what the ABI gained after those (each has a flow test of its own; here it meets a context that other
# calls have changed).  The draw then follows a few more facts of the model's state -- whether the device fill is the current
# image's, the kernel and "prescaled" settings (a pre-scaled stream on the explicit kernel is refused and changes nothing),
# the last two ops -- and still nothing the GPU returns:
#
#   native3   assembly kinds "3n" (deff_assemble_3phase_native) and "3g" (deff_assemble_3phase with the oracle's flood-filled
#             Grid), the ops "stage" (the native assembly again on the same image: a continuation stage) and "grid"
#             (deff_get_grid, while the device fill is the current image's), the keys "fill_impl" / "fill_tile_rows", and the
#             kernel draw on "3n" as on "2p" (explicit / scalar force the planes that are built on demand)
#   system    kinds "S" (deff_set_system with the oracle's system of a drawn 2p / 3p / D plane) and "Sw" (even widths: the same
#             with wall-column links into the neighbouring row, an explicit-only system), the op "getsys" (deff_get_system)
#   cgkeys    the keys "cg_planes" and "cg_fold"
#   cgstream  deff_solve_cg_stream of B ... 3B+1 images on a stack (B >= 2); about one in four is asked with Df = -1 and refused
#   sens      deff_sensitivity / deff_sensitivity_D of the current field
#   prescaled the key "prescaled" (never with fma or stamps: the pre-scaled sweeps ignore the one and have no stamped form)
#   adjoint   the field adjoint: "adj" (deff_solve_adjoint: refused on "Sw"; small max_iter leaves a partial lambda, which is
#             valid all the same; on a stack about one call in four has w = 0 on one image), "setadj" (deff_set_adjoint),
#             "getadj" (deff_get_adjoint + deff_device_adjoint) and "vjp" (deff_field_vjp_D on the model's planes or on a drawn
#             plane with zero cells, walls drawn anew, + deff_device_field_vjp; also the first reader of some solves).  The draw
#             follows one more fact: whether lambda is valid -- deff_amd.h's lifetime rule applied to the ops drawn so far

#
# ... and the second-order calls, which share five validity flags, one upload scratch of two planes, the CG work vectors and the
# field ping-pong with everything above.  The draw follows five facts by deff_amd.h's lifetime rules applied to the ops drawn so
# far -- lambda, the tangent's right-hand side and dx, dlambda's right-hand side and dlambda -- and whether flux maps exist:
#
#   tangent   "trhs" (deff_tangent_rhs_D on the model's planes or on a drawn plane with zero cells; dD drawn, dD = D and a dD that
#             is non-zero where D == 0 included; walls drawn anew, CR == CL included), "tan" (deff_solve_tangent, max_iter 0 / 3 /
#             large), "settan", "gettan" (deff_get_tangent + deff_device_tangent) and "hvp" (deff_sensitivity_hvp_D; CR == CL is
#             refused)
#   second    "arhs", "atan", "setatan", "getatan" and "fhvp": the same five for dlambda and deff_field_vjp_hvp_D
#   fluxfield "ff" (deff_flux_field_D, then deff_flux_field, whose outcome follows the kind of system), "ffptr"
#             (deff_device_flux_field) and the key "flux_kt"
#   onchip_planes  the key "cg_onchip_planes" (also "opflip": the key flipped between a right-hand side and its solve); after every
#             side solve and every plane-form cg the form that ran is asserted

# (key, values) pairs the tune draw gains per option; "cg keys" sets both CG keys in one draw, "prescaled" mostly toggles
TUNE_EXTRA = dict(fluxfield=[("flux_kt", [0, 1, 2])] * 8,
                  onchip_planes=[("cg_onchip_planes", [0, 1, 1])] * 6,
                  native3=[("fill_impl", [0, 1, 2])] * 3 + [("fill_tile_rows", [0, 8, 16])] * 4,
                  cgkeys=[("cg keys", None)] * 12,
                  prescaled=[("prescaled", None)] * 10,
                  sens=[("tb_impl", [2])] * 8 + [("tb_launch", [0])] * 2)     # (towards resident tiles: a gradient inside a pending interval)
CG_PLANES_DRAW, CG_FOLD_DRAW = [0, 0, 1, 2], [0, 1, 1, 2, 2]
PASS_WALLS = ASSEMBLE_C + [(0.5, 0.5)]                       # the walls of a drawn pass: CR == CL is allowed by all but "hvp"
PASSES = ("trhs", "arhs", "vjp", "hvp", "fhvp", "sens", "ff")       # every one uploads its planes into the one scratch


def draw_sequence(seed, with_cg=False, shapes=SHAPES, stacks=(1, 1, 3), steps=30, onchip=False, stream=False, ptr=False,
                  slot=False, stamps=False, fma=False, native3=False, system=False, cgkeys=False, cgstream=False, sens=False,
                  prescaled=False, adjoint=False, tangent=False, second=False, fluxfield=False, onchip_planes=False):
    """Generator of (op, arguments...) tuples; the first is ("open", nx, ny, B, fma) and the second the first image."""
    assert not (fma and with_cg)                             # CG's arithmetic has no contracted form to compare with
    assert not (prescaled and (fma or stamps))
    rng = np.random.default_rng(seed)
    nx, ny = shapes[rng.integers(len(shapes))]
    B = int(rng.choice(list(stacks)))
    use_fma = int(rng.integers(2)) if fma else 0
    yield ("open", nx, ny, B, use_fma)
    yield ("image", draw_images(rng, nx, ny, B))
    kind, have_x = None, False
    fill = False                                             # the context holds a device fill of the current image
    kset, pre = "auto", 0                                    # deff_set_kernel's and "prescaled"'s current values
    prev = prev2 = None                                      # the two ops before
    refused_on_3n = False                                    # the last call was a refused CG stream on a native 3-phase system
    after_stream = False                                     # a stream filled the slots and no assembly has followed
    pre_swept = False                                        # the current system has been swept under "prescaled" 1
    lam_valid = lam_lost = False                             # the adjoint field: valid / was valid and an invalidator has just run
    adj_since = False                                        # an adjoint solve has run on the current system
    refused_last = False                                     # the op before was refused (as far as the draw can know)
    tb_keys = {"tb_impl": 0, "tb_launch": 0}                 # (followed under `adjoint` only: towards resident tiles)
    sw = "Sw" if nx % 2 == 0 else "S"                        # (an odd width cannot represent a wall-column link: refused)
    kinds = ["2p", "2p", "3p", "D"] + (["3n", "3n", "3g"] if native3 else []) + (["S", sw, sw] if system else [])
    extra = [kv for name, on in (("native3", native3), ("cgkeys", cgkeys), ("prescaled", prescaled), ("sens", sens),
                                 ("fluxfield", fluxfield), ("onchip_planes", onchip_planes)) if on for kv in TUNE_EXTRA[name]]
    newer = tangent or second or fluxfield or onchip_planes
    assert not newer or (adjoint and not prescaled)          # (the later options extend the adjoint's bookkeeping)
    tan_rhs = tan_valid = atan_rhs = atan_valid = False      # the tangent's right-hand side and dx, dlambda's and dlambda
    dx_lost = dl_lost = False                                # dx / dlambda was valid and an invalidator has just run
    op_key = 0                                               # "cg_onchip_planes"
    hist = []                                                # every op drawn so far (followed under the later options only)
    for step in range(steps):
        ops = ["image", "assemble", "tune"]
        if kind is not None:
            ops += ["init", "set_field"]
            if have_x:
                ops += ["sweeps", "sweeps", "solve", "solve", "flux", "get", "residual"]
                if with_cg:
                    ops += ["cg", "cg"]
                if onchip:
                    ops += ["cg", "cg"]                      # (the seeds of the two forms are there for CG)
                if ptr:
                    ops += ["ptr"]
                if slot:
                    ops += ["slot"]
                if stamps:
                    ops += ["stamps"]
                if sens:
                    # (sweeps, the gradient, then a solve in a row -- the gradient inside a resident interval that no check has
                    # settled yet -- would be a rare order at even weights)
                    ops += ["sens", "sens"] + (["sens"] * 12 if prev == "sweeps" else []) + (["solve"] * 16 if (prev2, prev) == ("sweeps", "sens") else [])
            if system:
                ops += ["getsys"]
        if stream and B >= 2:
            ops += ["stream"]
        # The weights of the later options.  Even weights would leave the call orders they are there for (the list in
        # test_sequences_host.py) to a seed in a hundred: an order of three particular calls among twenty kinds.  So what has
        # just happened raises the weight of what makes such an order: keys change often; a native fill is followed by another
        # kind and by the native assembly again; wall-column links by a 2-phase assembly; a refused CG stream on a native
        # system by a read of its planes; pre-scaled sweeps by the key and by sweeps again.
        if extra:
            ops += ["tune", "tune"]
        if native3 or system:
            ops += ["assemble"] * (3 if fill or kind == "Sw" or after_stream else 1)
        if native3:
            ops += (["stage"] * 3 if kind == "3n" else []) + (["grid"] * 2 if fill else [])
            if system and kind == "3n":
                ops += ["getsys"] * 3                        # (the planes of a native system are built on demand)
        if system and kind == "Sw" and have_x and (with_cg or onchip):
            ops += ["cg"] * 9                                # (refused: an explicit-only system)
        if cgstream and B >= 2:
            ops += ["cgstream"] * (6 if kind == "3n" else 1)
            if refused_on_3n and kind == "3n":
                ops += ["getsys"] * 8
        if prescaled and have_x and kind is not None:
            ops += ["sweeps"] * (8 if pre_swept and not pre else 3) + (["prescaled"] * 5 if prev == "sweeps" and pre else [])
        if adjoint:
            tb2 = (tb_keys["tb_impl"], tb_keys["tb_launch"]) == (2, 0) and kset in ("auto", "matfree_tb") and kind != "Sw"
            # The adjoint's ops and the weights of the orders they are drawn for (A1 ... A8 in test_sequences_host.py).  The reads
            # are offered at a low weight whatever the state (refused while lambda is invalid or no field exists) and at a high
            # one right after an invalidator took a valid lambda away, or after a refused call left one in place.
            ops += ["getadj", "vjp"] + (["getadj"] * 10 + ["vjp"] * 10 if lam_lost else [])
            if kind is not None:
                ops += ["adj", "adj", "setadj", "tune", "tune", "tune"]
                if kind in ("2p", "3n"):                     # (the first call that needs a native system's planes, then a read of them)
                    ops += ["getsys"] * 6 if adj_since else ["adj"] * 8
                if kind == "Sw":                             # (refused: an explicit-only system; with a caller's lambda in place)
                    ops += ["adj"] * 30 if lam_valid else ["setadj"] * 20 + ["adj"] * 10
                if prev == "setadj":
                    ops += ["adj"] * 14
                if prev == "adj":                            # (then CG, in whichever form "cgform" has just chosen)
                    ops += ["setadj"] * 20 + (["cg"] * 10 + ["cgform"] * 40 if have_x else [])
                if (prev2, prev) == ("adj", "cgform") and have_x:
                    ops += ["cg"] * 100
                if prev == "cg":
                    ops += ["adj"] * 10
                if (prev2, prev) == ("cg", "adj") and have_x:
                    ops += ["cg"] * 40
                if tb2 and have_x and prev != "sweeps":
                    ops += ["sweeps"] * 8
                if prev == "sweeps":
                    ops += (["adj"] * 10 + (["vjp"] * 10 if lam_valid else [])) * (3 if tb2 else 1)
                if prev2 == "sweeps" and prev in ("adj", "vjp") and have_x:
                    ops += ["solve"] * (60 if tb2 else 10)   # (inside a resident interval that no check has settled)
                if lam_valid:
                    ops += ["getadj"] * 2 + (["vjp"] * 2 if have_x else [])
                    if refused_last or (prev == "cg" and prev2 in ("adj", "cgform")):
                        ops += ["getadj"] * 60
                    if (prev2, prev) == ("adj", "setadj") and have_x:
                        ops += ["vjp"] * 60
                    if have_x and prev == "vjp" and sens:
                        ops += ["sens"] * 14
                    if have_x and prev == "sens":
                        ops += ["vjp"] * 16
                    if have_x and prev == "solve" and B >= 2:
                        ops += ["solve"] * 2                 # (a stack's solve whose first reader may be the pass)
                    # the invalidators that even weights would leave rare while a lambda is there to lose
                    ops += (["stream"] * 2 if stream and B >= 2 else []) + (["cgstream"] * 5 if cgstream and B >= 2 else [])
                    ops += ["stage"] * 24 if native3 and kind == "3n" else []
        if newer:
            # The later options' ops and the weights of the orders they are drawn for (T1 ... T12 in test_sequences_host.py).  As
            # for the adjoint: every read and pass is offered at a low weight whatever the state (refused while what it needs is
            # missing), and at a high one where it continues a chain -- a right-hand side is followed by its solve, a solve by a
            # read and a pass, a lost vector by the calls that must now be refused.
            tb2 = (tb_keys["tb_impl"], tb_keys["tb_launch"]) == (2, 0) and kset in ("auto", "matfree_tb") and kind != "Sw"
            sysok = kind is not None
            h3 = tuple(hist[-3:])
            if tangent:
                ops += ["trhs", "trhs", "gettan", "hvp"] + (["trhs"] * 25 if have_x and sysok and kind != "Sw" and not tan_rhs else [])
                # (with no system the solve is drawn only where it is refused for lack of a right-hand side, and the setter not
                # at all: whether a context without a system still has one to solve on is not specified)
                ops += ["tan", "settan"] if sysok else [] if tan_rhs else ["tan"]
                if dx_lost:
                    ops += ["gettan"] * 40 + ["hvp"] * 40 + ["tan"] * 40
                if prev == "trhs" and sysok and tan_rhs:
                    ops += ["tan"] * 1000 + (["opflip"] * 150 if onchip_planes else [])
                if h3[-2:] == ("trhs", "opflip"):
                    ops += ["tan"] * 2000
                if prev == "tan" and tan_valid:
                    ops += ["gettan"] * 600 + ["hvp"] * 60 + (["cgform"] * 150 + ["cg"] * 20 if have_x and with_cg else []) + ["adj"] * 20
                    ops += ["atan"] * 150 if atan_rhs and second else []
                if h3[-2:] == ("tan", "gettan") and have_x:
                    ops += ["hvp"] * 1500
                if h3[-2:] == ("tan", "cgform") and have_x and with_cg:
                    ops += ["cg"] * 1500
                if h3 == ("tan", "cgform", "cg") and tan_valid:
                    ops += ["gettan"] * 1500
                if prev == "cg" and tan_rhs and sysok:
                    ops += ["tan"] * 300
                if h3[-2:] == ("cg", "tan") and have_x and with_cg:
                    ops += ["cg"] * 1500
                if prev == "settan" and have_x:
                    ops += ["hvp"] * 40
                if tan_valid:
                    ops += ["gettan", "hvp"] + (["adj"] * 200 if sysok and not lam_valid and kind != "Sw" else [])
                    if refused_last:
                        ops += ["gettan"] * 40
                    # the invalidators that even weights would leave rare while a dx is there to lose
                    ops += (["stream"] * 2 if stream and B >= 2 else []) + (["cgstream"] * 5 if cgstream and B >= 2 else [])
                    ops += ["stage"] * 24 if native3 and kind == "3n" else []
                    ops += ["image"] * 2 + ["assemble"] * 4
                if kind == "Sw":                             # (the side solves are refused: with a caller's dx in place)
                    ops += ["tan"] * 20 if tan_valid else ["settan"] * 20
            if second:
                ops += ["arhs", "getatan", "fhvp"] + (["atan", "setatan"] if sysok else [] if atan_rhs else ["atan"])
                if dl_lost:
                    ops += ["getatan"] * 40 + ["fhvp"] * 40 + ["atan"] * 40
                if lam_valid and prev in ("adj", "setadj") and not atan_valid and not dl_lost:
                    ops += ["arhs"] * 1000
                if prev == "arhs" and sysok and atan_rhs:
                    ops += ["atan"] * 1000 + (["opflip"] * 150 if onchip_planes else [])
                if h3[-2:] == ("arhs", "opflip"):
                    ops += ["atan"] * 2000
                if prev == "atan" and atan_valid:
                    ops += ["fhvp"] * 1000 + ["getatan"] * 60 + (["tan"] * 60 if tan_rhs else ["trhs"] * 30) + ["adj"] * 30 + ["setadj"] * 30
                if prev == "setatan" and have_x:
                    ops += ["fhvp"] * (300 if lam_valid and tan_valid else 40) + (["settan"] * 20 if not tan_valid and sysok else [])
                if lam_valid and tan_valid and have_x and sysok:
                    ops += ["setatan"] * 10
                if prev == "hvp" and tan_valid and have_x and sysok and kind != "Sw":       # (the tangent's chain, then dlambda's)
                    ops += ["adj"] * 1000
                if atan_valid:
                    ops += ["getatan", "fhvp"] + (["trhs"] * 4 if not tan_valid else [])
                    if refused_last:
                        ops += ["getatan"] * 40
                if kind == "Sw" and lam_valid:
                    ops += ["atan"] * 10 if atan_valid else ["setatan"] * 20
            if fluxfield:
                ops += ["ff", "ff", "ffptr"] + (["ff"] * 200 if kind == "3n" and have_x and (tan_valid or atan_valid) else [])
                if prev in ("image", "assemble", "stage") and have_x:
                    ops += ["ff"] * 60
                if prev == "ff":
                    ops += ["ffptr"] * 6
            if prev in PASSES:                               # three different passes in a row: the one upload scratch
                ops += [p for p, on in (("trhs", tangent), ("hvp", tangent and tan_valid), ("arhs", second and lam_valid),
                                        ("fhvp", second and atan_valid and tan_valid and lam_valid), ("ff", fluxfield),
                                        ("vjp", lam_valid), ("sens", sens and sysok and have_x)) if on and p != prev] * 5
            if have_x and sysok:
                # a pass inside a resident interval that no check has settled (sweeps, the pass, a solve in a row), and a
                # stack's solve whose first reader is the pass
                first = (["trhs"] if tangent else []) + (["ff"] if fluxfield else [])
                if tb2 and prev != "sweeps":
                    ops += ["sweeps"] * 60
                if prev == "sweeps":
                    ops += first * (100 if tb2 else 6) + (["ff"] * 80 if tb2 and fluxfield else [])
                if prev2 == "sweeps" and prev in ("trhs", "ff"):
                    ops += ["solve"] * (4000 if tb2 else 10)
                if onchip_planes and op_key == 1 and with_cg:    # (the plane form of the forward solve under the key)
                    ops += ["cgform"] * 10 + ["cg"] * (200 if prev == "cgform" else 4)
        op = ops[rng.integers(len(ops))]
        prev2, prev = prev, op
        hist.append(op)
        refused_on_3n = False
        refused_last = False
        dx_lost = dx_lost and op in ("tune", "kernel", "cgform", "opflip")       # (the boost lasts for one call that is no key)
        dl_lost = dl_lost and op in ("tune", "kernel", "cgform", "opflip")
        if op in ("image", "assemble", "stage"):             # (a new image or system: lambda was the old one's)
            dx_lost, dl_lost = tan_valid, atan_valid
            tan_rhs = tan_valid = atan_rhs = atan_valid = False
            lam_lost, lam_valid, adj_since = lam_lost or lam_valid, False, False
        if op == "image":
            yield ("image", draw_images(rng, nx, ny, B))
            kind, fill, after_stream, pre_swept = None, False, False, False
        elif op == "assemble":
            more = (["3n"] * 4 if (fill and kind != "3n") or (native3 and after_stream) else []) + (["2p"] * 4 if kind == "Sw" else [])
            if fill and kind == "3n":
                more = [k for k in kinds if k != "3n"]       # (another kind on the filled image, then "3n" again)
            if adjoint and system and sw == "Sw" and kind != "Sw":
                more = more + ["Sw"] * 3                     # (the system the adjoint solve refuses)
            kind = (kinds + more)[rng.integers(len(kinds) + len(more))]
            Ds, Df, Dg = ASSEMBLE_D[rng.integers(3)]
            CL, CR = ASSEMBLE_C[rng.integers(2)]
            if kind in ("S", "Sw"):                          # the plane whose system the caller hands over
                base = ["2p", "3p", "D"][rng.integers(3)]
                yield ("assemble", kind, Ds, Df, Dg, CL, CR, draw_D_planes(rng, nx, ny, B, Ds, Df, Dg) if base == "D" else None, base)
            else:
                yield ("assemble", kind, Ds, Df, Dg, CL, CR, draw_D_planes(rng, nx, ny, B, Ds, Df, Dg) if kind == "D" else None)
            fill = fill or kind == "3n"
            after_stream = pre_swept = False
            if kind in ("D", "S", "Sw"):
                kset = "auto"                                # (run_sequence sets the kernel back for a caller's planes)
        elif op == "stage":
            Ds, Df, Dg = ASSEMBLE_D[rng.integers(3)]
            CL, CR = ASSEMBLE_C[rng.integers(2)]
            yield ("stage", Ds, Df, Dg, CL, CR)
        elif op == "cgstream":
            count = int(rng.integers(B, 3 * B + 2))
            imgs = draw_images(rng, nx, ny, count)
            Ds, Df, _ = ASSEMBLE_D[rng.integers(3)]
            CL, CR = ASSEMBLE_C[rng.integers(2)]
            rtol = float(rng.choice([1e-6, 1e-10]))
            max_iter = int(rng.choice([3, 100000, 100000]))
            ce = int(rng.choice([1, 64]))
            refused = bool(rng.random() < (0.5 if kind == "3n" or (adjoint and lam_valid) or tan_valid or atan_valid else 0.2))       # (about one in four over a group)
            yield ("cgstream", imgs, Ds, -1.0 if refused else Df, CL, CR, rtol, max_iter, ce)
            if not refused:
                kind, have_x, fill, after_stream = "2p", True, False, True
                lam_lost, lam_valid, adj_since = lam_lost or lam_valid, False, False
                dx_lost, dl_lost = tan_valid, atan_valid
                tan_rhs = tan_valid = atan_rhs = atan_valid = False
            refused_on_3n = refused and kind == "3n"
            refused_last = refused
        elif op == "prescaled":
            pre = 1 - pre
            yield ("tune", "prescaled", pre)
        elif op == "tune":
            what = rng.integers((9 if onchip else 5) + len(extra))      # (cg_onchip is drawn as often as the four blocked-pass keys together)
            if what >= (9 if onchip else 5):
                key, values = extra[what - (9 if onchip else 5)]
                if key == "cg keys":
                    yield ("tune", "cg_planes", int(rng.choice(CG_PLANES_DRAW)))
                    yield ("tune", "cg_fold", int(rng.choice(CG_FOLD_DRAW)))
                elif key == "prescaled":
                    pre = 1 - pre if rng.random() < 0.8 else pre
                    yield ("tune", "prescaled", pre)
                else:
                    v = int(rng.choice(values))
                    if key in tb_keys:
                        tb_keys[key] = v
                    if key == "cg_onchip_planes":
                        op_key = v
                    yield ("tune", key, v)
            elif what == 0:
                yield ("tune", "tb_T", int(rng.choice([0, 2, 4, 8])))
            elif what == 1:
                tb_keys["tb_impl"] = int(rng.choice([0, 1, 2]))
                yield ("tune", "tb_impl", tb_keys["tb_impl"])
            elif what == 2:
                tb_keys["tb_launch"] = int(rng.choice([0, 1]))
                yield ("tune", "tb_launch", tb_keys["tb_launch"])
            elif what == 3:
                yield ("tune", "flux_reduce", int(rng.choice([0, 1])))
            elif what == 4:
                kset = ["auto", "matfree_tb", "explicit", "matfree"][rng.integers(4)] if kind in ("2p", "3n") else "auto"
                yield ("kernel", kset)
            else:
                yield ("tune", "cg_onchip", int(rng.choice([0, 1, 1])))
        elif op == "init":
            yield ("init",)
            have_x = True
        elif op == "set_field":
            yield ("set_field", [rng.random((ny, nx)) for _ in range(B)])
            have_x = True
        elif op == "sweeps":
            k = int(rng.choice([1, 3, 8, 17, 40, 64]))
            omega, kern = [(2.0 / 3.0, 0), (1.0, 1)][rng.integers(2)]
            yield ("sweeps", k, omega, kern)
            pre_swept = pre_swept or bool(pre)
        elif op == "solve":
            tol = float(rng.choice(SOLVE_TOL))
            max_iter = int(rng.choice(SOLVE_MAX_ITER))
            ce = int(rng.choice(SOLVE_CE))
            # what reads the stack after the solve.  Images of a stack stop at different sweeps and stay frozen in the buffer
            # they stopped in until a reader consolidates them; deff_get_field is one such reader, and with "ptr" / "slot" the
            # other two take its place in some solves: deff_device_field (consolidates itself) and deff_get_slot_field of
            # every slot (reads each slot where it froze and leaves the stack as it is for the next call)
            readers = ["get"] + (["ptr"] if ptr else []) + (["slot"] if slot else [])
            if adjoint and lam_valid:                        # ... and deff_field_vjp_D, which consolidates itself
                readers += ["vjp"] * 8
            readers += (["trhs"] * 6 if tangent else []) + (["ff"] * 6 if fluxfield else [])       # ... and so do these two
            reader = readers[rng.integers(len(readers))] if len(readers) > 1 else "get"
            yield ("solve", tol, max_iter, ce, reader)
            tan_rhs = tan_rhs or reader == "trhs"
        elif op == "cg":
            rtol = float(rng.choice([1e-6, 1e-10]))
            max_iter = int(rng.choice([0, 3, 100000]))
            yield ("cg", rtol, max_iter, int(rng.choice([1, 64])))
            refused_last = kind == "Sw"
        elif op == "adj":
            rtol = float(rng.choice([1e-6, 1e-10]))
            max_iter = int(rng.choice([0, 3, 100000, 100000]))
            ce = int(rng.choice([1, 64]))
            w = [rng.standard_normal((ny, nx)) for _ in range(B)]
            if B >= 2 and rng.random() < 0.25:               # one image of the stack has nothing to solve
                w[int(rng.integers(B))][:] = 0.0
            yield ("adj", w, rtol, max_iter, ce)
            if kind == "Sw":
                refused_last = True                          # (an explicit-only system; lambda stays what it was)
            else:
                lam_valid, lam_lost, adj_since = True, False, True
                dl_lost, atan_rhs, atan_valid = atan_valid, False, False         # (a new lambda: dlambda was the old one's)
        elif op == "cgform":                                 # the keys of one of CG's three forms, set together
            # (on chip where the system surely has a dictionary; elsewhere the form that never needs one is likelier)
            forms = [0, 1, 1, 1, 2] if kind in ("2p", "3n") else [0, 1, 2, 2]
            if onchip_planes and op_key == 1:
                forms = forms + [2, 2, 2]                    # (towards the plane form, which the key moves on chip)
            form = int(rng.choice(forms))
            yield ("tune", "cg_onchip", 1 if form == 1 else 0)
            yield ("tune", "cg_planes", 2 if form == 2 else 0)
            yield ("tune", "cg_fold", int(rng.choice(CG_FOLD_DRAW)))
        elif op == "setadj":
            yield ("setadj", [rng.standard_normal((ny, nx)) for _ in range(B)])
            lam_valid, lam_lost = True, False
            dl_lost, atan_rhs, atan_valid = atan_valid, False, False
        elif op == "getadj":
            yield ("getadj",)
            lam_lost = False
        elif op == "vjp":
            # the model's planes, or a plane of the caller's with zero cells; the walls are drawn independently of the system's
            own = kind is None or bool(rng.random() < 1.0 / 3.0)
            CL, CR = ASSEMBLE_C[rng.integers(2)]
            D = None
            if own:
                Ds, Df, Dg = ASSEMBLE_D[rng.integers(3)]
                D = draw_D_planes(rng, nx, ny, B, Ds, Df, Dg)
                for plane in D:
                    plane[rng.random((ny, nx)) < 0.05] = 0.0
            yield ("vjp", D, CL, CR)
            lam_lost = False
        elif op == "sens":
            yield ("sens",)
            refused_last = kind in ("3n", "3g")              # (the form without D is refused for a Grid system, then D is given)
        elif op in ("trhs", "arhs", "hvp", "fhvp", "ff"):
            # the model's planes, or a plane of the caller's with zero cells; the direction: random (non-zero where D == 0 too),
            # or D itself; the walls are drawn independently of the system's (the right-hand side of dlambda has none)
            own = kind is None or bool(rng.random() < 1.0 / 3.0)
            D = None
            if own:
                Ds, Df, Dg = ASSEMBLE_D[rng.integers(3)]
                D = draw_D_planes(rng, nx, ny, B, Ds, Df, Dg)
                for plane in D:
                    plane[rng.random((ny, nx)) < 0.05] = 0.0
            # (None: the direction D itself -- never for "hvp": H D = 0, and the bar of its curv is relative to the sum itself)
            dD = None
            if op != "ff" and (rng.random() < 0.8 or op == "hvp"):
                dD = [rng.standard_normal((ny, nx)) for _ in range(B)]
            CL, CR = PASS_WALLS[rng.integers(3)] if op != "arhs" else (0.0, 0.0)
            yield (op, D, dD, CL, CR)
            if op == "trhs":
                tan_rhs = tan_rhs or have_x
            elif op == "arhs" and lam_valid:
                dl_lost, atan_rhs, atan_valid = False, True, False
            elif op == "hvp":
                refused_last = not (have_x and tan_valid) or CL == CR
                dx_lost = False
            elif op == "fhvp":
                refused_last = not (have_x and tan_valid and lam_valid and atan_valid)
                dx_lost = dl_lost = False
            elif op == "ff":
                refused_last = kind in ("3n", "3g")          # (the form without D; the one with D went through)
        elif op in ("tan", "atan"):
            rtol = float(rng.choice([1e-6, 1e-10]))
            max_iter = int(rng.choice([0, 3, 100000, 100000]))
            yield (op, rtol, max_iter, int(rng.choice([1, 64])))
            ok = kind not in (None, "Sw") and (tan_rhs if op == "tan" else atan_rhs)
            refused_last = not ok
            if ok and op == "tan":
                tan_valid = True
            elif ok:
                atan_valid = True
            dx_lost, dl_lost = dx_lost and op != "tan", dl_lost and op != "atan"
        elif op in ("settan", "setatan"):
            yield (op, [rng.standard_normal((ny, nx)) for _ in range(B)])
            if op == "settan":
                tan_valid, dx_lost = True, False
            else:
                atan_valid, dl_lost = True, False
        elif op in ("gettan", "getatan"):
            yield (op,)
        elif op == "opflip":
            op_key = 1 - op_key
            yield ("tune", "cg_onchip_planes", op_key)
        elif op == "stream":
            count = int(rng.integers(B, 3 * B + 2))
            imgs = draw_images(rng, nx, ny, count)
            Ds, Df, _ = ASSEMBLE_D[rng.integers(3)]
            CL, CR = ASSEMBLE_C[rng.integers(2)]
            tol = float(rng.choice(SOLVE_TOL))
            max_iter = int(rng.choice(SOLVE_MAX_ITER))
            yield ("stream", imgs, Ds, Df, CL, CR, tol, max_iter, int(rng.choice(SOLVE_CE)))
            if not (pre and kset == "explicit"):             # (refused before anything changes: no pre-scaled explicit sweeps)
                kind, have_x, fill, after_stream = "2p", True, False, True
                lam_lost, lam_valid, adj_since = lam_lost or lam_valid, False, False
                dx_lost, dl_lost = tan_valid, atan_valid
                tan_rhs = tan_valid = atan_rhs = atan_valid = False
        elif op == "slot":
            yield ("slot", int(rng.integers(B)))
        elif op == "stamps":
            omega, kern = [(2.0 / 3.0, 0), (1.0, 1)][rng.integers(2)]
            yield ("stamps", omega, kern)
        else:
            yield (op,)                                      # flux, get, residual, ptr: no arguments


def stream_schedule(iters, B, max_iter, check_every):
    """deff_solve_stream's bookkeeping on iteration counts alone (iters[i] = sweeps image i runs: oracle.jacobi's count).  All
    slots share the check points; a free slot takes the next image one sweep before a check; an image leaves at the check
    that stops it, or where it reaches max_iter between two checks.  Returns (slot of every image, the sweep count of the
    stream at which it retired, the stream's last sweep)."""
    n = len(iters)
    slot_of, retired = [None] * n, [None] * n
    live = {}                                                # slot -> [image, sweeps done]
    nxt = t = 0

    def refill():
        nonlocal nxt
        for k in range(B):
            if k not in live and nxt < n:
                live[k] = [nxt, 0]
                slot_of[nxt] = k
                nxt += 1

    def advance(nsw):
        nonlocal t
        t += nsw
        for k in list(live):
            live[k][1] += nsw

    def retire_done():
        for k in list(live):
            i, done = live[k]
            assert done <= iters[i]
            if done == iters[i]:
                retired[i] = t
                del live[k]

    refill()
    while live:
        advance(1)
        retire_done()                                        # the check
        left = check_every - 1
        while left > 0 and live:
            seg = min([left] + [max_iter - done for _, done in live.values()])
            if seg > 0:
                advance(seg)
                left -= seg
            retire_done()                                    # max_iter between two checks
        refill()
    return slot_of, retired, t


def device_rows(ptr, rows, pitch_bytes):
    """rows x (pitch_bytes / 8) doubles from a device pointer, copied by the HIP runtime the library itself runs on (the one
    already mapped into this process: a second copy of the runtime would not know the pointer)."""
    import ctypes as C
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
    assert path, "no HIP runtime mapped into this process"
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    assert pitch_bytes % 8 == 0
    out = np.full((rows, pitch_bytes // 8), np.nan)
    rc = hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2)     # hipMemcpyDeviceToHost
    assert rc == 0, rc
    return out


def expected_cg_impl(nx, ny, onchip_key):
    return 2 if onchip_key == 1 and (nx + (nx & 1)) * ny <= ONCHIP_LIMIT else 1


def tb_stamps(s, omega):
    """deff_debug_tb_stamps: the sizing call, then the stamping one.  -> (pairs of the sizing call, pairs of the real call,
    the words)."""
    import ctypes as C
    from effectivediffusivityfvm_amd import _capi
    L = _capi.load()
    n0 = C.c_int(-1)
    _capi.check(L.deff_debug_tb_stamps(s._ctx, omega, None, C.byref(n0)))
    buf = np.zeros(2 * n0.value, dtype=np.uint64)
    n1 = C.c_int(-1)
    _capi.check(L.deff_debug_tb_stamps(s._ctx, omega, buf.ctypes.data_as(C.c_void_p), C.byref(n1)))
    return n0.value, n1.value, buf


def run_sequence(pkg, ob, seed, with_cg=False, **options):
    draw = draw_sequence(seed, with_cg=with_cg, **options)
    _, nx, ny, B, use_fma = next(draw)
    flavour = "fma" if use_fma else None
    m = Model(ob, nx, ny, B, None)
    log = []
    onchip_key = planes_key = fold_key = pre_key = op_key = 0
    kernel_set = "auto"
    m.fill_fresh, m.fill_count = False, 0                    # the device fill: of the current image? / how many were computed
    sens_model = pre_model = None
    if options.get("sens"):
        import sensitivity_model as sens_model
    if options.get("prescaled"):
        import prescaled_model as pre_model
    adjoint = bool(options.get("adjoint"))
    if adjoint:
        import field_vjp_model as vjp_model
        from test_cg_host import decoupled_of
    # the adjoint's side of the model: lambda per image as the context last returned or took it, whether deff_amd.h's lifetime
    # rule says it is valid, and the device buffers of the last pass and of the last gradient as they read when they were made
    m.lam, m.lam_valid, m.vjp_dev, m.sens_dev = None, False, None, None
    # ... and the second-order side: dx and dlambda the same way, the two right-hand side maps as the model computed them (what
    # a twin solves from), whether each may serve as one, the device maps of the other passes, and "cg_onchip_planes"
    m.dx, m.tan_valid, m.r, m.tan_rhs = None, False, None, False
    m.dl, m.atan_valid, m.q, m.atan_rhs = None, False, None, False
    m.dev = {}
    if any(options.get(k) for k in ("tangent", "second", "fluxfield")):
        import field_hvp_model
        import flux_model
        import sens_hvp_model
        import tangent_model
        from test_gpu_field_hvp import CURV_MASS_BAR
        from test_gpu_sens_hvp import CURV_BAR
        from test_gpu_tangent import NORM2_BAR

    def distinct_rows():
        return len(np.unique(np.column_stack([np.concatenate(m.A), np.concatenate(m.b)]), axis=0))

    with pkg.Solver(nx, ny, nimg=B) as s:
        def prescaled_refused(call, own_system=False):
            """While "prescaled" is 1 a call that would sweep is refused for a system or a kernel setting without a pre-scaled
            form (deff_amd.h) -- decided from the model alone -- and changes nothing."""
            if not pre_key:
                return False
            refuse = kernel_set in ("explicit", "scalar") or (not own_system and (m.kind == "Sw" or distinct_rows() > 511))
            try:
                call()
            except pkg.DeffError as e:
                assert refuse and e.code == -1 and "prescaled" in str(e), (seed, log, e)
                log[-1] += " refused"
                if m.x is not None:
                    fields_equal()
                lam_unchanged()
                return True
            assert not refuse, (seed, log, "a pre-scaled call that should have been refused")
            assert s.plan_value("prescaled") == 1, (seed, log)
            return False

        def native_counters():
            assert (s.plan_value("fill_runs"), s.plan_value("fill_fallbacks"), s.plan_value("native3_rows")) == (m.fill_count, 0, 452), \
                (seed, log, s.plan_value("fill_runs"), m.fill_count, s.plan_value("fill_fallbacks"), s.plan_value("native3_rows"))

        def fields_equal():
            got = s.get_field()
            for k in range(B):
                assert np.array_equal(got[k * ny:(k + 1) * ny], m.x[k]), (seed, log, "field of image %d" % k)

        def device_field_equal():
            # the pointer is taken on a settled context and the context is settled again before the copy below, which runs on
            # the null stream: the context's stream does not wait for that one, and deff_device_field may have enqueued the
            # copies that bring frozen images of a stack into the current buffer
            s.synchronize()
            p, pitch = s.device_field_ptr()
            s.synchronize()
            assert pitch == 8 * (nx + (nx & 1)), (seed, log, pitch)
            got = device_rows(p, B * ny, pitch)
            for k in range(B):
                assert np.array_equal(got[k * ny:(k + 1) * ny, :nx], m.x[k]), (seed, log, "device field of image %d" % k)
            if nx & 1:                                       # the pad cell holds 0 and is not part of the mesh (deff_amd.h)
                assert np.array_equal(got[:, nx], np.zeros(B * ny)), (seed, log, "pad column", got[:, nx][got[:, nx] != 0][:4])

        def slot_field_equal(k):
            from effectivediffusivityfvm_amd import _capi
            x = np.empty((ny, nx))
            _capi.check(_capi.load().deff_get_slot_field(s._ctx, k, x))
            assert np.array_equal(x, m.x[k]), (seed, log, "field of slot %d" % k)

        def lam_unchanged():
            """After a call that must leave lambda alone (a refusal, the pass): deff_get_adjoint returns the same bits."""
            if adjoint and m.lam_valid:
                got = s.get_adjoint()
                for k in range(B):
                    assert np.array_equal(got[k * ny:(k + 1) * ny], m.lam[k]), (seed, log, "lambda of image %d" % k)
            # ... and so do deff_get_tangent and deff_get_adjoint_tangent, each while the model says it is valid
            for valid, vec, get, what in ((m.tan_valid, m.dx, s.get_tangent, "dx"), (m.atan_valid, m.dl, s.get_adjoint_tangent, "dlambda")):
                if valid:
                    got = get()
                    for k in range(B):
                        assert np.array_equal(got[k * ny:(k + 1) * ny], vec[k]), (seed, log, "%s of image %d" % (what, k))

        def maps_unchanged(vjp=True, sens=True, skip=()):
            """The device buffers of the last pass and of the last gradient read as they did when they were written -- and those
            of the tangent's right-hand side (which deff_device_tangent_rhs hands out even after an invalidation), of the two
            Hessian-vector passes and of the flux field."""
            if vjp and m.vjp_dev is not None:
                p, pitch = s.device_field_vjp_ptr()
                assert np.array_equal(device_rows(p, B * ny, pitch), m.vjp_dev), (seed, log, "the pass's device map")
            if sens and m.sens_dev is not None:
                p, pitch = s.device_sensitivity_ptr()
                assert np.array_equal(device_rows(p, B * ny, pitch), m.sens_dev), (seed, log, "the gradient's device map")
            for name, ptr in (("trhs", s.device_tangent_rhs_ptr), ("hvp", s.device_sens_hvp_ptr), ("fhvp", s.device_field_vjp_hvp_ptr)):
                if name not in skip and m.dev.get(name) is not None:
                    p, pitch = ptr()
                    assert np.array_equal(device_rows(p, B * ny, pitch), m.dev[name], equal_nan=True), (seed, log, "device map of " + name)
            if "ff" not in skip and m.dev.get("ff") is not None:
                px, py, pitch = s.device_flux_field_ptrs()
                for p, want, what in ((px, m.dev["ff"][0], "fx"), (py, m.dev["ff"][1], "fy")):
                    assert np.array_equal(device_rows(p, B * ny, pitch), want, equal_nan=True), (seed, log, "device map of " + what)

        def lam_invalidated():
            m.lam_valid, m.sens_dev = False, None            # (deff_device_sensitivity: "valid until ... an assembly")
            m.tan_rhs = m.tan_valid = m.atan_rhs = m.atan_valid = False

        def adjoint_refused(*calls):
            """While lambda is invalid (or no field exists, for the pass): DEFF_ESTATE, and nothing else changes."""
            for call in calls:
                with pytest.raises(pkg.DeffError) as e:
                    call()
                assert e.value.code == -5, (seed, log, e.value)
            log[-1] += " refused"
            if m.x is not None:
                fields_equal()
            maps_unchanged()
            lam_unchanged()

        def field_vjp_checked(D, CL, CR):
            """deff_field_vjp_D of the model's field and lambda against tests/field_vjp_model.py: host copy, device map, pad
            column, Euler sums (check_map's bar in test_gpu_field_vjp.py); the field, lambda and the gradient's map stay."""
            planes = m.D if D is None else D
            if not (m.lam_valid and m.x is not None):
                adjoint_refused(lambda: s.field_vjp(m.stacked(planes), CL, CR))
                return
            g, euler = s.field_vjp(m.stacked(planes), CL, CR)
            g, euler = g.reshape(B, ny, nx), np.atleast_1d(euler)
            p, pitch = s.device_field_vjp_ptr()
            assert pitch == 8 * (nx + (nx & 1)), (seed, log, pitch)
            dev = device_rows(p, B * ny, pitch)
            for k in range(B):
                want, want_euler = vjp_model.field_vjp(m.x[k], m.lam[k], planes[k], CL, CR)
                assert np.array_equal(g[k], want), (seed, log, "field vjp of image %d" % k, np.argwhere(g[k] != want)[:4].tolist())
                assert np.array_equal(dev[k * ny:(k + 1) * ny, :nx], want), (seed, log, "device map of the pass, image %d" % k)
                size = float(np.sum(np.abs(planes[k] * want)))
                assert euler[k] == float(want_euler) or abs(float(np.longdouble(euler[k]) - want_euler)) <= 1e-13 * size, \
                    (seed, log, k, euler[k], want_euler, size)
            if nx & 1:
                assert np.array_equal(dev[:, nx], np.zeros(B * ny)), (seed, log, "pad column of the pass's map")
            m.vjp_dev = dev
            maps_unchanged(vjp=False)
            fields_equal()
            lam_unchanged()

        # ---- the second-order calls ------------------------------------------------------------------------------------
        def refused(reasons, *calls):
            """Every call is refused for one of `reasons` -- (code, keyword of deff_amd.h's message); where the model knows of
            one reason only, that one -- and nothing changes: the field, every valid vector and every map read as before."""
            for call in calls:
                with pytest.raises(pkg.DeffError) as e:
                    call()
                assert any(e.value.code == code and word in str(e.value) for code, word in reasons), (seed, log, reasons, e.value)
            log[-1] += " refused"
            if m.x is not None:
                fields_equal()
            maps_unchanged()
            lam_unchanged()

        def side_impl():
            """deff_get_plan "cg_impl" after a solve on the coefficient planes (deff_amd.h, "cg_onchip_planes")."""
            return 4 if op_key == 1 and (nx + (nx & 1)) * ny <= ONCHIP_LIMIT else 3

        def map_checked(what, g, ptr, want):
            """The host copy and the device map of a pass equal the model's bit for bit; the pad column of an odd width is 0."""
            g = np.asarray(g).reshape(B, ny, nx)
            p, pitch = ptr()
            assert pitch == 8 * (nx + (nx & 1)), (seed, log, what, pitch)
            dev = device_rows(p, B * ny, pitch)
            for k in range(B):
                assert np.array_equal(g[k], want[k], equal_nan=True), (seed, log, "%s of image %d" % (what, k), np.argwhere(g[k] != want[k])[:4].tolist())
                assert np.array_equal(dev[k * ny:(k + 1) * ny, :nx], want[k], equal_nan=True), (seed, log, "device map of %s, image %d" % (what, k))
            if nx & 1:
                assert np.array_equal(dev[:, nx], np.zeros(B * ny)), (seed, log, "pad column of " + what)
            return dev

        def sum_checked(what, k, got, want, bar):
            """A per-image sum against the model's long-double one, within the bar of the pass's own directed test."""
            off = abs(float(np.longdouble(got) - want))
            print(f"seed {seed} {what} image {k}: {got!r}, off the model's by {off:.3e}, bar {bar:.3e}")
            assert got == float(want) or off <= bar, (seed, log, what, k, got, float(want), off, bar)

        def after_pass(name):
            maps_unchanged(skip=(name,))
            if m.x is not None:
                fields_equal()
            lam_unchanged()

        def planes_of(D, dD):
            planes = m.D if D is None else D
            return planes, (planes if dD is None else dD)

        def trhs_checked(D, dD, CL, CR):
            """deff_tangent_rhs_D of the model's field against tests/tangent_model.py; norm2 within check_map's bar in
            test_gpu_tangent.py.  The map becomes a right-hand side for the current system."""
            planes, dirs = planes_of(D, dD)
            call = lambda: s.tangent_rhs(m.stacked(planes), m.stacked(dirs), CL, CR)     # noqa: E731
            if m.x is None:
                return refused([(-5, "no field")], call)
            r, n2 = call()
            want = [tangent_model.tangent_rhs(m.x[k], planes[k], dirs[k], CL, CR) for k in range(B)]
            m.dev["trhs"] = map_checked("the tangent's right-hand side", r, s.device_tangent_rhs_ptr, [w[0] for w in want])
            for k in range(B):
                sum_checked("norm2 of r", k, np.atleast_1d(n2)[k], want[k][1], NORM2_BAR * abs(float(want[k][1])))
            m.r, m.tan_rhs = [w[0] for w in want], True
            after_pass("trhs")

        def arhs_checked(D, dD):
            """deff_adjoint_tangent_rhs_D: the tangent's model on lambda with both wall values 0; a new right-hand side makes
            dlambda invalid.  The map has no device getter: the twin of the next "atan" solves from the model's copy."""
            planes, dirs = planes_of(D, dD)
            call = lambda: s.adjoint_tangent_rhs(m.stacked(planes), m.stacked(dirs))     # noqa: E731
            if not m.lam_valid:
                return refused([(-5, "no adjoint field")], call)
            q, n2 = call()
            q = np.asarray(q).reshape(B, ny, nx)
            want = [tangent_model.tangent_rhs(m.lam[k], planes[k], dirs[k], 0.0, 0.0) for k in range(B)]
            for k in range(B):
                assert np.array_equal(q[k], want[k][0], equal_nan=True), (seed, log, "q of image %d" % k, np.argwhere(q[k] != want[k][0])[:4].tolist())
                sum_checked("norm2 of q", k, np.atleast_1d(n2)[k], want[k][1], NORM2_BAR * abs(float(want[k][1])))
            m.q, m.atan_rhs, m.atan_valid = [w[0] for w in want], True, False
            with pytest.raises(pkg.DeffError) as e:          # (dlambda belonged to the previous right-hand side)
                s.get_adjoint_tangent()
            assert e.value.code == -5, (seed, log, e.value)
            after_pass("arhs")

        def hvp_checked(D, dD, CL, CR):
            """deff_sensitivity_hvp_D of the model's field and dx against tests/sens_hvp_model.py; curv within check_map's bar in
            test_gpu_sens_hvp.py."""
            planes, dirs = planes_of(D, dD)
            call = lambda: s.sens_hvp(m.stacked(planes), m.stacked(dirs), CL, CR)        # noqa: E731
            reasons = ([(-1, "CR == CL")] if CL == CR else []) + ([(-5, "no field")] if m.x is None else []) + \
                ([(-5, "no tangent field")] if not m.tan_valid else [])
            if reasons:
                return refused(reasons, call)
            hv, cv = call()
            want = [sens_hvp_model.sens_hvp(m.x[k], m.dx[k], planes[k], dirs[k], CL, CR) for k in range(B)]
            m.dev["hvp"] = map_checked("the Deff Hessian-vector product", hv, s.device_sens_hvp_ptr, [w[0] for w in want])
            for k in range(B):
                sum_checked("curv", k, np.atleast_1d(cv)[k], want[k][1], CURV_BAR * abs(float(want[k][1])))
            after_pass("hvp")

        def fhvp_checked(D, dD, CL, CR):
            """deff_field_vjp_hvp_D of the model's field, lambda, dx and dlambda against tests/field_hvp_model.py; curv within
            check_map's bar in test_gpu_field_hvp.py.  A refusal names what is missing."""
            planes, dirs = planes_of(D, dD)
            call = lambda: s.field_vjp_hvp(m.stacked(planes), m.stacked(dirs), CL, CR)   # noqa: E731
            reasons = [(-5, word) for word, have in (("no field", m.x is not None), ("no adjoint field", m.lam_valid),
                                                     ("no tangent field", m.tan_valid), ("no adjoint tangent", m.atan_valid)) if not have]
            if reasons:
                return refused(reasons, call)
            hv, cv = call()
            want = [field_hvp_model.field_hvp(m.x[k], m.lam[k], m.dx[k], m.dl[k], planes[k], dirs[k], CL, CR) for k in range(B)]
            m.dev["fhvp"] = map_checked("the field Hessian-vector product", hv, s.device_field_vjp_hvp_ptr, [w[0] for w in want])
            for k in range(B):
                mass = float(np.sum(np.abs(np.where(planes[k] == 0.0, 0.0, dirs[k]) * want[k][0])))
                sum_checked("curv of S_w", k, np.atleast_1d(cv)[k], want[k][1], CURV_MASS_BAR * mass)
            after_pass("fhvp")

        def flux_maps_checked(ff, planes, CL, CR):
            kt = s.plan_value("flux_kt")
            want = [flux_model.flux_field(m.x[k], planes[k], CL, CR) for k in range(B)]
            px, py, pitch = s.device_flux_field_ptrs()
            devx = map_checked("fx", ff.fx, lambda: (px, pitch), [w[0] for w in want])
            devy = map_checked("fy", ff.fy, lambda: (py, pitch), [w[1] for w in want])
            for k in range(B):
                assert np.array_equal(ff.left[k], want[k][2], equal_nan=True), (seed, log, "left wall of image %d" % k)
                Q = flux_model.sections(want[k][0], want[k][2], ny, kt)
                assert np.array_equal(ff.sections[k], Q, equal_nan=True), (seed, log, "sections of image %d under flux_kt %d" % (k, kt),
                                                                           np.flatnonzero(ff.sections[k] != Q)[:4].tolist())
            m.dev["ff"] = (devx, devy)
            after_pass("ff")

        def ff_checked(D, CL, CR):
            """deff_flux_field_D against tests/flux_model.py (sections in the order of the "flux_kt" the plan reports), then
            deff_flux_field, whose outcome follows how the current system was assembled (deff_amd.h)."""
            planes = m.D if D is None else D
            with_D = lambda: s.flux_field(m.stacked(planes), CL, CR)                     # noqa: E731
            image_form = {"2p": [], "3p": [], "3n": [(-1, "Grid")], "3g": [(-1, "Grid")]}.get(m.kind, [(-5, "assembled from the image")])
            if m.x is None:
                refused([(-5, "no field")], with_D)
                return refused(image_form + [(-5, "no field")], s.flux_field)
            flux_maps_checked(with_D(), planes, CL, CR)
            if image_form:
                return refused(image_form, s.flux_field)
            flux_maps_checked(s.flux_field(), m.D, m.CL, m.CR)

        def vector_read(which):
            """deff_get_tangent + deff_device_tangent (deff_get_adjoint_tangent + deff_device_adjoint_tangent)."""
            valid, vec, get, ptr, word = (m.tan_valid, m.dx, s.get_tangent, s.device_tangent_ptr, "no tangent field") if which == "gettan" \
                else (m.atan_valid, m.dl, s.get_adjoint_tangent, s.device_adjoint_tangent_ptr, "no adjoint tangent")
            if not valid:
                return refused([(-5, word)], get, ptr)
            lam_unchanged()
            p, pitch = ptr()
            assert pitch == 8 * (nx + (nx & 1)), (seed, log, pitch)
            dev = device_rows(p, B * ny, pitch)
            for k in range(B):
                assert np.array_equal(dev[k * ny:(k + 1) * ny, :nx], vec[k]), (seed, log, "device %s of image %d" % (which[3:], k))
            if nx & 1:
                assert np.array_equal(dev[:, nx], np.zeros(B * ny)), (seed, log, "pad column of " + which[3:])

        def side_solve_checked(which, rtol, max_iter, ce):
            """deff_solve_tangent / deff_solve_adjoint_tangent: "deff_solve_adjoint with w = r, bit for bit" (deff_amd.h).  The
            twin is a fresh context of the same stack size that is given the model's system through deff_set_system, the same
            "cg_fold" and "cg_onchip_planes" and the OTHER check interval, and solves deff_solve_adjoint(w = the model's map)."""
            solve, rhs_ok, rhs, get = (s.solve_tangent, m.tan_rhs, m.r, s.get_tangent) if which == "tan" \
                else (s.solve_adjoint_tangent, m.atan_rhs, m.q, s.get_adjoint_tangent)
            call = lambda: solve(rtol=rtol, max_iter=max_iter, check_every=ce)           # noqa: E731
            # (after a new image the context has no system of its own; the header leaves open whether the old one's wall-column
            # links still speak: the draw asks for a solve there only where there is no right-hand side either)
            reasons = ([(-1, "wall column")] if m.kind == "Sw" else []) + ([(-5, "right-hand side")] if not rhs_ok else []) + \
                ([(-5, "no system"), (-1, "wall column")] if m.kind is None else [])
            if reasons:
                return refused(reasons, call)
            kernel_before = s.kernel_in_use()
            tb_before = {k: v for k, v in s.plan().items() if k.startswith("tb_")}
            res = call()
            res = [res] if B == 1 else res
            got = get()
            impl = side_impl()
            want_fold = 0 if impl == 4 else min(fold_key, 1)
            assert (s.plan_value("cg_impl"), s.plan_value("cg_fold")) == (impl, want_fold), (seed, log, op_key, fold_key, s.plan_value("cg_impl"))
            assert s.kernel_in_use() == kernel_before, (seed, log, kernel_before, s.kernel_in_use())
            assert {k: v for k, v in s.plan().items() if k.startswith("tb_")} == tb_before, (seed, log, tb_before)
            with pkg.Solver(nx, ny, nimg=B) as f:
                f.set_tuning("cg_fold", fold_key)
                f.set_tuning("cg_onchip_planes", op_key)
                f.set_system(m.stacked(m.A), m.stacked(m.b), m.stacked(m.D), m.CL, m.CR)
                twin = f.solve_adjoint(m.stacked(rhs), rtol=rtol, max_iter=max_iter, check_every=1 if ce == 64 else 64)
                twin = [twin] if B == 1 else twin
                assert (f.plan_value("cg_impl"), f.plan_value("cg_fold")) == (impl, want_fold), (seed, log, "the twin's form")
                lam_f = f.get_adjoint()
            mine = [(r.iters, r.rel_residual, r.converged) for r in res]
            assert mine == [(r.iters, r.rel_residual, r.converged) for r in twin], (seed, log, mine, [(r.iters, r.rel_residual) for r in twin])
            assert np.array_equal(got, lam_f, equal_nan=True), (seed, log, which + " against solve_adjoint of the map on a fresh context",
                                                                  np.argwhere(got != lam_f)[:4].tolist())
            vec = []
            for k in range(B):
                dec = decoupled_of(m.A[k], m.b[k]).reshape(ny, nx)
                v = got[k * ny:(k + 1) * ny].copy()
                assert np.all(v[dec] == 0.0) and res[k].deff_raw == 0.0, (seed, log, k)
                assert res[k].iters <= max_iter and res[k].converged == (res[k].rel_residual <= rtol), (seed, log, k, mine[k])
                if res[k].converged:                         # the bar of test_gpu_cg.py::assert_honest, as for "adj"
                    rn = residual_np(m.A[k], np.where(dec, 0.0, rhs[k]).ravel(), v, nx, ny)
                    assert rn <= rtol * (1 + 1e-6) + 1e-13, (seed, log, k, rn)
                vec.append(v)
            if which == "tan":
                m.dx, m.tan_valid = vec, True
            else:
                m.dl, m.atan_valid = vec, True
            log[-1] += " impl %d iters %s" % (impl, [r.iters for r in res])
            if m.x is not None:
                fields_equal()
            maps_unchanged()
            lam_unchanged()                                  # (the other two vectors stay)

        if use_fma:
            s.set_tuning("fma", 1)
            log.append("fma 1")
        m.pix = next(draw)[1]
        s.set_image(np.stack(m.pix))
        for op, *args in draw:
            if op == "image":
                m.pix, m.kind, m.fill_fresh = args[0], None, False
                lam_invalidated()
                s.set_image(np.stack(m.pix))
                log.append("image")
                maps_unchanged()                             # (every other map stays until its own next call)
            elif op == "assemble":
                kind, Ds, Df, Dg, CL, CR, D, *base = args
                m.assemble(kind, Ds, Df, Dg, CL, CR, D, *base)
                m.phases = (Ds, Df, Dg)
                lam_invalidated()
                log.append(f"assemble {kind} {Ds} {Df} {CL}")
                if kind == "2p":
                    s.assemble_2phase(Ds, Df, CL, CR)
                elif kind == "3p":
                    s.assemble_3phase(Ds, Df, Dg, CL, CR)
                elif kind == "3g":
                    s.assemble_3phase(Ds, Df, Dg, CL, CR, grid=m.stacked(m.grid))
                elif kind == "3n":
                    m.fill_count += 0 if m.fill_fresh else 1
                    m.fill_fresh = True
                    s.assemble_3phase_native(Ds, Df, Dg, CL, CR)
                    native_counters()
                elif kind in ("S", "Sw"):
                    s.set_kernel("auto")                     # as for a caller's D plane
                    kernel_set = "auto"
                    s.set_system(m.stacked(m.A), m.stacked(m.b), m.stacked(m.D), CL, CR)
                    log[-1] += " of " + base[0]
                else:
                    s.set_kernel("auto")                     # a caller's D plane: explicit planes, dictionary if it has few rows
                    kernel_set = "auto"
                    s.assemble_from_D(m.stacked(m.D), CL, CR)
                if kind != "3n" and options.get("native3"):
                    assert s.plan_value("native3_rows") == 0, (seed, log)
                maps_unchanged()
            elif op == "stage":
                Ds, Df, Dg, CL, CR = args
                assert m.kind == "3n" and m.fill_fresh
                log.append(f"stage {Ds} {Df} {Dg} {CL}")
                m.assemble("3n", Ds, Df, Dg, CL, CR)
                m.phases = (Ds, Df, Dg)
                lam_invalidated()
                s.assemble_3phase_native(Ds, Df, Dg, CL, CR)
                native_counters()
                maps_unchanged()
            elif op == "grid":
                log.append("grid")
                g, path = s.grid()
                for k in range(B):
                    want, flag = ob.floodfill((m.pix[k] > 200).astype(np.uint32))
                    assert np.array_equal(g[k * ny:(k + 1) * ny], want) and bool(path[k]) == flag, (seed, log, k)
            elif op == "getsys":
                log.append("getsys")
                A, b = s.get_system()
                assert np.array_equal(A, m.stacked(m.A)) and np.array_equal(b, m.stacked(m.b)), (seed, log)
            elif op == "tune":
                key, v = args
                s.set_tuning(key, v)
                if key == "cg_onchip":
                    onchip_key = v
                elif key == "cg_planes":
                    planes_key = v
                elif key == "cg_fold":
                    fold_key = v
                elif key == "prescaled":
                    pre_key = v
                elif key == "cg_onchip_planes":
                    op_key = v
                log.append(f"{key} {v}")
            elif op == "kernel":
                s.set_kernel(args[0]); log.append(f"kernel {args[0]}")
                kernel_set = args[0]
            elif op == "init":
                s.init_linear(m.CL, m.CR)
                m.x = [ob.linear_guess(nx, ny, m.CL, m.CR, flavour=flavour) for _ in range(B)]
                log.append("init")
            elif op == "set_field":
                m.x = args[0]
                s.set_field(m.stacked(m.x))
                log.append("set_field")
            elif op == "sweeps":
                k, omega, kern = args
                log.append(f"sweeps {k} {omega:.3f}")
                if pre_key:
                    if prescaled_refused(lambda: s.sweeps(k, omega)):
                        continue
                    m.x = [pre_model.sweeps(m.A[i], m.b[i], m.x[i], k, omega=omega) for i in range(B)]
                else:
                    s.sweeps(k, omega)
                    m.x = [ob.sweeps(m.A[i], m.b[i], m.x[i], k, kernel=kern, omega=omega, flavour=flavour) for i in range(B)]
                if m.kind == "Sw":
                    assert s.kernel_in_use() in ("explicit", "scalar"), (seed, log, s.kernel_in_use())
                fields_equal()
            elif op == "solve":
                tol, max_iter, ce, reader = args
                log.append(f"solve {tol} {max_iter} {ce}")
                got_res = []
                if pre_key:
                    if prescaled_refused(lambda: got_res.append(s.solve(tol, max_iter, check_every=ce))):
                        continue
                    res = got_res[0]
                else:
                    res = s.solve(tol, max_iter, check_every=ce)
                res = [res] if B == 1 else res
                if m.kind == "Sw":
                    assert s.kernel_in_use() in ("explicit", "scalar"), (seed, log, s.kernel_in_use())
                for i in range(B):
                    if pre_key:
                        it, deff, conv, x, MFL, MFR = pre_model.jacobi(m.A[i], m.b[i], m.x[i], m.D[i], m.CL, m.CR, tol, max_iter, check_every=ce)
                    else:
                        it, deff, conv, x, MFL, MFR = ob.jacobi(m.A[i], m.b[i], m.x[i], m.D[i], m.CL, m.CR, tol, max_iter, check_every=ce,
                                                                flavour=flavour)
                    assert (res[i].iters, res[i].deff_raw, res[i].conv) == (it, deff, conv), (seed, log, i)
                    m.x[i] = x
                if reader == "ptr":
                    log[-1] += " then ptr"
                    device_field_equal()
                elif reader == "slot":
                    log[-1] += " then slots"
                    for k in range(B):
                        slot_field_equal(k)
                elif reader == "vjp":                        # (the pass consolidates the frozen images itself)
                    log[-1] += " then vjp"
                    field_vjp_checked(None, m.CL, m.CR)
                elif reader == "trhs":                       # (and so do these two; the direction D: the forward residual)
                    log[-1] += " then trhs"
                    trhs_checked(None, None, m.CL, m.CR)
                elif reader == "ff":
                    log[-1] += " then ff"
                    ff_checked(None, m.CL, m.CR)
                else:
                    fields_equal()
            elif op == "cg":
                rtol, max_iter, ce = args
                log.append(f"cg {rtol} {max_iter} {ce}")
                before = m.stacked(m.x)
                try:
                    res = s.solve_cg(rtol=rtol, max_iter=max_iter, check_every=ce)
                except pkg.DeffError as e:
                    # the refusals these sequences can meet: three pixel classes or a D plane drawn cell by cell can give more
                    # distinct rows than a dictionary holds (LUT_MAX_ROWS = 512 with the zero row, lut_layout.hpp), and CG runs on
                    # the dictionary form unless "cg_planes" lets it read the planes; a caller's system with wall-column links
                    # is explicit-only whatever the key says; nothing is changed then
                    if m.kind == "Sw":
                        assert e.code == -1 and "explicit-only" in str(e), (seed, log, e)
                    else:
                        rows = distinct_rows()
                        assert e.code == -1 and "no row dictionary" in str(e) and rows > 511 and planes_key == 0, (seed, log, e, rows)
                    log[-1] += " refused"
                    fields_equal()
                    lam_unchanged()
                    continue
                assert m.kind != "Sw", (seed, log, "CG ran on an explicit-only system")
                has_dict = True
                if options.get("cgkeys"):
                    has_dict = distinct_rows() <= 511
                    assert has_dict or planes_key, (seed, log, "CG ran without a dictionary and without cg_planes")
                want_impl = 3 if planes_key == 2 or not has_dict else expected_cg_impl(nx, ny, onchip_key)
                if want_impl == 3:                           # the plane form: on chip under "cg_onchip_planes" where an image fits
                    want_impl = side_impl()
                if options.get("onchip"):
                    assert s.plan_value("cg_impl") == want_impl, (seed, log, onchip_key, planes_key)
                    log[-1] += " impl %d" % want_impl
                if options.get("cgkeys"):
                    # the fold that ran: the key on the streaming forms (on the planes 2 means 1, deff_amd.h), 0 on chip
                    want_fold = {1: fold_key, 2: 0, 3: min(fold_key, 1), 4: 0}[want_impl]
                    assert s.plan_value("cg_fold") == want_fold, (seed, log, fold_key, want_impl, s.plan_value("cg_fold"))
                    log[-1] += " fold %d" % want_fold
                res = [res] if B == 1 else res
                got = s.get_field()
                if options.get("onchip"):
                    # nothing of the context's history is in the result: a fresh context with the same system, the same field
                    # and the same form gives the same bits -- under the OTHER check interval, which the results do not depend
                    # on (deff_amd.h); the forms share cg_p[0], the per-image scalars and the restart flag between calls
                    # With "cgkeys" the fresh context also runs four launches per iteration (cg_fold 0) and, where the system
                    # has a dictionary, on the table (cg_planes 0): the same bits in both cases (deff_amd.h; the plane form has
                    # the work items and summation order of the STREAMING table form, so that is the form it is compared with).
                    # The plane form on chip ("cg_impl" 4): "a system that has a dictionary gives the bits of "cg_onchip" 1" -- the
                    # fresh context runs the table form on chip --, and one without has the same form to run on the planes.
                    fresh_onchip = 0 if want_impl == 3 else 1 if want_impl == 4 else onchip_key
                    fresh_impl = (4 if want_impl == 4 else 3) if not has_dict else expected_cg_impl(nx, ny, fresh_onchip)
                    with pkg.Solver(nx, ny, nimg=B) as f:
                        f.set_tuning("cg_onchip", fresh_onchip)
                        if want_impl == 4 and not has_dict:
                            f.set_tuning("cg_onchip_planes", 1)
                        f.set_tuning("cg_planes", 0 if has_dict else planes_key)
                        f.set_image(np.stack(m.pix))
                        if m.kind == "2p":
                            f.assemble_2phase(m.phases[0], m.phases[1], m.CL, m.CR)
                        elif m.kind == "3p":
                            f.assemble_3phase(*m.phases, m.CL, m.CR)
                        elif m.kind == "3g":
                            f.assemble_3phase(*m.phases, m.CL, m.CR, grid=m.stacked(m.grid))
                        elif m.kind == "3n":
                            f.assemble_3phase_native(*m.phases, m.CL, m.CR)
                        elif m.kind == "S":
                            f.set_system(m.stacked(m.A), m.stacked(m.b), m.stacked(m.D), m.CL, m.CR)
                        else:
                            f.assemble_from_D(m.stacked(m.D), m.CL, m.CR)
                        f.set_field(before)
                        res_f = f.solve_cg(rtol=rtol, max_iter=max_iter, check_every=1 if ce == 64 else 64)
                        res_f = [res_f] if B == 1 else res_f
                        assert (f.plan_value("cg_impl"), f.plan_value("cg_fold")) == (fresh_impl, 0), (seed, log)
                        assert [(r.iters, r.rel_residual, r.deff_raw) for r in res_f] == [(r.iters, r.rel_residual, r.deff_raw) for r in res], (seed, log)
                        assert np.array_equal(f.get_field(), got), (seed, log, "CG on a fresh context")
                        assert all(np.array_equal(u.MFL, v.MFL) and np.array_equal(u.MFR, v.MFR) for u, v in zip(res_f, res)), (seed, log)
                for i in range(B):
                    x = got[i * ny:(i + 1) * ny].copy()
                    rn = residual_np(m.A[i], m.b[i], x, nx, ny)
                    assert res[i].iters <= max_iter and res[i].converged == (res[i].rel_residual <= rtol), (seed, log, i)
                    if res[i].converged:                     # the additive term: test_gpu_cg.py::assert_honest
                        assert rn <= rtol * (1 + 1e-6) + 1e-13, (seed, log, i, rn)
                    elif rn == np.inf:                       # b = 0 (no pore reaches the right wall of a Grid system, CL = 0) and A x != 0
                        assert res[i].rel_residual == np.inf, (seed, log, i, res[i].rel_residual)
                    elif rn >= 1e-6:                         # two float64 evaluations of a residual far above their rounding
                        assert abs(res[i].rel_residual - rn) <= 1e-9 * rn, (seed, log, i, res[i].rel_residual, rn)
                    want, L, R = ob.flux_deff(x, m.D[i], m.CL, m.CR)
                    assert res[i].deff_raw == want and np.array_equal(res[i].MFL, L) and np.array_equal(res[i].MFR, R), (seed, log, i)
                    m.x[i] = x
            elif op == "flux":
                d, MFL, MFR = s.flux()
                d = [d] if B == 1 else list(d)
                for i in range(B):
                    want, L, R = ob.flux_deff(m.x[i], m.D[i], m.CL, m.CR)
                    assert d[i] == want and np.array_equal(MFL[i * ny:(i + 1) * ny], L) and np.array_equal(MFR[i * ny:(i + 1) * ny], R), (seed, log, i)
                log.append("flux")
            elif op == "get":
                fields_equal()
                log.append("get")
            elif op == "residual":
                got = s.residual() if m.kind in ("2p", "3p", "3n", "3g") else s.residual(m.stacked(m.D), m.CL, m.CR)
                got = [got] if B == 1 else list(got)
                log.append("residual")
                for i in range(B):
                    try:
                        ob.assert_residual(got[i], m.x[i], m.D[i], m.CL, m.CR)
                    except AssertionError as e:
                        raise AssertionError((seed, log, i, e.args))
            elif op == "stream":
                # the model step of deff_solve_stream: every image is a one-image run of the reference loop from the linear
                # guess, and afterwards slot k is an ordinary image of the stack -- the last one that ran there, the call's
                # 2-phase system, that image's final field (deff_amd.h)
                imgs, Ds, Df, CL, CR, tol, max_iter, ce = args
                log.append(f"stream {len(imgs)} {Ds} {Df} {CL} {tol} {max_iter} {ce}")
                if pre_key:
                    # (a stream brings its own 2-phase dictionary: only the kernel setting can stand in the way)
                    got_res = []
                    if prescaled_refused(lambda: got_res.append(s.solve_stream(imgs, Ds, Df, CL, CR, tol, max_iter, check_every=ce,
                                                                               want_fields=True)), own_system=True):
                        if options.get("native3"):
                            assert s.plan_value("native3_rows") == (452 if m.kind == "3n" else 0), (seed, log)
                        continue
                    res = got_res[0]
                else:
                    res = s.solve_stream(imgs, Ds, Df, CL, CR, tol, max_iter, check_every=ce, want_fields=True)
                m.fill_fresh = False
                lam_invalidated()
                assert len(res) == len(imgs)
                want = []
                for i, pix in enumerate(imgs):
                    D = ob.fill_D_2phase(pix, Df, Ds)
                    A, b = ob.discretize(D, CL, CR)
                    if pre_key:
                        it, deff, conv, x, _, _ = pre_model.jacobi(A, b, ob.linear_guess(nx, ny, CL, CR), D, CL, CR, tol, max_iter, check_every=ce)
                    else:
                        it, deff, conv, x, _, _ = ob.jacobi(A, b, ob.linear_guess(nx, ny, CL, CR, flavour=flavour), D, CL, CR, tol, max_iter,
                                                            check_every=ce, flavour=flavour)
                    assert (res[i].iters, res[i].deff_raw, res[i].conv) == (it, deff, conv), (seed, log, i)
                    assert np.array_equal(res[i].field, x), (seed, log, "stream image %d" % i)
                    want.append((D, A, b, x))
                slot_of, retired, end = stream_schedule([r.iters for r in res], B, max_iter, ce)
                assert [r.slot for r in res] == slot_of, (seed, log, [r.slot for r in res], slot_of)
                last = {k: i for i, k in enumerate(slot_of)}                     # the last image of every slot
                assert sorted(last) == list(range(B))
                log[-1] += " early %s" % [k for k in range(B) if retired[last[k]] < end]
                m.pix = [imgs[last[k]] for k in range(B)]
                m.D, m.A, m.b = ([want[last[k]][j] for k in range(B)] for j in range(3))
                m.x = [want[last[k]][3] for k in range(B)]
                m.CL, m.CR, m.kind, m.phases = CL, CR, "2p", (Ds, Df, None)
                fields_equal()
                maps_unchanged()
            elif op == "sens":
                # the Deff gradient of the current field: it uses the upload scratch and events of its own and changes nothing
                # else -- the closing fields_equal() and every later op show that
                log.append("sens")
                if m.kind in ("3n", "3g"):                   # a Grid system's Deff is no function of the phase diffusivities alone
                    with pytest.raises(pkg.DeffError) as e:
                        s.sensitivity()
                    assert e.value.code == -1 and "Grid" in str(e.value), (seed, log, e.value)
                    lam_unchanged()
                g, euler = s.sensitivity() if m.kind in ("2p", "3p") else s.sensitivity(m.stacked(m.D), m.CL, m.CR)
                g, euler = g.reshape(B, ny, nx), np.atleast_1d(euler)
                p, pitch = s.device_sensitivity_ptr()
                assert pitch == 8 * (nx + (nx & 1)), (seed, log, pitch)
                dev = device_rows(p, B * ny, pitch)
                for k in range(B):
                    want, want_euler = sens_model.sensitivity(m.x[k], m.D[k], m.CL, m.CR)
                    assert np.array_equal(g[k], want), (seed, log, "sensitivity of image %d" % k)
                    # (a field that CG blew up on a system with b = 0 overflows both sums alike: inf - inf is no distance)
                    assert euler[k] == float(want_euler) or \
                        abs(float(np.longdouble(euler[k]) - want_euler)) <= 1e-13 * abs(float(want_euler)), (seed, log, k, euler[k], want_euler)
                    assert np.array_equal(dev[k * ny:(k + 1) * ny, :nx], want), (seed, log, "device map of image %d" % k)
                if nx & 1:
                    assert np.array_equal(dev[:, nx], np.zeros(B * ny)), (seed, log, "pad column of the map")
                m.sens_dev = dev
                maps_unchanged(sens=False)                   # (the gradient writes its own map, not the pass's)
            elif op == "cgstream":
                # deff_solve_cg_stream: every image is solved from the linear guess "exactly as a one-image deff_solve_cg call
                # would" (deff_amd.h) -- compared with that call on a fresh one-image context under the same cg_onchip key --
                # and afterwards slot k is an ordinary image of the stack: the last image reported there, the call's 2-phase
                # system, that image's field.  A refused call (Df = -1: no admissible table) changes nothing at all.
                imgs, Ds, Df, CL, CR, rtol, max_iter, ce = args
                log.append(f"cgstream {len(imgs)} {Ds} {Df} {CL} {rtol} {max_iter} {ce}")
                if Df < 0:
                    with pytest.raises(pkg.DeffError) as e:
                        s.solve_cg_stream(imgs, Ds, Df, CL, CR, rtol=rtol, max_iter=max_iter, check_every=ce, want_fields=True)
                    assert e.value.code == -1 and "admissible" in str(e.value), (seed, log, e.value)
                    log[-1] += " refused"
                    if options.get("native3"):
                        assert s.plan_value("native3_rows") == (452 if m.kind == "3n" else 0), (seed, log)
                        if m.fill_fresh:
                            assert s.plan_value("fill_runs") == m.fill_count, (seed, log)
                    if m.x is not None:
                        fields_equal()
                    lam_unchanged()
                    continue
                res = s.solve_cg_stream(imgs, Ds, Df, CL, CR, rtol=rtol, max_iter=max_iter, check_every=ce, want_fields=True)
                m.fill_fresh = False
                lam_invalidated()
                assert len(res) == len(imgs)
                assert [r.slot for r in res[:B]] == list(range(B)) and all(0 <= r.slot < B for r in res), (seed, log, [r.slot for r in res])
                want = []
                with pkg.Solver(nx, ny) as f:
                    f.set_tuning("cg_onchip", onchip_key)
                    for i, pix in enumerate(imgs):
                        D = ob.fill_D_2phase(pix, Df, Ds)
                        A, b = ob.discretize(D, CL, CR)
                        x = res[i].field
                        rn = residual_np(A, b, x, nx, ny)
                        assert res[i].iters <= max_iter and res[i].converged == (res[i].rel_residual <= rtol), (seed, log, i)
                        if res[i].converged:
                            assert rn <= rtol * (1 + 1e-6) + 1e-13, (seed, log, i, rn)
                        elif rn >= 1e-6:
                            assert abs(res[i].rel_residual - rn) <= 1e-9 * rn, (seed, log, i, res[i].rel_residual, rn)
                        assert res[i].deff_raw == ob.flux_deff(x, D, CL, CR)[0], (seed, log, i)
                        f.set_image(pix)
                        f.assemble_2phase(Ds, Df, CL, CR)
                        f.init_linear(CL, CR)
                        one = f.solve_cg(rtol=rtol, max_iter=max_iter, check_every=ce)
                        assert (one.iters, one.rel_residual, one.deff_raw) == (res[i].iters, res[i].rel_residual, res[i].deff_raw), (seed, log, i)
                        assert np.array_equal(f.get_field(), x), (seed, log, "cgstream image %d against a one-image solve_cg" % i)
                        want.append((D, A, b, x))
                last = {r.slot: i for i, r in enumerate(res)}                    # the last image of every slot
                assert sorted(last) == list(range(B))
                m.pix = [imgs[last[k]] for k in range(B)]
                m.D, m.A, m.b = ([want[last[k]][j] for k in range(B)] for j in range(3))
                m.x = [want[last[k]][3] for k in range(B)]
                m.CL, m.CR, m.kind, m.phases = CL, CR, "2p", (Ds, Df, None)
                fields_equal()
                maps_unchanged()
            elif op == "adj":
                # deff_solve_adjoint: every image against a twin -- a fresh one-image context that is given the image's matrix
                # with w' (w zeroed where the FORWARD system decouples the cell) as its right-hand side and solves it as a
                # forward system on the planes from a zero field, unfolded, under the OTHER check interval (deff_amd.h: "the
                # same work items, recurrence and summation order", "results independent of check_every").  The field, the
                # kernel in use and the Jacobi plan stay; refused on wall-column links, lambda then stays what it was.
                w, rtol, max_iter, ce = args
                log.append(f"adj {rtol} {max_iter} {ce}")
                kernel_before = s.kernel_in_use()
                tb_before = {k: v for k, v in s.plan().items() if k.startswith("tb_")}
                if m.kind == "Sw":
                    with pytest.raises(pkg.DeffError) as e:
                        s.solve_adjoint(m.stacked(w), rtol=rtol, max_iter=max_iter, check_every=ce)
                    assert e.value.code == -1 and "wall column" in str(e.value), (seed, log, e.value)
                    log[-1] += " refused"
                    if m.x is not None:
                        fields_equal()
                    lam_unchanged()
                    continue
                res = s.solve_adjoint(m.stacked(w), rtol=rtol, max_iter=max_iter, check_every=ce)
                res = [res] if B == 1 else res
                lam = s.get_adjoint()
                want_fold = 0 if side_impl() == 4 else min(fold_key, 1)
                assert (s.plan_value("cg_impl"), s.plan_value("cg_fold")) == (side_impl(), want_fold), (seed, log, fold_key, op_key)
                assert s.kernel_in_use() == kernel_before, (seed, log, kernel_before, s.kernel_in_use())
                assert {k: v for k, v in s.plan().items() if k.startswith("tb_")} == tb_before, (seed, log, tb_before)
                m.lam = []
                for k in range(B):
                    dec = decoupled_of(m.A[k], m.b[k]).reshape(ny, nx)
                    wp = np.where(dec, 0.0, w[k])
                    lk = lam[k * ny:(k + 1) * ny].copy()
                    got = (res[k].iters, res[k].rel_residual, res[k].converged)
                    assert np.all(lk[dec] == 0.0) and res[k].deff_raw == 0.0, (seed, log, k)
                    if not wp.any():
                        log[-1] += " zero %d" % k
                        assert got == (0, 0.0, True) and not lk.any(), (seed, log, k, got)
                    with pkg.Solver(nx, ny) as f:
                        f.set_tuning("cg_planes", 2)
                        f.set_tuning("cg_fold", 0)
                        f.set_tuning("cg_onchip_planes", op_key)
                        f.set_system(m.A[k], wp.ravel(), m.D[k], m.CL, m.CR)
                        f.set_field(np.zeros((ny, nx)))
                        one = f.solve_cg(rtol=rtol, max_iter=max_iter, check_every=1 if ce == 64 else 64)
                        assert f.plan_value("cg_impl") == side_impl() and f.plan_value("cg_fold") == 0, (seed, log)
                        assert (one.iters, one.rel_residual, one.converged) == got, (seed, log, k, got, (one.iters, one.rel_residual, one.converged))
                        assert np.array_equal(f.get_field(), lk), (seed, log, "lambda of image %d against its twin" % k)
                    assert res[k].iters <= max_iter and res[k].converged == (res[k].rel_residual <= rtol), (seed, log, k, got)
                    if res[k].converged:                     # the bar of test_gpu_cg.py::assert_honest, as for "cg"
                        rn = residual_np(m.A[k], wp.ravel(), lk, nx, ny)
                        assert rn <= rtol * (1 + 1e-6) + 1e-13, (seed, log, k, rn)
                    m.lam.append(lk)
                m.lam_valid = True
                m.atan_rhs = m.atan_valid = False            # (a new lambda: dlambda and its right-hand side were the old one's)
                log[-1] += " iters %s" % [r.iters for r in res]
                if m.x is not None:
                    fields_equal()
                lam_unchanged()                              # (dx stays)
            elif op == "setadj":
                log.append("setadj")
                m.lam, m.lam_valid = args[0], True
                m.atan_rhs = m.atan_valid = False
                s.set_adjoint(m.stacked(m.lam))
            elif op in ("trhs", "arhs", "hvp", "fhvp", "ff"):
                D, dD, CL, CR = args
                log.append(f"{op} {'D' if D is not None else 'model'} {'dD' if dD is not None else 'D'} {CL} {CR}")
                if op == "trhs":
                    trhs_checked(D, dD, CL, CR)
                elif op == "arhs":
                    arhs_checked(D, dD)
                elif op == "hvp":
                    hvp_checked(D, dD, CL, CR)
                elif op == "fhvp":
                    fhvp_checked(D, dD, CL, CR)
                else:
                    ff_checked(D, CL, CR)
            elif op in ("tan", "atan"):
                log.append(f"{op} {args[0]} {args[1]} {args[2]}")
                side_solve_checked(op, *args)
            elif op in ("settan", "setatan"):                # the model adopts the caller's plane, as for "setadj"
                log.append(op)
                if op == "settan":
                    m.dx, m.tan_valid = args[0], True
                    s.set_tangent(m.stacked(m.dx))
                else:
                    m.dl, m.atan_valid = args[0], True
                    s.set_adjoint_tangent(m.stacked(m.dl))
                lam_unchanged()
            elif op in ("gettan", "getatan"):
                log.append(op)
                vector_read(op)
            elif op == "ffptr":
                log.append("ffptr")
                if m.dev.get("ff") is None:
                    refused([(-5, "no flux field")], s.device_flux_field_ptrs)
                else:
                    maps_unchanged()
            elif op == "getadj":
                log.append("getadj")
                if not m.lam_valid:
                    adjoint_refused(s.get_adjoint, s.device_adjoint_ptr)
                    continue
                lam_unchanged()
                p, pitch = s.device_adjoint_ptr()
                assert pitch == 8 * (nx + (nx & 1)), (seed, log, pitch)
                dev = device_rows(p, B * ny, pitch)
                for k in range(B):
                    assert np.array_equal(dev[k * ny:(k + 1) * ny, :nx], m.lam[k]), (seed, log, "device lambda of image %d" % k)
                if nx & 1:
                    assert np.array_equal(dev[:, nx], np.zeros(B * ny)), (seed, log, "pad column of lambda")
            elif op == "vjp":
                D, CL, CR = args
                log.append(f"vjp {'D' if D is not None else 'model'} {CL} {CR}")
                field_vjp_checked(D, CL, CR)
            elif op == "ptr":
                log.append("ptr")
                device_field_equal()
            elif op == "slot":
                log.append(f"slot {args[0]}")
                slot_field_equal(args[0])
            elif op == "stamps":
                omega, kern = args
                log.append(f"stamps {omega:.3f}")
                try:
                    n0, n1, words = tb_stamps(s, omega)
                except pkg.DeffError as e:
                    assert e.code == -5 and "not on the temporally blocked kernel" in str(e), (seed, log, e)
                    assert s.kernel_in_use() != "matfree_tb", (seed, log)
                    log[-1] += " refused"
                    fields_equal()
                    continue
                assert s.kernel_in_use() == "matfree_tb", (seed, log)
                p = s.plan()
                resident = p["tb_impl"] == 2 and p["tb_resident"] == 1
                # where a tile's first clock lies: streaming form 2 words per wave tile; workgroup tiles T + 4 words per tile,
                # resident ones 12 (the last pair may be half padding)
                per = 2 if p["tb_impl"] == 1 else 12 if resident else p["tb_T"] + 4
                starts = words[:len(words) // per * per:per]
                assert n0 == n1 and n0 > 0 and len(starts) > 0 and np.all(starts != 0), (seed, log, n0, n1, p, np.flatnonzero(starts == 0)[:8])
                nsw = p["tb_T"] * (3 if resident else 1)
                log[-1] += f" T {p['tb_T']} sweeps {nsw}"
                m.x = [ob.sweeps(m.A[i], m.b[i], m.x[i], nsw, kernel=kern, omega=omega, flavour=flavour) for i in range(B)]
                fields_equal()
            else:
                raise AssertionError(op)
        if m.x is not None:
            fields_equal()
        assert s.plan_value("tb_fallbacks") == 0
    return log


@pytest.mark.parametrize("seed", range(40))
def test_random_call_sequences_match_the_oracle(pkg, oracle, seed):
    run_sequence(pkg, oracle, 1000 + seed)


@pytest.mark.parametrize("seed", range(24))
def test_random_call_sequences_with_cg(pkg, oracle, seed):
    run_sequence(pkg, oracle, 2000 + seed, with_cg=True)


# The rest of the ABI, each group of options on its own seeds (tests/test_sequences_host.py counts what these seeds reach).
# Shapes of the on-chip seeds: most fit one compute unit (row pitch x ny <= 16 384: an odd width, and 128 x 128 exactly at the
# limit), (130, 128) and (256, 130) do not and keep the streaming kernels whatever the key says.
ONCHIP_SHAPES = [(64, 48), (97, 41), (128, 128), (40, 300), (130, 70), (33, 21), (130, 128), (256, 130)]
ABI_SHAPES = [(64, 48), (130, 70), (97, 41), (256, 130), (40, 300), (129, 200)]
ONCHIP_SEEDS = dict(first=3000, count=48, with_cg=True, shapes=ONCHIP_SHAPES, steps=40, onchip=True)
STREAM_SEEDS = dict(first=4000, count=48, shapes=ABI_SHAPES, stacks=(2, 3, 4), stream=True, ptr=True, slot=True, stamps=True)
FMA_SEEDS = dict(first=6000, count=24, shapes=ABI_SHAPES, stacks=(1, 2, 3), stream=True, ptr=True, slot=True, stamps=True, fma=True)
# ... and what came after those: the native 3-phase assembly and its fill, a caller's system, the Deff gradient; the CG keys and
# the CG stream; the pre-scaled sweeps.  Their shapes add the even width (64, 24) of the directed tests above: a wall-column
# link can be represented there.  On every shape one workgroup holds an image's fill bitmaps ("fill_impl" 1 is never refused:
# test_sequences_host.py checks the rule of api_fill.hip).
NATIVE_SHAPES = ABI_SHAPES + [(64, 24)]
CGKEY_SHAPES = ONCHIP_SHAPES + [(64, 24)]
NATIVE_SEEDS = dict(first=7000, count=40, shapes=NATIVE_SHAPES, stacks=(1, 2, 3), steps=40, native3=True, system=True, sens=True,
                    ptr=True, slot=True, stream=True)
CGKEY_SEEDS = dict(first=8000, count=40, with_cg=True, shapes=CGKEY_SHAPES, stacks=(1, 2, 2, 3), steps=40, onchip=True, cgkeys=True,
                   cgstream=True, native3=True, system=True)
PRESCALED_SEEDS = dict(first=9000, count=40, shapes=NATIVE_SHAPES, stacks=(1, 2, 3), steps=40, prescaled=True, native3=True,
                       system=True, stream=True)
# ... and the field adjoint, among everything it shares buffers, planes built on demand, scratch and plan keys with: the three CG
# forms and the CG stream, native and caller's systems, the gradient (whose tune draws lead to resident tiles), streams and
# the readers of frozen images.
ADJOINT_SEEDS = dict(first=10000, count=40, with_cg=True, shapes=CGKEY_SHAPES, stacks=(1, 2, 2, 3), steps=40, onchip=True, cgkeys=True,
                     cgstream=True, native3=True, system=True, sens=True, stream=True, ptr=True, slot=True, adjoint=True)

# ... and the second-order calls -- the field tangent, the two Hessian-vector products, the on-chip plane form of the side solves
# and the flux field -- among everything the adjoint's group has: five validity flags, one upload scratch of two planes and one
# set of CG work vectors are shared by all of it.
SECOND_ORDER_SEEDS = dict(first=11000, count=48, with_cg=True, shapes=CGKEY_SHAPES, stacks=(1, 2, 2, 3), steps=40, onchip=True,
                          cgkeys=True, cgstream=True, native3=True, system=True, sens=True, stream=True, ptr=True, slot=True,
                          adjoint=True, tangent=True, second=True, fluxfield=True, onchip_planes=True)


def seed_options(group):
    return {k: v for k, v in group.items() if k not in ("first", "count")}


@pytest.mark.parametrize("seed", range(NATIVE_SEEDS["count"]))
def test_random_call_sequences_with_native_3phase_systems_and_sensitivities(pkg, oracle, seed):
    run_sequence(pkg, oracle, NATIVE_SEEDS["first"] + seed, **seed_options(NATIVE_SEEDS))


@pytest.mark.parametrize("seed", range(CGKEY_SEEDS["count"]))
def test_random_call_sequences_with_cg_keys_and_cg_streams(pkg, oracle, seed):
    run_sequence(pkg, oracle, CGKEY_SEEDS["first"] + seed, **seed_options(CGKEY_SEEDS))


@pytest.mark.parametrize("seed", range(PRESCALED_SEEDS["count"]))
def test_random_call_sequences_with_prescaled_sweeps(pkg, oracle, seed):
    run_sequence(pkg, oracle, PRESCALED_SEEDS["first"] + seed, **seed_options(PRESCALED_SEEDS))


@pytest.mark.parametrize("seed", range(ADJOINT_SEEDS["count"]))
def test_random_call_sequences_with_the_field_adjoint(pkg, oracle, seed):
    run_sequence(pkg, oracle, ADJOINT_SEEDS["first"] + seed, **seed_options(ADJOINT_SEEDS))


@pytest.mark.parametrize("seed", range(SECOND_ORDER_SEEDS["count"]))
def test_random_call_sequences_with_tangents_hessian_products_and_the_flux_field(pkg, oracle, seed):
    run_sequence(pkg, oracle, SECOND_ORDER_SEEDS["first"] + seed, **seed_options(SECOND_ORDER_SEEDS))


@pytest.mark.parametrize("seed", range(ONCHIP_SEEDS["count"]))
def test_random_call_sequences_with_both_cg_forms(pkg, oracle, seed):
    run_sequence(pkg, oracle, ONCHIP_SEEDS["first"] + seed, **seed_options(ONCHIP_SEEDS))


@pytest.mark.parametrize("seed", range(STREAM_SEEDS["count"]))
def test_random_call_sequences_with_streams_pointers_slots_and_stamps(pkg, oracle, seed):
    run_sequence(pkg, oracle, STREAM_SEEDS["first"] + seed, **seed_options(STREAM_SEEDS))


@pytest.mark.parametrize("seed", range(FMA_SEEDS["count"]))
def test_random_call_sequences_with_contracted_arithmetic(pkg, oracle, seed):
    run_sequence(pkg, oracle, FMA_SEEDS["first"] + seed, **seed_options(FMA_SEEDS))


def test_cg_ignores_the_fma_key(pkg, oracle):
    """api_cg.hip: "the fma knob does not apply here".  Both CG forms on a context with fma = 1 give the bits of one with
    fma = 0 -- iterations, residual, Deff, wall fluxes and field -- from the same caller's field (the linear guess itself is
    the one thing the key changes before a CG call, so it is not used here)."""
    nx, ny = 97, 41
    pix = oracle.synth_mask(nx, ny, 777, 0)
    x0 = np.random.default_rng(5).random((ny, nx))
    for onchip_key in (0, 1):
        got = []
        for fma in (0, 1):
            with pkg.Solver(nx, ny) as s:
                s.set_tuning("fma", fma)
                s.set_tuning("cg_onchip", onchip_key)
                s.set_image(pix)
                s.assemble_2phase(1e-3, 1.0, 0.0, 1.0)
                s.set_field(x0)
                r = s.solve_cg(rtol=1e-10, max_iter=100000)
                assert r.converged and s.plan_value("cg_impl") == 1 + onchip_key
                got.append((r.iters, r.rel_residual, r.deff_raw, r.MFL.copy(), r.MFR.copy(), s.get_field()))
        a, b = got
        assert a[:3] == b[:3] and all(np.array_equal(u, v) for u, v in zip(a[3:], b[3:])), (onchip_key, a[:3], b[:3])


def wrap_system(ob, pix, Ds, Df, CL, CR):
    """The oracle's 2-phase system of `pix` with a W link in column 0 of every row but the first (it reads the previous row's
    last cell: test_gpu_parity.py::test_wall_column_links_keep_linear_addressing) -> (A, b, D)."""
    ny, nx = pix.shape
    D = ob.fill_D_2phase(pix, Df, Ds)
    A, b = ob.discretize(D, CL, CR)
    A = A.copy().reshape(ny, nx, 5)
    A[1:, 0, 1] = -0.125
    return A.reshape(-1, 5), b, D


@pytest.mark.parametrize("assembly", ["assemble_2phase", "solve_stream"])
def test_a_native_assembly_forgets_the_wrap_links_of_a_callers_system(pkg, oracle, assembly):
    """deff_set_system marks a system whose A links a wall column to the neighbouring row as explicit-only, and deff_solve_cg
    refuses such a system.  The mark belongs to that system: after set_image + assemble_2phase (or a deff_solve_stream) the
    context holds the native 2-phase system, and CG on it gives the bits of a context that never saw the caller's A."""
    nx, ny = 64, 24
    B = 1 if assembly == "assemble_2phase" else 2
    rng = np.random.default_rng(64024)
    pix = [np.where(rng.random((ny, nx)) < 0.5, 0, 255).astype(np.uint8) for _ in range(B)]
    x0 = [rng.random((ny, nx)) for _ in range(B)]
    wrapped = [wrap_system(oracle, p, 1e-2, 1.0, 0.0, 1.0) for p in pix]

    def native(s):
        if assembly == "assemble_2phase":
            s.set_image(np.stack(pix))
            s.assemble_2phase(1e-2, 1.0, 0.0, 1.0)
        else:
            res = s.solve_stream(pix, 1e-2, 1.0, 0.0, 1.0, 1e-2, 7, check_every=7)
            assert [r.slot for r in res] == [0, 1]
        s.init_linear(0.0, 1.0)
        r = s.solve_cg(rtol=1e-10)
        r = r if isinstance(r, list) else [r]
        assert all(q.converged for q in r)
        return [(q.iters, q.rel_residual, q.deff_raw) for q in r], s.get_field()

    with pkg.Solver(nx, ny, nimg=B) as s:
        s.set_system(np.concatenate([w[0] for w in wrapped]), np.concatenate([w[1] for w in wrapped]),
                     np.concatenate([w[2] for w in wrapped]), 0.0, 1.0)
        s.set_field(np.concatenate(x0))
        s.sweeps(3)
        assert s.kernel_in_use() in ("explicit", "scalar")
        got = s.get_field()
        for k in range(B):
            assert np.array_equal(got[k * ny:(k + 1) * ny], oracle.sweeps(wrapped[k][0], wrapped[k][1], x0[k], 3)), k
        with pytest.raises(pkg.DeffError) as e:              # the caller's system itself stays refused
            s.solve_cg(rtol=1e-10)
        assert e.value.code == -1 and "explicit-only" in str(e.value)
        after = native(s)
    with pkg.Solver(nx, ny, nimg=B) as f:
        fresh = native(f)
    assert after[0] == fresh[0], (after[0], fresh[0])
    assert np.array_equal(after[1], fresh[1])


def test_a_refused_cg_stream_leaves_a_native_3phase_system_alone(pkg, oracle):
    """deff_solve_cg_stream validates its table and its image shape before it changes anything: after a refusal (an
    inadmissible Df, images that do not match the mesh) the context still holds the native 3-phase system -- its 452 rows,
    the planes built on demand from the fill, the refusal of deff_sensitivity for a Grid system -- and its field."""
    import ctypes as C
    from effectivediffusivityfvm_amd import _capi
    nx, ny, B = 64, 24, 2
    rng = np.random.default_rng(3452)
    pix = []
    for k in range(B):
        f = rng.random((ny, nx))
        p = np.where(f < 0.3, 255, np.where(f < 0.55, 20, 150)).astype(np.uint8)      # solid > 200, gas < 50, fluid
        p[8:13, 30 + k:35 + k] = 255                         # a ring of solid around one fluid cell: a pocket the fill takes out
        p[10, 32 + k] = 150
        pix.append(p)
    grids = [oracle.floodfill((p > 200).astype(np.uint32))[0] for p in pix]
    assert all(g[10, 32 + k] == 2 for k, g in enumerate(grids)) and all(len(np.unique(p)) == 3 for p in pix)
    Ds, Df, Dg, CL, CR = 1e-3, 1.0, 10.0, 0.0, 1.0
    sys_ = [oracle.discretize(oracle.fill_D_3phase(p, Df, Ds, Dg), CL, CR, grid=g) for p, g in zip(pix, grids)]
    with pkg.Solver(nx, ny, nimg=B) as s:
        s.set_image(np.stack(pix))
        s.assemble_3phase_native(Ds, Df, Dg, CL, CR)
        s.init_linear(CL, CR)
        A0, b0 = s.get_system()
        x0 = s.get_field()
        assert np.array_equal(A0, np.concatenate([q[0] for q in sys_])) and np.array_equal(b0, np.concatenate([q[1] for q in sys_]))
        assert s.plan_value("native3_rows") == 452

        def unchanged(what):
            assert s.plan_value("native3_rows") == 452, what
            A1, b1 = s.get_system()
            assert np.array_equal(A1, A0) and np.array_equal(b1, b0), what
            with pytest.raises(pkg.DeffError) as e:
                s.sensitivity()
            assert e.value.code == -1 and "Grid" in str(e.value), (what, str(e.value))
            assert np.array_equal(s.get_field(), x0), what

        with pytest.raises(pkg.DeffError) as e:
            s.solve_cg_stream(pix, Ds, -1.0, CL, CR, rtol=1e-6, max_iter=10)
        assert e.value.code == -1 and "admissible" in str(e.value), str(e.value)
        unchanged("an inadmissible Df")
        called = []
        nxt = _capi.NEXT_IMAGE_FN(lambda *a: called.append("next") or 0)
        dn = _capi.CG_IMAGE_DONE_FN(lambda *a: called.append("done"))
        rc = _capi.load().deff_solve_cg_stream(s._ctx, nx + 1, ny, 1, 1, Ds, Df, CL, CR, 1e-6, 10, 64, nxt, dn, None)
        assert rc == -1 and not called, (rc, called)
        unchanged("images of the wrong shape")
        s.set_kernel("explicit")
        s.sweeps(5)
        assert s.kernel_in_use() == "explicit"
        got = s.get_field()
        for k in range(B):
            want = oracle.sweeps(sys_[k][0], sys_[k][1], oracle.linear_guess(nx, ny, CL, CR), 5)
            assert np.array_equal(got[k * ny:(k + 1) * ny], want), k


def test_a_prescaled_stream_refused_for_the_explicit_kernel_changes_nothing(pkg, oracle):
    """"prescaled" is refused "at the call that would sweep (field, system and plan stay as they were)" (deff_amd.h).  For
    deff_solve_stream on a context set to the explicit kernel that call is the stream itself: it must say so before it asks
    for an image, zeroes the slots or replaces the system (found while the refusal was modelled for PRESCALED_SEEDS, whose
    draw knows this refusal; few of its seeds reach it, so it is held here by construction)."""
    nx, ny, B = 64, 24, 2
    rng = np.random.default_rng(9)
    pix = [np.where(rng.random((ny, nx)) < 0.5, 0, 255).astype(np.uint8) for _ in range(B)]
    sys_ = [oracle.discretize(oracle.fill_D_2phase(p, 1.0, 1e-2), 0.25, 0.75) for p in pix]
    pulled = []

    def images():
        for p in pix:
            pulled.append(1)
            yield 255 - p

    with pkg.Solver(nx, ny, nimg=B, kernel="explicit") as s:
        s.set_image(np.stack(pix))
        s.assemble_2phase(1e-2, 1.0, 0.25, 0.75)
        s.init_linear(0.25, 0.75)
        s.sweeps(3)
        x0 = s.get_field()
        s.set_tuning("prescaled", 1)
        with pytest.raises(pkg.DeffError) as e:
            s.solve_stream(images(), 1e-3, 1.0, 0.0, 1.0, 1e-2, 7, check_every=7)
        assert e.value.code == -1 and "prescaled" in str(e.value) and not pulled, (str(e.value), pulled)
        assert np.array_equal(s.get_field(), x0)
        A, b = s.get_system()
        assert np.array_equal(A, np.concatenate([q[0] for q in sys_])) and np.array_equal(b, np.concatenate([q[1] for q in sys_]))
        s.set_tuning("prescaled", 0)
        s.sweeps(2)
        got = s.get_field()
        for k in range(B):
            assert np.array_equal(got[k * ny:(k + 1) * ny], oracle.sweeps(sys_[k][0], sys_[k][1], x0[k * ny:(k + 1) * ny], 2)), k


def test_the_image_forms_follow_the_assembly_sequence_and_a_new_image(pkg, oracle):
    """deff_flux_field, deff_sensitivity and deff_residual take D "from the context's image system"; with no image system they
    are DEFF_ESTATE (deff_amd.h).  A new image without an assembly is no image system: the stored phase diffusivities belonged
    to the old image's (found by the "ff" op of SECOND_ORDER_SEEDS right after "image": deff_set_image left the phase count in
    place, and the three calls evaluated the new pixels with the old system's diffusivities).  Held here by construction with
    the two assembly chains few seeds reach: "2p" -> a caller's D plane, and "3p" -> native 3-phase -> "3p" again."""
    import flux_model
    nx, ny = 33, 20
    rng = np.random.default_rng(909)
    pix = [rng.choice(np.array([0, 30, 120, 199, 201, 255], dtype=np.uint8), size=(ny, nx)) for _ in range(2)]
    Ds, Df, Dg, CL, CR = 1e-2, 1.0, 50.0, 0.25, 0.75
    x0 = rng.random((ny, nx))

    def image_forms_refused(s, code, word):
        for call in (s.flux_field, s.sensitivity, s.residual):
            with pytest.raises(pkg.DeffError) as e:
                call()
            assert e.value.code == code and word in str(e.value), (call.__name__, e.value)
        assert np.array_equal(s.get_field(), x0)

    def image_form_matches(s, D):
        ff = s.flux_field()
        fx, fy, left = flux_model.flux_field(x0, D, CL, CR)
        assert np.array_equal(ff.fx, fx) and np.array_equal(ff.fy, fy) and np.array_equal(ff.left[0], left)
        assert np.array_equal(ff.sections[0], flux_model.sections(fx, left, ny, s.plan_value("flux_kt")))
        with_D = s.flux_field(D, CL, CR)
        assert all(np.array_equal(u, v) for u, v in zip(ff, with_D))

    with pkg.Solver(nx, ny) as s:
        s.set_image(pix[0])
        s.assemble_2phase(Ds, Df, CL, CR)
        s.set_field(x0)
        image_form_matches(s, oracle.fill_D_2phase(pix[0], Df, Ds))
        s.set_image(pix[1])                                  # a new image, no assembly: the field stays, the image system is gone
        image_forms_refused(s, -5, "assembled from the image")
        s.assemble_2phase(Ds, Df, CL, CR)
        image_form_matches(s, oracle.fill_D_2phase(pix[1], Df, Ds))
        s.synth_image(7, 0)                                  # ... and so does a synthetic one
        image_forms_refused(s, -5, "assembled from the image")
        s.set_image(pix[1])
        s.assemble_2phase(Ds, Df, CL, CR)
        D = oracle.fill_D_3phase(pix[1], Df, Ds, Dg)
        s.assemble_from_D(D, CL, CR)                         # "2p" -> "D": a caller's plane is no image system
        with pytest.raises(pkg.DeffError) as e:
            s.flux_field()
        assert e.value.code == -5 and "assembled from the image" in str(e.value), e.value
        s.assemble_3phase(Ds, Df, Dg, CL, CR)                # "3p" -> "3n" -> "3p"
        image_form_matches(s, D)
        s.assemble_3phase_native(Ds, Df, Dg, CL, CR)
        with pytest.raises(pkg.DeffError) as e:
            s.flux_field()
        assert e.value.code == -1 and "Grid" in str(e.value), e.value
        s.assemble_3phase(2 * Ds, Df, Dg, CL, CR)
        image_form_matches(s, oracle.fill_D_3phase(pix[1], Df, 2 * Ds, Dg))


@pytest.mark.parametrize("launch,T", [(0, 4), (0, 8), (1, 4), (1, 8)])     # workgroup tiles exist for passes of 4 and 8
def test_stamps_advance_one_pass_or_three_on_a_resident_plan(pkg, oracle, launch, T):
    """deff_debug_tb_stamps by construction on both kinds of plan, so that the 3 T of deff_amd.h does not rest on what the
    seeds happen to draw: workgroup tiles of a small stack are resident under tb_launch 0 (the field advances by three
    passes) and one launch per pass under tb_launch 1 (one pass)."""
    nx, ny, B = 97, 41, 2
    rng = np.random.default_rng(11 + T)
    pix = [np.where(rng.random((ny, nx)) < 0.5, 0, 255).astype(np.uint8) for _ in range(B)]
    x0 = [rng.random((ny, nx)) for _ in range(B)]
    with pkg.Solver(nx, ny, nimg=B, kernel="matfree_tb") as s:
        s.set_tuning("tb_impl", 2); s.set_tuning("tb_launch", launch); s.set_tuning("tb_T", T)
        s.set_image(np.stack(pix))
        s.assemble_2phase(1e-2, 1.0, 0.0, 1.0)
        s.set_field(np.concatenate(x0, axis=0))
        n0, n1, words = tb_stamps(s, 2.0 / 3.0)
        p = s.plan()
        assert (p["tb_impl"], p["tb_T"], p["tb_resident"]) == (2, T, 1 - launch), p
        per = 12 if p["tb_resident"] else T + 4
        assert n0 == n1 > 0 and np.all(words[:len(words) // per * per:per] != 0), (n0, n1)
        got = s.get_field()
        for k in range(B):
            A, b = oracle.discretize(oracle.fill_D_2phase(pix[k], 1.0, 1e-2), 0.0, 1.0)
            assert np.array_equal(got[k * ny:(k + 1) * ny], oracle.sweeps(A, b, x0[k], T * (3 if p["tb_resident"] else 1))), (p, k)
        assert s.plan_value("tb_fallbacks") == 0


@pytest.mark.parametrize("reader", ["ptr", "slots"])
def test_device_field_and_slot_reads_of_a_stack_with_frozen_images(pkg, oracle, reader):
    """A batch solve leaves an image that stopped early in the buffer it stopped in.  deff_device_field has to bring it into
    the buffer it hands out, and deff_get_slot_field has to read it where it is and leave the stack as it found it -- with
    no deff_get_field in between, which would do the work for them.  One image of three stops at its second check (parallel
    stripes: the wall fluxes settle after one sweep), the others run to max_iter, on the single-sweep kernel (one buffer flip
    per sweep) for two consecutive max_iter: both parities of the flips after the early stop."""
    nx, ny, B, ce = 97, 41, 3, 10
    rng = np.random.default_rng(99)
    pix = [np.where(rng.random((ny, nx)) < p, 0, 255).astype(np.uint8) for p in (0.45, 0.5, 0.6)]
    pix[1][:] = 255
    pix[1][:10, :] = 0
    for max_iter in (ce + 2, ce + 3):
        want, iters, sys_ = [], [], []
        for k in range(B):
            D = oracle.fill_D_2phase(pix[k], 1.0, 1e-2)
            A, b = oracle.discretize(D, 0.25, 0.75)
            it, _, _, x, _, _ = oracle.jacobi(A, b, oracle.linear_guess(nx, ny, 0.25, 0.75), D, 0.25, 0.75, 1e-6, max_iter, check_every=ce)
            want.append(x); iters.append(it); sys_.append((A, b))
        assert iters == [max_iter, ce + 1, max_iter]
        with pkg.Solver(nx, ny, nimg=B, kernel="matfree") as s:
            s.set_image(np.stack(pix))
            s.assemble_2phase(1e-2, 1.0, 0.25, 0.75)
            s.init_linear(0.25, 0.75)
            res = s.solve(1e-6, max_iter, check_every=ce)
            assert [r.iters for r in res] == iters
            if reader == "ptr":
                p, pitch = s.device_field_ptr()
                s.synchronize()
                got = device_rows(p, B * ny, pitch)[:, :nx]
            else:
                from effectivediffusivityfvm_amd import _capi
                got = np.empty((B * ny, nx))
                for k in range(B):
                    _capi.check(_capi.load().deff_get_slot_field(s._ctx, k, got[k * ny:(k + 1) * ny]))
            for k in range(B):
                assert np.array_equal(got[k * ny:(k + 1) * ny], want[k]), (max_iter, k)
            s.sweeps(3)                                      # and the stack goes on from every image's final field
            got = s.get_field()
            for k in range(B):
                assert np.array_equal(got[k * ny:(k + 1) * ny], oracle.sweeps(sys_[k][0], sys_[k][1], want[k], 3)), (max_iter, k)


def run_slab_sequence(pkg, ob, seed):
    """The same idea for one image split into row slabs (deff_slab_group_*, N slabs on one GPU: peer copies between their
    buffers, one exchange of 8 halo rows per pass, optionally overlapped with the interior): random sizes (odd widths, slabs
    that differ by a row), slab counts, sweeps per pass, overlap modes and call sequences; every read against the oracle."""
    rng = np.random.default_rng(seed)
    nx = int(rng.integers(8, 420))
    nslabs = int(rng.integers(2, 5))
    ny = int(rng.integers(8 * nslabs, 8 * nslabs + 500))
    m = Model(ob, nx, ny, 1, rng)
    log = [f"nx {nx} ny {ny} slabs {nslabs}"]
    with pkg.SlabGroup(nx, ny, [0] * nslabs) as g:
        m.new_image()
        g.set_image(m.pix[0])
        for step in range(16):
            ops = ["image", "assemble", "tune"]
            if m.kind is not None:
                ops += ["init", "set_field"]
                if m.x is not None:
                    ops += ["sweeps", "sweeps", "solve", "flux", "get"]
            op = ops[rng.integers(len(ops))]
            if op == "image":
                m.new_image()
                g.set_image(m.pix[0])
                log.append("image")
            elif op == "assemble":
                kind = ["2p", "2p", "3p"][rng.integers(3)]
                Ds, Df, Dg = [(1e-3, 1.0, 10.0), (1e-2, 1.0, 50.0), (0.1, 2.0, 7.0)][rng.integers(3)]
                CL, CR = [(0.0, 1.0), (0.25, 0.75)][rng.integers(2)]
                m.assemble(kind, Ds, Df, Dg, CL, CR)
                if kind == "2p":
                    g.assemble_2phase(Ds, Df, CL, CR)
                else:
                    g.assemble_3phase(Ds, Df, Dg, CL, CR)
                log.append(f"assemble {kind} {Ds} {Df} {CL}")
            elif op == "tune":
                if rng.random() < 0.5:
                    v = int(rng.choice([0, 1, 2, 4, 8])); g.set_tuning("tb_T", v); log.append(f"tb_T {v}")
                else:
                    v = int(rng.choice([0, 1, 2])); g.set_tuning("slab_overlap", v); log.append(f"slab_overlap {v}")
            elif op == "init":
                g.init_linear(m.CL, m.CR)
                m.x = [ob.linear_guess(nx, ny, m.CL, m.CR)]
                log.append("init")
            elif op == "set_field":
                m.x = [rng.random((ny, nx))]
                g.set_field(m.x[0])
                log.append("set_field")
            elif op == "sweeps":
                k = int(rng.choice([1, 3, 8, 17, 40]))
                omega, kern = [(2.0 / 3.0, 0), (1.0, 1)][rng.integers(2)]
                g.sweeps(k, omega)
                m.x = [ob.sweeps(m.A[0], m.b[0], m.x[0], k, kernel=kern, omega=omega)]
                log.append(f"sweeps {k} {omega:.3f}")
                assert np.array_equal(g.get_field(), m.x[0]), (seed, log)
            elif op == "solve":
                tol = float(rng.choice([1e-2, 1e-4, 1e-12]))
                max_iter = int(rng.choice([1, 7, 100, 101, 130]))
                ce = int(rng.choice([7, 50, 100]))
                r = g.solve(tol, max_iter, check_every=ce)
                log.append(f"solve {tol} {max_iter} {ce}")
                it, deff, conv, x, MFL, MFR = ob.jacobi(m.A[0], m.b[0], m.x[0], m.D[0], m.CL, m.CR, tol, max_iter, check_every=ce)
                assert (r.iters, r.deff_raw, r.conv) == (it, deff, conv), (seed, log)
                m.x = [x]
                assert np.array_equal(g.get_field(), x), (seed, log)
            elif op == "flux":
                d, MFL, MFR = g.flux()
                want, L, R = ob.flux_deff(m.x[0], m.D[0], m.CL, m.CR)
                assert d == want and np.array_equal(MFL, L) and np.array_equal(MFR, R), (seed, log)
                log.append("flux")
            elif op == "get":
                assert np.array_equal(g.get_field(), m.x[0]), (seed, log)
                log.append("get")
    return log


@pytest.mark.parametrize("seed", range(16))
def test_random_call_sequences_on_row_slabs_match_the_oracle(pkg, oracle, seed):
    run_slab_sequence(pkg, oracle, 5000 + seed)


# ---------------------------------------------------------------------------------------------------------------------------
# Volumes (deff_volume_*): a second state machine -- a private context, two link planes and a have_system flag.

VOLUME_SHAPES = [(9, 7, 3), (16, 3, 5), (130, 5, 4), (33, 5, 1)]


def run_volume_sequence(pkg, seed):
    """About 20 calls on one Volume against tests/volume_model.py: assemblies from a drawn D (about 10 % zeros), linear guesses
    and caller's fields, CG (max_iter 0 / 2 / 7 / large, two tolerances, two check intervals), fluxes, reads of the field and
    of the system, and in between a second Volume of another shape or a 2-D Solver that is opened, solved and closed.  CG is
    compared with a twin -- a fresh Volume given the same D, the same field through set_field and the OTHER check interval:
    field, result and wall fluxes bit for bit -- and rel_residual with the model's residual under the bars of
    test_gpu_volume.py; the model then adopts the field.  The refusals a Volume has (cg before a field, cg before a system,
    get_system before a system: DEFF_ESTATE) change nothing."""
    import oracle_binding as ob
    import volume_model as vm
    from test_gpu_cg import EPS
    from test_gpu_volume import ESTATE, RES_BAR, RES_BAR_CONVERGED
    ob.build()
    rng = np.random.default_rng(seed)
    nx, ny, nz = VOLUME_SHAPES[rng.integers(len(VOLUME_SHAPES))]
    shape = (nz, ny, nx)
    log = [f"volume {nx} {ny} {nz}"]
    D = A = b = x = None
    CL, CR = 0.0, 1.0

    def draw_D(shp):
        d = rng.uniform(1e-3, 2.0, shp)
        d[rng.random(shp) < 0.10] = 0.0
        return d

    with pkg.Volume(nx, ny, nz) as v:
        def unchanged():
            if x is not None:
                assert vm.same_bits(v.get_field(), x), (seed, log, "field")
            if A is not None:
                Ag, bg = v.get_system()
                assert vm.same_bits(Ag, A) and vm.same_bits(bg, b), (seed, log, "system")

        def refused(call, word):
            with pytest.raises(pkg.DeffError) as e:
                call()
            assert e.value.code == ESTATE and word in str(e.value), (seed, log, e.value)
            log[-1] += " refused"
            unchanged()

        for step in range(20):
            ops = ["assemble", "init", "set_field", "cg", "cg", "getsys", "other"]
            if x is not None:
                ops += ["get"] + (["flux", "flux", "cg"] if A is not None else [])
            op = ops[rng.integers(len(ops))]
            if op == "assemble":
                D = draw_D(shape)
                CL, CR = ASSEMBLE_C[rng.integers(2)]
                log.append(f"assemble {CL} {CR}")
                v.assemble_from_D(D, CL, CR)
                A, b = vm.rows3(D, CL, CR)
                unchanged()                                  # (get_system gives the model's rows bit for bit; the field stays)
            elif op == "init":
                log.append("init")
                v.init_linear(CL, CR)
                x = v.get_field()
                # (every row of every slice is the 2-D guess's: test_gpu_volume.py::test_one_slice_is_the_2d_plane_form)
                assert np.array_equal(x, np.broadcast_to(ob.linear_guess(nx, ny, CL, CR)[0], shape)), (seed, log)
            elif op == "set_field":
                log.append("set_field")
                x = rng.random(shape)
                v.set_field(x)
                unchanged()
            elif op == "getsys":
                log.append("getsys")
                if A is None:
                    refused(v.get_system, "system")
                else:
                    unchanged()
            elif op == "get":
                log.append("get")
                unchanged()
            elif op == "flux":
                log.append("flux")
                d, MFL, MFR = v.flux()
                d2, MFL2, MFR2 = v.flux()
                assert d == d2 and np.array_equal(MFL, MFL2) and np.array_equal(MFR, MFR2), (seed, log)
                want = vm.deff_of(x, D, CL, CR)
                assert abs(d - want) <= 64 * EPS * abs(want), (seed, log, d, want)
                unchanged()
            elif op == "cg":
                rtol = float(rng.choice([1e-6, 1e-10]))
                max_iter = int(rng.choice([0, 2, 7, 100000]))
                ce = int(rng.choice([1, 64]))
                log.append(f"cg {rtol} {max_iter} {ce}")
                call = lambda: v.solve_cg(rtol=rtol, max_iter=max_iter, check_every=ce)     # noqa: E731
                if x is None or A is None:
                    # (with neither, the header names no order of the two checks: either word)
                    refused(call, "" if x is None and A is None else "field" if x is None else "system")
                    continue
                r = call()
                got = v.get_field()
                assert v.plan_value("cg_impl") == 5, (seed, log)
                with pkg.Volume(nx, ny, nz) as f:
                    f.assemble_from_D(D, CL, CR)
                    f.set_field(x)
                    rf = f.solve_cg(rtol=rtol, max_iter=max_iter, check_every=1 if ce == 64 else 64)
                    assert (rf.iters, rf.rel_residual, rf.converged, rf.deff_raw) == (r.iters, r.rel_residual, r.converged, r.deff_raw), \
                        (seed, log, r, rf)
                    assert vm.same_bits(f.get_field(), got), (seed, log, "CG on a fresh volume")
                    assert np.array_equal(rf.MFL, r.MFL) and np.array_equal(rf.MFR, r.MFR), (seed, log)
                dec = vm.decoupled3(A, b).reshape(shape)
                assert np.all(got[dec] == 0.0), (seed, log)
                assert r.iters <= max_iter and r.converged == (r.rel_residual <= rtol), (seed, log, r)
                res = vm.residual3(A, b, got, shape)
                res_ld = vm.residual3(A, b, got, shape, np.longdouble)
                print(f"seed {seed} {log[-1]}: iters {r.iters} rel_residual {r.rel_residual:.6e}, model {res:.6e}, long double {res_ld:.6e}")
                if r.converged:
                    assert res_ld <= rtol * (1 + 1e-6) + 1e-13, (seed, log, res_ld)
                if not r.converged and res >= 1e-6:
                    assert abs(r.rel_residual - res) <= RES_BAR * res, (seed, log, r.rel_residual, res)
                else:
                    # test_gpu_volume.py holds a converged field to 1e-3 of the long-double residual at rtol = 1e-13, where
                    # that is 1e-16 absolute.  rel_residual is a float64 evaluation: its rounding error is absolute (it
                    # does not shrink with the residual), and CG often lands far below a loose rtol, so the same 1e-16 is
                    # what the bar means for residuals smaller than 1e-13 (seed 12002: 1.666e-15 against 1.654e-15).
                    assert abs(r.rel_residual - res_ld) <= RES_BAR_CONVERGED * max(res_ld, 1e-13), (seed, log, r.rel_residual, res_ld)
                x = got
                d, MFL, MFR = v.flux()
                assert r.deff_raw == d and np.array_equal(r.MFL, MFL) and np.array_equal(r.MFR, MFR), (seed, log)
                log[-1] += " iters %d" % r.iters
                unchanged()
            else:
                # something else on the device in between: a second Volume of another shape, or a 2-D Solver
                if rng.random() < 0.5:
                    ox, oy, oz = VOLUME_SHAPES[(VOLUME_SHAPES.index((nx, ny, nz)) + 1 + int(rng.integers(3))) % 4]
                    log.append(f"other volume {ox} {oy} {oz}")
                    with pkg.Volume(ox, oy, oz) as o:
                        o.assemble_from_D(draw_D((oz, oy, ox)), 0.0, 1.0)
                        o.init_linear(0.0, 1.0)
                        o.solve_cg(rtol=1e-8, max_iter=200)
                else:
                    log.append("other solver")
                    with pkg.Solver(33, 20) as o:
                        o.set_tuning("cg_planes", 1)
                        o.assemble_from_D(draw_D((20, 33)), 0.0, 1.0)
                        o.init_linear(0.0, 1.0)
                        o.solve_cg(rtol=1e-8, max_iter=200)
                unchanged()
        unchanged()
    return log


@pytest.mark.parametrize("seed", range(16))
def test_random_call_sequences_on_volumes(pkg, seed):
    run_volume_sequence(pkg, 12000 + seed)
