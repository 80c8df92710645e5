"""What the random call sequences of test_gpu_sequences.py reach, counted without a GPU.

The draw of a sequence depends on the generator and on the model's state, never on what the GPU returns, so draw_sequence()
can be replayed here.  Two things are pinned: the 64 seeds that existed before the draw had options still draw what they
drew (tests/golden/sequence_draws_seeds_1000_2000.json: their op logs and a SHA-1 of every array they hand to the solver, in
call order.  The file was recorded from run_sequence() as it was before the draw was separated from it -- that function run
on a GPU with the Solver wrapped so that every array passed to set_image, assemble_from_D and set_field was hashed on its
way in, and its own log taken without the "refused" marks), and the seed ranges of the options reach the call orders they were added
for -- an option nobody draws, or a stream nobody reads after, would leave the GPU tests green and empty.

The seeds of those option groups are pinned in turn (tests/golden/sequence_draws_option_seeds.json, written with draw_log()
below before the draw gained its later options), and the later groups -- the native 3-phase assembly, a caller's system, the
Deff gradient, the CG keys and the CG stream, the pre-scaled sweeps -- have a census of their own: every op, kind and key value
they add, and the call orders they are there for.  Those three groups are pinned as well
(tests/golden/sequence_draws_later_seeds.json, recorded before the draw gained `adjoint`, with the images and arguments of
every stream in the digest and the log), and the field adjoint's group has its census below; its draws are pinned too
(tests/golden/sequence_draws_adjoint_seeds.json, recorded before the draw gained `tangent`, `second`, `fluxfield` and
`onchip_planes`).  The group of those four options has its census at the end of this file, with a replay under a flipped rule that
shows the validity checks bite."""
import hashlib
import json
import os

import numpy as np
import pytest

import test_gpu_sequences as seq
from conftest import GOLDEN

GROUPS = {"onchip": seq.ONCHIP_SEEDS, "stream": seq.STREAM_SEEDS, "fma": seq.FMA_SEEDS}
READS = ("sweeps", "solve", "flux", "get", "residual", "ptr", "slot", "stamps", "cg")     # read or advance the current field
REPLACES = ("init", "set_field", "stream")                                                # a new field: the old one is gone


def seeds_of(group):
    g = GROUPS[group]
    return [(g["first"] + i, seq.seed_options(g)) for i in range(g["count"])]


def draw_log(seed, every_array=False, **options):
    """The op log run_sequence() writes (without what only a run can add: "refused", the CG form, the stream's early slots, the
    stamps' sweeps) and the digest of the arrays in the order the solver receives them.  The two older golden files were
    recorded while a "stream" was logged by its name alone and its images were left out of the digest; `every_array` (the
    later groups' file and every one after it) logs and hashes a stream as a CG stream is, and logs the arguments the older
    form leaves out (a solve's reader, the slot read, the stamps' omega)."""
    draw = seq.draw_sequence(seed, **options)
    _, nx, ny, B, fma = next(draw)
    h = hashlib.sha1(repr((nx, ny, B)).encode())
    h.update(np.stack(next(draw)[1]).tobytes())
    log = []
    for op, *a in draw:
        if op == "image":
            h.update(np.stack(a[0]).tobytes())
            log.append("image")
        elif op == "assemble":
            if a[6] is not None:                             # a D plane, or the plane behind a caller's system
                h.update(np.concatenate(a[6], axis=0).tobytes())
            log.append(f"assemble {a[0]} {a[1]} {a[2]} {a[4]}" + (f" of {a[7]}" if len(a) > 7 else ""))
        elif op == "tune":
            log.append(f"{a[0]} {a[1]}")
        elif op == "kernel":
            log.append(f"kernel {a[0]}")
        elif op == "set_field":
            h.update(np.concatenate(a[0], axis=0).tobytes())
            log.append("set_field")
        elif op == "sweeps":
            log.append(f"sweeps {a[0]} {a[1]:.3f}")
        elif op in ("solve", "cg"):
            log.append(f"{op} {a[0]} {a[1]} {a[2]}" + (f" then {a[3]}" if every_array and op == "solve" else ""))
        elif op == "stage":
            log.append(f"stage {a[0]} {a[1]} {a[2]} {a[3]}")
        elif op == "cgstream" or (op == "stream" and every_array):
            h.update(np.stack(a[0]).tobytes())
            log.append(f"{op} {len(a[0])} {a[1]} {a[2]} {a[3]} {a[5]} {a[6]} {a[7]}")
        elif op == "slot" and every_array:
            log.append(f"slot {a[0]}")
        elif op == "stamps" and every_array:
            log.append(f"stamps {a[0]:.3f}")
        elif op == "adj":                                    # w, rtol, max_iter, check_every
            h.update(np.concatenate(a[0], axis=0).tobytes())
            log.append(f"adj {a[1]} {a[2]} {a[3]}")
        elif op == "setadj":
            h.update(np.concatenate(a[0], axis=0).tobytes())
            log.append("setadj")
        elif op == "vjp":                                    # a drawn D plane or None (the model's), CL, CR
            if a[0] is not None:
                h.update(np.concatenate(a[0], axis=0).tobytes())
            log.append(f"vjp {'D' if a[0] is not None else 'model'} {a[1]} {a[2]}")
        else:
            log.append(op)
    return log, h.hexdigest()


def test_the_old_seeds_draw_what_they_always_drew():
    with open(os.path.join(GOLDEN, "sequence_draws_seeds_1000_2000.json")) as f:
        recorded = json.load(f)
    assert len(recorded) == 64
    for seed in list(range(1000, 1040)) + list(range(2000, 2024)):
        log, digest = draw_log(seed, with_cg=seed >= 2000)
        assert "|".join(log) == recorded[str(seed)]["log"], seed
        assert digest == recorded[str(seed)]["data"], seed


def test_the_option_seeds_draw_what_they_drew_before_the_later_options():
    """The seeds of the on-chip, stream and fma groups, recorded (with draw_log above) before the draw gained native3, system,
    cgkeys, cgstream, sens and prescaled: with those off the generator is consumed as it was."""
    with open(os.path.join(GOLDEN, "sequence_draws_option_seeds.json")) as f:
        recorded = json.load(f)
    seeds = [(seed, options) for group in ("onchip", "stream", "fma") for seed, options in seeds_of(group)]
    assert len(recorded) == len(seeds) == 120
    for seed, options in seeds:
        log, digest = draw_log(seed, **options)
        assert "|".join(log) == recorded[str(seed)]["log"], seed
        assert digest == recorded[str(seed)]["data"], seed


def test_the_later_seeds_draw_what_they_drew_before_the_adjoint():
    """The native, CG-key and pre-scaled groups, recorded (draw_log with every_array) before the draw gained `adjoint`: with
    that option off the generator is consumed as it was, streams' images and arguments included."""
    with open(os.path.join(GOLDEN, "sequence_draws_later_seeds.json")) as f:
        recorded = json.load(f)
    seeds = [(g["first"] + i, seq.seed_options(g)) for g in (seq.NATIVE_SEEDS, seq.CGKEY_SEEDS, seq.PRESCALED_SEEDS)
             for i in range(g["count"])]
    assert len(recorded) == len(seeds) == 120
    for seed, options in seeds:
        log, digest = draw_log(seed, every_array=True, **options)
        assert "|".join(log) == recorded[str(seed)]["log"], seed
        assert digest == recorded[str(seed)]["data"], seed


def test_stream_schedule_follows_the_refill_rule():
    """stream_schedule against cases worked by hand (C = check interval; a free slot is refilled after the C - 1 sweeps that
    follow a check, its image's first sweep is the next check)."""
    # 2 slots, C = 10: images of 11, 25 (max_iter between checks), 25 and 1 sweeps
    slot_of, retired, end = seq.stream_schedule([11, 25, 25, 1], 2, 25, 10)
    assert slot_of == [0, 1, 0, 1]
    # image 0 leaves at sweep 11; slot 0 is refilled at 20 and image 2 runs 21 ... 45; image 1 leaves at 25, slot 1 is refilled
    # at 30 (phase of slot 0's image: checks at 21, 31, 41): image 3 runs sweep 31 only
    assert retired == [11, 25, 45, 31] and end == 45
    # everything stops together: nobody retires early
    slot_of, retired, end = seq.stream_schedule([7, 7, 7], 3, 7, 100)
    assert slot_of == [0, 1, 2] and retired == [7, 7, 7] and end == 7
    # one slot left running alone; the stream's phase restarts when all slots are empty between two checks
    # (C = 4, max_iter 7: both slots stop at the check of sweep 5; image 2 then runs sweeps 6 ... 12 with checks of its own)
    slot_of, retired, end = seq.stream_schedule([5, 5, 7], 2, 7, 4)
    assert slot_of == [0, 1, 0] and retired == [5, 5, 12] and end == 12


def census(oracle):
    """Per seed of the option groups: the op kinds drawn, the CG forms that run, and what follows them and the streams."""
    out = {}
    for group in GROUPS:
        for seed, options in seeds_of(group):
            draw = seq.draw_sequence(seed, **options)
            _, nx, ny, B, fma = next(draw)
            next(draw)
            flavour = "fma" if fma else None
            kinds, forms = set(["fma"] if fma else []), set()
            onchip_key, kind = 0, None
            cg2_pending = stream_pending = False
            cg2_followed = stream_followed = False
            frozen_readers = set()                           # a solve of a stack read first by deff_device_field / deff_get_slot_field
            for op, *a in draw:
                kinds.add("cg_onchip" if op == "tune" and a[0] == "cg_onchip" else op)
                if op == "tune" and a[0] == "cg_onchip":
                    onchip_key = a[1]
                if op == "image":
                    kind = None
                if op == "solve" and B > 1 and a[3] != "get":
                    frozen_readers.add(a[3])
                if op == "assemble":
                    kind = a[0]
                if op in ("sweeps", "solve") and cg2_pending:
                    cg2_followed = True
                if op in READS and stream_pending:
                    stream_followed = True
                if op in REPLACES:
                    cg2_pending = stream_pending = False
                if op == "cg" and kind in ("2p", "3p"):  # two or three pixel classes: at most 3^5 rows, a dictionary, never refused
                    impl = seq.expected_cg_impl(nx, ny, onchip_key)
                    forms.add(impl)
                    cg2_pending = cg2_pending or impl == 2
                if op == "stream":
                    imgs, Ds, Df, CL, CR, tol, max_iter, ce = a
                    kind = "2p"
                    iters = []
                    for pix in imgs:
                        D = oracle.fill_D_2phase(pix, Df, Ds)
                        A, b = oracle.discretize(D, CL, CR)
                        iters.append(oracle.jacobi(A, b, oracle.linear_guess(nx, ny, CL, CR, flavour=flavour), D, CL, CR, tol, max_iter,
                                                   check_every=ce, flavour=flavour)[0])
                    slot_of, retired, end = seq.stream_schedule(iters, B, max_iter, ce)
                    last = {k: i for i, k in enumerate(slot_of)}
                    stream_pending = any(retired[i] < end for i in last.values())
            out[seed] = dict(group=group, kinds=kinds, forms=forms, cg2_followed=cg2_followed, stream_followed=stream_followed,
                             frozen_readers=frozen_readers)
    return out


def test_the_option_seeds_reach_what_they_were_added_for(oracle):
    c = census(oracle)
    count = lambda pred: sum(1 for v in c.values() if pred(v))
    reached = {k: count(lambda v: k in v["kinds"]) for k in ("stream", "ptr", "slot", "stamps", "cg_onchip", "fma")}
    both = count(lambda v: v["forms"] == {1, 2})
    cg2 = count(lambda v: v["cg2_followed"])
    early = count(lambda v: v["stream_followed"])
    print(f"seeds that draw: {reached}; an on-chip CG followed by sweeps or a solve: {cg2}; both CG forms on one context: {both}; "
          f"a stream with a slot frozen before its end, then read or advanced: {early}")
    assert all(n >= 8 for n in reached.values()), reached
    # a stack's solve whose first reader is the device pointer / the slot reads, not deff_get_field: as many seeds as an op kind
    frozen = {k: count(lambda v: k in v["frozen_readers"]) for k in ("ptr", "slot")}
    print(f"seeds with a stack's solve read first through: {frozen}")
    assert all(n >= 8 for n in frozen.values()), frozen
    assert cg2 >= 8 and both >= 4 and early >= 8, (cg2, both, early)
    # the contracted arithmetic never meets CG, whose arithmetic has one form only
    assert all("cg" not in v["kinds"] for v in c.values() if v["group"] == "fma")
    # at least one on-chip seed has a shape that is not eligible, and most are
    shapes = [(nx + (nx & 1)) * ny <= seq.ONCHIP_LIMIT for nx, ny in seq.ONCHIP_SHAPES]
    assert not all(shapes) and sum(shapes) > len(shapes) / 2 and (128, 128) in seq.ONCHIP_SHAPES
    assert any(nx & 1 and (nx + 1) * ny <= seq.ONCHIP_LIMIT for nx, ny in seq.ONCHIP_SHAPES)


# ---------------------------------------------------------------------------------------------------------------------------
# The later option groups: what their seeds draw, and the call orders they were added for.  All of it follows from the draw
# and from facts of the model's state (kind of system, keys set, whether the device fill is the current image's); the one
# thing that needs the oracle is the number of distinct rows of a system (whether it has a dictionary: the CG form).

NEW_GROUPS = {"native": seq.NATIVE_SEEDS, "cgkey": seq.CGKEY_SEEDS, "prescaled": seq.PRESCALED_SEEDS}


def distinct_rows(oracle, pix, kind, Ds, Df, Dg, CL, CR, D, base):
    m = seq.Model(oracle, pix[0].shape[1], pix[0].shape[0], len(pix), None)
    m.pix = pix
    m.assemble(kind, Ds, Df, Dg, CL, CR, D, base)
    return len(np.unique(np.column_stack([np.concatenate(m.A), np.concatenate(m.b)]), axis=0))


def new_census(oracle):
    """Per seed of the later groups: `kinds` = the ops, assembly kinds ("assemble 3n") and key values ("cg_fold 2") drawn, and
    `orders` = which of the call orders below it reaches."""
    out = {}
    for group, g in NEW_GROUPS.items():
        for i in range(g["count"]):
            seed, options = g["first"] + i, seq.seed_options(g)
            draw = seq.draw_sequence(seed, **options)
            _, nx, ny, B, _ = next(draw)
            pix = next(draw)[1]
            kinds, orders = set(), set()
            kind, asm, nrows = None, None, None              # the system: its kind, the arguments it was assembled with, its rows
            keys = dict(cg_onchip=0, cg_planes=0, cg_fold=0, prescaled=0, tb_impl=0, tb_launch=0)
            kset = "auto"
            planes_built = False                             # of a "3n" system: its planes exist already
            n3_chain = 0                                     # 1: "3n" on this image; 2: ... then another kind
            after_stream = False                             # a stream put images into the slots, no deff_set_image since
            sw_chain = 0                                     # 1: "Sw"; 2: ... then assemble "2p" or a stream
            b_pending = False                                # a refused cgstream on a "3n" system, no assembly since
            pre_chain, pre_omegas = {}, set()                # per omega: 1 = sweeps under prescaled 1, 2 = then prescaled 0
            hist = []

            def rows():
                nonlocal nrows
                if nrows is None:
                    nrows = distinct_rows(oracle, pix, *asm)
                return nrows

            def took_stream():
                nonlocal kind, asm, nrows, after_stream, n3_chain, b_pending, sw_chain, pre_chain
                kind, nrows, asm = "2p", 1, None
                after_stream, n3_chain, b_pending, pre_chain = True, 0, False, {}
                sw_chain = 2 if sw_chain >= 1 else 0

            for op, *a in draw:
                explicit_sweep = op in ("sweeps", "solve") and kset == "explicit" and not keys["prescaled"]
                if op == "tune":
                    kinds.add(f"{a[0]} {a[1]}")
                    if a[0] in keys:
                        keys[a[0]] = a[1]
                    if a[0] == "prescaled" and a[1] == 0:
                        pre_chain = {w: 2 for w in pre_chain}
                elif op == "assemble":
                    kinds.add("assemble " + a[0])
                else:
                    kinds.add(op)
                if op == "kernel":
                    kset = a[0]
                elif op == "image":
                    pix, kind = a[0], None
                    n3_chain, after_stream, b_pending, pre_chain = 0, False, False, {}
                elif op in ("assemble", "stage"):
                    if op == "stage":
                        a = ["3n"] + a + [None]
                    if a[0] == "3n":
                        if n3_chain == 2:
                            orders.add(2)
                        if after_stream:
                            orders.add(3)
                        n3_chain, after_stream = 1, False
                    elif n3_chain:
                        n3_chain = 2
                    sw_chain = 1 if a[0] == "Sw" else 2 if a[0] == "2p" and sw_chain >= 1 else 0
                    if a[0] in ("D", "S", "Sw"):
                        kset = "auto"
                    kind, asm, nrows = a[0], (a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7] if len(a) > 7 else None), None
                    planes_built, b_pending, pre_chain = False, False, {}
                elif op == "stream":
                    if not (keys["prescaled"] and kset == "explicit"):
                        took_stream()
                elif op == "cgstream":
                    if a[2] < 0:
                        kinds.add("cgstream refused")
                        b_pending = b_pending or kind == "3n"
                    else:
                        took_stream()
                elif op == "cg" and kind != "Sw":
                    has_dict = kind in ("2p", "3n") or rows() <= 511
                    if has_dict or keys["cg_planes"]:
                        impl = 3 if keys["cg_planes"] == 2 or not has_dict else seq.expected_cg_impl(nx, ny, keys["cg_onchip"])
                        kinds.add(f"cg impl {impl}")
                        if impl in (1, 3) and keys["cg_fold"]:
                            kinds.add(f"cg impl {impl} fold {keys['cg_fold']}")
                        if kind == "3n" and impl == 3 and not planes_built:
                            orders.add(1)
                            planes_built = True
                        if sw_chain == 2:
                            orders.add(4)
                elif op == "cg":
                    kinds.add("cg on Sw")
                if kind == "3n" and (op == "getsys" or explicit_sweep):
                    if not planes_built:
                        orders.add(1)
                    planes_built = True
                    if b_pending:
                        orders.add(5)
                if op == "solve" and hist[-2:] == ["sweeps", "sens"] and keys["tb_impl"] == 2 and keys["tb_launch"] == 0 \
                        and kset in ("auto", "matfree_tb") and kind != "Sw" and keys_at_sweeps == (2, 0):
                    orders.add(6)
                if op == "sweeps":
                    keys_at_sweeps = (keys["tb_impl"], keys["tb_launch"])
                    refused = keys["prescaled"] and (kset == "explicit" or kind == "Sw" or (kind not in ("2p", "3n") and rows() > 511))
                    if keys["prescaled"] and not refused:
                        kinds.add("prescaled sweeps")
                        pre_chain[a[1]] = 1
                    elif keys["prescaled"]:
                        kinds.add("prescaled refused")
                    elif pre_chain.get(a[1]) == 2 and kset != "explicit":
                        orders.add(7)
                        pre_omegas.add(a[1])
                if op in ("init", "set_field"):
                    pass                                     # (a new field does not touch the tables the orders are about)
                hist.append(op)
            out[seed] = dict(group=group, kinds=kinds, orders=orders, pre_omegas=pre_omegas, shape=(nx, ny), B=B)
    return out


NEW_KINDS = {
    "native": ["assemble 3n", "assemble 3g", "stage", "grid", "fill_impl 0", "fill_impl 1", "fill_impl 2", "fill_tile_rows 0",
               "fill_tile_rows 8", "fill_tile_rows 16", "assemble S", "assemble Sw", "getsys", "sens"],
    "cgkey": ["cg_planes 0", "cg_planes 1", "cg_planes 2", "cg_fold 0", "cg_fold 1", "cg_fold 2", "cgstream", "cgstream refused",
              "assemble 3n", "assemble S", "assemble Sw", "getsys", "cg on Sw"],
    "prescaled": ["prescaled 0", "prescaled 1", "prescaled sweeps", "prescaled refused", "assemble 3n", "assemble S", "stream"],
}
NEW_ORDERS = {"native": [1, 2, 3, 6], "cgkey": [1, 2, 3, 4, 5], "prescaled": [7]}


def test_the_later_option_seeds_reach_what_they_were_added_for(oracle):
    """Every new op, kind and key value is drawn by at least 8 seeds of its group, and at least 4 seeds of a group reach each of
    1  "3n", then what needs its planes built on demand: an explicit sweep, deff_get_system, CG under cg_planes 2
    2  "3n" -> an assembly of another kind -> "3n" on the same image (the fill is reused)
    3  a stream or a CG stream, then "3n" (a fresh fill of the slots' images)
    4  "Sw" -> assemble "2p" or a stream -> cg (a caller's wall-column links must not outlive its system)
    5  a refused CG stream on a "3n" system, then deff_get_system or an explicit sweep (the refusal must change nothing)
    6  sweeps, the gradient, a solve in a row under tb_impl 2 / tb_launch 0 (a resident interval no check has settled)
    7  prescaled 1 -> sweeps -> prescaled 0 -> sweeps on one system (the pre-scaled table next to the dictionary's)
    8  CG in each of its three forms, and folded (cg_fold 1 and 2) on the table and on the planes."""
    c = new_census(oracle)
    for group in NEW_GROUPS:
        mine = [v for v in c.values() if v["group"] == group]
        drawn = {k: sum(1 for v in mine if k in v["kinds"]) for k in NEW_KINDS[group]}
        reached = {k: sum(1 for v in mine if k in v["orders"]) for k in NEW_ORDERS[group]}
        print(f"{group}: seeds that draw {drawn}; seeds that reach the orders {reached}")
        assert all(n >= 8 for n in drawn.values()), (group, drawn)
        assert all(n >= 4 for n in reached.values()), (group, reached)
    cg = [v for v in c.values() if v["group"] == "cgkey"]
    forms = {k: sum(1 for v in cg if k in v["kinds"]) for k in ["cg impl 1", "cg impl 2", "cg impl 3", "cg impl 1 fold 1", "cg impl 1 fold 2",
                                                                 "cg impl 3 fold 1", "cg impl 3 fold 2"]}
    print(f"cgkey: seeds that run {forms}")
    assert all(n >= 4 for n in forms.values()), forms
    omegas = set().union(*(v["pre_omegas"] for v in c.values() if v["group"] == "prescaled"))
    assert len(omegas) == 2, omegas
    # the even width on which a wall-column link can be represented, and stacks for the streams
    assert all(any(v["shape"][0] % 2 == 0 for v in c.values() if v["group"] == g) for g in NEW_GROUPS)
    # "fill_impl" 1 is never refused: one workgroup holds the fill bitmaps of every shape (api_fill.hip: fill_fits_one_workgroup,
    # ny rows of ceil(nx / 64) words within FILL_LARGE_WORDS = 8192); and nothing is larger than 256 x 130 cells
    for nx, ny in set(seq.NATIVE_SHAPES + seq.CGKEY_SHAPES):
        assert ny * ((nx + 63) // 64) <= 8192 and nx * ny <= 256 * 130, (nx, ny)


# ---------------------------------------------------------------------------------------------------------------------------
# The field adjoint's group.  Lambda's validity is worked out here from deff_amd.h's lifetime rule alone, independently of the
# draw's own bookkeeping, and the two have to agree: the draw offers the pass as a solve's first reader only while it is valid.

ADJ_INVALIDATORS = ("image", "native", "D/S", "stage", "stream", "cgstream")
ADJ_KINDS = ["adj", "adj on Sw", "adj max_iter 0", "adj max_iter 3", "adj zero image", "setadj", "getadj", "vjp", "vjp refused",
             "getadj refused"]
ADJ_ORDERS = (["A1"] + ["A2 " + k for k in ADJ_INVALIDATORS] + ["A3 cgstream refused", "A3 adj on Sw"]
              + ["A4 impl 1", "A4 impl 2", "A4 impl 3", "A4 cg adj cg", "A5", "A6", "A7 setadj adj", "A7 adj setadj vjp",
                 "A8 vjp sens", "A8 sens vjp"])


def adjoint_census(oracle):
    """Per seed of ADJOINT_SEEDS: `kinds` = which of ADJ_KINDS it draws, `orders` = which of ADJ_ORDERS it reaches."""
    out = {}
    g = seq.ADJOINT_SEEDS
    for i in range(g["count"]):
        seed, options = g["first"] + i, seq.seed_options(g)
        draw = seq.draw_sequence(seed, **options)
        _, nx, ny, B, _ = next(draw)
        pix = next(draw)[1]
        kinds, orders = set(), set()
        kind, asm, nrows = None, None, None
        keys = dict(cg_onchip=0, cg_planes=0, cg_fold=0, tb_impl=0, tb_launch=0)
        kset, keys_at_sweeps = "auto", None
        have_x = lam_valid = False
        planes_built = False                                 # of a native "2p" / "3n" system
        a1 = None                                            # after an adj that built those planes: what has followed it
        lost_by = refused = None                             # the invalidator that took a valid lambda / the refusal that left one
        a4 = None                                            # the CG forms that ran since the last adj, lambda still its
        hist = []                                            # every op drawn: (name, accepted)

        def rows():
            nonlocal nrows
            if nrows is None:
                nrows = distinct_rows(oracle, pix, *asm)
            return nrows

        def invalidate(by):
            nonlocal lam_valid, lost_by, a4, planes_built, a1
            if lam_valid:
                lost_by = by
            lam_valid, a4 = False, None
            if by != "image":
                planes_built, a1 = False, None

        for op, *a in draw:
            ok = True
            was_refused, refused = refused, None
            if op == "tune":
                if a[0] in keys:
                    keys[a[0]] = a[1]
                hist.append((op, True))
                refused = was_refused                        # (a key in between does not touch lambda)
                continue
            if op == "kernel":
                kset = a[0]
            elif op == "image":
                pix, kind = a[0], None
                invalidate("image")
            elif op in ("assemble", "stage"):
                if op == "stage":
                    a = ["3n"] + a + [None]
                invalidate("stage" if op == "stage" else "native" if a[0] in ("2p", "3p", "3n", "3g") else "D/S")
                if a[0] in ("D", "S", "Sw"):
                    kset = "auto"
                kind, asm, nrows = a[0], (a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7] if len(a) > 7 else None), None
            elif op in ("stream", "cgstream"):
                ok = not (op == "cgstream" and a[2] < 0)
                if ok:
                    invalidate(op)
                    kind, nrows, asm, have_x = "2p", 1, None, True
                elif lam_valid:
                    refused = "cgstream refused"
            elif op in ("init", "set_field"):
                have_x = True
            elif op == "cg":
                has_dict = kind in ("2p", "3n") or (kind != "Sw" and rows() <= 511)
                ok = kind != "Sw" and (has_dict or keys["cg_planes"] > 0)
                if ok:
                    impl = 3 if keys["cg_planes"] == 2 or not has_dict else seq.expected_cg_impl(nx, ny, keys["cg_onchip"])
                    if kind in ("2p", "3n") and impl == 3:
                        planes_built = True
                    if a4 is not None:
                        a4.add(impl)
                    if hist[-2:] == [("cg", True), ("adj", True)]:
                        orders.add("A4 cg adj cg")
                    if a1 is not None and impl in (1, 2):
                        a1.add("table")
                elif lam_valid:
                    refused = "cg on Sw" if kind == "Sw" else "cg without a dictionary"
            elif op == "sens":
                if lam_valid and kind in ("3n", "3g"):
                    refused = "sens on a Grid system"
                if hist[-1:] == [("vjp", True)]:
                    orders.add("A8 vjp sens")
            elif op == "getsys":
                if kind in ("2p", "3n"):
                    planes_built = True
                if a1 is not None:
                    a1.add("getsys")
            elif op in ("sweeps", "solve"):
                if kind in ("2p", "3n") and kset == "explicit":
                    planes_built = True
                if a1 is not None and kset != "explicit":
                    a1.add("table")
                if op == "sweeps":
                    keys_at_sweeps = (keys["tb_impl"], keys["tb_launch"])
                elif a[3] == "vjp":
                    assert lam_valid, (seed, "the pass drawn as a reader without a valid lambda")
                    kinds.add("vjp")
                    if B >= 2:
                        orders.add("A5")
                if op == "solve" and len(hist) >= 2 and hist[-2] == ("sweeps", True) and hist[-1] in (("adj", True), ("vjp", True)) \
                        and (keys["tb_impl"], keys["tb_launch"]) == (2, 0) and kset in ("auto", "matfree_tb") and kind != "Sw" \
                        and keys_at_sweeps == (2, 0):
                    orders.add("A6")
            elif op == "adj":
                ok = kind != "Sw"
                if not ok:
                    kinds.add("adj on Sw")
                    if lam_valid:
                        refused = "adj on Sw"
                else:
                    kinds.add("adj")
                    if a[2] in (0, 3):
                        kinds.add(f"adj max_iter {a[2]}")
                    if B >= 2 and any(not w.any() for w in a[0]):
                        kinds.add("adj zero image")
                    if kind in ("2p", "3n") and not planes_built:
                        planes_built, a1 = True, set()
                    if hist[-1:] == [("setadj", True)]:
                        orders.add("A7 setadj adj")
                    lam_valid, lost_by, a4 = True, None, set()
            elif op == "setadj":
                kinds.add("setadj")
                lam_valid, lost_by, a4 = True, None, None
            elif op == "getadj":
                ok = lam_valid
                kinds.add("getadj" if ok else "getadj refused")
                if ok and was_refused in ("cgstream refused", "adj on Sw"):
                    orders.add("A3 " + was_refused)
                if ok and a4:
                    orders.update("A4 impl %d" % k for k in a4)
                if not ok and lost_by:
                    orders.add("A2 " + lost_by)
                    lost_by = None
            elif op == "vjp":
                ok = lam_valid and have_x
                kinds.add("vjp" if ok else "vjp refused")
                if ok and hist[-2:] == [("adj", True), ("setadj", True)]:
                    orders.add("A7 adj setadj vjp")
                if ok and hist[-1:] == [("sens", True)]:
                    orders.add("A8 sens vjp")
                if not lam_valid and lost_by:
                    orders.add("A2 " + lost_by)
                    lost_by = None
            if a1 is not None and a1 == {"table", "getsys"}:
                orders.add("A1")
            hist.append((op, ok))
        out[seed] = dict(kinds=kinds, orders=orders, shape=(nx, ny), B=B)
    return out


def test_the_adjoint_seeds_reach_what_they_were_added_for(oracle):
    """Every kind of the adjoint's ops is drawn by at least 8 seeds and at least 4 seeds reach each of
    A1  adj is the first call that needs the planes of a native "2p" / "3n" system; a sweep, solve or CG on the row table and
        deff_get_system follow on that system
    A2  a valid lambda, an invalidator (counted per kind: a new image, a native assembly, a caller's plane or system, a
        continuation stage, a stream, a CG stream), then getadj or vjp, refused
    A3  a valid lambda, a refused call (a CG stream with Df = -1; adj on wall-column links), then getadj
    A4  adj, CG (counted per form), then getadj with lambda still that solve's; and cg, adj, cg in a row
    A5  a solve of a stack (B >= 2) whose first reader is the pass
    A6  sweeps, adj or vjp, a solve in a row under tb_impl 2 / tb_launch 0, with the conditions of order 6 above
    A7  setadj then adj; adj, setadj, vjp in a row
    A8  vjp then the gradient (which reads the pass's device map afterwards); the gradient then vjp (which reads the gradient's)."""
    c = adjoint_census(oracle)
    drawn = {k: sum(1 for v in c.values() if k in v["kinds"]) for k in ADJ_KINDS}
    reached = {k: sum(1 for v in c.values() if k in v["orders"]) for k in ADJ_ORDERS}
    print(f"adjoint: seeds that draw {drawn}; seeds that reach the orders {reached}")
    assert all(n >= 8 for n in drawn.values()), drawn
    assert all(n >= 4 for n in reached.values()), reached
    assert any(v["shape"][0] % 2 == 0 for v in c.values()) and any(v["shape"][0] % 2 == 1 for v in c.values())
    for nx, ny in seq.CGKEY_SHAPES:
        assert nx * ny <= 256 * 130, (nx, ny)


def test_the_adjoint_seeds_draw_what_they_drew_before_the_second_order_options():
    """ADJOINT_SEEDS, recorded (draw_log with every_array) before the draw gained `tangent`, `second`, `fluxfield` and
    `onchip_planes`: with those off the generator is consumed as it was."""
    with open(os.path.join(GOLDEN, "sequence_draws_adjoint_seeds.json")) as f:
        recorded = json.load(f)
    g = seq.ADJOINT_SEEDS
    assert len(recorded) == g["count"] == 40
    for seed in range(g["first"], g["first"] + g["count"]):
        log, digest = draw_log(seed, every_array=True, **seq.seed_options(g))
        assert "|".join(log) == recorded[str(seed)]["log"], seed
        assert digest == recorded[str(seed)]["data"], seed


# ---------------------------------------------------------------------------------------------------------------------------
# The second-order group.  The five validity facts (lambda, the tangent's right-hand side and dx, dlambda's right-hand side and
# dlambda) and the existence of flux maps are worked out here from deff_amd.h's lifetime rules alone, independently of the
# draw's own bookkeeping; `predicted` is what the model of run_sequence() will expect of every call (accepted or refused).

KEY_OPS = ("tune", "kernel")
SIDE_SOLVES = ("adj", "tan", "atan")
SO_INVALIDATORS = ("image", "native", "D/S", "stage", "stream", "cgstream")
SO_KINDS = (["trhs", "trhs dD = D", "tan", "tan refused", "tan max_iter 0", "tan max_iter 3", "settan", "gettan", "gettan refused",
             "hvp", "hvp refused", "hvp CR == CL", "arhs", "arhs refused", "atan", "atan refused", "atan max_iter 0", "atan max_iter 3",
             "setatan", "getatan", "getatan refused", "fhvp", "fhvp refused", "ff", "ff image ok", "ff image EINVAL", "ff image ESTATE",
             "ffptr", "ffptr refused", "flux_kt 0", "flux_kt 1", "flux_kt 2", "cg_onchip_planes 0", "cg_onchip_planes 1",
             "side impl 3", "side impl 4", "side impl 3 under the key", "cg impl 4", "solve then trhs", "solve then ff"])
SO_ORDERS = (["T1 tangent one image", "T1 tangent stack", "T1 second one image", "T1 second stack"]
             + ["T2 " + k for k in SO_INVALIDATORS] + ["T2 tan without a right-hand side"]
             + ["T3 getatan", "T3 fhvp", "T3 atan", "T3 dx stays"]
             + ["T4 cgstream", "T4 tan on Sw", "T4 adj on Sw", "T4 hvp walls", "T4 ff on 3n"]
             + ["T5 tan cgform cg gettan", "T5 cg tan cg"]
             + ["T6 %s %s" % (a, b) for a in SIDE_SOLVES for b in SIDE_SOLVES if a != b]
             + ["T7", "T8 resident trhs", "T8 resident ff", "T8 stack trhs", "T8 stack ff", "T9 image ff", "T9 2p D ff", "T9 3p 3n 3p ff",
                "T10 eligible", "T10 ineligible", "T11 settan hvp", "T11 setatan fhvp", "T12 tan", "T12 atan"])
# orders the weights cannot make common: held by a directed GPU test of test_gpu_sequences.py, by construction
SO_DIRECTED = {"T9 3p 3n 3p ff": "test_the_image_forms_follow_the_assembly_sequence_and_a_new_image",
               "T9 2p D ff": "test_the_image_forms_follow_the_assembly_sequence_and_a_new_image"}


def second_order_census(oracle, lambda_keeps_dlambda=False):
    """Per seed of SECOND_ORDER_SEEDS: `kinds` it draws (of SO_KINDS), `orders` it reaches (of SO_ORDERS) and `predicted`, the
    (step, op, accepted) of every second-order call.  `lambda_keeps_dlambda` flips one rule of the model -- "a new lambda does
    not invalidate dlambda" -- to show that the flag checks bite: the seeds on which `predicted` then differs are the ones
    whose GPU run tells the two models apart."""
    out = {}
    g = seq.SECOND_ORDER_SEEDS
    for i in range(g["count"]):
        seed, options = g["first"] + i, seq.seed_options(g)
        draw = seq.draw_sequence(seed, **options)
        _, nx, ny, B, _ = next(draw)
        pix = next(draw)[1]
        eligible = (nx + (nx & 1)) * ny <= seq.ONCHIP_LIMIT
        kinds, orders, predicted = set(), set(), []
        kind, asm, nrows, prev_asm = None, None, None, None
        keys = dict(cg_onchip=0, cg_planes=0, cg_fold=0, tb_impl=0, tb_launch=0, cg_onchip_planes=0, flux_kt=0)
        kset, keys_at_sweeps = "auto", None
        have_x = lam = tan_rhs = tan = atan_rhs = atan = ff_have = False
        dx_src = dl_src = None                               # "set", "solve" or "partial": where the valid vector came from
        lost_by = None                                       # the invalidator that took a valid dx or dlambda
        t3 = False                                           # a new lambda took a valid dlambda; no new right-hand side yet
        last_solve = None                                    # the last accepted side solve since an invalidator
        rhs_key = {}                                         # "cg_onchip_planes" when the right-hand side of tan / atan was made
        hist = []                                            # (op, accepted, keys set since the op before) of every op that is no key
        since = set()

        def rows():
            nonlocal nrows
            if nrows is None:
                nrows = distinct_rows(oracle, pix, *asm)
            return nrows

        def invalidate(by):
            nonlocal lam, tan_rhs, tan, atan_rhs, atan, lost_by, t3, last_solve, dx_src, dl_src
            if tan or atan:
                lost_by = by
            lam = tan_rhs = tan = atan_rhs = atan = t3 = False
            last_solve = dx_src = dl_src = None

        def new_lambda():
            nonlocal atan_rhs, atan, t3, dl_src
            if lambda_keeps_dlambda:
                return
            t3 = t3 or atan
            atan_rhs = atan = False
            dl_src = None

        def side_solved(which):
            nonlocal last_solve
            impl = 4 if keys["cg_onchip_planes"] == 1 and eligible else 3
            kinds.add("side impl %d" % impl)
            if impl == 3 and keys["cg_onchip_planes"] == 1:
                kinds.add("side impl 3 under the key")
            if last_solve is not None and last_solve != which:
                orders.add("T6 %s %s" % (last_solve, which))
            last_solve = which

        for step, (op, *a) in enumerate(draw):
            ok = True
            if op == "tune":
                if a[0] in keys:
                    keys[a[0]] = a[1]
                if a[0] in ("flux_kt", "cg_onchip_planes"):
                    kinds.add(f"{a[0]} {a[1]}")
                since.add(a[0])
                continue
            if op == "kernel":
                kset = a[0]
                continue
            ops3 = [h[0] for h in hist[-3:]]
            oks3 = all(h[1] for h in hist[-3:])
            if op == "image":
                pix, kind, prev_asm = a[0], None, None
                invalidate("image")
            elif op in ("assemble", "stage"):
                if op == "stage":
                    a = ["3n"] + a + [None]
                invalidate("stage" if op == "stage" else "native" if a[0] in ("2p", "3p", "3n", "3g") else "D/S")
                if a[0] in ("D", "S", "Sw"):
                    kset = "auto"
                prev_asm = (prev_asm or ()) + (a[0],)
                kind, asm, nrows = a[0], (a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7] if len(a) > 7 else None), None
            elif op in ("stream", "cgstream"):
                ok = not (op == "cgstream" and a[2] < 0)
                if ok:
                    invalidate(op)
                    kind, nrows, asm, have_x, prev_asm = "2p", 1, None, True, None
                elif tan or atan:
                    orders.add("T4 cgstream")
            elif op in ("init", "set_field"):
                have_x = True
            elif op == "cg":
                has_dict = kind in ("2p", "3n") or (kind != "Sw" and rows() <= 511)
                ok = kind != "Sw" and (has_dict or keys["cg_planes"] > 0)
                if ok:
                    plane = keys["cg_planes"] == 2 or not has_dict
                    if plane and keys["cg_onchip_planes"] == 1 and eligible:
                        kinds.add("cg impl 4")
                    if ops3[-2:] == ["cg", "tan"] and all(h[1] for h in hist[-2:]):
                        orders.add("T5 cg tan cg")
            elif op in ("sweeps", "solve"):
                if op == "sweeps":
                    keys_at_sweeps = (keys["tb_impl"], keys["tb_launch"])
                else:
                    resident = (keys["tb_impl"], keys["tb_launch"]) == (2, 0) and kset in ("auto", "matfree_tb") and kind != "Sw" \
                        and keys_at_sweeps == (2, 0)
                    if resident and len(hist) >= 2 and hist[-2][0] == "sweeps" and hist[-1][:2] in (("trhs", True), ("ff", True)):
                        orders.add("T8 resident " + hist[-1][0])
                    if a[3] == "vjp":
                        assert lam, (seed, "the pass drawn as a reader without a valid lambda")
                    if a[3] in ("trhs", "ff"):
                        kinds.add("solve then " + a[3])
                        if B >= 2:
                            orders.add("T8 stack " + a[3])
                        if a[3] == "trhs":
                            tan_rhs, rhs_key["tan"] = True, keys["cg_onchip_planes"]
                        else:
                            ff_have = True
            elif op == "adj":
                ok = kind != "Sw"
                if ok:
                    lam = True
                    new_lambda()
                    side_solved("adj")
                elif tan or atan:
                    orders.add("T4 adj on Sw")
            elif op == "setadj":
                lam = True
                new_lambda()
            elif op == "vjp":
                ok = lam and have_x
            elif op == "trhs":
                ok = have_x
                if ok:
                    tan_rhs, rhs_key["tan"] = True, keys["cg_onchip_planes"]
                    if a[1] is None:
                        kinds.add("trhs dD = D")
            elif op == "arhs":
                ok = lam
                if ok:
                    atan_rhs, atan, t3, dl_src, rhs_key["atan"] = True, False, False, None, keys["cg_onchip_planes"]
            elif op in ("tan", "atan"):
                rhs = tan_rhs if op == "tan" else atan_rhs
                ok = kind not in (None, "Sw") and rhs
                if ok:
                    src = "partial" if a[1] in (0, 3) else "solve"
                    if a[1] in (0, 3):
                        kinds.add(f"{op} max_iter {a[1]}")
                    if op == "tan":
                        tan, dx_src = True, src
                    else:
                        atan, dl_src = True, src
                    side_solved(op)
                    if hist and hist[-1][:2] == ({"tan": "trhs", "atan": "arhs"}[op], True) and "cg_onchip_planes" in since \
                            and rhs_key[op] != keys["cg_onchip_planes"]:
                        orders.add("T10 eligible" if eligible else "T10 ineligible")
                else:
                    if kind == "Sw" and (tan or atan):
                        orders.add("T4 tan on Sw")
                    if not rhs and lost_by:
                        orders.update(["T2 " + lost_by, "T2 tan without a right-hand side"] if op == "tan" else ["T2 " + lost_by])
                    if op == "atan" and t3 and not rhs:
                        orders.add("T3 atan")
            elif op == "settan":
                tan, dx_src = True, "set"
            elif op == "setatan":
                atan, dl_src, t3 = True, "set", False
            elif op in ("gettan", "getatan"):
                ok = tan if op == "gettan" else atan
                if not ok and lost_by:
                    orders.add("T2 " + lost_by)
                if op == "getatan" and not ok and t3:
                    orders.add("T3 getatan")
                if op == "gettan" and ok and t3:
                    orders.add("T3 dx stays")
                if op == "gettan" and ok and ops3[-2:] == ["tan", "cg"] and all(h[1] for h in hist[-2:]) \
                        and {"cg_onchip", "cg_planes", "cg_fold"} <= hist[-1][2]:
                    orders.add("T5 tan cgform cg gettan")
            elif op == "hvp":
                ok = have_x and tan and a[2] != a[3]
                if a[2] == a[3]:
                    kinds.add("hvp CR == CL")
                    if have_x and tan:
                        orders.add("T4 hvp walls")
                if not tan and lost_by:
                    orders.add("T2 " + lost_by)
                if ok and ops3 == ["trhs", "tan", "gettan"] and oks3:
                    orders.add("T1 tangent " + ("one image" if B == 1 else "stack"))
                if ok and dx_src == "set":
                    orders.add("T11 settan hvp")
                if ok and dx_src == "partial":
                    orders.add("T12 tan")
            elif op == "fhvp":
                ok = have_x and lam and tan and atan
                if not ok and lost_by and not (tan and atan):
                    orders.add("T2 " + lost_by)
                if not atan and t3:
                    orders.add("T3 fhvp")
                if ok and ops3 == ["adj", "arhs", "atan"] and oks3:
                    orders.add("T1 second " + ("one image" if B == 1 else "stack"))
                if ok and dl_src == "set":
                    orders.add("T11 setatan fhvp")
                if ok and dx_src == "partial":
                    orders.add("T12 tan")
                if ok and dl_src == "partial":
                    orders.add("T12 atan")
            elif op == "ff":
                ok = have_x
                if ok:
                    ff_have = True
                    form = "ok" if kind in ("2p", "3p") else "EINVAL" if kind in ("3n", "3g") else "ESTATE"
                    kinds.add("ff image " + form)
                    if kind == "3n" and (tan or atan):
                        orders.add("T4 ff on 3n")
                    if kind is None and hist and hist[-1][0] == "image":
                        orders.add("T9 image ff")
                    if kind == "D" and prev_asm and prev_asm[-2:] == ("2p", "D"):
                        orders.add("T9 2p D ff")
                    if kind == "3p" and prev_asm and prev_asm[-3:] == ("3p", "3n", "3p"):
                        orders.add("T9 3p 3n 3p ff")
            elif op == "ffptr":
                ok = ff_have
            if op in ("trhs", "tan", "settan", "gettan", "hvp", "arhs", "atan", "setatan", "getatan", "fhvp", "ff", "ffptr"):
                kinds.add(op if ok else op + " refused")
                predicted.append((step, op, bool(ok)))
            if ok and op in seq.PASSES and len(hist) >= 2 and all(h[1] and h[0] in seq.PASSES for h in hist[-2:]) \
                    and len({op, hist[-1][0], hist[-2][0]}) == 3:
                orders.add("T7")
            if lost_by and op in ("tan", "settan", "atan", "setatan") and ok:
                lost_by = None
            hist.append((op, bool(ok), since))
            since = set()
        out[seed] = dict(kinds=kinds, orders=orders, predicted=predicted, shape=(nx, ny), B=B)
    return out


def test_the_second_order_seeds_reach_what_they_were_added_for(oracle):
    """Every kind of SO_KINDS is drawn and every order of SO_ORDERS is reached by at least one seed of SECOND_ORDER_SEEDS, or is
    held by the directed GPU test SO_DIRECTED names:
    T1   trhs, tan, gettan, hvp in a row, and adj, arhs, atan, fhvp, all accepted; on one image and on a stack
    T2   a valid dx or dlambda, an invalidator (counted per kind), then a getter, a pass or a side solve refused for it
    T3   a new lambda (adj, setadj) while dlambda is valid: getatan, fhvp and atan refused, gettan still accepted
    T4   a refused call while dx or dlambda is valid: a CG stream with Df = -1, tan or adj on wall-column links, hvp with
         CR == CL, the image form of ff on a native 3-phase system
    T5   tan, the keys of a CG form, cg, gettan in a row; cg, tan, cg in a row
    T6   adj, tan and atan as consecutive accepted side solves on one system, in every order of two
    T7   three different accepted passes in a row (the shared upload scratch of two planes)
    T8   sweeps, trhs or ff, a solve in a row on resident workgroup tiles; a stack's solve whose first reader is trhs or ff
    T9   ff right after a new image; ff on a caller's plane assembled after "2p"; ff after "3p", "3n", "3p"
    T10  "cg_onchip_planes" changed between a right-hand side and its solve, on a shape that fits one compute unit and on one
         that does not
    T11  hvp with a caller's dx, fhvp with a caller's dlambda
    T12  a pass that uses the partial vector of a side solve stopped by max_iter 0 or 3."""
    c = second_order_census(oracle)
    drawn = {k: sum(1 for v in c.values() if k in v["kinds"]) for k in SO_KINDS}
    reached = {k: sum(1 for v in c.values() if k in v["orders"]) for k in SO_ORDERS}
    print(f"second order: seeds that draw {drawn}; seeds that reach the orders {reached}")
    assert all(n >= 1 for n in drawn.values()), {k: n for k, n in drawn.items() if n < 1}
    missing = [k for k, n in reached.items() if n < 1 and k not in SO_DIRECTED]
    assert not missing, (missing, reached)
    assert all(callable(getattr(seq, name)) for name in SO_DIRECTED.values())
    assert any(v["shape"][0] % 2 == 0 for v in c.values()) and any(v["shape"][0] % 2 == 1 for v in c.values())
    assert {v["B"] for v in c.values()} == {1, 2, 3}


# the seeds whose predictions change when the model is told that a new lambda leaves dlambda valid
FLIPPED_SEEDS = [11008, 11011, 11021, 11026, 11030, 11041]


def test_the_validity_checks_bite(oracle):
    """Without touching the library: a model with one rule flipped -- "a new lambda does not invalidate dlambda" -- predicts
    other outcomes (getatan, atan and fhvp accepted where deff_amd.h refuses them) on the seeds of FLIPPED_SEEDS, so a library
    that forgot that rule would fail there, and the library as it is would fail the flipped model."""
    right, flipped = second_order_census(oracle), second_order_census(oracle, lambda_keeps_dlambda=True)
    differ = sorted(seed for seed in right if right[seed]["predicted"] != flipped[seed]["predicted"])
    print(f"seeds that tell the two models apart: {differ}")
    for seed in differ:
        a, b = right[seed]["predicted"], flipped[seed]["predicted"]
        first = next(u for u, v in zip(a, b) if u != v)
        assert first[1] in ("getatan", "atan", "fhvp") and not first[2], (seed, first)
    assert differ == FLIPPED_SEEDS, differ
