"""What the random call sequences of test_gpu_sequences.py reach, counted without a GPU.

The draw of a sequence depends on the generator and on the model's state, never on what the GPU returns, so draw_sequence()
can be replayed here.  Two things are pinned: the 64 seeds that existed before the draw had options still draw what they
drew (tests/golden/sequence_draws_seeds_1000_2000.json: their op logs and a SHA-1 of every array they hand to the solver, in
call order.  The file was recorded from run_sequence() as it was before the draw was separated from it -- that function run
on a GPU with the Solver wrapped so that every array passed to set_image, assemble_from_D and set_field was hashed on its
way in, and its own log taken without the "refused" marks), and the seed ranges of the options reach the call orders they were added
for -- an option nobody draws, or a stream nobody reads after, would leave the GPU tests green and empty."""
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


def draw_log(seed, **options):
    """The op log run_sequence() writes (without what only a run can add: "refused", the CG form, the stream's early slots, the
    stamps' sweeps) and the digest of the arrays in the order the solver receives them."""
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
            if a[0] == "D":
                h.update(np.concatenate(a[6], axis=0).tobytes())
            log.append(f"assemble {a[0]} {a[1]} {a[2]} {a[4]}")
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
            log.append(f"{op} {a[0]} {a[1]} {a[2]}")
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
