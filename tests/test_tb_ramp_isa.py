"""The straight-line ramp of tb_strip (kernels_tb.hpp), checked on the ISA hipcc emits for gfx950, T = 8, in the one-pass kernel
and in the chained one.  No GPU needed; compiled and read through the helpers of tests/test_tb_stream_isa.py.

A tile whose window starts a full halo above its chunk runs its first 18 steps with exactly the levels 1 ... j / 2 in step j:
0 + 0 + 1 + 1 + ... + 8 + 8 = 72 level steps, 22 FP64 instructions each.  The ramp is found as what it is meant to be: a run
of instructions between two labels that holds exactly those 72 * 22 FP64 instructions.  Of each such run:

 1. no branch from its first row request to its last FP64 instruction -- not around a level, and none between the groups
    either (a chunk of one row already runs all six groups, kernels_tb.hpp says why);
 2. no scratch access;
 3. at least six rows of x requested before the first row is consumed (the `v_mov_b64` of the inline assembly that takes a
    row into the window), and that first wait leaves at least ten vector-memory operations in flight;
 4. one level fence per level step, so the levels stand in the order written."""
import re

import pytest

import test_tb_chain_isa as chained
import test_tb_stream_isa as one

T = 8
LEVEL_STEPS = sum(min(T, j // 2) for j in range(((2 * T + 2) // 3) * 3))


def ramps(lines):
    """Runs of lines between two labels with exactly LEVEL_STEPS * 22 FP64 instructions."""
    cuts = [i for i, ln in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:$", ln)] + [len(lines)]
    runs = [lines[a + 1:b] for a, b in zip(cuts, cuts[1:])]
    return [r for r in runs if sum(1 for ln in r if one.FP64.match(ln)) == 22 * LEVEL_STEPS]


@pytest.fixture(scope="module", params=["one_pass", "chained"])
def kernel(request, tmp_path_factory):
    text = one.INSTANCE % T if request.param == "one_pass" else chained.CHAIN
    lines, _ = chained.compile_instance(tmp_path_factory.mktemp(f"tb_ramp_{request.param}"), request.param, text)
    return request.param, lines


def test_ramp_is_straight_code_with_six_rows_in_flight(kernel):
    name, lines = kernel
    assert LEVEL_STEPS == 72
    found = ramps(lines)
    # wall strips and inner strips; the one-pass kernel has the ramp on its dealt path only
    assert len(found) == 2, (name, len(found))
    for run in found:
        # (the run may begin with the branch that chooses the ramp and end with the test that guards the loop)
        begin = next(i for i, ln in enumerate(run) if re.match(r"^buffer_load_dwordx4\b", ln))
        end = max(i for i, ln in enumerate(run) if one.FP64.match(ln))
        assert not [ln for ln in run[begin:end] if one.BRANCH.match(ln)], name
        run = run[begin:end + 1] + [ln for ln in run[end + 1:] if ln == "; sched_barrier"]
        assert not [ln for ln in run if re.match(r"^scratch_", ln)], name
        assert sum(1 for ln in run if ln == "; sched_barrier") == LEVEL_STEPS, name
        first_take = next(i for i, ln in enumerate(run) if re.match(r"^v_mov_b64\s", ln))
        before = run[:first_take]
        rows = sum(1 for ln in before if re.match(r"^buffer_load_dwordx4\b", ln))
        waits = [int(one.VMCNT.search(ln).group(1)) for ln in before if ln.startswith("s_waitcnt") and one.VMCNT.search(ln)]
        print(f"{name}: ramp of {len(run)} lines, {rows} rows requested before the first is consumed, waits before it {waits}")
        assert rows >= 6, (name, rows)
        assert waits and min(waits) >= 10, (name, waits)
        # every row of the ramp travels device-coherently in the chained kernel, plainly in the one-pass kernel
        sc1 = [bool(re.search(r"\bsc1\b", ln)) for ln in run if re.match(r"^buffer_(load|store)_dwordx4\b", ln)]
        assert sc1 and all(v == (name == "chained") for v in sc1), name


def test_without_the_ramp_the_chained_kernel_is_the_generic_one(tmp_path):
    """The measurement switch TB_STRAIGHT_RAMP = 0 (every tile through the generic trimmed groups: what the ramp is timed
    against) must keep building, with no ramp in it and the steady-state loops as test_tb_stream_isa.py asks."""
    lines, remarks = chained.compile_instance(tmp_path, "no_ramp", "#define TB_STRAIGHT_RAMP 0\n" + chained.CHAIN)
    assert not ramps(lines)
    assert len(one.steady_loops(T, lines)) == 2
    one.test_steady_state_loop((T, lines, remarks))
    got = chained.budget(remarks)
    assert got["VGPRs"] <= 168 and got["Occupancy"] >= 3 and got["ScratchSize"] <= 28, got
