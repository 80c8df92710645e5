"""The steady-state loop of the streaming kernel, k_sweep_matfree_tb<T, false, false> (kernels_tb.hpp), checked on the ISA hipcc
emits for gfx950.  No GPU needed: one small file per T that instantiates the kernel is compiled to assembly with the Makefile's
flags (seconds each).

What the loop is meant to be cannot be said in the source alone -- where hipcc puts the wait for the prefetched rows, and whether
it can count the operations in flight, is decided by its sinking and its waitcnt pass -- so it is pinned here as properties of
the emitted code.  The steady-state loops are the innermost loops whose body holds 22 * 3 * T FP64 instructions (one group =
3 steps x T levels x 22 operations per lane pair).  For each of them:

 1. one branch: the back edge;
 2. no wait forces a fresh store: walking the body cyclically with the vector-memory operations in issue order, what an
    `s_waitcnt vmcnt(N)` forces to complete is everything but the N youngest; no store in that set was issued fewer than T level
    fences (`; sched_barrier` markers) earlier, i.e. less than one step -- in particular no wait in the loop has vmcnt 0;
 3. prefetch distance: the first instruction that reads a register written by a row load comes at least 2 T level fences after
    that load, in the cyclic order;
 4. no select and no 64-bit per-lane address arithmetic.

Before the rows went through buffer descriptors the same kernel (global loads from clamped addresses, `ok ? v : 0` selects, stores
behind exec branches) read: (1) 5 branches (three around the stores, the loop's exit, the back edge); (2) vmcnt(0) one instruction behind step 2's store -- the selects of the prefetched
group had been sunk into the block behind that store, whose branch the waitcnt pass cannot count across; (4) 24 selects and 12
64-bit address instructions; (3) held, the rows being first read two steps after issue.  Buffer descriptors alone, with the
copy `cur = next` at the top of a group, fail (3): hipcc places the copies inside level 1 of step 0 and waits for the loads some
50 instructions after issuing them.

The resource remarks of the same compile pin the register budget of T = 8: at most 168 VGPRs, 3 waves per SIMD, and no more
scratch than the 28 B the kernel had before."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]        # csrc/Makefile: CXXFLAGS (without the warnings)
INSTANCE = """#include "kernels_tb.hpp"
template __global__ void deff::k_sweep_matfree_tb<%d, false, false>(const double *, const uint16_t *, const double *, double *, int,
    int, int, int, int, int, int, const uint8_t *, int, int, int, int, int, int, int, int, int, double, unsigned long long *,
    const int4 *);
"""

FP64 = re.compile(r"^v_(mul|add|fma)_f64\b")
VMEM = re.compile(r"^(buffer|global|flat|scratch)_(load|store|atomic)")
BRANCH = re.compile(r"^s_(c?branch|setpc|call)")
VMCNT = re.compile(r"vmcnt\((\d+)\)")
REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def regs_of(text):
    out = set()
    for m in REG.finditer(text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


@pytest.fixture(scope="module", params=[8, 6, 4])
def compiled(request, tmp_path_factory):
    """(T, assembly lines of the kernel, resource remarks)"""
    T = request.param
    d = tmp_path_factory.mktemp(f"tb_isa_T{T}")
    src = d / "instance.hip"
    src.write_text(INSTANCE % T)
    asm = d / "instance.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *FLAGS, "--cuda-device-only", "-S", "-I", CSRC,
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(asm), str(src)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # (a level fence is sched_barrier(0); the fences between the arithmetic stages inside a level carry a non-zero mask)
    lines = [ln.split(";")[0].strip() if "sched_barrier mask(0x00000000)" not in ln else "; sched_barrier" for ln in asm.read_text().splitlines()]
    return T, [ln for ln in lines if ln], r.stderr


def steady_loops(T, lines):
    """Bodies (label line excluded, back edge included) of the innermost loops with 22 * 3 * T FP64 instructions."""
    at = {ln[:-1]: i for i, ln in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:$", ln)}
    ends = {}                                                             # loop header -> its last back edge
    for i, ln in enumerate(lines):
        m = re.match(r"^s_c?branch\w*\s+(\.LBB\d+_\d+)$", ln)
        if m and m.group(1) in at and at[m.group(1)] < i:
            ends[at[m.group(1)]] = i
    loops = [(a + 1, b + 1) for a, b in ends.items()]
    inner = [(a, b) for a, b in loops if not any((c, d) != (a, b) and a <= c and d <= b for c, d in loops)]
    bodies = [lines[a:b] for a, b in inner]
    return [b for b in bodies if sum(1 for ln in b if FP64.match(ln)) == 22 * 3 * T]


def test_steady_state_loop(compiled):
    T, lines, _ = compiled
    loops = steady_loops(T, lines)
    assert loops, "no innermost loop with 22 * 3 * T FP64 instructions"
    for body in loops:
        fences = sum(1 for ln in body if ln == "; sched_barrier")
        assert fences == 3 * T, fences

        # 1. one branch
        branches = [ln for ln in body if BRANCH.match(ln)]
        print(f"T={T}: {len(body)} lines, branches {len(branches)}")
        assert len(branches) == 1, branches

        # 4. no selects, no 64-bit address arithmetic
        bad = [ln for ln in body if re.match(r"^v_(cndmask|lshl_add_u64|mad_i64_i32|mad_u64_u32)", ln)]
        print(f"T={T}: selects / 64-bit address instructions {len(bad)}")
        assert not bad, bad[:5]

        # 2. what each wait forces: the queue of vector-memory operations in flight, oldest first, as (is_store, fence count at issue)
        queue, fence, waits = [], 0, []
        for lap in range(3):
            for ln in body:
                if ln == "; sched_barrier":
                    fence += 1
                elif VMEM.match(ln):
                    queue.append(("store" in ln.split()[0], fence))
                elif ln.startswith("s_waitcnt") and VMCNT.search(ln):
                    n = int(VMCNT.search(ln).group(1))
                    forced, queue = queue[:max(len(queue) - n, 0)], queue[max(len(queue) - n, 0):]
                    if lap > 0:
                        waits.append((n, [fence - f for st, f in forced if st]))
        print(f"T={T}: vmcnt waits per lap (N, ages in fences of the stores forced): {waits[:len(waits) // 2]}")
        assert waits, "no vmcnt wait in the loop"
        for n, ages in waits:
            assert n > 0, "vmcnt(0) in the steady-state loop"
            assert all(a >= T for a in ages), (n, ages)

        # 3. prefetch distance: from each load to the first read of a register it wrote, in fences, cyclically
        two = body + body
        distances = []
        for i, ln in enumerate(body):
            if not (VMEM.match(ln) and "load" in ln.split()[0]):
                continue
            dst = regs_of(ln.split(",")[0])
            assert dst, ln
            seen = 0
            for later in two[i + 1:i + 1 + len(body)]:
                if later == "; sched_barrier":
                    seen += 1
                    continue
                ops = later.split(None, 1)
                if len(ops) < 2:
                    continue
                args = ops[1].split(",")
                # sources: every operand but the first; all of them for stores and for multiply-accumulates
                srcs = args if re.match(r"^((buffer|global|flat|scratch|ds)_(store|write)|v_fmac|v_mac)", ops[0]) else args[1:]
                if regs_of(",".join(srcs)) & dst:
                    break
                dst -= regs_of(args[0])                                  # overwritten before it was read: no longer the load's value
                if not dst:
                    break
            distances.append(seen)
        print(f"T={T}: fences between a row load and its first use: {distances}")
        assert len(distances) == 6, distances                           # 3 rows of x, 3 rows of codes
        assert all(dist >= 2 * T for dist in distances), distances


def test_register_budget(compiled):
    T, _, remarks = compiled
    got = {k.split(" ")[0]: int(v) for k, v in
           re.findall(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", remarks)}
    print(f"T={T}: {got}")
    assert set(got) == {"VGPRs", "ScratchSize", "Occupancy"}, remarks[-2000:]
    if T == 8:
        assert got["VGPRs"] <= 168 and got["Occupancy"] >= 3 and got["ScratchSize"] <= 28, got
    elif T == 6:
        assert got["Occupancy"] >= 3 and got["ScratchSize"] == 0, got      # (as tests/test_kernel_resources.py asks of every T = 6 kernel)
    else:
        assert got["VGPRs"] <= 128 and got["Occupancy"] >= 4 and got["ScratchSize"] == 0, got
