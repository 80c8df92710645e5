"""The pre-scaled streaming kernel, k_sweep_matfree_tb_pre<T> (kernels_tb.hpp), and the pre-scaled single-sweep kernel,
k_sweep_matfree_pre<R> (kernels_sweep.hpp), checked on what hipcc emits for gfx950.  No GPU needed: one small file per T that
instantiates the new kernel beside k_sweep_matfree_tb<T, true, false> -- the contracted arithmetic, the lighter of the two
existing ones -- is compiled to assembly with the Makefile's flags, in the style of tests/test_tb_stream_isa.py.

 - occupancy not below, scratch not above the contracted instantiation of the same T;
 - the steady-state loops (four: strips with and without the b' lookup, on the dealt and on the undealt path) hold 10 * 3 * T
   FP64 fused multiply-adds (v_fma_f64, or its accumulating encoding v_fmac_f64) -- five per cell, two cells per lane, three
   steps of T levels per group -- and no v_mul_f64 / v_add_f64: the arithmetic is five FMAs and nothing else;
 - one branch (the back edge), no select, no wait with vmcnt(0) in those loops;
 - the single-sweep kernel: no scratch, occupancy >= 4."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]        # csrc/Makefile: CXXFLAGS (without the warnings)
TB_ARGS = """(const double *, const uint16_t *, const double *, double *, int,
    int, int, int, int, int, int, const uint8_t *, int, int, int, int, int, int, int, int, int, double, unsigned long long *,
    const int4 *);
"""
INSTANCE = ('#include "kernels_tb.hpp"\n'
            "template __global__ void deff::k_sweep_matfree_tb_pre<%(T)d>" + TB_ARGS +
            "template __global__ void deff::k_sweep_matfree_tb<%(T)d, true, false>" + TB_ARGS +
            "template __global__ void deff::k_sweep_matfree_pre<4>(const double *, const uint16_t *, const double *, double *, int, int,\n"
            "    int, int, const uint8_t *, int, int, int, int, double);\n")
PRE, FMA, SINGLE = "k_sweep_matfree_tb_pre", "k_sweep_matfree_tbI", "k_sweep_matfree_preI"

FMA64 = r"^v_fmac?_f64(_e32|_e64)?\s"
BRANCH = re.compile(r"^s_(c?branch|setpc|call)")
VMCNT = re.compile(r"vmcnt\((\d+)\)")


@pytest.fixture(scope="module", params=[8, 6, 4])
def compiled(request, tmp_path_factory):
    """(T, {function symbol: its assembly lines}, {function symbol: resource figures})"""
    T = request.param
    d = tmp_path_factory.mktemp(f"pre_isa_T{T}")
    src = d / "instance.hip"
    src.write_text(INSTANCE % {"T": T})
    asm = d / "instance.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *FLAGS, "--cuda-device-only", "-S", "-I", CSRC,
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(asm), str(src)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    funcs, name = {}, None
    for ln in asm.read_text().splitlines():
        m = re.match(r"^(_ZN4deff\w+):", ln)
        if m:
            name = m.group(1)
            funcs[name] = []
        elif ln.startswith(".Lfunc_end"):
            name = None
        elif name is not None:
            code = ln.split(";")[0].strip()
            if code:
                funcs[name].append(code)
    usage, name = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", ln)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return T, funcs, usage


def one(table, part):
    hits = [v for k, v in table.items() if part in k]
    assert len(hits) == 1, (part, list(table))
    return hits[0]


def innermost_loops(lines):
    at = {ln[:-1]: i for i, ln in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:$", ln)}
    ends = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^s_c?branch\w*\s+(\.LBB\d+_\d+)$", ln)
        if m and m.group(1) in at and at[m.group(1)] < i:
            ends[at[m.group(1)]] = i
    loops = [(a + 1, b + 1) for a, b in ends.items()]
    inner = [(a, b) for a, b in loops if not any((c, d) != (a, b) and a <= c and d <= b for c, d in loops)]
    return [lines[a:b] for a, b in inner]


def count(body, pattern):
    return sum(1 for ln in body if re.match(pattern, ln))


def test_resources_not_worse_than_the_contracted_kernel(compiled):
    T, _, usage = compiled
    pre, fma = one(usage, PRE), one(usage, FMA)
    print(f"T={T}: pre-scaled {pre}, contracted {fma}")
    assert pre["Occupancy"] >= fma["Occupancy"] and pre["ScratchSize"] <= fma["ScratchSize"], (pre, fma)


def test_steady_state_loop_is_five_fmas_per_cell(compiled):
    T, funcs, _ = compiled
    loops = [b for b in innermost_loops(one(funcs, PRE)) if count(b, FMA64) == 10 * 3 * T]
    print(f"T={T}: {len(loops)} steady-state loops; per loop: lines {[len(b) for b in loops]}, "
          f"ds_read_b64 {[count(b, r'^ds_read_b64') for b in loops]}")
    assert len(loops) == 4, "one steady-state loop per strip kind (with and without the b' lookup) and path (dealt, undealt)"
    for body in loops:
        assert count(body, r"^v_(mul|add)_f64\b") == 0
        branches = [ln for ln in body if BRANCH.match(ln)]
        assert len(branches) == 1, branches
        assert count(body, r"^v_cndmask") == 0
        waits = [int(VMCNT.search(ln).group(1)) for ln in body if ln.startswith("s_waitcnt") and VMCNT.search(ln)]
        assert waits and all(n > 0 for n in waits), waits
    # the strip without a wall column skips the b' lookups: 8 instead of 10 per level
    assert sorted(count(b, r"^ds_read_b64") for b in loops) == [8 * 3 * T] * 2 + [10 * 3 * T] * 2


def test_single_sweep_kernel_is_light(compiled):
    _, funcs, usage = compiled
    u = one(usage, SINGLE)
    print(f"k_sweep_matfree_pre<4>: {u}")
    assert u["ScratchSize"] == 0 and u["Occupancy"] >= 4, u
    body = one(funcs, SINGLE)
    assert count(body, FMA64) == 5 * 2 * 4 and count(body, r"^v_(mul|add)_f64\b") == 0
