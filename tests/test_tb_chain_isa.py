"""The chained streaming kernel, k_sweep_matfree_tb_chain<8, false, false> (kernels_tb.hpp), on the ISA hipcc emits for gfx950.
No GPU needed.  Its row loop is tb_strip with device-coherent rows inside a loop over passes; what tests/test_tb_stream_isa.py
asks of the one-pass kernel's steady-state loop must survive that -- the same checks run here on this kernel, through that
file's own code --, the register budget must still give 3 waves per SIMD with no more scratch than the one-pass kernel compiled
beside it, and the flag a tile publishes after a pass must stand behind a wait for ALL its stores: vmcnt(0), spelled out in the
source, because nothing else orders the flag after the rows."""
import re
import subprocess

import pytest

import test_tb_stream_isa as one

CHAIN = """#include "kernels_tb.hpp"
template __global__ void deff::k_sweep_matfree_tb_chain<8, false, false>(const double *, const uint16_t *, double *, double *, int, int,
    int, int, int, int, int, int, int, int, double, const int4 *, const unsigned *, unsigned *, int, unsigned *, unsigned, unsigned *,
    unsigned long long *);
"""


def compile_instance(d, name, text):
    src, asm = d / f"{name}.hip", d / f"{name}.s"
    src.write_text(text)
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *one.FLAGS, "--cuda-device-only", "-S", "-I", one.CSRC,
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(asm), str(src)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split(";")[0].strip() if "sched_barrier mask(0x00000000)" not in ln else "; sched_barrier" for ln in asm.read_text().splitlines()]
    return [ln for ln in lines if ln], r.stderr


def budget(remarks):
    got = {k.split(" ")[0]: int(v) for k, v in
           re.findall(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", remarks)}
    assert set(got) == {"VGPRs", "ScratchSize", "Occupancy"}, remarks[-2000:]
    return got


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    return compile_instance(tmp_path_factory.mktemp("tb_chain_isa"), "chain", CHAIN)


def test_steady_state_loop_of_the_chained_kernel(chain):
    lines, remarks = chain
    assert len(one.steady_loops(8, lines)) == 2                               # wall strips and inner strips
    one.test_steady_state_loop((8, lines, remarks))
    # ... and its rows really are device-coherent: every 16-byte row access carries sc1, the code loads do not
    rows = [ln for ln in lines if re.match(r"^buffer_(load|store)_dwordx4\b", ln)]
    assert rows and all(re.search(r"\bsc1\b", ln) for ln in rows), [ln for ln in rows if "sc1" not in ln][:3]
    codes = [ln for ln in lines if re.match(r"^buffer_load_dword\b", ln)]
    assert codes and not any(re.search(r"\bsc1\b", ln) for ln in codes)


def test_register_budget_of_the_chained_kernel(chain, tmp_path):
    _, remarks = chain
    got = budget(remarks)
    _, remarks1 = compile_instance(tmp_path, "one_pass", one.INSTANCE % 8)
    ref = budget(remarks1)
    print(f"chained {got}, one pass {ref}")
    assert got["VGPRs"] <= 168 and got["Occupancy"] >= 3 and got["ScratchSize"] <= ref["ScratchSize"], (got, ref)


def test_flag_is_stored_behind_a_wait_for_every_store(chain):
    lines, _ = chain
    flags = 0
    for i, ln in enumerate(lines):
        if not (re.match(r"^global_store_dword\b", ln) and re.search(r"\bsc1\b", ln)):
            continue                                                          # (agent-scope stores of one word: the flags, the abort word)
        back = lines[:i][::-1]
        k = next((j for j, b in enumerate(back) if re.match(r"^buffer_store_dwordx4\b", b)), None)
        if k is None:
            continue                                                          # in front of every row store: not a published pass
        between = back[:k]
        assert any(re.match(r"^s_waitcnt\b", b) and "vmcnt(0)" in b for b in between), (i, ln)
        flags += 1
    assert flags >= 2, flags                                                  # one per instantiation of the pass loop
