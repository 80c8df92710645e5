"""The on-chip conjugate-gradient kernel (kernels_cg_image.hpp, tuning key "cg_onchip") and the driver's --cg-batch, host
side: the kernel's register / scratch / LDS budget on the ISA hipcc emits for gfx950, the streaming CG kernels' unchanged
figures, and the option's refusals, which come before any device work.  No GPU needed."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "effectivediffusivityfvm_amd", "csrc")
EXE = os.path.join(ROOT, "effectivediffusivityfvm_amd", "deff2d")


def cg_usage():
    path = os.path.join(CSRC, "build", "api_cg.usage.txt")
    assert os.path.exists(path), "build/api_cg.usage.txt missing: api_cg.hip is not part of the build"
    usage, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return usage


def test_image_kernel_resources():
    """k_cg_image: one workgroup of 1024 threads per compute unit = 4 waves per SIMD = 128 VGPRs a lane, of which x, r and the
    codes of its 16 cells take 72; nothing may spill (the iteration runs out of registers and LDS alone), no AGPR, and the
    table + 128 KiB of p + the wave sums fit the CU's 160 KiB of LDS."""
    got = {k: v for k, v in cg_usage().items() if "10k_cg_image" in k}
    assert len(got) == 1, list(got)
    (name, u), = got.items()
    print(name, u)
    assert u["ScratchSize"] == 0 and u["AGPRs"] == 0, u
    assert u["VGPRs"] <= 128 and u["Occupancy"] >= 4, u
    assert 128 * 1024 < u["LDS"] <= 163840, u


def test_streaming_cg_kernels_are_unchanged():
    """The figures of the streaming kernels as they were before the on-chip kernel joined their translation unit."""
    want = {"8k_cg_dir": (54, 29120), "11k_cg_update": (70, 29120), "10k_cg_resid": (48, 29120), "15k_cg_admissible": (21, 29120),
            "10k_cg_alpha": (12, 32), "9k_cg_beta": (18, 32), "10k_cg_check": (27, 32)}
    seen = set()
    for name, u in cg_usage().items():
        for k, (vgprs, lds) in want.items():
            if name.startswith("_ZN4deff" + k + "E"):
                seen.add(k)
                assert (u["VGPRs"], u["LDS"], u["ScratchSize"], u["AGPRs"]) == (vgprs, lds, 0, 0), (name, u)
    assert seen == set(want)


def test_help_names_cg_batch():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--cg-batch" in r.stdout


def test_cg_batch_refusals(tmp_path):
    """Exit 2 with a message, before the input file is read or a device touched (there is no input.txt here, and no GPU)."""
    for args, word in ((["input.txt", "--cg-batch", "8"], "--solver cg"),
                       (["input.txt", "--solver", "cg", "--cg-batch", "-1"], "--cg-batch"),
                       (["input.txt", "--cg-batch", "-1", "--solver", "cg"], "--cg-batch"),
                       (["input.txt", "--solver", "cg", "--cg-batch", "many"], "--cg-batch"),
                       (["input.txt", "--solver", "cg", "--cg-batch", "8x"], "--cg-batch")):
        r = subprocess.run([EXE] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert word in r.stderr and not r.stdout, (args, r.stderr, r.stdout)
    assert not os.listdir(tmp_path)
