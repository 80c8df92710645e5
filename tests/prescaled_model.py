"""ctypes binding of tests/cpp/prescaled_model.c: the CPU model of the pre-scaled five-FMA sweep (set_tuning("prescaled", 1)).

The model is built on first use as a shared object with -ffp-contract=off (and -mfma where the CPU has the instruction, so
that fma() is the hardware's correctly rounded one instead of libm's slower software path -- the same values either way).
The check loop (jacobi below) is the oracle's JacobiGPU restatement in Python around the model's sweeps, with the oracle's own
flux evaluation (oracle_binding.flux_deff)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import oracle_binding as ob

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "prescaled_model.c")
_LIB = None


def _cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(ln.startswith("flags") and " fma " in ln + " " for ln in f)
    except OSError:
        return False


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    flags = ["-O2", "-ffp-contract=off", "-fPIC", "-shared"] + (["-mfma"] if _cpu_has_fma() else [])
    out = os.path.join(HERE, "cpp", "libprescaled_model.so")
    if not (os.path.exists(out) and os.path.getmtime(out) >= os.path.getmtime(SRC)):
        if not os.access(os.path.dirname(out), os.W_OK):
            out = os.path.join(tempfile.mkdtemp(prefix="prescaled_model_"), "libprescaled_model.so")
        subprocess.run(["gcc", *flags, "-o", out, SRC, "-lm"], check=True)
    L = C.CDLL(out)
    dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    L.prescaled_table.argtypes = [dp, dp, C.c_long, C.c_double, dp, dp]
    L.prescaled_table.restype = None
    L.prescaled_sweeps.argtypes = [dp, dp, dp, dp, C.c_int, C.c_int, C.c_long, C.c_double]
    L.prescaled_sweeps.restype = None
    _LIB = L
    return L


def table(A, b, omega=ob.OMEGA_REF):
    """(Ap[n, 4], bp[n]) = the pre-scaled links and right-hand side of the oracle's system (A[n, 5], b[n])."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    Ap = np.empty((b.size, 4))
    bp = np.empty(b.size)
    lib().prescaled_table(A, b, b.size, omega, Ap, bp)
    return Ap, bp


def sweeps(A, b, x, nsweeps, omega=ob.OMEGA_REF, tab=None):
    """The field after nsweeps pre-scaled sweeps from x (ny, nx)."""
    Ap, bp = tab if tab is not None else table(A, b, omega)
    ny, nx = x.shape
    x = np.array(x, dtype=np.float64, order="C", copy=True)
    lib().prescaled_sweeps(Ap, bp, x, np.empty_like(x), nx, ny, int(nsweeps), omega)
    return x


def jacobi(A, b, x0, D, CL, CR, tol, max_iter, check_every=10000, omega=ob.OMEGA_REF):
    """oracle_binding.jacobi with the model's sweeps: (iters, deff_raw, conv, field, MFL, MFR).  The sweep with 0-based index
    k is followed by a check iff k % check_every == 0; deff is the value at the last check."""
    tab = table(A, b, omega)
    ny, nx = x0.shape
    x = np.array(x0, dtype=np.float64, order="C", copy=True)
    MFL, MFR = np.zeros(ny), np.zeros(ny)
    it, deff_new, deff_old, change, conv = 0, 1.0, 5.0, 100.0, 0.0
    while it < max_iter and tol < abs(change):
        nxt = ((it + check_every - 1) // check_every) * check_every      # index of the next sweep that is followed by a check
        n = nxt - it + 1 if nxt < max_iter else max_iter - it
        x = sweeps(None, None, x, n, omega, tab)
        it += n
        if nxt < max_iter:
            deff_new, MFL, MFR = ob.flux_deff(x, D, CL, CR)
            change = (deff_old - deff_new) / deff_old
            deff_old = deff_new
            conv = change
    return it, deff_new, conv, x, MFL, MFR
