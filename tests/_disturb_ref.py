"""Shared by tests/test_disturb_host.py (CPU) and tests/test_gpu_disturbance.py (GPU): the host driver of the disturbance model
(tests/native/disturb_driver.cpp over rlao_amd/csrc/disturb.hpp) and the model restated for one (mode, line) at a time."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(out_dir, sanitize=False):
    """Compiles the driver for the host; None when there is no hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    exe = os.path.join(str(out_dir), "disturb_driver" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([hipcc, *flags, "-std=c++17", "-x", "hip", "--cuda-host-only", f"-I{REPO}/include", f"-I{REPO}/rlao_amd/csrc",
                    os.path.join(REPO, "tests", "native", "disturb_driver.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def host_modes(exe, amp, freq, phase, taus, env=None):
    """float64 v[len(taus)][M] of the host driver; amp, freq (cycles per frame), phase [M][J]"""
    amp, freq, phase = (np.ascontiguousarray(x, dtype=np.float64) for x in (amp, freq, phase))
    M, J = amp.shape
    out = subprocess.run([exe, str(M), str(J), *(str(int(t)) for t in taus)], input=amp.tobytes() + freq.tobytes() + phase.tobytes(),
                         check=True, capture_output=True, env=env)
    v = np.frombuffer(out.stdout, dtype=np.float64)
    assert v.size == len(taus) * M, (v.size, out.stderr)
    return v.reshape(len(taus), M).copy(), out.stderr.decode("utf-8", "replace")


def numpy_lines(amp, freq, phase, tau):
    """The model in NumPy float64, term by term: amp sin(2 pi (x - floor(x))), x = freq tau + phase.  [M][J]"""
    x = freq * float(tau) + phase
    return amp * np.sin(2.0 * np.pi * (x - np.floor(x)))


def exact_phase_lines(amp, freq, phase, tau):
    """The same with the phase f tau + phi formed and reduced in exact rational arithmetic before NumPy's float64 sine: the
    checker for tau near 2^40, where the float64 product itself has lost the fraction of a cycle.  [M][J]"""
    out = np.empty_like(amp)
    for idx in np.ndindex(amp.shape):
        x = Fraction(float(freq[idx])) * int(tau) + Fraction(float(phase[idx]))
        out[idx] = amp[idx] * np.sin(2.0 * np.pi * float(x - (x.numerator // x.denominator)))
    return out


def line_tolerance(amp, freq, phase, tau):
    """Per line: amp (2 pi 2^-52 (|f| tau + |phi| + 1) + 4 2^-53): the rounding of the phase before floor, and the sines of two
    correct libraries.  [M][J]"""
    return amp * (2.0 * np.pi * 2.0 ** -52 * (np.abs(freq) * float(tau) + np.abs(phase) + 1.0) + 4.0 * 2.0 ** -53)
