"""CPU: the host side of the control delay inside the library (aoenv_set_delay / BatchedAOEnv.set_delay).  The index arithmetic
of the delay line (rlao_amd/csrc/delay.hpp, the ONE source env.hip uses for every loop) is replayed by the stand-alone driver
tests/native/delay_driver.cpp and compared with a Python list FIFO -- the contract of the reference's TimeDelayEnv
(MAIN/PO4AO/util_simple.py:46-52: append, apply action_buffer[0], drop it); plus the ABI that goes with it, the refusals that need
no device and the wrappers.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from rlao_amd import _lib as L
from rlao_amd.wrappers import TorchWrapper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "aoenv.h")
NAMES = ("aoenv_set_delay", "aoenv_get_delay", "aoenv_get_delay_line", "aoenv_set_delay_line")


def _build(out_dir, sanitize=False):
    """The driver as a stand-alone host program (delay.hpp is plain C++); None when there is no compiler."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    if not (shutil.which(cxx) or os.path.exists(cxx)):
        return None
    exe = os.path.join(str(out_dir), "delay_driver" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([cxx, *flags, "-std=c++17", "-Wall", "-Werror", f"-I{REPO}/rlao_amd/csrc", os.path.join(REPO, "tests", "native", "delay_driver.cpp"),
                    "-o", exe], check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("delay"))
    if exe is None:
        pytest.skip("no C++ compiler")
    return exe


def _operations(d, seed, n_ops=60):
    """Random operations: pushes, recorded loops of n steps with n below, at and above d (0 and 1 included), clears.  Every
    issued action has an id of its own (> 0)."""
    rng = np.random.RandomState(seed)
    lengths = sorted({0, 1, max(d - 1, 0), d, d + 1, 2 * d + 3})
    ops, nxt = [], 1
    for i in range(n_ops):
        kind = "C" if i % 17 == 16 else rng.choice(["P", "L"], p=[0.4, 0.6])
        if kind == "P":
            ops.append(("P", [nxt]))
            nxt += 1
        elif kind == "L":
            n = int(lengths[rng.randint(len(lengths))])
            ops.append(("L", list(range(nxt, nxt + n))))
            nxt += n
        else:
            ops.append(("C", []))
    return ops


def _fifo(d, ops):
    """The checker: a Python list, used as TimeDelayEnv.step uses action_buffer.  Per operation (applied ids, the line)."""
    buf, out = [0] * d, []
    for kind, ids in ops:
        applied = []
        if kind == "C":
            buf = [0] * d
        for a in ids:
            buf.append(a)
            applied.append(buf[0])
            del buf[0]
        out.append((applied, list(buf)))
    return out


def _run(exe, d, ops, env=None):
    text = "\n".join(" ".join([k] + ([str(len(ids))] if k == "L" else []) + [str(i) for i in ids]) for k, ids in ops) + "\n"
    res = subprocess.run([exe, str(d)], input=text.encode(), capture_output=True, env=env)
    err = res.stderr.decode("utf-8", "replace")
    assert res.returncode == 0, (res.returncode, err)
    got = []
    for ln in res.stdout.decode().splitlines():
        a, b = ln.split("|")
        got.append(([int(x) for x in a.split()], [int(x) for x in b.split()]))
    return got, err


@pytest.mark.parametrize("d", range(9))
def test_driver_against_a_list_fifo(driver, d):
    """Every slot a step reads (the id it applies) and the logical order after every operation, three random sequences per delay;
    also the fixed sequence of the GPU test: a loop of 2 at d, a loop of 5, two steps, three steps."""
    for seed in range(3):
        ops = _operations(d, 100 * d + seed)
        got, _ = _run(driver, d, ops)
        want = _fifo(d, ops)
        assert len(got) == len(want) == len(ops)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, (d, seed, k, ops[k], g, w)
        assert {k for k, _ in ops} == {"P", "L", "C"}
    fixed = [("L", [1, 2]), ("L", [3, 4, 5, 6, 7]), ("P", [8]), ("P", [9]), ("P", [10]), ("P", [11]), ("P", [12])]
    assert _run(driver, d, fixed)[0] == _fifo(d, fixed)
    if d:
        assert _fifo(d, fixed)[0][0] == [0] * min(d, 2) + [1] * (d < 2)        # the checker itself delays


def test_driver_is_clean_under_asan_and_ubsan(tmp_path):
    """The same replay in a stand-alone sanitized program, run directly: a clean exit, no report, the same answers."""
    exe = _build(tmp_path, sanitize=True)
    if exe is None:
        pytest.skip("no C++ compiler")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for d in range(9):
        ops = _operations(d, 7 + d, n_ops=40)
        got, err = _run(exe, d, ops, env=env)
        assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
        assert got == _fifo(d, ops)


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_header_exports_and_binding_agree(tmp_path):
    prog = ['#include <stdio.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("abi %d\\ncount %d\\nseen %d\\nmax %d\\n", AOENV_ABI_VERSION, (int)AOENV_B_COUNT, (int)AOENV_B_COEFS_SEEN, AOENV_MAX_DELAY);',
            'printf("copt %d\\nck %d\\n", (int)AOENV_OPT_ENV_WIND_PIXELS, (int)AOENV_K_COUNT);', "return 0;}"]
    src, exe = tmp_path / "delay_abi.c", tmp_path / "delay_abi"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    out = {k: int(v) for k, v in (l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    # additive: the version and every enum stay where they were
    assert out == dict(abi=7, count=14, seen=13, max=8, copt=10, ck=13)
    assert L.ABI_VERSION == 7 and L.B_COEFS_SEEN == 13 and L.MAX_DELAY == 8
    text = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = L.load()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert lib.aoenv_abi_version() == 7
    for cite in ("util_simple.py:25-52", "mbrl_main.py:46", "mbrl_main_network.py:41", "mbrl_funcsRAZOR.py:32-33", "OOPAOEnv_VPG.py:562-566",
                 "modalAOEnv.py:150-154", "IM_delayEnv.py:164-165"):
        assert cite in text, cite
    # the checkpoint paragraph lists the line next to dm_prev
    para = text[text.index("State access (SURVEY.md"):text.index("int aoenv_buffer(")]
    assert "AOENV_B_DM_PREV" in para and "aoenv_get_delay_line" in para


def test_the_library_refuses_a_null_env():
    lib = L.load()
    buf = np.zeros(16)
    d = C.c_int(-5)
    calls = (lambda: lib.aoenv_set_delay(None, 1, None), lambda: lib.aoenv_get_delay(None, C.byref(d)),
             lambda: lib.aoenv_get_delay_line(None, buf.ctypes.data_as(C.c_void_p), buf.nbytes, None),
             lambda: lib.aoenv_set_delay_line(None, buf.ctypes.data_as(C.c_void_p), buf.nbytes, None))
    for call in calls:
        assert call() != 0
        assert b"null" in lib.aoenv_last_error()
    assert d.value == -5


class _StubEnv:
    """The batched env's surface as far as the wrappers use it: records what reaches it."""
    output = "torch"
    nActuator = 3
    n_envs = 4
    device = "cpu"
    tdtype = torch.float64

    def __init__(self):
        self.calls = []
        self.param = type("P", (), {"nLoop": 50})()
        self.delay = 0

    def set_delay(self, d):
        self.calls.append(("set_delay", d))
        self.delay = d

    def delay_line(self):
        return torch.full((self.delay, self.n_envs, 3, 3), 7.0)


def test_torch_wrapper_forwards_the_delay():
    inner = _StubEnv()
    env = TorchWrapper(inner)
    env.set_delay(2)
    assert inner.calls == [("set_delay", 2)] and env.delay == 2
    assert tuple(env.delay_line().shape) == (2, 4, 3, 3) and float(env.delay_line()[1, 3, 2, 2]) == 7.0


def test_the_env_surface():
    """``delay`` is a read-only property of the env (nothing in __init__ may shadow it), next to set_delay / delay_line."""
    from rlao_amd.env import BatchedAOEnv
    assert isinstance(BatchedAOEnv.delay, property) and BatchedAOEnv.delay.fset is None
    assert callable(BatchedAOEnv.set_delay) and callable(BatchedAOEnv.delay_line)
    src = open(os.path.join(REPO, "rlao_amd", "env.py")).read()
    assert not re.search(r"^\s*self\.delay\s*=", src, flags=re.M)
