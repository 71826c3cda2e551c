"""CPU: plan_step_pair (rlao_amd/csrc/common.hpp), the host function that decides which launches of aoenv_run_integrator take the
step behind them along (AOENV_OPT_STEP_PAIRS), compiled for the host and run through the loop of aoenv_run_integrator
(tests/native/step_pairs_driver.cpp) next to a brute-force stepping of the clock restated here (clock_subpixel and the whole-pixel
rounds, after OOPAO/Atmosphere.py:378-404): step k takes step k + 1 along if and only if k + 1 lies in the call and no layer makes
a round or crosses a pixel in it; the accumulators handed out for the second step are the brute-force ones, bit for bit; and no
covered step's real clock ever crosses."""
import os
import shutil
import subprocess

import numpy as np
import pytest


def _r(px, deg):
    return (float(px * np.cos(np.deg2rad(deg))), float(px * np.sin(np.deg2rad(deg))))


# pixels per frame of every layer
WINDS = {
    "C2": [_r(0.3, 72.0)],                                         # 10 m/s at 72 deg, 8 m over 120 pixels, 500 Hz
    "C5": [_r(0.3, 0.0), _r(0.36, 72.0), _r(0.33, 144.0)],
    "calm_layer": [_r(0.3, 72.0), (0.0, 0.0)],
    "negative": [_r(0.41, 200.0), _r(0.17, -45.0)],
    "0.84": [(0.84, 0.0)],
    "0.84_diagonal": [_r(0.84, 250.0)],
    "integer": [(1.0, 0.0)],                                       # a whole-pixel round in every step: never pairs
    "integer_and_slow": [(0.1, 0.05), (-2.0, 0.25)],
    "calm": [(0.0, 0.0)],                                          # every step quiet: every launch a pair
}
N_TOTAL = 2000
CALLS = {"long": (2000, 1), "n1": (1, 40), "n2": (2, 40), "n3": (3, 40), "n7": (7, 30)}


def _brute(ratios, n):
    """per step: does any layer make a round or cross a pixel; and the accumulators after the step"""
    ratio = np.array(ratios, dtype=np.float64)
    buff = np.zeros_like(ratio)
    busy, after = [], []
    rounds = bool((np.abs(ratio).astype(int) > 0).any())
    for _ in range(n):
        buff = buff + np.fmod(np.abs(ratio), 1.0) * np.sign(ratio)
        cross = bool((np.abs(buff) >= 1).any())
        buff = np.fmod(np.abs(buff), 1.0) * np.sign(buff)
        busy.append(rounds or cross)
        after.append(buff.copy())
    return busy, after


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path_factory.mktemp("pairs") / "step_pairs_driver"
    subprocess.run([hipcc, "-O1", "-std=c++17", "-x", "hip", "--cuda-host-only", f"-I{repo}/include", f"-I{repo}/rlao_amd/csrc",
                    os.path.join(repo, "tests", "native", "step_pairs_driver.cpp"), "-o", str(exe)], check=True, capture_output=True)
    cases = [(w, c) for w in WINDS for c in CALLS]
    text = "".join(f"{len(WINDS[w])} {CALLS[c][0]} {CALLS[c][1]} " + " ".join(f"{x!r} {y!r}" for x, y in WINDS[w]) + "\n" for w, c in cases)
    out = subprocess.run([str(exe)], input=text, text=True, capture_output=True, check=True)
    blocks = []
    for line in out.stdout.strip().splitlines():
        tag, *v = line.split()
        if tag == "C":
            blocks.append({"launches": [], "bad": [], "ends": None})
        elif tag == "L":
            blocks[-1]["launches"].append({"call": int(v[0]), "k": int(v[1]), "pair": int(v[2]), "buff2": {}})
        elif tag == "b":
            blocks[-1]["launches"][-1]["buff2"][int(v[0])] = (float(v[1]), float(v[2]))
        elif tag == "X":
            blocks[-1]["bad"].append(v)
        elif tag == "E":
            blocks[-1]["ends"] = [int(x) for x in v]
    assert len(blocks) == len(cases)
    return dict(zip(cases, blocks))


@pytest.mark.parametrize("wind", list(WINDS))
@pytest.mark.parametrize("calls", list(CALLS))
def test_plan_is_the_brute_force_pairing(driver, wind, calls):
    blk = driver[(wind, calls)]
    n, n_calls = CALLS[calls]
    busy, after = _brute(WINDS[wind], n * n_calls)
    assert not blk["bad"], "a covered step's real clock crossed a pixel"
    it = iter(blk["launches"])
    pairs = 0
    for c in range(n_calls):
        k = 0
        while k < n:
            la = next(it)
            g = c * n + k                                           # the step's index from rest
            want = k + 1 < n and not busy[g + 1]                    # (step k itself may cross)
            assert (la["call"], la["k"], la["pair"]) == (c, k, int(want)), (wind, calls, c, k)
            if want:
                pairs += 1
                for l, b in la["buff2"].items():
                    assert b == tuple(after[g + 1][l]), (wind, calls, c, k, l)
                assert len(la["buff2"]) == len(WINDS[wind])
            k += 2 if want else 1
    assert next(it, None) is None
    assert blk["ends"] == [0, 0, 0, 0]                              # not eligible; n_steps = 1; the call's last step; k < 0
    if wind.startswith("integer") or n == 1:
        assert pairs == 0
    if wind == "calm":
        assert pairs == n_calls * (n // 2)
    if calls == "long" and wind == "C2":
        assert 0.55 < (n - pairs) / n < 0.60                       # launches per step at the headline's wind
