"""CPU: the whole-pixel rounds of the atmosphere clock (rlao_amd/csrc/common.hpp: clock_rounds / clock_rounds_origin) -- ONE source
for the shared host clock (advance_atmosphere) and for the per-env device clocks above one pixel per frame (k_ring_round_env,
AOENV_OPT_ENV_WIND_PIXELS) -- compiled for the host and run next to the loops of the oracle's updateLayer
(oracle/ao_oracle.py OracleLayer.update, after OOPAO/Atmosphere.py:378-389), restated here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

CASES = [(1.18, 0.21), (0.0, -1.5), (1.59, -1.59), (-2.33, 2.33), (2.47, 1.425), (1.0, 0.0), (-2.0, 1.0), (0.4, 0.3),
         (7.9, -3.2), (-0.999, 4.0)]
N_STEPS = 50
S = 54                                                             # a torus size (N + 2); the origins wrap several times in 50 steps


def _oracle_rounds(ratio):
    """the two whole-pixel loops of OracleLayer.update: the direction of every add_row in front of the sub-pixel part"""
    ratio = np.asarray(ratio, dtype=np.float64)
    tmp = np.abs(ratio)
    tmp[np.isinf(tmp)] = 0
    nscr = tmp.astype(int)
    out = []
    for _ in range(nscr.min()):
        out.append(np.ones(2) * np.sign(ratio))
    for _ in range(nscr.max() - nscr.min()):
        step = np.ones(2) * np.sign(ratio)
        step[np.where(nscr == nscr.min())] = 0
        out.append(step)
    return out


def _oracle_subpixel(ratio, buff):
    ratio = np.asarray(ratio, dtype=np.float64)
    buff = buff + (np.abs(ratio) % 1) * np.sign(ratio)
    step = np.zeros(2)
    if np.abs(buff[0]) >= 1 or np.abs(buff[1]) >= 1:
        step = 1 * np.sign(buff)
        step[np.where(np.abs(buff) < 1)] = 0
    return step, (np.abs(buff) % 1) * np.sign(buff)


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path_factory.mktemp("rounds") / "clock_rounds_driver"
    subprocess.run([hipcc, "-O1", "-std=c++17", "-x", "hip", "--cuda-host-only", f"-I{repo}/include", f"-I{repo}/rlao_amd/csrc",
                    os.path.join(repo, "tests", "native", "clock_rounds_driver.cpp"), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], input="".join(f"{rx!r} {ry!r} {N_STEPS} {S}\n" for rx, ry in CASES), text=True,
                         capture_output=True, check=True)
    blocks, cur = [], None
    for line in out.stdout.strip().splitlines():
        tag, *v = line.split()
        if tag == "R":
            cur = {"mx": int(v[0]), "rounds": [], "steps": []}
            blocks.append(cur)
        elif tag == "r":
            cur["rounds"].append([int(x) for x in v])
        else:
            cur["steps"].append([int(x) for x in v])
    assert len(blocks) == len(CASES)
    return blocks


def test_round_count_and_directions_match_the_oracle_loops(driver_output):
    for ratio, blk in zip(CASES, driver_output):
        want = _oracle_rounds(ratio)
        assert blk["mx"] == len(want) == max(int(abs(ratio[0])), int(abs(ratio[1]))), ratio
        assert len(blk["rounds"]) == len(want) + 1
        oy = ox = 0
        for j, step in enumerate(want):
            jj, sx, sy, gy, gx = blk["rounds"][j]
            assert jj == j and (gy, gx) == (oy % S, ox % S), (ratio, j)      # origin after the j earlier rounds, closed form
            assert sx == step[0] and sy == step[1], (ratio, j)
            oy, ox = oy - sy, ox - sx                                        # a shift moves the origin the other way
        jj, sx, sy, gy, gx = blk["rounds"][-1]                               # past the last round: sits out, origin after all rounds
        assert (sx, sy) == (0, 0) and (gy, gx) == (oy % S, ox % S), ratio
    assert [b["mx"] for b in driver_output[:8]] == [1, 1, 1, 2, 2, 1, 2, 0]


def test_rounds_chained_with_the_subpixel_clock_move_as_far_as_the_oracle(driver_output):
    for ratio, blk in zip(CASES, driver_output):
        assert len(blk["steps"]) == N_STEPS
        buff = np.zeros(2)
        total = np.zeros(2)
        for i in range(N_STEPS):
            moved = sum(_oracle_rounds(ratio), np.zeros(2))
            step, buff = _oracle_subpixel(ratio, buff)
            moved = moved + step
            total += moved
            dx, dy, oy, ox = blk["steps"][i]
            assert dx == moved[0] and dy == moved[1], (ratio, i)
            assert (oy, ox) == (int(-total[1]) % S, int(-total[0]) % S), (ratio, i)
        # the clock moves |ratio| pixels per frame: after 50 frames within one pixel of 50 ratio, on each axis
        assert np.all(np.abs(total - N_STEPS * np.asarray(ratio)) < 1 + 1e-9), (ratio, total)
