"""The sweep rule of the CG bodies (conjugategradient_amd/csrc/cgx_sweep.h,
sweep_dir) checked on the host: the header has no HIP dependency, so
examples/sweep_check.cpp compiles with g++ alone and runs without a GPU.

For 1, 2 and 3 launches per body over 16 consecutive bodies (slot = body & 3):
  * consecutive launches in stream order run in opposite directions, the step
    from slot 3 to slot 0 included;
  * three launches per body give slot & 1, 1 - (slot & 1), slot & 1: the rule
    the three-kernel bodies have always been launched with, written out here;
  * two launches per body give 0, 1 in every slot.
The program checks the first two itself (its exit status); the table it
prints is checked again here.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sweep") / "sweep_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "conjugategradient_amd", "csrc"),
                        os.path.join(ROOT, "examples", "sweep_check.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    rows = [tuple(int(v) for v in line.split()) for line in p.stdout.splitlines()]
    assert len(rows) == 16 * (1 + 2 + 3)
    return rows


@pytest.mark.parametrize("launches", [1, 2, 3])
def test_stream_order_alternates(table, launches):
    seq = [(body, slot, k, d) for L, body, slot, k, d in table if L == launches]
    # stream order: bodies 0 .. 15, launches 0 .. L - 1 of each
    assert [(b, k) for b, _, k, _ in seq] == [(b, k) for b in range(16) for k in range(launches)]
    assert all(slot == body & 3 for body, slot, _, _ in seq)
    dirs = [d for _, _, _, d in seq]
    assert dirs[0] == 0
    assert set(dirs) == {0, 1}
    for i in range(1, len(dirs)):
        assert dirs[i] == 1 - dirs[i - 1], (launches, seq[i - 1], seq[i])


def test_three_launches_keep_the_old_rule(table):
    got = {(slot, k): d for L, _, slot, k, d in table if L == 3}
    for slot in range(4):
        par = slot & 1
        rpar = 1 - par
        assert (got[slot, 0], got[slot, 1], got[slot, 2]) == (par, rpar, par), slot


def test_two_launches_are_forward_then_back_in_every_slot(table):
    for L, _, slot, k, d in table:
        if L == 2:
            assert d == k, (slot, k, d)
