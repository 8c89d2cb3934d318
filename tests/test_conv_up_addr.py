"""Source addresses and padding of the ping-pong conv3x3 tiles with a nearest-2x upsampled input, on the host: the arithmetic
lives in seed-story_amd/csrc/ss_conv_up.h as plain functions which the kernel calls; tests/conv_up_addr_check.cpp composes them
the way the kernel does and compares every (tile, wave, piece, tap, lane) of the GPU test's cases with the definition
((oy + dy) >> 1, (ox + dx) >> 1) and with the bounds of the source tensor.  The program is built with the address and
undefined-behaviour sanitizers and run as a process of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "conv_up_addr_check.cpp")
INC = os.path.join(ROOT, "seed-story_amd", "csrc")

# (B, Ci, H_in, W_in) of tests/test_conv_pp_upsample_gpu.py CASES (Co plays no part in the A operand)
CASES = [(8, 64, 2, 4), (2, 64, 8, 4), (1, 128, 8, 8), (1, 1280, 4, 16), (4, 192, 4, 4), (1, 64, 16, 16)]


def _compiler():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if os.path.exists(hipcc):
        return [hipcc, "-x", "c++", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler found")
    return [cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_up") / "conv_up_addr_check")
    subprocess.run(_compiler() + ["-O1", "-g", "-std=c++17", "-I", INC, SRC, "-o", exe], check=True)
    return exe


def test_conv_up_addresses(program):
    r = subprocess.run([program] + ["%d,%d,%d,%d" % c for c in CASES], capture_output=True, text=True)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.endswith(" wrong")]
    assert len(lines) == len(CASES)
    for (B, Ci, H, W), ln in zip(CASES, lines):
        # tiles x waves x pieces x taps x K tiles per tap x lanes
        n = (B * 4 * H * W // 256) * 8 * 4 * 9 * (Ci // 64) * 64
        assert ln == "B=%d Ci=%d H=%d W=%d: %d addresses, 0 wrong" % (B, Ci, H, W, n)


def test_conv_up_check_refuses_ineligible_shape(program):
    """a shape outside pp_launch's rule (output H = 6) is refused with exit status 2, not walked and passed"""
    r = subprocess.run([program, "1,64,3,4"], capture_output=True, text=True)
    assert r.returncode == 2
