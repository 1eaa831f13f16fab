"""The device std::mt19937_64 (gcsa2_amd/csrc/mt64.hpp) built for the host and checked against the standard library:
outputs, the 10000th output of the default seed, and the wave-parallel three-phase twist emulated lane by lane.
Needs a host C++ compiler, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mt64_driver.cpp")
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("mt64") / "mt64_driver")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-o", exe, SRC])
    return exe


def outputs(driver, seed, count):
    out = subprocess.run([driver, "outputs", str(seed), str(count)], check=True, capture_output=True, text=True).stdout.split()
    vals = [int(v) for v in out]
    assert len(vals) == 2 * count
    return vals[:count], vals[count:]


@pytest.mark.parametrize("seed", [0, 1, 5489, U64, 0x8000000000000000, 17 ^ 311, 1000 ^ 1623, 123456789 ^ 987654321,
                                  0xDEADBEEFCAFEF00D])
def test_outputs_match_std(driver, seed):
    mine, theirs = outputs(driver, seed, 2000)
    assert mine == theirs


def test_ten_thousandth_output_of_default_seed(driver):
    # [rand.predef]: the 10000th consecutive invocation of a default-constructed mt19937_64 produces 9981545732273789042
    mine, theirs = outputs(driver, 5489, 10000)
    assert mine[-1] == 9981545732273789042
    assert theirs[-1] == 9981545732273789042


@pytest.mark.parametrize("lanes", [64, 32, 7, 1])
@pytest.mark.parametrize("seed", [0, U64, 42 ^ 4242])
def test_three_phase_twist_matches_serial(driver, seed, lanes):
    res = subprocess.run([driver, "twist", str(seed), str(lanes), "3"], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
