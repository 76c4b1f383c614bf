"""The wide signed DIT butterflies of babybear.h (the LDE's forward passes), host side: tests/cpp/wide_quad_test.cpp compiled with g++ against the header
alone.  It checks the radix-4 quad against bb::mul / add / sub on every combination of the edge words {0, +-1, +-(p-1), +-(2^31-1), INT32_MIN+1} and edge
twiddles {0, +-1, +-(p-1)/2}, on 10^6 seeded random quads, and through 64 chained rounds fed with their own outputs (|x| < p from the second round on),
with every 64-bit sum compared with the exact integer and held against the reduction's input bound."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_quad_host(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "wide_quad_test.cpp")
    exe = str(tmp_path / "wide_quad_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("OK "), p.stdout
    n = int(p.stdout.split()[1])
    assert n >= 8 ** 4 * 5 ** 3 + 1000000 + 3 * 64 * 256
