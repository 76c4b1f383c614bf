"""The multiply-first natural -> bit-reversed quad of babybear.h (the LDE's inverse rounds) and the signed coset-scale product, host side:
tests/cpp/ct_quad_test.cpp compiled with g++ against the header alone.  It checks the quad's wiring against bb::mul / add / sub on every combination of the
edge words {0, +-1, +-(p-1), +-(2^31-1), INT32_MIN+1} and edge twiddles {0, +-1, +-(p-1)/2}, on 10^6 seeded random quads, and through 64 chained rounds fed
with their own outputs (|x| < p from the second round on; from the first when the words start canonical), with every 64-bit sum compared with the exact
integer and held against the reduction's input bound; the scale product x g / R the same way, on words of (-p, p) and canonical factors."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ct_quad_host(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "ct_quad_test.cpp")
    exe = str(tmp_path / "ct_quad_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("OK "), p.stdout
    words = p.stdout.split()
    assert int(words[1]) >= 8 ** 4 * 5 ** 3 + 1000000 + 4 * 64 * 256
    assert int(words[3]) >= 7 * 7 + 1000000
