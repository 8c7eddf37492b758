"""csrc/secret.h holds everything that touches a secret scalar on the host: wipe, the "below r" test, the operating
system's generator, the pooled rejection sampler of Fr (FrPool::draw_fr) and draw_rho.  It is plain C++ over field.h,
so it is compiled here with the stand-alone tests/host/secret_main.cpp by g++ -fsanitize=address,undefined and run as
a program of its own, with a scripted source of bytes in place of the operating system's: the edges of the range, the
masked top bits, failing sources, and that consumed slots and a pool that has gone read as zero.  No GPU code runs and
nothing is loaded into Python.  Where the sanitizers' runtime is not installed the same program is built without them
and every check still runs."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "secret_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_secret_helpers_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the library anyway"
    exe = str(tmp_path / "secret_host")
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", SOURCE, "-o", exe]
    r = subprocess.run(base + SANITIZE, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)\b", r.stderr):   # the linker's wording only
        print("the sanitizer runtime is not installed; building without it:", r.stderr.strip().splitlines()[-1])
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"(\d+) checks, (\d+) failures", r.stdout)
    assert m, r.stdout[-1000:]
    assert int(m.group(2)) == 0, r.stderr[-4000:]
    assert int(m.group(1)) >= 40, r.stdout[-1000:]
