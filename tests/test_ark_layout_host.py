"""The layout walk of the arkworks containers (g16_ark_pk_layout / g16_ark_vk_layout in csrc/loaders.cpp) is pure
host code over untrusted bytes: it is compiled here, together with the stand-alone tests/arkser/layout_main.cpp, by
g++ with -fsanitize=address,undefined, and walks a valid blob and a few hundred truncations and mutations of it, each
in a heap block of exactly its length.  No GPU code runs and nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_walk_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the library anyway"
    exe = str(tmp_path / "layout_main")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "circom_compat_amd", "csrc", "loaders.cpp"),
           os.path.join(ROOT, "tests", "arkser", "layout_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)\b", r.stderr):   # the linker's wording only
        pytest.skip("the sanitizer runtime is not installed: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"(\d+) cases, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 200, r.stdout
