"""csrc/f64_key.h: the order-preserving uint64 keys of a float64 shared by every kernel that sorts or selects on float64 values."""
import os
import shutil
import subprocess

import pytest


def test_f64_keys_under_sanitizers(tmp_path):
    """+-inf, +-DBL_MAX, +-1, the smallest normal and denormal of both signs, +-0 and a few hundred random doubles: both encoders
    strictly monotone, -0 and +0 one key, a NaN below everything in one encoder and above everything in the other, the decoder
    gives the input's bits back (+0 for -0), the complement reverses the order.  tests/f64_key_check.cpp, compiled with the host
    compiler under AddressSanitizer and UBSan and run as a program of its own; nothing is loaded into Python."""
    here = os.path.dirname(os.path.abspath(__file__))
    cxx = next((shutil.which(c) for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "f64_key_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", os.path.join(here, "f64_key_check.cpp"), "-o", exe]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    r = subprocess.run(base + sanitize + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base + sanitize, capture_output=True, text=True)
    if r.returncode != 0:                          # the sanitizer runtimes are a package of their own: the program's checks still run
        assert "sanitizer" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr, r.stderr[-3000:]
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout[-2000:], run.stderr[-4000:])
    assert run.returncode == 0 and "f64_key_check ok" in run.stdout
