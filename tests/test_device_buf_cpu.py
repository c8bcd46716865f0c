"""csrc/device_buf.h (the owning device buffer of the handles) on the host: tests/device_buf_check.cpp supplies malloc / free /
memcpy in place of the HIP runtime, counts live allocations and drives the type through every state.  Compiled here with the host
compiler under AddressSanitizer and UBSan and run as a program of its own; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if name and shutil.which(name):
            return name
    return None


def test_device_buf_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "device_buf_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", os.path.join(HERE, "device_buf_check.cpp"), "-o", exe]
    # the runtimes linked into the program where the compiler can (g++): it then starts under any preloaded library
    r = subprocess.run(base + SANITIZE + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base + SANITIZE, capture_output=True, text=True)
    sanitized = r.returncode == 0
    if not sanitized:
        # the sanitizer runtimes are a package of their own: without them the checks of the program itself still run
        assert "sanitizer" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr, r.stderr[-3000:]
        print("sanitizer runtime missing, building without:", r.stderr[-300:])
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(run.stdout[-2000:], run.stderr[-4000:])
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "device_buf_check ok" in run.stdout
    print("sanitized build" if sanitized else "plain build")
