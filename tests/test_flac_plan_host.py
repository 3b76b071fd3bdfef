"""CPU: the FLAC stage's host arithmetic (fish-tts_amd/csrc/flac_plan.h: the argument checks in their stated order, the frame
count and the last frame's size, the frame header and STREAMINFO bytes, the number coding at its seams, the CRC tables and the
rule that joins the CRC-16 of byte runs, ft_flac_bound) driven by the stand-alone program tools/flac_check.cpp, built with
AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own - no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flac_plan_under_sanitizers(tmp_path):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx is not None, "no host C++ compiler (the project itself cannot be built without one)"
    exe = str(tmp_path / "flac_check")
    # the sanitizer runtimes linked statically: the program needs nothing from its environment
    static = ["-static-libsan"] if "clang" in os.path.basename(os.path.realpath(cxx)) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", *static, os.path.join(ROOT, "tools", "flac_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "flac_check: ok" in run.stdout, run.stdout + run.stderr


def test_bound_and_symbols_without_a_gpu():
    """ft_flac_bound is host arithmetic: the library answers it without a device, as the header states it."""
    from fish_tts_amd import _lib
    lib = _lib.load()
    assert lib.ft_flac_bound(1, 1, 256) == 42 + 18 + 2
    assert lib.ft_flac_bound(257, 2, 256) == 42 + 2 * 19 + 4 * 257
    assert lib.ft_flac_bound(1 << 28, 2, 4096) == 42 + (1 << 16) * 19 + 4 * (1 << 28)
    for bad in ((0, 1, 256), ((1 << 28) + 1, 1, 256), (10, 3, 256), (10, 0, 256), (10, 1, 300), (-1, 2, 4096)):
        assert lib.ft_flac_bound(*bad) == -1, bad
