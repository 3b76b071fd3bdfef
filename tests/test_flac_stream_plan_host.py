"""CPU: the live FLAC stage's host arithmetic (fish-tts_amd/csrc/flac_plan.h: the emission rule over some thousand cuttings
against the whole's frame count and last frame, the carry below the blocksize, the byte bound, the per-push refusals in their
stated order, the 2^36 - 1 limit, the head bytes before and after the final push) driven by the stand-alone program
tools/flac_stream_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own - no
GPU, nothing loaded into Python.  ft_flac_stream_plan is then asked of the library itself."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flac_stream_plan_under_sanitizers(tmp_path):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx is not None, "no host C++ compiler (the project itself cannot be built without one)"
    exe = str(tmp_path / "flac_stream_check")
    # the sanitizer runtimes linked statically: the program needs nothing from its environment
    static = ["-static-libsan"] if "clang" in os.path.basename(os.path.realpath(cxx)) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", *static, os.path.join(ROOT, "tools", "flac_stream_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "flac_stream_check: ok" in run.stdout, run.stdout + run.stderr


def test_stream_plan_without_a_gpu():
    """ft_flac_stream_plan is host arithmetic: the library answers it without a device, as the header states it."""
    from fish_tts_amd import _lib
    lib = _lib.load()

    def plan(B, ch, before, n, final):
        frames, nbytes = C.c_int64(-1), C.c_int64(-1)
        st = lib.ft_flac_stream_plan(B, ch, before, n, 1 if final else 0, C.byref(frames), C.byref(nbytes))
        return st, frames.value, nbytes.value

    assert plan(256, 1, 0, 255, False) == (0, 0, 0)
    assert plan(256, 1, 255, 1, False) == (0, 1, 18 + 2 * 256)
    assert plan(256, 2, 255, 258, False) == (0, 2, 2 * 19 + 4 * 512)
    assert plan(256, 2, 255, 258, True) == (0, 3, 3 * 19 + 4 * 513)
    assert plan(4096, 1, 10 * 4096 + 7, 0, True) == (0, 1, 18 + 2 * 7)
    assert plan(4096, 1, 10 * 4096, 0, True) == (0, 0, 0)
    # a whole piece in one final push: ft_flac_bound without the 42
    for n, ch, B in ((1, 1, 256), (257, 2, 256), (100000, 2, 4096), (1 << 28, 1, 1024)):
        assert plan(B, ch, 0, n, True) == (0, -(-n // B), lib.ft_flac_bound(n, ch, B) - 42)
    assert lib.ft_flac_stream_plan(256, 1, 0, 300, 0, None, None) == 0            # either pointer may be NULL
    arg, too_long = 1, 6
    for bad in ((300, 1, 0, 1), (256, 3, 0, 1), (256, 0, 0, 1), (256, 1, -1, 1), (256, 1, 0, -1)):
        assert plan(*bad, False)[0] == arg, bad
    assert plan(256, 1, 0, (1 << 28) + 1, False)[0] == too_long
    assert plan(256, 1, (1 << 36) - 11, 10, True)[0] == 0
    assert plan(256, 1, (1 << 36) - 11, 11, True)[0] == too_long
