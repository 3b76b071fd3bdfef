"""CPU: the stereo mix stage's host arithmetic (fish-tts_amd/csrc/fx_chain.h, the ms_* block: the region checks in their
stated order and their place among the mix stage's, the region lookup, the pan table, the side selection) driven by the
stand-alone program tools/stereo_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process
of its own - no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stereo_plan_under_sanitizers(tmp_path):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx is not None, "no host C++ compiler (the project itself cannot be built without one)"
    exe = str(tmp_path / "stereo_check")
    # the sanitizer runtimes linked statically: the program needs nothing from its environment
    static = ["-static-libsan"] if "clang" in os.path.basename(os.path.realpath(cxx)) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", *static, os.path.join(ROOT, "tools", "stereo_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "stereo_check: ok" in run.stdout, run.stdout + run.stderr
