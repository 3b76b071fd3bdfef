"""CPU: the live room stage's host arithmetic (fish-tts_amd/csrc/fx_chain.h, the rl_* block: the values of `begin`, a stream's
counters over random cuttings, the bound of its carry, the per-push checks in their stated order, the buffer sizes, the
staging's pick of a sent sample and the roll of the carry) driven by the stand-alone program tools/room_live_check.cpp, built
with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own - no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_room_live_plan_under_sanitizers(tmp_path):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx is not None, "no host C++ compiler (the project itself cannot be built without one)"
    exe = str(tmp_path / "room_live_check")
    # the sanitizer runtimes linked statically: the program needs nothing from its environment
    static = ["-static-libsan"] if "clang" in os.path.basename(os.path.realpath(cxx)) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", *static, os.path.join(ROOT, "tools", "room_live_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "room_live_check: ok" in run.stdout, run.stdout + run.stderr
