"""CPU: the ride stage's host arithmetic (fish-tts_amd/csrc/fx_chain.h: rd_plan, RdStage, its place in StageChain and
FxDesc) driven by the stand-alone program tools/ride_plan_check.cpp, built with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a process of its own - no GPU, nothing loaded into Python.  It walks RdStage over
random chunkings: emitted totals equal n, held-back below (A + 1) H, the plan independent of the chunking and equal to the
emission rule that ft_ride_plan reports.  ft_ride_plan itself (host only) is compared with the same rule here."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from tests import ride_ref as RR
from tests.level_ref import RATES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ride_plan_under_sanitizers(tmp_path):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx is not None, "no host C++ compiler (the project itself cannot be built without one)"
    exe = str(tmp_path / "ride_plan_check")
    # the sanitizer runtimes linked statically: the program needs nothing from its environment
    static = ["-static-libsan"] if "clang" in os.path.basename(os.path.realpath(cxx)) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", *static, os.path.join(ROOT, "tools", "ride_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ride_plan_check: ok" in run.stdout, run.stdout + run.stderr


def test_ft_ride_plan_is_the_emission_rule():
    from fish_tts_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(18)
    for rate in RATES + (22050, 24000):
        H = RR.hop(rate)
        ns = [0, 1, H - 1, H, 4 * H, RR.A * H - 1, RR.A * H, (RR.A + 1) * H - 1, (RR.A + 1) * H, (RR.A + 1) * H + 1] + \
             [int(v) for v in rng.integers(0, 200 * H, 20)]
        for n in ns:
            for final in (False, True):
                k, out = C.c_int64(-1), C.c_int64(-1)
                assert lib.ft_ride_plan(rate, n, int(final), C.byref(k), C.byref(out)) == L.FT_OK
                assert (k.value, out.value) == RR.plan(n, H, final), (rate, n, final)
                assert n - out.value < (RR.A + 1) * H
    k = C.c_int64(-1)
    assert lib.ft_ride_plan(16000, 5, 0, None, None) == L.FT_OK
    for rate, n in ((7999, 5), (44101, 5), (16000, -1)):
        assert lib.ft_ride_plan(rate, n, 0, C.byref(k), None) == L.FT_ERR_ARG and k.value == -1
