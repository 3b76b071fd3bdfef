#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds, kernel by kernel:  python tools/codeobj_diff.py OLD NEW [-v]

OLD and NEW are host objects of hipcc (engine.o, codec.o), offload bundles (--cuda-device-only output) or bare code objects.
The gfx950 part is taken out with clang-offload-bundler, the .text function symbols are read with llvm-objdump -t, and every
kernel's machine code and descriptor (NAME.kd: registers, LDS, scratch; its offset to the code left out) are compared byte for
byte.  Per kernel (-v: all of them, else those that differ): identical, moved by N, differs (old size, new size), only in
one; then the totals.  Exit status 1 if a kernel differs or is only in one."""
import collections
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
SECTIONS = (".text", ".rodata")


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def code_object(path, tmp):
    """The path of the bare gfx950 ELF inside `path`."""
    head = open(path, "rb").read(64)
    if head[:4] == b"\x7fELF" and head[18:20] == b"\xe0\x00":                         # e_machine 224: EM_AMDGPU
        return path
    if not head.startswith(b"__CLANG_OFFLOAD_BUNDLE__"):                                # a host object: its fat binary
        run("llvm-objcopy", "--dump-section", f".hip_fatbin={tmp}/fb", path, f"{tmp}/host")
        path = f"{tmp}/fb"
    target = [t for t in run("clang-offload-bundler", "--list", "--type=o", "--input=" + path).split() if "gfx950" in t]
    if len(target) != 1:
        raise SystemExit(f"{path}: {len(target)} gfx950 entries in the bundle")
    run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + target[0], "--input=" + path, f"--output={tmp}/co")
    return f"{tmp}/co"


def kernels(path):
    """{name: (address, code bytes, descriptor bytes)} of the .text functions, and the code object's size."""
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(path, tmp)
        size, data, base, syms = os.path.getsize(co), {}, {}, {}
        for sec in SECTIONS:
            run("llvm-objcopy", "--dump-section", f"{sec}={tmp}/sec", co, f"{tmp}/rest")
            data[sec] = open(f"{tmp}/sec", "rb").read()
        for f in map(str.split, run("llvm-objdump", "-h", co).splitlines()):
            if len(f) >= 4 and f[1] in SECTIONS:
                base[f[1]] = int(f[3], 16)
        for f in map(str.split, run("llvm-objdump", "-t", co).splitlines()):     # ADDR FLAGS.. SECTION SIZE [.protected] NAME
            s = next((k for k, v in enumerate(f) if v in SECTIONS), 0)
            if s and ("F" in f[1:s] or f[-1].endswith(".kd")):
                addr, n = int(f[0], 16), int(f[s + 1], 16)
                syms[f[-1]] = (addr, data[f[s]][addr - base[f[s]]:addr - base[f[s]] + n])
    kd = {k: v[1][:16] + v[1][24:] for k, v in syms.items() if k.endswith(".kd")}       # bytes 16..23: the entry's offset
    return {k: (*v, kd.get(k + ".kd", b"")) for k, v in syms.items() if not k.endswith(".kd")}, size


def main():
    paths = [a for a in sys.argv[1:] if a != "-v"]
    if len(paths) != 2:
        raise SystemExit(__doc__)
    (old, so), (new, sn) = kernels(paths[0]), kernels(paths[1])
    count, moves = collections.Counter(), collections.Counter()
    for name in sorted(set(old) | set(new), key=lambda k: (old.get(k) or new[k])[0]):
        o, n = old.get(name), new.get(name)
        if o is None or n is None:
            key = "only in " + ("new" if o is None else "old")
            what = f"{key} ({len((o or n)[1])} bytes)"
        elif o[1:] != n[1:]:
            key = "differs"
            what = f"differs ({len(o[1])}, {len(n[1])} bytes)" + ("" if o[2] == n[2] else ", descriptor too")
        else:
            key = "moved" if n[0] != o[0] else "identical"
            what = f"moved by {n[0] - o[0]:+#x}" if n[0] != o[0] else key
            moves[n[0] - o[0]] += 1
        count[key] += 1
        if "-v" in sys.argv or key not in ("identical", "moved"):
            print(f"{what:32s} {name}")
    print(f"{len(old)} kernels in {so} bytes -> {len(new)} in {sn}: " + ", ".join(f"{n} {k}" for k, n in sorted(count.items())))
    for d, n in sorted(moves.items()):
        print(f"  {n} at {d:+#x}")
    return 1 if set(count) - {"identical", "moved"} else 0


if __name__ == "__main__":
    sys.exit(main())
