#!/usr/bin/env python3
"""Compare the gfx950 device code of two versions of csrc/ (CPU only: nothing is run).

    python tools/device_code_diff.py OLD_CSRC NEW_CSRC [file.hip ...] [--ignore-names]

Each file is cross-compiled device-only on both sides with mobi_amd/build.py's flags (and its per-file EXTRA), the gfx950
code object is disassembled, and one line per file reports the kernel count and a sha256 of the disassembly of either side.
--ignore-names replaces every function's mangled symbol by its ordinal first and drops the addresses, keeping the encodings
(for a change of template parameters that must leave the instructions alone: shorter names move the text section).
Object files are not compared: their __hip_cuid_* symbol hashes the translation unit.  Both directories must sit in a tree where "../../include/mobi_engine.h" resolves.  A file that only NEW_CSRC has is reported as new (its kernel count and sha256) and is no
difference.  Exit status 1 if any file that both sides have differs."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobi_amd import build as B  # noqa: E402

LLVM = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(B.hipcc()))), "llvm", "bin")
LABEL = re.compile(r"^<([^>+]+)>:$", re.M)


def disassemble(csrc, name, tmp, ignore_names):
    obj = os.path.join(tmp, "dev.o")
    cmd = [B.hipcc(), f"--offload-arch={B.ARCH}", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-result", "--offload-device-only"]
    cmd += os.environ.get("MOBI_HIPCC_FLAGS", "").split() + B.EXTRA.get(name, [])
    subprocess.run(cmd + ["-c", os.path.join(csrc, name), "-o", obj], check=True)
    with open(obj, "rb") as f:
        bundled = f.read(24) == b"__CLANG_OFFLOAD_BUNDLE__"
    if bundled:
        elf = os.path.join(tmp, "dev.elf")
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={obj}",
                        f"--targets=hip-amdgcn-amd-amdhsa--{B.ARCH}", f"--output={elf}"], check=True)
        obj = elf
    syms = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-t", obj], check=True, capture_output=True, text=True).stdout
    kernels = sum(1 for ln in syms.splitlines() if ln.endswith(".kd"))
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", obj], check=True, capture_output=True, text=True).stdout
    text = text[text.find("Disassembly of section"):] if kernels else ""       # (the lines before it name the object file)
    if ignore_names:
        text = re.sub(r"(?m)^[0-9a-f]{16} <", "<", re.sub(r"// [0-9A-F]{12}: ", "// ", text))
        for i, sym in enumerate(dict.fromkeys(LABEL.findall(text))):
            text = text.replace(f"<{sym}>", f"<#{i}>").replace(f"<{sym}+", f"<#{i}+")
    return kernels, text


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old_csrc")
    ap.add_argument("new_csrc")
    ap.add_argument("files", nargs="*", help="default: every .hip of NEW_CSRC")
    ap.add_argument("--ignore-names", action="store_true")
    a = ap.parse_args()
    files = a.files or sorted(f for f in os.listdir(a.new_csrc) if f.endswith(".hip"))
    differ = 0
    for name in files:
        if not os.path.exists(os.path.join(a.old_csrc, name)):
            with tempfile.TemporaryDirectory() as tmp:
                kn, new = disassemble(a.new_csrc, name, tmp, a.ignore_names)
            print(f"{name:20s} kernels   - | {kn:3d}   disassembly lines       - | {new.count(chr(10)):7d}   "
                  f"sha256 {'-':16s} | {hashlib.sha256(new.encode()).hexdigest()[:16]}   new file")
            continue
        with tempfile.TemporaryDirectory() as tmp:
            (ko, old), (kn, new) = (disassemble(d, name, tmp, a.ignore_names) for d in (a.old_csrc, a.new_csrc))
        same = old == new and ko == kn
        differ += not same
        sha = [hashlib.sha256(t.encode()).hexdigest()[:16] for t in (old, new)]
        print(f"{name:20s} kernels {ko:3d} | {kn:3d}   disassembly lines {old.count(chr(10)):7d} | {new.count(chr(10)):7d}   "
              f"sha256 {sha[0]} | {sha[1]}   {'identical' if same else 'DIFFERENT'}{' (names ignored)' if a.ignore_names else ''}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
