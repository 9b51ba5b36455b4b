#!/usr/bin/env python3
"""sha256 and size of the gfx950 code object inside every shipped object file: `unit sha256 size` per line.

A change that must not alter a shipped instruction is checked by building two trees with the same compiler and comparing the two
listings (HISTORY.md, "Rejected forms retired").  The units are the Makefile's SRCS; of each unit.o the .hip_fatbin section is dumped
with llvm-objcopy and the device entry is unbundled with clang-offload-bundler.  Nothing is disassembled or searched: bytes are hashed.
CPU only, no GPU, no torch.

    python tools/code_object_hashes.py [CSRC_DIR] [--arch gfx950]
"""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "gps_optimize_slam_amd", "csrc")


def llvm_tool(name):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/lib/llvm/bin", os.environ.get("ROCM_PATH", "/opt/rocm") + "/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    p = shutil.which(name)
    if not p:
        sys.exit(f"{name} not found (looked under ROCM_PATH and on PATH)")
    return p


def units(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    m = re.search(r"^SRCS\s*:?=\s*(.*)$", text, re.M)
    if not m:
        sys.exit("no SRCS line in the Makefile")
    return [s[:-len(".hip")] for s in m.group(1).split()]


def code_object(obj, arch, tmp, objcopy, bundler):
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    r = subprocess.run([objcopy, "--dump-section", f".hip_fatbin={fat}", obj], capture_output=True, text=True)
    if r.returncode != 0:
        if "section '.hip_fatbin' not found" in r.stderr:                # a host-only unit (gsf_capi): no kernels, nothing to hash
            return None
        sys.exit(r.stderr)
    ids = subprocess.run([bundler, "--list", "--type=o", f"--input={fat}"], check=True, capture_output=True, text=True).stdout.split()
    want = [i for i in ids if i.startswith("hip") and i.endswith("-" + arch)]
    if len(want) != 1:
        sys.exit(f"{obj}: expected one {arch} entry, the bundle lists {ids}")
    subprocess.run([bundler, "--unbundle", "--type=o", f"--input={fat}", f"--targets={want[0]}", f"--output={co}"], check=True)
    with open(co, "rb") as f:
        return f.read()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("csrc", nargs="?", default=CSRC, help="directory with the Makefile and the built objects")
    ap.add_argument("--arch", default="gfx950")
    a = ap.parse_args()
    objcopy, bundler = llvm_tool("llvm-objcopy"), llvm_tool("clang-offload-bundler")
    with tempfile.TemporaryDirectory() as tmp:
        for u in units(a.csrc):
            obj = os.path.join(a.csrc, u + ".o")
            if not os.path.exists(obj):
                sys.exit(f"{obj} is missing: build the library first")
            b = code_object(obj, a.arch, tmp, objcopy, bundler)
            print(u, "no-device-code 0" if b is None else f"{hashlib.sha256(b).hexdigest()} {len(b)}")


if __name__ == "__main__":
    main()
