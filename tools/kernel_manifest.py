#!/usr/bin/env python3
"""Prints one line per gfx950 kernel of the engine's kernel objects: a SHA-256 of the kernel's
code bytes, its register and segment figures, and a SHA-256 of its whole metadata entry
(the figures, the kernarg layout and the rest of the code object's note for it).

    python tools/kernel_manifest.py                 # the product objects of bitcoin-miner_amd/build
    python tools/kernel_manifest.py build/tie_*.o   # or the objects named

tests/golden/kernel_manifest.txt is this tool's output for the product objects up to MODE 5, and
tests/test_codegen.py holds the build against it; tests/golden/kernel_manifest_collect_batch.txt is
its output for build/kernels_{plain,ut,misc}_collectbatch.o (MODE 6), held by
tests/test_collect_below_batch_cpu.py; tests/golden/kernel_manifest_packed.txt is its output for
build/pack.o (the packed kernel, which the default glob kernels*.o leaves out), held by
tests/test_packed_cpu.py.  The objects must exist (make builds them).
"""
import glob
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "bitcoin-miner_amd", "build")
LLVM = os.environ.get("LLVMBIN", "/opt/rocm/lib/llvm/bin")
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
          "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size")


def code_object(obj, tmp):
    """The gfx950 code object embedded in a host object, as a path."""
    fat, co = os.path.join(tmp, "fatbin.bin"), os.path.join(tmp, "k.co")
    # an explicit output file: objcopy with only an input rewrites it in place
    subprocess.check_call(["objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(tmp, "copy.o")])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                           f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    return co


def function_bytes(co):
    """{symbol: code bytes} of the FUNC symbols of an ELF64 little-endian code object."""
    d = open(co, "rb").read()
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", d, 0x3A)
    # per section: type, address, file offset, size, link, entry size
    sec = [struct.unpack_from("<4xI8xQQQI12xQ", d, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for typ, _, off, size, link, entsize in sec:
        if typ != 2:  # SHT_SYMTAB
            continue
        stroff = sec[link][2]
        for p in range(off, off + size, entsize):
            name, info, shndx, value, length = struct.unpack_from("<IBxHQQ", d, p)
            if info & 0xF != 2 or not 0 < shndx < shnum:  # STT_FUNC, defined here
                continue
            start = sec[shndx][2] + value - sec[shndx][1]
            out[d[stroff + name:d.index(b"\0", stroff + name)].decode()] = d[start:start + length]
    return out


def kernel_entries(co):
    """{kernel symbol: text of its entry in the code object's metadata note}."""
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    kernels = notes[notes.index("amdhsa.kernels:"):]
    kernels = kernels[:kernels.index("\namdhsa.", 1)]
    out = {}
    for block in re.split(r"^  - ", kernels, flags=re.M)[1:]:
        out[re.search(r"\.name:\s+(\S+)", block).group(1)] = block
    return out


def manifest(objs):
    lines = []
    for obj in objs:
        with tempfile.TemporaryDirectory() as tmp:
            co = code_object(obj, tmp)
            code, entries = function_bytes(co), kernel_entries(co)
        for sym in sorted(entries):
            figures = " ".join(f + "=" + re.search(r"\.%s:\s+(\d+)" % f, entries[sym]).group(1) for f in FIELDS)
            lines.append(f"{os.path.basename(obj)} {sym} code={hashlib.sha256(code[sym]).hexdigest()} "
                         f"bytes={len(code[sym])} {figures} meta={hashlib.sha256(entries[sym].encode()).hexdigest()}")
    return lines


if __name__ == "__main__":
    # the default is kernel_manifest.txt's set: the MODE 6 objects have a fixture of their own
    objs = sys.argv[1:] or sorted(o for o in glob.glob(os.path.join(BUILD, "kernels*.o"))
                                  if not o.endswith((".dev.o", "_collectbatch.o")))
    print("\n".join(manifest(objs)))
