#!/usr/bin/env python3
"""device_code_diff.py OLD.so NEW.so - do two builds of the library hold the same gfx950 device code?

For refactors whose acceptance is "no device instruction changed". Every gfx950 code object of both libraries is taken out of
.hip_fatbin, its symbol table is listed and its text disassembled (llvm-objdump -d --no-show-raw-insn); addresses and the
trailing address comments are dropped, and the two libraries are compared code object by code object: the set of symbols, and
the instruction text of every symbol. Not compared: __hip_cuid_* (the name is a hash of the source) and objdump's "..." line
for the zero padding behind the LAST function of a code object (it moves with the order in which instances are emitted,
profiles/launch_refactor.txt B). Prints the counts; exit status 0 only if nothing differs. No GPU needed.
"""
import hashlib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
HEADER = re.compile(r"^[0-9a-f]+ <(.+)>:$")


def code_objects(lib, td):
    """paths of the gfx950 code objects of `lib`, in the order of the bundles in .hip_fatbin"""
    fat = Path(td) / "fat.bin"
    subprocess.check_call([str(LLVM / "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", str(lib), str(fat)])
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)] + [len(blob)]
    if len(starts) == 1:
        sys.exit(f"{lib}: no offload bundle in .hip_fatbin")
    out = []
    for i in range(len(starts) - 1):
        piece, co = Path(td) / f"bundle{i}.bin", Path(td) / f"dev{i}.co"
        piece.write_bytes(blob[starts[i] : starts[i + 1]])
        subprocess.check_call([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                               f"--input={piece}", f"--output={co}"], stderr=subprocess.DEVNULL)
        out.append(co)
    return out


def symbols(co):
    """the functions and objects of the code object's symbol table (not the assembler's *ABS* register-count records) but __hip_cuid_*"""
    table = subprocess.run([str(LLVM / "llvm-objdump"), "-t", str(co)], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in table.splitlines() if re.match(r"^[0-9a-f]{8,} ", line) and "*ABS*" not in line}
    return {n for n in names if not n.startswith("__hip_cuid_")}


def instructions(co):
    """symbol -> (instruction lines, digest of their text)"""
    proc = subprocess.Popen([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", str(co)], stdout=subprocess.PIPE, text=True)
    out, name, count, digest = {}, None, 0, None
    for line in proc.stdout:
        line = line.rstrip()
        head = HEADER.match(line)
        if head:
            if name is not None:
                out[name] = (count, digest.hexdigest())
            name, count, digest = head.group(1), 0, hashlib.sha256()
            continue
        text = line.split("//")[0].strip()
        if name is None or not text or text == "...":
            continue
        count += 1
        digest.update(text.encode() + b"\n")
    if name is not None:
        out[name] = (count, digest.hexdigest())
    if proc.wait() != 0:
        sys.exit(f"llvm-objdump failed on {co}")
    return out


def read_library(lib):
    with tempfile.TemporaryDirectory() as td:
        return [(symbols(co), instructions(co)) for co in code_objects(lib, td)]


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = read_library(sys.argv[1]), read_library(sys.argv[2])
    print(f"code objects: {len(old)} / {len(new)}")
    bad = len(old) != len(new)
    n_syms = [0, 0]
    n_lines = [0, 0]
    differing = 0
    for i, ((syms_o, ins_o), (syms_n, ins_n)) in enumerate(zip(old, new)):
        n_syms[0] += len(syms_o)
        n_syms[1] += len(syms_n)
        n_lines[0] += sum(c for c, _ in ins_o.values())
        n_lines[1] += sum(c for c, _ in ins_n.values())
        for n in sorted(syms_o - syms_n):
            print(f"code object {i}: symbol only in OLD: {n}")
        for n in sorted(syms_n - syms_o):
            print(f"code object {i}: symbol only in NEW: {n}")
        bad |= syms_o != syms_n or ins_o.keys() != ins_n.keys()
        for n in sorted(ins_o.keys() & ins_n.keys()):
            if ins_o[n] != ins_n[n]:
                differing += 1
                print(f"code object {i}: instructions differ ({ins_o[n][0]} / {ins_n[n][0]} lines): {n}")
    print(f"symbols: {n_syms[0]} / {n_syms[1]}, symbol sets {'differ' if bad else 'identical'}")
    print(f"instruction lines: {n_lines[0]} / {n_lines[1]}")
    print(f"symbols with a differing instruction: {differing}")
    sys.exit(1 if bad or differing else 0)


if __name__ == "__main__":
    main()
