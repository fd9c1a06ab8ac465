"""Diagnostic only: are the gfx950 code objects of two builds of libgymchess.so the same?  (no GPU needed)

    python tools/codeobj_diff.py <a.so> <b.so>

For a change that only moves source text: build both trees with the same flags and the same
-DGC_SRC_HASH="...", then compare.  Three sections, one line each -- `same`, or where the two
first differ -- and a non-zero exit status on any difference:

    disassembly   llvm-objdump -d               (every kernel's and device function's instructions)
    notes         llvm-readelf --notes          (every kernel's VGPR / SGPR / LDS / scratch figures, its arguments)
    data          llvm-objdump -s of .rodata, .data and .bss

Ignored: the line that names the input file, and the digits of hipcc's per-translation-unit
__hip_cuid_<hash> symbol (made from the source's path and content).  The sha256 printed is the
compared text's."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from static_counts import LLVM, code_object  # noqa: E402

SECTIONS = [
    ("disassembly", ["llvm-objdump", "-d"]),
    ("notes", ["llvm-readelf", "--notes"]),
    ("data", ["llvm-objdump", "-s", "-j", ".rodata", "-j", ".data", "-j", ".bss"]),
]


def text(cmd, co):
    out = subprocess.run([os.path.join(LLVM, cmd[0])] + cmd[1:] + [co], check=True, capture_output=True, text=True)
    lines = [ln for ln in out.stdout.splitlines() if co not in ln]
    return [re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", ln) for ln in lines]


def first_difference(a, b):
    """the first line that differs, and the symbol (`<name>:` of a disassembly) it lies in"""
    sym = None
    for k in range(max(len(a), len(b))):
        la, lb = (a[k] if k < len(a) else "<end>"), (b[k] if k < len(b) else "<end>")
        if la != lb:
            where = f"in {sym}, " if sym else ""
            return f"{where}line {k + 1}: {la.strip()!r} != {lb.strip()!r}"
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", la)
        if m:
            sym = m.group(1)
    return None


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    differ = False
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        ca, cb = code_object(sys.argv[1], ta), code_object(sys.argv[2], tb)
        for name, cmd in SECTIONS:
            a, b = text(cmd, ca), text(cmd, cb)
            sha = [hashlib.sha256("\n".join(t).encode()).hexdigest() for t in (a, b)]
            d = first_difference(a, b)
            differ = differ or d is not None
            if d is None:
                syms = sum(bool(re.match(r"^[0-9a-f]+ <[^>]+>:", ln)) for ln in a)
                what = f", {syms} symbols" if name == "disassembly" else ""
                print(f"{name}: same ({len(a)} lines{what}, sha256 {sha[0]})")
            else:
                print(f"{name}: DIFFERENT, {d} (sha256 {sha[0]} != {sha[1]})")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
