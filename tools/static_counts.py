"""Diagnostic only: static instruction counts of the fused rollout's kernels per loop and per
barrier-to-barrier segment, from a build's gfx950 code object (no GPU needed).

    python tools/static_counts.py <libgymchess.so> [kernel-name-substring]   (default k_env_rollout4)

A role's plies are one loop of four barriers (k_env_rollout4 switches on the role, so each role's
loop stands alone in the listing); a loop is a backward branch and its target, and its segments
are cut at s_barrier: seg0 runs from the loop's top to the first barrier (the end of phase 0),
seg1-3 are phases 1-3, the last one runs on into the loop's tail.  Classes: valu (v_*), salu
(s_*, waits and nops among them), ds, glob (global_ / buffer_), xbr (s_cbranch_execz / execnz:
the skips of per-lane regions), mul (v_mad_u64_u32, v_mul_*: the slow multiplies among the valu),
and all of them."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def code_object(lib, tmp):
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    co = os.path.join(tmp, "gfx950.co")
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    return co


def kernels(co):
    """name -> the kernel's instructions (mnemonic, branch target or None, label or None)"""
    txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                         capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if cur is None or not m:
            continue
        op, args, addr = m.group(1), m.group(2), int(m.group(3), 16)
        tgt = None
        if op.startswith("s_cbranch") or op == "s_branch":
            t = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", line)
            tgt = int(t.group(1), 16) if t else None
        cur.append((op, tgt, addr))
    return out


def klass(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "glob"
    return "salu" if op.startswith("s_") else "other"


def report(name, ins):
    base = ins[0][2]
    index = {a: i for i, (_, _, a) in enumerate(ins)}
    print(f"== {name} instructions {len(ins)} s_barrier total {sum(op == 's_barrier' for op, _, _ in ins)}")
    loops = set()
    for i, (op, tgt, addr) in enumerate(ins):
        if tgt is not None and base + tgt in index and index[base + tgt] <= i:
            loops.add((index[base + tgt], i))
    for lo, hi in sorted(loops):
        body = ins[lo:hi + 1]
        nb = sum(op == "s_barrier" for op, _, _ in body)
        if nb == 0:
            continue
        print(f"  loop {lo}-{hi}: barriers {nb}")
        seg, counts = 0, {}
        for op, _, _ in body:
            if op == "s_barrier":
                seg += 1
                continue
            c = counts.setdefault(seg, dict(valu=0, salu=0, ds=0, glob=0, xbr=0, mul=0, all=0))
            k = klass(op)
            if k in c:
                c[k] += 1
            c["xbr"] += op.startswith("s_cbranch_exec")
            c["mul"] += op.startswith(("v_mad_u64_u32", "v_mad_i64_i32", "v_mul_"))
            c["all"] += 1
        for s in sorted(counts):
            c = counts[s]
            print(f"     seg{s}: valu {c['valu']:4d} salu {c['salu']:4d} ds {c['ds']:3d} glob {c['glob']:3d} xbr {c['xbr']:2d} mul {c['mul']:2d} all {c['all']}")


def main():
    lib = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "k_env_rollout4"
    with tempfile.TemporaryDirectory() as tmp:
        ks = kernels(code_object(lib, tmp))
    for name, ins in ks.items():
        if want in name and ins:
            report(name, ins)


if __name__ == "__main__":
    main()
