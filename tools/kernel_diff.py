#!/usr/bin/env python3
"""Device code of two builds of the library, kernel by kernel:  tools/kernel_diff.py PARENT.so BRANCH.so
The gfx950 code object of each (unbundled as tools/kernel_resources.sh does) is disassembled; per kernel symbol the instruction text -- address comments and
<symbol+offset> annotations stripped -- and the register / scratch / LDS notes are compared. Exit 1 if a kernel both builds have differs. Needs no GPU."""
import os, re, subprocess, sys, tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "lib", "llvm", "bin")
ARCH = os.environ.get("RNB_OFFLOAD_ARCH", "gfx950")


def code_object(so, tmp):
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, os.path.basename(so) + "." + str(len(os.listdir(tmp))) + ".co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, so])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--" + ARCH, "--input=" + fat, "--output=" + co, "--unbundle"])
    return co


def kernels(co):
    """{symbol: [instruction lines]}, {symbol: 'vgpr sgpr scratch vgpr_spill sgpr_spill lds'}"""
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", "--mcpu=" + ARCH, co], text=True)
    code, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^<(\S+)>:$", line.strip())
        if m:
            name = m.group(1); code[name] = []
        elif name and line.strip():
            code[name].append(re.sub(r"\s*<[^>]+>", "", re.sub(r"\s*//.*$", "", line)).strip())
    notes, res, cur = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True), {}, {}
    for key, val in re.findall(r"\.(name|vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size|wavefront_size):\s+(\S+)", notes):
        cur[key] = val
        if key == "wavefront_size":  # the last key of a kernel's record
            res[cur["name"]] = " ".join("%s %s" % (k, cur.get(k)) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size"))
    return {k: v for k, v in code.items() if k in res}, res


def literals_only(x, y):
    """x and y are one PC-relative address computation with another literal (constant data moves when the object in front of it changes length)"""
    blank = lambda t: re.sub(r"0x[0-9a-f]+|\b\d+\b", "#", t)
    return x.startswith(("s_add_u32", "s_addc_u32", "s_getpc")) and blank(x) == blank(y)


def main(parent, branch):
    with tempfile.TemporaryDirectory() as tmp:
        (ca, ra), (cb, rb) = kernels(code_object(parent, tmp)), kernels(code_object(branch, tmp))
    print("kernels: %d in %s, %d in %s" % (len(ca), parent, len(cb), branch))
    for k in sorted(set(ca) - set(cb)): print("only in parent:", k)
    for k in sorted(set(cb) - set(ca)): print("only in branch:", k)
    common, differ = sorted(set(ca) & set(cb)), 0
    for k in common:
        lines = [(x, y) for x, y in zip(ca[k], cb[k]) if x != y]
        code_differs = len(ca[k]) != len(cb[k]) or not all(literals_only(x, y) for x, y in lines)
        if ra[k] != rb[k]: print("RESOURCES DIFFER %s\n  parent %s\n  branch %s" % (k, ra[k], rb[k]))
        if code_differs: print("CODE DIFFERS %s: %d vs %d instructions, %d differing lines" % (k, len(ca[k]), len(cb[k]), len(lines)))
        elif lines: print("pc-relative literals only: %s" % k)
        for x, y in (lines[:8] if code_differs else lines): print("  - %s\n  + %s" % (x, y))
        differ += code_differs or ra[k] != rb[k]
    print("%d common kernels, %d differ in instructions or resources" % (len(common), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
