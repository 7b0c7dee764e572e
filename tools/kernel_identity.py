#!/usr/bin/env python3
"""Are the device kernels of two builds the same instruction streams?  Compares, kernel by kernel, two hipcc -S listings or two object
directories (learn-fhe_amd/lib/obj: the gfx950 code object of every unit is disassembled with llvm-objdump) and prints the kernels
that differ or exist on one side only, with their instruction counts.  What is compared: mnemonics and operands in order.  Left out:
comments, assembler directives, the function number in local labels (.LBB<n>_<m>) and the addresses llvm-objdump prints.  Needs no
GPU.  Exit status 1 if anything differs.
usage: kernel_identity.py OLD NEW     (both *.s listings, or both object directories)"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def norm(line):
    line = re.split(r";|//", line, 1)[0].strip()
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    line = re.sub(r"\s*<[^>]*>", "", line)  # objdump's symbolic branch targets
    return re.sub(r"\s+", " ", line)


def streams(text, head):
    """{kernel: [instruction, ...]} of one listing; `head` matches the line that opens a function"""
    out, cur = {}, None
    for line in text.splitlines():
        m = head.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        ins = norm(line)
        if re.match(r"^[a-z]+_", ins):
            cur.append(ins)
            if ins.startswith("s_endpgm"):
                cur = None
    return {k: v for k, v in out.items() if v}


def load(path):
    if os.path.isfile(path):
        return {("", k): v for k, v in streams(open(path).read(), re.compile(r"^(_Z\S+):")).items()}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(f for f in os.listdir(path) if f.endswith(".o")):
            fat, co = os.path.join(tmp, obj + ".fat"), os.path.join(tmp, obj + ".co")
            subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, os.path.join(path, obj), os.devnull])
            subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
            dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
            for k, v in streams(dis, re.compile(r"^(?:[0-9a-f]+ )?<(_Z\S+)>:")).items():
                out[(obj[:-2], k)] = v
    return out


def main():
    old, new = load(sys.argv[1]), load(sys.argv[2])
    differ = 0
    for key in sorted(set(old) | set(new)):
        a, b = old.get(key), new.get(key)
        if a == b:
            continue
        differ += 1
        name = " ".join(x for x in key if x)
        if a is None or b is None:
            print("%s  only in %s  %d instructions" % (name, "NEW" if a is None else "OLD", len(b if a is None else a)))
        else:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print("%s  differs  %d -> %d instructions, first at %d" % (name, len(a), len(b), first))
    total = sum(len(v) for v in new.values())
    print("# kernels: %d old, %d new; %d differ; %d instructions compared" % (len(old), len(new), differ, total))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
