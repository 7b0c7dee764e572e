#!/usr/bin/env python3
"""Lists every device kernel the library was built with: one sorted line per kernel with its unit, mangled name, VGPRs, SGPRs,
scratch bytes, static LDS bytes, VGPR and SGPR spills, read from the gfx950 code object inside each object file
(llvm-objcopy -> clang-offload-bundler -> llvm-readelf --notes).  Needs no GPU.  A change to host code alone (csrc/dispatch.hpp and
the entry points) must leave the listing as it is: a line more is a list crossed too widely, a line less a combination dropped.
usage: kernel_inventory.py [learn-fhe_amd/lib/obj] > profiles/kernel_inventory.txt   (the kernel count goes to stderr)"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
FIELDS = ("name", "vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")

objdir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "learn-fhe_amd", "lib", "obj")
rows = []
with tempfile.TemporaryDirectory() as tmp:
    for obj in sorted(os.listdir(objdir)):
        if not obj.endswith(".o"):
            continue
        unit = obj[:-2]
        fat, co = os.path.join(tmp, unit + ".fat"), os.path.join(tmp, unit + ".co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, os.path.join(objdir, obj), os.devnull])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
        for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
            rows.append((unit,) + tuple(re.search(r"\.%s:\s+(\S+)" % f, blk).group(1) for f in FIELDS))
rows.sort()
print("# unit name vgpr sgpr scratch_bytes static_lds_bytes vgpr_spill sgpr_spill")
for r in rows:
    print(" ".join(r))
print("# kernels: %d" % len(rows), file=sys.stderr)
