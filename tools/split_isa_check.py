#!/usr/bin/env python3
"""Checks the disassembly of the split blind-rotation kernels (learn-fhe_amd/csrc/fhew_split_kernels.hpp) against the four points
of an in-launch hand-off: (1) every payload store is write-through (sc1), (2) an `s_waitcnt vmcnt(0)` and the workgroup barrier lie
between the last payload store and the flag store, (3) flag, timeout and status words are written by sc1 vector stores (what an
agent-scope atomic store lowers to) and polled by an sc1 vector load, (4) the slabs are read by vector loads behind ONE
`buffer_inv sc1`: the scalar loads of the kernel read kernel arguments, twiddles and the op list only (their count is printed so
that a change shows).  Prints registers and spills per instantiation from the compiler's remarks.
usage: split_isa_check.py fhew_api.s [resource-usage remarks]; exit status 1 if a point fails"""
import re
import sys

text = open(sys.argv[1]).read()
remarks = open(sys.argv[2]).read() if len(sys.argv) > 2 else ""
bad = 0
for f in re.split(r"\n(?=_ZN3fhe\w+:\s)", text):
    name = f.split(":", 1)[0]
    if "blind_rotate_split_kernel" not in name:
        continue
    lines = f.split("\n")
    payload = [i for i, l in enumerate(lines) if "buffer_store_dwordx4" in l]
    words = [i for i, l in enumerate(lines) if re.search(r"global_store_dword\b", l)]
    flag = words[0] if words else -1
    between = lines[payload[-1]:flag] if payload and flag > payload[-1] else []
    checks = {
        "payload stores sc1": bool(payload) and all("sc1" in lines[i] for i in payload),
        "vmcnt(0) and barrier before the flag": any("s_waitcnt vmcnt(0)" in x for x in between) and any("s_barrier" in x for x in between),
        "flag/timeout/status stores sc1": bool(words) and all("sc1" in lines[i] for i in words),
        "poll is an sc1 vector load": sum(1 for l in lines if re.search(r"global_load_dword\b.*sc1", l)) == 1,
        "one buffer_inv sc1": sum(1 for l in lines if "buffer_inv sc1" in l) == 1,
        "no scalar store or scalar atomic": not any(re.match(r"\s*s_(buffer_|scratch_)?(store|atomic)", l) for l in lines),
        "no scratch": not any(re.match(r"\s*scratch_", l) for l in lines),
    }
    slab_loads = sum(1 for l in lines if re.search(r"global_load_dwordx4", l))
    scalar_loads = sum(1 for l in lines if re.match(r"\s*s_(buffer_)?load", l))
    short = re.sub(r"_ZN3fhe25blind_rotate_split_kernelINS_|EEEEEvNS.*", "", name)
    m = re.search(re.escape(name) + r".*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)",
                  remarks, flags=re.S)
    regs = "sgpr %s vgpr %s scratch %s sgpr-spill %s vgpr-spill %s" % m.groups() if m else "(no remarks given)"
    if m and (int(m.group(3)) or int(m.group(4)) or int(m.group(5))):
        checks["zero spills"] = False
    print("%s: %s; payload stores %d, 16-byte vector loads %d, scalar loads %d" % (short, regs, len(payload), slab_loads, scalar_loads))
    for k, v in checks.items():
        print("    %-40s %s" % (k, "ok" if v else "FAIL"))
        bad += not v
sys.exit(1 if bad else 0)
