#!/usr/bin/env python3
"""Developer lab: the split TFHE blind rotation at cfg5's parameters -- N = 1024, n_lwe = 630, bootstrapping gadget (7, 3) in the exact
three-piece form; uniform-random keys and ciphertexts (the work does not depend on their values; a~ = 0, a skipped step, has its natural
share of one in 2N).  Timing only.

  tfhe_split_lab.py [--out FILE]   fhe_tfhe_blind_rotate with G = 1, 2, 6 workgroups per ciphertext (set_option("TFHE_SPLIT", 0 / 2 / 6))
                                   x batch 1, 2, 4, 8, 16, 32, 42, 64, 128, each where the call admits it (batch x G <= compute units,
                                   else "-"): the table of DESIGN.md section 9.6 and of the rule in csrc/tfhe_split.hpp.  Interleaved
                                   rounds in one process (round 0 warms up), median of five, with the spread of the G = 1 runs; the
                                   TFHE_SPLIT_LAB lines also go to FILE (default profiles/tfhe_split_lab.txt)
  tfhe_split_lab.py --wop          fhe_tfhe_wop_pbs at m = 8, n_out = 1, batch 1 and 64 (the rows of DESIGN.md section 9.5) under
                                   TFHE_SPLIT = 0 (the one-workgroup kernel: what the library ran before the split) and -1 (the rule),
                                   interleaved, median of five
A library status other than FHE_OK (a timeout word) ends the run.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, LOG_B, D, N_LWE = 1024, 7, 3, 630
BATCHES = (1, 2, 4, 8, 16, 32, 42, 64, 128)
ROUNDS = 5


def setup():
    import torch
    import learn_fhe_amd as F
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(17)
    rnd = lambda *shape: torch.randint(-(1 << 63), (1 << 63) - 1, shape, dtype=torch.int64, device=dev, generator=gen)  # noqa: E731
    t = F.TorusContext()
    brk = F.TggswKey(t, LOG_B, D, rnd(N_LWE, 2 * D, N), rnd(N_LWE, 2 * D, N), N)
    assert brk.form == "x3"
    return torch, F, rnd, t, brk


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def sweep(out_path):
    torch, F, rnd, t, brk = setup()
    v = rnd(N)
    lines = []
    try:
        for batch in BATCHES:
            at, bt = rnd(batch, N_LWE) & (2 * N - 1), rnd(batch) & (2 * N - 1)
            times = {1: [], 2: [], 6: []}
            for r in range(ROUNDS + 1):
                for g in times:
                    F.set_option("TFHE_SPLIT", 0 if g == 1 else g)
                    if brk.split(batch) != g:
                        continue
                    dt = timed(torch, lambda: brk.blind_rotate(at, bt, v))
                    brk.check(at)  # raises on a timeout word: the run ends here
                    if r:
                        times[g].append(dt)
            row = dict(batch=batch, n_lwe=N_LWE,
                       ms={g: (round(1e3 * statistics.median(x), 4) if x else None) for g, x in times.items()},
                       spread_ms={g: ([round(1e3 * min(x), 4), round(1e3 * max(x), 4)] if x else None) for g, x in times.items()})
            line = "TFHE_SPLIT_LAB " + json.dumps(row)
            print(line, flush=True)
            lines.append(line)
    finally:
        F.set_option("TFHE_SPLIT", -1)
        with open(out_path, "w") as f:
            f.writelines(x + "\n" for x in lines)


def wop():
    torch, F, rnd, t, brk = setup()
    C, W = F.tfhe_cbs, F.tfhe_wop
    CB, PF, KS = (8, 3), (7, 3), (4, 8)
    m, n_out = 8, 1
    pfksk = rnd(PF[1] * (N + 1), 2, 2, N)
    ks = (KS[0], KS[1], rnd(N * KS[1], N_LWE), rnd(N * KS[1]))
    oks = ks + (N_LWE,)
    polys = rnd(C.lut_shape(m, n_out, N)[3], N)
    try:
        for batch in (1, 64):
            sel = F.TggswKey.reserve(t, CB[0], CB[1], N, batch * m)
            a, b = rnd(batch, N_LWE), rnd(batch)
            times = {0: [], -1: []}
            for r in range(ROUNDS + 1):
                for opt in times:
                    F.set_option("TFHE_SPLIT", opt)
                    dt = timed(torch, lambda: W.wop_pbs(brk, ks, CB[0], CB[1], PF[0], PF[1], pfksk, m, a, b, sel, 0, polys, n_out, oks))
                    brk.check(a)
                    if r:
                        times[opt].append(dt)
            F.set_option("TFHE_SPLIT", -1)
            row = dict(wop_pbs=dict(m=m, n_out=n_out, batch=batch), g_of_the_rotations=brk.split(batch),
                       ms={("one_workgroup" if o == 0 else "rule"): round(1e3 * statistics.median(x), 3) for o, x in times.items()},
                       spread_ms={("one_workgroup" if o == 0 else "rule"): [round(1e3 * min(x), 3), round(1e3 * max(x), 3)] for o, x in times.items()})
            print("TFHE_SPLIT_LAB " + json.dumps(row), flush=True)
    finally:
        F.set_option("TFHE_SPLIT", -1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--wop":
        wop()
    else:
        sweep(sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "tfhe_split_lab.txt"))
