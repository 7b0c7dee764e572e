#!/usr/bin/env python3
"""Developer lab: the packing key switch fhe_tlwe_pack against the composed route (fhe_tlwe_pfks with a one-function key, fhe_tglwe_rotate
per position, additions) at n = 1024.  Uniform-random keys and ciphertexts: the work does not depend on their values.  Before a cell is
timed its five outputs are compared bit for bit.

  tfhe_pack_lab.py                       every step -- n_in in {630, 1024} x gadget in {(7, 5), (8, 4)} -- each in a child process of its
                                         own under `timeout`; the first step that fails or runs out of time ends the run
  tfhe_pack_lab.py --step N_IN LOG_B D   one step in this process: count in {1, 16, 32, 64, 128, 1024} x packs in {1, 16}; per cell
                                         interleaved rounds of fhe_tlwe_pack under the library's rules, on the transforms (PACK_ROUTE = 1)
                                         with PACK_SPLIT = 0 (the library's rule) and 1 (one chunk per pack), on the scalar product
                                         (PACK_ROUTE = 2), and of the composed route, each repeated until a round lasts 50 ms; median
                                         seconds per call, host clock around a device synchronise

The table of DESIGN.md section 9.8 comes from the TFHE_PACK_LAB lines.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_SECONDS = 240
N = 1024
N_INS = (630, 1024)
GADGETS = ((7, 5), (8, 4))
COUNTS = (1, 16, 32, 64, 128, 1024)
PACKS = (1, 16)
WINDOW_S = 0.05


def timed(torch, routes, rounds):
    """-> {route: median seconds per call}, {route: [min, max]}: every round runs each route `reps` times between two synchronises"""
    reps, times = {}, {k: [] for k in routes}
    for name, fn in routes.items():  # warm-up, and how often a call fits the window
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps[name] = max(1, min(200, int(WINDOW_S / max(time.perf_counter() - t0, 1e-6)) + 1))
    for _ in range(rounds):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps[name])
    return {k: statistics.median(v) for k, v in times.items()}, {k: [round(min(v), 7), round(max(v), 7)] for k, v in times.items()}


def step(n_in, log_b, d, rounds=5):
    import torch
    import learn_fhe_amd as F
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    rnd = lambda *shape: torch.randint(-(1 << 63), (1 << 63) - 1, shape, dtype=torch.int64, device=dev, generator=gen)  # noqa: E731
    t = F.TorusContext()
    pfksk = rnd(d * (n_in + 1), 1, 2, N)
    key = F.PackKey(t, log_b, d, pfksk, n_in, N)

    def fused(route, split, ca, cb, count, stride):
        F.set_option("PACK_ROUTE", route)
        F.set_option("PACK_SPLIT", split)
        return F.pack(key, ca, cb, count, stride)

    try:
        for count in COUNTS:
            stride = N // count
            for packs in PACKS:
                ca, cb = rnd(packs, count, n_in), rnd(packs, count)
                routes = {"pack_rule": lambda: fused(0, 0, ca, cb, count, stride), "pack_transforms": lambda: fused(1, 0, ca, cb, count, stride),
                          "pack_one_chunk": lambda: fused(1, 1, ca, cb, count, stride), "pack_scalar": lambda: fused(2, 0, ca, cb, count, stride),
                          "composed": lambda: F.pack_composed(log_b, d, pfksk, ca, cb, n_in, N, count, stride)}
                outs = {k: fn() for k, fn in routes.items()}
                same = all(torch.equal(outs[k][h], outs["composed"][h]) for k in routes for h in (0, 1))
                del outs
                if not same:
                    print("TFHE_PACK_LAB outputs differ at", n_in, log_b, d, count, packs, flush=True)
                    return 1
                med, spread = timed(torch, routes, rounds)
                print("TFHE_PACK_LAB", json.dumps({"n": N, "n_in": n_in, "gadget": [log_b, d], "count": count, "stride": stride, "packs": packs,
                                                   "key_rows": d * (n_in + 1), "pack_rule_ms": round(1e3 * med["pack_rule"], 4),
                                                   "pack_transforms_ms": round(1e3 * med["pack_transforms"], 4),
                                                   "pack_one_chunk_ms": round(1e3 * med["pack_one_chunk"], 4),
                                                   "pack_scalar_ms": round(1e3 * med["pack_scalar"], 4),
                                                   "composed_ms": round(1e3 * med["composed"], 4),
                                                   "composed_over_rule": round(med["composed"] / med["pack_rule"], 2), "spread_s": spread}), flush=True)
    finally:
        F.set_option("PACK_SPLIT", 0)
        F.set_option("PACK_ROUTE", 0)
    return 0


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--step":
        return step(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    for n_in in N_INS:
        for log_b, d in GADGETS:
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", str(n_in), str(log_b), str(d)]
            rc = subprocess.call(cmd)
            if rc != 0:
                print("step %d (%d, %d) ended with status %d: nothing more is started" % (n_in, log_b, d, rc), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
