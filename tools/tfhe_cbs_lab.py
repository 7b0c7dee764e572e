#!/usr/bin/env python3
"""Developer lab: the circuit bootstrap at cfg5's ring (bench.tfhe_setup: N = 1024, n_lwe = 630, bootstrapping gadget (7, 3); uniform-random
keys: the work does not depend on the key's values).  Timing only, nothing is decoded.  cb gadget (8, 3) (nu = 2); pf gadget (7, 3)
(100.8 MB of key) and (7, 5) (168.0 MB).

  tfhe_cbs_lab.py                 every step -- batches 1, 64 and 1024 -- each in a child process of its own under `timeout`; the first
                                  step that fails or runs out of time ends the run
  tfhe_cbs_lab.py --step BATCH    one step in this process: interleaved rounds (round 0 warms up), median seconds per call of
                                  the many-LUT blind rotation that feeds the key switch (existing code: the yardstick), of fhe_tlwe_pfks
                                  alone on its batch * 3 extracted rows and of fhe_tfhe_circuit_bootstrap; bits bootstrapped per second;
                                  key bytes read (passes over the key x its size) over time against 8 TB/s
  tfhe_cbs_lab.py --chunk BATCH   fhe_tlwe_pfks alone under the lab switch PFKS_CHUNK = 32, 64, 128, 256, 1024 (digits a block keeps in LDS)

The table of DESIGN.md section 9.3 comes from the TFHE_CBS_LAB lines.
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
CB = (8, 3)
PF = ((7, 3), (7, 5))
HBM_BYTES_PER_S = 8e12


def setup(batch):
    import torch
    import bench
    import learn_fhe_amd as F
    dev = torch.device("cuda:0")
    S = bench.tfhe_setup(torch, F, dev, 0, batch)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    rnd = lambda *shape: torch.randint(-(1 << 63), (1 << 63) - 1, shape, dtype=torch.int64, device=dev, generator=gen)  # noqa: E731
    return torch, F, S, rnd


def timed(torch, routes, rounds):
    times = {k: [] for k in routes}
    for r in range(rounds + 1):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                times[name].append(time.perf_counter() - t0)
    return {k: statistics.median(v) for k, v in times.items()}, {k: [round(min(v), 6), round(max(v), 6)] for k, v in times.items()}


def step(batch, rounds=5):
    torch, F, S, rnd = setup(batch)
    C = F.tfhe_cbs
    n, cb_d = S["n"], CB[1]
    nu = C.cbs_nu(cb_d)
    table = torch.from_numpy(C.cbs_table(CB[0], cb_d, n).view("int64")).cuda()
    at, bt = F.TorusContext.mod_switch_many(S["a_raw"], n, nu), F.TorusContext.mod_switch_many(S["b_raw"], n, nu)
    ea, eb = rnd(batch * cb_d, n), rnd(batch * cb_d)
    keys = {pf: rnd(pf[1] * (n + 1), 2, 2, n) for pf in PF}
    routes = {"rotation": lambda: S["key"].blind_rotate(at, bt, table)}
    for pf in PF:
        routes["pfks_%d_%d" % pf] = (lambda pf=pf: C.pfks(pf[0], pf[1], keys[pf], 2, ea, eb, n, n, group=cb_d))
        routes["cbs_%d_%d" % pf] = (lambda pf=pf: C.circuit_bootstrap(S["key"], CB[0], cb_d, pf[0], pf[1], keys[pf], S["a_raw"], S["b_raw"]))
    med, spread = timed(torch, routes, rounds)
    tile = 1 if batch * cb_d == 1 else (4 if batch * cb_d <= 4 else 16)
    passes = -(-batch * cb_d // tile)
    out = {"batch": batch, "n": n, "n_lwe": S["n_lwe"], "brk_gadget": [S["log_b"], S["d"]], "cb_gadget": list(CB), "rotation_ms": round(1e3 * med["rotation"], 3),
           "key_passes": passes, "spread_s": spread}
    for pf in PF:
        key_bytes = keys[pf].numel() * 8
        p, c = med["pfks_%d_%d" % pf], med["cbs_%d_%d" % pf]
        out["pf_%d_%d" % pf] = {"key_MB": round(key_bytes / 1e6, 1), "pfks_ms": round(1e3 * p, 3), "cbs_ms": round(1e3 * c, 3), "bits_per_s": round(batch / c),
                                "key_bytes_read_over_time_vs_8TBs": round(passes * key_bytes / p / HBM_BYTES_PER_S, 4),
                                "pfks_over_rotation": round(p / med["rotation"], 3)}
    print("TFHE_CBS_LAB", json.dumps(out), flush=True)
    return 0


def chunk_step(batch, rounds=5):
    torch, F, S, rnd = setup(batch)
    n, cb_d, pf = S["n"], CB[1], PF[0]
    ea, eb, key = rnd(batch * cb_d, n), rnd(batch * cb_d), rnd(pf[1] * (n + 1), 2, 2, n)
    chunks = (32, 64, 128, 256, 1024)

    def run(c):
        F.set_option("PFKS_CHUNK", c)
        return F.tfhe_cbs.pfks(pf[0], pf[1], key, 2, ea, eb, n, n, group=cb_d)

    try:
        med, spread = timed(torch, {str(c): (lambda c=c: run(c)) for c in chunks}, rounds)
    finally:
        F.set_option("PFKS_CHUNK", 0)
    print("TFHE_CBS_CHUNK_LAB", json.dumps({"batch": batch, "pf_gadget": list(pf), "pfks_ms_by_chunk": {k: round(1e3 * v, 3) for k, v in med.items()},
                                            "spread_s": spread}), flush=True)
    return 0


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        return step(int(sys.argv[2]))
    if len(sys.argv) == 3 and sys.argv[1] == "--chunk":
        return chunk_step(int(sys.argv[2]))
    for batch in (1, 64, 1024):
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", str(batch)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("step %d ended with status %d: nothing more is started" % (batch, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
