#!/usr/bin/env python3
"""Developer lab: `FhewU8::wrapping_add` / `wrapping_mul` as ONE circuit call (fhe_fhew_circuit_run) against the same netlist run
gate by gate through ring.Fhew, at cfg3's parameters (bench.fhew_setup: N = 1024, 54-bit q, base 2^6 x 9, n_lwe = 100, w = 10, key
switch over 2^16 with base 2^4 x 4; uniform-random keys: the work of a gate does not depend on the key's values).

  fhew_circuit_lab.py                      every step -- add and mul at 1, 16 and 256 bytes -- each in a child process of its own
                                           under `timeout`; the first step that fails or runs out of time ends the run
  fhew_circuit_lab.py --step OP BYTES      one step in this process: interleaved rounds (round 0 warms up), median seconds per
                                           call of both routes, and whether their outputs are the same bits

The table of DESIGN.md section 4.4c comes from the CIRCUIT_LAB lines.
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


def step(op, nbytes, rounds=5):
    import torch
    import bench
    import learn_fhe_amd as F
    from learn_fhe_amd import circuit as K
    dev = torch.device("cuda:0")
    S = bench.fhew_setup(torch, F, dev, 0)
    ev = F.Fhew(S["bk"], S["q_ks"], S["kb"], S["kd"], S["ksk_a"], S["ksk_b"])
    c = F.Circuit()
    x, y = c.input_u8(), c.input_u8()
    outs = K.u8_wrapping_add(c, x, y) if op == "add" else K.u8_wrapping_mul(c, x, y)
    cc = c.compile(outs)
    in_a, in_b = S["rnd"](16, nbytes, S["n"]), S["rnd"](16, nbytes)
    pairs = [(in_a[i], in_b[i]) for i in range(16)]
    routes = {"circuit": lambda: cc.run(ev, (in_a, in_b), nbytes),
              "gate_by_gate": lambda: c.evaluate_fhew(ev, pairs, outs)}
    times, last = {k: [] for k in routes}, {}
    for r in range(rounds + 1):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            S["bk"].check(in_a)  # raises on a status word: the step ends here
            if r:
                times[name].append(dt)
    same = all(torch.equal(last["circuit"][0][o], g[0].reshape(nbytes, S["n"])) and torch.equal(last["circuit"][1][o], g[1].reshape(nbytes))
               for o, g in enumerate(last["gate_by_gate"]))
    info = cc.info()
    med = {k: statistics.median(v) for k, v in times.items()}
    print("CIRCUIT_LAB", json.dumps({"op": op, "bytes": nbytes, "gates": len(c.gates), "live_gates": info["live_gates"], "levels": info["levels"],
                                     "max_width": info["max_width"], "split_at_width_1": S["bk"].split(nbytes),
                                     "circuit_s": round(med["circuit"], 5), "gate_by_gate_s": round(med["gate_by_gate"], 5),
                                     "circuit_spread_s": [round(min(times["circuit"]), 5), round(max(times["circuit"]), 5)],
                                     "gate_by_gate_spread_s": [round(min(times["gate_by_gate"]), 5), round(max(times["gate_by_gate"]), 5)],
                                     "speedup": round(med["gate_by_gate"] / med["circuit"], 2), "same_bits": bool(same)}), flush=True)
    return 0 if same else 1


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(sys.argv[3]))
    for op in ("add", "mul"):
        for nbytes in (1, 16, 256):
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", op, str(nbytes)]
            rc = subprocess.call(cmd)
            if rc != 0:
                print("step %s %d ended with status %d: nothing more is started" % (op, nbytes, rc), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
