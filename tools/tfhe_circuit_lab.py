#!/usr/bin/env python3
"""Developer lab: the 8-bit adder of 4 blocks of 2 message + 2 carry bits (tfhe_circuit.radix_add) as ONE circuit call
(fhe_tfhe_circuit_run) against the same netlist run node by node through what the library offered before the circuits: the linear
combination as wrapping int64 tensor arithmetic, then fhe_tfhe_bootstrap with the node's table.  cfg5's parameters (bench.tfhe_setup:
N = 1024, n_lwe = 630, gadget (7, 3), key switch (4, 5); uniform-random keys: the work of a bootstrap does not depend on the key's
values), exact key form or fft64.

  tfhe_circuit_lab.py                      every step -- batches 1, 64 and 1024, exact and fft64 -- each in a child process of its own
                                           under `timeout`; the first step that fails or runs out of time ends the run
  tfhe_circuit_lab.py --step MODE BATCH    one step in this process: interleaved rounds (round 0 warms up), median seconds per call of
                                           both routes, gates (live nodes x batch) per second, and whether their outputs are the same bits

The table of DESIGN.md section 9 comes from the TFHE_CIRCUIT_LAB lines.
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


def step(mode, batch, rounds=5):
    import torch
    import bench
    import learn_fhe_amd as F
    from learn_fhe_amd import tfhe_circuit as T
    dev = torch.device("cuda:0")
    S = bench.tfhe_setup(torch, F, dev, 0, batch)
    key = S["key"] if mode == "exact" else F.TggswKey(S["t"], S["log_b"], S["d"], S["raw"][0], S["raw"][1], S["n"], fft64=True)
    b, _, _, outs = T.radix_add(4, 2, 2)
    cc = b.compile(outs, 4, 1, S["n"])
    tables = torch.from_numpy(cc.tables.view("int64")).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    in_a = torch.randint(-(1 << 63), (1 << 63) - 1, (8, batch, S["n_lwe"]), dtype=torch.int64, device=dev, generator=gen)
    in_b = torch.randint(-(1 << 63), (1 << 63) - 1, (8, batch), dtype=torch.int64, device=dev, generator=gen)
    live = cc.levels()

    def node_by_node():
        vals = []
        get = lambda w: (in_a[w.index], in_b[w.index]) if w.is_input else vals[w.index]  # noqa: E731
        for g, (terms, table, constant) in enumerate(b.nodes):
            if not live[g]:
                vals.append(None)
                continue
            sa = sum(k * get(w)[0] for w, k in terms)
            sb = sum(k * get(w)[1] for w, k in terms)
            vals.append(key.bootstrap(S["ks_lb"], S["ks_d"], S["ksa"], S["ksb"], tables[table], sa, sb))
        return torch.stack([get(w)[0] for w in outs]), torch.stack([get(w)[1] for w in outs])

    routes = {"circuit": lambda: cc.run(key, S["ks_lb"], S["ks_d"], S["ksa"], S["ksb"], (in_a, in_b), batch, tables=tables), "node_by_node": node_by_node}
    times, last = {k: [] for k in routes}, {}
    for r in range(rounds + 1):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if r:
                times[name].append(time.perf_counter() - t0)
    same = all(torch.equal(last["circuit"][i].reshape(-1), last["node_by_node"][i].reshape(-1)) for i in (0, 1))
    info = cc.info()
    med = {k: statistics.median(v) for k, v in times.items()}
    gates = info["live_nodes"] * batch
    print("TFHE_CIRCUIT_LAB", json.dumps({"mode": mode, "batch": batch, "live_nodes": info["live_nodes"], "levels": info["levels"], "max_width": info["max_width"],
                                          "circuit_s": round(med["circuit"], 5), "node_by_node_s": round(med["node_by_node"], 5),
                                          "circuit_gates_per_s": round(gates / med["circuit"]), "node_by_node_gates_per_s": round(gates / med["node_by_node"]),
                                          "circuit_spread_s": [round(min(times["circuit"]), 5), round(max(times["circuit"]), 5)],
                                          "node_by_node_spread_s": [round(min(times["node_by_node"]), 5), round(max(times["node_by_node"]), 5)],
                                          "speedup": round(med["node_by_node"] / med["circuit"], 2), "same_bits": bool(same)}), flush=True)
    return 0 if same else 1


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(sys.argv[3]))
    for mode in ("exact", "fft64"):
        for batch in (1, 64, 1024):
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", mode, str(batch)]
            rc = subprocess.call(cmd)
            if rc != 0:
                print("step %s %d ended with status %d: nothing more is started" % (mode, batch, rc), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
