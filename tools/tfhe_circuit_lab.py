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

  tfhe_circuit_lab.py --many               the many-LUT row: the same steps, each timing the two-table adder circuit against the adder
                                           of one many-LUT node per block (--many-step MODE BATCH: one step in this process)

The table of DESIGN.md section 9 comes from the TFHE_CIRCUIT_LAB lines, that of section 9.2 from the TFHE_MANY_LAB lines.
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


def many_step(mode, batch, rounds=5):
    """The many-LUT row: the two-table adder circuit (7 blind rotations; unchanged code) against
    radix_add(..., many=True) (4 blind rotations of an interleaved table, 7 key-switch rows), interleaved rounds, median seconds per call.
    Timing only: at cfg5's parameters (n_lwe = 630) the mod-switch drift at log_funcs = 1 leaves about 3 sigma of margin at p = 16, so
    nothing is checked at decode level here (tests/test_tfhe_many_gpu.py decodes at n_lwe = 12)."""
    import torch
    import bench
    import learn_fhe_amd as F
    from learn_fhe_amd import tfhe_circuit as T
    dev = torch.device("cuda:0")
    S = bench.tfhe_setup(torch, F, dev, 0, batch)
    key = S["key"] if mode == "exact" else F.TggswKey(S["t"], S["log_b"], S["d"], S["raw"][0], S["raw"][1], S["n"], fft64=True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    in_a = torch.randint(-(1 << 63), (1 << 63) - 1, (8, batch, S["n_lwe"]), dtype=torch.int64, device=dev, generator=gen)
    in_b = torch.randint(-(1 << 63), (1 << 63) - 1, (8, batch), dtype=torch.int64, device=dev, generator=gen)
    routes, infos = {}, {}
    for name, many in (("two_table", False), ("many_lut", True)):
        b, _, _, outs = T.radix_add(4, 2, 2, many=many)
        cc = b.compile(outs, 4, 1, S["n"])
        tables = torch.from_numpy(cc.tables.view("int64")).to(dev)
        infos[name] = dict(cc.info(), **cc.info_many())
        routes[name] = (lambda cc=cc, tables=tables: cc.run(key, S["ks_lb"], S["ks_d"], S["ksa"], S["ksb"], (in_a, in_b), batch, tables=tables))
    times = {k: [] for k in routes}
    for r in range(rounds + 1):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                times[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    print("TFHE_MANY_LAB", json.dumps({"mode": mode, "batch": batch, "n": S["n"], "n_lwe": S["n_lwe"], "gadget": [S["log_b"], S["d"]],
                                       "key_switch": [S["ks_lb"], S["ks_d"]], "log_p": 4, "log_funcs": 1,
                                       "two_table": infos["two_table"], "many_lut": infos["many_lut"],
                                       "two_table_s": round(med["two_table"], 5), "many_lut_s": round(med["many_lut"], 5),
                                       "two_table_spread_s": [round(min(times["two_table"]), 5), round(max(times["two_table"]), 5)],
                                       "many_lut_spread_s": [round(min(times["many_lut"]), 5), round(max(times["many_lut"]), 5)],
                                       "additions_per_s": round(batch / med["many_lut"]), "speedup": round(med["two_table"] / med["many_lut"], 2),
                                       "decode_checked": False}), flush=True)
    return 0


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--step":
        return step(sys.argv[2], int(sys.argv[3]))
    if len(sys.argv) == 4 and sys.argv[1] == "--many-step":
        return many_step(sys.argv[2], int(sys.argv[3]))
    flag = "--many-step" if sys.argv[1:] == ["--many"] else "--step"
    for mode in ("exact", "fft64"):
        for batch in (1, 64, 1024):
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), flag, mode, str(batch)]
            rc = subprocess.call(cmd)
            if rc != 0:
                print("step %s %d ended with status %d: nothing more is started" % (mode, batch, rc), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
