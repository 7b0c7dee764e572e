#!/usr/bin/env python3
"""Developer lab: the vertically packed table look-up (fhe_tfhe_lut_eval) at cfg5's ring -- N = 1024, selector gadget (7, 3), the exact
three-piece key form; uniform-random selector rows: the work does not depend on their values.  Timing only, nothing is decoded.

  tfhe_lut_lab.py                      every point -- m = 8 and 12, n_out = 1 and 8, batch 1, 64, 1024 -- each in a child process of its own
                                       under `timeout`; the first point that fails or runs out of time ends the run
  tfhe_lut_lab.py --point M N_OUT BATCH
                                       one point in this process: interleaved rounds (round 0 warms up), median of 5, seconds per call of
                                         new     lut_eval_batch: one call for the batch
                                         fused, kernel
                                                 the same call with the lab switch LUT_EXTRACT = 1 (the ladder writes the extractions from its
                                                 registers) and = 2 (the accumulators are stored and a kernel of its own extracts)
                                         parent  the route before it: lut_eval (a CMUX tree over all m bits, one fhe_tggsw_cmux call per level)
                                                 looped over the ciphertexts and the n_out outputs.  A host loop is linear in its trips:
                                                 above 64 trips it is timed on 64 and scaled (the line says so)
                                         rotate  fhe_tfhe_blind_rotate at the same ring, gadget and batch (630 CMUXes per ciphertext)
                                       and from them the factor parent / new, the look-up's time per CMUX (new / CMUXes) against the
                                       blind rotation's (a look-up runs r + 2^h - 1 CMUXes per accumulator), and the key bytes a call streams (every ciphertext its own m selectors) against 8 TB/s

The table of DESIGN.md section 9.4 comes from the TFHE_LUT_LAB lines.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POINT_SECONDS = 240
N, LOG_B, D, N_LWE = 1024, 7, 3, 630
PARENT_TRIPS = 64
HBM_BYTES_PER_S = 8e12


def point(m, n_out, batch, rounds=5):
    import torch
    import learn_fhe_amd as F
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(12)
    rnd = lambda *shape: torch.randint(-(1 << 63), (1 << 63) - 1, shape, dtype=torch.int64, device=dev, generator=gen)  # noqa: E731
    C, t = F.tfhe_cbs, F.TorusContext()
    sel = F.TggswKey(t, LOG_B, D, rnd(batch * m, 2 * D, N), rnd(batch * m, 2 * D, N), N)
    brk = F.TggswKey(t, LOG_B, D, rnd(N_LWE, 2 * D, N), rnd(N_LWE, 2 * D, N), N)
    r, per_acc, n_acc, n_polys = C.lut_shape(m, n_out, N)
    polys = rnd(n_polys, N)
    tree = rnd(1 << m, N)                                   # the parent's table: 2^m polynomials, one entry each
    at, bt, v = rnd(batch, N_LWE) & (2 * N - 1), rnd(batch) & (2 * N - 1), rnd(N)
    trips = min(batch * n_out, PARENT_TRIPS)

    def parent():
        for i in range(trips):
            C.lut_eval(tree, sel, (i % batch) * m, m)

    def extract_route(value):
        def run():
            F.set_option("LUT_EXTRACT", value)
            try:
                C.lut_eval_batch(polys, sel, 0, m, n_out, batch)
            finally:
                F.set_option("LUT_EXTRACT", 0)
        return run

    routes = {"new": lambda: C.lut_eval_batch(polys, sel, 0, m, n_out, batch), "fused": extract_route(1), "kernel": extract_route(2), "parent": parent,
              "rotate": lambda: brk.blind_rotate(at, bt, v)}
    times = {k: [] for k in routes}
    for rd in range(rounds + 1):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rd:
                times[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(x) for k, x in times.items()}
    parent_s = med["parent"] * (batch * n_out) / trips
    cmuxes = batch * n_acc * (r + (1 << (m - r)) - 1)                    # per accumulator: r rotation steps and 2^h - 1 tree nodes
    key_bytes = cmuxes * (2 * D) * 2 * 3 * (N // 2) * 16                # per CMUX: 2d rows x (a | b) x 3 pieces x N / 2 complex
    out = dict(m=m, n_out=n_out, batch=batch, r=r, tree_bits=m - r, n_acc=n_acc, new_s=round(med["new"], 6), parent_s=round(parent_s, 6),
               parent_timed_trips=trips, parent_scaled=trips != batch * n_out, factor=round(parent_s / med["new"], 1),
               fused_extract_s=round(med["fused"], 6), kernel_extract_s=round(med["kernel"], 6), rotate_s=round(med["rotate"], 6), cmuxes=cmuxes,
               us_per_cmux_lut=round(1e6 * med["new"] / cmuxes, 3),
               us_per_cmux_rotate=round(1e6 * med["rotate"] / (N_LWE * batch), 3), key_gb=round(key_bytes / 1e9, 3),
               key_floor_s=round(key_bytes / HBM_BYTES_PER_S, 6), spread={k: [round(min(x), 6), round(max(x), 6)] for k, x in times.items()})
    print("TFHE_LUT_LAB " + json.dumps(out), flush=True)


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--point":
        point(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
        return 0
    for m in (8, 12):
        for n_out in (1, 8):
            for batch in (1, 64, 1024):
                rc = subprocess.call(["timeout", "-k", "10", str(POINT_SECONDS), sys.executable, os.path.abspath(__file__), "--point", str(m), str(n_out),
                                      str(batch)])
                if rc != 0:
                    print("TFHE_LUT_LAB point m=%d n_out=%d batch=%d ended with status %d: stopping" % (m, n_out, batch, rc), flush=True)
                    return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
