#!/usr/bin/env python3
"""Developer lab: the look-up without a padding bit (fhe_tfhe_wop_pbs) at cfg5's ring -- N = 1024, n_lwe = 630, bootstrapping gadget (7, 3)
in the exact three-piece form, cb gadget (8, 3), pf gadget (7, 3), TLWE key switch (4, 8); uniform-random keys and ciphertexts: the work
does not depend on their values.  Timing only, nothing is decoded.

  tfhe_wop_lab.py [--out FILE]         every point -- m = 8 and 12, n_out = 1 and 8, batch 1, 64, 1024 -- each in a child process of its own
                                       under `timeout`; the first point that fails or runs out of time ends the run; the TFHE_WOP_LAB
                                       lines also go to FILE (default profiles/tfhe_wop_lab.txt)
  tfhe_wop_lab.py --point M N_OUT BATCH
                                       one point in this process: interleaved rounds (round 0 warms up), median of 5, seconds per call of
                                         whole    wop_pbs: one call
                                         rotate   its parts alone on the same stream: m many-LUT blind rotations of the batch,
                                         pfks     the private functional key switch of batch m cb_d rows,
                                         fill     TggswKey.fill of batch m selectors,
                                         lut      lut_eval_batch with the output key switch
                                                  (whole - the four = what the front, extraction and key-switch launches cost)
                                         parent   the route a user has without this entry, the bits already apart at bit << 62: one
                                                  bootstrap per bit in front (the extraction the parent cannot do in fewer),
                                                  circuit_bootstrap, TggswKey (fhe_tggsw_prepare), lut_eval_batch
                                         prepare  TggswKey (fhe_tggsw_prepare) of batch m selectors: host time blocked = the whole call;
                                         fill_host  host time of TggswKey.fill before it returns (device time: `fill`)
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POINT_SECONDS = 400
N, LOG_B, D, N_LWE = 1024, 7, 3, 630
CB, PF, KS = (8, 3), (7, 3), (4, 8)


def point(m, n_out, batch, rounds=5):
    import torch
    import learn_fhe_amd as F
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    rnd = lambda *shape: torch.randint(-(1 << 63), (1 << 63) - 1, shape, dtype=torch.int64, device=dev, generator=gen)  # noqa: E731
    C, W, t = F.tfhe_cbs, F.tfhe_wop, F.TorusContext()
    brk = F.TggswKey(t, LOG_B, D, rnd(N_LWE, 2 * D, N), rnd(N_LWE, 2 * D, N), N)
    sel = F.TggswKey.reserve(t, CB[0], CB[1], N, batch * m)
    pfksk = rnd(PF[1] * (N + 1), 2, 2, N)
    ks = (KS[0], KS[1], rnd(N * KS[1], N_LWE), rnd(N * KS[1]))
    oks = ks + (N_LWE,)
    r, per_acc, n_acc, n_polys = C.lut_shape(m, n_out, N)
    polys = rnd(n_polys, N)
    a, b = rnd(batch, N_LWE), rnd(batch)
    bits_a, bits_b = rnd(batch * m, N_LWE), rnd(batch * m)
    at, bt = a & (2 * N - 1), b & (2 * N - 1)
    tab = torch.from_numpy(W.wop_table(CB[0], CB[1], N, 56).view("int64")).to(dev)
    lev_a, lev_b = rnd(batch * m * CB[1], N), rnd(batch * m * CB[1])
    rows_a, rows_b = rnd(batch * m, 2 * CB[1], N), rnd(batch * m, 2 * CB[1], N)
    sel.fill(0, rows_a, rows_b)
    host = {}

    def rotate():
        for _ in range(m):
            brk.blind_rotate(at, bt, tab)

    def fill():
        t0 = time.perf_counter()
        sel.fill(0, rows_a, rows_b)
        host["fill_host"] = time.perf_counter() - t0

    def parent():
        xa, xb = brk.bootstrap(ks[0], ks[1], ks[2], ks[3], tab, bits_a, bits_b)
        sa, sb = C.circuit_bootstrap(brk, CB[0], CB[1], PF[0], PF[1], pfksk, xa, xb)
        key = F.TggswKey(t, CB[0], CB[1], sa, sb, N)
        C.lut_eval_batch(polys, key, 0, m, n_out, batch, oks)

    routes = {"whole": lambda: W.wop_pbs(brk, ks, CB[0], CB[1], PF[0], PF[1], pfksk, m, a, b, sel, 0, polys, n_out, oks),
              "rotate": rotate, "pfks": lambda: C.pfks(PF[0], PF[1], pfksk, 2, lev_a, lev_b, N, N, group=CB[1]), "fill": fill,
              "lut": lambda: C.lut_eval_batch(polys, sel, 0, m, n_out, batch, oks), "parent": parent,
              "prepare": lambda: F.TggswKey(t, CB[0], CB[1], rows_a, rows_b, N)}
    times = {k: [] for k in list(routes) + ["fill_host"]}
    for rd in range(rounds + 1):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rd:
                times[name].append(time.perf_counter() - t0)
                if name == "fill":
                    times["fill_host"].append(host["fill_host"])
    med = {k: statistics.median(x) for k, x in times.items()}
    parts = med["rotate"] + med["pfks"] + med["fill"] + med["lut"]
    out = dict(m=m, n_out=n_out, batch=batch, whole_s=round(med["whole"], 6), parts_s=round(parts, 6), rest_s=round(med["whole"] - parts, 6),
               rotate_s=round(med["rotate"], 6), pfks_s=round(med["pfks"], 6), fill_s=round(med["fill"], 6), lut_s=round(med["lut"], 6),
               parent_s=round(med["parent"], 6), factor=round(med["parent"] / med["whole"], 2), prepare_s=round(med["prepare"], 6),
               fill_host_s=round(med["fill_host"], 6), spread={k: [round(min(x), 6), round(max(x), 6)] for k, x in times.items()})
    print("TFHE_WOP_LAB " + json.dumps(out), flush=True)


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--point":
        point(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
        return 0
    out_path = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--out" else os.path.join(ROOT, "profiles", "tfhe_wop_lab.txt")
    with open(out_path, "w") as out:
        for m in (8, 12):
            for n_out in (1, 8):
                for batch in (1, 64, 1024):
                    r = subprocess.run(["timeout", "-k", "10", str(POINT_SECONDS), sys.executable, os.path.abspath(__file__), "--point", str(m), str(n_out),
                                        str(batch)], capture_output=True, text=True)
                    sys.stdout.write(r.stdout)
                    sys.stdout.flush()
                    out.writelines(line + "\n" for line in r.stdout.splitlines() if line.startswith("TFHE_WOP_LAB"))
                    out.flush()
                    if r.returncode != 0:
                        sys.stderr.write(r.stderr)
                        print("TFHE_WOP_LAB point m=%d n_out=%d batch=%d ended with status %d: stopping" % (m, n_out, batch, r.returncode), flush=True)
                        return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
