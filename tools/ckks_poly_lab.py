#!/usr/bin/env python3
"""Times fhe_ckks_poly_apply against the op-by-op composition (fhe_ckks_mul on prefix slices + fhe_ckks_lincomb) for a degree-31
Chebyshev series: n = 2^13 and 2^15, L = 12, batch 1 / 8 / 64.  Prints one line per shape with both times (median of --samples runs,
after --warmup) and the polynomial-transform counts of the two routes.  The composition's slices, its per-call constant tables and the
stream wait of every fhe_ckks_lincomb are part of what a caller of the small entries pays, so they are inside its time.

    python tools/ckks_poly_lab.py [--log-n 13 15] [--batch 1 8 64] [--degree 31] [--samples 7] [--warmup 2]"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[13, 15])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--degree", type=int, default=31)
    ap.add_argument("--limbs", type=int, default=12)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import learn_fhe_amd as F
    from oracle import pyref as P
    poly = F.ckks_poly
    coeffs = np.random.Generator(np.random.PCG64(1)).uniform(-1, 1, args.degree + 1)
    plan = F.CkksPolyPlan(coeffs, 0)
    ops = plan.ops
    fused_t, comp_t = poly.transform_counts(ops)
    print("degree %d: depth %d, %d ops (%d MUL), %d registers; polynomial transforms per limb and ciphertext (key switches apart): fused %d, "
          "composition %d" % (args.degree, plan.depth, len(ops), sum(o["kind"] == poly.MUL for o in ops), plan.n_regs, fused_t, comp_t))
    big_l = args.limbs
    for log_n in args.log_n:
        n = 1 << log_n
        qs, ps = P.ckks_primes(log_n, 55, big_l)
        ctx = {lv: F.RnsContext(qs[:lv], ps) for lv in range(big_l - plan.depth, big_l + 1)}
        like = torch.zeros(1, dtype=torch.int64, device="cuda")
        sk = F.sample_zo(0.5, 5, 0, like, n)
        rlk = ctx[big_l].ksk_gen(sk, None, n, 6, 0)
        keys = {lv: F.CkksKey(ctx[lv], *(torch.cat([k[:lv], k[big_l:]]).contiguous() for k in rlk), n) for lv in ctx}
        ev = F.CkksPolyEval(plan, [ctx[lv] for lv in range(big_l, big_l - plan.depth - 1, -1)], qs[-1], rlk[0], rlk[1], n)
        for batch in args.batch:
            rng = np.random.Generator(np.random.PCG64(batch))
            halves = []
            for _ in range(2):
                a = rng.integers(0, 1 << 62, (batch, big_l, n), dtype=np.uint64)
                for l, q in enumerate(qs):
                    a[:, l] %= np.uint64(q)
                halves.append(torch.from_numpy(a.view(np.int64)).cuda())
            cb, ca = halves

            def timed(fn):
                out = []
                for i in range(args.warmup + args.samples):
                    torch.cuda.synchronize()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    res = fn()
                    t1.record()
                    torch.cuda.synchronize()
                    if i >= args.warmup:
                        out.append(t0.elapsed_time(t1))
                return statistics.median(out), res

            tf, (gb, ga) = timed(lambda: ev.apply(cb, ca))
            tc, (wb, wa) = timed(lambda: poly.replay_composed(ops, lambda lv: ctx[lv], lambda lv: keys[lv], cb, ca, n, qs[-1]))
            same = torch.equal(gb, wb) and torch.equal(ga, wa)
            print("n=2^%d L=%d batch=%d: fhe_ckks_poly_apply %.3f ms, composition %.3f ms, same bits: %s" % (log_n, big_l, batch, tf, tc, same), flush=True)
            del cb, ca, gb, ga, wb, wa, halves
            torch.cuda.empty_cache()
            F.lib().fhe_trim()


if __name__ == "__main__":
    main()
