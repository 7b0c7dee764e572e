#!/usr/bin/env python3
"""Times fhe_ckks_bootstrap_apply against the seven public calls chained by hand (ckks_bootstrap.replay_composed): n = 2^13 and 2^15,
batch 1 / 8 / 64, 55-bit chain, L = depth + 2, linear plans with chunk --chunk, eval_mod K = 8, r = 3, degree 31.  Prints one line per
shape with both times (median of --samples runs, after --warmup) and whether the two gave the same bits.  The composition's clone of the
slots and the allocation of its intermediate results are inside its time, as a caller of the small entries would pay them.

    python tools/ckks_bootstrap_lab.py [--log-n 13 15] [--batch 1 8 64] [--chunk 4] [--samples 5] [--warmup 2]"""
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
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import learn_fhe_amd as F
    from oracle import pyref as P
    boot = F.ckks_bootstrap
    K, r, degree = 8, 3, 31
    for log_n in args.log_n:
        n = 1 << log_n
        enc = F.CkksEncoder(n)
        p_c2s, p_s2c = F.CkksLinearPlan(enc, args.chunk, True), F.CkksLinearPlan(enc, args.chunk, False)
        d_mod = F.eval_mod_plan(K, r, degree).depth
        depth = p_c2s.depth + d_mod + p_s2c.depth
        big_l = depth + 2
        l1, l2 = big_l - p_c2s.depth, big_l - p_c2s.depth - d_mod
        qs, ps = P.ckks_primes(log_n, 55, big_l)
        ps = ps[:4]
        scale = qs[-1]
        ctx = {lv: F.RnsContext(qs[:lv], ps) for lv in range(big_l - depth, big_l + 1)}
        like = torch.zeros(1, dtype=torch.int64, device="cuda")
        sk = F.sample_zo(0.5, 5, 0, like, n)
        cut = lambda k, lv: k if lv == big_l else torch.cat([k[:lv], k[big_l:]]).contiguous()  # noqa: E731
        rot = {j: F.rtk_gen(ctx[big_l], sk, n, j, 6, j) for j in sorted(set(p_c2s.rotations) | set(p_s2c.rotations))}
        rlk = ctx[big_l].ksk_gen(sk, None, n, 7, 0)
        cjk = boot.cjk_gen(ctx[big_l], sk, n, 8, 0)
        plan = boot.bootstrap_eval_mod_plan(K, r, degree, qs[0], scale)
        chain = lambda top, d: [ctx[lv] for lv in range(top, top - d - 1, -1)]  # noqa: E731
        c2s = F.CkksLinearTransform(p_c2s, chain(big_l, p_c2s.depth), scale, {j: rot[j] for j in p_c2s.rotations})
        ev = F.CkksPolyEval(plan, chain(l1, d_mod), scale, cut(rlk[0], l1), cut(rlk[1], l1), n)
        s2c = F.CkksLinearTransform(p_s2c, chain(l2, p_s2c.depth), scale, {j: (cut(rot[j][0], l2), cut(rot[j][1], l2)) for j in p_s2c.rotations})
        bs = F.CkksBootstrapper(chain(big_l, depth), c2s, ev, s2c, cjk[0], cjk[1], n)
        cj_key = F.CkksKey(ctx[l1], cut(cjk[0], l1), cut(cjk[1], l1), n)
        del rot, rlk
        print("n=2^%d: depth %d = %d + %d + %d, L = %d, %d p-limbs, %d rotation keys" % (log_n, depth, p_c2s.depth, d_mod, p_s2c.depth, big_l, len(ps),
                                                                                        len(set(p_c2s.rotations) | set(p_s2c.rotations))), flush=True)
        for batch in args.batch:
            rng = np.random.Generator(np.random.PCG64(batch))
            cb, ca = (torch.from_numpy((rng.integers(0, 1 << 62, (batch, 1, n), dtype=np.uint64) % np.uint64(qs[0])).view(np.int64)).cuda() for _ in range(2))

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

            tf, (gb, ga) = timed(lambda: bs.apply(cb, ca))
            tc, (wb, wa) = timed(lambda: boot.replay_composed(ctx[big_l], c2s, cj_key, ev, s2c, cb, ca, n))
            same = torch.equal(gb, wb) and torch.equal(ga, wa)
            print("n=2^%d L=%d batch=%d: fhe_ckks_bootstrap_apply %.3f ms, composition %.3f ms, same bits: %s" % (log_n, big_l, batch, tf, tc, same), flush=True)
            del cb, ca, gb, ga, wb, wa
            torch.cuda.empty_cache()
            F.lib().fhe_trim()
        del bs, c2s, ev, s2c, cj_key, cjk, ctx
        torch.cuda.empty_cache()
        F.lib().fhe_trim()


if __name__ == "__main__":
    main()
