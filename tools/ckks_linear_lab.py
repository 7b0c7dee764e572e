#!/usr/bin/env python3
"""Times the CKKS linear transforms (include/fhe_ring.h fhe_ckks_linear_*) at the cfg4 ring: plan creation, prepare and apply of
slot_to_coeff / coeff_to_slot at n = 2^15, r = 3 (log_qi = 55, L = 8), next to the same matrices applied as a hand-made chain of
fhe_ckks_mul_mat (CkksDiagMatrix built from the read-back diagonals) in the same run.  Apply IS that chain's kernels: the two
figures differ by the Python between the calls.  Prints one JSON line per direction.

    python tools/ckks_linear_lab.py [--log-n 15] [--r 3] [--limbs 8] [--batch 1] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=15)
    ap.add_argument("--r", type=int, default=3)
    ap.add_argument("--limbs", type=int, default=8)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import learn_fhe_amd as fhe
    from oracle import pyref as P

    n, L = 1 << a.log_n, a.limbs
    qs, ps = P.ckks_primes(a.log_n, 55, L)
    scale = qs[-1]
    ctx = {lv: fhe.RnsContext(qs[:lv], ps) for lv in range(1, L + 1)}
    enc = fhe.CkksEncoder(n)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    sk = fhe.sample_zo(0.5, 1, 0, dev(np.zeros(1, dtype=np.int64)), n)

    def timed(f, reps=1):
        out, ts = None, []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return out, float(np.median(ts))

    def cut(key, lv):
        return key if lv == L else torch.cat([key[:lv], key[L:]]).contiguous()

    for inverse in (False, True):
        plan, t_plan = timed(lambda: fhe.CkksLinearPlan(enc, a.r, inverse))
        if plan.depth + 1 > L:
            raise SystemExit("depth %d needs more than %d limbs" % (plan.depth, L))
        keys, t_keys = timed(lambda: {j: fhe.rtk_gen(ctx[L], sk, n, j, 2, j) for j in plan.rotations})
        levels = [ctx[lv] for lv in range(L, L - plan.depth - 1, -1)]
        tr, t_prep = timed(lambda: fhe.CkksLinearTransform(plan, levels, scale, keys))
        rng = np.random.Generator(np.random.PCG64(3))
        cb, ca = (dev(np.stack([rng.integers(0, q, (a.batch, n), dtype=np.uint64) for q in qs], axis=1).view(np.int64)) for _ in range(2))
        tr.apply(cb, ca)  # warm-up: first launches, LDS limits, the pool
        got, t_apply = timed(lambda: tr.apply(cb, ca), a.reps)
        # the same matrices by hand
        chain, lv = [], L
        for k in reversed(range(plan.depth)):
            idx, _, split = plan.matrix(k)
            vals = plan.diags(k)
            terms = [(i, j) for i in sorted(split) for j in sorted(split[i])]
            rot = np.stack([np.roll(vals[idx.index(i + j)], i, axis=0) for i, j in terms])
            pts = enc.encode(ctx[lv], scale, dev(rot[..., 0] + 1j * rot[..., 2]), dev(rot[..., 1] + 1j * rot[..., 3]))
            mk = lambda c, x, at: fhe.CkksKey(c, cut(keys[x][0], at), cut(keys[x][1], at), n)  # noqa: E731
            chain.append(fhe.CkksDiagMatrix(ctx[lv], ctx[lv - 1], n, split, pts, {j: mk(ctx[lv], j, lv) for js in split.values() for j in js if j},
                                            {i: mk(ctx[lv - 1], i, lv - 1) for i in split if i}))
            lv -= 1

        def by_hand():
            b, c = cb, ca
            for m in chain:
                b, c = m.apply(b, c)
            return b, c

        by_hand()
        want, t_chain = timed(by_hand, a.reps)
        same = bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))
        print(json.dumps({"direction": "coeff_to_slot" if inverse else "slot_to_coeff", "log_n": a.log_n, "r": a.r, "L": L, "batch": a.batch,
                          "depth": plan.depth, "diagonals": [len(plan.matrix(k)[0]) for k in range(plan.depth)], "rotation_keys": len(plan.rotations),
                          "plan_create_ms": round(t_plan, 3), "rtk_gen_all_ms": round(t_keys, 3), "prepare_ms": round(t_prep, 3),
                          "apply_ms": round(t_apply, 3), "mul_mat_chain_ms": round(t_chain, 3), "bit_identical": same}))
        del tr, chain, keys
        if not same:
            raise SystemExit("apply differs from the chain")


if __name__ == "__main__":
    main()
