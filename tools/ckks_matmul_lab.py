#!/usr/bin/env python3
"""Developer lab: the CKKS diagonal-matrix product (`Bootstrapping::mul_mat`) at cfg4's base -- N = 2^15, the 8 + 8 primes of
tests/golden/moduli.json -- with a 4 x 4 baby-step / giant-step split (16 terms), batch 1 and 8.  Times, on the same operands,
  composed: CkksKey.rotate_ / RnsContext.mul_plain / RnsContext.add_ in the reference's order (bootstrapping.rs:95-107),
  fused:    CkksDiagMatrix.apply (fhe_ckks_mul_mat),
with device events after a warm-up, the two paths alternating; checks that both give the same bits before it prints one JSON line
per batch with both times and the transforms each path runs (key switches apart: both run the same ones).
`--log-n`, `--limbs`, `--k` and `--reps` shrink it for a rehearsal."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
import learn_fhe_amd as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=15)
ap.add_argument("--limbs", type=int, default=8)
ap.add_argument("--k", type=int, default=4, help="baby steps 0..k-1, giant steps 0, k, .., (k-1) k")
ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda", 0)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "moduli.json")) as f:
    gold = json.load(f)
n, big_l, k = 1 << args.log_n, args.limbs, args.k
qs, ps = gold["cfg4_qs"][:big_l], gold["cfg4_ps"][:big_l]
hi, lo = F.RnsContext(qs, ps), F.RnsContext(qs[:-1], ps)
gen = torch.Generator(device=dev)
gen.manual_seed(5)
limbs = lambda ms, *lead: torch.stack([torch.randint(0, m, (*lead, n), dtype=torch.int64, device=dev, generator=gen) for m in ms], dim=len(lead)).contiguous()  # noqa: E731
baby, giant = list(range(k)), [i * k for i in range(k)]
split = {i: list(baby) for i in giant}
raw = {idx: (limbs(qs + ps), limbs(qs + ps)) for idx in sorted(set(baby + giant) - {0})}
cut = lambda t: torch.cat([t[:big_l - 1], t[big_l:]]).contiguous()  # noqa: E731  (the key without limb L-1)
keys_hi = {j: F.CkksKey(hi, raw[j][0], raw[j][1], n) for j in baby if j}
keys_lo = {i: F.CkksKey(lo, cut(raw[i][0]), cut(raw[i][1]), n) for i in giant if i}
terms = len(baby) * len(giant)
diags = limbs(qs, terms)
mat = F.CkksDiagMatrix(hi, lo, n, split, diags, keys_hi, keys_lo)


def composed(cb, ca):
    total, t = None, 0
    rot = {}
    for j in baby:
        b, a = cb.clone(), ca.clone()
        if j:
            keys_hi[j].rotate_(pow(5, j, 2 * n), b, a)
        rot[j] = (b, a)
    for i in giant:
        s = None
        for j in baby:
            p = hi.mul_plain(diags[t:t + 1], rot[j][0], rot[j][1], n)
            t += 1
            s = p if s is None else (lo.add_(s[0], p[0], n), lo.add_(s[1], p[1], n))
        if i:
            keys_lo[i].rotate_(pow(5, i, 2 * n), s[0], s[1])
        total = s if total is None else (lo.add_(total[0], s[0], n), lo.add_(total[1], s[1], n))
    return total


def timed(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(*a)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3  # us


nb, ng = len(baby), len(giant)
for batch in args.batches:
    cb, ca = limbs(qs, batch), limbs(qs, batch)
    want, got = composed(cb, ca), mat.apply(cb, ca)  # warm-up of both paths at this shape, and the parity check
    torch.cuda.synchronize()
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]), "fused != composed"
    tc, tf = [], []
    for _ in range(args.reps):  # alternating
        tc.append(timed(composed, cb, ca))
        tf.append(timed(mat.apply, cb, ca))
    print(json.dumps({
        "log_n": args.log_n, "L": big_l, "terms": terms, "batch": batch, "reps": args.reps,
        "composed_us_median": sorted(tc)[len(tc) // 2], "composed_us_min": min(tc),
        "fused_us_median": sorted(tf)[len(tf) // 2], "fused_us_min": min(tf),
        # per ciphertext, outside the key switches: mul_plain = L (plaintext) + 2 L forward + 2 L inverse per term
        "composed_transforms": 5 * big_l * terms,
        # fused: 2 L forward per baby slot, 2 (L - 1) inverse per giant step, 2 inverse per term (the diagonals' L per term are paid once, at prepare)
        "fused_transforms": 2 * big_l * nb + 2 * (big_l - 1) * ng + 2 * terms,
    }), flush=True)
