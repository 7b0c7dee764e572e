#!/usr/bin/env python3
"""Developer lab: the hoisted CKKS entries against the ones that keep the reference's bits, at cfg4's base -- N = 2^15, the 8 + 8
primes of tests/golden/moduli.json.  On the same commit and the same operands it times
  fhe_ckks_mul_mat against fhe_ckks_mul_mat_hoisted for a 4 x 4 and a 4 giant x 8 baby split, at batch 1 and 8,
  R = 8 calls of fhe_ckks_rotate against one fhe_ckks_rotate_many, at batch 1 and 8,
with device events around whole calls, in interleaved rounds (one call of each side per round), and reports the median with
min ... max.  Before any timing the hoisted outputs are compared bit for bit with their compositions from public entries
(learn-fhe_amd/ckks_hoist.py) at batch 1: the two sides of a row are different roundings of the same plaintext and are not expected
to agree bit for bit with each other.  `--log-n`, `--limbs` and `--rounds` shrink it for a rehearsal.

    python tools/ckks_hoist_lab.py [--rounds 9] [--out profiles/ckks_hoist_lab.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import learn_fhe_amd as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=15)
ap.add_argument("--limbs", type=int, default=8)
ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda", 0)
with open(os.path.join(ROOT, "tests", "golden", "moduli.json")) as f:
    gold = json.load(f)
n, big_l = 1 << args.log_n, args.limbs
qs, ps = gold["cfg4_qs"][:big_l], gold["cfg4_ps"][:big_l]
big_k = len(ps)
hi, lo = F.RnsContext(qs, ps), F.RnsContext(qs[:-1], ps)
gen = torch.Generator(device=dev)
gen.manual_seed(5)
limbs = lambda ms, *lead: torch.stack([torch.randint(0, m, (*lead, n), dtype=torch.int64, device=dev, generator=gen) for m in ms], dim=len(lead)).contiguous()  # noqa: E731
cut = lambda t: torch.cat([t[:big_l - 1], t[big_l:]]).contiguous()  # noqa: E731  (the key without limb L-1)
host = lambda t: t.cpu().numpy().view("uint64")  # noqa: E731
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3  # us


def rounds(f_ref, f_new):
    f_ref(); f_new()  # warm-up of both sides at this shape
    torch.cuda.synchronize()
    tr, tn = [], []
    for _ in range(args.rounds):  # interleaved
        tr.append(timed(f_ref))
        tn.append(timed(f_new))
    fmt = lambda v: "%9.0f (%.0f ... %.0f)" % (sorted(v)[len(v) // 2], min(v), max(v))  # noqa: E731
    return fmt(tr), fmt(tn), sorted(tn)[len(tn) // 2] / sorted(tr)[len(tr) // 2]


say("ckks_hoist_lab: %s, N = 2^%d, %d + %d primes; %d interleaved rounds, device events around whole calls, us: median (min ... max)"
    % (torch.cuda.get_device_name(0), args.log_n, big_l, big_k, args.rounds))
raw = {idx: (limbs(qs + ps), limbs(qs + ps)) for idx in range(1, 8)}
raw.update({i: (limbs(qs + ps), limbs(qs + ps)) for i in (8, 16, 24, 12)})
keys_hi = {j: F.CkksKey(hi, raw[j][0], raw[j][1], n) for j in range(1, 8)}
for nb in (4, 8):
    baby, giant = list(range(nb)), [i * nb for i in range(4)]
    split = {i: list(baby) for i in giant}
    keys_lo = {i: F.CkksKey(lo, cut(raw[i][0]), cut(raw[i][1]), n) for i in giant if i}
    terms, ng = len(baby) * len(giant), len(giant)
    diags = limbs(qs + ps, terms)
    mat = F.CkksDiagMatrix(hi, lo, n, split, diags[:, :big_l].contiguous(), keys_hi, keys_lo)
    hoisted = F.CkksDiagMatrixHoisted(hi, lo, n, split, diags, keys_hi, keys_lo)
    cb, ca = limbs(qs, 1), limbs(qs, 1)
    got = hoisted.apply(cb, ca)
    want = F.ckks_hoist.mul_mat_hoisted_composed(hi, lo, n, split, host(diags), {j: (host(raw[j][0]), host(raw[j][1])) for j in baby if j}, keys_lo, cb, ca)
    torch.cuda.synchronize()
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]), "hoisted != its composition from public entries"
    # transforms outside the giant steps' key switches: fused 2 L n_b + 2 (L - 1) n_g + 2 T of its own + (n_b - 1) baby key switches of
    # L + K forward and 2 (L + K) inverse; hoisted 2 L + K forward and 2 (L + K) n_g inverse
    t_fused = 2 * big_l * nb + 2 * (big_l - 1) * ng + 2 * terms + (nb - 1) * 3 * (big_l + big_k)
    t_hoist = 2 * big_l + big_k + 2 * (big_l + big_k) * ng
    for batch in args.batches:
        cb, ca = limbs(qs, batch), limbs(qs, batch)
        ref, new, ratio = rounds(lambda: mat.apply(cb, ca), lambda: hoisted.apply(cb, ca))
        say("mul_mat %d giant x %d baby  batch %d  transforms %3d / %3d   fhe_ckks_mul_mat %s   hoisted %s   hoisted / mul_mat %.2f%s"
            % (ng, nb, batch, t_fused, t_hoist, ref, new, ratio, "   SLOWER" if ratio > 1 else ""))
    del mat, hoisted, diags
amounts = list(range(1, 8)) + [9]
raw[9] = (limbs(qs + ps), limbs(qs + ps))
keys_hi[9] = F.CkksKey(hi, raw[9][0], raw[9][1], n)
keys = [keys_hi[j] for j in amounts]
cb, ca = limbs(qs, 1), limbs(qs, 1)
got = F.CkksKey.rotate_many(hi, n, amounts[:2], keys[:2], cb, ca)
want = F.ckks_hoist.rotate_many_composed(hi, n, amounts[:2], [(host(raw[j][0]), host(raw[j][1])) for j in amounts[:2]], cb, ca)
torch.cuda.synchronize()
assert all(torch.equal(g[0], w[0]) and torch.equal(g[1], w[1]) for g, w in zip(got, want)), "rotate_many != its composition from public entries"
for batch in args.batches:
    cb, ca = limbs(qs, batch), limbs(qs, batch)
    outs = [(torch.empty_like(cb), torch.empty_like(ca)) for _ in amounts]

    def eight_rotates():
        for j, key, (ob, oa) in zip(amounts, keys, outs):  # fhe_ckks_rotate works in place: the copies are part of using it this way
            ob.copy_(cb)
            oa.copy_(ca)
            key.rotate_(pow(5, j, 2 * n), ob, oa)

    ref, new, ratio = rounds(eight_rotates, lambda: F.CkksKey.rotate_many(hi, n, amounts, keys, cb, ca, outs=outs))
    say("rotate x %d                batch %d                         8 fhe_ckks_rotate %s   rotate_many %s   rotate_many / rotate %.2f%s"
        % (len(amounts), batch, ref, new, ratio, "   SLOWER" if ratio > 1 else ""))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
