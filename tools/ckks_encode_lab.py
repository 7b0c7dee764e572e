#!/usr/bin/env python3
"""Developer lab: the CKKS encoder (fhe_ckks_encode / fhe_ckks_decode / fhe_ckks_sifft / fhe_ckks_sfft) at cfg4's ring -- N = 2^15
(l = 2^14 slots), the first 8 primes of tests/golden/moduli.json's cfg4 chain -- batch 64 and 256.  Each entry is timed with device
events on device-resident operands: after a warm-up, `--reps` samples, each one event pair around `--inner` back-to-back calls (so
that launch overhead and the event pair itself are amortised), reported per call as median, minimum and maximum (the spread), as
messages per second and as
the bytes the entry MUST move (inputs read once, outputs written once; the two-pass route's workspace and the twiddle gathers are
extra traffic and are not counted) per second against the 8 TB/s HBM roofline.  One JSON line per (entry, batch).
`--log-n`, `--limbs`, `--batches` and `--reps` shrink it for a rehearsal."""
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
ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=10, help="calls per timed event pair")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda", 0)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "moduli.json")) as f:
    gold = json.load(f)
n, big_l = 1 << args.log_n, args.limbs
l = n // 2
qs, ps = gold["cfg4_qs"][:big_l], gold["cfg4_ps"][:1]
rns, enc = F.RnsContext(qs, ps), F.CkksEncoder(n)
scale = qs[-1]
ROOF = 8e12
gen = torch.Generator(device=dev)
gen.manual_seed(9)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / args.inner  # s per call


for batch in args.batches:
    m_hi = torch.view_as_complex(torch.rand((batch, l, 2), dtype=torch.float64, device=dev, generator=gen) * 2 - 1).contiguous()
    m_lo = (m_hi * 2.0 ** -56).contiguous()
    pt = enc.encode(rns, scale, m_hi, m_lo)
    z_hi, z_lo = m_hi.clone(), m_lo.clone()
    slots, limbs = batch * l * 32, batch * big_l * n * 8
    entries = {
        "encode": (lambda: enc.encode(rns, scale, m_hi, m_lo), slots + limbs),
        "decode": (lambda: enc.decode(rns, scale, pt, want_lo=True), slots + limbs),
        "sifft": (lambda: enc.sifft(z_hi, z_lo), 2 * slots),
        "sfft": (lambda: enc.sfft(z_hi, z_lo), 2 * slots),
    }
    for name, (fn, nbytes) in entries.items():
        for _ in range(3):  # warm-up: first-use costs (LDS limit, pool growth) and clocks
            fn()
        torch.cuda.synchronize()
        ts = sorted(timed(fn) for _ in range(args.reps))
        med = ts[len(ts) // 2]
        print(json.dumps({"entry": name, "log_n": args.log_n, "L": big_l, "batch": batch, "reps": args.reps, "inner": args.inner, "ms_median": med * 1e3, "ms_min": ts[0] * 1e3, "ms_max": ts[-1] * 1e3,
                          "messages_per_s": batch / med, "bytes": nbytes, "GB_per_s": nbytes / med / 1e9, "of_8TBps_roofline": nbytes / med / ROOF}), flush=True)
    enc.status(m_hi)
