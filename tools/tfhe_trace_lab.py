"""Lab of the TGLWE automorphism key switch, trace and ring packing: first the routes bit for bit (the fused trace against
its composition, the ring pack against its composition), then times in interleaved rounds -- every round runs each route once, in turn,
so that clock and temperature drift fall on all alike.  A route's window is `reps` calls between two events, with reps calibrated so
that the window lasts about --window seconds; its figure is the median over the rounds of window / reps, with min and max.

  (a) fhe_tglwe_automorphism beside fhe_tglwe_relin: the same key-switch work, the difference is the permutation
  (b) fhe_tglwe_trace (one launch) beside trace_composed (fhe_tglwe_automorphism + an addition per step): a schedule comparison
  (c) fhe_tlwe_ring_pack beside fhe_tlwe_pack under a fhe_tlwe_pfksk_gen key with n_in = n and the same gadget, with the device bytes
      of both prepared keys

    python tools/tfhe_trace_lab.py [--n 1024] [--log-b 7] [--d 5] [--batches 1,16,64,1024] [--counts 1,16,1024] [--packs 1,16]
                                   [--rounds 5] [--window 1.0] [--out profiles/tfhe_trace_lab.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--log-b", type=int, default=7)
    ap.add_argument("--d", type=int, default=5)
    ap.add_argument("--batches", default="1,16,64,1024")
    ap.add_argument("--counts", default="1,16,1024")
    ap.add_argument("--packs", default="1,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tfhe_trace_lab.txt"))
    a = ap.parse_args()
    import torch
    import learn_fhe_amd as F
    X, XM = F.tfhe_trace, F.tfhe_mul
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    dev = torch.device("cuda:0")
    n, log_b, d = a.n, a.log_b, a.d
    log_n = n.bit_length() - 1
    t = F.TorusContext()
    like = torch.zeros(1, dtype=torch.int64, device=dev)
    s = F.sample_binary(77, 1, like, n)
    gs = X.galois_set(n)
    atk = X.atk_gen(t, log_b, d, s, n, gs, 2.0 ** -55, 78, 0)
    key = X.AutoKey(t, log_b, d, atk[0], atk[1], n, gs)
    rlk = XM.rlk_gen(t, log_b, d, s, n, 2.0 ** -55, 79, 0)
    rkey = XM.RelinKey(t, log_b, d, rlk[0], rlk[1], n)
    pfksk = F.tfhe_cbs.pfksk_gen(t, log_b, d, s, s, F.pack_funcs(n, like), 2.0 ** -55, 80, 0)
    pk = F.PackKey(t, log_b, d, pfksk, n, n)
    pack_rows, pack_bytes = d * (n + 1), 3 * d * (n + 1) * 2 * n * 8  # the rows as they came and the two primes' planes
    say("tfhe_trace_lab: %s, n = %d, gadget (%d, %d); %d interleaved rounds, windows of about %.1f s" % (torch.cuda.get_device_name(0), n, log_b, d, a.rounds, a.window))
    say("prepared keys on the device: automorphism set %d rows, %d bytes; packing key (n_in = n) %d rows, %d bytes; ratio %.1f in rows, %.1f in bytes"
        % (len(gs) * d, key.device_bytes(), pack_rows, pack_bytes, pack_rows / (len(gs) * d), pack_bytes / key.device_bytes()))

    def window(f, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / 1000.0

    def timed(routes):
        """routes: name -> callable; -> name -> (median, min, max microseconds per call, reps)"""
        reps = {}
        for k, f in routes.items():
            window(f, 3)  # warm-up
            per = window(f, 5) / 5
            reps[k] = max(3, int(a.window / per))
        samples = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, f in routes.items():
                samples[k].append(window(f, reps[k]) * 1e6 / reps[k])
        return {k: (statistics.median(v), min(v), max(v), reps[k]) for k, v in samples.items()}

    lib, H = F.lib(), lambda x: x.data_ptr()  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.Generator(np.random.PCG64(5))
    rnd = lambda *shape: torch.from_numpy(rng.integers(-(1 << 63), 1 << 63, size=shape, dtype=np.int64)).to(dev)  # noqa: E731
    cell = lambda v: "%.1f (%.1f .. %.1f; %d)" % v  # noqa: E731
    rows = []
    for batch in [int(b) for b in a.batches.split(",")]:
        ca, cb, c2 = rnd(batch, n), rnd(batch, n), rnd(batch, n)
        fa, fb = X.trace(key, ca, cb)
        xa, xb = X.trace_composed(key, ca, cb)
        assert torch.equal(fa, xa) and torch.equal(fb, xb), "fused trace != composed"
        out = (torch.empty_like(ca), torch.empty_like(ca))

        def auto():
            lib.fhe_tglwe_automorphism(t.handle, key._h, 3, H(ca), H(cb), H(out[0]), H(out[1]), batch, 1, st)

        def relin():
            lib.fhe_tglwe_relin(t.handle, rkey._h, H(cb), H(ca), H(c2), H(out[0]), H(out[1]), batch, 1, st)

        def fused():
            lib.fhe_tglwe_trace(t.handle, key._h, 0, log_n, H(ca), H(cb), H(out[0]), H(out[1]), batch, 1, st)

        def composed():
            return X.trace_composed(key, ca, cb)

        rows.append((batch, timed({"auto": auto, "relin": relin, "fused": fused, "composed": composed})))
    say("")
    say("(a) one key switch of `batch` ciphertexts: fhe_tglwe_automorphism (g = 3) beside fhe_tglwe_relin (median us a call; min .. max; reps a window)")
    say("%6s %30s %30s %12s" % ("batch", "automorphism", "relin", "auto/relin"))
    for batch, r in rows:
        say("%6d %30s %30s %12.3f" % (batch, cell(r["auto"]), cell(r["relin"]), r["auto"][0] / r["relin"][0]))
    say("")
    say("(b) full trace (%d steps) of `batch` ciphertexts: fhe_tglwe_trace beside trace_composed" % log_n)
    say("%6s %32s %32s %16s" % ("batch", "fused", "composed", "composed/fused"))
    for batch, r in rows:
        say("%6d %32s %32s %16.3f" % (batch, cell(r["fused"]), cell(r["composed"]), r["composed"][0] / r["fused"][0]))
    say("")
    say("(c) `packs` packs of `count` TLWE ciphertexts (n_in = n): fhe_tlwe_ring_pack beside fhe_tlwe_pack (stride n / count)")
    say("%6s %6s %34s %34s %16s" % ("count", "packs", "ring_pack", "pack", "ring_pack/pack"))
    for count in [int(c) for c in a.counts.split(",")]:
        for packs in [int(p) for p in a.packs.split(",")]:
            ta, tb = rnd(packs, count, n), rnd(packs, count)
            if count <= 16 and packs == 1:
                ga, gb = X.ring_pack(key, ta, tb, count)
                xa, xb = X.ring_pack_composed(key, ta, tb, count)
                assert torch.equal(ga, xa) and torch.equal(gb, xb), "ring_pack != composed"
            oa, ob = torch.empty(packs, n, dtype=torch.int64, device=dev), torch.empty(packs, n, dtype=torch.int64, device=dev)

            def ring():
                lib.fhe_tlwe_ring_pack(t.handle, key._h, H(ta), H(tb), count, packs, H(oa), H(ob), 1, st)

            def pack():
                lib.fhe_tlwe_pack(t.handle, pk._h, H(ta), H(tb), count, max(1, n // count), packs, H(oa), H(ob), 1, st)

            r = timed({"ring": ring, "pack": pack})
            say("%6d %6d %34s %34s %16.2f" % (count, packs, cell(r["ring"]), cell(r["pack"]), r["ring"][0] / r["pack"][0]))


if __name__ == "__main__":
    main()
