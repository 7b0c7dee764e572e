"""Lab of the TGLWE ciphertext product: first every route bit for bit (fused fhe_tglwe_mul, fhe_tglwe_tensor + fhe_tglwe_relin
chained, the external-product relinearisation), then times in interleaved rounds -- every round runs each route once, in turn, so that
clock and temperature drift fall on all alike.  A route's window is `reps` calls between two events, with reps calibrated so that the
window lasts about --window seconds; its figure is the median over the rounds of window / reps.

Routes, per batch:
  fused, chained   fhe_tglwe_mul against fhe_tglwe_tensor + fhe_tglwe_relin on TGLWE operands (a schedule comparison)
  lwe_mul          TLWE x TLWE through the product: two packs of one input, fhe_tglwe_mul, sample_extract(0)
  bootstrap        the product route the library had before: tfhe_circuit.bivariate's table through fhe_tfhe_bootstrap_tables on 4 x + y,
                   under cfg5's key (bench.tfhe_setup: N = 1024, n_lwe = 630, gadget (7, 3), key switch (4, 5), uniform-random key words --
                   the work of a bootstrap does not depend on their values)
and once: dot of n entries against n such bootstraps in one call plus the additions of their outputs.
lwe_mul and dot take TLWE inputs of the same n_in = 630 words; their outputs are TLWE ciphertexts under the TGLWE key's n bits, those
of the bootstrap route are switched back to 630.

    python tools/tfhe_mul_lab.py [--p 56] [--log-b 7] [--d 5] [--batches 1,16,64,1024] [--rounds 5] [--window 1.0] [--out profiles/tfhe_mul_lab.txt]
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
    ap.add_argument("--log-b", type=int, default=7)
    ap.add_argument("--d", type=int, default=5)
    ap.add_argument("--p", type=int, default=56)
    ap.add_argument("--batches", default="1,16,64,1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tfhe_mul_lab.txt"))
    a = ap.parse_args()
    import torch
    import bench
    import learn_fhe_amd as F
    from learn_fhe_amd import tfhe_circuit as T
    X = F.tfhe_mul
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    batches = [int(b) for b in a.batches.split(",")]
    S = bench.tfhe_setup(torch, F, dev, 0, max(batches))  # cfg5's bootstrapping and key-switching keys
    n, n_in, log_b, d, p = S["n"], S["n_lwe"], a.log_b, a.d, a.p
    t = S["t"]
    like = torch.zeros(1, dtype=torch.int64, device=dev)
    s = F.sample_binary(77, 1, like, n)
    rlk = X.rlk_gen(t, log_b, d, s, n, 2.0 ** -55, 78, 0)
    key = X.RelinKey(t, log_b, d, rlk[0], rlk[1], n)
    pf = (8, 7)
    z = F.sample_binary(77, 2, like, n_in)
    pfksk = F.tfhe_cbs.pfksk_gen(t, pf[0], pf[1], z, s, F.pack_funcs(n, like), 2.0 ** -55, 79, 0)
    pk = F.PackKey(t, pf[0], pf[1], pfksk, n_in, n)
    # the bivariate product table of two 2-bit messages over Z_16 with a padding bit, as tfhe_circuit.bivariate builds it
    bld, _, _, wire = T.bivariate(lambda u, v: u * v, 2)
    cc = bld.compile([wire], 4, 1, n)
    tables = torch.from_numpy(cc.tables.view("int64")).to(dev)
    say("tfhe_mul_lab: %s, n = %d, relinearisation gadget (%d, %d), p = %d, packing gadget (%d, %d), n_in = %d; %d interleaved rounds, windows of about %.1f s"
        % (torch.cuda.get_device_name(0), n, log_b, d, p, pf[0], pf[1], n_in, a.rounds, a.window))

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
    rows = []
    for batch in batches:
        ops = [rnd(batch, n) for _ in range(4)]
        fa, fb = X.mul(key, *ops, p)
        ca, cb = X.relin(key, *X.tensor(t, *ops, n, p))
        assert torch.equal(fa, ca) and torch.equal(fb, cb), "fused != chained"
        if batch <= 16:
            xa, xb = X.relin_composed(t, log_b, d, rlk[0], rlk[1], *X.tensor(t, *ops, n, p), n)
            assert torch.equal(fa, xa) and torch.equal(fb, xb), "fused != external-product route"
        out = (torch.empty_like(ops[0]), torch.empty_like(ops[0]))
        c = [torch.empty_like(ops[0]) for _ in range(3)]
        cx, cy = (rnd(batch, n_in), rnd(batch)), (rnd(batch, n_in), rnd(batch))  # TLWE words: the work does not depend on their values
        table_of = torch.zeros(batch, dtype=torch.int32, device=dev)

        def fused():
            lib.fhe_tglwe_mul(t.handle, key._h, H(ops[0]), H(ops[1]), H(ops[2]), H(ops[3]), p, H(out[0]), H(out[1]), batch, 1, st)

        def chained():
            lib.fhe_tglwe_tensor(t.handle, H(ops[0]), H(ops[1]), H(ops[2]), H(ops[3]), n, p, H(c[0]), H(c[1]), H(c[2]), batch, 1, st)
            lib.fhe_tglwe_relin(t.handle, key._h, H(c[0]), H(c[1]), H(c[2]), H(out[0]), H(out[1]), batch, 1, st)

        def lwe_mul():
            return X.lwe_mul(pk, key, cx, cy, p)

        def bootstrap():
            return S["key"].bootstrap_tables(S["ks_lb"], S["ks_d"], S["ksa"], S["ksb"], tables, table_of, 4 * cx[0] + cy[0], 4 * cx[1] + cy[1])

        r = timed({"fused": fused, "chained": chained, "lwe_mul": lwe_mul, "bootstrap": bootstrap})
        rows.append((batch, r))
    say("")
    say("product of `batch` TGLWE pairs: fused = fhe_tglwe_mul, chained = fhe_tglwe_tensor + fhe_tglwe_relin (median us a call; min .. max; reps a window)")
    say("%6s %30s %30s %14s %18s" % ("batch", "fused", "chained", "chained/fused", "fused products/s"))
    cell = lambda v: "%.1f (%.1f .. %.1f; %d)" % v  # noqa: E731
    for batch, r in rows:
        say("%6d %30s %30s %14.3f %18.0f" % (batch, cell(r["fused"]), cell(r["chained"]), r["chained"][0] / r["fused"][0], batch * 1e6 / r["fused"][0]))
    say("")
    say("product of `batch` TLWE pairs: lwe_mul (pack, multiply, extract) against the bivariate bootstrap under cfg5's key (median us a call; min .. max; reps a window)")
    say("%6s %34s %34s %18s %16s %18s" % ("batch", "lwe_mul", "bootstrap", "bootstrap/lwe_mul", "lwe_mul prod/s", "bootstrap prod/s"))
    for batch, r in rows:
        say("%6d %34s %34s %18.2f %16.0f %18.0f" % (batch, cell(r["lwe_mul"]), cell(r["bootstrap"]), r["bootstrap"][0] / r["lwe_mul"][0],
                                                    batch * 1e6 / r["lwe_mul"][0], batch * 1e6 / r["bootstrap"][0]))

    # the inner product of n entries: one dot against n bivariate bootstraps in one call and the sum of their outputs
    cx, cy = (rnd(n, n_in), rnd(n)), (rnd(n, n_in), rnd(n))
    table_of = torch.zeros(n, dtype=torch.int32, device=dev)

    def dot():
        return X.dot(pk, key, cx, cy, p)

    def bootstraps_and_sum():
        oa, ob = S["key"].bootstrap_tables(S["ks_lb"], S["ks_d"], S["ksa"], S["ksb"], tables, table_of, 4 * cx[0] + cy[0], 4 * cx[1] + cy[1])
        return oa.sum(dim=0), ob.sum()

    r = timed({"dot": dot, "bootstraps_and_sum": bootstraps_and_sum})
    say("")
    say("inner product of %d entries: dot %s us, %d bootstraps + additions %s us, ratio %.1f" % (n, cell(r["dot"]), n, cell(r["bootstraps_and_sum"]),
                                                                                                r["bootstraps_and_sum"][0] / r["dot"][0]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
