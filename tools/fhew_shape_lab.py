#!/usr/bin/env python3
"""Developer lab: FHEW blind rotations/s by launch shape.

  fhew_shape_lab.py [batch ...]          cfg3 at several batch sizes; run once per shape with FHE_RING_SMALL_BATCH=0 (throughput
                                         shape everywhere) and FHE_RING_SMALL_BATCH=1000000 (latency shape everywhere)
  fhew_shape_lab.py --split [N ...]      workgroups per ciphertext G = 1, 2, 4, 8 (set_option("BR_SPLIT", G); 1 = one workgroup)
                                         x batch 1 .. 128 at cfg3's parameters on ring size N (default 1024 and 2048): the table
                                         above split_g() in learn-fhe_amd/csrc/fhew_api.hip.  Interleaved rounds in one process,
                                         median of the rounds; a cell the call does not admit (batch x G > compute units) is "-".
                                         A library status other than FHE_OK (a timeout word) ends the run.
"""
import os, sys, json, statistics, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
import learn_fhe_amd as F
dev = torch.device("cuda:0")


def setup(n):
    q, log_b, d, w, n_lwe = 18014398509404161, 6, 9, 10, 100
    ctx = F.NttContext(q, device=0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    rnd = lambda *shape: torch.randint(0, q, shape, dtype=torch.int64, device=dev, generator=gen)  # noqa: E731
    brk = F.GadgetKey(ctx, log_b, d, rnd(n_lwe, 2 * d, n), rnd(n_lwe, 2 * d, n), n, rgsw=True)
    ak = F.GadgetKey(ctx, log_b, d, rnd(w + 1, d, n), rnd(w + 1, d, n), n, rgsw=False)
    return dict(n=n, n_lwe=n_lwe, gen=gen, bk=F.BootstrapKey(ctx, brk, ak, F.ak_t(n, w), w), f=rnd(n), keep=(ctx, brk, ak))


def split_sweep(sizes, rounds=5):
    for n in sizes:
        S = setup(n)
        bk = S["bk"]
        table = {}
        for batch in (1, 2, 4, 8, 16, 32, 64, 128):
            lwe_a = torch.randint(0, n, (batch, S["n_lwe"]), dtype=torch.int64, device=dev, generator=S["gen"]) * 2 + 1
            lwe_b = torch.randint(0, 2 * n, (batch,), dtype=torch.int64, device=dev, generator=S["gen"])
            times = {1: [], 2: [], 4: [], 8: []}
            for r in range(rounds + 1):  # round 0 warms up
                for g in times:
                    F.set_option("BR_SPLIT", 0 if g == 1 else g)
                    if bk.split(batch) != g:
                        continue
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    bk.blind_rotate(lwe_a, lwe_b, S["f"])
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    bk.check(lwe_a)  # raises on a timeout word: the run ends here
                    if r:
                        times[g].append(dt)
            table[batch] = {g: (round(batch / statistics.median(t)) if t else None) for g, t in times.items()}
            print("N=%d batch %4d  " % (n, batch) + "  ".join("G=%d %8s/s (%7s us)" % (g, v if v else "-", round(1e6 * batch / v) if v else "-")
                                                               for g, v in table[batch].items()), flush=True)
        F.set_option("BR_SPLIT", -1)
        print("SPLIT_TABLE", json.dumps({"n": n, "blind_rotations_per_sec": table}), flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "--split":
    split_sweep([int(a) for a in sys.argv[2:]] or [1024, 2048])
    sys.exit(0)

S = bench.fhew_setup(torch, F, dev, 0)
out = {}
for batch in [int(a) for a in sys.argv[1:]] or [768, 1024, 1536, 2048, 3072, 4096]:
    lwe_a = torch.randint(0, S["n"], (batch, S["n_lwe"]), dtype=torch.int64, device=dev, generator=S["gen"]) * 2 + 1
    lwe_b = torch.randint(0, 2 * S["n"], (batch,), dtype=torch.int64, device=dev, generator=S["gen"])
    dt = bench._timeit(torch, lambda: S["bk"].blind_rotate(lwe_a, lwe_b, S["f"]), 3)
    out[batch] = round(batch / dt)
print(os.environ.get("FHE_RING_SMALL_BATCH", "default"), json.dumps(out))
