#!/usr/bin/env python3
"""Developer lab: the composed FHEW route (fhew_composed_kernels.hpp).

  rates (default): cfg3 blind rotations/s, composed (FHEW_COMPOSED keys) against fused, both routes alternated in one process;
                   composed external products/s and blind rotations/s at N = 4096 and 8192.  Prints one JSON line.
  prof:            a few external products at N = 4096 / 8192, batches 64 and 1024, for a kernel-trace run:
                   rocprofv3 --kernel-trace --stats -d OUT -- python tools/fhew_anysize_lab.py prof
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import learn_fhe_amd as F  # noqa: E402
from oracle import cref  # noqa: E402

dev = torch.device("cuda:0")
BATCHES = (1, 64, 1024)


def keys(q, n, log_b, d, w, n_lwe, composed, seed):
    F.set_option("FHEW_COMPOSED", 1 if composed else 0)
    try:
        ctx = F.NttContext(q)
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        rnd = lambda *shape: torch.randint(0, q, shape, dtype=torch.int64, device=dev, generator=gen)  # noqa: E731
        brk = F.GadgetKey(ctx, log_b, d, rnd(n_lwe, 2 * d, n), rnd(n_lwe, 2 * d, n), n, rgsw=True)
        ak = F.GadgetKey(ctx, log_b, d, rnd(w + 1, d, n), rnd(w + 1, d, n), n, rgsw=False)
        return dict(ctx=ctx, brk=brk, ak=ak, bk=F.BootstrapKey(ctx, brk, ak, F.ak_t(n, w), w), f=rnd(n), gen=gen)
    finally:
        F.set_option("FHEW_COMPOSED", 0)


def lwe(n, n_lwe, batch, gen):
    a = torch.randint(0, n, (batch, n_lwe), dtype=torch.int64, device=dev, generator=gen) * 2 + 1
    b = torch.randint(0, 2 * n, (batch,), dtype=torch.int64, device=dev, generator=gen)
    return a, b


def rates():
    out = {}
    # cfg3: N = 1024, q = 18014398509404161, (6, 9), n_lwe = 100, w = 10 (bench.py fhew_setup's shape)
    q, n, lb, d, w, n_lwe = 18014398509404161, 1024, 6, 9, 10, 100
    K = {r: keys(q, n, lb, d, w, n_lwe, r == "composed", 3) for r in ("fused", "composed")}
    for batch in BATCHES:
        a, b = lwe(n, n_lwe, batch, K["fused"]["gen"])
        for rnd in range(2):  # alternated: fused, composed, fused, composed
            for r in ("fused", "composed"):
                bk, f = K[r]["bk"], K["fused"]["f"]
                dt = bench._timeit(torch, lambda: bk.blind_rotate(a, b, f), 2)
                out.setdefault("cfg3_%s_br_per_s_batch%d" % (r, batch), []).append(round(batch / dt, 1))
        o1, o2 = K["fused"]["bk"].blind_rotate(a, b, K["fused"]["f"]), K["composed"]["bk"].blind_rotate(a, b, K["fused"]["f"])
        assert torch.equal(o1[0], o2[0]) and torch.equal(o1[1], o2[1]), "routes differ"
    # composed route at N = 4096 and 8192: a 54-bit prime, the same key shape
    for log_n in (12, 13):
        n = 1 << log_n
        q = cref.two_adic_primes(54, log_n + 1, 1)[0]
        S = keys(q, n, lb, d, w, n_lwe, True, 4)
        for batch in BATCHES:
            ca = torch.randint(0, q, (batch, n), dtype=torch.int64, device=dev, generator=S["gen"])
            cb = torch.randint(0, q, (batch, n), dtype=torch.int64, device=dev, generator=S["gen"])
            dt = bench._timeit(torch, lambda: S["brk"].external_product_(0, ca, cb), 5)
            out["n%d_external_products_per_s_batch%d" % (n, batch)] = round(batch / dt, 1)
            a, b = lwe(n, n_lwe, batch, S["gen"])
            dt = bench._timeit(torch, lambda: S["bk"].blind_rotate(a, b, S["f"]), 1)
            out["n%d_br_per_s_batch%d" % (n, batch)] = round(batch / dt, 2)
            S["bk"].check(a)
    print(json.dumps(out))


def prof():
    lb, d = 6, 9
    for log_n in (12, 13):
        n = 1 << log_n
        q = cref.two_adic_primes(54, log_n + 1, 1)[0]
        S = keys(q, n, lb, d, 1, 1, True, 5)
        for batch in (64, 1024):
            ca = torch.randint(0, q, (batch, n), dtype=torch.int64, device=dev, generator=S["gen"])
            cb = torch.randint(0, q, (batch, n), dtype=torch.int64, device=dev, generator=S["gen"])
            for _ in range(3):
                S["brk"].external_product_(0, ca, cb)
            torch.cuda.synchronize()
    print("prof ok")


if __name__ == "__main__":
    prof() if sys.argv[1:] == ["prof"] else rates()
