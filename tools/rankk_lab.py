"""Lab: whole gate bootstraps through the rank-k entries (torusk_api.hip) at a few shapes, on the fused route (torusk_fused_kernels.hpp)
where the shape is eligible and on the composed route (a second key of the same rows prepared under NO_RANKK_FUSED = 1), both in this one
session.  The two routes must give the same bits before any time is printed.  usage: python tools/rankk_lab.py"""
import os, statistics, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import learn_fhe_amd as F
dev = torch.device("cuda:0")
rnd = lambda *shape: torch.randint(-(1 << 63), (1 << 63) - 1, shape, dtype=torch.int64, device=dev)
REPS = 5


def timed(fn):
    fn(); torch.cuda.synchronize()  # warm-up
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


t = F.TorusContext()
for k, n, n_lwe, log_b, d in [(2, 512, 630, 7, 3), (3, 256, 630, 6, 2), (1, 1024, 630, 7, 3), (2, 256, 64, 8, 8)]:
    k1 = k + 1
    rows = rnd(n_lwe, k1 * d, k1, n)
    keys = {}
    if F.tggswk_form_for(k, n, log_b, d) == F.TGGSWK_FORM_X3:
        keys["fused"] = F.TggswKeyK(t, k, log_b, d, rows, n)
        assert keys["fused"].form() == F.TGGSWK_FORM_X3
    try:
        F.set_option("NO_RANKK_FUSED", 1)
        keys["composed"] = F.TggswKeyK(t, k, log_b, d, rows, n)
    finally:
        F.set_option("NO_RANKK_FUSED", 0)
    assert keys["composed"].form() == F.TGGSWK_FORM_COMPOSED
    for batch in (1, 64, 1024):
        ksa, ksb, v, a, b = rnd(k * n * 5, n_lwe), rnd(k * n * 5), rnd(n), rnd(batch, n_lwe), rnd(batch)
        outs = {route: key.bootstrap(4, 5, ksa, ksb, v, a, b) for route, key in keys.items()}
        if "fused" in outs:
            assert torch.equal(outs["fused"][0], outs["composed"][0]) and torch.equal(outs["fused"][1], outs["composed"][1]), (k, n, batch)
        for route, key in keys.items():
            dt = timed(lambda: key.bootstrap(4, 5, ksa, ksb, v, a, b))
            print("k=%d N=%d n_lwe=%d (%d,%d) batch %4d %-8s: %9.1f gates/s (%.2f ms)" % (k, n, n_lwe, log_b, d, batch, route, batch / dt, dt * 1e3), flush=True)
    del keys, rows
