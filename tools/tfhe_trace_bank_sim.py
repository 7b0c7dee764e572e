#!/usr/bin/env python3
"""Bank-conflict check of the signed permutation of csrc/tfhe_trace_kernels.hpp (team_torus_automorphism) with the rules of
tools/lds_bank_sim.py: every lane scatters the coefficient it holds to i g mod n with an 8-byte store and reads its own coefficients back
with 8-byte loads.  Two addressings of the team's exchange image: linear (what the kernel uses) and the transforms' padded one
(lds_phys: i + i / 16).  Prints the worst multiplicity per ring, over every g of galois_set and 2n - 1 and every register (1 = conflict
free)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lds_bank_sim import conflicts  # noqa: E402

# (log2 n, log2 coefficients per lane) of the torus team shapes (torus_dispatch.hpp: TorusRing)
SHAPES = [(8, 2), (9, 3), (10, 2), (11, 2)]


def coef_index(log_n, log_e, thread, k):
    """fhew_kernels.hpp coef_index: the coefficient register k of a team's thread holds (first-pass layout of the transform)"""
    passes = -(-log_n // log_e)
    r0 = log_n - (passes - 1) * log_e
    team = 1 << (log_n - log_e)
    gg, r = k >> r0, k & ((1 << r0) - 1)
    grp = thread + team * gg
    h = log_n - r0
    return ((grp >> h) << (h + r0)) | (r << h) | (grp & ((1 << h) - 1))


def main():
    phys = {"linear": lambda i: i, "padded": lambda i: i + (i >> 4)}
    for log_n, log_e in SHAPES:
        n, team = 1 << log_n, 1 << (log_n - log_e)
        gs = [(1 << u) + 1 for u in range(1, log_n + 1)] + [2 * n - 1]
        for name, f in phys.items():
            worst_w = worst_r = 1
            for wave in range(team // 64):
                for k in range(1 << log_e):
                    idx = [coef_index(log_n, log_e, 64 * wave + lane, k) for lane in range(64)]
                    worst_r = max(worst_r, conflicts([f(i) for i in idx], "read64"))
                    for g in gs:
                        worst_w = max(worst_w, conflicts([f((i * g) % n) for i in idx], "write64"))
            print("n = %4d (%d waves, %d a lane)  %-7s scatter write worst multiplicity %d, read-back %d" % (n, team // 64, 1 << log_e, name, worst_w, worst_r))


if __name__ == "__main__":
    main()
