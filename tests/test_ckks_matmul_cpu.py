"""No-GPU checks of the CKKS diagonal-matrix product: the baby-step / giant-step split (`bsgs_split`, util/src/misc/matrix.rs:45-52,
125-150) against brute force, and the summed-rescale identity of csrc/ckks_matmul_kernels.hpp with Python integers."""
import pytest


def rotations(indices, k):
    """the distinct non-zero rotations of the split at k (matrix.rs:147-149 `ijs` without 0)"""
    return len(({(d // k) * k for d in indices} | {d % k for d in indices}) - {0})


N = 16
INDEX_SETS = [[0]] + [[0, N - m] for m in (1, 2, 4)] + [[0, m, N - m] for m in (1, 2, 4)] + [list(range(16)), [0, 1, 15], [3, 6, 9]]


@pytest.mark.parametrize("indices", INDEX_SETS, ids=str)
def test_bsgs_split_against_brute_force(fhe, indices):
    k, split = fhe.bsgs_split(indices)
    counts = {kk: rotations(indices, kk) for kk in range(1, max(max(indices), 1) + 1)}
    assert counts[k] == min(counts.values())                       # the fewest non-zero rotations
    assert all(counts[kk] > counts[k] for kk in range(1, k))       # the first such k (`min_by_key` keeps the first minimum)
    assert sorted(i + j for i, js in split.items() for j in js) == sorted(indices)
    assert all(i % k == 0 and all(0 <= j < k for j in js) and js == sorted(set(js)) for i, js in split.items())


def test_bsgs_split_known_answers(fhe):
    assert fhe.bsgs_split(range(16)) == (4, {i: [0, 1, 2, 3] for i in (0, 4, 8, 12)})  # k = 3 and k = 5 need 7 rotations, k = 4 six
    # {0, 1, 15}: k = 1 rotates by {1, 15}, k = 2 by {14, 1}: a tie, the first k wins
    assert rotations([0, 1, 15], 1) == rotations([0, 1, 15], 2) == 2
    assert fhe.bsgs_split([0, 1, 15]) == (1, {0: [0], 1: [0], 15: [0]})
    # {3, 6, 9}: k = 6 puts 9 = 6 + 3 on rotations it already has: {6, 3} against {3, 6, 9} at k = 1 or 3
    assert fhe.bsgs_split([3, 6, 9]) == (6, {0: [3], 6: [0, 3]})
    assert fhe.bsgs_split([0]) == (1, {0: [0]})


def rescale(x, mods):
    """rns.rs:99-118 `rescale()` (K == 1) of one coefficient: residues over mods -> residues over mods[:-1]"""
    ql = mods[-1]
    vp = (x[-1] + ql // 2) % ql
    return [((x[l] + (ql // 2) % q - vp % q) * pow(ql, -1, q)) % q for l, q in enumerate(mods[:-1])]


@pytest.mark.parametrize("terms", [1, 2, 17])
def test_summed_rescale_identity(terms):
    """sum_j rescale(x^j)_l == (sum_j x^j_l + J h_l - sum_j lift((x^j_last + h_last) mod q_last)) q_last^-1 mod q_l, with limbs both
    smaller and larger than q_last and residues at the edges (0, 1, h, h + 1, q - 1)"""
    q_small, q_last, q_big = (1 << 50) - 27, (1 << 60) - 93, (1 << 61) - 1  # q_0 < q_last < q_1; only coprimality matters here
    mods = [q_small, q_big, q_last]
    edges = lambda q: [0, 1, q // 2 - 1, q // 2, q // 2 + 1, q - 2, q - 1]  # noqa: E731
    h = q_last // 2
    for shift in range(7):
        xs = [[edges(q)[(shift + 3 * j + l) % 7] for l, q in enumerate(mods)] for j in range(terms)]
        for last_edge in (0, 3, 6):  # the last limbs as drawn, then all at h (the lift is q_last - 1), then all at q_last - 1
            for x in xs:
                x[-1] = edges(q_last)[last_edge] if last_edge else x[-1]
            want = [sum(rescale(x, mods)[l] for x in xs) % q for l, q in enumerate(mods[:-1])]
            lifts = [(x[-1] + h) % q_last for x in xs]
            if terms == 17 and last_edge == 3:
                assert sum(lifts) >= 1 << 64  # why the kernel reduces every lift into q_l before adding
            for l, q in enumerate(mods[:-1]):
                acc = sum(x[l] for x in xs) % q                     # what the evaluation-domain accumulation leaves
                lift_sum = 0
                for v in lifts:                                     # the kernel's order: reduce, then add mod q_l
                    lift_sum = (lift_sum + v % q) % q
                got = ((acc + terms * (h % q) - lift_sum) * pow(q_last, -1, q)) % q
                assert got == want[l], (terms, shift, last_edge, l)
