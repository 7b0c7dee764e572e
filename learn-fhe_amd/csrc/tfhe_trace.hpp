// Host and device logic of the TGLWE automorphism key switch, the trace and the ring packing (fhe_tglwe_automorphism, fhe_tglwe_trace,
// fhe_tlwe_ring_pack): plain C++ (no HIP), so that it also builds into a stand-alone program.  What is here: the
// admission rules, the index maps -- the signed permutation X -> X^g, the monomial rotation folded into a load, the embedding of a
// TLWE ciphertext -- and the level plan of the packing tree.
//
// Conventions: ring Z[X]/(X^n + 1), n = 2^log_n; an index map says which coefficient a value is read from or goes to, and whether it
// changes sign on the way (X^n = -1).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/fhe_ring.h"

#if defined(__HIPCC__)
#define FHE_TRACE_HD __host__ __device__ inline
#else
#define FHE_TRACE_HD inline
#endif

namespace fhe {

constexpr int TRACE_MAX_STEPS = 11;  // log2 of the largest ring

// log2 n for a ring the torus team kernels cover, -1 otherwise
inline int trace_log_n(size_t n) { return n == 256 ? 8 : n == 512 ? 9 : n == 1024 ? 10 : n == 2048 ? 11 : -1; }

// g odd, 1 <= g < 2n
inline bool trace_g_ok(uint64_t g, size_t n) { return (g & 1) != 0 && g < 2 * (uint64_t)n; }

// the steps lo < u <= hi of a trace: 0 <= lo < hi <= log2 n
inline bool trace_range_ok(int lo, int hi, int log_n) { return lo >= 0 && lo < hi && hi <= log_n; }

// the Galois element of trace step u (1 <= u <= log2 n) and of merge level l = 2^u: 2^u + 1
inline unsigned trace_g(int u) { return (1u << u) + 1; }

// count = 2^c with c <= log2 n: c, else -1
inline int pack_log_count(size_t count, int log_n) {
    if (count == 0 || (count & (count - 1)) != 0) return -1;
    int c = 0;
    while ((size_t(1) << c) < count) ++c;
    return c <= log_n ? c : -1;
}

struct SignedIdx {
    unsigned idx;
    bool neg;
};

// sigma_g: coefficient i of p goes to coefficient idx of p(X^g), negated if neg.  i < n, g < 2n: i g < 2^23
FHE_TRACE_HD SignedIdx auto_target(unsigned i, unsigned g, int log_n) {
    const unsigned n = 1u << log_n, m = (i * g) & (2 * n - 1);
    return SignedIdx{m & (n - 1), m >= n};
}

// coefficient i of X^r p is coefficient idx of p, negated if neg; r < 2n
FHE_TRACE_HD SignedIdx rot_source(unsigned i, unsigned r, int log_n) {
    const unsigned n = 1u << log_n, m = (i + 2 * n - r) & (2 * n - 1);
    return SignedIdx{m & (n - 1), m >= n};
}

// embed: the mask polynomial of the TGLWE ciphertext whose sample_extract(0) is the TLWE ciphertext (a'[n], b').  Coefficient j of it
// is a'[idx], negated if neg (sample_extract(0): a'[0] = a[0], a'[j] = -a[n - j]); the body is b' at coefficient 0 and zero elsewhere
FHE_TRACE_HD SignedIdx embed_source(unsigned j, int log_n) {
    const unsigned n = 1u << log_n;
    return j == 0 ? SignedIdx{0, false} : SignedIdx{n - j, true};
}

// The packing tree of count = 2^c inputs a pack.  Level v = 1 .. c merges pairs with l = 2^v: s = count / l nodes a pack come out,
// node o < s from nodes o and o + s of the level below (level 0: the embedded inputs), the second rotated by n / l, under g = l + 1.
// Node o of level v holds inputs o, o + s, o + 2 s, ... at coefficients 0, n / l, 2 n / l, ...
struct PackLevel {
    unsigned g;      // l + 1
    unsigned rot;    // n / l
    unsigned nodes;  // s: nodes a pack that this level writes
};
inline PackLevel pack_level(int v, int c, int log_n) {
    const unsigned l = 1u << v;
    return PackLevel{l + 1, (1u << log_n) / l, (1u << c) / l};
}
// Words of scratch a pack needs: levels 1 .. c - 1 alternate between two buffers of count / 2 and count / 4 ciphertexts (2 n words
// each); level c writes the result in place.  c <= 1: none
inline size_t pack_scratch_words(int c, int log_n) {
    const size_t n = size_t(1) << log_n, count = size_t(1) << c;
    if (c <= 1) return 0;
    return (count / 2 + (c > 2 ? count / 4 : 0)) * 2 * n;
}
// the trace that follows the tree keeps the multiples of n / count: steps u = log2 n .. c + 1 (none when count = n)
inline int pack_trace_steps(int c, int log_n) { return log_n - c; }

// packs of one launch group: as many as fit `budget` bytes of scratch and `max_teams` teams of the widest level, at least one.
// force > 0 (lab): that many
inline size_t ring_pack_slab(size_t packs, size_t per_pack_bytes, size_t budget, size_t teams_per_pack, size_t max_teams, long force) {
    size_t s = packs;
    if (per_pack_bytes && s > budget / per_pack_bytes) s = budget / per_pack_bytes;
    if (teams_per_pack && s > max_teams / teams_per_pack) s = max_teams / teams_per_pack;
    if (force > 0) s = (size_t)force;
    if (s > packs) s = packs;
    return s ? s : 1;
}

}  // namespace fhe
