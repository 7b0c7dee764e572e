// csrc/tfhe_trace.hpp as a stand-alone host program (built with -fsanitize=address,undefined by tests/test_tfhe_trace_cpu.py): the
// signed permutation's index map against tables that the Python test computes, the level plan of the packing tree, the embedding's and
// the rotation's index maps against their definitions, and the admission rules at their edges.
//   argv[1]: a text file of lines
//     auto  <n> <g> <n values 2 target + negated>       auto_target(i, g, log2 n) for i = 0 .. n - 1
//     level <n> <c> <v> <g> <rot> <nodes>               pack_level(v, c, log2 n)
//     plan  <n> <c> <scratch words> <trace steps>       pack_scratch_words, pack_trace_steps
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../learn-fhe_amd/csrc/tfhe_trace.hpp"

static int fails = 0;
#define CHECK(c)                                                 \
    do {                                                         \
        if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

int main(int argc, char **argv) {
    using namespace fhe;
    // rings
    CHECK(trace_log_n(256) == 8 && trace_log_n(512) == 9 && trace_log_n(1024) == 10 && trace_log_n(2048) == 11);
    CHECK(trace_log_n(0) == -1 && trace_log_n(128) == -1 && trace_log_n(300) == -1 && trace_log_n(4096) == -1);
    // g odd, below 2n
    CHECK(trace_g_ok(1, 256) && trace_g_ok(3, 256) && trace_g_ok(511, 256) && trace_g_ok(4095, 2048));
    CHECK(!trace_g_ok(0, 256) && !trace_g_ok(2, 256) && !trace_g_ok(512, 256) && !trace_g_ok(513, 256) && !trace_g_ok(4097, 2048));
    CHECK(!trace_g_ok((uint64_t(1) << 32) + 3, 256));
    // 0 <= lo < hi <= log2 n
    for (int lo = -1; lo <= 12; ++lo)
        for (int hi = -1; hi <= 12; ++hi) CHECK(trace_range_ok(lo, hi, 10) == (lo >= 0 && lo < hi && hi <= 10));
    for (int u = 1; u <= 11; ++u) CHECK(trace_g(u) == (1u << u) + 1);
    // count = 2^c <= n
    CHECK(pack_log_count(1, 8) == 0 && pack_log_count(2, 8) == 1 && pack_log_count(256, 8) == 8 && pack_log_count(2048, 11) == 11);
    CHECK(pack_log_count(0, 8) == -1 && pack_log_count(3, 8) == -1 && pack_log_count(512, 8) == -1 && pack_log_count(255, 8) == -1);
    CHECK(pack_log_count(size_t(1) << 40, 11) == -1);
    // slabs: the budget, the team limit, the lab's force, never zero, never more than there are
    CHECK(ring_pack_slab(10, 100, 1000, 4, 1000, 0) == 10 && ring_pack_slab(100, 100, 1000, 4, 1000, 0) == 10);
    CHECK(ring_pack_slab(100, 100, 100000, 4, 40, 0) == 10 && ring_pack_slab(100, 100, 10, 4, 1000, 0) == 1);
    CHECK(ring_pack_slab(100, 0, 10, 4, 1000, 0) == 100 && ring_pack_slab(3, 100, 1000, 4, 1000, 2) == 2 && ring_pack_slab(3, 100, 1000, 4, 1000, 7) == 3);
    // the rotation folded into a load, and the embedding, against their definitions at every ring
    for (int log_n = 8; log_n <= 11; ++log_n) {
        const unsigned n = 1u << log_n;
        for (unsigned r : {0u, 1u, n / 2, n - 1, n, n + 1, 2 * n - 1}) {
            std::vector<int> seen(n, 0);
            for (unsigned i = 0; i < n; ++i) {
                const SignedIdx s = rot_source(i, r, log_n);
                CHECK(s.idx < n);
                const unsigned m = (s.idx + r) % (2 * n);  // X^idx X^r = +-X^i
                CHECK(m % n == i && (m >= n) == s.neg);
                ++seen[s.idx];
            }
            for (unsigned i = 0; i < n; ++i) CHECK(seen[i] == 1);
        }
        CHECK(embed_source(0, log_n).idx == 0 && !embed_source(0, log_n).neg);
        for (unsigned j = 1; j < n; ++j) CHECK(embed_source(j, log_n).idx == n - j && embed_source(j, log_n).neg);
    }

    if (argc < 2) { std::printf("usage: %s vectors.txt\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    char kind[8];
    size_t autos = 0, levels = 0, plans = 0;
    while (std::fscanf(f, "%7s", kind) == 1) {
        if (!std::strcmp(kind, "auto")) {
            unsigned n, g;
            if (std::fscanf(f, "%u %u", &n, &g) != 2 || trace_log_n(n) < 0) { ++fails; break; }
            CHECK(trace_g_ok(g, n));
            bool ok = true;
            for (unsigned i = 0; i < n; ++i) {
                unsigned want;
                if (std::fscanf(f, "%u", &want) != 1) { ok = false; break; }
                const SignedIdx t = auto_target(i, g, trace_log_n(n));
                if (t.idx * 2 + (t.neg ? 1 : 0) != want) ok = false;
            }
            CHECK(ok);
            ++autos;
        } else if (!std::strcmp(kind, "level")) {
            unsigned n, c, v, g, rot, nodes;
            if (std::fscanf(f, "%u %u %u %u %u %u", &n, &c, &v, &g, &rot, &nodes) != 6) { ++fails; break; }
            const PackLevel L = pack_level((int)v, (int)c, trace_log_n(n));
            CHECK(L.g == g && L.rot == rot && L.nodes == nodes && L.g == trace_g((int)v));
            ++levels;
        } else if (!std::strcmp(kind, "plan")) {
            unsigned n, c, steps;
            unsigned long long words;
            if (std::fscanf(f, "%u %u %llu %u", &n, &c, &words, &steps) != 4) { ++fails; break; }
            CHECK(pack_scratch_words((int)c, trace_log_n(n)) == words && pack_trace_steps((int)c, trace_log_n(n)) == (int)steps);
            CHECK(pack_log_count(size_t(1) << c, trace_log_n(n)) == (int)c);
            ++plans;
        } else {
            ++fails;
            break;
        }
    }
    std::fclose(f);
    CHECK(autos > 0 && levels > 0 && plans > 0);
    if (fails) return 1;
    std::printf("tfhe_trace_host_test ok (%zu index tables, %zu levels, %zu plans)\n", autos, levels, plans);
    return 0;
}
