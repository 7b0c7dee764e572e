// csrc/tfhe_lut.hpp alone (no HIP, no library): the shape of a vertically packed look-up, the packing, the extraction indices, the
// workspace and the argument checks.  A stand-alone program (AddressSanitizer + UBSan in tests/test_tfhe_lut_cpu.py).
// `tfhe_lut_host_test pack <m> <n_out> <n>` packs the table T[o][x] = (o << 32) + x + 1 and prints the polynomials, one word per line,
// for the Python model to compare; without arguments it runs the checks and prints "tfhe_lut_host_test ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../learn-fhe_amd/csrc/tfhe_lut.hpp"

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static std::vector<uint64_t> demo_table(int m, size_t n_out) {
    std::vector<uint64_t> t(n_out << m);
    for (size_t o = 0; o < n_out; ++o)
        for (size_t x = 0; x < (size_t(1) << m); ++x) t[(o << m) + x] = (uint64_t(o) << 32) + x + 1;  // never 0: a placed word shows
    return t;
}

// every table word exactly once, zeros elsewhere, extraction indices below n and on the word of address 0
static int check_pack(int m, size_t n_out, size_t n) {
    using namespace fhe;
    LutShape S;
    CHECK(lut_shape(m, n_out, n, &S) == FHE_OK);
    const std::vector<uint64_t> t = demo_table(m, n_out);
    std::vector<uint64_t> polys(S.n_polys * n, ~uint64_t(0));
    CHECK(lut_pack(t.data(), m, n_out, n, polys.data()) == FHE_OK);
    std::vector<int> seen(t.size(), 0);
    size_t zeros = 0;
    for (size_t p = 0; p < S.n_polys; ++p)
        for (size_t j = 0; j < n; ++j) {
            const uint64_t w = polys[p * n + j];
            if (!w) { ++zeros; continue; }
            const size_t o = size_t(w >> 32), x = size_t(w & 0xffffffffu) - 1;
            CHECK(o < n_out && x < (size_t(1) << m) && !seen[(o << m) + x]);
            seen[(o << m) + x] = 1;
            // the issue's statement of the place: polynomial (g, t), coefficient u 2^m + i
            const size_t g = p >> S.h, tt = p & ((size_t(1) << S.h) - 1), u = j >> m, i = j & ((size_t(1) << S.r) - 1);
            CHECK(o == g * S.per_acc + u && x == (tt << S.r) + i && (m >= S.log_n || j == (u << m) + i));
        }
    for (int s : seen) CHECK(s == 1);
    CHECK(zeros == S.n_polys * n - t.size());
    for (size_t o = 0; o < n_out; ++o) {
        CHECK(lut_extract_index(S, o) < n && lut_acc_of(S, o) < S.n_acc);
        CHECK(polys[(lut_acc_of(S, o) << S.h) * n + lut_extract_index(S, o)] == t[o << m]);  // address 0 needs no rotation and leaf 0
    }
    return 0;
}

static int checks() {
    using namespace fhe;
    LutShape S;
    // m < log n: no tree, several outputs per accumulator
    CHECK(lut_shape(3, 3, 256, &S) == FHE_OK && S.r == 3 && S.h == 0 && S.per_acc == 32 && S.n_acc == 1 && S.n_polys == 1);
    CHECK(lut_shape(7, 5, 256, &S) == FHE_OK && S.r == 7 && S.h == 0 && S.per_acc == 2 && S.n_acc == 3 && S.n_polys == 3);
    CHECK(lut_shape(8, 8, 1024, &S) == FHE_OK && S.r == 8 && S.h == 0 && S.per_acc == 4 && S.n_acc == 2 && S.n_polys == 2);
    // m = log n: one output fills an accumulator
    CHECK(lut_shape(8, 3, 256, &S) == FHE_OK && S.r == 8 && S.h == 0 && S.per_acc == 1 && S.n_acc == 3 && S.n_polys == 3);
    // m > log n: a tree over the high bits
    CHECK(lut_shape(10, 3, 256, &S) == FHE_OK && S.r == 8 && S.h == 2 && S.per_acc == 1 && S.n_acc == 3 && S.n_polys == 12);
    CHECK(lut_shape(12, 1, 1024, &S) == FHE_OK && S.r == 10 && S.h == 2 && S.n_polys == 4);
    CHECK(lut_shape(21, 1, 2048, &S) == FHE_OK && S.h == 10 && S.n_polys == 1024);
    // rejections
    CHECK(lut_shape(0, 1, 256, &S) == FHE_ERR_INVALID && lut_shape(-1, 1, 256, &S) == FHE_ERR_INVALID && lut_shape(3, 0, 256, &S) == FHE_ERR_INVALID);
    CHECK(lut_shape(3, 1, 1000, &S) == FHE_ERR_INVALID && lut_shape(3, 1, 0, &S) == FHE_ERR_INVALID && lut_shape(3, 1, 256, nullptr) == FHE_ERR_INVALID);
    CHECK(lut_shape(3, 1, 128, &S) == FHE_ERR_UNSUPPORTED && lut_shape(3, 1, 4096, &S) == FHE_ERR_UNSUPPORTED);
    CHECK(lut_shape(19, 1, 256, &S) == FHE_ERR_UNSUPPORTED && lut_shape(18, 1, 256, &S) == FHE_OK);          // 11 and 10 tree bits
    CHECK(lut_shape(18, 64, 256, &S) == FHE_OK && S.n_polys == 65536 && lut_shape(18, 65, 256, &S) == FHE_ERR_UNSUPPORTED);
    CHECK(lut_shape(8, 65536, 256, &S) == FHE_OK && lut_shape(8, 65537, 256, &S) == FHE_ERR_UNSUPPORTED);
    CHECK(lut_shape(8, ~size_t(0), 256, &S) == FHE_ERR_UNSUPPORTED);
    // packing
    for (size_t n : {size_t(256), size_t(1024)})
        for (int m : {1, 3, 7, 8, 10, 11})
            for (size_t n_out : {size_t(1), size_t(3), size_t(5)})
                if (check_pack(m, n_out, n)) return 1;
    if (check_pack(8, 8, 1024)) return 1;  // the C example's shape
    std::vector<uint64_t> w(4096);
    CHECK(lut_pack(nullptr, 3, 1, 256, w.data()) == FHE_ERR_INVALID && lut_pack(w.data(), 3, 1, 256, nullptr) == FHE_ERR_INVALID);
    CHECK(lut_pack(w.data(), 0, 1, 256, w.data()) == FHE_ERR_INVALID && lut_pack(w.data(), 3, 1, 128, w.data()) == FHE_ERR_UNSUPPORTED);
    // the tree's two areas: a level's output fits its area, the areas do not overlap, the accumulators stand where the last level wrote
    for (int h = 0; h <= LUT_MAX_TREE_BITS; ++h) {
        const size_t accs = 6, nodes = accs * lut_nodes_per_acc(h);
        for (int v = 0; v < h; ++v) {
            const size_t out = accs << (h - 1 - v), at = lut_level_area(h, v, accs);
            CHECK(at + out <= nodes);
            CHECK((v & 1) ? at == accs << (h - 1) : at + out <= accs << (h - 1));  // Y starts where X ends
            if (v) CHECK(lut_level_area(h, v - 1, accs) != at);                     // a level never writes the area it reads
        }
        CHECK(lut_acc_area(h, accs) + accs <= nodes);
        CHECK(h == 0 || lut_acc_area(h, accs) == lut_level_area(h, h - 1, accs));
    }
    CHECK(lut_nodes_per_acc(0) == 1 && lut_nodes_per_acc(1) == 1 && lut_nodes_per_acc(2) == 3 && lut_nodes_per_acc(10) == 768);
    // the workspace, stated once by TfheScratch: nodes a | nodes b | extracted a | b~ (unused, one word per node) | extracted b
    size_t words = 0;
    CHECK(lut_workspace(256, 10, 3, 0, 5, &words) == FHE_OK && words == 2 * (5 * 3 * 3) * 256 + 5 * 3 * 3);
    CHECK(lut_workspace(256, 10, 3, 8, 5, &words) == FHE_OK && words == 2 * (5 * 3 * 3) * 256 + 15 * 256 + 5 * 3 * 3 + 15);
    CHECK(lut_workspace(1024, 8, 8, 630, 3, &words) == FHE_OK && words == 2 * (3 * 2) * 1024 + 24 * 1024 + 6 + 24);
    CHECK(lut_workspace(1024, 8, 8, 630, 3, nullptr) == FHE_ERR_INVALID && lut_workspace(1000, 8, 8, 630, 3, &words) == FHE_ERR_INVALID);
    CHECK(lut_workspace(256, 19, 1, 0, 1, &words) == FHE_ERR_UNSUPPORTED);
    CHECK(lut_workspace(256, 8, 1, 0, size_t(1) << 31, &words) == FHE_ERR_UNSUPPORTED && lut_workspace(256, 18, 1, 0, size_t(1) << 22, &words) == FHE_ERR_UNSUPPORTED);
    CHECK(lut_shape(10, 3, 256, &S) == FHE_OK);
    const TfheScratch L = lut_scratch(S, 8, 5);
    CHECK(L.acc_a == 0 && L.acc_b == 45 * 256 && L.ext_a == 90 * 256 && L.ext_b == 90 * 256 + 15 * 256 + 45 && L.acc_b % 2 == 0 && L.ext_a % 2 == 0);
    // the selectors of a call lie inside the key
    CHECK(lut_selectors_ok(0, 3, 8, 24) && !lut_selectors_ok(1, 3, 8, 24) && lut_selectors_ok(1, 3, 8, 25) && !lut_selectors_ok(30, 0, 8, 24));
    CHECK(lut_selectors_ok(24, 0, 8, 24) && !lut_selectors_ok(~size_t(0), 1, 8, 24) && !lut_selectors_ok(0, ~size_t(0), 8, 24));
    std::printf("tfhe_lut_host_test ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 5 && !std::strcmp(argv[1], "pack")) {
        const int m = std::atoi(argv[2]);
        const size_t n_out = (size_t)std::atol(argv[3]), n = (size_t)std::atol(argv[4]);
        fhe::LutShape S;
        int rc = fhe::lut_shape(m, n_out, n, &S);
        if (rc != FHE_OK) { std::printf("status %d\n", rc); return 2; }
        const std::vector<uint64_t> t = demo_table(m, n_out);
        std::vector<uint64_t> polys(S.n_polys * n);
        rc = fhe::lut_pack(t.data(), m, n_out, n, polys.data());
        if (rc != FHE_OK) { std::printf("status %d\n", rc); return 2; }
        for (uint64_t v : polys) std::printf("%llu\n", (unsigned long long)v);
        return 0;
    }
    return checks();
}
