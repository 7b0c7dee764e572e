// csrc/ckks_hoist.hpp as a stand-alone host program (built with -fsanitize=address,undefined by tests/test_ckks_hoist_cpu.py): the
// evaluation-domain permutation against tables made in Python from the transform's output order, the two facts the kernels lean on
// (pairs, blocks), the fold bound, the term tables and the workspace layouts with their admission rules.
//
// usage: ckks_hoist_host_test vectors.txt
//   pi <log_n> <t> <pi(0)> ... <pi(n-1)>
//   fold <bits> <F>
//   rot <n> <L> <K> <batch> <ok> <ext> <bh> <p> <total>
//   mat <n> <L> <K> <batch> <n_giant> <ok> <ext> <bh> <w> <x> <tmp> <total>
//   terms <n_giant> <n_baby> <present bits as one string> <terms> <max> <tab ...>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../learn-fhe_amd/csrc/ckks_hoist.hpp"

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: %s (line: %s)\n", __FILE__, __LINE__, #cond, line.c_str()); \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    size_t pis = 0, lays = 0, others = 0;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        if (kind == "pi") {
            int log_n;
            unsigned t;
            in >> log_n >> t;
            const unsigned n = 1u << log_n;
            std::vector<unsigned> want(n), seen(n, 0);
            for (unsigned k = 0; k < n; ++k) in >> want[k];
            CHECK(!in.fail());
            for (unsigned k = 0; k < n; ++k) {
                const unsigned p = fhe::hoist_pi(k, t, log_n);
                CHECK(p < n && p == want[k]);
                ++seen[p];
                if (n >= 2) CHECK(fhe::hoist_pi(k ^ 1u, t, log_n) == (p ^ 1u));  // pairs
                for (int s = 0; s <= log_n; ++s)                                   // blocks: the block of pi(k) depends on the block of k alone
                    CHECK((fhe::hoist_pi(k & ~((1u << s) - 1), t, log_n) >> s) == (p >> s));
            }
            for (unsigned k = 0; k < n; ++k) CHECK(seen[k] == 1);
            ++pis;
        } else if (kind == "fold") {
            int bits, want;
            in >> bits >> want;
            CHECK(!in.fail() && fhe::hoist_fold_bound(bits) == want);
            CHECK(fhe::hoist_bits((uint64_t(1) << bits) - 1) == bits && fhe::hoist_bits(uint64_t(1) << (bits - 1)) == bits);
            ++others;
        } else if (kind == "rot") {
            size_t n, L, K, batch, e, b, p, total;
            int ok;
            in >> n >> L >> K >> batch >> ok >> e >> b >> p >> total;
            CHECK(!in.fail());
            fhe::HoistRotWs ws;
            CHECK(fhe::hoist_rot_ws(n, L, K, batch, &ws) == (ok != 0));
            if (ok) CHECK(ws.ext == e && ws.bh == b && ws.p == p && ws.total == total && ws.total * 8 / 8 == ws.total);
            ++lays;
        } else if (kind == "mat") {
            size_t n, L, K, batch, ng, e, b, w, x, tmp, total;
            int ok;
            in >> n >> L >> K >> batch >> ng >> ok >> e >> b >> w >> x >> tmp >> total;
            CHECK(!in.fail());
            fhe::HoistMatWs ws;
            CHECK(fhe::hoist_mat_ws(n, L, K, batch, ng, &ws) == (ok != 0));
            if (ok) {
                CHECK(ws.ext == e && ws.bh == b && ws.w == w && ws.x == x && ws.tmp == tmp && ws.total == total);
                CHECK(ng * 2 * batch * (L - 1) * n <= ws.x - ws.w);  // the v_i fit where w was
            }
            ++lays;
        } else if (kind == "terms") {
            int ng, nb, want_terms, want_max;
            std::string bits;
            in >> ng >> nb >> bits >> want_terms >> want_max;
            CHECK(!in.fail() && bits.size() == size_t(ng) * nb);
            std::vector<uint8_t> present(bits.size());
            for (size_t i = 0; i < bits.size(); ++i) present[i] = bits[i] == '1';
            std::vector<int> tab(size_t(ng) + 1 + size_t(ng) * nb, -1);
            int mx = -1;
            CHECK(fhe::hoist_terms(present.data(), ng, nb, tab.data(), &mx) == want_terms && mx == want_max);
            for (int i = 0; i < ng + 1 + want_terms; ++i) {
                int v;
                in >> v;
                CHECK(!in.fail() && tab[i] == v);
            }
            ++others;
        } else if (!kind.empty()) {
            CHECK(false);
        }
    }
    const uint32_t up[3] = {0, 3, 7}, flat[3] = {0, 3, 3}, down[2] = {4, 1};
    line = "ascending";
    CHECK(fhe::hoist_ascending(up, 3) && !fhe::hoist_ascending(flat, 3) && !fhe::hoist_ascending(down, 2) && fhe::hoist_ascending(up, 1));
    if (!pis || !lays || !others) return 3;
    std::printf("ckks_hoist_host_test ok (%zu permutations, %zu layouts, %zu tables)\n", pis, lays, others);
    return 0;
}
