// Stand-alone host program over learn-fhe_amd/csrc/tfhe_circuit.hpp (the netlist compiler of fhe_tfhe_circuit_create; no HIP):
// random netlists against a restatement (liveness by recursion from the outputs, levels from the original netlist), the slot
// numbering's and the repacked term list's invariants, and every rejected case.  Built with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "../learn-fhe_amd/csrc/tfhe_circuit.hpp"

static uint64_t state = 0x13198a2e03707344ull;
static uint32_t rnd(uint32_t m) {
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return (uint32_t)((state >> 11) % m);
}

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static int one(size_t n_inputs, size_t n_nodes, size_t n_outputs, size_t n_tables) {
    std::vector<fhe_tfhe_node> nodes(n_nodes);
    std::vector<fhe_tfhe_term> terms;
    for (uint32_t pad = rnd(3); pad--;) terms.push_back(fhe_tfhe_term{0xffffffffu, 0});  // unused terms may hold anything
    for (size_t g = 0; g < n_nodes; ++g) {
        nodes[g] = fhe_tfhe_node{};
        nodes[g].first_term = (uint32_t)terms.size();
        nodes[g].n_terms = 1 + rnd(rnd(4) ? 3 : 16);
        nodes[g].constant = ((uint64_t)rnd(1u << 31) << 33) | rnd(1u << 31);
        nodes[g].table = rnd((uint32_t)n_tables);
        nodes[g].pad = rnd(7);
        const uint32_t below = (uint32_t)(n_inputs + g);
        for (uint32_t k = 0; k < nodes[g].n_terms; ++k) {
            // mostly recent wires (deep circuits), sometimes any lower wire; a wire may appear twice in a node
            const uint32_t w = rnd(4) ? below - 1 - rnd(below < 6 ? below : 6) : rnd(below);
            int32_t weight = (int32_t)rnd(9) - 4;
            if (!weight) weight = rnd(2) ? INT32_MIN : INT32_MAX;
            terms.push_back(fhe_tfhe_term{w, weight});
        }
        if (rnd(5) == 0) terms.push_back(fhe_tfhe_term{0xffffffffu, 0});
    }
    std::vector<uint32_t> outputs(n_outputs);
    for (auto &o : outputs) o = rnd((uint32_t)(n_inputs + n_nodes));
    fhe::TfheCircuitPlan P;
    REQUIRE(fhe::tfhe_circuit_compile(nodes.data(), n_nodes, terms.data(), terms.size(), n_inputs, n_tables, outputs.data(), n_outputs, &P) == FHE_OK);
    // restatement: live = reachable from an output; level by recursion
    std::vector<int> live(n_inputs + n_nodes, 0), level(n_inputs + n_nodes, -1);
    std::function<void(uint32_t)> mark = [&](uint32_t w) {
        if (live[w]) return;
        live[w] = 1;
        if (w >= n_inputs)
            for (uint32_t k = 0; k < nodes[w - n_inputs].n_terms; ++k) mark(terms[nodes[w - n_inputs].first_term + k].wire);
    };
    for (uint32_t o : outputs) mark(o);
    std::function<int(uint32_t)> lev = [&](uint32_t w) {
        if (w < n_inputs) return 0;
        if (level[w] >= 0) return level[w];
        int l = 0;
        for (uint32_t k = 0; k < nodes[w - n_inputs].n_terms; ++k) l = std::max(l, lev(terms[nodes[w - n_inputs].first_term + k].wire));
        return level[w] = l + 1;
    };
    size_t n_live = 0, n_levels = 0;
    std::vector<size_t> width;
    for (size_t g = 0; g < n_nodes; ++g) {
        const uint32_t expect = live[n_inputs + g] ? (uint32_t)lev((uint32_t)(n_inputs + g)) : 0u;
        REQUIRE(P.level_of_node[g] == expect);
        if (!expect) continue;
        ++n_live;
        n_levels = std::max(n_levels, (size_t)expect);
        if (width.size() < expect) width.resize(expect, 0);
        ++width[expect - 1];
    }
    REQUIRE(P.n_live == n_live && P.n_levels == n_levels && P.nodes.size() == n_live && P.level_start.size() == n_levels + 1);
    REQUIRE(P.max_width == (width.empty() ? 0 : *std::max_element(width.begin(), width.end())));
    // slots: level l + 1 is level_start[l] .. level_start[l + 1] - 1, netlist order within a level; a node reads lower LEVELS only
    std::vector<uint32_t> slot_of(n_inputs + n_nodes, 0xffffffffu);
    for (size_t w = 0; w < n_inputs; ++w) slot_of[w] = (uint32_t)w;
    for (size_t l = 0; l < n_levels; ++l) {
        REQUIRE(P.level_start[l + 1] - P.level_start[l] == width[l]);
        uint32_t s = (uint32_t)(n_inputs + P.level_start[l]);
        for (size_t g = 0; g < n_nodes; ++g)
            if (P.level_of_node[g] == l + 1) slot_of[n_inputs + g] = s++;
    }
    size_t t_at = 0;
    for (size_t g = 0; g < n_nodes; ++g) {
        if (!P.level_of_node[g]) continue;
        const size_t i = slot_of[n_inputs + g] - n_inputs;
        REQUIRE(i < n_live);
        const fhe_tfhe_node &nd = P.nodes[i];
        REQUIRE(nd.n_terms == nodes[g].n_terms && nd.constant == nodes[g].constant && nd.table == nodes[g].table && nd.pad == 0);
        REQUIRE((size_t)nd.first_term + nd.n_terms <= P.terms.size());
        for (uint32_t k = 0; k < nd.n_terms; ++k) {
            const fhe_tfhe_term &src = terms[nodes[g].first_term + k], &dst = P.terms[nd.first_term + k];
            REQUIRE(dst.wire == slot_of[src.wire] && dst.weight == src.weight);
            REQUIRE(dst.wire < n_inputs + P.level_start[P.level_of_node[g] - 1]);  // produced by an earlier level
        }
    }
    // the repacked terms: the live nodes' terms in slot order, nothing else
    for (size_t i = 0; i < n_live; ++i) {
        REQUIRE(P.nodes[i].first_term == t_at);
        t_at += P.nodes[i].n_terms;
    }
    REQUIRE(t_at == P.terms.size());
    for (size_t o = 0; o < n_outputs; ++o) REQUIRE(P.outputs[o] == slot_of[outputs[o]]);
    return 0;
}

static int rejected() {
    fhe::TfheCircuitPlan P;
    fhe_tfhe_term terms[3] = {{0, 1}, {1, -1}, {2, 4}};
    fhe_tfhe_node ok[2] = {{0, 2, 7, 0, 0}, {1, 2, 0, 1, 0}};
    uint32_t out[2] = {3, 0};
    auto run = [&](const fhe_tfhe_node *nodes, size_t n_nodes, const fhe_tfhe_term *t, size_t n_terms, size_t n_inputs, size_t n_tables,
                   const uint32_t *o, size_t n_outputs) { return fhe::tfhe_circuit_compile(nodes, n_nodes, t, n_terms, n_inputs, n_tables, o, n_outputs, &P); };
    REQUIRE(run(ok, 2, terms, 3, 2, 2, out, 2) == FHE_OK);
    REQUIRE(P.n_live == 2 && P.n_levels == 2);
    REQUIRE(run(ok, 2, terms, 2, 2, 2, out, 2) == FHE_ERR_INVALID);               // a term range outside terms
    fhe_tfhe_node bad = ok[0];
    bad.first_term = 0xffffffffu;
    REQUIRE(run(&bad, 1, terms, 3, 2, 2, out + 1, 1) == FHE_ERR_INVALID);         // ... without wrapping
    bad = ok[0]; bad.n_terms = 0;
    REQUIRE(run(&bad, 1, terms, 3, 2, 2, out + 1, 1) == FHE_ERR_INVALID);
    bad = ok[0]; bad.n_terms = 17;
    std::vector<fhe_tfhe_term> many(17, fhe_tfhe_term{0, 1});
    REQUIRE(run(&bad, 1, many.data(), 17, 2, 2, out + 1, 1) == FHE_ERR_INVALID);
    bad.n_terms = 16;
    REQUIRE(run(&bad, 1, many.data(), 17, 2, 2, out + 1, 1) == FHE_OK);
    fhe_tfhe_term fwd[2] = {{0, 1}, {2, 1}};                                       // node 0 reading its own wire
    REQUIRE(run(ok, 1, fwd, 2, 2, 2, out + 1, 1) == FHE_ERR_INVALID);
    fhe_tfhe_term far[2] = {{0, 1}, {1u << 30, 1}};
    REQUIRE(run(ok, 1, far, 2, 2, 2, out + 1, 1) == FHE_ERR_INVALID);
    fhe_tfhe_term zero[2] = {{0, 1}, {1, 0}};
    REQUIRE(run(ok, 1, zero, 2, 2, 2, out + 1, 1) == FHE_ERR_INVALID);             // a weight of 0
    REQUIRE(run(ok, 2, terms, 3, 2, 1, out, 2) == FHE_ERR_INVALID);                // table >= n_tables
    REQUIRE(run(ok, 2, terms, 3, 0, 2, out, 2) == FHE_ERR_INVALID);                // no inputs
    REQUIRE(run(ok, 2, terms, 3, 2, 2, out, 0) == FHE_ERR_INVALID);                // no outputs
    REQUIRE(run(ok, 2, terms, 3, 2, 2, nullptr, 2) == FHE_ERR_INVALID);
    uint32_t out_bad[1] = {4};
    REQUIRE(run(ok, 2, terms, 3, 2, 2, out_bad, 1) == FHE_ERR_INVALID);            // an output past the last wire
    REQUIRE(run(ok, 2, terms, 3, 2, 65537, out, 2) == FHE_ERR_INVALID);            // too many tables
    REQUIRE(run(ok, 2, terms, 3, 2, 65536, out, 2) == FHE_OK);
    REQUIRE(run(nullptr, 0, nullptr, 0, (size_t(1) << 24) + 1, 1, out + 1, 1) == FHE_ERR_INVALID);  // more than 2^24 wires
    REQUIRE(run(nullptr, 0, nullptr, 0, 3, 0, out + 1, 1) == FHE_OK);              // no nodes: outputs name inputs
    REQUIRE(P.n_live == 0 && P.n_levels == 0 && P.max_width == 0);
    return 0;
}

int main() {
    if (rejected()) return 1;
    for (int it = 0; it < 300; ++it)
        if (one(1 + rnd(6), rnd(60), 1 + rnd(5), 1 + rnd(4))) return 1;
    if (one(3, 2000, 4, 9)) return 1;
    std::printf("tfhe_circuit_host_test ok\n");
    return 0;
}
