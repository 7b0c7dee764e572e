// Stand-alone host program over learn-fhe_amd/csrc/netlist_levels.hpp (no HIP): the pruning and levelling core that the FHEW and the TFHE
// netlist compilers share.  Random DAGs of two-input gates -- fan-out, dead gates, outputs that name inputs, no gates at all -- go to the
// core and, translated gate for gate (a FHEW gate with free inversions; a TFHE node with one term per gate input and log_funcs = 0), to
// both compilers.  Required: the core's liveness, levels and live-node order equal a direct restatement (a stable sort by level, not the
// counting sort); both plans carry those levels, level_start, max_width and n_live; and both plans are the translation of the live gates
// in that order.
// Built with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../learn-fhe_amd/csrc/fhew_circuit.hpp"
#include "../learn-fhe_amd/csrc/tfhe_circuit.hpp"

static uint64_t state = 0x452821e638d01377ull;
static uint32_t rnd(uint32_t m) {
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return (uint32_t)((state >> 11) % m);
}

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

struct Dag {
    size_t n_inputs = 0;
    std::vector<uint32_t> in0, in1;   // gate g reads wires in0[g], in1[g] < n_inputs + g
    std::vector<uint32_t> outputs;    // wires
};

// `near`: inputs from the last few wires (deep netlists) instead of from all lower wires (wide ones)
static Dag random_dag(size_t n_inputs, size_t n_gates, size_t n_outputs, bool near, bool outputs_from_inputs) {
    Dag D;
    D.n_inputs = n_inputs;
    for (size_t g = 0; g < n_gates; ++g) {
        const uint32_t below = (uint32_t)(n_inputs + g), span = near && below > 4 ? 4 : below;
        D.in0.push_back(below - 1 - rnd(span));
        D.in1.push_back(below - 1 - rnd(span));
    }
    for (size_t o = 0; o < n_outputs; ++o) D.outputs.push_back(rnd((uint32_t)(outputs_from_inputs ? n_inputs : n_inputs + n_gates)));
    return D;
}

static int check(const Dag &D) {
    const size_t n_inputs = D.n_inputs, n_gates = D.in0.size(), n_wires = n_inputs + n_gates;
    // the restatement
    std::vector<unsigned char> live(n_wires, 0);
    for (uint32_t w : D.outputs) live[w] = 1;
    for (size_t g = n_gates; g-- > 0;)
        if (live[n_inputs + g]) live[D.in0[g]] = live[D.in1[g]] = 1;
    std::vector<uint32_t> level(n_wires, 0), level_of(n_gates, 0), order;
    for (size_t g = 0; g < n_gates; ++g) {
        if (!live[n_inputs + g]) continue;
        level[n_inputs + g] = level_of[g] = 1 + std::max(level[D.in0[g]], level[D.in1[g]]);
        order.push_back((uint32_t)g);
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return level_of[a] < level_of[b]; });
    const uint32_t n_levels = order.empty() ? 0 : level_of[order.back()];
    std::vector<uint32_t> level_start(n_levels + 1, 0);
    size_t max_width = 0;
    for (uint32_t l = 1; l <= n_levels; ++l) {
        const size_t width = (size_t)std::count(level_of.begin(), level_of.end(), l);
        level_start[l] = level_start[l - 1] + (uint32_t)width;
        max_width = std::max(max_width, width);
    }
    std::vector<uint32_t> slot(n_wires, 0xffffffffu);
    for (size_t w = 0; w < n_inputs; ++w) slot[w] = (uint32_t)w;
    for (size_t i = 0; i < order.size(); ++i) slot[n_inputs + order[i]] = (uint32_t)(n_inputs + i);

    // the core
    std::vector<uint32_t> first_wire(n_gates + 1);
    for (size_t g = 0; g <= n_gates; ++g) first_wire[g] = (uint32_t)(n_inputs + g);
    fhe::NetlistLevels L;
    fhe::netlist_levels(first_wire.data(), n_gates, D.outputs.data(), D.outputs.size(), [&](size_t g, auto &&f) { f(D.in0[g]); f(D.in1[g]); }, &L);
    REQUIRE(L.wire_live == live && L.level_of_node == level_of && L.level_start == level_start && L.source == order);
    REQUIRE(L.n_levels == n_levels && L.max_width == max_width && L.node_live.size() == n_gates);
    for (size_t g = 0; g < n_gates; ++g) REQUIRE(L.node_live[g] == live[n_inputs + g]);

    // FHEW: a random two-input op, free inversions on inputs and outputs
    std::vector<fhe_fhew_gate> gates(n_gates);
    std::vector<uint32_t> fo(D.outputs);
    for (size_t g = 0; g < n_gates; ++g) {
        gates[g] = fhe_fhew_gate{};
        gates[g].op = (uint8_t)rnd(FHE_GATE_MAJORITY);
        gates[g].in[0] = D.in0[g] | (rnd(2) ? FHE_WIRE_NOT : 0u);
        gates[g].in[1] = D.in1[g] | (rnd(2) ? FHE_WIRE_NOT : 0u);
    }
    for (uint32_t &w : fo) w |= rnd(2) ? FHE_WIRE_NOT : 0u;
    fhe::CircuitPlan F;
    REQUIRE(fhe::circuit_compile(gates.data(), n_gates, n_inputs, fo.data(), fo.size(), &F) == FHE_OK);
    // TFHE: one term per gate input, the gate's index as the constant
    std::vector<fhe_tfhe_node> nodes(n_gates);
    std::vector<fhe_tfhe_term> terms;
    for (size_t g = 0; g < n_gates; ++g) {
        nodes[g] = fhe_tfhe_node{};
        nodes[g].first_term = (uint32_t)terms.size();
        nodes[g].n_terms = 2;
        nodes[g].constant = g;
        terms.push_back(fhe_tfhe_term{D.in0[g], 1});
        terms.push_back(fhe_tfhe_term{D.in1[g], -3});
    }
    fhe::TfheCircuitPlan T;
    REQUIRE(fhe::tfhe_circuit_compile(nodes.data(), n_gates, terms.data(), terms.size(), n_inputs, 1, D.outputs.data(), D.outputs.size(), &T) == FHE_OK);

    // the same levels in both plans
    REQUIRE(F.level_of_gate == level_of && T.level_of_node == level_of);
    REQUIRE(F.level_start == level_start && T.level_start == level_start);
    REQUIRE(F.n_levels == n_levels && T.n_levels == n_levels && F.max_width == max_width && T.max_width == max_width);
    REQUIRE(F.n_live == order.size() && T.n_live == order.size() && F.gates.size() == order.size() && T.nodes.size() == order.size());
    // the same live-node order: plan entry i is gate order[i], its wires renumbered into slots
    auto to_slot = [&](uint32_t ref) { return slot[ref & ~FHE_WIRE_NOT] | (ref & FHE_WIRE_NOT); };
    REQUIRE(T.terms.size() == 2 * order.size());
    for (size_t i = 0; i < order.size(); ++i) {
        const uint32_t g = order[i];
        REQUIRE(F.gates[i].op == gates[g].op && F.gates[i].in[0] == to_slot(gates[g].in[0]) && F.gates[i].in[1] == to_slot(gates[g].in[1]));
        REQUIRE(T.nodes[i].constant == g && T.nodes[i].first_term == 2 * i && T.nodes[i].n_terms == 2);
        REQUIRE(T.terms[2 * i].wire == slot[D.in0[g]] && T.terms[2 * i + 1].wire == slot[D.in1[g]] && T.terms[2 * i + 1].weight == -3);
        REQUIRE(slot[D.in0[g]] < n_inputs + level_start[level_of[g] - 1] && slot[D.in1[g]] < n_inputs + level_start[level_of[g] - 1]);  // a lower level
    }
    for (size_t o = 0; o < D.outputs.size(); ++o) REQUIRE(F.outputs[o] == to_slot(fo[o]) && T.outputs[o] == slot[D.outputs[o]]);
    return 0;
}

int main() {
    for (int it = 0; it < 200; ++it) {
        const size_t n_gates = it < 4 ? it : rnd(201);  // 0, 1, 2, 3 gates, then up to 200
        if (check(random_dag(1 + rnd(40), n_gates, 1 + rnd(6), it % 3 == 1, it % 10 == 9))) return 1;
    }
    if (check(random_dag(40, 200, 12, true, false)) || check(random_dag(40, 200, 1, false, false))) return 1;
    std::printf("netlist_levels_host_test ok\n");
    return 0;
}
