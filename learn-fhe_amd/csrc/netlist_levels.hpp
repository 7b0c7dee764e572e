// What the FHEW and the TFHE netlist compilers (fhew_circuit.hpp, tfhe_circuit.hpp) share: plain host C++ (no HIP).
// A validated netlist -- wires 0 .. n_inputs - 1 are the inputs, node g owns the wires first_wire[g] .. first_wire[g + 1] - 1 and only
// reads lower ones -- is pruned to the nodes an output depends on and levelled: level = 1 + max level of the input wires, inputs at
// level 0, every wire of a node at the node's level.  The live nodes are then sorted by level; ties keep the netlist's order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fhe {

struct NetlistLevels {
    std::vector<unsigned char> wire_live;  // [n_wires]: an output, or read by a live node
    std::vector<unsigned char> node_live;  // [n_nodes]: owns a live wire
    std::vector<uint32_t> level_of_node;   // [n_nodes], 0 = dead
    std::vector<uint32_t> level_start;     // [n_levels + 1]: live nodes level_start[l] .. level_start[l + 1] - 1 (level order) form level l + 1
    std::vector<uint32_t> source;          // [n_live]: live node in level order -> netlist index
    size_t n_levels = 0, max_width = 0;
};

// first_wire [n_nodes + 1] (first_wire[0] = n_inputs, first_wire[n_nodes] = number of wires); outputs [n_outputs]: wires;
// inputs_of(g, f) calls f(wire) for every wire node g reads.  The caller has checked every range.
template <class InputsOf>
void netlist_levels(const uint32_t *first_wire, size_t n_nodes, const uint32_t *outputs, size_t n_outputs, InputsOf &&inputs_of, NetlistLevels *L) {
    const size_t n_wires = first_wire[n_nodes];
    // liveness: backwards from the outputs (a node only reads lower wires)
    L->wire_live.assign(n_wires, 0);
    for (size_t o = 0; o < n_outputs; ++o) L->wire_live[outputs[o]] = 1;
    L->node_live.assign(n_nodes, 0);
    for (size_t g = n_nodes; g-- > 0;) {
        for (uint32_t w = first_wire[g]; w < first_wire[g + 1]; ++w) L->node_live[g] |= L->wire_live[w];
        if (L->node_live[g]) inputs_of(g, [&](uint32_t w) { L->wire_live[w] = 1; });
    }
    // levels: forwards
    std::vector<uint32_t> level(n_wires, 0);
    L->level_of_node.assign(n_nodes, 0);
    uint32_t n_levels = 0;
    for (size_t g = 0; g < n_nodes; ++g) {
        if (!L->node_live[g]) continue;
        uint32_t lv = 0;
        inputs_of(g, [&](uint32_t w) { if (level[w] > lv) lv = level[w]; });
        L->level_of_node[g] = lv + 1;
        for (uint32_t w = first_wire[g]; w < first_wire[g + 1]; ++w) level[w] = lv + 1;
        if (lv + 1 > n_levels) n_levels = lv + 1;
    }
    // live nodes in level order: a counting sort by level
    L->level_start.assign(size_t(n_levels) + 1, 0);
    for (size_t g = 0; g < n_nodes; ++g)
        if (L->level_of_node[g]) ++L->level_start[L->level_of_node[g]];
    L->max_width = 0;
    for (uint32_t l = 1; l <= n_levels; ++l) {
        if (L->level_start[l] > L->max_width) L->max_width = L->level_start[l];
        L->level_start[l] += L->level_start[l - 1];
    }
    std::vector<uint32_t> next(L->level_start);
    L->source.assign(L->level_start[n_levels], 0);
    for (size_t g = 0; g < n_nodes; ++g)
        if (L->level_of_node[g]) L->source[next[L->level_of_node[g] - 1]++] = (uint32_t)g;
    L->n_levels = n_levels;
}

}  // namespace fhe
