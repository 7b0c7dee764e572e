// The netlist compiler behind fhe_tfhe_circuit_create: plain host C++ (no HIP), so that it also builds into a stand-alone program.
// A netlist of look-up-table nodes -- node g = bootstrap(tables[table], constant + sum weight * wire), the pattern of
// scheme/tfhe/src/bootstrapping.rs:118-165 over the free TLWE arithmetic of tlwe.rs:22-75 -- is validated, pruned to the nodes an output
// depends on, levelled (level = 1 + max level of the inputs, inputs at level 0) and renumbered into SLOTS: slot s < n_inputs is input s,
// slot n_inputs + i the i-th live node in level order (ties keep the netlist's order), so the nodes of one level write one contiguous
// run of the wire table.  The terms of the live nodes are repacked in the same order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/fhe_ring.h"

namespace fhe {

constexpr size_t TFHE_CIRCUIT_MAX_WIRES = size_t(1) << 24;
constexpr size_t TFHE_CIRCUIT_MAX_TABLES = 65536;
constexpr uint32_t TFHE_NODE_MAX_TERMS = 16;

struct TfheCircuitPlan {
    size_t n_inputs = 0, n_nodes = 0, n_outputs = 0, n_tables = 0;
    size_t n_levels = 0, n_live = 0, max_width = 0;
    std::vector<uint32_t> level_of_node;  // [n_nodes], 0 = dead
    std::vector<uint32_t> level_start;    // [n_levels + 1]: live nodes level_start[l] .. level_start[l + 1] - 1 form level l + 1
    std::vector<fhe_tfhe_node> nodes;     // [n_live], level order; first_term indexes `terms` below
    std::vector<fhe_tfhe_term> terms;     // the live nodes' terms, node after node; wire = slot
    std::vector<uint32_t> outputs;        // [n_outputs] slots
};

inline int tfhe_circuit_compile(const fhe_tfhe_node *nodes, size_t n_nodes, const fhe_tfhe_term *terms, size_t n_terms, size_t n_inputs,
                                size_t n_tables, const uint32_t *outputs, size_t n_outputs, TfheCircuitPlan *plan) {
    if (!plan || !outputs || n_outputs == 0 || n_inputs == 0 || (!nodes && n_nodes) || (!terms && n_terms)) return FHE_ERR_INVALID;
    if (n_inputs > TFHE_CIRCUIT_MAX_WIRES || n_nodes > TFHE_CIRCUIT_MAX_WIRES || n_inputs + n_nodes > TFHE_CIRCUIT_MAX_WIRES) return FHE_ERR_INVALID;
    if (n_outputs > 0xffffffffull || n_tables > TFHE_CIRCUIT_MAX_TABLES) return FHE_ERR_INVALID;
    const size_t n_wires = n_inputs + n_nodes;
    for (size_t g = 0; g < n_nodes; ++g) {
        const fhe_tfhe_node &nd = nodes[g];
        if (nd.n_terms == 0 || nd.n_terms > TFHE_NODE_MAX_TERMS) return FHE_ERR_INVALID;
        if (nd.first_term > n_terms || nd.n_terms > n_terms - nd.first_term) return FHE_ERR_INVALID;  // a term range outside terms
        if (nd.table >= n_tables) return FHE_ERR_INVALID;
        for (uint32_t k = 0; k < nd.n_terms; ++k) {
            const fhe_tfhe_term &tm = terms[nd.first_term + k];
            if (tm.wire >= n_inputs + g) return FHE_ERR_INVALID;  // forward (or out-of-range) reference
            if (tm.weight == 0) return FHE_ERR_INVALID;
        }
    }
    for (size_t o = 0; o < n_outputs; ++o)
        if (outputs[o] >= n_wires) return FHE_ERR_INVALID;
    // liveness: backwards from the outputs (a node only reads lower wires)
    std::vector<unsigned char> live(n_wires, 0);
    for (size_t o = 0; o < n_outputs; ++o) live[outputs[o]] = 1;
    for (size_t g = n_nodes; g-- > 0;) {
        if (!live[n_inputs + g]) continue;
        for (uint32_t k = 0; k < nodes[g].n_terms; ++k) live[terms[nodes[g].first_term + k].wire] = 1;
    }
    // levels: forwards
    std::vector<uint32_t> level(n_wires, 0);
    plan->level_of_node.assign(n_nodes, 0);
    uint32_t n_levels = 0;
    size_t live_terms = 0;
    for (size_t g = 0; g < n_nodes; ++g) {
        if (!live[n_inputs + g]) continue;
        uint32_t lv = 0;
        for (uint32_t k = 0; k < nodes[g].n_terms; ++k) {
            const uint32_t l = level[terms[nodes[g].first_term + k].wire];
            if (l > lv) lv = l;
        }
        level[n_inputs + g] = plan->level_of_node[g] = lv + 1;
        if (lv + 1 > n_levels) n_levels = lv + 1;
        live_terms += nodes[g].n_terms;
    }
    // slots: a counting sort of the live nodes by level
    plan->level_start.assign(size_t(n_levels) + 1, 0);
    for (size_t g = 0; g < n_nodes; ++g)
        if (plan->level_of_node[g]) ++plan->level_start[plan->level_of_node[g]];
    size_t max_width = 0;
    for (uint32_t l = 1; l <= n_levels; ++l) {
        if (plan->level_start[l] > max_width) max_width = plan->level_start[l];
        plan->level_start[l] += plan->level_start[l - 1];
    }
    const size_t n_live = plan->level_start[n_levels];
    std::vector<uint32_t> slot(n_wires, 0), next(plan->level_start.begin(), plan->level_start.end());
    for (size_t w = 0; w < n_inputs; ++w) slot[w] = (uint32_t)w;
    std::vector<uint32_t> source(n_live, 0);  // live node in slot order -> netlist index
    for (size_t g = 0; g < n_nodes; ++g) {
        if (!plan->level_of_node[g]) continue;
        const uint32_t i = next[plan->level_of_node[g] - 1]++;
        slot[n_inputs + g] = (uint32_t)(n_inputs + i);
        source[i] = (uint32_t)g;
    }
    plan->nodes.assign(n_live, fhe_tfhe_node{});
    plan->terms.clear();
    plan->terms.reserve(live_terms);
    for (size_t i = 0; i < n_live; ++i) {
        const fhe_tfhe_node &nd = nodes[source[i]];
        fhe_tfhe_node &out = plan->nodes[i];
        out.first_term = (uint32_t)plan->terms.size();
        out.n_terms = nd.n_terms;
        out.constant = nd.constant;
        out.table = nd.table;
        out.pad = 0;
        for (uint32_t k = 0; k < nd.n_terms; ++k) {
            const fhe_tfhe_term &tm = terms[nd.first_term + k];
            plan->terms.push_back(fhe_tfhe_term{slot[tm.wire], tm.weight});
        }
    }
    plan->outputs.resize(n_outputs);
    for (size_t o = 0; o < n_outputs; ++o) plan->outputs[o] = slot[outputs[o]];
    plan->n_inputs = n_inputs; plan->n_nodes = n_nodes; plan->n_outputs = n_outputs; plan->n_tables = n_tables;
    plan->n_levels = n_levels; plan->n_live = n_live; plan->max_width = max_width;
    return FHE_OK;
}

}  // namespace fhe
