// The netlist compiler behind fhe_tfhe_circuit_create and fhe_tfhe_circuit_create_many: plain host C++ (no HIP), so that it also builds
// into a stand-alone program.
// A netlist of look-up-table nodes -- node g = bootstrap(tables[table], constant + sum weight * wire), the pattern of
// scheme/tfhe/src/bootstrapping.rs:118-165 over the free TLWE arithmetic of tlwe.rs:22-75 -- is validated, pruned to the nodes an output
// depends on and levelled (netlist_levels.hpp: level = 1 + max level of the inputs, inputs at level 0), then renumbered into SLOTS:
// slot s < n_inputs is input s, slot n_inputs + i the i-th live node in level order (ties keep the netlist's order), so the nodes of
// one level write one contiguous run of the wire table.  The terms of the live nodes are repacked in the same order.
//
// Many-LUT nodes (tfhe_circuit_compile_many): a node with log_funcs = v > 0 is ONE blind rotation of a test polynomial that interleaves
// 2^v tables and owns 2^v consecutive wires, output i = sample_extract(acc, i) (tglwe.rs:115-127).  Liveness is per OUTPUT: a node is
// live when any of its outputs is, and only live outputs get a slot -- slot n_inputs + s, s counting the live outputs in level order,
// node after node, output index ascending -- an extraction descriptor and (in the executor) a key-switch row.  With every log_funcs == 0
// an output is a node, s = i, and the plan is that of tfhe_circuit_compile.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/fhe_ring.h"
#include "netlist_levels.hpp"

namespace fhe {

constexpr size_t TFHE_CIRCUIT_MAX_WIRES = size_t(1) << 24;
constexpr size_t TFHE_CIRCUIT_MAX_TABLES = 65536;
constexpr uint32_t TFHE_NODE_MAX_TERMS = 16;
constexpr uint32_t TFHE_MAX_LOG_FUNCS = 4;

// one live output: sample_extract(accumulator of live node `node` (level order), `index`)
struct TfheExtract {
    uint32_t node, index;
};

struct TfheCircuitPlan {
    size_t n_inputs = 0, n_nodes = 0, n_outputs = 0, n_tables = 0;
    size_t n_levels = 0, n_live = 0, max_width = 0;
    std::vector<uint32_t> level_of_node;  // [n_nodes], 0 = dead
    std::vector<uint32_t> level_start;    // [n_levels + 1]: live nodes level_start[l] .. level_start[l + 1] - 1 form level l + 1
    std::vector<fhe_tfhe_node> nodes;     // [n_live], level order; first_term indexes `terms` below; pad = log_funcs
    std::vector<fhe_tfhe_term> terms;     // the live nodes' terms, node after node; wire = slot
    std::vector<uint32_t> outputs;        // [n_outputs] slots
    // live outputs (for a plan of tfhe_circuit_compile: n_slots = n_live, out_start[i] = i, extracts[i] = {i, 0}, max_rows = max_width)
    bool many = false;                    // some live or dead node has log_funcs > 0
    size_t n_slots = 0, max_rows = 0;     // live outputs; those of the level that has most
    std::vector<uint32_t> out_start;      // [n_live + 1]: live node i owns slots n_inputs + out_start[i] .. n_inputs + out_start[i + 1] - 1
    std::vector<TfheExtract> extracts;    // [n_slots], slot order: the level's extraction descriptors are those of its nodes' slots
};

// The stream-ordered scratch of every composition "mod switch (or level front) -> blind rotation -> sample extraction -> key switch":
// fhe_tfhe_bootstrap, _tables and _many, fhe_tfhe_circuit_run and fhe_tfhe_circuit_bootstrap.  Offsets in 64-bit words from a base that
// is 16-byte aligned.  THE LAYOUT RULE: the [..][n] arrays come first, so that each starts on an even word (n is even) and the kernels
// may use 16-byte accesses on them; the rest follows in the order the steps touch it.
//   acc.a, acc.b [jobs][n] | extracted a [rows][n] | wire table a [wt_rows][n_lwe] | a~ [jobs][n_lwe] | wire table b [wt_rows] |
//   b~ [jobs] | extracted b [rows] | table_of [jobs] (32-bit, two to a word; only with `table`)
// jobs: blind rotations of the widest step; rows: extracted TLWEs of the widest step; wt_rows: rows of a circuit's wire table (else 0).
struct TfheScratch {
    size_t acc_a, acc_b, ext_a, wt_a, at, wt_b, bt, ext_b, table_of, total;
    TfheScratch(size_t jobs, size_t rows, size_t n, size_t n_lwe, size_t wt_rows, bool table) {
        acc_a = 0;
        acc_b = acc_a + jobs * n;
        ext_a = acc_b + jobs * n;
        wt_a = ext_a + rows * n;
        at = wt_a + wt_rows * n_lwe;
        wt_b = at + jobs * n_lwe;
        bt = wt_b + wt_rows;
        ext_b = bt + jobs;
        table_of = ext_b + rows;
        total = table_of + (table ? (jobs + 1) / 2 : 0);
    }
};

namespace detail {

// `many`: the node's fourth 32-bit field is log_funcs; otherwise it is ignored (every node has one output)
inline int tfhe_circuit_compile_any(const fhe_tfhe_node *nodes, size_t n_nodes, const fhe_tfhe_term *terms, size_t n_terms, size_t n_inputs,
                                    size_t n_tables, const uint32_t *outputs, size_t n_outputs, bool many, TfheCircuitPlan *plan) {
    if (!plan || !outputs || n_outputs == 0 || n_inputs == 0 || (!nodes && n_nodes) || (!terms && n_terms)) return FHE_ERR_INVALID;
    if (n_inputs > TFHE_CIRCUIT_MAX_WIRES || n_nodes > TFHE_CIRCUIT_MAX_WIRES || n_inputs + n_nodes > TFHE_CIRCUIT_MAX_WIRES) return FHE_ERR_INVALID;
    if (n_outputs > 0xffffffffull || n_tables > TFHE_CIRCUIT_MAX_TABLES) return FHE_ERR_INVALID;
    // first_wire[g]: the wire of node g's output 0; first_wire[n_nodes] = number of wires
    std::vector<uint32_t> first_wire(n_nodes + 1, 0);
    bool any_many = false;
    size_t n_wires = n_inputs;
    for (size_t g = 0; g < n_nodes; ++g) {
        const fhe_tfhe_node &nd = nodes[g];
        const uint32_t lf = many ? nd.pad : 0;
        if (lf > TFHE_MAX_LOG_FUNCS) return FHE_ERR_INVALID;
        any_many |= lf != 0;
        first_wire[g] = (uint32_t)n_wires;
        if (nd.n_terms == 0 || nd.n_terms > TFHE_NODE_MAX_TERMS) return FHE_ERR_INVALID;
        if (nd.first_term > n_terms || nd.n_terms > n_terms - nd.first_term) return FHE_ERR_INVALID;  // a term range outside terms
        if (nd.table >= n_tables) return FHE_ERR_INVALID;
        for (uint32_t k = 0; k < nd.n_terms; ++k) {
            const fhe_tfhe_term &tm = terms[nd.first_term + k];
            if (tm.wire >= n_wires) return FHE_ERR_INVALID;  // forward (or out-of-range) reference: at or above the node's own first wire
            if (tm.weight == 0) return FHE_ERR_INVALID;
        }
        n_wires += size_t(1) << lf;
        if (n_wires > TFHE_CIRCUIT_MAX_WIRES) return FHE_ERR_INVALID;  // the cap counts output wires
    }
    first_wire[n_nodes] = (uint32_t)n_wires;
    for (size_t o = 0; o < n_outputs; ++o)
        if (outputs[o] >= n_wires) return FHE_ERR_INVALID;
    // pruning and levels (netlist_levels.hpp): a node is live when any of its outputs is, every output carries the node's level
    NetlistLevels L;
    netlist_levels(first_wire.data(), n_nodes, outputs, n_outputs, [&](size_t g, auto &&f) {
        for (uint32_t k = 0; k < nodes[g].n_terms; ++k) f(terms[nodes[g].first_term + k].wire);
    }, &L);
    const std::vector<uint32_t> &source = L.source;
    const size_t n_live = source.size();
    // slots: the live outputs of the live nodes, in that order
    std::vector<uint32_t> slot(n_wires, 0xffffffffu);
    for (size_t w = 0; w < n_inputs; ++w) slot[w] = (uint32_t)w;
    plan->out_start.assign(n_live + 1, 0);
    plan->extracts.clear();
    size_t max_rows = 0, level_rows = 0;
    for (size_t i = 0, l = 0; i < n_live; ++i) {
        const uint32_t g = source[i];
        while (i == L.level_start[l + 1]) { ++l; level_rows = 0; }
        plan->out_start[i] = (uint32_t)plan->extracts.size();
        for (uint32_t w = first_wire[g]; w < first_wire[g + 1]; ++w) {
            if (!L.wire_live[w]) continue;
            slot[w] = (uint32_t)(n_inputs + plan->extracts.size());
            plan->extracts.push_back(TfheExtract{(uint32_t)i, w - first_wire[g]});
            ++level_rows;
        }
        if (level_rows > max_rows) max_rows = level_rows;
    }
    plan->out_start[n_live] = (uint32_t)plan->extracts.size();
    plan->nodes.assign(n_live, fhe_tfhe_node{});
    plan->terms.clear();
    for (size_t i = 0; i < n_live; ++i) {
        const fhe_tfhe_node &nd = nodes[source[i]];
        fhe_tfhe_node &out = plan->nodes[i];
        out.first_term = (uint32_t)plan->terms.size();
        out.n_terms = nd.n_terms;
        out.constant = nd.constant;
        out.table = nd.table;
        out.pad = many ? nd.pad : 0;
        for (uint32_t k = 0; k < nd.n_terms; ++k) {
            const fhe_tfhe_term &tm = terms[nd.first_term + k];
            plan->terms.push_back(fhe_tfhe_term{slot[tm.wire], tm.weight});
        }
    }
    plan->outputs.resize(n_outputs);
    for (size_t o = 0; o < n_outputs; ++o) plan->outputs[o] = slot[outputs[o]];
    plan->n_inputs = n_inputs; plan->n_nodes = n_nodes; plan->n_outputs = n_outputs; plan->n_tables = n_tables;
    plan->n_levels = L.n_levels; plan->n_live = n_live; plan->max_width = L.max_width;
    plan->many = any_many; plan->n_slots = plan->extracts.size(); plan->max_rows = max_rows;
    plan->level_of_node = std::move(L.level_of_node);
    plan->level_start = std::move(L.level_start);
    return FHE_OK;
}

}  // namespace detail

inline int tfhe_circuit_compile(const fhe_tfhe_node *nodes, size_t n_nodes, const fhe_tfhe_term *terms, size_t n_terms, size_t n_inputs,
                                size_t n_tables, const uint32_t *outputs, size_t n_outputs, TfheCircuitPlan *plan) {
    return detail::tfhe_circuit_compile_any(nodes, n_nodes, terms, n_terms, n_inputs, n_tables, outputs, n_outputs, false, plan);
}

// The same with the node's fourth 32-bit field (`pad`, fhe_tfhe_node_many's `log_funcs`) read as log_funcs <= 4: node g owns 2^log_funcs
// consecutive wires, the wire of (g, i) is n_inputs + sum_{h < g} 2^log_funcs_h + i.  Further rejections: log_funcs > 4; the cap of
// 2^24 wires counts output wires.
inline int tfhe_circuit_compile_many(const fhe_tfhe_node *nodes, size_t n_nodes, const fhe_tfhe_term *terms, size_t n_terms, size_t n_inputs,
                                     size_t n_tables, const uint32_t *outputs, size_t n_outputs, TfheCircuitPlan *plan) {
    return detail::tfhe_circuit_compile_any(nodes, n_nodes, terms, n_terms, n_inputs, n_tables, outputs, n_outputs, true, plan);
}

}  // namespace fhe
