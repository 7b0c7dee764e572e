// The netlist compiler behind fhe_fhew_circuit_create: plain host C++ (no HIP), so that it also builds into a stand-alone program.
// A netlist of `Fhew` gates (scheme/fhew/src/fhew.rs:59-67) with free inversions (fhew.rs:27-29) is validated, pruned to the gates an
// output depends on and levelled (netlist_levels.hpp: level = 1 + max level of the inputs, inputs at level 0), then renumbered into
// SLOTS: slot s < n_inputs is input s, slot n_inputs + i the i-th live gate in level order (ties keep the netlist's order), so the gates
// of one level write one contiguous run of the wire table.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/fhe_ring.h"
#include "netlist_levels.hpp"

namespace fhe {

constexpr size_t CIRCUIT_MAX_WIRES = size_t(1) << 24;
constexpr uint32_t WIRE_INDEX_MASK = ~uint32_t(FHE_WIRE_NOT);

// one live gate as the front kernel reads it (16 bytes): in[] are slots, FHE_WIRE_NOT kept on each
struct CircuitGate {
    uint32_t op;
    uint32_t in[3];
};

struct CircuitPlan {
    size_t n_inputs = 0, n_gates = 0, n_outputs = 0;
    size_t n_levels = 0, n_live = 0, max_width = 0;
    std::vector<uint32_t> level_of_gate;  // [n_gates], 0 = dead
    std::vector<uint32_t> level_start;    // [n_levels + 1]: live gates level_start[l] .. level_start[l + 1] - 1 form level l + 1
    std::vector<CircuitGate> gates;       // [n_live], level order
    std::vector<uint32_t> outputs;        // [n_outputs] slots, FHE_WIRE_NOT kept
};

inline int gate_arity(unsigned op) { return op == FHE_GATE_MAJORITY ? 3 : 2; }

inline int circuit_compile(const fhe_fhew_gate *gates, size_t n_gates, size_t n_inputs, const uint32_t *outputs, size_t n_outputs,
                           CircuitPlan *plan) {
    if (!plan || !outputs || n_outputs == 0 || n_inputs == 0 || (!gates && n_gates)) return FHE_ERR_INVALID;
    if (n_inputs > CIRCUIT_MAX_WIRES || n_gates > CIRCUIT_MAX_WIRES || n_inputs + n_gates > CIRCUIT_MAX_WIRES) return FHE_ERR_INVALID;
    if (n_outputs > 0xffffffffull) return FHE_ERR_INVALID;
    const size_t n_wires = n_inputs + n_gates;
    for (size_t g = 0; g < n_gates; ++g) {
        if (gates[g].op > FHE_GATE_MAJORITY) return FHE_ERR_INVALID;
        for (int k = 0; k < gate_arity(gates[g].op); ++k)
            if ((gates[g].in[k] & WIRE_INDEX_MASK) >= n_inputs + g) return FHE_ERR_INVALID;  // forward (or out-of-range) reference
    }
    for (size_t o = 0; o < n_outputs; ++o)
        if ((outputs[o] & WIRE_INDEX_MASK) >= n_wires) return FHE_ERR_INVALID;
    // pruning and levels (netlist_levels.hpp): a gate owns one wire
    std::vector<uint32_t> first_wire(n_gates + 1), out_wires(n_outputs);
    for (size_t g = 0; g <= n_gates; ++g) first_wire[g] = (uint32_t)(n_inputs + g);
    for (size_t o = 0; o < n_outputs; ++o) out_wires[o] = outputs[o] & WIRE_INDEX_MASK;
    NetlistLevels L;
    netlist_levels(first_wire.data(), n_gates, out_wires.data(), n_outputs, [&](size_t g, auto &&f) {
        for (int k = 0; k < gate_arity(gates[g].op); ++k) f(gates[g].in[k] & WIRE_INDEX_MASK);
    }, &L);
    // slots: the live gates in level order
    const size_t n_live = L.source.size();
    std::vector<uint32_t> slot(n_wires, 0);
    for (size_t w = 0; w < n_inputs; ++w) slot[w] = (uint32_t)w;
    for (size_t i = 0; i < n_live; ++i) slot[n_inputs + L.source[i]] = (uint32_t)(n_inputs + i);
    auto to_slot = [&](uint32_t ref) { return slot[ref & WIRE_INDEX_MASK] | (ref & FHE_WIRE_NOT); };
    plan->gates.assign(n_live, CircuitGate{});
    for (size_t i = 0; i < n_live; ++i) {
        const fhe_fhew_gate &gt = gates[L.source[i]];
        plan->gates[i].op = gt.op;
        for (int k = 0; k < 3; ++k) plan->gates[i].in[k] = k < gate_arity(gt.op) ? to_slot(gt.in[k]) : 0u;
    }
    plan->outputs.resize(n_outputs);
    for (size_t o = 0; o < n_outputs; ++o) plan->outputs[o] = to_slot(outputs[o]);
    plan->n_inputs = n_inputs; plan->n_gates = n_gates; plan->n_outputs = n_outputs;
    plan->n_levels = L.n_levels; plan->n_live = n_live; plan->max_width = L.max_width;
    plan->level_of_gate = std::move(L.level_of_node);
    plan->level_start = std::move(L.level_start);
    return FHE_OK;
}

}  // namespace fhe
