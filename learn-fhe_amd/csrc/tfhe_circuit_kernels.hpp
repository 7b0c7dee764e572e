// Kernels of the TFHE circuit executor (tfhe_circuit_api.hip): the FRONT of a level -- what the node-by-node route spends one
// fhe_tlwe_lincomb launch and two mod-switch launches on, for every node of the level and every ciphertext of the batch in one launch --
// and the copy of the outputs out of the wire table.
//
// Wire table: slot s < n_inputs is the caller's input s (read where it lies), slot n_inputs + i is live node i (level order) in the
// call's workspace; a slot holds a [batch][n_lwe] and b [batch].  Job m = node * batch + batch index of a level is the unit every later
// launch of the level (blind rotation .. key switch) sees, so the key switch writes the level's slots as one [width * batch][n_lwe].
//
// Both kernels are element-wise and memory bound.  ONE WAVE owns a job at a time: its node descriptor and term list are the same for all
// 64 lanes (the job index goes through readfirstlane, so descriptors and terms are scalar loads and the term loop is uniform), and the
// lanes walk the n_lwe + 1 words of the job (index n_lwe = the b word) with consecutive lanes on consecutive words of every term.
#pragma once
#include "arith.hpp"
#include "tfhe_circuit.hpp"

namespace fhe {

struct TfheWires {
    const u64 *in_a, *in_b;  // slots < n_inputs: [n_inputs][batch][n_lwe], [n_inputs][batch]
    const u64 *wt_a, *wt_b;  // slots >= n_inputs: [n_live][batch][n_lwe], [n_live][batch]
    unsigned n_inputs;
    unsigned batch;
    unsigned n_lwe;
};

__device__ __forceinline__ const u64 *tfhe_wire_a(const TfheWires &W, unsigned slot, unsigned bi) {
    return slot < W.n_inputs ? W.in_a + (size_t(slot) * W.batch + bi) * W.n_lwe : W.wt_a + (size_t(slot - W.n_inputs) * W.batch + bi) * W.n_lwe;
}
__device__ __forceinline__ const u64 *tfhe_wire_b(const TfheWires &W, unsigned slot, unsigned bi) {
    return slot < W.n_inputs ? W.in_b + size_t(slot) * W.batch + bi : W.wt_b + size_t(slot - W.n_inputs) * W.batch + bi;
}

// Level front.  nodes: the level's descriptors [width] (first_term indexes `terms`, the circuit's whole term list; wire = slot);
// jobs = width * batch.  Out, per job m: a1 [m][n_lwe], b1 [m] = `mod_switch` (bootstrapping.rs:99-104: rounding_shr by `bits`, the
// sequence of torus_rounding_shr_kernel) of constant + sum weight * wire mod 2^64 (constant on b only), table_of [m] = the node's table.
FHE_HEADER_KERNEL __launch_bounds__(256) void tfhe_circuit_front_kernel(TfheWires W, const fhe_tfhe_node *__restrict__ nodes, const fhe_tfhe_term *__restrict__ terms,
                                                                 unsigned width, int bits, u64 *__restrict__ a1, u64 *__restrict__ b1,
                                                                 unsigned *__restrict__ table_of) {
    const size_t jobs = size_t(width) * W.batch;
    const unsigned lane = threadIdx.x & 63u, waves_per_block = blockDim.x >> 6;
    const size_t first = size_t(blockIdx.x) * waves_per_block + (threadIdx.x >> 6), step = size_t(gridDim.x) * waves_per_block;
    const u64 half = (u64(1) << bits) >> 1;
    for (size_t job = first; job < jobs; job += step) {
        const unsigned m = __builtin_amdgcn_readfirstlane(unsigned(job));  // jobs < 2^31 (checked by the entry point)
        const unsigned node = m / W.batch, bi = m - node * W.batch;
        const fhe_tfhe_node nd = nodes[node];
        const fhe_tfhe_term *tm = terms + nd.first_term;
        for (unsigned j = lane; j <= W.n_lwe; j += 64) {
            const bool is_b = j == W.n_lwe;
            u64 acc = is_b ? nd.constant : 0;
            for (unsigned k = 0; k < nd.n_terms; ++k) {
                const unsigned slot = tm[k].wire;
                const u64 x = is_b ? *tfhe_wire_b(W, slot, bi) : tfhe_wire_a(W, slot, bi)[j];
                acc += u64(int64_t(tm[k].weight)) * x;
            }
            const u64 sw = (acc + half) >> bits;
            if (is_b) b1[m] = sw;
            else a1[size_t(m) * W.n_lwe + j] = sw;
        }
        if (lane == 0) table_of[m] = nd.table;
    }
}

// outputs [n_outputs] slots -> out_a [n_outputs][batch][n_lwe], out_b [n_outputs][batch]; one wave per (output, batch index)
FHE_HEADER_KERNEL __launch_bounds__(256) void tfhe_circuit_output_kernel(TfheWires W, const unsigned *__restrict__ outputs, unsigned n_outputs,
                                                                  u64 *__restrict__ out_a, u64 *__restrict__ out_b) {
    const size_t jobs = size_t(n_outputs) * W.batch;
    const unsigned lane = threadIdx.x & 63u, waves_per_block = blockDim.x >> 6;
    const size_t first = size_t(blockIdx.x) * waves_per_block + (threadIdx.x >> 6), step = size_t(gridDim.x) * waves_per_block;
    for (size_t job = first; job < jobs; job += step) {
        const unsigned m = __builtin_amdgcn_readfirstlane(unsigned(job));
        const unsigned o = m / W.batch, bi = m - o * W.batch;
        const unsigned slot = outputs[o];
        const u64 *src = tfhe_wire_a(W, slot, bi);
        for (unsigned j = lane; j < W.n_lwe; j += 64) out_a[size_t(m) * W.n_lwe + j] = src[j];
        if (lane == 0) out_b[m] = *tfhe_wire_b(W, slot, bi);
    }
}

}  // namespace fhe
