// Kernels of the FHEW circuit executor (fhew_circuit_api.hip): the FRONT of a level -- what the gate-by-gate route spends two
// fhe_lwe_lincomb launches, a look-up polynomial and two mod-switch launches on, for every gate of the level and every ciphertext of
// the batch in one launch -- and the copy of the outputs out of the wire table.
//
// Wire table: slot s < n_inputs is the caller's input s (read where it lies), slot n_inputs + i is live gate i (level order) in the
// call's workspace; a slot holds a [batch][n] and b [batch].  Ciphertext m = gate * batch + batch index of a level is the unit every
// later launch of the level (key switch .. sample extract) sees, so the sample extract writes the level's slots as one [g * batch][n].
//
// Both kernels are element-wise and memory bound: a lane owns V consecutive coefficients of one ciphertext (V = 2: one 16-byte
// access per operand; V = 1 where n is odd-aligned or a caller's pointer is not 16-byte aligned), consecutive lanes consecutive
// coefficients, no LDS.  The gate descriptor (16 bytes) is the same for the batch * n / V consecutive items of a gate: one cached
// load, uniform across nearly every wave.
#pragma once
#include "fhew_circuit.hpp"
#include "fhew_kernels.hpp"

namespace fhe {

struct CircuitWires {
    const u64 *in_a, *in_b;  // slots < n_inputs: [n_inputs][batch][n], [n_inputs][batch]
    const u64 *wt_a, *wt_b;  // slots >= n_inputs: [n_live][batch][n], [n_live][batch]
    unsigned n_inputs;
    unsigned batch;
    unsigned log_n;
    u64 q;      // Q
    u64 q_by_4; // round(Q / 4): `Fhew::not` adds it to b (fhew.rs:27-29)
    u64 q_by_8; // round(Q / 8): the look-up values are +- this (fhew.rs:32)
};

__device__ __forceinline__ const u64 *wire_a(const CircuitWires &W, unsigned slot, unsigned bi) {
    const size_t n = size_t(1) << W.log_n;
    return slot < W.n_inputs ? W.in_a + (size_t(slot) * W.batch + bi) * n : W.wt_a + (size_t(slot - W.n_inputs) * W.batch + bi) * n;
}
__device__ __forceinline__ u64 wire_b(const CircuitWires &W, unsigned slot, unsigned bi) {
    return slot < W.n_inputs ? W.in_b[size_t(slot) * W.batch + bi] : W.wt_b[size_t(slot - W.n_inputs) * W.batch + bi];
}

// c * x mod q for the gate coefficients c = +-1, +-2 (x < q < 2^62)
__device__ __forceinline__ u64 gate_term(u64 x, bool twice, bool neg, u64 q) {
    if (twice) x = csub(x + x, q);
    return neg ? (x ? q - x : 0) : x;
}

// fhew.rs:59-67, the tables as 4-bit masks (bit r = the output of run r) and the linear parts: +1, +1 | +2, -2 | +1, +1, +1
__device__ __forceinline__ unsigned gate_table(unsigned op) {
    //                 and, nand, or, nor, xor, xnor, majority
    return (0x8u | 0x7u << 4 | 0xeu << 8 | 0x1u << 12 | 0xeu << 16 | 0x1u << 20 | 0x8u << 24) >> (4 * op) & 0xfu;
}

template <int V>
struct VecIo;
template <>
struct VecIo<1> {
    u64 v[1];
    __device__ __forceinline__ void load(const u64 *p) { v[0] = p[0]; }
    __device__ __forceinline__ void store(u64 *p) const { p[0] = v[0]; }
};
template <>
struct VecIo<2> {
    u64 v[2];
    __device__ __forceinline__ void load(const u64 *p) {
        const ulonglong2 t = *reinterpret_cast<const ulonglong2 *>(p);
        v[0] = t.x; v[1] = t.y;
    }
    __device__ __forceinline__ void store(u64 *p) const { *reinterpret_cast<ulonglong2 *>(p) = make_ulonglong2(v[0], v[1]); }
};

// Level front.  gates: the level's descriptors [g]; items = g * batch * n / V.  Out, per ciphertext m = gate * batch + bi:
// a1 [m][n], b1 [m] = mod_switch(q_ks) of the gate's linear combination over Q (zq_mod_switch: the sequence of lwe_mod_switch_kernel),
// lut [m][n] = the gate's look-up row (`Fhew::op`, fhew.rs:31-36: four runs of n / 4).
template <int V>
__global__ __launch_bounds__(256) void circuit_front_kernel(CircuitWires W, const CircuitGate *__restrict__ gates, unsigned n_level_gates,
                                                            u64 q_ks, u64 *__restrict__ a1, u64 *__restrict__ b1, u64 *__restrict__ lut) {
    const unsigned per_ct = (1u << W.log_n) / V;
    const size_t total = size_t(n_level_gates) * W.batch * per_ct;
    const u64 q = W.q;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const size_t m = idx / per_ct;
        const unsigned j = unsigned(idx - m * per_ct) * V;
        const unsigned gate = unsigned(m / W.batch), bi = unsigned(m - size_t(gate) * W.batch);
        const uint4 gd = *reinterpret_cast<const uint4 *>(gates + gate);  // op, in[0 .. 2]
        const unsigned op = gd.x, refs[3] = {gd.y, gd.z, gd.w};
        const bool sub = op == FHE_GATE_XOR || op == FHE_GATE_XNOR;  // (ct0 - ct1).double()
        const int k = op == FHE_GATE_MAJORITY ? 3 : 2;
        u64 acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0;
        u64 acc_b = 0;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            if (t >= k) break;
            const unsigned slot = refs[t] & WIRE_INDEX_MASK;
            const bool inv = (refs[t] & FHE_WIRE_NOT) != 0;
            const bool coef_neg = sub && t == 1;  // the gate's own coefficient; an inverted wire flips it
            VecIo<V> x;
            x.load(wire_a(W, slot, bi) + j);
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] = csub(acc[e] + gate_term(x.v[e], sub, coef_neg != inv, q), q);
            if (j == 0) {
                // not(ct) = (-a, -b + Q/4): coef * b' = -coef * b + coef * Q/4
                acc_b = csub(acc_b + gate_term(wire_b(W, slot, bi), sub, coef_neg != inv, q), q);
                if (inv) acc_b = csub(acc_b + gate_term(W.q_by_4, sub, coef_neg, q), q);
            }
        }
        VecIo<V> o, f;
        const unsigned table = gate_table(op);
        const u64 neg8 = q - W.q_by_8;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            o.v[e] = zq_mod_switch(acc[e], q, q_ks, false);
            f.v[e] = (table >> ((j + e) >> (W.log_n - 2)) & 1u) ? W.q_by_8 : neg8;
        }
        o.store(a1 + m * (size_t(1) << W.log_n) + j);
        f.store(lut + m * (size_t(1) << W.log_n) + j);
        if (j == 0) b1[m] = zq_mod_switch(acc_b, q, q_ks, false);
    }
}

// outputs [n_outputs] slots (FHE_WIRE_NOT: -a, -b + Q/4) -> out_a [n_outputs][batch][n], out_b [n_outputs][batch]
template <int V>
__global__ __launch_bounds__(256) void circuit_output_kernel(CircuitWires W, const unsigned *__restrict__ outputs, unsigned n_outputs,
                                                             u64 *__restrict__ out_a, u64 *__restrict__ out_b) {
    const unsigned per_ct = (1u << W.log_n) / V;
    const size_t total = size_t(n_outputs) * W.batch * per_ct;
    const u64 q = W.q;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < total; idx += size_t(gridDim.x) * blockDim.x) {
        const size_t m = idx / per_ct;
        const unsigned j = unsigned(idx - m * per_ct) * V;
        const unsigned o = unsigned(m / W.batch), bi = unsigned(m - size_t(o) * W.batch);
        const unsigned ref = outputs[o], slot = ref & WIRE_INDEX_MASK;
        const bool inv = (ref & FHE_WIRE_NOT) != 0;
        VecIo<V> x;
        x.load(wire_a(W, slot, bi) + j);
#pragma unroll
        for (int e = 0; e < V; ++e) x.v[e] = gate_term(x.v[e], false, inv, q);
        x.store(out_a + m * (size_t(1) << W.log_n) + j);
        if (j == 0) {
            const u64 b = wire_b(W, slot, bi);
            out_b[m] = inv ? csub(gate_term(b, false, true, q) + W.q_by_4, q) : b;
        }
    }
}

}  // namespace fhe
