// Kernels of the TFHE circuit executor (tfhe_circuit_api.hip): the FRONT of a level -- what the node-by-node route spends one
// fhe_tlwe_lincomb launch and two mod-switch launches on, for every node of the level and every ciphertext of the batch in one launch --
// and the copy of the outputs out of the wire table.
//
// Wire table: slot s < n_inputs is the caller's input s (read where it lies), slot n_inputs + i is live output i (level order; a node
// without many-LUT outputs has one) in the call's workspace; a slot holds a [batch][n_lwe] and b [batch].  Job m = node * batch + batch
// index of a level is the unit the front and the blind rotation see; the extraction turns jobs into rows, one per live output and batch
// index, so the key switch writes the level's slots as one [rows][n_lwe].
//
// Both kernels are element-wise and memory bound.  ONE WAVE owns a job at a time: its node descriptor and term list are the same for all
// 64 lanes (the job index goes through readfirstlane, so descriptors and terms are scalar loads and the term loop is uniform), and the
// lanes walk the n_lwe + 1 words of the job (index n_lwe = the b word) with consecutive lanes on consecutive words of every term.
#pragma once
#include <algorithm>

#include "arith.hpp"
#include "dispatch.hpp"  // launch(), with_bool()
#include "tfhe_circuit.hpp"
#include "torus_kernels.hpp"  // tglwe_sample_extract_kernel

namespace fhe {

struct TfheWires {
    const u64 *in_a, *in_b;  // slots < n_inputs: [n_inputs][batch][n_lwe], [n_inputs][batch]
    const u64 *wt_a, *wt_b;  // slots >= n_inputs: [n_live][batch][n_lwe], [n_live][batch] (with many-LUT nodes: a row per live OUTPUT)
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

// Level front.  nodes: the level's descriptors [width] (first_term indexes `terms`, the circuit's whole term list; wire = slot;
// pad = log_funcs of the node, scalar and uniform per wave); jobs = width * batch.  Out, per job m: a1 [m][n_lwe], b1 [m] = `mod_switch`
// to multiples of 2^log_funcs (torus_rounding_shr_many_kernel below; log_funcs = 0: bootstrapping.rs:99-104, the sequence of
// torus_rounding_shr_kernel) of constant + sum weight * wire mod 2^64 (constant on b only), table_of [m] = the node's table.
FHE_HEADER_KERNEL __launch_bounds__(256) void tfhe_circuit_front_kernel(TfheWires W, const fhe_tfhe_node *__restrict__ nodes, const fhe_tfhe_term *__restrict__ terms,
                                                                 unsigned width, int bits, u64 *__restrict__ a1, u64 *__restrict__ b1,
                                                                 unsigned *__restrict__ table_of) {
    const size_t jobs = size_t(width) * W.batch;
    const unsigned lane = threadIdx.x & 63u, waves_per_block = blockDim.x >> 6;
    const size_t first = size_t(blockIdx.x) * waves_per_block + (threadIdx.x >> 6), step = size_t(gridDim.x) * waves_per_block;
    for (size_t job = first; job < jobs; job += step) {
        const unsigned m = __builtin_amdgcn_readfirstlane(unsigned(job));  // jobs < 2^31 (checked by the entry point)
        const unsigned node = m / W.batch, bi = m - node * W.batch;
        const fhe_tfhe_node nd = nodes[node];
        const fhe_tfhe_term *tm = terms + nd.first_term;
        const int nu = int(nd.pad), sh = bits + nu;  // nu <= 4 (checked by create): sh <= 59
        const u64 half = (u64(1) << sh) >> 1;
        for (unsigned j = lane; j <= W.n_lwe; j += 64) {
            const bool is_b = j == W.n_lwe;
            u64 acc = is_b ? nd.constant : 0;
            for (unsigned k = 0; k < nd.n_terms; ++k) {
                const unsigned slot = tm[k].wire;
                const u64 x = is_b ? *tfhe_wire_b(W, slot, bi) : tfhe_wire_a(W, slot, bi)[j];
                acc += u64(int64_t(tm[k].weight)) * x;
            }
            const u64 sw = ((acc + half) >> sh) << nu;
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

// ---- many-LUT nodes (PBSmanyLUT: one blind rotation serves 2^v functions) ----------------------------------------------------------

// `mod_switch` (bootstrapping.rs:99-104) to multiples of 2^nu: rounding_shr by bits + nu, then << nu -- the reference's mod_switch for
// big_n >> nu, shifted left; nu = 0 is torus_rounding_shr_kernel.  bits + nu <= 63 (checked by the entry point).
FHE_HEADER_KERNEL void torus_rounding_shr_many_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, size_t count, int bits, int nu) {
    const int sh = bits + nu;
    const u64 half = (u64(1) << sh) >> 1;
    for (size_t idx = blockIdx.x * size_t(blockDim.x) + threadIdx.x; idx < count; idx += size_t(gridDim.x) * blockDim.x)
        out[idx] = ((in[idx] + half) >> sh) << nu;
}

// scheme/tfhe/src/tglwe.rs:115-127 `sample_extract(acc, i)` (k = 1) for SEVERAL i of one accumulator.  Job m = node * batch + bi reads
// the accumulator acc_a [m][n], acc_b [m][n]; ONE WAVE owns a job: it stages the row a [n] in its own n words of LDS once (16-byte
// loads) and writes every extraction e of the node from there -- out_a [r][n], out_b [r], r = (e - base) * stride_e + bi * stride_b,
// the key switch's input layout -- as row[j] = a[i - j] for j <= i, -a[n + i - j] for j > i (two words per lane, 16-byte stores) and
// out_b [r] = b[i].
//   ext != null: node's extractions are ext[out_start[node] .. out_start[node + 1] - 1], i = ext[e].index  (out_start, ext: device)
//   ext == null: the dense list of one node (width = 1): e = i = 0 .. dense - 1, base = 0
// n a power of two >= 2; dynamic LDS = waves per block * n * 8 bytes.  The job loop is uniform per BLOCK (every wave of a block makes the
// same number of trips; a wave past the last job only keeps the barriers).  WIDE: acc_a and out_a are 16-byte aligned (the executor's
// workspace always is: TfheScratch); otherwise the same words go as 8-byte accesses.
template <bool WIDE>
__global__ __launch_bounds__(256) void tglwe_sample_extract_many_kernel(const u64 *__restrict__ acc_a, const u64 *__restrict__ acc_b, unsigned n,
                                                                        unsigned width, unsigned batch, const unsigned *__restrict__ out_start,
                                                                        const TfheExtract *__restrict__ ext, unsigned base, unsigned dense,
                                                                        size_t stride_e, size_t stride_b, u64 *__restrict__ out_a,
                                                                        u64 *__restrict__ out_b) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves_per_block = blockDim.x >> 6;
    u64 *row = reinterpret_cast<u64 *>(smem_raw) + size_t(wave) * n;
    const size_t jobs = size_t(width) * batch;
    for (size_t job0 = size_t(blockIdx.x) * waves_per_block; job0 < jobs; job0 += size_t(gridDim.x) * waves_per_block) {
        const unsigned m = __builtin_amdgcn_readfirstlane(unsigned(job0 + wave));  // jobs < 2^31 (checked by the entry point)
        const bool active = m < jobs;
        if (active) {
            const u64 *src = acc_a + size_t(m) * n;
            for (unsigned t = lane; t < n / 2; t += 64) {
                ulonglong2 v;
                if constexpr (WIDE) v = reinterpret_cast<const ulonglong2 *>(src)[t];
                else { v.x = src[2 * t]; v.y = src[2 * t + 1]; }
                reinterpret_cast<ulonglong2 *>(row)[t] = v;
            }
        }
        __syncthreads();
        if (active) {
            const unsigned node = m / batch, bi = m - node * batch;
            const unsigned e0 = ext ? out_start[node] : 0u, e1 = ext ? out_start[node + 1] : dense;
            for (unsigned e = e0; e < e1; ++e) {
                const unsigned i = ext ? ext[e].index : e;
                const size_t r = size_t(e - base) * stride_e + size_t(bi) * stride_b;
                u64 *dst = out_a + r * n;
                for (unsigned t = lane; t < n / 2; t += 64) {
                    const unsigned j0 = 2 * t, j1 = j0 + 1;
                    ulonglong2 v;
                    v.x = j0 <= i ? row[i - j0] : u64(0) - row[n + i - j0];
                    v.y = j1 <= i ? row[i - j1] : u64(0) - row[n + i - j1];
                    if constexpr (WIDE) reinterpret_cast<ulonglong2 *>(dst)[t] = v;
                    else { dst[j0] = v.x; dst[j1] = v.y; }
                }
                if (lane == 0) out_b[r] = acc_b[size_t(m) * n + i];
            }
        }
        __syncthreads();
    }
}

// Every launch of the kernel above: WAVES rows of n words in LDS per block (n <= 2048, checked by the entry points), a block per WAVES
// jobs up to a cap, WIDE where acc_a and out_a allow it.  index0: the caller states that every job has ONE extraction, of index 0, into
// row = job (a circuit level of one-output nodes): the element-wise kernel of fhe_tglwe_sample_extract writes the same rows and is what
// such levels ran before the executors became one; the measurement rule of DESIGN.md 9.1 kept it for them.
inline int launch_sample_extract_many(const u64 *acc_a, const u64 *acc_b, size_t n, size_t width, size_t batch, const unsigned *out_start,
                                      const TfheExtract *ext, size_t base, size_t dense, size_t stride_e, size_t stride_b, u64 *out_a, u64 *out_b,
                                      hipStream_t st, bool index0 = false) {
    if (index0) return launch<tglwe_sample_extract_kernel>(grid_for(n * width * batch), 256, 0, st, acc_a, acc_b, (unsigned)n, width * batch, 0u, out_a, out_b);
    constexpr unsigned WAVES = 4;
    const unsigned grid = (unsigned)std::min<size_t>((width * batch + WAVES - 1) / WAVES, 8192);
    const bool wide = ((reinterpret_cast<uintptr_t>(acc_a) | reinterpret_cast<uintptr_t>(out_a)) & 15) == 0;
    return with_bool(wide, [&](auto w) {
        return launch<tglwe_sample_extract_many_kernel<decltype(w)::value>>(grid, 64 * WAVES, WAVES * n * sizeof(u64), st, acc_a, acc_b, (unsigned)n,
                                                                            (unsigned)width, (unsigned)batch, out_start, ext, (unsigned)base,
                                                                            (unsigned)dense, stride_e, stride_b, out_a, out_b);
    });
}

}  // namespace fhe
