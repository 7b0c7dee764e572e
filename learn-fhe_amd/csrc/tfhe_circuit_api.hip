// extern "C" entry points of the TFHE look-up-table circuits: a levelled netlist of programmable bootstraps
// (scheme/tfhe/src/bootstrapping.rs:78-82 through the tables of 118-128) over free TLWE arithmetic (tlwe.rs:22-75) -- what
// bootstrapping.rs:141-165 does one call after the other -- prepared once and run in one call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "api_common.hpp"
#include "tfhe_circuit.hpp"
#include "tfhe_circuit_kernels.hpp"
#include "torus_ctx.hpp"

struct fhe_tfhe_circuit {
    fhe::TfheCircuitPlan plan;
    // the plan as the kernels read it: nodes [n_live] | terms | outputs [n_outputs] | out_start [n_live + 1] | extracts [n_slots]
    mutable DeviceImage image;
};

static_assert(sizeof(fhe_tfhe_node_many) == sizeof(fhe_tfhe_node) && sizeof(fhe_tfhe_node) == 24, "a many-LUT node is the same 24 bytes");

extern "C" {

int fhe_tfhe_circuit_create(const fhe_tfhe_node *nodes, size_t n_nodes, const fhe_tfhe_term *terms, size_t n_terms, size_t n_inputs,
                            size_t n_tables, const uint32_t *outputs, size_t n_outputs, fhe_tfhe_circuit **out) {
    return create_handle(out, [&](fhe_tfhe_circuit *c) {
        return fhe::tfhe_circuit_compile(nodes, n_nodes, terms, n_terms, n_inputs, n_tables, outputs, n_outputs, &c->plan);
    });
}

// fhe_tfhe_circuit_create with many-LUT nodes (bootstrapping.rs:78-128, tglwe.rs:115-127): the node's fourth field is log_funcs
int fhe_tfhe_circuit_create_many(const fhe_tfhe_node *nodes, size_t n_nodes, const fhe_tfhe_term *terms, size_t n_terms, size_t n_inputs,
                                 size_t n_tables, const uint32_t *outputs, size_t n_outputs, fhe_tfhe_circuit **out) {
    return create_handle(out, [&](fhe_tfhe_circuit *c) {
        return fhe::tfhe_circuit_compile_many(nodes, n_nodes, terms, n_terms, n_inputs, n_tables, outputs, n_outputs, &c->plan);
    });
}

int fhe_tfhe_circuit_info_many(const fhe_tfhe_circuit *c, size_t *n_live_outputs, size_t *max_rows) {
    if (!c) return FHE_ERR_INVALID;
    if (n_live_outputs) *n_live_outputs = c->plan.n_slots;
    if (max_rows) *max_rows = c->plan.max_rows;
    return FHE_OK;
}

void fhe_tfhe_circuit_destroy(fhe_tfhe_circuit *c) { delete c; }

int fhe_tfhe_circuit_info(const fhe_tfhe_circuit *c, size_t *n_levels, size_t *n_live_nodes, size_t *max_width) {
    if (!c) return FHE_ERR_INVALID;
    if (n_levels) *n_levels = c->plan.n_levels;
    if (n_live_nodes) *n_live_nodes = c->plan.n_live;
    if (max_width) *max_width = c->plan.max_width;
    return FHE_OK;
}

int fhe_tfhe_circuit_levels(const fhe_tfhe_circuit *c, uint32_t *level_of_node) {
    if (!c || (!level_of_node && c->plan.n_nodes)) return FHE_ERR_INVALID;
    for (size_t g = 0; g < c->plan.n_nodes; ++g) level_of_node[g] = c->plan.level_of_node[g];
    return FHE_OK;
}

int fhe_tfhe_circuit_run(const fhe_tfhe_circuit *c, const fhe_torus_ctx *t, const fhe_tggsw_key *brk, int ks_log_b, int ks_d, const uint64_t *ksk_a,
                         const uint64_t *ksk_b, const uint64_t *tables, const uint64_t *in_a, const uint64_t *in_b, uint64_t *out_a, uint64_t *out_b,
                         size_t batch, fhe_mem mem, void *stream) {
    fhe::TDecomp KP;
    FHE_TRY(make_tdecomp(ks_log_b, ks_d, &KP));
    if (!c || !t || !brk || brk->t != t || !ksk_a || !ksk_b || !tables || ((!in_a || !in_b || !out_a || !out_b) && batch)) return FHE_ERR_INVALID;
    if (t->device < 0) return FHE_ERR_NO_DEVICE;
    if (brk->log_n < 8 || brk->log_n > 11) return FHE_ERR_UNSUPPORTED;  // what the fused k = 1 kernels take
    if (batch == 0) return FHE_OK;
    const fhe::TfheCircuitPlan &P = c->plan;
    const size_t n = size_t(1) << brk->log_n, n_lwe = brk->count;
    // every level is one batch of the existing entry points, which count ciphertexts in 31 bits
    const size_t widest = std::max(P.max_rows, P.n_outputs);  // max_rows >= max_width
    if (batch > 0x7fffffffull || widest * batch > 0x7fffffffull || n_lwe > 0x7ffffffeull) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const ImagePart parts[] = {{P.nodes.data(), P.n_live * sizeof(fhe_tfhe_node)}, {P.terms.data(), P.terms.size() * sizeof(fhe_tfhe_term)},
                               {P.outputs.data(), P.n_outputs * sizeof(unsigned)}, {P.out_start.data(), P.out_start.size() * sizeof(unsigned)},
                               {P.extracts.data(), P.extracts.size() * sizeof(fhe::TfheExtract)}};
    const unsigned char *img[5];
    FHE_TRY(c->image.get(t->device, parts, img));
    const fhe_tfhe_node *d_nodes = (const fhe_tfhe_node *)img[0];
    const unsigned *d_out_start = (const unsigned *)img[3];
    const size_t ks_rows = n * ks_d;
    Mirror mka(ksk_a, ks_rows * n_lwe, mem, true, st), mkb(ksk_b, ks_rows, mem, true, st), mtb(tables, P.n_tables * n, mem, true, st);
    Mirror mia(in_a, P.n_inputs * batch * n_lwe, mem, true, st), mib(in_b, P.n_inputs * batch, mem, true, st);
    Mirror moa(out_a, P.n_outputs * batch * n_lwe, mem, false, st), mob(out_b, P.n_outputs * batch, mem, false, st);
    if (mka.rc | mkb.rc | mtb.rc | mia.rc | mib.rc | moa.rc | mob.rc) return FHE_ERR_HIP;
    // one workspace (tfhe_circuit.hpp: TfheScratch): the widest level's blind rotations and extractions, a wire-table row per live output
    const fhe::TfheScratch L(P.max_width * batch, P.max_rows * batch, n, n_lwe, P.n_slots * batch, true);
    StreamWs wsp(L.total * sizeof(u64), st);
    if (wsp.rc != FHE_OK) return wsp.rc;
    u64 *ws = wsp.as<u64>(), *ra = ws + L.acc_a, *rb = ws + L.acc_b, *ea = ws + L.ext_a, *eb = ws + L.ext_b, *at = ws + L.at, *bt = ws + L.bt;
    u64 *wt_a = ws + L.wt_a, *wt_b = ws + L.wt_b;
    unsigned *table_of = reinterpret_cast<unsigned *>(ws + L.table_of);
    fhe::TfheWires W;
    W.in_a = mia.d; W.in_b = mib.d;
    W.wt_a = (const u64 *)wt_a; W.wt_b = (const u64 *)wt_b;
    W.n_inputs = (unsigned)P.n_inputs;
    W.batch = (unsigned)batch;
    W.n_lwe = (unsigned)n_lwe;
    const int bits = 64 - (brk->log_n + 1);
    typedef uint64_t U;
    int rc = FHE_OK;
    // a level is g blind rotations and r >= g * batch live outputs
    for (size_t l = 0; l < P.n_levels && rc == FHE_OK; ++l) {
        const size_t g0 = P.level_start[l], g = P.level_start[l + 1] - g0, m = g * batch;
        const size_t s0 = P.out_start[g0], r = (P.out_start[P.level_start[l + 1]] - s0) * batch;
        rc = fhe::launch<fhe::tfhe_circuit_front_kernel>(grid_for(m * 64, 8192), 256, 0, st, W, d_nodes + g0, (const fhe_tfhe_term *)img[1], (unsigned)g, bits,
                                                         at, bt, table_of);
        if (rc == FHE_OK)
            rc = fhe_tfhe_blind_rotate_tables(t, brk, (const U *)at, (const U *)bt, (const U *)mtb.d, P.n_tables, (const uint32_t *)table_of, (U *)ra, (U *)rb,
                                              m, FHE_MEM_DEVICE, stream);
        // every live output of the level, straight into the key switch's input rows: row (slot - s0) * batch + bi; a level whose nodes all
        // have one output, of index 0, is row = job
        bool index0 = r == m;
        for (size_t s = s0; index0 && s < s0 + g; ++s) index0 = P.extracts[s].index == 0;
        if (rc == FHE_OK)
            rc = fhe::launch_sample_extract_many(ra, rb, n, g, batch, d_out_start + g0, (const fhe::TfheExtract *)img[4], s0, 0, batch, 1, ea, eb, st,
                                                 index0);
        // the key switch, straight into the level's slots
        if (rc == FHE_OK)
            rc = fhe_tlwe_key_switch(ks_log_b, ks_d, (const U *)mka.d, (const U *)mkb.d, (const U *)ea, (const U *)eb, n, n_lwe,
                                     (U *)(wt_a + s0 * batch * n_lwe), (U *)(wt_b + s0 * batch), r, FHE_MEM_DEVICE, stream);
    }
    if (rc == FHE_OK)
        rc = fhe::launch<fhe::tfhe_circuit_output_kernel>(grid_for(P.n_outputs * batch * 64, 8192), 256, 0, st, W, (const unsigned *)img[2],
                                                          (unsigned)P.n_outputs, moa.d, mob.d);
    if (rc == FHE_OK) rc = moa.sync_out(st);
    if (rc == FHE_OK) rc = mob.sync_out(st);
    return rc;
}

}  // extern "C"
