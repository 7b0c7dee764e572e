// extern "C" entry points of the TFHE look-up-table circuits: a levelled netlist of programmable bootstraps
// (scheme/tfhe/src/bootstrapping.rs:78-82 through the tables of 118-128) over free TLWE arithmetic (tlwe.rs:22-75) -- what
// bootstrapping.rs:141-165 does one call after the other -- prepared once and run in one call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "api_common.hpp"
#include "tfhe_circuit.hpp"
#include "tfhe_circuit_kernels.hpp"
#include "torus_ctx.hpp"

struct fhe_tfhe_circuit {
    fhe::TfheCircuitPlan plan;
    // the plan as the kernels read it, uploaded to a device when the circuit first runs there: nodes [n_live] | terms | outputs [n_outputs]
    mutable std::mutex mu;
    mutable void *d_image[fhe::MAX_DEVICES] = {};
};

namespace {

static_assert(sizeof(fhe_tfhe_node_many) == sizeof(fhe_tfhe_node) && sizeof(fhe_tfhe_node) == 24, "a many-LUT node is the same 24 bytes");

struct TfheImage {
    const fhe_tfhe_node *nodes;
    const fhe_tfhe_term *terms;
    const unsigned *outputs;
    // a plan with many-LUT nodes only:
    const unsigned *out_start;          // [n_live + 1]
    const fhe::TfheExtract *extracts;   // [n_slots]
};

int device_image(const fhe_tfhe_circuit *c, int dev, TfheImage *img) {
    if (dev < 0 || dev >= fhe::MAX_DEVICES) return FHE_ERR_INVALID;
    std::lock_guard<std::mutex> lock(c->mu);
    const fhe::TfheCircuitPlan &P = c->plan;
    // every part a multiple of 8 bytes (a node is 24, a term 8), so that each starts aligned; the outputs and what follows are 32-bit
    const size_t nb = (P.n_live ? P.n_live : 1) * sizeof(fhe_tfhe_node), tb = (P.terms.size() ? P.terms.size() : 1) * sizeof(fhe_tfhe_term),
                 ob = P.n_outputs * sizeof(unsigned);
    const size_t sb = P.many ? P.out_start.size() * sizeof(unsigned) : 0, xb = P.many ? P.extracts.size() * sizeof(fhe::TfheExtract) : 0;
    if (!c->d_image[dev]) {
        void *p = nullptr;
        HIP_TRY(hipMalloc(&p, nb + tb + ob + sb + xb));
        hipError_t e = P.n_live ? hipMemcpy(p, P.nodes.data(), P.n_live * sizeof(fhe_tfhe_node), hipMemcpyHostToDevice) : hipSuccess;
        if (e == hipSuccess && !P.terms.empty())
            e = hipMemcpy((unsigned char *)p + nb, P.terms.data(), P.terms.size() * sizeof(fhe_tfhe_term), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy((unsigned char *)p + nb + tb, P.outputs.data(), ob, hipMemcpyHostToDevice);
        if (e == hipSuccess && sb) e = hipMemcpy((unsigned char *)p + nb + tb + ob, P.out_start.data(), sb, hipMemcpyHostToDevice);
        if (e == hipSuccess && xb) e = hipMemcpy((unsigned char *)p + nb + tb + ob + sb, P.extracts.data(), xb, hipMemcpyHostToDevice);
        if (e != hipSuccess) { g_last_hip = (int)e; (void)hipFree(p); return FHE_ERR_HIP; }
        c->d_image[dev] = p;
    }
    const unsigned char *base = (const unsigned char *)c->d_image[dev];
    img->nodes = (const fhe_tfhe_node *)base;
    img->terms = (const fhe_tfhe_term *)(base + nb);
    img->outputs = (const unsigned *)(base + nb + tb);
    img->out_start = (const unsigned *)(base + nb + tb + ob);
    img->extracts = (const fhe::TfheExtract *)(base + nb + tb + ob + sb);
    return FHE_OK;
}

// fhe_tfhe_circuit_run for a plan with many-LUT nodes: a level is `g` blind rotations and `r` >= g live outputs.  Same arguments, checked
// by the caller; mirrors made by the caller.
int run_many(const fhe_tfhe_circuit *c, const fhe_torus_ctx *t, const fhe_tggsw_key *brk, int ks_log_b, int ks_d, const u64 *ksk_a, const u64 *ksk_b,
             const u64 *tables, const u64 *in_a, const u64 *in_b, u64 *out_a, u64 *out_b, size_t batch, const TfheImage &img, hipStream_t st) {
    const fhe::TfheCircuitPlan &P = c->plan;
    const size_t n = size_t(1) << brk->log_n, n_lwe = brk->count;
    const size_t widest = P.max_rows > P.n_outputs ? P.max_rows : P.n_outputs;
    if (widest * batch > 0x7fffffffull) return FHE_ERR_UNSUPPORTED;
    // one workspace, in 8-byte words, the [..][n] arrays first so that each starts on a 16-byte boundary (jobs = max_width * batch blind
    // rotations, rows = max_rows * batch extractions):
    //   acc.a, acc.b [jobs][n] | extracted a [rows][n] | wt_a [n_slots][batch][n_lwe] | a~ [jobs][n_lwe] | wt_b [n_slots][batch] | b~ [jobs] |
    //   extracted b [rows] | table_of [jobs] (32-bit)
    const size_t jobs_max = P.max_width * batch, rows_max = P.max_rows * batch;
    const size_t words = jobs_max * (2 * n + n_lwe + 1) + rows_max * (n + 1) + P.n_slots * batch * (n_lwe + 1) + (jobs_max + 1) / 2;
    StreamWs wsp(words * sizeof(u64), st);
    if (wsp.rc != FHE_OK) return wsp.rc;
    u64 *ra = wsp.as<u64>(), *rb = ra + jobs_max * n, *ea = rb + jobs_max * n, *wt_a = ea + rows_max * n, *at = wt_a + P.n_slots * batch * n_lwe;
    u64 *wt_b = at + jobs_max * n_lwe, *bt = wt_b + P.n_slots * batch, *eb = bt + jobs_max;
    unsigned *table_of = reinterpret_cast<unsigned *>(eb + rows_max);
    fhe::TfheWires W;
    W.in_a = in_a; W.in_b = in_b;
    W.wt_a = (const u64 *)wt_a; W.wt_b = (const u64 *)wt_b;
    W.n_inputs = (unsigned)P.n_inputs;
    W.batch = (unsigned)batch;
    W.n_lwe = (unsigned)n_lwe;
    const int bits = 64 - (brk->log_n + 1);
    typedef uint64_t U;
    constexpr unsigned WAVES = 4;  // of the extraction: a row of n words per wave in LDS, n <= 2048 (checked by the caller)
    int rc = FHE_OK;
    for (size_t l = 0; l < P.n_levels && rc == FHE_OK; ++l) {
        const size_t g0 = P.level_start[l], g = P.level_start[l + 1] - g0, m = g * batch;
        const size_t s0 = P.out_start[g0], r = (P.out_start[P.level_start[l + 1]] - s0) * batch;
        rc = fhe::launch<fhe::tfhe_circuit_front_many_kernel>(grid_for(m * 64, 8192), 256, 0, st, W, img.nodes + g0, img.terms, (unsigned)g, bits, at, bt,
                                                              table_of);
        if (rc == FHE_OK)
            rc = fhe_tfhe_blind_rotate_tables(t, brk, (const U *)at, (const U *)bt, (const U *)tables, P.n_tables, (const uint32_t *)table_of, (U *)ra, (U *)rb,
                                              m, FHE_MEM_DEVICE, st);
        // every live output of the level, straight into the key switch's input rows: row (slot - s0) * batch + bi
        if (rc == FHE_OK)
            rc = fhe::launch<fhe::tglwe_sample_extract_many_kernel<true>>((unsigned)std::min<size_t>((m + WAVES - 1) / WAVES, 8192), 64 * WAVES,
                                                                          WAVES * n * sizeof(u64), st, (const u64 *)ra, (const u64 *)rb, (unsigned)n, (unsigned)g,
                                                                          (unsigned)batch, img.out_start + g0, img.extracts, (unsigned)s0, 0u, batch, size_t(1),
                                                                          ea, eb);
        // the key switch, straight into the level's slots
        if (rc == FHE_OK)
            rc = fhe_tlwe_key_switch(ks_log_b, ks_d, (const U *)ksk_a, (const U *)ksk_b, (const U *)ea, (const U *)eb, n, n_lwe,
                                     (U *)(wt_a + s0 * batch * n_lwe), (U *)(wt_b + s0 * batch), r, FHE_MEM_DEVICE, st);
    }
    if (rc != FHE_OK) return rc;
    return fhe::launch<fhe::tfhe_circuit_output_kernel>(grid_for(P.n_outputs * batch * 64, 8192), 256, 0, st, W, img.outputs, (unsigned)P.n_outputs, out_a, out_b);
}

}  // namespace

extern "C" {

int fhe_tfhe_circuit_create(const fhe_tfhe_node *nodes, size_t n_nodes, const fhe_tfhe_term *terms, size_t n_terms, size_t n_inputs,
                            size_t n_tables, const uint32_t *outputs, size_t n_outputs, fhe_tfhe_circuit **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    fhe_tfhe_circuit *c = new (std::nothrow) fhe_tfhe_circuit();
    if (!c) return FHE_ERR_INVALID;
    int rc;
    try {
        rc = fhe::tfhe_circuit_compile(nodes, n_nodes, terms, n_terms, n_inputs, n_tables, outputs, n_outputs, &c->plan);
    } catch (const std::bad_alloc &) {
        rc = FHE_ERR_INVALID;
    }
    if (rc != FHE_OK) { delete c; return rc; }
    *out = c;
    return FHE_OK;
}

// fhe_tfhe_circuit_create with many-LUT nodes (bootstrapping.rs:78-128, tglwe.rs:115-127): the node's fourth field is log_funcs
int fhe_tfhe_circuit_create_many(const fhe_tfhe_node *nodes, size_t n_nodes, const fhe_tfhe_term *terms, size_t n_terms, size_t n_inputs,
                                 size_t n_tables, const uint32_t *outputs, size_t n_outputs, fhe_tfhe_circuit **out) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    fhe_tfhe_circuit *c = new (std::nothrow) fhe_tfhe_circuit();
    if (!c) return FHE_ERR_INVALID;
    int rc;
    try {
        rc = fhe::tfhe_circuit_compile_many(nodes, n_nodes, terms, n_terms, n_inputs, n_tables, outputs, n_outputs, &c->plan);
    } catch (const std::bad_alloc &) {
        rc = FHE_ERR_INVALID;
    }
    if (rc != FHE_OK) { delete c; return rc; }
    *out = c;
    return FHE_OK;
}

int fhe_tfhe_circuit_info_many(const fhe_tfhe_circuit *c, size_t *n_live_outputs, size_t *max_rows) {
    if (!c) return FHE_ERR_INVALID;
    if (n_live_outputs) *n_live_outputs = c->plan.n_slots;
    if (max_rows) *max_rows = c->plan.max_rows;
    return FHE_OK;
}

void fhe_tfhe_circuit_destroy(fhe_tfhe_circuit *c) {
    if (!c) return;
    for (int dev = 0; dev < fhe::MAX_DEVICES; ++dev) {
        if (!c->d_image[dev]) continue;
        DeviceGuard guard(dev);
        (void)hipFree(c->d_image[dev]);
    }
    delete c;
}

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
    const size_t widest = P.max_width > P.n_outputs ? P.max_width : P.n_outputs;
    if (batch > 0x7fffffffull || widest * batch > 0x7fffffffull || n_lwe > 0x7ffffffeull) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(t->device);
    if (!guard.ok) return FHE_ERR_HIP;
    TfheImage img{};
    FHE_TRY(device_image(c, t->device, &img));
    const size_t ks_rows = n * ks_d;
    Mirror mka(ksk_a, ks_rows * n_lwe, mem, true, st), mkb(ksk_b, ks_rows, mem, true, st), mtb(tables, P.n_tables * n, mem, true, st);
    Mirror mia(in_a, P.n_inputs * batch * n_lwe, mem, true, st), mib(in_b, P.n_inputs * batch, mem, true, st);
    Mirror moa(out_a, P.n_outputs * batch * n_lwe, mem, false, st), mob(out_b, P.n_outputs * batch, mem, false, st);
    if (mka.rc | mkb.rc | mtb.rc | mia.rc | mib.rc | moa.rc | mob.rc) return FHE_ERR_HIP;
    if (P.many) {  // a handle of fhe_tfhe_circuit_create_many with some log_funcs > 0
        int rc = run_many(c, t, brk, ks_log_b, ks_d, mka.d, mkb.d, mtb.d, mia.d, mib.d, moa.d, mob.d, batch, img, st);
        if (rc == FHE_OK) rc = moa.sync_out(st);
        if (rc == FHE_OK) rc = mob.sync_out(st);
        return rc;
    }
    // one workspace: the wire table of the live nodes and the scratch of the widest level (jobs = max_width * batch), in 8-byte words;
    // the [..][n] arrays first, so that each starts on a 16-byte boundary:
    //   acc.a, acc.b, extracted a [jobs][n] | wt_a [n_live][batch][n_lwe] | a~ [jobs][n_lwe] | wt_b [n_live][batch] | b~ [jobs] |
    //   extracted b [jobs] | table_of [jobs] (32-bit)
    const size_t jobs_max = P.max_width * batch;
    const size_t words = P.n_live * batch * (n_lwe + 1) + jobs_max * (3 * n + n_lwe + 2) + (jobs_max + 1) / 2;
    StreamWs wsp(words * sizeof(u64), st);
    if (wsp.rc != FHE_OK) return wsp.rc;
    u64 *ra = wsp.as<u64>(), *rb = ra + jobs_max * n, *ea = rb + jobs_max * n, *wt_a = ea + jobs_max * n, *at = wt_a + P.n_live * batch * n_lwe;
    u64 *wt_b = at + jobs_max * n_lwe, *bt = wt_b + P.n_live * batch, *eb = bt + jobs_max;
    unsigned *table_of = reinterpret_cast<unsigned *>(eb + jobs_max);
    fhe::TfheWires W;
    W.in_a = mia.d; W.in_b = mib.d;
    W.wt_a = (const u64 *)wt_a; W.wt_b = (const u64 *)wt_b;
    W.n_inputs = (unsigned)P.n_inputs;
    W.batch = (unsigned)batch;
    W.n_lwe = (unsigned)n_lwe;
    const int bits = 64 - (brk->log_n + 1);
    typedef uint64_t U;
    int rc = FHE_OK;
    for (size_t l = 0; l < P.n_levels && rc == FHE_OK; ++l) {
        const size_t g0 = P.level_start[l], g = P.level_start[l + 1] - g0, m = g * batch;
        rc = fhe::launch<fhe::tfhe_circuit_front_kernel>(grid_for(m * 64, 8192), 256, 0, st, W, img.nodes + g0, img.terms, (unsigned)g, bits, at, bt, table_of);
        if (rc == FHE_OK)
            rc = fhe_tfhe_blind_rotate_tables(t, brk, (const U *)at, (const U *)bt, (const U *)mtb.d, P.n_tables, (const uint32_t *)table_of, (U *)ra, (U *)rb,
                                              m, FHE_MEM_DEVICE, stream);
        if (rc == FHE_OK) rc = fhe_tglwe_sample_extract((const U *)ra, (const U *)rb, n, 0, (U *)ea, (U *)eb, m, FHE_MEM_DEVICE, stream);
        // the key switch, straight into the level's slots
        if (rc == FHE_OK)
            rc = fhe_tlwe_key_switch(ks_log_b, ks_d, (const U *)mka.d, (const U *)mkb.d, (const U *)ea, (const U *)eb, n, n_lwe,
                                     (U *)(wt_a + g0 * batch * n_lwe), (U *)(wt_b + g0 * batch), m, FHE_MEM_DEVICE, stream);
    }
    if (rc != FHE_OK) return rc;
    rc = fhe::launch<fhe::tfhe_circuit_output_kernel>(grid_for(P.n_outputs * batch * 64, 8192), 256, 0, st, W, img.outputs, (unsigned)P.n_outputs, moa.d, mob.d);
    if (rc == FHE_OK) rc = moa.sync_out(st);
    if (rc == FHE_OK) rc = mob.sync_out(st);
    return rc;
}

}  // extern "C"
