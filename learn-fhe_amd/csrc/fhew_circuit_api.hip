// extern "C" entry points of the FHEW gate circuits: a levelled netlist of `Fhew` gates (scheme/fhew/src/fhew.rs:27-29, 59-67) --
// what scheme/fhew/src/fhew/boolean.rs:134-176 and fhew/uint8.rs:50-163 compose gate by gate -- prepared once and run in one call.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "api_common.hpp"
#include "fhew_circuit.hpp"
#include "fhew_circuit_kernels.hpp"
#include "fhew_keys.hpp"

struct fhe_fhew_circuit {
    fhe::CircuitPlan plan;
    mutable DeviceImage image;  // the plan as the kernels read it: gates [n_live] | outputs [n_outputs]
};

namespace {

// BootstrappingParam::big_q_by_8 / big_q_by_4 (scheme/fhew/src/bootstrapping.rs:62-68): Zq::from_f64(q, q as f64 / k as f64)
uint64_t round_div(uint64_t q, double k) { return (uint64_t)std::round((double)q / k) % q; }

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" {

int fhe_fhew_circuit_create(const fhe_fhew_gate *gates, size_t n_gates, size_t n_inputs, const uint32_t *outputs, size_t n_outputs,
                            fhe_fhew_circuit **out) {
    return create_handle(out, [&](fhe_fhew_circuit *c) { return fhe::circuit_compile(gates, n_gates, n_inputs, outputs, n_outputs, &c->plan); });
}

void fhe_fhew_circuit_destroy(fhe_fhew_circuit *c) { delete c; }

int fhe_fhew_circuit_info(const fhe_fhew_circuit *c, size_t *n_levels, size_t *n_live_gates, size_t *max_width) {
    if (!c) return FHE_ERR_INVALID;
    if (n_levels) *n_levels = c->plan.n_levels;
    if (n_live_gates) *n_live_gates = c->plan.n_live;
    if (max_width) *max_width = c->plan.max_width;
    return FHE_OK;
}

int fhe_fhew_circuit_levels(const fhe_fhew_circuit *c, uint32_t *level_of_gate) {
    if (!c || (!level_of_gate && c->plan.n_gates)) return FHE_ERR_INVALID;
    for (size_t g = 0; g < c->plan.n_gates; ++g) level_of_gate[g] = c->plan.level_of_gate[g];
    return FHE_OK;
}

int fhe_fhew_circuit_run(const fhe_fhew_circuit *c, const fhe_bootstrap_key *bk, uint64_t q_ks, int ks_log_b, int ks_d,
                         const uint64_t *lwe_ksk_a, const uint64_t *lwe_ksk_b, const uint64_t *in_a, const uint64_t *in_b, uint64_t *out_a,
                         uint64_t *out_b, size_t batch, fhe_mem mem, void *stream) {
    if (!c || !bk || !lwe_ksk_a || !lwe_ksk_b || ((!in_a || !in_b || !out_a || !out_b) && batch)) return FHE_ERR_INVALID;
    if (q_ks < 2 || ks_log_b < 1 || ks_d < 1 || ks_d > 64) return FHE_ERR_INVALID;  // (the key switch validates the gadget in full)
    const fhe_ctx *ctx = bk->ctx;
    if (ctx->device < 0) return FHE_ERR_NO_DEVICE;
    if (batch == 0) return FHE_OK;
    const fhe::CircuitPlan &P = c->plan;
    const int log_n = bk->brk->log_n;
    if (log_n < 2) return FHE_ERR_UNSUPPORTED;
    const size_t n = size_t(1) << log_n, n_lwe = bk->brk->count;
    const uint64_t big_q = ctx->q;
    // every level is one batch of the existing entry points, which count ciphertexts in 31 bits
    const size_t widest = P.max_width > P.n_outputs ? P.max_width : P.n_outputs;
    if (batch > 0x7fffffffull || widest * batch > 0x7fffffffull) return FHE_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return FHE_ERR_HIP;
    const ImagePart parts[] = {{P.gates.data(), P.n_live * sizeof(fhe::CircuitGate)}, {P.outputs.data(), P.n_outputs * sizeof(unsigned)}};
    const unsigned char *img[2];
    FHE_TRY(c->image.get(ctx->device, parts, img));
    const fhe::CircuitGate *d_gates = (const fhe::CircuitGate *)img[0];
    const unsigned *d_outputs = (const unsigned *)img[1];
    const size_t ks_rows = n * ks_d;
    Mirror mka(lwe_ksk_a, ks_rows * n_lwe, mem, true, st), mkb(lwe_ksk_b, ks_rows, mem, true, st);
    Mirror mia(in_a, P.n_inputs * batch * n, mem, true, st), mib(in_b, P.n_inputs * batch, mem, true, st);
    Mirror moa(out_a, P.n_outputs * batch * n, mem, false, st), mob(out_b, P.n_outputs * batch, mem, false, st);
    if (mka.rc | mkb.rc | mia.rc | mib.rc | moa.rc | mob.rc) return FHE_ERR_HIP;
    // one workspace: the wire table of the live gates, then the scratch of the widest level (cts = max_width * batch ciphertexts);
    // every [..][n] array first, so that each starts on a 16-byte boundary:
    //   wt_a [n_live][batch][n] | a1, lut, ra, rb [cts][n] | wt_b [n_live][batch] | b1 [cts] | a2 [cts][n_lwe], b2 [cts] | a3, b3
    const size_t cts = P.max_width * batch;
    const size_t words = P.n_live * batch * (n + 1) + cts * (4 * n + 1 + 2 * (n_lwe + 1));
    StreamWs wsp(words * sizeof(u64), st);
    if (wsp.rc != FHE_OK) return wsp.rc;
    uint64_t *wt_a = wsp.as<uint64_t>(), *a1 = wt_a + P.n_live * batch * n, *lut = a1 + cts * n, *ra = lut + cts * n, *rb = ra + cts * n;
    uint64_t *wt_b = rb + cts * n, *b1 = wt_b + P.n_live * batch, *a2 = b1 + cts, *a3 = a2 + cts * (n_lwe + 1);
    fhe::CircuitWires W;
    W.in_a = mia.d; W.in_b = mib.d;
    W.wt_a = (const u64 *)wt_a; W.wt_b = (const u64 *)wt_b;
    W.n_inputs = (unsigned)P.n_inputs;
    W.batch = (unsigned)batch;
    W.log_n = (unsigned)log_n;
    W.q = big_q;
    W.q_by_4 = round_div(big_q, 4.0);
    W.q_by_8 = round_div(big_q, 8.0);
    // 16-byte accesses where every operand allows them (the workspace does; a caller's device pointer may not)
    const bool vec = aligned16(mia.d) && aligned16(moa.d) && aligned16(wt_a);
    int rc = FHE_OK;
    for (size_t l = 0; l < P.n_levels && rc == FHE_OK; ++l) {
        const size_t g0 = P.level_start[l], g = P.level_start[l + 1] - g0, m = g * batch;
        // the level's tail: b2 directly behind a2 and b3 behind a3, so that mod_switch_odd is ONE launch over both
        uint64_t *b2 = a2 + m * n_lwe, *b3 = a3 + m * n_lwe;
        const unsigned grid = grid_for(m * n / (vec ? 2 : 1), 8192);
        rc = vec ? fhe::launch<fhe::circuit_front_kernel<2>>(grid, 256, 0, st, W, d_gates + g0, (unsigned)g, (u64)q_ks, (u64 *)a1, (u64 *)b1, (u64 *)lut)
                 : fhe::launch<fhe::circuit_front_kernel<1>>(grid, 256, 0, st, W, d_gates + g0, (unsigned)g, (u64)q_ks, (u64 *)a1, (u64 *)b1, (u64 *)lut);
        if (rc == FHE_OK) rc = fhe_lwe_key_switch(q_ks, ks_log_b, ks_d, (const uint64_t *)mka.d, (const uint64_t *)mkb.d, a1, b1, n, n_lwe, a2, b2, m, FHE_MEM_DEVICE, stream);
        if (rc == FHE_OK) rc = fhe_lwe_mod_switch(q_ks, 2 * n, a2, a3, m * (n_lwe + 1), 1, FHE_MEM_DEVICE, stream);
        if (rc == FHE_OK) rc = fhe_blind_rotate(bk, a3, b3, lut, n, ra, rb, m, FHE_MEM_DEVICE, stream, nullptr, nullptr);
        // sample_extract(0) + Q/8 (fhew.rs:37-38), straight into the level's slots
        if (rc == FHE_OK) rc = fhe_rlwe_sample_extract(big_q, ra, rb, n, 0, W.q_by_8, wt_a + g0 * batch * n, wt_b + g0 * batch, m, FHE_MEM_DEVICE, stream);
    }
    if (rc != FHE_OK) return rc;
    {
        const unsigned grid = grid_for(P.n_outputs * batch * n / (vec ? 2 : 1), 8192);
        rc = vec ? fhe::launch<fhe::circuit_output_kernel<2>>(grid, 256, 0, st, W, d_outputs, (unsigned)P.n_outputs, moa.d, mob.d)
                 : fhe::launch<fhe::circuit_output_kernel<1>>(grid, 256, 0, st, W, d_outputs, (unsigned)P.n_outputs, moa.d, mob.d);
    }
    if (rc == FHE_OK) rc = moa.sync_out(st);
    if (rc == FHE_OK) rc = mob.sync_out(st);
    // host-memory calls have synchronised for their outputs: report the blind rotations' data-dependent checks with them
    if (rc == FHE_OK && mem == FHE_MEM_HOST) rc = fhe_bootstrap_key_status(bk, stream, 1);
    return rc;
}

}  // extern "C"
