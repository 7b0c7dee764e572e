// The prepared FHEW keys behind the opaque handles of include/fhe_ring.h, shared by the translation units that run on them
// (fhew_api.hip prepares them and owns their entry points; fhew_circuit_api.hip reads the ring and the LWE dimension).
#pragma once
#include "ctx.hpp"
#include "fhew_kernels.hpp"

struct fhe_key {
    const fhe_ctx *ctx = nullptr;
    int log_n = 0;
    int log_b = 0, d = 0;
    int rows_per_ct = 0;  // 2d (RGSW) or d (key-switching key)
    size_t count = 0;
    bool composed = false;  // route: the composed launches (fhew_composed_kernels.hpp) or the fused kernels (N = 128 .. 2048)
    // fused: [count][rows_per_ct][2][N], evaluation domain, key_perm layout
    // composed: [2][count][rows_per_ct][N] (every a row, then every b row), evaluation domain in ntt_fwd_device's order
    u64 *d_rows = nullptr;
    u64 *d_rows_small = nullptr;  // N >= 1024: the same rows in the layout of the small-batch kernels (4 coefficients per lane)
    fhe::DecompParams P{};
};

struct fhe_bootstrap_key {
    const fhe_ctx *ctx = nullptr;
    const fhe_key *brk = nullptr, *ak = nullptr;
    int w = 0;
    unsigned *d_ak_t = nullptr;  // [w + 1] exponents mod 2N
    unsigned *d_dlog = nullptr;  // [2N]
    int *d_status = nullptr;     // sticky device-side error word of asynchronous (device-memory) blind rotations: fhe_bootstrap_key_status
};
