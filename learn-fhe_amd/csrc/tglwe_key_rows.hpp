// The prepared form of key rows that are TGLWE ciphertexts (k = 1) for the team kernels of the two 60-bit primes: shared by the
// relinearisation key (tfhe_mul_api.hip) and the automorphism keys (tfhe_trace_api.hip).
#pragma once
#include "dispatch.hpp"
#include "torus_ctx.hpp"
#include "torus_dispatch.hpp"

namespace {

// rows_a, rows_b [rows][n] on the device -> out[pi] [rows][2][n] per prime pi: residues, forward transform, key_perm layout
// (fhew_kernels.hpp).  Stream ordered on st; the staging area comes from the library's pool.
inline int tglwe_rows_prepare(const fhe_torus_ctx *t, int log_n, const u64 *rows_a, const u64 *rows_b, size_t rows, u64 *const (&out)[2], hipStream_t st) {
    const size_t half = rows << log_n, words = 2 * half;  // of one prime
    StreamWs wsp(words * sizeof(u64), st);                // the residues of one prime, a then b, transformed in place
    int rc = wsp.rc;
    u64 *ta = wsp.as<u64>(), *tb = ta + half;
    for (int pi = 0; pi < 2 && rc == FHE_OK; ++pi) {
        const u64 p = pi ? t->T.p1 : t->T.p0;
        rc = fhe::launch<fhe::torus_residue_kernel>(grid_for(half), 256, 0, st, rows_a, ta, half, p);
        if (rc == FHE_OK) rc = fhe::launch<fhe::torus_residue_kernel>(grid_for(half), 256, 0, st, rows_b, tb, half, p);
        if (rc == FHE_OK) rc = fhe::ntt_fwd_multi(t->d_descs + pi, 1, ta, log_n, 2 * rows, st, 60);
        if (rc == FHE_OK)
            rc = with_torus<TorusRing>(log_n, [&](auto wr) {
                using W = typename decltype(wr)::type;
                return fhe::launch<fhe::key_permute_kernel<W>>(grid_for(half), 256, 0, st, (const u64 *)ta, (const u64 *)tb, out[pi], rows, 60);
            });
    }
    return rc;
}

}  // namespace
