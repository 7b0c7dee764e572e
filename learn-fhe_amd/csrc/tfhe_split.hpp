// Low-latency TFHE blind rotation, the host's half (torus_split_kernels.hpp has the kernel): who computes what in a cluster of G
// workgroups that owns one ciphertext, when a call takes that route, and what workspace it needs.  Plain C++: the kernel, the entry
// points (torus_api.hip) and the stand-alone test (tests/tfhe_split_host_test.cpp) read the same statements.
//
// One CMUX of the three-piece f64 form (torusf_kernels.hpp: TorusX3) computes two outputs (a, b), each the recombination of three
// rounded piece products.  The six (output, piece) pairs are independent; a member of the cluster computes a set of them:
//   G = 2   member `rank` computes output `rank` with all three pieces
//   G = 6   member `rank` computes output `rank % 2`, piece `rank / 2`
// Members of even rank therefore hold shares of the a half, members of odd rank shares of the b half, under both G.
#pragma once
#include <cstddef>

#include "../../include/fhe_ring.h"

namespace fhe {

constexpr int TFHE_SPLIT_LOG_N = 10;                // the x3 ring whose team is a whole workgroup
constexpr size_t TFHE_SPLIT_CTL_BYTES = 64;         // a cluster's polled words: one line (fhew_split_kernels.hpp: SPLIT_CTL_WORDS)

struct TfheSplitRole {
    int output;       // 0: the a half, 1: the b half
    unsigned pieces;  // bit p set: key piece p (weights 2^0, 2^22, 2^43) is this member's
};
constexpr TfheSplitRole tfhe_split_role(int G, int rank) {
    return G == 2 ? TfheSplitRole{rank, 7u} : TfheSplitRole{rank % 2, 1u << (rank / 2)};
}

// values of the lab switch "TFHE_SPLIT": -1 the rule, 0 never, 2 / 6 that G wherever the call is eligible
constexpr bool tfhe_split_value_ok(long v) { return v == -1 || v == 0 || v == 2 || v == 6; }

// The rule (option -1), read off the table in DESIGN.md section 9.6 (tools/tfhe_split_lab.py; 256 compute units): six workgroups
// per ciphertext are the fastest shape wherever they fit, two where only they fit.
constexpr int tfhe_split_rule(size_t batch, size_t cus) {
    return batch * 6 <= cus ? 6 : (batch * 2 <= cus ? 2 : 1);
}

// Workgroups per ciphertext of a blind rotation: form one of FHE_TGGSW_FORM_*, log_n the key's ring, cus the compute units of the
// device, option the lab switch.  Eligible: the x3 form at N = 1024 with every workgroup of the launch certainly resident -- one
// member per compute unit, batch * G <= cus.  Everything else is 1, the one-workgroup kernel: the integer forms, fft64 (its sums
// depend on the order of the additions, and tests pin its bits), x3 at N = 256 and 512 (teams of one wave, four to a workgroup).
constexpr int tfhe_split_g(int form, int log_n, size_t batch, size_t cus, long option) {
    if (form != FHE_TGGSW_FORM_X3 || log_n != TFHE_SPLIT_LOG_N || batch == 0 || option == 0 || !tfhe_split_value_ok(option)) return 1;
    if (option > 0) return batch <= cus / (size_t)option ? (int)option : 1;
    return batch <= cus / 2 ? tfhe_split_rule(batch, cus) : 1;
}

// the call's workspace: [batch] control lines, then the slabs [2 (hand-off parity)][batch][G][n] of 8-byte words
constexpr size_t tfhe_split_ctl_bytes(size_t batch) { return batch * TFHE_SPLIT_CTL_BYTES; }
constexpr size_t tfhe_split_slab_bytes(size_t batch, int G, size_t n) { return 2 * batch * (size_t)G * n * 8; }
constexpr size_t tfhe_split_ws_bytes(size_t batch, int G, size_t n) { return tfhe_split_ctl_bytes(batch) + tfhe_split_slab_bytes(batch, G, n); }

}  // namespace fhe
