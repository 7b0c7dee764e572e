// Which instantiation a call runs: the only place that turns run-time integers (ring size, pseudo-Mersenne bit length, flags)
// into template arguments.  A call site names its kernel, the arguments and the LISTS of values it is instantiated for; the
// helpers pick the entry that matches and hand it to a generic lambda as a type.  A lambda crossed with a list instantiates
// every entry of it: where one policy or size has a shorter list, the call site says so with `if constexpr`
// (tools/kernel_inventory.py lists what was compiled).
#pragma once
#include <type_traits>

#include "api_common.hpp"
#include "arith.hpp"

namespace fhe {
template <int V>
using Int = std::integral_constant<int, V>;
template <class T>
struct Type { using type = T; };

// f(Int<v>{}) for the v among Vs that equals `value`; FHE_ERR_UNSUPPORTED if none does
template <int... Vs, class F>
int with_int(int value, F &&f) {
    int rc = FHE_ERR_UNSUPPORTED;
    (void)(... || (value == Vs ? (rc = f(Int<Vs>{}), true) : false));
    return rc;
}

// f(std::true_type{}) or f(std::false_type{})
template <class F>
int with_bool(bool value, F &&f) {
    return value ? f(std::true_type{}) : f(std::false_type{});
}

// f(Type<Fam<b>>{}) for the b among Bs that equals pm (the common pseudo-Mersenne bit length of the moduli), else f(Type<ArithShoup>{})
template <template <int> class Fam, int... Bs, class F>
int with_policy(int pm, F &&f) {
    int rc = FHE_ERR_UNSUPPORTED;
    if ((... || (pm == Bs ? (rc = f(Type<Fam<Bs>>{}), true) : false))) return rc;
    return f(Type<ArithShoup>{});
}

// The RNS kernels keep their limb vectors in registers: f(Int<M>{}, std::bool_constant<FULL>{}) for the smallest bound M that holds
// `la` source limbs; FULL: exactly M limbs, no limb predicates at all.
template <class F>
int with_limb_bound(int la, F &&f) {
    if (la == 8) return f(Int<8>{}, std::true_type{});  // the BASELINE shape
    if (la == 1) return f(Int<1>{}, std::true_type{});  // `rescale()` and K = 1
    if (la <= 4) return f(Int<4>{}, std::false_type{});
    if (la <= 8) return f(Int<8>{}, std::false_type{});
    if (la <= 16) return f(Int<16>{}, std::false_type{});
    return f(Int<32>{}, std::false_type{});
}

// a team kernel over `jobs` polynomials: ceil(jobs / WR::TEAMS) workgroups of WR::THREADS threads
template <auto K, class WR, class... A>
int launch_teams(size_t jobs, size_t lds, hipStream_t st, A... args) {
    return launch<K>((unsigned)((jobs + WR::TEAMS - 1) / WR::TEAMS), WR::THREADS, lds, st, args...);
}
}  // namespace fhe
