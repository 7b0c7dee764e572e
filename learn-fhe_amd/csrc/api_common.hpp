// Shared helpers of the extern "C" translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

#include "../../include/fhe_ring.h"
#include "dev_arith.hpp"
#include "tfhe_split.hpp"

namespace fhe {
inline thread_local int g_last_hip = 0;
}
using fhe::g_last_hip;
using fhe::u64;

#define HIP_TRY(expr)                         \
    do {                                      \
        hipError_t e_ = (expr);               \
        if (e_ != hipSuccess) {               \
            fhe::g_last_hip = (int)e_;        \
            return FHE_ERR_HIP;               \
        }                                     \
    } while (0)

namespace {
inline bool is_pow2(size_t n) { return n && !(n & (n - 1)); }
inline int ilog2(size_t n) { return 63 - __builtin_clzll((unsigned long long)n); }
// t.rem_euclid(2n): the exponent of X^t in Z[X] / (X^n + 1)
inline unsigned rem_euclid_2n(int64_t t, size_t n) {
    const int64_t two_n = 2 * (int64_t)n;
    return (unsigned)(((t % two_n) + two_n) % two_n);
}

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) prev = -1;
        if (prev != dev) e = hipSetDevice(dev);
        if (e != hipSuccess) { ok = false; fhe::g_last_hip = (int)e; }
        if (prev == dev) prev = -1;  // nothing to restore
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Entry points that take a modulus instead of a context have no device of their own: they run where their DEVICE operands
// live (hipPointerGetAttributes of the first one), whatever the caller's current device is; host-memory calls use the current
// device.
struct PtrDeviceGuard {
    DeviceGuard *g = nullptr;
    bool ok = true;
    PtrDeviceGuard(const void *p, fhe_mem mem) {
        if (mem != FHE_MEM_DEVICE || !p) return;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return; }  // not a HIP allocation: leave the device alone
        g = new DeviceGuard(at.device);
        ok = g->ok;
    }
    ~PtrDeviceGuard() { delete g; }
    PtrDeviceGuard(const PtrDeviceGuard &) = delete;
    PtrDeviceGuard &operator=(const PtrDeviceGuard &) = delete;
};
}  // namespace

// Per-call device workspace, allocated and released IN STREAM ORDER from a pool of the LIBRARY'S OWN (one per device, created on
// first use): an entry point neither pays a device-wide hipMalloc / hipFree nor has to synchronise the stream before it returns
// to keep its workspace alive, and the device's default pool -- which a co-resident framework may be using -- keeps its
// settings.  The pool holds on to freed blocks up to FHE_POOL_KEEP_BYTES; fhe_trim() hands everything back to the driver.
namespace fhe {
constexpr uint64_t POOL_KEEP_BYTES = uint64_t(4) << 30;
constexpr int MAX_DEVICES = 64;
inline hipMemPool_t g_pools[MAX_DEVICES] = {};
inline std::mutex &pool_mutex() {
    static std::mutex mu;
    return mu;
}
inline hipMemPool_t private_pool(int dev) {
    if (dev < 0 || dev >= MAX_DEVICES) return nullptr;
    std::lock_guard<std::mutex> lock(pool_mutex());
    if (!g_pools[dev]) {
        hipMemPoolProps props = {};
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = dev;
        hipMemPool_t pool = nullptr;
        if (hipMemPoolCreate(&pool, &props) != hipSuccess) return nullptr;
        uint64_t keep = POOL_KEEP_BYTES;
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
        g_pools[dev] = pool;
    }
    return g_pools[dev];
}
}  // namespace fhe

// Lab switches: routes that a faster one replaced stay in the library so that tests can compare the two bit for bit and A/B runs
// need no second build.  None changes a result.  Each is read from the environment ONCE (FHE_RING_<NAME>, when the library first
// looks at any of them) and afterwards only changes through fhe_set_option(): no getenv on any call path.
namespace fhe {
// FHEW_COMPOSED: FHEW keys prepared while it is set run the composed route (fhew_composed_kernels.hpp) at N = 128 .. 2048 as well.
// BR_SPLIT: workgroups per ciphertext of the FHEW blind rotation (fhew_split_kernels.hpp): -1 the library's rule, 0 never split, 2 / 4 / 8.
// PFKS_SPLIT: blocks that share the input rows of one output tile of fhe_tlwe_pfks (pfks_kernels.hpp): 0 the library's rule, 1 never split,
// k >= 2: k blocks where the rows allow it.  PFKS_CHUNK: input coefficients whose digits a block keeps in LDS at a time: 0 the library's
// rule, c >= 1: at most c.
// TFHE_SPLIT: workgroups per ciphertext of the TFHE blind rotation (torus_split_kernels.hpp): -1 the library's rule, 0 never split, 2 / 6.
// LUT_EXTRACT: who writes the extractions of fhe_tfhe_lut_eval: 0 the library's rule, 1 the rotation ladder from its registers, 2 a kernel
// of its own that reads the stored accumulators (tfhe_lut_kernels.hpp).
// NO_RANKK_FUSED: rank-k TGGSW keys prepared while it is set take the composed route (torusk_kernels.hpp) where the fused three-piece
// kernels (torusk_fused_kernels.hpp) would serve them.
// PACK_SPLIT: teams that share the key rows of one pack of fhe_tlwe_pack (tfhe_pack_kernels.hpp): 0 the library's rule, k >= 1: k chunks of
// rows per pack, clamped to what the exactness bound needs and to one row per chunk (tfhe_pack.hpp: pack_plan).
// PACK_ROUTE: which product fhe_tlwe_pack runs: 0 the library's rule (tfhe_pack.hpp: pack_scalar_route), 1 the transforms, 2 the scalar
// digits x key product of fhe_tlwe_pfks followed by one rotate-and-add kernel.  PACK_SLAB: packs one launch group of fhe_tlwe_pack works on:
// 0 the library's rule (what 256 MiB of scratch hold), s >= 1: at most s.
enum Opt { OPT_NO_EDGE = 0, OPT_NO_LIMB_MAJOR, OPT_NO_W12, OPT_NO_FUSED_MUL, OPT_SMALL_BATCH, OPT_NO_PACKED_DIGITS, OPT_NO_F64_EXACT, OPT_FHEW_COMPOSED,
           OPT_BR_SPLIT, OPT_PFKS_SPLIT, OPT_PFKS_CHUNK, OPT_LUT_EXTRACT, OPT_TFHE_SPLIT, OPT_NO_RANKK_FUSED, OPT_PACK_SPLIT, OPT_PACK_ROUTE, OPT_PACK_SLAB,
           OPT_COUNT };
inline const char *const OPT_NAMES[OPT_COUNT] = {"NO_EDGE", "NO_LIMB_MAJOR", "NO_W12", "NO_FUSED_MUL", "SMALL_BATCH", "NO_PACKED_DIGITS", "NO_F64_EXACT",
                                                 "FHEW_COMPOSED", "BR_SPLIT", "PFKS_SPLIT", "PFKS_CHUNK", "LUT_EXTRACT", "TFHE_SPLIT", "NO_RANKK_FUSED", "PACK_SPLIT", "PACK_ROUTE", "PACK_SLAB"};
inline bool br_split_value_ok(long v) { return v == -1 || v == 0 || v == 2 || v == 4 || v == 8; }
// the values an option admits (tfhe_split.hpp states TFHE_SPLIT's); the others take any
inline bool opt_value_ok(int i, long v) {
    if (i == OPT_BR_SPLIT) return br_split_value_ok(v);
    if (i == OPT_TFHE_SPLIT) return tfhe_split_value_ok(v);
    return true;
}
struct Options {
    std::atomic<long> v[OPT_COUNT];
    Options() {
        for (int i = 0; i < OPT_COUNT; ++i) {
            char name[64] = "FHE_RING_";
            std::strncat(name, OPT_NAMES[i], sizeof(name) - 10);
            const char *e = std::getenv(name);
            long val = e ? std::atol(e) : ((i == OPT_SMALL_BATCH || i == OPT_BR_SPLIT || i == OPT_TFHE_SPLIT) ? -1L : 0L);
            if (!opt_value_ok(i, val)) val = -1L;
            v[i].store(val, std::memory_order_relaxed);
        }
    }
};
inline Options &options() {
    static Options o;
    return o;
}
inline long opt(Opt k) { return options().v[k].load(std::memory_order_relaxed); }

// compute units of a device (cached): dispatch thresholds are stated in workgroup generations of THIS chip, not in literals
inline int cu_count(int dev) {
    static std::atomic<int> cache[MAX_DEVICES] = {};
    if (dev < 0 || dev >= MAX_DEVICES) return 256;
    int c = cache[dev].load(std::memory_order_relaxed);
    if (c > 0) return c;
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) { (void)hipGetLastError(); c = 256; }
    cache[dev].store(c, std::memory_order_relaxed);
    return c;
}
inline int current_cu_count() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 256; }
    return cu_count(dev);
}

// blocks of 256 threads for `total` items of a grid-stride kernel: at least one, at most `cap`
inline unsigned grid_for(size_t total, unsigned cap = 16384) {
    size_t b = (total + 255) / 256;
    return (unsigned)(b > cap ? cap : (b ? b : 1));
}

// K's dynamic-LDS limit on the current device, raised to at least `lds`.  Registered per (kernel, device) at the largest size
// asked for so far: once that covers the call, one acquire load and no lock; the slow path only ever raises the limit.
template <auto K>
int raise_lds(size_t lds) {
    static std::atomic<size_t> registered[MAX_DEVICES];
    static std::mutex mu;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && (dev < 0 || dev >= MAX_DEVICES)) e = hipErrorInvalidDevice;
    if (e == hipSuccess && registered[dev].load(std::memory_order_acquire) < lds) {
        std::lock_guard<std::mutex> lock(mu);
        if (registered[dev].load(std::memory_order_relaxed) < lds) {
            e = hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e == hipSuccess) registered[dev].store(lds, std::memory_order_release);
        }
    }
    if (e != hipSuccess) { g_last_hip = (int)e; return FHE_ERR_HIP; }
    return FHE_OK;
}

// Every kernel launch of the library: raises K's LDS limit above 64 KiB (raise_lds), launches, and returns FHE_OK or
// FHE_ERR_HIP with g_last_hip set.
template <auto K, class... A>
int launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
    if (lds > 64 * 1024) {
        const int rc = raise_lds<K>(lds);
        if (rc != FHE_OK) return rc;
    }
    hipLaunchKernelGGL(K, grid, block, lds, st, args...);
    HIP_TRY(hipGetLastError());
    return FHE_OK;
}
}  // namespace fhe
using fhe::grid_for;

// returns from the enclosing function with the FHE_* status of `expr` unless it is FHE_OK
#define FHE_TRY(expr)                   \
    do {                                \
        const int rc_ = (expr);         \
        if (rc_ != FHE_OK) return rc_;  \
    } while (0)

namespace {
struct StreamWs {
    void *p = nullptr;
    hipStream_t st;
    int rc = FHE_OK;
    StreamWs(size_t bytes, hipStream_t s) : st(s) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        hipMemPool_t pool = e == hipSuccess ? fhe::private_pool(dev) : nullptr;
        if (e == hipSuccess) e = pool ? hipMallocFromPoolAsync(&p, bytes ? bytes : 8, pool, s) : hipMallocAsync(&p, bytes ? bytes : 8, s);
        if (e != hipSuccess) { fhe::g_last_hip = (int)e; rc = FHE_ERR_HIP; p = nullptr; }
    }
    ~StreamWs() {
        if (p) (void)hipFreeAsync(p, st);
    }
    StreamWs(const StreamWs &) = delete;
    StreamWs &operator=(const StreamWs &) = delete;
    template <class T>
    T *as() const { return static_cast<T *>(p); }
};

// Host-memory convenience path (FHE_MEM_HOST): a device mirror of a host array.  `in`: copy host -> device on
// construction; sync_out(): copy back.  Device-memory callers (FHE_MEM_DEVICE) get the pointer passed through.
struct Mirror {
    u64 *d = nullptr;
    void *host = nullptr;
    size_t bytes = 0;
    bool owned = false;
    int rc = FHE_OK;
    hipStream_t st_ = nullptr;
    Mirror(const void *p, size_t count, fhe_mem mem, bool copy_in, hipStream_t st) : st_(st) {
        bytes = count * sizeof(u64);
        if (mem == FHE_MEM_DEVICE || count == 0) { d = (u64 *)p; return; }
        host = const_cast<void *>(p);
        owned = true;
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        hipMemPool_t pool = e == hipSuccess ? fhe::private_pool(dev) : nullptr;
        if (e == hipSuccess) e = pool ? hipMallocFromPoolAsync((void **)&d, bytes, pool, st) : hipMallocAsync((void **)&d, bytes, st);
        if (e == hipSuccess && copy_in) e = hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) { fhe::g_last_hip = (int)e; rc = FHE_ERR_HIP; }
    }
    int sync_out(hipStream_t st) {
        if (!owned || rc != FHE_OK) return rc;
        hipError_t e = hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { fhe::g_last_hip = (int)e; rc = FHE_ERR_HIP; }
        return rc;
    }
    ~Mirror() {
        if (owned && d) (void)hipFreeAsync(d, st_);  // stream ordered: after the kernels and copies that use it
    }
    Mirror(const Mirror &) = delete;
    Mirror &operator=(const Mirror &) = delete;
};

// What a prepared handle's kernels read (a compiled circuit's descriptors), uploaded to a device when the handle first runs there and
// freed with the handle.  The image is the parts laid end to end, each padded to a multiple of 8 bytes (an empty part takes 8).
struct ImagePart {
    const void *p;
    size_t bytes;
};
struct DeviceImage {
    std::mutex mu;
    void *d[fhe::MAX_DEVICES] = {};
    static size_t padded(size_t bytes) { return bytes ? (bytes + 7) & ~size_t(7) : 8; }
    // at[i]: part i on device `dev`; the parts must be the same on every call
    template <size_t N>
    int get(int dev, const ImagePart (&parts)[N], const unsigned char *(&at)[N]) {
        if (dev < 0 || dev >= fhe::MAX_DEVICES) return FHE_ERR_INVALID;
        std::lock_guard<std::mutex> lock(mu);
        size_t total = 0;
        for (const ImagePart &pt : parts) total += padded(pt.bytes);
        if (!d[dev]) {
            void *p = nullptr;
            HIP_TRY(hipMalloc(&p, total));
            hipError_t e = hipSuccess;
            size_t off = 0;
            for (const ImagePart &pt : parts) {
                if (e == hipSuccess && pt.bytes) e = hipMemcpy((unsigned char *)p + off, pt.p, pt.bytes, hipMemcpyHostToDevice);
                off += padded(pt.bytes);
            }
            if (e != hipSuccess) { fhe::g_last_hip = (int)e; (void)hipFree(p); return FHE_ERR_HIP; }
            d[dev] = p;
        }
        size_t off = 0;
        for (size_t i = 0; i < N; ++i) {
            at[i] = (const unsigned char *)d[dev] + off;
            off += padded(parts[i].bytes);
        }
        return FHE_OK;
    }
    ~DeviceImage() {
        for (int dev = 0; dev < fhe::MAX_DEVICES; ++dev) {
            if (!d[dev]) continue;
            DeviceGuard guard(dev);
            (void)hipFree(d[dev]);
        }
    }
};

// The body of a handle's create entry: a new H, compile(h) -> FHE_* with an allocation failure caught, no handle unless FHE_OK
template <class H, class F>
int create_handle(H **out, F &&compile) {
    if (!out) return FHE_ERR_INVALID;
    *out = nullptr;
    H *h = new (std::nothrow) H();
    if (!h) return FHE_ERR_INVALID;
    int rc;
    try {
        rc = compile(h);
    } catch (const std::bad_alloc &) {
        rc = FHE_ERR_INVALID;
    }
    if (rc != FHE_OK) { delete h; return rc; }
    *out = h;
    return FHE_OK;
}
}  // namespace
