// A click log split by time on the GPU (include/serenade_hip.h, "preparing a click log"): srn_events_split and srn_events_take.
//
// The rule needs no order of the rows, only a maximum per session, two counts per item and two counts per session.  Two open-addressing tables on the full 64-bit
// keys (srn_events.h) give every row the slot of its session and of its item once; after that a pass is a gather through two 32-bit slot columns.  Integer atomics
// arrive in any order and give the same sums, so code, pos and info are the same bytes from run to run.
//   k_insert    slots of the row's session and item; last(s) = max time (atomicMax); distinct sessions and items, t_min, t_max
//   k_side      OUT / train side / test side from last(s); train-side rows per item
//   k_rare      RARE from the item's train-side rows; rows left per train session
//   k_train     SHORT_TRAIN from the session's rows left, else TRAIN: the item has a TRAIN row
//   k_unknown   UNKNOWN from the item's TRAIN mark; rows left per test session
//   k_test      SHORT_TEST from the session's rows left, else TEST: the item has a TEST row; (is TRAIN, is TEST) packed for the scan; rows per drop code
//   k_tables    sessions and items of each side, from the slots
//   rocprim::exclusive_scan over the packed pairs (both ranks in one scan: neither half reaches 2^32), k_pos writes pos.
// The item column is Zipf: in k_side a block first adds equal items in a small LDS table (CombTable, srn_events.h) and then adds each LDS entry once.
// SRN_SPLIT_NO_COMBINE=1 takes the plain form; tools/prepare_bench.py measures both (config 3's 60.6 M rows: 17.1 ms against 61.0 ms for the whole split, profiles/prepare_cfg3.json).
//
// Scratch, allocated for the call and released: with T = the power of two >= 2 n (at least 64, at most 2^31) slots per table,
//   36 (T + 1) bytes of tables (session: key 8, last 8, rows left 4; item: key 8, train-side rows 4, marks 4), 8 n of slot columns, 16 (n + 1) for the scan and its
//   result, rocPRIM's scan storage and 128 bytes of counters: between 96 n and 168 n bytes.  Host arrays add 24 n for the uploaded rows and 5 n for code and pos.
#include <cstring>   // rocprim's texture iterator calls the host memset
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <string>

#include "srn_internal.h"
#include "srn_hipsync.h"
#include "srn_events.h"

namespace srn {

#define SPLIT_TRY(expr)                                                                                 \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(SRN_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace {

constexpr int TPB = 256;                      // 4 waves
constexpr unsigned kMaxBlocks = 2048;         // grid-stride loops: a block's counts leave it as one atomic per counter
constexpr uint32_t kNoPos = 0xFFFFFFFFu;

enum : uint8_t { kTrain = SRN_SPLIT_TRAIN, kTest = SRN_SPLIT_TEST, kOut = SRN_SPLIT_OUT, kRare = SRN_SPLIT_RARE, kShortTrain = SRN_SPLIT_SHORT_TRAIN,
                 kUnknown = SRN_SPLIT_UNKNOWN, kShortTest = SRN_SPLIT_SHORT_TEST };
// counters
enum { C_SESSIONS = 0, C_ITEMS, C_TMIN, C_TMAX, C_FULL, C_TRAIN_SESSIONS, C_TEST_SESSIONS, C_TRAIN_ITEMS, C_TEST_ITEMS, C_DROP /* + code - 16, 5 of them */, C_N = 16 };

struct Tables {
    KeyTable sess, item;
    unsigned long long* sess_last;   // largest time of the session
    uint32_t* sess_left;             // rows of the session no step has dropped yet (a session is on one side)
    uint32_t* item_train;            // train-side rows of the item
    uint32_t* item_marks;            // bit 0: the item has a TRAIN row, bit 1: a TEST row
};
struct Rule { uint64_t cutoff, start, end; uint32_t S, L; bool known; };

__device__ inline uint8_t side_of(const Rule& r, uint64_t last) {
    if (last < r.start || (r.end && last >= r.end)) return kOut;
    return last >= r.cutoff ? kTest : kTrain;
}
__device__ inline unsigned long long block_sum(unsigned long long v, unsigned long long* lds) {   // the sum in thread 0
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x / 64] = v;
    __syncthreads();
    unsigned long long t = 0;
    for (int i = 0; i < TPB / 64; ++i) t += lds[i];
    return t;
}
__device__ inline unsigned long long block_max(unsigned long long v, unsigned long long* lds) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x / 64] = v;
    __syncthreads();
    unsigned long long t = 0;
    for (int i = 0; i < TPB / 64; ++i) t = max(t, lds[i]);
    return t;
}

__global__ void __launch_bounds__(TPB) k_insert(const uint64_t* __restrict__ sess, const uint64_t* __restrict__ item, const void* __restrict__ times, bool i64, uint64_t n,
                                                Tables T, uint32_t* __restrict__ sslot, uint32_t* __restrict__ islot, unsigned long long* ctr) {
    __shared__ unsigned long long lds[TPB / 64];
    unsigned long long ns = 0, ni = 0, tmin = ~0ull, tmax = 0, full = 0;
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t t = event_time(times, i64, j);
        tmin = min(tmin, (unsigned long long)t); tmax = max(tmax, (unsigned long long)t);
        bool fresh;
        uint32_t s = key_table_insert(T.sess, sess[j], &fresh); ns += fresh;
        uint32_t i = key_table_insert(T.item, item[j], &fresh); ni += fresh;
        if (s == kNone || i == kNone) { full = 1; s = i = 0; }   // (slot 0 keeps the later passes inside the tables; the call fails)
        else atomicMax(&T.sess_last[s], (unsigned long long)t);
        sslot[j] = s; islot[j] = i;
    }
    ns = block_sum(ns, lds); ni = block_sum(ni, lds); full = block_sum(full, lds);
    tmax = block_max(tmax, lds); tmin = ~block_max(~tmin, lds);
    if (threadIdx.x == 0) {
        if (ns) atomicAdd(&ctr[C_SESSIONS], ns);
        if (ni) atomicAdd(&ctr[C_ITEMS], ni);
        if (full) atomicAdd(&ctr[C_FULL], full);
        atomicMin(&ctr[C_TMIN], tmin); atomicMax(&ctr[C_TMAX], tmax);
    }
}

template <bool COMBINE>
__global__ void __launch_bounds__(TPB) k_side(const uint32_t* __restrict__ sslot, const uint32_t* __restrict__ islot, uint64_t n, Tables T, Rule r, uint8_t* __restrict__ code) {
    __shared__ CombTable comb;
    if (COMBINE) comb_init(comb);
    for (uint64_t base = blockIdx.x * (uint64_t)kCombTile; base < n; base += (uint64_t)gridDim.x * kCombTile) {   // whole blocks stay in the loop together
        for (uint32_t q = 0; q < kCombTile / TPB; ++q) {
            const uint64_t j = base + q * TPB + threadIdx.x;
            if (j >= n) break;
            const uint8_t c = side_of(r, T.sess_last[sslot[j]]);
            code[j] = c;
            if (c != kTrain) continue;
            if (COMBINE) comb_add(comb, T.item_train, islot[j]);
            else atomicAdd(&T.item_train[islot[j]], 1u);
        }
        if (COMBINE) comb_flush(comb, T.item_train);
    }
}

__global__ void __launch_bounds__(TPB) k_rare(const uint32_t* __restrict__ sslot, const uint32_t* __restrict__ islot, uint64_t n, Tables T, Rule r, uint8_t* __restrict__ code) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
        if (code[j] != kTrain) continue;
        if (T.item_train[islot[j]] < r.S) code[j] = kRare;
        else atomicAdd(&T.sess_left[sslot[j]], 1u);
    }
}
__global__ void __launch_bounds__(TPB) k_train(const uint32_t* __restrict__ sslot, const uint32_t* __restrict__ islot, uint64_t n, Tables T, Rule r, uint8_t* __restrict__ code) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
        if (code[j] != kTrain) continue;
        if (T.sess_left[sslot[j]] < r.L) { code[j] = kShortTrain; continue; }
        uint32_t* m = &T.item_marks[islot[j]];
        if (!(__hip_atomic_load(m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u)) atomicOr(m, 1u);   // (a popular item is marked once and read from then on)
    }
}
__global__ void __launch_bounds__(TPB) k_unknown(const uint32_t* __restrict__ sslot, const uint32_t* __restrict__ islot, uint64_t n, Tables T, Rule r, uint8_t* __restrict__ code) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
        if (code[j] != kTest) continue;
        if (r.known && !(T.item_marks[islot[j]] & 1u)) code[j] = kUnknown;
        else atomicAdd(&T.sess_left[sslot[j]], 1u);
    }
}
// ... and every code is final: pair[j] = (is TRAIN, is TEST << 32), pair[n] = 0 (the scan's total), rows per drop code
__global__ void __launch_bounds__(TPB) k_test(const uint32_t* __restrict__ sslot, const uint32_t* __restrict__ islot, uint64_t n, Tables T, Rule r, uint8_t* __restrict__ code,
                                              unsigned long long* __restrict__ pair, unsigned long long* ctr) {
    __shared__ unsigned long long lds[TPB / 64];
    unsigned long long drop[5] = {0, 0, 0, 0, 0};
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j <= n; j += (uint64_t)gridDim.x * blockDim.x) {
        if (j == n) { pair[j] = 0; continue; }
        uint8_t c = code[j];
        if (c == kTest) {
            if (T.sess_left[sslot[j]] < r.L) { c = kShortTest; code[j] = c; }
            else {
                uint32_t* m = &T.item_marks[islot[j]];
                if (!(__hip_atomic_load(m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2u)) atomicOr(m, 2u);
            }
        }
        pair[j] = c == kTrain ? 1ull : c == kTest ? 1ull << 32 : 0ull;
        if (c >= kOut) ++drop[c - kOut];
    }
    for (int d = 0; d < 5; ++d) {
        const unsigned long long t = block_sum(drop[d], lds);
        if (threadIdx.x == 0 && t) atomicAdd(&ctr[C_DROP + d], t);
    }
}
// slot mask + 1 of a table is the key ~0's: taken iff its key word is 0
__device__ inline bool slot_taken(const KeyTable& t, uint64_t e) { return e == (uint64_t)t.mask + 1 ? t.keys[e] == 0 : t.keys[e] != kEmptyKey; }
__global__ void __launch_bounds__(TPB) k_tables(Tables T, Rule r, unsigned long long* ctr) {
    __shared__ unsigned long long lds[TPB / 64];
    unsigned long long trs = 0, tes = 0, tri = 0, tei = 0;
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e <= (uint64_t)T.sess.mask + 1; e += (uint64_t)gridDim.x * blockDim.x) {
        if (!slot_taken(T.sess, e) || T.sess_left[e] < r.L) continue;   // (L >= 1: a session without rows left counts nowhere)
        const uint8_t c = side_of(r, T.sess_last[e]);
        trs += c == kTrain; tes += c == kTest;
    }
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e <= (uint64_t)T.item.mask + 1; e += (uint64_t)gridDim.x * blockDim.x) {
        if (!slot_taken(T.item, e)) continue;
        const uint32_t m = T.item_marks[e];
        tri += m & 1u; tei += (m >> 1) & 1u;
    }
    trs = block_sum(trs, lds); tes = block_sum(tes, lds); tri = block_sum(tri, lds); tei = block_sum(tei, lds);
    if (threadIdx.x == 0) {
        if (trs) atomicAdd(&ctr[C_TRAIN_SESSIONS], trs);
        if (tes) atomicAdd(&ctr[C_TEST_SESSIONS], tes);
        if (tri) atomicAdd(&ctr[C_TRAIN_ITEMS], tri);
        if (tei) atomicAdd(&ctr[C_TEST_ITEMS], tei);
    }
}
__global__ void __launch_bounds__(TPB) k_pos(const uint8_t* __restrict__ code, const unsigned long long* __restrict__ rank, uint64_t n, uint32_t* __restrict__ pos) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t c = code[j];
        pos[j] = c == kTrain ? (uint32_t)rank[j] : c == kTest ? (uint32_t)(rank[j] >> 32) : kNoPos;
    }
}
// row j goes to pos[j]
__global__ void __launch_bounds__(TPB) k_take(const uint8_t* __restrict__ code, const uint32_t* __restrict__ pos, uint64_t n, uint8_t which, const uint64_t* __restrict__ s,
                                              const uint64_t* __restrict__ i, const uint64_t* __restrict__ t, uint64_t* __restrict__ os, uint64_t* __restrict__ oi, uint64_t* __restrict__ ot) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x)
        if (code[j] == which) { const uint32_t p = pos[j]; os[p] = s[j]; oi[p] = i[j]; ot[p] = t[j]; }
}

inline dim3 grid_for(uint64_t n, uint64_t per_block = TPB) { return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + per_block - 1) / per_block, kMaxBlocks))); }

// SRN_SPLIT_HASH_BITS (tests): the tables' hash cut to this many bits; SRN_SPLIT_NO_COMBINE (measurements): k_side's plain form
std::once_flag g_knob_once; uint32_t g_hash_bits = 0; bool g_no_combine = false;
void read_knobs() {
    const char* e = getenv("SRN_SPLIT_HASH_BITS");
    g_hash_bits = e ? (uint32_t)std::min(32l, std::max(0l, atol(e))) : 0;
    e = getenv("SRN_SPLIT_NO_COMBINE");
    g_no_combine = e && *e && *e != '0';
}

}  // namespace

void split_reload_knobs() { std::call_once(g_knob_once, read_knobs); read_knobs(); }
uint32_t split_hash_bits() { std::call_once(g_knob_once, read_knobs); return g_hash_bits; }

int events_split(const uint64_t* sess, const uint64_t* item, const void* times, size_t n, unsigned flags, const srn_split_t& sp, int device, void* stream,
                 uint8_t* code, uint32_t* pos, srn_split_info_t* info) {
    std::call_once(g_knob_once, read_knobs);
    const bool on_device = flags & SRN_EVENTS_DEVICE, i64 = flags & SRN_EVENTS_TIME_I64;
    if (on_device) {
        int rc;
        if ((rc = check_device_rows(sess, device, "session_ids")) || (rc = check_device_rows(item, device, "item_ids")) || (rc = check_device_rows(times, device, "times")) ||
            (rc = check_device_rows(code, device, "code")) || (rc = check_device_rows(pos, device, "pos"))) return rc;
    }
    SPLIT_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    DevBuf u_s, u_i, u_t, u_code, u_pos;
    const uint64_t* ps = sess; const uint64_t* pi = item; const void* pt = times; uint8_t* pcode = code; uint32_t* ppos = pos;
    if (!on_device) {
        SPLIT_TRY(u_s.alloc(n * 8)); SPLIT_TRY(u_i.alloc(n * 8)); SPLIT_TRY(u_t.alloc(n * 8)); SPLIT_TRY(u_code.alloc(n)); SPLIT_TRY(u_pos.alloc(n * 4));
        SPLIT_TRY(hipMemcpyAsync(u_s.p, sess, n * 8, hipMemcpyHostToDevice, st));
        SPLIT_TRY(hipMemcpyAsync(u_i.p, item, n * 8, hipMemcpyHostToDevice, st));
        SPLIT_TRY(hipMemcpyAsync(u_t.p, times, n * 8, hipMemcpyHostToDevice, st));
        ps = u_s.as<uint64_t>(); pi = u_i.as<uint64_t>(); pt = u_t.p; pcode = u_code.as<uint8_t>(); ppos = u_pos.as<uint32_t>();
    }
    const uint32_t slots = key_table_slots(n);
    const uint64_t T1 = (uint64_t)slots + 1;
    DevBuf skeys, slast, sleft, ikeys, itrain, imarks, sslot, islot, pair, rank, ctr, tmp;
    SPLIT_TRY(skeys.alloc(T1 * 8)); SPLIT_TRY(slast.alloc(T1 * 8)); SPLIT_TRY(sleft.alloc(T1 * 4));
    SPLIT_TRY(ikeys.alloc(T1 * 8)); SPLIT_TRY(itrain.alloc(T1 * 4)); SPLIT_TRY(imarks.alloc(T1 * 4));
    SPLIT_TRY(sslot.alloc(n * 4)); SPLIT_TRY(islot.alloc(n * 4)); SPLIT_TRY(pair.alloc((n + 1) * 8)); SPLIT_TRY(rank.alloc((n + 1) * 8)); SPLIT_TRY(ctr.alloc(C_N * 8));
    size_t tb = 0;
    SPLIT_TRY(rocprim::exclusive_scan(nullptr, tb, pair.as<unsigned long long>(), rank.as<unsigned long long>(), 0ull, n + 1, rocprim::plus<unsigned long long>(), st));
    SPLIT_TRY(tmp.alloc(tb));
    SPLIT_TRY(hipMemsetAsync(skeys.p, 0xFF, T1 * 8, st)); SPLIT_TRY(hipMemsetAsync(ikeys.p, 0xFF, T1 * 8, st));
    SPLIT_TRY(hipMemsetAsync(slast.p, 0, T1 * 8, st)); SPLIT_TRY(hipMemsetAsync(sleft.p, 0, T1 * 4, st));
    SPLIT_TRY(hipMemsetAsync(itrain.p, 0, T1 * 4, st)); SPLIT_TRY(hipMemsetAsync(imarks.p, 0, T1 * 4, st));
    SPLIT_TRY(hipMemsetAsync(ctr.p, 0, C_N * 8, st));
    unsigned long long* c = ctr.as<unsigned long long>();
    SPLIT_TRY(hipMemsetAsync(c + C_TMIN, 0xFF, 8, st));
    Tables T{KeyTable{skeys.as<unsigned long long>(), slots - 1, g_hash_bits}, KeyTable{ikeys.as<unsigned long long>(), slots - 1, g_hash_bits},
             slast.as<unsigned long long>(), sleft.as<uint32_t>(), itrain.as<uint32_t>(), imarks.as<uint32_t>()};
    const Rule r{sp.cutoff, sp.start, sp.end, std::max(sp.min_item_support, 1u), std::max(sp.min_session_len, 1u), (sp.flags & SRN_SPLIT_TEST_KNOWN_ITEMS) != 0};
    const uint64_t N = n;
    uint32_t* ss = sslot.as<uint32_t>(); uint32_t* is = islot.as<uint32_t>();
    hipLaunchKernelGGL(k_insert, grid_for(N), dim3(TPB), 0, st, ps, pi, pt, i64, N, T, ss, is, c);
    if (g_no_combine) hipLaunchKernelGGL(k_side<false>, grid_for(N, kCombTile), dim3(TPB), 0, st, ss, is, N, T, r, pcode);
    else hipLaunchKernelGGL(k_side<true>, grid_for(N, kCombTile), dim3(TPB), 0, st, ss, is, N, T, r, pcode);
    hipLaunchKernelGGL(k_rare, grid_for(N), dim3(TPB), 0, st, ss, is, N, T, r, pcode);
    hipLaunchKernelGGL(k_train, grid_for(N), dim3(TPB), 0, st, ss, is, N, T, r, pcode);
    hipLaunchKernelGGL(k_unknown, grid_for(N), dim3(TPB), 0, st, ss, is, N, T, r, pcode);
    hipLaunchKernelGGL(k_test, grid_for(N + 1), dim3(TPB), 0, st, ss, is, N, T, r, pcode, pair.as<unsigned long long>(), c);
    hipLaunchKernelGGL(k_tables, grid_for(T1), dim3(TPB), 0, st, T, r, c);
    SPLIT_TRY(hipGetLastError());
    SPLIT_TRY(rocprim::exclusive_scan(tmp.p, tb, pair.as<unsigned long long>(), rank.as<unsigned long long>(), 0ull, n + 1, rocprim::plus<unsigned long long>(), st));
    hipLaunchKernelGGL(k_pos, grid_for(N), dim3(TPB), 0, st, pcode, rank.as<unsigned long long>(), N, ppos);
    SPLIT_TRY(hipGetLastError());
    unsigned long long h[C_N], total = 0;
    SPLIT_TRY(hipMemcpyAsync(h, ctr.p, sizeof h, hipMemcpyDeviceToHost, st));
    SPLIT_TRY(hipMemcpyAsync(&total, rank.as<unsigned long long>() + n, 8, hipMemcpyDeviceToHost, st));
    if (!on_device) {
        SPLIT_TRY(hipMemcpyAsync(code, pcode, n, hipMemcpyDeviceToHost, st));
        SPLIT_TRY(hipMemcpyAsync(pos, ppos, n * 4, hipMemcpyDeviceToHost, st));
    }
    SPLIT_TRY(hipStreamSynchronize(st));
    if (h[C_FULL]) return fail(SRN_ERANGE, "the split's key tables are full: more distinct sessions or items than their 2^31 slots");
    srn_split_info_t o{};
    o.train_rows = total & 0xFFFFFFFFull; o.train_sessions = h[C_TRAIN_SESSIONS]; o.train_items = h[C_TRAIN_ITEMS];
    o.test_rows = total >> 32; o.test_sessions = h[C_TEST_SESSIONS]; o.test_items = h[C_TEST_ITEMS];
    o.dropped_out = h[C_DROP]; o.dropped_rare = h[C_DROP + 1]; o.dropped_short_train = h[C_DROP + 2]; o.dropped_unknown = h[C_DROP + 3]; o.dropped_short_test = h[C_DROP + 4];
    o.sessions = h[C_SESSIONS]; o.items = h[C_ITEMS]; o.t_min = h[C_TMIN]; o.t_max = h[C_TMAX];
    *info = o;
    return SRN_OK;
}

int events_take(const uint8_t* code, const uint32_t* pos, size_t n, uint8_t which, const uint64_t* sess, const uint64_t* item, const void* times, unsigned flags,
                uint64_t* out_s, uint64_t* out_i, void* out_t, int device, void* stream) {
    if (!(flags & SRN_EVENTS_DEVICE)) {   // host memory in, host memory out: the same scatter as a loop
        const uint64_t* t = (const uint64_t*)times; uint64_t* ot = (uint64_t*)out_t;
        for (size_t j = 0; j < n; ++j)
            if (code[j] == which) { const uint32_t p = pos[j]; out_s[p] = sess[j]; out_i[p] = item[j]; ot[p] = t[j]; }
        return SRN_OK;
    }
    for (const void* p : {(const void*)code, (const void*)pos, (const void*)sess, (const void*)item, times, (const void*)out_s, (const void*)out_i, (const void*)out_t}) {
        const int rc = check_device_rows(p, device, "an array of srn_events_take");
        if (rc) return rc;
    }
    SPLIT_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(k_take, grid_for(n), dim3(TPB), 0, (hipStream_t)stream, code, pos, (uint64_t)n, which, sess, item, (const uint64_t*)times, out_s, out_i, (uint64_t*)out_t);
    SPLIT_TRY(hipGetLastError());
    return SRN_OK;
}

}  // namespace srn
