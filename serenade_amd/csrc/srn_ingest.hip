// Training data on the GPU: read_from_file (src/vmisknn/vmis_index.rs:591-686) with the device doing the parsing and the grouping.
//
// Grouping (group_rows_device), in closed form.  Input: n rows (session, item, time) in file order, time already rounded.  read_from_file
// stable-sorts the rows by session (:620-621) and walks them once (:660-686).  Its loop never adds the row it ends on -- that row opens a
// session which is never pushed (:669, :675-686) -- so, writing "last" for the last in stable session order:
//   * the row that is last in stable session order is dropped: the last row, in file order, of the largest session id (n == 1: no sessions);
//   * a row survives iff it is the first, in file order, with its (session, item) pair (the `contains` test, :670);
//   * a session's items are its surviving items in ascending order (:676);
//   * a session's ts is the low 32 bits of the max time over its surviving rows (only non-duplicate rows move the max, :670-673);
//   * sessions come out in ascending session id.
// On the device: two stable LSD radix sorts carry the row index (by item, then by session), so the rows stand in (session, item, file
// order); k_mark keeps the heads of the (session, item) runs except the dropped row; a scan compacts them; a scan of the session heads
// gives the offsets; k_session_max takes the max time per session (a wave-segmented max, then one atomic per session and wave).
//
// Parsing (tsv_rows_device: shared by sessions_from_tsv_gpu, which groups the rows, and events_from_tsv_gpu, which hands them out).  The host reads the file in chunks into two pinned staging buffers and uploads one while it reads the
// next; a chunk ends at its last '\n' and the tail is carried into the next.  Per chunk: k_nl_count / k_nl_ends find the line ends with a
// wave64 ballot per 64 bytes plus a scan over 4 KiB tiles; k_row_count / k_row_scatter parse one line per thread, mirroring parse_line
// (srn_index.cpp) exactly for the ids and the field structure, and compact the kept lines into the row arrays in file order.  The time
// field is certified on the device only in the form [+-]?digits[.digits][(e|E)[+-]?digits] with <= 19 significant digits, significand
// <= 2^53 and |exp10| <= 22: one correctly rounded f64 multiply or divide by an exact power of ten, i.e. strtod's value.  Every other
// time field (hex floats, inf / nan, leading whitespace, long significands, large exponents, a field past the 63 bytes the host copies,
// trailing characters) is left to the host: the line's slot holds (file offset, length, kFallback) and parse_tsv_line re-reads the line
// from the file after the last chunk, so file order -- and with it the stable sort -- is untouched.
#include <cstring>   // rocprim's texture iterator calls the host memset
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "srn_internal.h"
#include "srn_hipsync.h"
#include "srn_events.h"

namespace srn {

#define ING_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(SRN_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace {

constexpr uint64_t kFallback = ~0ull;          // time of a row slot the host parses (never a parsed time: those are < 2^63 or llround's 2^63)
constexpr int TPB = 256;                       // 4 waves
constexpr uint32_t kByteTile = 4096;           // bytes per block of the line-end kernels: 16 ballots of 64 bytes per wave
constexpr uint32_t kLineTile = 1024;           // lines per block of the parse kernels: 4 rounds of 256
constexpr size_t kDefaultChunk = 32u << 20;

struct PinnedBuf {
    void* p = nullptr;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t bytes) { if (p) { (void)hipHostFree(p); p = nullptr; } return hipHostMalloc(&p, std::max<size_t>(bytes, 16), hipHostMallocDefault); }
    char* c() const { return (char*)p; }
};

inline dim3 grid_for(uint64_t n) { return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + TPB - 1) / TPB, 1u << 16))); }
inline int bits_of(uint64_t v) { int b = 0; while (v) { ++b; v >>= 1; } return std::max(b, 1); }
__device__ inline uint32_t lane_id() { return __lane_id(); }
__device__ inline uint32_t rank_below(unsigned long long mask) { return (uint32_t)__popcll(mask & ((1ull << lane_id()) - 1ull)); }

// ---------------------------------------------------------------------------------------------
// grouping
// ---------------------------------------------------------------------------------------------
__global__ void k_item_keys(const uint64_t* item, uint64_t n, uint64_t* key, uint32_t* idx) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) { key[j] = item[j]; idx[j] = (uint32_t)j; }
}
__global__ void k_gather_u64(const uint64_t* src, const uint32_t* idx, uint64_t n, uint64_t* out) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) out[j] = src[idx[j]];
}
// the reductions below run on a grid of at most kReduceBlocks blocks and take one atomic per block (one per wave on a full grid is
// 2^18 atomics on one address: 6 ms at 60 M rows)
constexpr unsigned kReduceBlocks = 1024;
__device__ inline unsigned long long block_max(unsigned long long v, unsigned long long* lds) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    if (lane_id() == 0) lds[threadIdx.x / 64] = v;
    __syncthreads();
    for (int i = 0; i < TPB / 64; ++i) v = max(v, lds[i]);
    return v;
}
// largest session id and item id (the sorts' bit widths)
__global__ void k_max2(const uint64_t* a, const uint64_t* b, uint64_t n, unsigned long long* out2) {
    __shared__ unsigned long long lds[2][TPB / 64];
    unsigned long long ma = 0, mb = 0;
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) { ma = max(ma, (unsigned long long)a[j]); mb = max(mb, (unsigned long long)b[j]); }
    ma = block_max(ma, lds[0]); mb = block_max(mb, lds[1]);
    if (threadIdx.x == 0) { atomicMax(&out2[0], ma); atomicMax(&out2[1], mb); }
}
// the dropped row: the largest row index among the rows of the largest session id (the tail of the session-sorted order)
__global__ void k_drop_row(const uint64_t* sess_sorted, const uint32_t* idx, uint64_t n, unsigned* drop) {
    __shared__ unsigned long long lds[TPB / 64];
    const uint64_t last = sess_sorted[n - 1];
    unsigned long long m = 0;
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x)
        if (sess_sorted[j] == last) m = max(m, (unsigned long long)idx[j]);
    m = block_max(m, lds);
    if (threadIdx.x == 0 && m) atomicMax(drop, (unsigned)m);
}
// rows in (session, item, file order): keep the head of each (session, item) run unless it is the dropped row.  The dropped row is the
// last in file order of its session, so it heads its run only when it is alone in it.  flag[n] = 0 (the scan's total).
__global__ void k_mark(const uint64_t* sess_sorted, const uint64_t* item_sorted, const uint32_t* idx, uint64_t n, const unsigned* drop, uint32_t* flag) {
    const unsigned d = *drop;
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j <= n; j += (uint64_t)gridDim.x * blockDim.x) {
        if (j == n) { flag[j] = 0; continue; }
        const bool head = j == 0 || sess_sorted[j] != sess_sorted[j - 1] || item_sorted[j] != item_sorted[j - 1];
        flag[j] = head && idx[j] != d ? 1u : 0u;
    }
}
__global__ void k_compact_rows(const uint64_t* sess_sorted, const uint64_t* item_sorted, const uint32_t* idx, const uint64_t* time, const uint32_t* flag,
                               const uint32_t* pos, uint64_t n, uint64_t* c_sess, uint64_t* c_item, uint64_t* c_time) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x)
        if (flag[j]) { const uint32_t p = pos[j]; c_sess[p] = sess_sorted[j]; c_item[p] = item_sorted[j]; c_time[p] = time[idx[j]]; }
}
// session heads of the surviving rows; flag[m] = 0
__global__ void k_session_heads(const uint64_t* c_sess, uint64_t m, uint32_t* head) {
    for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k <= m; k += (uint64_t)gridDim.x * blockDim.x)
        head[k] = k < m && (k == 0 || c_sess[k] != c_sess[k - 1]) ? 1u : 0u;
}
__global__ void k_session_off(const uint32_t* head, const uint32_t* sid, const uint64_t* c_sess, uint64_t m, uint64_t* off, uint64_t* session_ids) {
    for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k <= m; k += (uint64_t)gridDim.x * blockDim.x)
        if (k == m || head[k]) {   // sid = exclusive scan of head: the session a head opens; sid[m] = number of sessions
            off[sid[k]] = k;
            if (k < m) session_ids[sid[k]] = c_sess[k];
        }
}
// max time per session: a segmented inclusive max across the wave (a session's rows are contiguous), then one atomic per (session, wave)
__global__ void k_session_max(const uint32_t* head, const uint32_t* sid, const uint64_t* c_time, uint64_t m, unsigned long long* ts64) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k0 = blockIdx.x * (uint64_t)blockDim.x; k0 < m; k0 += stride) {   // whole waves stay in the loop together (the shuffles)
        const uint64_t k = k0 + threadIdx.x;
        const bool in = k < m;
        const uint32_t s = in ? sid[k] + head[k] - 1 : 0xFFFFFFFFu;
        unsigned long long v = in ? c_time[k] : 0;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long ov = __shfl_up(v, o);
            const uint32_t os = __shfl_up(s, o);
            if (lane_id() >= (uint32_t)o && os == s) v = max(v, ov);
        }
        const uint32_t ns = __shfl_down(s, 1);
        if (in && (lane_id() == 63 || ns != s)) atomicMax(&ts64[s], v);
    }
}
__global__ void k_low32(const unsigned long long* in, uint64_t n, uint32_t* out) {
    for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s < n; s += (uint64_t)gridDim.x * blockDim.x) out[s] = (uint32_t)in[s];
}

// ---------------------------------------------------------------------------------------------
// parsing
// ---------------------------------------------------------------------------------------------
__device__ const double kPow10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16,
                                      1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
__device__ inline bool is_digit(unsigned char c) { return c >= '0' && c <= '9'; }

// One line [p, end) without its '\n'.  0: skipped (the host's parse_line returns false), 1: a row, 2: the host parses the time field.
__device__ int parse_line_dev(const unsigned char* p, const unsigned char* end, uint64_t& s, uint64_t& it, uint64_t& t) {
    if (p >= end || !is_digit(*p)) return 0;
    s = 0; while (p < end && is_digit(*p)) s = s * 10 + (uint64_t)(*p++ - '0');
    if (p >= end || *p != '\t') return 0; ++p;
    if (p >= end || !is_digit(*p)) return 0;
    it = 0; while (p < end && is_digit(*p)) it = it * 10 + (uint64_t)(*p++ - '0');
    if (p >= end || *p != '\t') return 0; ++p;
    if (p >= end) return 0;                       // empty field: strtod consumes nothing
    if (end - p > 63) return 2;                   // the host copies 63 bytes of the field: let it decide what they hold
    bool neg = false;
    if (*p == '+' || *p == '-') { neg = *p == '-'; ++p; }
    uint64_t mant = 0; int sig = 0, nd = 0, frac = 0;
    while (p < end && is_digit(*p)) { const int d = *p++ - '0'; ++nd; if (sig || d) { if (sig < 19) mant = mant * 10 + (uint64_t)d; ++sig; } }
    if (nd == 0) return 2;                        // ".5", inf, nan, leading whitespace, garbage
    if (p < end && *p == '.') {
        if (p + 1 >= end || !is_digit(p[1])) return 2;   // "5." and the like
        ++p;
        while (p < end && is_digit(*p)) { const int d = *p++ - '0'; ++frac; if (sig || d) { if (sig < 19) mant = mant * 10 + (uint64_t)d; ++sig; } }
    }
    int e = 0;
    if (p < end && (*p == 'e' || *p == 'E')) {
        const unsigned char* q = p + 1; bool eneg = false;
        if (q < end && (*q == '+' || *q == '-')) { eneg = *q == '-'; ++q; }
        if (q >= end || !is_digit(*q)) return 2;
        int ev = 0; while (q < end && is_digit(*q)) { if (ev < 100000) ev = ev * 10 + (*q - '0'); ++q; }
        e = eneg ? -ev : ev; p = q;
    }
    while (p < end && (*p == ' ' || *p == '\r')) ++p;
    if (p < end && *p != '\t' && *p != '\0') return 2;   // (the host's buffer ends at a NUL byte)
    if (sig > 19) return 2;
    // the digits of both parts, read as one integer, are mant (leading zeros add nothing): the value is mant * 10^(e - frac)
    const int e10 = e - frac;
    if (mant == 0) { t = 0; return 1; }
    if (mant > (1ull << 53) || e10 > 22 || e10 < -22) return 2;
    double v = (double)mant;
    v = e10 >= 0 ? v * kPow10[e10] : v / kPow10[-e10];
    if (neg) v = -v;
    if (v >= 9223372036854775808.0) return 2;     // llround undefined there: the host's value, whatever it is
    t = round_time(v);
    return 1;
}

// '\n' per 4 KiB tile; cnt[n_tiles] = 0 (the scan's total)
__global__ void k_nl_count(const unsigned char* text, uint64_t len, uint32_t* cnt) {
    __shared__ uint32_t wsum[TPB / 64];
    const uint32_t w = threadIdx.x / 64;
    const uint64_t base = blockIdx.x * (uint64_t)kByteTile + w * 1024ull;
    uint32_t c = 0;
    for (int step = 0; step < 16; ++step) {
        const uint64_t pos = base + step * 64 + lane_id();
        c += (uint32_t)__popcll(__ballot(pos < len && text[pos] == '\n'));
    }
    if (lane_id() == 0) wsum[w] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0; for (int i = 0; i < TPB / 64; ++i) t += wsum[i];
        cnt[blockIdx.x] = t;
        if (blockIdx.x == 0) cnt[gridDim.x] = 0;
    }
}
// ends[k] = position of the k-th '\n'
__global__ void k_nl_ends(const unsigned char* text, uint64_t len, const uint32_t* tile_base, uint32_t* ends) {
    __shared__ uint32_t wsum[TPB / 64];
    const uint32_t w = threadIdx.x / 64;
    const uint64_t base = blockIdx.x * (uint64_t)kByteTile + w * 1024ull;
    uint32_t c = 0;
    for (int step = 0; step < 16; ++step) {
        const uint64_t pos = base + step * 64 + lane_id();
        c += (uint32_t)__popcll(__ballot(pos < len && text[pos] == '\n'));
    }
    if (lane_id() == 0) wsum[w] = c;
    __syncthreads();
    uint32_t off = tile_base[blockIdx.x];
    for (uint32_t i = 0; i < w; ++i) off += wsum[i];
    for (int step = 0; step < 16; ++step) {
        const uint64_t pos = base + step * 64 + lane_id();
        const bool nl = pos < len && text[pos] == '\n';
        const unsigned long long m = __ballot(nl);
        if (nl) ends[off + rank_below(m)] = (uint32_t)pos;
        off += (uint32_t)__popcll(m);
    }
}

struct ChunkArgs {
    const unsigned char* text; uint64_t len;
    const uint32_t* ends; const uint32_t* nl_base; uint32_t nl_tiles;   // nl_base[nl_tiles] = number of '\n'
    uint32_t extra;        // 1: the chunk ends with a line that has no '\n' (end of file)
    uint32_t first;        // 1: the chunk's first line is the file's first line (the header: skipped whatever it holds)
    uint64_t file_off;     // file offset of text[0]
};
__device__ inline uint32_t chunk_lines(const ChunkArgs& a) { return a.nl_base[a.nl_tiles] + a.extra; }
__device__ inline int chunk_line(const ChunkArgs& a, uint32_t k, uint64_t& s, uint64_t& it, uint64_t& t) {
    const uint32_t nnl = a.nl_base[a.nl_tiles];
    const uint64_t start = k == 0 ? 0 : (uint64_t)a.ends[k - 1] + 1;
    const uint64_t end = k < nnl ? (uint64_t)a.ends[k] : a.len;
    if (k == 0 && a.first) return 0;
    if (end == start) return 0;
    const int st = parse_line_dev(a.text + start, a.text + end, s, it, t);
    if (st == 2) { s = a.file_off + start; it = end - start; t = kFallback; }
    return st;
}
// kept lines per tile of kLineTile lines; cnt[n_tiles] = 0
__global__ void k_row_count(ChunkArgs a, uint32_t* cnt) {
    __shared__ uint32_t wsum[TPB / 64];
    const uint32_t nl = chunk_lines(a);
    uint32_t c = 0;
    for (uint32_t r = 0; r < kLineTile / TPB; ++r) {
        const uint32_t k = blockIdx.x * kLineTile + r * TPB + threadIdx.x;
        uint64_t s, it, t;
        const bool keep = k < nl && chunk_line(a, k, s, it, t) != 0;
        c += (uint32_t)__popcll(__ballot(keep));
    }
    if (lane_id() == 0) wsum[threadIdx.x / 64] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0; for (int i = 0; i < TPB / 64; ++i) t += wsum[i];
        cnt[blockIdx.x] = t;
        if (blockIdx.x == 0) cnt[gridDim.x] = 0;
    }
}
// the kept lines in file order at rows[*n_rows + tile base + rank]; host-parsed lines are counted
__global__ void k_row_scatter(ChunkArgs a, const uint32_t* tile_base, const unsigned long long* n_rows, uint64_t* rs, uint64_t* ri, uint64_t* rt,
                              unsigned long long* n_fallback) {
    __shared__ uint32_t wsum[TPB / 64];
    const uint32_t nl = chunk_lines(a);
    const uint32_t w = threadIdx.x / 64;
    uint64_t off = *n_rows + tile_base[blockIdx.x];
    for (uint32_t r = 0; r < kLineTile / TPB; ++r) {
        const uint32_t k = blockIdx.x * kLineTile + r * TPB + threadIdx.x;
        uint64_t s = 0, it = 0, t = 0;
        const int st = k < nl ? chunk_line(a, k, s, it, t) : 0;
        const unsigned long long m = __ballot(st != 0);
        const unsigned long long fb = __ballot(st == 2);
        if (lane_id() == 0) { wsum[w] = (uint32_t)__popcll(m); if (fb) atomicAdd(n_fallback, (unsigned long long)__popcll(fb)); }
        __syncthreads();
        uint64_t mine = off; uint32_t round_total = 0;
        for (uint32_t i = 0; i < TPB / 64; ++i) { if (i < w) mine += wsum[i]; round_total += wsum[i]; }
        if (st) { const uint64_t p = mine + rank_below(m); rs[p] = s; ri[p] = it; rt[p] = t; }
        off += round_total;
        __syncthreads();
    }
}
__global__ void k_chunk_done(const uint32_t* nl_base, uint32_t nl_tiles, uint32_t extra, const uint32_t* row_base, uint32_t row_tiles,
                             unsigned long long* n_rows, unsigned long long* n_lines) {
    *n_lines += nl_base[nl_tiles] + extra;
    *n_rows += row_base[row_tiles];
}
// host-parsed slots: collect, then write back what the host made of them (rejected lines keep kFallback and are compacted away)
__global__ void k_fallback_list(const uint64_t* rt, uint64_t n, uint32_t* list, unsigned* cursor) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x)
        if (rt[j] == kFallback) list[atomicAdd(cursor, 1u)] = (uint32_t)j;
}
__global__ void k_fallback_gather(const uint32_t* list, uint64_t nf, const uint64_t* rs, const uint64_t* ri, uint64_t* off_len) {
    for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < nf; q += (uint64_t)gridDim.x * blockDim.x) {
        off_len[2 * q] = rs[list[q]]; off_len[2 * q + 1] = ri[list[q]]; }
}
__global__ void k_fallback_write(const uint32_t* list, uint64_t nf, const uint64_t* vals, uint64_t* rs, uint64_t* ri, uint64_t* rt) {
    for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < nf; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t j = list[q]; rs[j] = vals[3 * q]; ri[j] = vals[3 * q + 1]; rt[j] = vals[3 * q + 2]; }
}
__global__ void k_live(const uint64_t* rt, uint64_t n, uint32_t* flag) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j <= n; j += (uint64_t)gridDim.x * blockDim.x) flag[j] = j < n && rt[j] != kFallback ? 1u : 0u;
}
__global__ void k_compact3(const uint64_t* s, const uint64_t* i, const uint64_t* t, const uint32_t* flag, const uint32_t* pos, uint64_t n,
                           uint64_t* os, uint64_t* oi, uint64_t* ot) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x)
        if (flag[j]) { const uint32_t p = pos[j]; os[p] = s[j]; oi[p] = i[j]; ot[p] = t[j]; }
}
// in-memory events: times as f64 (rounded like the file's) or int64 seconds (negative -> 0)
__global__ void k_times_f64(const double* in, uint64_t n, uint64_t* out) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) out[j] = round_time(in[j]);
}
__global__ void k_times_i64(const int64_t* in, uint64_t n, uint64_t* out) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) out[j] = in[j] < 0 ? 0 : (uint64_t)in[j];
}

template <typename T> hipError_t scan_excl(void* tmp, size_t tb, const T* in, T* out, size_t n, hipStream_t st) {
    return rocprim::exclusive_scan(tmp, tb, in, out, T(0), n, rocprim::plus<T>(), st);
}
template <typename T> size_t scan_bytes(size_t n) {
    size_t tb = 0; (void)rocprim::exclusive_scan(nullptr, tb, (const T*)nullptr, (T*)nullptr, T(0), n, rocprim::plus<T>()); return tb;
}
double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// SRN_INGEST_CHUNK_BYTES: the TSV reader's chunk size, read once (tests force lines across chunk boundaries with a few hundred bytes)
std::once_flag g_chunk_once; size_t g_chunk = kDefaultChunk;
void read_chunk_knob() { const char* e = getenv("SRN_INGEST_CHUNK_BYTES"); g_chunk = e ? (size_t)std::max(64ll, atoll(e)) : kDefaultChunk; }
size_t chunk_bytes() { std::call_once(g_chunk_once, read_chunk_knob); return g_chunk; }

}  // namespace

void ingest_reload_knobs() { std::call_once(g_chunk_once, read_chunk_knob); read_chunk_knob(); }

// rows (device, file order, times rounded) -> sessions on the device
int group_rows_device_core(const uint64_t* sess, const uint64_t* item, const uint64_t* time, size_t n, hipStream_t st, DevSessions& out, srn_load_info_t* info) {
    if (n == 0) return fail(SRN_EINVAL, "no training rows");
    if (n >= 0xFFFFFFFFull) return fail(SRN_ERANGE, "the GPU loader groups < 2^32 rows per call; use the host loader");
    auto t0 = std::chrono::steady_clock::now();
    DevBuf keyA, keyB, idxA, idxB, mx;
    ING_TRY(keyA.alloc(n * 8)); ING_TRY(keyB.alloc(n * 8)); ING_TRY(idxA.alloc(n * 4)); ING_TRY(idxB.alloc(n * 4)); ING_TRY(mx.alloc(16));
    ING_TRY(hipMemsetAsync(mx.p, 0, 16, st));
    hipLaunchKernelGGL(k_max2, dim3(std::min(grid_for(n).x, kReduceBlocks)), dim3(TPB), 0, st, sess, item, (uint64_t)n, mx.as<unsigned long long>());
    unsigned long long maxes[2];
    ING_TRY(hipMemcpyAsync(maxes, mx.p, 16, hipMemcpyDeviceToHost, st));
    ING_TRY(hipStreamSynchronize(st));
    const int sess_bits = bits_of(maxes[0]), item_bits = bits_of(maxes[1]);
    size_t tb = 0, t1 = 0;
    ING_TRY(rocprim::radix_sort_pairs(nullptr, t1, keyA.as<uint64_t>(), keyB.as<uint64_t>(), idxA.as<uint32_t>(), idxB.as<uint32_t>(), n, 0, 64, st)); tb = std::max(tb, t1);
    tb = std::max(tb, scan_bytes<uint32_t>(n + 1));
    DevBuf tmp; ING_TRY(tmp.alloc(tb));
    // 1. stable by item, then stable by session: (session, item, file order)
    hipLaunchKernelGGL(k_item_keys, grid_for(n), dim3(TPB), 0, st, item, (uint64_t)n, keyA.as<uint64_t>(), idxA.as<uint32_t>());
    t1 = tb; ING_TRY(rocprim::radix_sort_pairs(tmp.p, t1, keyA.as<uint64_t>(), keyB.as<uint64_t>(), idxA.as<uint32_t>(), idxB.as<uint32_t>(), n, 0, item_bits, st));
    hipLaunchKernelGGL(k_gather_u64, grid_for(n), dim3(TPB), 0, st, sess, idxB.as<uint32_t>(), (uint64_t)n, keyA.as<uint64_t>());
    t1 = tb; ING_TRY(rocprim::radix_sort_pairs(tmp.p, t1, keyA.as<uint64_t>(), keyB.as<uint64_t>(), idxB.as<uint32_t>(), idxA.as<uint32_t>(), n, 0, sess_bits, st));
    // keyB = sessions, idxA = row index; keyA <- items in that order
    hipLaunchKernelGGL(k_gather_u64, grid_for(n), dim3(TPB), 0, st, item, idxA.as<uint32_t>(), (uint64_t)n, keyA.as<uint64_t>());
    // 2. the dropped row, the surviving rows
    DevBuf drop, flag, pos;
    ING_TRY(drop.alloc(4)); ING_TRY(flag.alloc((n + 1) * 4)); ING_TRY(pos.alloc((n + 1) * 4));
    ING_TRY(hipMemsetAsync(drop.p, 0, 4, st));
    hipLaunchKernelGGL(k_drop_row, dim3(std::min(grid_for(n).x, kReduceBlocks)), dim3(TPB), 0, st, keyB.as<uint64_t>(), idxA.as<uint32_t>(), (uint64_t)n, drop.as<unsigned>());
    hipLaunchKernelGGL(k_mark, grid_for(n + 1), dim3(TPB), 0, st, keyB.as<uint64_t>(), keyA.as<uint64_t>(), idxA.as<uint32_t>(), (uint64_t)n, drop.as<unsigned>(), flag.as<uint32_t>());
    t1 = tb; ING_TRY(scan_excl(tmp.p, t1, flag.as<uint32_t>(), pos.as<uint32_t>(), n + 1, st));
    uint32_t m32 = 0;
    ING_TRY(hipMemcpyAsync(&m32, pos.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, st));
    ING_TRY(hipStreamSynchronize(st));
    const uint64_t m = m32;
    DevBuf c_sess, c_item, c_time;
    ING_TRY(c_sess.alloc(m * 8)); ING_TRY(c_item.alloc(m * 8)); ING_TRY(c_time.alloc(m * 8));
    hipLaunchKernelGGL(k_compact_rows, grid_for(n), dim3(TPB), 0, st, keyB.as<uint64_t>(), keyA.as<uint64_t>(), idxA.as<uint32_t>(), time, flag.as<uint32_t>(),
                       pos.as<uint32_t>(), (uint64_t)n, c_sess.as<uint64_t>(), c_item.as<uint64_t>(), c_time.as<uint64_t>());
    // 3. sessions: heads -> offsets, max time per session
    hipLaunchKernelGGL(k_session_heads, grid_for(m + 1), dim3(TPB), 0, st, c_sess.as<uint64_t>(), m, flag.as<uint32_t>());
    t1 = tb; ING_TRY(scan_excl(tmp.p, t1, flag.as<uint32_t>(), pos.as<uint32_t>(), m + 1, st));
    uint32_t ns32 = 0;
    ING_TRY(hipMemcpyAsync(&ns32, pos.as<uint32_t>() + m, 4, hipMemcpyDeviceToHost, st));
    ING_TRY(hipStreamSynchronize(st));
    const uint64_t ns = ns32;
    DevBuf d_off, d_sid, d_ts64, d_ts;
    ING_TRY(d_off.alloc((ns + 1) * 8)); ING_TRY(d_sid.alloc(ns * 8)); ING_TRY(d_ts64.alloc(ns * 8)); ING_TRY(d_ts.alloc(ns * 4));
    hipLaunchKernelGGL(k_session_off, grid_for(m + 1), dim3(TPB), 0, st, flag.as<uint32_t>(), pos.as<uint32_t>(), c_sess.as<uint64_t>(), m, d_off.as<uint64_t>(), d_sid.as<uint64_t>());
    if (m) {
        ING_TRY(hipMemsetAsync(d_ts64.p, 0, ns * 8, st));
        hipLaunchKernelGGL(k_session_max, grid_for(m), dim3(TPB), 0, st, flag.as<uint32_t>(), pos.as<uint32_t>(), c_time.as<uint64_t>(), m, d_ts64.as<unsigned long long>());
        hipLaunchKernelGGL(k_low32, grid_for(ns), dim3(TPB), 0, st, d_ts64.as<unsigned long long>(), ns, d_ts.as<uint32_t>());
    }
    ING_TRY(hipGetLastError());
    ING_TRY(hipStreamSynchronize(st));
    if (info) info->ms_group = ms_since(t0);
    std::swap(out.off.p, d_off.p); std::swap(out.items.p, c_item.p); std::swap(out.ts.p, d_ts.p); std::swap(out.session_ids.p, d_sid.p);   // (what `out` held before goes with the locals)
    out.n_sessions = ns; out.nnz = m;
    return SRN_OK;
}

// ... -> sessions on the host: the core, then the download
int group_rows_device(const uint64_t* sess, const uint64_t* item, const uint64_t* time, size_t n, hipStream_t st, Sessions& out, srn_load_info_t* info) {
    DevSessions d;
    int rc = group_rows_device_core(sess, item, time, n, st, d, info); if (rc) return rc;
    const uint64_t ns = d.n_sessions, m = d.nnz;
    auto t0 = std::chrono::steady_clock::now();
    out = Sessions();
    out.off.resize(ns + 1); out.items.resize(m); out.ts.resize(ns); out.session_ids.resize(ns);
    ING_TRY(hipMemcpyAsync(out.off.data(), d.off.p, (ns + 1) * 8, hipMemcpyDeviceToHost, st));
    if (m) ING_TRY(hipMemcpyAsync(out.items.data(), d.items.p, m * 8, hipMemcpyDeviceToHost, st));
    if (ns) {
        ING_TRY(hipMemcpyAsync(out.ts.data(), d.ts.p, ns * 4, hipMemcpyDeviceToHost, st));
        ING_TRY(hipMemcpyAsync(out.session_ids.data(), d.session_ids.p, ns * 8, hipMemcpyDeviceToHost, st));
    }
    ING_TRY(hipStreamSynchronize(st));
    if (info) info->ms_download = ms_since(t0);
    return SRN_OK;
}

namespace {
// the rows of an in-memory call on the device, times rounded: host arrays are uploaded once, device arrays read in place
struct EventRows { DevBuf d_s, d_i, d_tin, d_t; const uint64_t* s = nullptr; const uint64_t* i = nullptr; };
int event_rows_device(const uint64_t* sess, const uint64_t* item, const void* times, size_t n, unsigned flags, int device, hipStream_t st, EventRows& r, srn_load_info_t* info) {
    if (n == 0) return fail(SRN_EINVAL, "no training rows");
    if (n >= 0xFFFFFFFFull) return fail(SRN_ERANGE, "the GPU loader groups < 2^32 rows per call; use the host loader");
    ING_TRY(hipSetDevice(device));
    const bool on_device = flags & SRN_EVENTS_DEVICE;
    auto t0 = std::chrono::steady_clock::now();
    DevBuf& d_s = r.d_s; DevBuf& d_i = r.d_i; DevBuf& d_tin = r.d_tin; DevBuf& d_t = r.d_t;
    const uint64_t* ps = sess; const uint64_t* pi = item; const void* pt = times;
    if (!on_device) {
        ING_TRY(d_s.alloc(n * 8)); ING_TRY(d_i.alloc(n * 8)); ING_TRY(d_tin.alloc(n * 8));
        ING_TRY(hipMemcpyAsync(d_s.p, sess, n * 8, hipMemcpyHostToDevice, st));
        ING_TRY(hipMemcpyAsync(d_i.p, item, n * 8, hipMemcpyHostToDevice, st));
        ING_TRY(hipMemcpyAsync(d_tin.p, times, n * 8, hipMemcpyHostToDevice, st));
        ING_TRY(hipStreamSynchronize(st));
        ps = d_s.as<uint64_t>(); pi = d_i.as<uint64_t>(); pt = d_tin.p;
    }
    if (info) info->ms_upload = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    ING_TRY(d_t.alloc(n * 8));
    if (flags & SRN_EVENTS_TIME_I64) hipLaunchKernelGGL(k_times_i64, grid_for(n), dim3(TPB), 0, st, (const int64_t*)pt, (uint64_t)n, d_t.as<uint64_t>());
    else hipLaunchKernelGGL(k_times_f64, grid_for(n), dim3(TPB), 0, st, (const double*)pt, (uint64_t)n, d_t.as<uint64_t>());
    ING_TRY(hipGetLastError());
    ING_TRY(hipStreamSynchronize(st));
    if (info) { info->ms_parse = ms_since(t0); info->lines = n; info->rows = n; }
    r.s = ps; r.i = pi;
    return SRN_OK;
}
}  // namespace

int sessions_from_events(const uint64_t* sess, const uint64_t* item, const void* times, size_t n, unsigned flags, int device, void* stream, Sessions& out,
                         srn_load_info_t* info) {
    EventRows r;
    int rc = event_rows_device(sess, item, times, n, flags, device, (hipStream_t)stream, r, info); if (rc) return rc;
    return group_rows_device(r.s, r.i, r.d_t.as<uint64_t>(), n, (hipStream_t)stream, out, info);
}
int device_sessions_from_events(const uint64_t* sess, const uint64_t* item, const void* times, size_t n, unsigned flags, int device, void* stream, DevSessions& out,
                                srn_load_info_t* info) {
    EventRows r;
    int rc = event_rows_device(sess, item, times, n, flags, device, (hipStream_t)stream, r, info); if (rc) return rc;
    return group_rows_device_core(r.s, r.i, r.d_t.as<uint64_t>(), n, (hipStream_t)stream, out, info);
}

// the file's rows on the device, in file order (what group_rows_device takes); li: lines, rows, skipped, host_parsed and the read / upload / parse times
int tsv_rows_device(const char* path, int device, hipStream_t st, TsvRows& out, srn_load_info_t& li) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(SRN_EIO, std::string("cannot open ") + path);
    struct FdGuard { int fd; ~FdGuard() { close(fd); } } guard{fd};
    struct stat sb;
    if (fstat(fd, &sb) != 0) return fail(SRN_EIO, std::string("cannot stat ") + path);
    const uint64_t file_size = (uint64_t)sb.st_size;
    ING_TRY(hipSetDevice(device));

    // chunk buffers (grown when a line is longer than a chunk)
    size_t cap = std::max<size_t>(64, std::min<size_t>(chunk_bytes(), std::max<uint64_t>(file_size, 64)));
    PinnedBuf stage[2]; DevBuf d_text, d_ends, d_nlcnt, d_nlbase, d_rcnt, d_rbase, d_scan_tmp;
    size_t scan_tb = 0;
    auto alloc_chunk = [&](size_t c) -> int {
        ING_TRY(stage[0].alloc(c)); ING_TRY(stage[1].alloc(c)); ING_TRY(d_text.alloc(c)); ING_TRY(d_ends.alloc((c + 1) * 4));
        const size_t bt = c / kByteTile + 2, lt = (c + 1) / kLineTile + 2;
        ING_TRY(d_nlcnt.alloc(bt * 4)); ING_TRY(d_nlbase.alloc(bt * 4)); ING_TRY(d_rcnt.alloc(lt * 4)); ING_TRY(d_rbase.alloc(lt * 4));
        scan_tb = std::max(scan_bytes<uint32_t>(bt), scan_bytes<uint32_t>(lt));
        ING_TRY(d_scan_tmp.alloc(scan_tb));
        return SRN_OK;
    };
    int rc = alloc_chunk(cap); if (rc) return rc;
    // rows: grown on demand; a kept line holds at least "d\td\tX" and its '\n', so a chunk of `len` bytes adds at most len / 6 + 1 rows
    DevBuf& rs = out.s; DevBuf& ri = out.i; DevBuf& rt = out.t;
    DevBuf counters;   // n_rows, n_lines, n_fallback
    uint64_t rcap = file_size / 24 + 2 * (cap / 6 + 1) + 16;
    ING_TRY(rs.alloc(rcap * 8)); ING_TRY(ri.alloc(rcap * 8)); ING_TRY(rt.alloc(rcap * 8)); ING_TRY(counters.alloc(24));
    ING_TRY(hipMemsetAsync(counters.p, 0, 24, st));
    unsigned long long* d_nrows = counters.as<unsigned long long>();
    auto grow_rows = [&](uint64_t need) -> int {
        const uint64_t nc = std::max(need, rcap * 3 / 2);
        DevBuf a, b, c; ING_TRY(a.alloc(nc * 8)); ING_TRY(b.alloc(nc * 8)); ING_TRY(c.alloc(nc * 8));
        ING_TRY(hipMemcpyAsync(a.p, rs.p, rcap * 8, hipMemcpyDeviceToDevice, st)); ING_TRY(hipMemcpyAsync(b.p, ri.p, rcap * 8, hipMemcpyDeviceToDevice, st));
        ING_TRY(hipMemcpyAsync(c.p, rt.p, rcap * 8, hipMemcpyDeviceToDevice, st));
        ING_TRY(hipStreamSynchronize(st));
        std::swap(a.p, rs.p); std::swap(b.p, ri.p); std::swap(c.p, rt.p); rcap = nc;
        return SRN_OK;
    };
    struct Ev { hipEvent_t up0 = nullptr, up1 = nullptr, done = nullptr; };
    std::vector<Ev> evs;
    struct EvGuard { std::vector<Ev>& v; ~EvGuard() { for (Ev& e : v) { (void)hipEventDestroy(e.up0); (void)hipEventDestroy(e.up1); (void)hipEventDestroy(e.done); } } } eguard{evs};
    int last_chunk_of[2] = {-1, -1};   // the chunk whose bytes stage[b] holds (its `done` event frees the buffer)
    unsigned long long* h_nrows = nullptr;
    ING_TRY(hipHostMalloc((void**)&h_nrows, 16, hipHostMallocDefault));
    struct HGuard { unsigned long long* p; ~HGuard() { (void)hipHostFree(p); } } hguard{h_nrows};
    uint64_t rows_known = 0, rows_pending = 0;   // rows known exact at the last synchronisation; bound of the rows enqueued since

    std::vector<char> carry;
    uint64_t file_off = 0;
    bool eof = false, first = true;
    int c = 0;
    while (!eof || !carry.empty()) {
        const int b = c & 1;
        if (last_chunk_of[b] >= 0) ING_TRY(hipEventSynchronize(evs[last_chunk_of[b]].done));
        char* buf = stage[b].c();
        size_t len = carry.size();
        if (len) memcpy(buf, carry.data(), len);
        carry.clear();
        auto tr = std::chrono::steady_clock::now();
        while (!eof && len < cap) {
            const ssize_t got = read(fd, buf + len, cap - len);
            if (got < 0) return fail(SRN_EIO, std::string("read failed: ") + path);
            if (got == 0) eof = true; else len += (size_t)got;
        }
        li.ms_read += ms_since(tr);
        if (len == 0) break;
        size_t use = len;
        if (!eof) {
            const char* nl = (const char*)memrchr(buf, '\n', len);
            if (!nl) {   // a line longer than a chunk: keep its bytes, grow the buffers, read on
                carry.assign(buf, buf + len);
                ING_TRY(hipStreamSynchronize(st));
                cap *= 2; rc = alloc_chunk(cap); if (rc) return rc;
                last_chunk_of[0] = last_chunk_of[1] = -1;
                continue;
            }
            use = (size_t)(nl - buf) + 1;
            carry.assign(buf + use, buf + len);
        }
        // room for this chunk's rows
        const uint64_t bound = use / 6 + 1;
        if (rows_known + rows_pending + bound > rcap) {
            ING_TRY(hipMemcpyAsync(h_nrows, d_nrows, 8, hipMemcpyDeviceToHost, st));
            ING_TRY(hipStreamSynchronize(st));
            rows_known = *h_nrows; rows_pending = 0;
            if (rows_known + bound > rcap) { rc = grow_rows(rows_known + bound); if (rc) return rc; }
        }
        rows_pending += bound;
        Ev ev; ING_TRY(hipEventCreate(&ev.up0)); ING_TRY(hipEventCreate(&ev.up1)); ING_TRY(hipEventCreate(&ev.done));
        evs.push_back(ev);
        ING_TRY(hipEventRecord(ev.up0, st));
        ING_TRY(hipMemcpyAsync(d_text.p, buf, use, hipMemcpyHostToDevice, st));
        ING_TRY(hipEventRecord(ev.up1, st));
        const uint32_t bt = (uint32_t)((use + kByteTile - 1) / kByteTile);
        const uint32_t lt = (uint32_t)((use + 1 + kLineTile - 1) / kLineTile);
        const unsigned char* text = (const unsigned char*)d_text.p;
        hipLaunchKernelGGL(k_nl_count, dim3(bt), dim3(TPB), 0, st, text, (uint64_t)use, d_nlcnt.as<uint32_t>());
        size_t t1 = scan_tb; ING_TRY(scan_excl(d_scan_tmp.p, t1, d_nlcnt.as<uint32_t>(), d_nlbase.as<uint32_t>(), bt + 1, st));
        hipLaunchKernelGGL(k_nl_ends, dim3(bt), dim3(TPB), 0, st, text, (uint64_t)use, d_nlbase.as<uint32_t>(), d_ends.as<uint32_t>());
        ChunkArgs a{text, use, d_ends.as<uint32_t>(), d_nlbase.as<uint32_t>(), bt, (uint32_t)(buf[use - 1] != '\n'), (uint32_t)first, file_off};
        hipLaunchKernelGGL(k_row_count, dim3(lt), dim3(TPB), 0, st, a, d_rcnt.as<uint32_t>());
        t1 = scan_tb; ING_TRY(scan_excl(d_scan_tmp.p, t1, d_rcnt.as<uint32_t>(), d_rbase.as<uint32_t>(), lt + 1, st));
        hipLaunchKernelGGL(k_row_scatter, dim3(lt), dim3(TPB), 0, st, a, d_rbase.as<uint32_t>(), d_nrows, rs.as<uint64_t>(), ri.as<uint64_t>(), rt.as<uint64_t>(),
                           counters.as<unsigned long long>() + 2);
        hipLaunchKernelGGL(k_chunk_done, dim3(1), dim3(1), 0, st, d_nlbase.as<uint32_t>(), bt, a.extra, d_rbase.as<uint32_t>(), lt, d_nrows, counters.as<unsigned long long>() + 1);
        ING_TRY(hipGetLastError());
        ING_TRY(hipEventRecord(ev.done, st));
        last_chunk_of[b] = (int)evs.size() - 1;
        file_off += use; first = false; ++c;
    }
    unsigned long long cnt[3];
    ING_TRY(hipMemcpyAsync(cnt, counters.p, 24, hipMemcpyDeviceToHost, st));
    ING_TRY(hipStreamSynchronize(st));
    for (const Ev& e : evs) {
        float a = 0, p = 0;
        ING_TRY(hipEventElapsedTime(&a, e.up0, e.up1)); ING_TRY(hipEventElapsedTime(&p, e.up1, e.done));
        li.ms_upload += a; li.ms_parse += p;
    }
    uint64_t n = cnt[0];
    li.lines = cnt[1]; li.host_parsed = cnt[2];

    // the host's lines: re-read from the file, parsed by parse_line itself, written back into their slots
    if (li.host_parsed) {
        auto tf = std::chrono::steady_clock::now();
        const uint64_t nf = li.host_parsed;
        DevBuf list, cur, offlen, vals;
        ING_TRY(list.alloc(nf * 4)); ING_TRY(cur.alloc(4)); ING_TRY(offlen.alloc(nf * 16)); ING_TRY(vals.alloc(nf * 24));
        ING_TRY(hipMemsetAsync(cur.p, 0, 4, st));
        hipLaunchKernelGGL(k_fallback_list, grid_for(n), dim3(TPB), 0, st, rt.as<uint64_t>(), n, list.as<uint32_t>(), cur.as<unsigned>());
        hipLaunchKernelGGL(k_fallback_gather, grid_for(nf), dim3(TPB), 0, st, list.as<uint32_t>(), nf, rs.as<uint64_t>(), ri.as<uint64_t>(), offlen.as<uint64_t>());
        std::vector<uint64_t> ol(2 * nf), v(3 * nf);
        ING_TRY(hipMemcpyAsync(ol.data(), offlen.p, nf * 16, hipMemcpyDeviceToHost, st));
        ING_TRY(hipStreamSynchronize(st));
        std::vector<char> line;
        uint64_t dead = 0;
        for (uint64_t q = 0; q < nf; ++q) {
            line.resize(ol[2 * q + 1]);
            if (pread(fd, line.data(), line.size(), (off_t)ol[2 * q]) != (ssize_t)line.size()) return fail(SRN_EIO, std::string("re-read failed: ") + path);
            uint64_t s = 0, i = 0, t = 0;
            if (parse_tsv_line(line.data(), line.data() + line.size(), s, i, t)) { v[3 * q] = s; v[3 * q + 1] = i; v[3 * q + 2] = t; }
            else { v[3 * q] = v[3 * q + 1] = 0; v[3 * q + 2] = kFallback; ++dead; }
        }
        ING_TRY(hipMemcpyAsync(vals.p, v.data(), nf * 24, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_fallback_write, grid_for(nf), dim3(TPB), 0, st, list.as<uint32_t>(), nf, vals.as<uint64_t>(), rs.as<uint64_t>(), ri.as<uint64_t>(), rt.as<uint64_t>());
        if (dead) {   // lines the host rejected leave the row arrays (stable compaction)
            DevBuf flag, pos, a, b2, c2, tmp;
            ING_TRY(flag.alloc((n + 1) * 4)); ING_TRY(pos.alloc((n + 1) * 4)); ING_TRY(a.alloc((n - dead) * 8)); ING_TRY(b2.alloc((n - dead) * 8)); ING_TRY(c2.alloc((n - dead) * 8));
            const size_t tb = scan_bytes<uint32_t>(n + 1); ING_TRY(tmp.alloc(tb));
            hipLaunchKernelGGL(k_live, grid_for(n + 1), dim3(TPB), 0, st, rt.as<uint64_t>(), n, flag.as<uint32_t>());
            size_t t1 = tb; ING_TRY(scan_excl(tmp.p, t1, flag.as<uint32_t>(), pos.as<uint32_t>(), n + 1, st));
            hipLaunchKernelGGL(k_compact3, grid_for(n), dim3(TPB), 0, st, rs.as<uint64_t>(), ri.as<uint64_t>(), rt.as<uint64_t>(), flag.as<uint32_t>(), pos.as<uint32_t>(), n,
                               a.as<uint64_t>(), b2.as<uint64_t>(), c2.as<uint64_t>());
            ING_TRY(hipStreamSynchronize(st));
            std::swap(a.p, rs.p); std::swap(b2.p, ri.p); std::swap(c2.p, rt.p);
            n -= dead;
        }
        ING_TRY(hipGetLastError());
        ING_TRY(hipStreamSynchronize(st));
        li.ms_parse += ms_since(tf);
    }
    li.rows = n; li.skipped = li.lines - n;
    out.n = n;
    return SRN_OK;
}

namespace {
struct OwnStream {   // a stream of the call's own, drained and destroyed when the call leaves
    hipStream_t s = nullptr;
    ~OwnStream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
};

// a missing file is SRN_EIO before the device is touched
int check_readable(const char* path) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(SRN_EIO, std::string("cannot open ") + path);
    close(fd);
    return SRN_OK;
}
}  // namespace

int sessions_from_tsv_gpu(const char* path, int device, Sessions& out, srn_load_info_t* info) {
    if (int rc0 = check_readable(path)) return rc0;
    ING_TRY(hipSetDevice(device));
    OwnStream own;
    ING_TRY(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    TsvRows rows; srn_load_info_t li{};
    int rc = tsv_rows_device(path, device, own.s, rows, li);
    if (rc) return rc;
    if (rows.n >= 0xFFFFFFFFull) return fail(SRN_ERANGE, "the GPU loader groups < 2^32 rows per call; use the host loader");
    rc = group_rows_device(rows.s.as<uint64_t>(), rows.i.as<uint64_t>(), rows.t.as<uint64_t>(), rows.n, own.s, out, &li);
    if (rc) return rc;
    if (info) *info = li;
    return SRN_OK;
}

int events_from_tsv_gpu(const char* path, int device, srn_events** out) {
    if (int rc0 = check_readable(path)) return rc0;
    ING_TRY(hipSetDevice(device));
    OwnStream own;
    ING_TRY(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    TsvRows rows; srn_load_info_t li{};
    int rc = tsv_rows_device(path, device, own.s, rows, li);
    if (rc) return rc;
    ING_TRY(hipStreamSynchronize(own.s));
    srn_events* e = new srn_events();
    e->n = rows.n; e->device = device;
    e->s = (uint64_t*)rows.s.release(); e->i = (uint64_t*)rows.i.release(); e->t = (uint64_t*)rows.t.release();
    *out = e;
    return SRN_OK;
}
void events_free(srn_events* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    for (void* p : {(void*)e->s, (void*)e->i, (void*)e->t}) if (p) (void)hipFree(p);
    delete e;
}

// exact q-quantile of the session lengths, as sessions_length_quantile computes it, by counting instead of sorting
uint64_t sessions_length_quantile_counting(const uint64_t* off, size_t n, double q) {
    if (n == 0) return 0;
    uint64_t maxlen = 0;
    for (size_t i = 0; i < n; ++i) maxlen = std::max(maxlen, off[i + 1] - off[i]);
    std::vector<uint64_t> hist(maxlen + 2, 0);
    for (size_t i = 0; i < n; ++i) ++hist[off[i + 1] - off[i]];
    auto kth = [&](size_t k) {   // k-th smallest length (0-based)
        uint64_t acc = 0;
        for (uint64_t L = 0; L <= maxlen; ++L) { acc += hist[L]; if (acc > k) return L; }
        return maxlen; };
    const double pos = q * (double)(n - 1); const size_t lo = (size_t)std::floor(pos);
    const size_t hi = std::min(n - 1, lo + 1); const double frac = pos - (double)lo;
    const double a = (double)kth(lo), b = (double)kth(hi);
    return (uint64_t)std::llround(a + frac * (b - a));
}

// ... and on offsets that are still on the device
namespace {
constexpr uint32_t kLenBins = 4096;       // lengths 0..4095: 16 KiB of LDS per block
constexpr unsigned kHistBlocks = 256;     // one block per CU: a block adds each bin it touched once, so fewer blocks mean fewer global atomics
// hist[L] = sessions of length L < kLenBins (dropped ones included); over[0] = the sessions longer than that, over[1] = the longest of them.  Counted in LDS first
// (the lengths 1..3 draw most of the adds), then one atomic per touched bin and block
__global__ void k_len_hist(const uint64_t* off, uint64_t n, unsigned long long* hist, unsigned long long* over) {
    __shared__ uint32_t bins[kLenBins];
    __shared__ unsigned long long lds[2][TPB / 64];
    for (uint32_t e = threadIdx.x; e < kLenBins; e += blockDim.x) bins[e] = 0;
    __syncthreads();
    unsigned long long n_over = 0, longest = 0;
    for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s < n; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t len = off[s + 1] - off[s];
        if (len < kLenBins) atomicAdd(&bins[len], 1u);
        else { ++n_over; longest = max(longest, (unsigned long long)len); }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < kLenBins; e += blockDim.x) if (bins[e]) atomicAdd(&hist[e], (unsigned long long)bins[e]);
    for (int o = 32; o > 0; o >>= 1) n_over += __shfl_xor(n_over, o);
    if (lane_id() == 0) lds[0][threadIdx.x / 64] = n_over;
    longest = block_max(longest, lds[1]);   // (synchronises)
    if (threadIdx.x == 0) {
        unsigned long long t = 0; for (int i = 0; i < TPB / 64; ++i) t += lds[0][i];
        if (t) { atomicAdd(&over[0], t); atomicMax(&over[1], longest); }
    }
}
}  // namespace

int device_length_quantile(const uint64_t* d_off, uint64_t n, double q, hipStream_t st, uint64_t* out) {
    *out = 0;
    if (n == 0) return SRN_OK;
    DevBuf d_hist;
    ING_TRY(d_hist.alloc((kLenBins + 2) * 8));
    ING_TRY(hipMemsetAsync(d_hist.p, 0, (kLenBins + 2) * 8, st));
    hipLaunchKernelGGL(k_len_hist, dim3(std::min(grid_for(n).x, kHistBlocks)), dim3(TPB), 0, st, d_off, n, d_hist.as<unsigned long long>(), d_hist.as<unsigned long long>() + kLenBins);
    ING_TRY(hipGetLastError());
    std::vector<unsigned long long> hist(kLenBins + 2);
    ING_TRY(hipMemcpyAsync(hist.data(), d_hist.p, (kLenBins + 2) * 8, hipMemcpyDeviceToHost, st));
    ING_TRY(hipStreamSynchronize(st));
    bool overflow = false;
    auto kth = [&](size_t k) -> uint64_t {   // k-th smallest length (0-based), as in sessions_length_quantile_counting
        uint64_t acc = 0;
        for (uint64_t L = 0; L < kLenBins; ++L) { acc += hist[L]; if (acc > k) return L; }
        overflow = true; return 0; };
    const double pos = q * (double)(n - 1); const size_t lo = (size_t)std::floor(pos);
    const size_t hi = std::min<size_t>(n - 1, lo + 1); const double frac = pos - (double)lo;
    const double a = (double)kth(lo), b = (double)kth(hi);
    if (!overflow) { *out = (uint64_t)std::llround(a + frac * (b - a)); return SRN_OK; }
    // an order statistic lies among the hist[kLenBins] sessions of 4096 items or more (the longest has hist[kLenBins + 1]): their lengths are not binned
    std::vector<uint64_t> off(n + 1);
    ING_TRY(hipMemcpyAsync(off.data(), d_off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    ING_TRY(hipStreamSynchronize(st));
    *out = sessions_length_quantile_counting(off.data(), n, q);
    return SRN_OK;
}

}  // namespace srn
