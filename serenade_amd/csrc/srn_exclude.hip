// =====================================================================================
// Exclusion lists for the batch predict calls: "do not recommend what the visitor has seen, or what the page already shows".
//
// A row is the first how_many entries of a TOTAL order over the query's candidates (score descending, public id ascending, behind the business rules and without the
// session's most recent item), and scores do not depend on how_many.  With at most E excluded ids, the first how_many + E entries of that order hold the first
// how_many entries that survive the exclusion, in the same relative order.  So the launch sequence runs unchanged at an internal how_many of W = how_many + E into
// WIDE rows (scratch of the call's workspace), and one kernel behind it drops the excluded ids and compacts every row to how_many: the very bytes of "filter all
// candidates, then cut".
//
//   vmis_exclude_kernel   one wave of 64 lanes per query, four queries per workgroup of 256 threads.  The query's list -- its exclusion CSR entry and, with
//                         SRN_FLAG_EXCLUDE_SESSION, the items of its own session -- sits one id per lane in registers, 64 ids per pass (the first pass is kept across
//                         the row's chunks: lists of more than 64 ids re-read the further passes per chunk, from L2).  The row's min(count, W) entries are walked in
//                         chunks of 64, one coalesced 512-byte read per array; an entry is compared against every list id (a broadcast of lane j's two dwords);
//                         the keep mask's ballot ranks the kept entries (mbcnt), which are written -- id and score -- at written + rank while that is below how_many.
//                         counts[q] = min(kept, how_many); a wide count of 0xFFFFFFFF is passed on; a list longer than max_excl gives 0xFFFFFFFF.
//                         No LDS, no scratch memory: 0 bytes of either in the resource-usage remarks.
// =====================================================================================
#include <hip/hip_runtime.h>

#include "srn_runtime.h"

namespace srn {

namespace {
__device__ __forceinline__ uint64_t lane_bcast64(uint64_t v, uint32_t j) {   // lane j's value to every lane; j is wave-uniform
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)j), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)j);
    return ((uint64_t)hi << 32) | lo;
}
}  // namespace

__global__ __launch_bounds__(256) void vmis_exclude_kernel(uint32_t nq, const uint64_t* __restrict__ w_ids, const double* __restrict__ w_scores, const uint32_t* __restrict__ w_counts, uint32_t W,
                                                           const uint64_t* __restrict__ x_flat, const uint32_t* __restrict__ x_off, uint32_t max_excl,
                                                           const uint64_t* __restrict__ items_flat, const uint32_t* __restrict__ q_off,
                                                           uint64_t* __restrict__ out_ids, double* __restrict__ out_scores, uint32_t* __restrict__ out_counts, uint32_t how_many) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);   // (wave-uniform)
    if (q >= nq) return;
    const uint32_t c = w_counts[q];
    uint32_t xb = 0u, xn = 0u, sb = 0u, sn = 0u;
    if (x_flat) { xb = x_off[q]; xn = x_off[q + 1] - xb; }
    if (items_flat) { sb = q_off[q]; sn = q_off[q + 1] - sb; }
    if (c == 0xFFFFFFFFu || xn > max_excl) {   // not served (empty / over-long session, table limits) | a list beyond the call's capacity: the wide row may be too short for it
        if (lane == 0u) out_counts[q] = 0xFFFFFFFFu;
        return;
    }
    const uint32_t T = xn + sn, n = min(c, W);
    // list entry t: the exclusion list first, the session's items behind it
    auto list_id = [&](uint32_t t) -> uint64_t { return t < xn ? x_flat[(size_t)xb + t] : items_flat[(size_t)sb + (t - xn)]; };
    const uint32_t n0 = min(T, 64u);
    const uint64_t l0 = lane < n0 ? list_id(lane) : 0ull;
    const uint64_t* __restrict__ ri = w_ids + (size_t)q * W; const double* __restrict__ rs = w_scores + (size_t)q * W;
    uint64_t* __restrict__ oi = out_ids + (size_t)q * how_many; double* __restrict__ os = out_scores + (size_t)q * how_many;
    uint32_t written = 0u;
    for (uint32_t cb = 0u; cb < n && written < how_many; cb += 64u) {
        const uint32_t e = cb + lane;
        bool keep = e < n;
        const uint64_t id = keep ? ri[e] : 0ull;
        const double sc = keep ? rs[e] : 0.0;
        for (uint32_t j = 0u; j < n0; ++j) keep = keep && id != lane_bcast64(l0, j);
        for (uint32_t tb = 64u; tb < T; tb += 64u) {   // lists of more than 64 ids: the further passes
            const uint32_t nt = min(T - tb, 64u);
            const uint64_t lt = lane < nt ? list_id(tb + lane) : 0ull;
            for (uint32_t j = 0u; j < nt; ++j) keep = keep && id != lane_bcast64(lt, j);
        }
        const unsigned long long mask = __ballot(keep);
        const uint32_t pos = written + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (keep && pos < how_many) { oi[pos] = id; os[pos] = sc; }
        written += (uint32_t)__popcll(mask);
    }
    if (lane == 0u) out_counts[q] = min(written, how_many);
}

hipError_t launch_exclude(hipStream_t st, uint32_t nq, const uint64_t* w_ids, const double* w_scores, const uint32_t* w_counts, uint32_t W, const uint64_t* x_flat, const uint32_t* x_off,
                          uint32_t max_excl, const uint64_t* items_flat, const uint32_t* q_off, uint64_t* out_ids, double* out_scores, uint32_t* out_counts, uint32_t how_many) {
    hipLaunchKernelGGL(vmis_exclude_kernel, dim3((nq + 3u) / 4u), dim3(256), 0, st, nq, w_ids, w_scores, w_counts, W, x_flat, x_off, max_excl, items_flat, q_off, out_ids, out_scores, out_counts, how_many);
    return hipGetLastError();
}

int device_exclude_filter(DeviceState* d, uint32_t nq, const uint64_t* w_ids, const double* w_scores, const uint32_t* w_counts, uint32_t wide, const uint64_t* x_flat, const uint32_t* x_off,
                          uint32_t max_excl, const uint64_t* items_flat, const uint32_t* q_off, uint64_t* out_ids, double* out_scores, uint32_t* out_counts, uint32_t how_many, void* stream) {
    HIP_TRY(hipSetDevice(d->device));
    if (nq == 0) return SRN_OK;
    HIP_TRY(launch_exclude((hipStream_t)stream, nq, w_ids, w_scores, w_counts, wide, x_flat, x_off, max_excl, items_flat, q_off, out_ids, out_scores, out_counts, how_many));
    return SRN_OK;
}

// The wide rows of a call in the workspace's scratch: ids [nq][W] | scores [nq][W] | counts [nq], 16 * nq * W + 4 * nq bytes (2^20 queries at how_many 21 and 16
// excluded ids: 620 MB).  Grow-only like every buffer of the workspace: equal-shaped calls allocate nothing, and the reuse is ordered by the stream the workspace is bound to.
int exclude_wide_room(Workspace* w, uint32_t nq, uint32_t W, uint64_t** ids, double** scores, uint32_t** counts) {
    const size_t rows = ((size_t)nq * W * 8 + 255) / 256 * 256;
    const int rc = ensure(&w->wide, &w->wide_bytes, 2 * rows + (size_t)nq * 4); if (rc) return rc;
    *ids = (uint64_t*)w->wide; *scores = (double*)(w->wide + rows); *counts = (uint32_t*)(w->wide + 2 * rows);
    return SRN_OK;
}

// srn_predict_batch_excl (host pointers): the call's own workspace serves it.  The launch sequence's staged output rows ARE the wide rows; this buffer takes the rest --
// the lists (x.x_flat / x.x_off: host pointers on entry, their device copies on return) and the caller-sized rows the filter writes (x.out_*), cleared: the tail of a
// row reads as 0, as for srn_predict_batch.  Everything on `st`.
int exclude_host_room(Workspace* w, hipStream_t st, uint32_t nq, ExclSpec& x) {
    const uint64_t* h_xflat = x.x_flat; const uint32_t* h_xoff = x.x_off;
    const size_t nx = h_xoff ? h_xoff[nq] : 0, n_out = (size_t)nq * x.how_many;
    Bump b;
    const auto r_x = b.take<const uint64_t>(nx * 8); const auto r_xoff = b.take<const uint32_t>(h_xoff ? ((size_t)nq + 1) * 4 : 0);
    const auto r_ids = b.take<uint64_t>(n_out * 8); const auto r_sc = b.take<double>(n_out * 8); const auto r_cnt = b.take<uint32_t>((size_t)nq * 4);
    { const int rc = ensure(&w->wide, &w->wide_bytes, b.bytes); if (rc) return rc; }
    char* s = w->wide;
    x.x_flat = h_xoff ? r_x.at(s) : nullptr; x.x_off = h_xoff ? r_xoff.at(s) : nullptr;
    x.out_ids = r_ids.at(s); x.out_scores = r_sc.at(s); x.out_counts = r_cnt.at(s);
    HIP_TRY(hipMemsetAsync(x.out_ids, 0, n_out * 8, st));
    HIP_TRY(hipMemsetAsync(x.out_scores, 0, n_out * 8, st));
    if (h_xoff) {
        if (nx) HIP_TRY(hipMemcpyAsync((void*)x.x_flat, h_xflat, nx * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync((void*)x.x_off, h_xoff, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice, st));
    }
    return SRN_OK;
}
int exclude_fetch_host(hipStream_t st, uint32_t nq, const ExclSpec& x, uint64_t* h_ids, double* h_scores, uint32_t* h_counts) {
    const size_t n_out = (size_t)nq * x.how_many;
    HIP_TRY(hipMemcpyAsync(h_ids, x.out_ids, n_out * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_scores, x.out_scores, n_out * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_counts, x.out_counts, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SRN_OK;
}

}  // namespace srn
