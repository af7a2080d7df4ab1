// Today's per-request path as a library call, for tools/recommend_bench.py's baseline (3): `threads` host threads call srn_recommend -- host session store,
// dynamic batcher -- on the requests i with i % threads == t, in order.  Built by the tool with g++ against libserenade_hip.so.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <thread>
#include <vector>

#include "../include/serenade_hip.h"

extern "C" int srn_host_recommend_path(srn_batcher_t* b, srn_session_store_t* store, const char* ids_flat, const uint64_t* off, const uint64_t* items,
                                       const uint8_t* consent, size_t n, size_t max_items, uint64_t now, size_t how_many, unsigned threads, double* out_secs,
                                       uint64_t* out_checksum) {
    std::atomic<int> err{0};
    std::atomic<uint64_t> sum{0};
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (unsigned t = 0; t < threads; ++t)
        th.emplace_back([&, t] {
            std::vector<uint64_t> ids(how_many); size_t got = 0; uint64_t s = 0;
            for (size_t i = t; i < n && !err.load(std::memory_order_relaxed); i += threads) {
                const int rc = srn_recommend(b, store, ids_flat + off[i], (size_t)(off[i + 1] - off[i]), items[i], consent ? consent[i] : 1, max_items, now,
                                             ids.data(), nullptr, &got);
                if (rc) { err = rc; break; }
                s += got ? ids[0] : 0;
            }
            sum += s;
        });
    for (auto& x : th) x.join();
    *out_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (out_checksum) *out_checksum = sum;
    return err;
}
