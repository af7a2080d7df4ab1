// The evaluator's path (serenade_amd/csrc/host/evaluator.cpp) as a library call, for tools/eval_bench.py's baseline (c): prefixes expanded on
// the host, one srn_predict_batch from pageable memory, ids copied back, metrics on one host core with a hash set per query (the same
// Reporter formulas).  Built by the tool with g++ against libserenade_hip.so.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../include/serenade_hip.h"

extern "C" int srn_host_eval_path(const srn_index_t* idx, const uint64_t* items, const uint64_t* sess_off, size_t n_sessions,
                                  const uint64_t* train_items, size_t n_train, size_t k, size_t m, size_t how_many, size_t window, size_t length,
                                  unsigned flags, double* out_ms3, double* out_mrr) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    std::vector<uint64_t> flat; std::vector<uint32_t> qoff{0}; std::vector<std::pair<size_t, size_t>> truth;   // (session, state)
    for (size_t s = 0; s < n_sessions; ++s) {
        const uint64_t* ev = items + sess_off[s]; const size_t len = sess_off[s + 1] - sess_off[s];
        for (size_t state = 1; state < len; ++state) {
            const size_t start = state > window ? state - window : 0;
            flat.insert(flat.end(), ev + start, ev + state); qoff.push_back((uint32_t)flat.size()); truth.push_back({s, state});
        }
    }
    const size_t nq = truth.size();
    std::vector<uint64_t> ids(nq * how_many); std::vector<double> scores(nq * how_many); std::vector<uint32_t> counts(nq);
    const auto t1 = clk::now();
    int rc = srn_predict_batch(idx, flat.data(), qoff.data(), nq, k, m, how_many, flags, ids.data(), scores.data(), counts.data());
    if (rc) return rc;
    const auto t2 = clk::now();
    std::unordered_map<uint64_t, uint64_t> freq; uint64_t max_freq = 0;
    for (size_t i = 0; i < n_train; ++i) max_freq = std::max(max_freq, ++freq[train_items[i]]);
    double mrr = 0, ndcg = 0, hit = 0, pop = 0, prec = 0, rec = 0;
    std::unordered_set<uint64_t> covered;
    for (size_t q = 0; q < nq; ++q) {
        const uint64_t* ev = items + sess_off[truth[q].first];
        const size_t state = truth[q].second, len = sess_off[truth[q].first + 1] - sess_off[truth[q].first];
        std::vector<uint64_t> next(ev + state, ev + len), top(ids.begin() + q * how_many, ids.begin() + q * how_many + std::min<size_t>(counts[q], length));
        auto pos = std::find(top.begin(), top.end(), next[0]);
        if (pos != top.end()) { mrr += 1.0 / (double)(pos - top.begin() + 1); hit += 1.0; }
        std::unordered_set<uint64_t> next_set(next.begin(), next.end()), top_set(top.begin(), top.end());
        double num = 0, den = 0;
        for (size_t i = 0; i < top.size(); ++i) if (next_set.count(top[i])) num += i == 0 ? 1.0 : 1.0 / std::log2((double)i + 1.0);
        for (size_t i = 0; i < std::min(next.size(), length); ++i) den += i == 0 ? 1.0 : 1.0 / std::log2((double)i + 1.0);
        ndcg += num / den;
        size_t inter = 0; for (uint64_t x : top_set) inter += next_set.count(x);
        prec += (double)inter / (double)length; rec += (double)inter / (double)next.size();
        if (!top_set.empty()) { double s = 0; for (uint64_t x : top_set) { auto f = freq.find(x); if (f != freq.end()) s += (double)f->second / (double)max_freq; }
                                pop += s / (double)top_set.size(); }
        for (uint64_t x : top) covered.insert(x);
    }
    const auto t3 = clk::now();
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    out_ms3[0] = ms(t0, t1); out_ms3[1] = ms(t1, t2); out_ms3[2] = ms(t2, t3);
    *out_mrr = nq ? mrr / (double)nq : 0.0;
    (void)ndcg; (void)hit; (void)pop; (void)prec; (void)rec;
    return 0;
}
