// How the radius lists of W row shards become one list per query.  Every shard (part) answers the same batch with a CSR
// of its own; the host entry points of sharded.hip splice them: radius_splice into the result arrays of
// pn_sharded_query_radius_*, self_splice into the growing lists of pn_sharded_query_radius_self_*.  Host code only (no
// HIP): both splice through csr_splice_query, and tests/cpp/csr_splice.cpp asks it on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>

namespace pn {

// one part's CSR over a batch: the entries of query q are [off[q], off[q + 1]) of rows (global row numbers) and dist
// (nullptr: no distances).  off[0] need not be 0.
template <typename T>
struct CsrPart {
    const uint64_t *off = nullptr;
    const uint64_t *rows = nullptr;
    const T *dist = nullptr;
};

// what W parts hold for queries [0, nq) together: no splice of them keeps more
template <typename T>
inline uint64_t csr_splice_entries(const CsrPart<T> *parts, size_t W, size_t nq) {
    uint64_t total = 0;
    for (size_t r = 0; r < W; ++r) total += parts[r].off[nq] - parts[r].off[0];
    return total;
}

// The entries of query q across the W parts, each kept one handed to sink(part, position in that part's arrays):
//   not sorted: the parts' lists in part order (parts are ascending row ranges and a list ascends, so the rows ascend);
//   sorted:     every part's list is sorted by (distance, global row) and the W lists are merged in that order -- the
//               lists hold no NaN, and -0 compares equal to +0 as in the k-NN order.
// drop (nullable): entries whose row equals *drop are left out (a self-query's own row).  cur: W words of scratch.
template <typename T, typename Sink>
inline void csr_splice_query(const CsrPart<T> *parts, size_t W, size_t q, bool sorted, const uint64_t *drop, uint64_t *cur,
                             Sink &&sink) {
    const bool dropping = drop != nullptr;
    const uint64_t own = dropping ? *drop : 0;  // (copies: what the sink stores cannot change them)
    auto keep = [&](size_t r, uint64_t e) {
        if (!dropping || parts[r].rows[e] != own) sink(r, e);
    };
    if (!sorted) {
        for (size_t r = 0; r < W; ++r) {
            const uint64_t end = parts[r].off[q + 1];
            for (uint64_t e = parts[r].off[q]; e < end; ++e) keep(r, e);
        }
        return;
    }
    for (size_t r = 0; r < W; ++r) cur[r] = parts[r].off[q];
    for (;;) {
        size_t best = W;
        for (size_t r = 0; r < W; ++r) {
            if (cur[r] == parts[r].off[q + 1]) continue;
            if (best == W) {
                best = r;
                continue;
            }
            const T d = parts[r].dist[cur[r]], db = parts[best].dist[cur[best]];
            if (d < db || (d == db && parts[r].rows[cur[r]] < parts[best].rows[cur[best]])) best = r;
        }
        if (best == W) break;
        keep(best, cur[best]++);
    }
}

}  // namespace pn
