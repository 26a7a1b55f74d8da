// What do these parts splice to?  Reads one case per line from stdin --
//   bits W nq sorted wd q0 m drop g0   then for each of the W parts:   off[0] .. off[nq]  L  row[0 .. L)  dist[0 .. L)
// -- bits 32 or 64 (float / double), distances as hexadecimal bit patterns and only when wd = 1, L the length of the
// part's arrays (off[nq]: entries in front of off[0] are never read).  Queries q0 .. q0 + m of the batch are spliced as
// sharded.hip does it: csr_splice_query per query, with drop = 1 the entries equal to the query's own row g0 + t left out
// (the self form), written one after the other.  Prints "offsets | rows | distance bits" on one line.
// Every input array is a heap allocation of exactly its length and the output arrays hold exactly csr_splice_entries
// words, so a read or write past either end is the sanitizer's.
// Host code only: csrc/csr_splice.h is all it includes (tests/test_csr_splice.py compiles and runs it).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../petal-neighbors_amd/csrc/csr_splice.h"

template <typename T, typename Bits>
static int run(size_t W, size_t nq, bool sorted, bool wd, size_t q0, size_t m, bool drop, uint64_t g0) {
    std::vector<std::unique_ptr<uint64_t[]>> off(W), rows(W);
    std::vector<std::unique_ptr<T[]>> dist(W);
    std::vector<pn::CsrPart<T>> parts(W), from_q0(W);
    for (size_t r = 0; r < W; ++r) {
        off[r].reset(new uint64_t[nq + 1]);
        for (size_t i = 0; i <= nq; ++i)
            if (std::scanf("%" SCNu64, &off[r][i]) != 1) return 2;
        unsigned long long L;
        if (std::scanf("%llu", &L) != 1 || L != off[r][nq]) return 2;
        rows[r].reset(new uint64_t[L]);
        for (size_t i = 0; i < L; ++i)
            if (std::scanf("%" SCNu64, &rows[r][i]) != 1) return 2;
        if (wd) {
            dist[r].reset(new T[L]);
            for (size_t i = 0; i < L; ++i) {
                uint64_t b;
                if (std::scanf("%" SCNx64, &b) != 1) return 2;
                const Bits bits = (Bits)b;
                std::memcpy(&dist[r][i], &bits, sizeof(T));
            }
        }
        parts[r] = {off[r].get(), rows[r].get(), dist[r].get()};
        from_q0[r] = {off[r].get() + q0, rows[r].get(), dist[r].get()};
    }
    const uint64_t room = pn::csr_splice_entries(from_q0.data(), W, m);
    std::unique_ptr<uint64_t[]> out_rows(new uint64_t[room]), out_off(new uint64_t[m + 1]), cur(new uint64_t[W]);
    std::unique_ptr<T[]> out_dist(new T[wd ? room : 0]);
    uint64_t w = 0;
    for (size_t t = 0; t < m; ++t) {
        const uint64_t own = g0 + t;
        out_off[t] = w;
        pn::csr_splice_query(parts.data(), W, q0 + t, sorted, drop ? &own : nullptr, cur.get(), [&](size_t r, uint64_t e) {
            out_rows[w] = parts[r].rows[e];
            if (wd) out_dist[w] = parts[r].dist[e];
            ++w;
        });
    }
    out_off[m] = w;
    for (size_t t = 0; t <= m; ++t) std::printf("%s%" PRIu64, t ? " " : "", out_off[t]);
    std::printf(" |");
    for (uint64_t i = 0; i < w; ++i) std::printf(" %" PRIu64, out_rows[i]);
    std::printf(" |");
    for (uint64_t i = 0; wd && i < w; ++i) {
        Bits bits;
        std::memcpy(&bits, &out_dist[i], sizeof(T));
        std::printf(" %" PRIx64, (uint64_t)bits);
    }
    std::printf("\n");
    return 0;
}

int main() {
    unsigned long long bits, W, nq, sorted, wd, q0, m, drop, g0;
    int lines = 0;
    while (std::scanf("%llu %llu %llu %llu %llu %llu %llu %llu %llu", &bits, &W, &nq, &sorted, &wd, &q0, &m, &drop, &g0) == 9) {
        if ((bits != 32 && bits != 64) || W == 0 || q0 + m > nq || (sorted && !wd)) return 3;
        const int rc = bits == 32 ? run<float, uint32_t>(W, nq, sorted, wd, q0, m, drop, g0)
                                  : run<double, uint64_t>(W, nq, sorted, wd, q0, m, drop, g0);
        if (rc) return rc;
        ++lines;
    }
    return lines > 0 ? 0 : 1;
}
