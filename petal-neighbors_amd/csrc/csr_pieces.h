// How a counted CSR is cut into pieces.  DBSCAN, OPTICS, KDE and mean shift count their radius lists first, read the
// offsets back and then ask for the lists piece by piece, so that the device never holds the whole graph.  Host
// arithmetic only (no HIP): the piece walker (index.hip) cuts with this function, and tests/cpp/csr_pieces.cpp asks it
// "where would these offsets be cut?" on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace pn {

constexpr uint64_t kGraphPiece = (uint64_t)1 << 27;  // list entries per piece where PN_OPT_*_PIECE is 0

// The piece that starts at row a of off [n + 1] (ascending), a < n: rows [a, b), b returned.  A piece is a contiguous
// range of at most `chunk` rows whose lists hold at most E entries together: with lim = min(n, a + chunk), b is the last
// index in (a, lim] with off[b] - off[a] <= E, and at least a + 1 -- a single row longer than E is a piece of its own.
// (off[a] + E does not wrap: offsets count entries in memory, E <= 2^63 - 1.)
inline size_t csr_piece_end(const uint64_t *off, size_t a, size_t n, size_t chunk, uint64_t E) {
    const size_t lim = n - a < chunk ? n : a + chunk;
    const size_t b = (size_t)(std::upper_bound(off + a + 1, off + lim + 1, off[a] + E) - off) - 1;
    return b <= a ? a + 1 : b;
}

}  // namespace pn
