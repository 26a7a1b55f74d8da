// Where would these offsets be cut?  Reads one case per line from stdin --
//   chunk E n off[0] .. off[n]
// -- and prints the pieces csr_piece_end walks through, "a:b" each, on one line.  The offsets live in a heap array of
// exactly n + 1 words, so a read past either end is the sanitizer's.
// Host code only: csrc/csr_pieces.h is all it includes (tests/test_csr_pieces.py compiles and runs it).
#include <cstdio>
#include <vector>

#include "../../petal-neighbors_amd/csrc/csr_pieces.h"

int main() {
    unsigned long long chunk, E, n;
    int lines = 0;
    while (std::scanf("%llu %llu %llu", &chunk, &E, &n) == 3) {
        std::vector<uint64_t> off((size_t)n + 1);
        for (auto &o : off) {
            unsigned long long v;
            if (std::scanf("%llu", &v) != 1) return 2;
            o = v;
        }
        for (size_t a = 0; a < (size_t)n;) {
            const size_t b = pn::csr_piece_end(off.data(), a, (size_t)n, (size_t)chunk, (uint64_t)E);
            if (b <= a || b > (size_t)n) return 3;  // (no progress, or past the end: the walk would not end / would overrun)
            std::printf("%s%zu:%zu", a ? " " : "", a, b);
            a = b;
        }
        std::printf("\n");
        ++lines;
    }
    return lines > 0 ? 0 : 1;
}
