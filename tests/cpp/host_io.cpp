// Where would these slots lie?  Reads one case per line from stdin --
//   k elem_bytes[0] count[0] .. elem_bytes[k - 1] count[k - 1]
// -- declares the k slots in order and prints "off[0] .. off[k - 1] total" on one line, or "error" where the layout
// reports one (a product or a sum beyond size_t, more slots than kIoSlots).  The layout lives in a heap allocation of
// exactly its size, so a write past its slot arrays is the sanitizer's.
// Host code only: csrc/host_io.h is all it includes (tests/test_host_io.py compiles and runs it).
#include <cstdio>
#include <memory>

#include "../../petal-neighbors_amd/csrc/host_io.h"

int main() {
    unsigned long long k;
    int lines = 0;
    while (std::scanf("%llu", &k) == 1) {
        auto lay = std::make_unique<pn::IoLayout>();
        bool bad = false;
        for (unsigned long long i = 0; i < k; ++i) {
            unsigned long long elem, count;
            if (std::scanf("%llu %llu", &elem, &count) != 2) return 2;
            const size_t slot = lay->add((size_t)elem, (size_t)count);
            if (slot == pn::kIoSlots) bad = true;
            else if (bad || slot != (size_t)i) return 3;  // (an error is for good; slots are numbered in order)
        }
        if (bad != !lay->ok) return 4;
        if (bad) {
            std::printf("error\n");
        } else {
            if (lay->slots != (size_t)k) return 5;
            for (size_t i = 0; i < lay->slots; ++i) std::printf("%zu ", lay->off[i]);
            std::printf("%zu\n", lay->total);
        }
        ++lines;
    }
    return lines > 0 ? 0 : 1;
}
