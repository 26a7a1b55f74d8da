// Which paired kernel would a first-tier launch take?  Reads one case per line from stdin --
//   n nq_pad n_wg split cap pass refreshers image_bytes wg_slots forced_waves
// (pass: 0 ScoutOnly, 1 SelfScout, 2 Seeded, 3 Radius) -- and prints bf16_main_kernel's answer, whether that kernel
// applies by bf16_kernel_applies, and the run length:
//   kernel applies run_tiles
// Host code only: csrc/bf16_launch.h is all it includes (tests/test_bf16_choice_meet.py compiles and runs it).
#include <cstdio>

#include "../../petal-neighbors_amd/csrc/bf16_launch.h"

static const char *name(pn::Bf16Kernel k) {
    switch (k) {
        case pn::Bf16Kernel::Four: return "Four";
        case pn::Bf16Kernel::Eight: return "Eight";
        case pn::Bf16Kernel::Pair: return "Pair";
        case pn::Bf16Kernel::Wide: return "Wide";
        case pn::Bf16Kernel::PairTwo: return "PairTwo";
    }
    return "?";
}

int main() {
    static_assert(static_cast<int>(pn::Bf16Kernel::Four) == 0 && static_cast<int>(pn::Bf16Kernel::Eight) == 1 &&
                      static_cast<int>(pn::Bf16Kernel::Pair) == 2 && static_cast<int>(pn::Bf16Kernel::Wide) == 3,
                  "the kernels that were there keep their values");
    unsigned long long n, nq_pad, image_bytes;
    int n_wg, split, cap, pass, refreshers, wg_slots, forced, lines = 0;
    while (std::scanf("%llu %llu %d %d %d %d %d %llu %d %d", &n, &nq_pad, &n_wg, &split, &cap, &pass, &refreshers, &image_bytes,
                      &wg_slots, &forced) == 10) {
        if (pass < 0 || pass > 3) return 2;
        const pn::Bf16Grid g = pn::bf16_grid((size_t)n, (size_t)nq_pad, n_wg, split);
        const pn::Bf16Pass p = static_cast<pn::Bf16Pass>(pass);
        const pn::Bf16Kernel k = pn::bf16_main_kernel(g, cap, p, refreshers != 0, (size_t)image_bytes, wg_slots, forced);
        std::printf("%s %d %u\n", name(k), (int)pn::bf16_kernel_applies(k, g, cap, p, refreshers != 0), g.run_tiles);
        ++lines;
    }
    return lines > 0 ? 0 : 1;
}
