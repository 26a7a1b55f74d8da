// What would a first-tier launch be?  Reads one case per line from stdin --
//   n nq_pad n_wg split cap pass refreshers image_bytes wg_slots forced_waves wide
// (pass: 0 ScoutOnly, 1 SelfScout, 2 Seeded, 3 Radius; wide: 1 = the partition of wide rows, which have one kernel:
// "-" is printed for it) -- and prints bf16_grid's and bf16_main_kernel's answer:
//   kernel q_tiles n_tiles n_wg split aligned nseg run_tiles
// Host code only: csrc/bf16_launch.h is all it includes (tests/test_bf16_choice.py compiles and runs it).
#include <cstdio>

#include "../../petal-neighbors_amd/csrc/bf16_launch.h"

int main() {
    static const char *const kernels[] = {"Four", "Eight", "Pair", "Wide"};
    unsigned long long n, nq_pad, image_bytes;
    int n_wg, split, cap, pass, refreshers, wg_slots, forced, wide, lines = 0;
    while (std::scanf("%llu %llu %d %d %d %d %d %llu %d %d %d", &n, &nq_pad, &n_wg, &split, &cap, &pass, &refreshers,
                      &image_bytes, &wg_slots, &forced, &wide) == 11) {
        if (pass < 0 || pass > 3) return 2;
        const pn::Bf16Grid g = pn::bf16_grid((size_t)n, (size_t)nq_pad, n_wg, split, wide != 0);
        const pn::Bf16Kernel k = pn::bf16_main_kernel(g, cap, static_cast<pn::Bf16Pass>(pass), refreshers != 0,
                                                      (size_t)image_bytes, wg_slots, forced);
        std::printf("%s %u %u %d %d %d %d %u\n", wide ? "-" : kernels[static_cast<int>(k)], g.q_tiles, g.n_tiles, g.n_wg, g.split,
                    (int)g.aligned, g.nseg, g.run_tiles);
        ++lines;
    }
    return lines > 0 ? 0 : 1;
}
