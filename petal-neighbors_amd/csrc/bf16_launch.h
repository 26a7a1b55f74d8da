// What one launch of the bf16 first tier is: its pass, its partition and the main-pass kernel that runs it.  Host
// arithmetic only (no HIP): the plan (index.hip) decides with these functions, the launchers (bf16_filter.hip) obey,
// and tests/cpp/bf16_choice.cpp asks them "what would this call launch?" on the CPU.
#pragma once

#include <cstddef>
#include <cstdint>

namespace pn {

// ScoutOnly: no buffers touched, every run leaves its smallest block minima (kernel MODE 1).  SelfScout: a run scouts
// its own first tiles, then filters (MODE 0).  Seeded: filters against given starting thresholds (MODE 2, k-NN
// buffers) -- the main pass.  Radius: fixed thresholds, 256-slot buffers that overflow instead of compacting (MODE 2, RAD).
enum class Bf16Pass { ScoutOnly, SelfScout, Seeded, Radius };
// Four: bf16_filter_kernel (4 waves, every pass).  Eight: bf16_filter8_kernel, Pair: bf16_filter_kernel_pair (8 waves,
// main pass of an aligned partition only).  Wide: bf16_wide_kernel (128 < D, every pass).  PairTwo: the paired kernel
// with two row tiles per workgroup meeting and six LDS tile buffers (bf16_filter_kernel_meet_pair<KS, CI, 2>).
enum class Bf16Kernel { Four, Eight, Pair, Wide, PairTwo };

constexpr uint32_t kBf16QueryTile = 256;  // queries per query tile (narrow and wide rows)
constexpr uint32_t kBf16RowTile = 64;     // rows per tile, narrow rows
constexpr uint32_t kBf16WideTile = 256;   // rows per tile, wide rows

// workgroups that touch a query tile at most when n_wg equal slices are laid over the (query tile, row tile) list
// (the f32 MFMA tier partitions the same way: mfma_v2_max_segments in mfma_filter_v2.hip returns this)
inline int bf16_touching(size_t q_tiles, int n_wg) { return (int)(((size_t)n_wg + q_tiles - 1) / q_tiles) + 1; }
// segments per query of an UNALIGNED partition (split: row parts per query tile, each with its own segments)
inline int bf16_segments(size_t q_tiles, int n_wg, int split) {
    return split * bf16_touching(q_tiles * (size_t)split, n_wg);
}

struct Bf16Grid {
    uint32_t q_tiles, n_tiles;
    int n_wg, split;
    // a whole number of workgroups per query tile and no row parts: every (segment, query) cell has exactly one writer
    // (no memsets), there are exactly n_wg / q_tiles segments and every workgroup's slice is ONE run of run_tiles tiles
    bool aligned;
    int nseg;            // segments per query (wide rows: a workgroup's two row halves are two segments)
    uint32_t run_tiles;  // narrow rows, aligned: row tiles per run; otherwise 0
};
inline Bf16Grid bf16_grid(size_t n, size_t nq_pad, int n_wg, int split, bool wide = false) {
    Bf16Grid g{};
    const uint32_t rows = wide ? kBf16WideTile : kBf16RowTile;
    g.q_tiles = (uint32_t)(nq_pad / kBf16QueryTile);
    g.n_tiles = (uint32_t)((n + rows - 1) / rows);
    g.n_wg = n_wg;
    g.split = split;
    g.aligned = split == 1 && g.q_tiles > 0 && n_wg >= (int)g.q_tiles && (uint32_t)n_wg % g.q_tiles == 0;
    const int per_query = g.aligned ? n_wg / (int)g.q_tiles : g.q_tiles ? bf16_segments(g.q_tiles, n_wg, split) : 0;
    g.nseg = wide ? 2 * per_query : per_query;
    g.run_tiles = g.aligned && !wide ? g.n_tiles / (uint32_t)per_query : 0u;
    return g;
}

// (450 until the end of round 4; with thresholds from the seed model and 25 row ranges per query tile a 500 k-row shard
// of C2 runs 312-tile runs and the 4-wave kernel is 3.5 % faster there, 156- and 78-tile runs are even / 1 % in favour
// of 8 waves: profiles/r04_waves_ab_model.log)
constexpr uint32_t kBf8MaxRun = 200;  // runs shorter than this many tiles take the 8-wave main-pass kernel
constexpr size_t kBf8MaxImage = (size_t)768 << 20;  // ... on corpora whose tile image is at most this large
#ifndef PN_DIAG_PAIR_MIN_RUN
#define PN_DIAG_PAIR_MIN_RUN 200
#endif
constexpr uint32_t kPairMinRun = PN_DIAG_PAIR_MIN_RUN;  // the paired kernel: runs of at least this many tiles (64-slot buffers, >= 2 query tiles)
// Two tiles per meeting: where the paired kernel is chosen AND the runs are at least this long.
// Measured interleaved with the parent build, one device per session (profiles/r06_pair_meet_ab.log): 625-tile runs
// -- C2 -1.6 % / -2.1 % at 200 steps (sessions 1 / 3), -2.1 % / -2.5 % at 20 steps, c5s -4.1 % -- and the 312-tile runs
// of a 500 k-row shard of C2 -3.7 % / -3.4 % (sessions 2 / 3), every run below every run of the parent.  Only the regime measured: the
// shortest runs measured are those 312 tiles (shorter ones keep one tile per meeting), the largest image is C2's
// (15 625 tiles of 17 408 B = 272 MB; larger ones, up to the paired kernel's 768 MiB, keep one tile per meeting too).
#ifndef PN_DIAG_PAIR2_MIN_RUN
#define PN_DIAG_PAIR2_MIN_RUN 312
#endif
constexpr uint32_t kPairTwoMinRun = PN_DIAG_PAIR2_MIN_RUN;
constexpr size_t kPairTwoMaxImage = (size_t)15625 * 17408;

// The main-pass kernel of a narrow-row launch.  cap: slots per buffer (64 / 128 / 256); refreshers: shared thresholds
// on; image_bytes: the corpus' tile image; wg_slots: the device's workgroup slots of the 4-wave kernel (2 per CU; 0 =
// unknown, and the automatic choice then never takes the paired kernel); forced: PN_OPT_BF16_WAVES -- 0 = the rule
// below, 4 / 8 = that kernel, 16 = the paired kernel, 32 = the paired kernel with two tiles per meeting, each only
// where it applies (elsewhere: the 4-wave kernel).
// The 8-wave kernels serve the main pass of a k-NN call (thresholds given) on an aligned partition only.
// Where a kernel can run at all (the launcher refuses it elsewhere): the 4-wave kernel everywhere on narrow rows; the
// paired kernel where the 8-wave kernel may run, with 64-slot buffers, no refreshers and at least two query tiles.
inline bool bf16_kernel_applies(Bf16Kernel k, const Bf16Grid &g, int cap, Bf16Pass pass, bool refreshers) {
    if (k == Bf16Kernel::Four) return true;
    if (k == Bf16Kernel::Wide || pass != Bf16Pass::Seeded || !g.aligned) return false;
    return k == Bf16Kernel::Eight || (cap == 64 && !refreshers && g.q_tiles >= 2);  // (Pair and PairTwo alike)
}
inline Bf16Kernel bf16_main_kernel(const Bf16Grid &g, int cap, Bf16Pass pass, bool refreshers, size_t image_bytes,
                                   int wg_slots, int forced) {
    if (!bf16_kernel_applies(Bf16Kernel::Eight, g, cap, pass, refreshers)) return Bf16Kernel::Four;
    // The paired kernel: the automatic choice takes it for the long runs (the A/B behind kPairMinRun) --
    // (only grids of the 4-wave kernel that fill every workgroup slot: two of its workgroups then share a CU anyway,
    // which is the regime of the A/B.  A grid below that gives each 4-wave workgroup a CU or a SIMD quarter of its own;
    // pairing would put two waves on every SIMD of half as many CUs: not measured, and by the cycle budget a loss.)
    if (bf16_kernel_applies(Bf16Kernel::Pair, g, cap, pass, refreshers)) {
        const bool fills = wg_slots > 0 && g.n_wg >= wg_slots;
        if (forced == 32) return Bf16Kernel::PairTwo;
        if (forced == 16 || (forced == 0 && fills && g.run_tiles >= kPairMinRun && image_bytes <= kBf8MaxImage))
            return forced == 0 && g.run_tiles >= kPairTwoMinRun && image_bytes <= kPairTwoMaxImage ? Bf16Kernel::PairTwo
                                                                                                   : Bf16Kernel::Pair;
    }
    // Measured on one device (round 4, profiles/r04_waves_ab.log): at C2 (1302-tile runs) the 8-wave kernel is 7-9 %
    // SLOWER than the 4-wave kernel (2.47-2.50 vs 2.28-2.31 ms: twice the LDS fragment traffic, an 8-wave meeting per
    // tile), on a 125 k-row shard of C2 (163-tile runs, where the per-run fixed costs and the buffers' warm-up
    // dominate) 3-5 % faster -- so it serves the short runs (kBf8MaxRun tiles) and the 128-slot buffers.
    // (second box: a 250 k-row shard, 326-tile runs, 2.5 % faster; a 500 k-row shard, 651 tiles, 3 % slower; 128-slot
    // buffers -- k = 100, survivors frequent -- 2 % faster at 1M x 128 and 10 % at 1M x 64 whatever the run length)
    // (end of round 4, profiles/r04_waves_ab_long_runs.log: on corpora whose image is far beyond the 256 MB Infinity
    // Cache the 4-wave kernel wins at every buffer size -- 10M x 128: k = 100 193 vs 205 ms, k = 10 with 128-slot
    // buffers 181 vs 196 ms; 12.5M x 96: 1.89 vs 2.01 s -- while at 1M rows the 8-wave kernel holds its 0-9 %: the
    // automatic choice takes it only where the image is at most kBf8MaxImage bytes)
    const bool want8 = forced == 8 || (forced == 0 && image_bytes <= kBf8MaxImage && (cap >= 128 || g.run_tiles < kBf8MaxRun));
    return want8 ? Bf16Kernel::Eight : Bf16Kernel::Four;
}

}  // namespace pn
