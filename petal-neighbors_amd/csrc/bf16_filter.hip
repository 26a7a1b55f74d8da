// bf16_filter.hip -- first-tier filter of the k-NN path: a PROVEN lower bound of |q-p|^2 - |q|^2
// from one bf16 MFMA contraction (v_mfma_f32_32x32x16_bf16, 16x the f32 MFMA rate), with the same
// running top-k' candidate buffers, exact re-rank and per-query proof as mfma_filter_v2.hip.  The
// results of the k-NN call do not depend on this filter's arithmetic: candidates are re-ranked with the
// reference's exact fold (select.hip) and a query whose exclusions cannot be proven falls back to the
// f32 engines.  Only the filter's COST depends on how tight the bound is.
//
// ---- the bound ------------------------------------------------------------------------------------
// Everything below is written for TRANSLATED vectors q := q - mu, p := p - mu (mu = per-dimension mean of the
// corpus, f32, kept with the index -- or zero when translating would shrink the squared norms by less than 16x):
// distances do not change, the norms that the bound's slack is proportional to shrink, and data with a large
// common offset becomes servable at all.  (Mild cases are left alone on purpose: on uniform [0,1) data the
// translation tightens the bound 4x but the signed operands cost the matrix pipe 4 % of its clock.)  The subtraction is
// done in f64; its rounding (2^-53 relative per coordinate) disappears in the 2^-40 the norm sums are widened by.
// q^ = bf16(q), p^ = bf16(p) (round to nearest; |x| < 2^-60 -> 0 so no product is subnormal),
// eq = q - q^, ep = p - p^.  Then q.p = q^.p^ + q^.ep + eq.p  <=  q^.p^ + |q^||ep| + |eq||p|, so
//     |q-p|^2 - |q|^2  =  |p|^2 - 2 q.p  >=  |p|^2 - 2 q^.p^ - 2|q^||ep| - 2|eq||p|.
// The right-hand side is ONE dot product of K = 16*KS bf16 columns (KS-1 data steps + one extra step):
//     query row  [ -2 q^_k ...          | 1     1     1     -Aq  -Cq  0 ... ]
//     corpus row [    p^_k ...          | n_hi  n_mi  n_lo   Bp   Dp  0 ... ]
//   n_hi + n_mi + n_lo <= |p|^2 (1 - g)          (three bf16 pieces, each truncated toward zero)
//   Aq >= |q^|,  Bp >= (2|ep| + 2 g |p^|)(1 + 2g),  Cq >= |eq|,  Dp >= 2|p|(1 + 2g)   (rounded UP to bf16)
// bf16 x bf16 products are exact in f32; the matrix core's f32 accumulation of the K + 1 terms is assumed
// to err by at most g * (sum of the terms' magnitudes) with g = 2^-13 -- 7x the (K+1) * 2^-23 of a
// truncating adder tree over 145 terms; tests/test_gpu_bf16.py measures the actual error against the terms rebuilt
// on the host: at most 0.16 % of this allowance.
// The magnitudes are bounded by |p|^2 + 2|q^||p^| + Aq Bp + Cq Dp, each of which is paid for above
// (the (1-g), the 2g|p^| inside Bp, and the (1+2g) factors), so the computed value L' satisfies
//     L'(q,p)  <=  |q-p|^2 - |q-mu|^2     for every finite q, p with |q-mu|^2, |p-mu|^2 < 2^100.
// Rows / queries outside that range raise a flag (index not eligible / query re-run exactly).
// Padding rows carry n_hi = 1.7e38: they can enter a buffer only while its threshold is still +inf, are the
// first to be compacted away, and select.hip ignores row numbers >= n.
//
// ---- the kernel -----------------------------------------------------------------------------------
// Same persistent balanced partition and candidate-buffer protocol as mfma_filter_v2.hip; what differs
// is sized for a matrix pipe that is 16x faster:
//  * a workgroup is 4 waves x 64 queries (two 32-query MFMA column blocks per wave): every A fragment
//    read from LDS feeds two MFMAs, the 2 x KS B fragments of the wave's 64 queries stay in registers;
//  * the corpus is stored as ready-made LDS tile images (64 rows x (2 KS + 1) 16-byte chunks: the odd
//    row pitch makes the ds_read_b128 fragment reads conflict-free), so staging is a linear LDS-DMA copy;
//  * all per-query bookkeeping (threshold, fill count) lives in registers, appends are plain global
//    stores into the (segment, query) buffers the select kernel reads -- no LDS atomics, no fences on
//    the fast path, no flush copy; the tile barrier waits for the LDS-DMA but not for those stores
//    (bf_wait_dma);
//  * the main loop is software-pipelined over three tile buffers: every chain of 2 KS MFMAs starts from fragments
//    and row norms requested during the previous chain, the workgroup's one barrier per tile sits between the tile's
//    two chains (bf_chain_p and the loop in the kernel say why);
//  * the fast path per 16 bounds is a v_min3 tree and one compare in the chain's shadow; the row a surviving minimum
//    belongs to is found in the rare path (bf_slow: tags + a second-smallest network, one append for all lanes);
//  * thresholds do not start at +inf: a scout pass over the run's first tiles seeds them -- within the
//    launch from the run's own rows, or, with several segments per query, in a scout-only launch whose
//    lists bf16_seed_kernel merges per query over all segments (host: bf16_plan in index.hip).
// Measurements behind each of these, and what was tried and dropped: DESIGN.md section 4.0.
#include "pn_internal.h"
#include "topk_buffer.h"

#include <cstdio>
#include <cstdlib>

namespace pn {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_b;
typedef const __attribute__((address_space(1))) void glb_void_b;

#ifdef PN_DIAG_BF_COUNT  // diagnostic build only: event counters
__device__ unsigned long long g_bfdbg[16];  // 12.. refreshers: query visits, updates, passes, rejected reads
__device__ unsigned long long g_bfdbg_lag[16];  // the paired kernels' lagging half (waves 4-7), same slots
// per-wave accumulators in registers (dbg_), flushed by one atomic per counter at the end of a run: an atomic per
// event would itself be what the barrier waits for
#define BF_COUNT(i, v) (dbg_[i] += (unsigned long long)(v))
#define BF_DBG_DECL unsigned long long dbg_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define BF_DBG_ARG , unsigned long long (&dbg_)[12]
#define BF_DBG_PASS , dbg_
#define BF_DBG_FLUSH(lane)                                                        \
    do {                                                                          \
        if ((lane) == 0)                                                          \
            for (int i_ = 0; i_ < 12; ++i_) {                                     \
                atomicAdd(&g_bfdbg[i_], dbg_[i_]);                                \
                dbg_[i_] = 0;                                                     \
            }                                                                     \
    } while (0)
__device__ __forceinline__ unsigned long long bf_stamp() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
// a stamp that does not wait for itself (the wait would also wait for the fragment reads in flight): settle it before use
__device__ __forceinline__ unsigned long long bf_stamp_nw() {
    unsigned long long t;
    asm volatile("s_memtime %0" : "=s"(t));
    return t;
}
__device__ __forceinline__ void bf_settle(unsigned long long &t) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(t)::"memory"); }
#else
#define BF_COUNT(i, v) ((void)0)
#define BF_DBG_DECL ((void)0)
#define BF_DBG_ARG
#define BF_DBG_PASS
#define BF_DBG_FLUSH(lane) ((void)0)
#endif

constexpr int kBQ = 256;  // queries per workgroup (4 waves x 64)
constexpr int kBP = 64;   // rows per tile
constexpr double kG = 1.0 / 8192.0;          // g = 2^-13 (accumulation-error allowance, see header)
constexpr double kUp = 1.0 + 1.0 / 1099511627776.0;  // 1 + 2^-40: covers the f64 rounding of the norm sums
// Column of the first of the five extra values, and the number of 16-column MFMA steps: the extras use the free
// columns of the last data step when it has five (D mod 16 in 1..11), else a step of their own; at least two steps.
__host__ __device__ inline int bf16_extra_col(int dim) {
    const int room = (dim + 15) / 16 * 16 - dim;
    return room >= 5 && dim > 16 ? dim : (dim + 15) / 16 * 16;
}
__host__ __device__ inline int bf16_steps(int dim) { return (bf16_extra_col(dim) + 5 + 15) / 16; }
// "Norm in the accumulator" layout (CI), for row lengths whose five extra columns would cost an MFMA step of their own
// (D mod 16 in {0, 12..15}; D = 128: 8 steps instead of 9, D = 96: 6 instead of 7).  The extra columns disappear:
//   * |p|^2 (1 - g), rounded down to f32, enters the chain as the accumulator's INITIAL value (the C operand of the
//     first MFMA step) instead of as three bf16 pieces -- the row norms travel in the tile image's padding chunks;
//   * the two error products Aq Bp + Cq Dp are replaced by the per-QUERY constant E(q) = Aq Bmax + Cq Dmax with the
//     corpus-wide maxima of Bp, Dp.  A per-query constant shifts all of a query's bounds alike, so it never enters
//     the kernel: comparisons, thresholds and keys are unchanged, and the proof adds |q|^2 - E(q) back where it used to
//     add |q|^2 (pack_queries writes that difference, rounded down, into qn).
// L'(q,p) - E(q) <= |q-p|^2 - |q|^2 holds exactly as in the header (Bmax >= Bp, Dmax >= Dp; the accumulation
// allowance g (|C| + sum |products|) is paid by the (1 - g) on the norm and the 2g|p^| inside Bp as before).  The price
// is slack where row norms differ a lot inside one corpus, so the index uses this layout only when
// Bmax <= 1.3 mean(Bp) and Dmax <= 1.3 mean(Dp) (bf16_row_stats_kernel; uniform [0,1) 1M x 128: 1.16 / 1.18).
__host__ __device__ inline bool bf16_ci_dim(int dim) { return dim >= 17 && dim <= 128 && bf16_steps(dim) > (dim + 15) / 16; }
__host__ __device__ inline int bf16_steps_for(int dim, bool ci) { return ci ? (dim + 15) / 16 : bf16_steps(dim); }

// ---------------------------------------------------------------------------
// bf16 helpers on raw bits (host of the proofs above: every rounding direction is explicit)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint16_t bf_rne(float x) {  // finite x
    const uint32_t u = __float_as_uint(x);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float bf_f(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }
__device__ __forceinline__ float f_down(double x) {  // largest float <= x (x >= 0, finite, < 2^127)
    float f = (float)x;
    if ((double)f > x) f = __uint_as_float(__float_as_uint(f) - 1u);
    return f;
}
__device__ __forceinline__ float f_up(double x) {  // smallest float >= x (x >= 0)
    float f = (float)x;
    if ((double)f < x) f = __uint_as_float(__float_as_uint(f) + 1u);
    return f;
}
__device__ __forceinline__ float f_up_signed(double x) {  // smallest float >= x, any sign (finite x)
    float f = (float)x;
    if ((double)f < x) f = (f >= 0.0f) ? __uint_as_float(__float_as_uint(f) + 1u) : __uint_as_float(__float_as_uint(f) - 1u);
    return f;
}
__device__ __forceinline__ uint16_t bf_trunc(float x) { return (uint16_t)(__float_as_uint(x) >> 16); }  // x >= 0
__device__ __forceinline__ uint16_t bf_up(float x) {  // x >= 0: smallest bf16 >= x
    const uint32_t u = __float_as_uint(x);
    return (uint16_t)((u >> 16) + ((u & 0xFFFFu) ? 1u : 0u));
}

// ---- wide rows (D > 128): K-chunked images.  The contraction is cut into chunks of 4 MFMA steps (64 columns); one
// (256-row tile, chunk) piece is a ready-made LDS image of 256 rows x 128 bytes (eight 16-byte slots, XOR-swizzled by
// the row number so that the ds_read_b128 fragment reads are conflict-free without padding).  Corpus and queries
// use the same layout: [tile][chunk][256][64] bf16.
constexpr int kWR = 256;                       // rows (or queries) per wide tile
constexpr int kWPitch = 128;                   // bytes per (row, chunk): 8 slots of 16 B, no padding
constexpr int kWPiece = kWR * kWPitch;         // 32 768 B = 32 LDS-DMA instructions of 1 KiB
constexpr int kWStage = 2 * kWPiece;           // corpus piece + query piece
constexpr int kWDma = kWStage / 1024 / 8;      // LDS-DMA instructions per wave and stage (8)
// Data chunks of a wide row and where the five extra values live: in the zero columns of the last data chunk when it
// has five, else in an EXTRAS PIECE of their own behind the tile's chunks -- 256 rows x 16 columns = 8 KiB, contracted
// by one more MFMA step after the last chunk (same position in the accumulation order as a 13th chunk's first step,
// without that chunk's three zero steps, its barrier and its 64 KiB of LDS-DMA: D = 768 12 chunks instead of 13,
// D = 256 4 instead of 5).
__host__ __device__ inline int bf16_wide_nkc(int dim) { return (dim + 63) / 64; }
__host__ __device__ inline bool bf16_wide_has_x(int dim) { return bf16_extra_col(dim) + 5 > 64 * bf16_wide_nkc(dim); }
constexpr int kWXPiece = kWR * 32;             // extras piece: 32 B per row (two 16-byte slots), 8 LDS-DMA instructions
__host__ __device__ inline size_t bf16_wide_tile_bytes(int dim) {
    return (size_t)bf16_wide_nkc(dim) * kWPiece + (bf16_wide_has_x(dim) ? kWXPiece : 0);
}
// XOR swizzle of the 16-byte slots inside a row: slot' = slot ^ ((row >> 1) & 7).  A ds_read_b128 is served in four
// groups of 16 lanes ({0-3,12-15,20-27}, ...; MI355X_MICROARCH.md, LDS): with it the 16 rows of a group cover all
// eight slots on both 128-byte halves of the 256-byte bank row -- conflict-free without a padding slot.
// (Extras piece, 32-byte rows: slot' = slot ^ ((row >> 3) & 1), conflict-free for the same lane groups.)
__host__ __device__ inline unsigned bf_wide_swz(size_t r) { return (unsigned)((r >> 1) & 7); }
__host__ __device__ inline unsigned bf_wide_xswz(size_t r) { return (unsigned)((r >> 3) & 1); }
__device__ __forceinline__ size_t bf_wide_at(size_t r, int k, int dim) {  // bf16 index of column k of row r
    const int nkc = bf16_wide_nkc(dim);
    const size_t tile = (r / kWR) * (bf16_wide_tile_bytes(dim) / 2), rr = r % kWR;
    if ((k >> 6) >= nkc) {  // extras piece (columns 64 nkc .. 64 nkc + 15)
        const unsigned slot = (unsigned)(((k - 64 * nkc) >> 3) & 1) ^ bf_wide_xswz(rr);
        return tile + (size_t)nkc * (kWPiece / 2) + rr * 16 + (size_t)slot * 8 + (size_t)(k & 7);
    }
    const unsigned slot = (unsigned)((k & 63) >> 3) ^ bf_wide_swz(rr);
    return tile + ((size_t)(k >> 6) * kWR + rr) * (size_t)(kWPitch / 2) + (size_t)slot * 8 + (size_t)(k & 7);
}

// The tile image of a corpus row: its bf16 coordinates + the five extra columns (or, CI layout, its norm in the tile's
// padding chunks).  narrow (D <= 128): img = [n_tiles][64][CP][8] bf16, CP = 2*KS + 1 chunks per row (last chunk is padding).
// T: the index's element type.  An f64 corpus gets the SAME bf16 images (the bound is a statement about real vectors;
// every constant is computed in f64 from the f64 coordinates), so f64 indexes are served by this tier too.
// A query's image: bf16 B row [K] (chunk c at 8c), |q|^2 rounded down (f64), flag; ci: no extra columns,
// qn[q] = |q|^2 (down) - E(q) (up), E(q) = Aq bmax + Cq dmax (header of bf16_ci_dim).
//
// Eight lanes per row (narrow rows): lane `sub` of a row owns the CH = 2 KS columns [sub CH, sub CH + CH) -- 16-byte
// loads from the padded rows, its part of the three f64 sums, an 8-lane butterfly for the row's totals (any summation
// order is inside the 2^-40 the norms are widened by) -- what bf16_pack_queries8_kernel does for queries.  The
// thread-per-row kernels before these read their rows one 4-byte element at a time, 64 rows' lines per instruction, and
// wrote the image in 2-byte stores twice (zero fill, then values): 1M x 128 took 3.46 ms to pack and 2.1 ms for the row
// statistics -- 0.23 TB/s.  x[i] (centred coordinate, f64) and hb[i] (its bf16) of column c0 + i; columns at or beyond
// dim are zero.  Returns false for a non-finite coordinate in the lane's part.
template <typename T>
__device__ __forceinline__ bool bf_row_part8(const T *__restrict__ src, const float *__restrict__ mu, int dim, size_t ld,
                                             int c0, int CH, bool in_rows, uint16_t (&hb)[18], double &pn, double &en,
                                             double &hn) {
    T xf[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) xf[i] = (T)0;
    constexpr int VE = 16 / (int)sizeof(T);  // elements per 16-byte access
    const bool vec = (CH % 4) == 0 && c0 + CH <= (int)ld;  // (rows of the padded copy are 32-byte aligned, ld a multiple of 8)
    if (in_rows) {
        if (vec) {
#pragma unroll
            for (int i = 0; i < 18; i += VE)
                if (i + VE <= CH) {
                    typedef T tv_ __attribute__((ext_vector_type(VE)));
                    const tv_ t4 = *reinterpret_cast<const tv_ *>(src + c0 + i);
#pragma unroll
                    for (int j = 0; j < VE; ++j) xf[i + j] = t4[j];
                }
        } else {
#pragma unroll
            for (int i = 0; i < 18; ++i)
                if (i < CH && c0 + i < dim) xf[i] = src[c0 + i];
        }
    }
    bool finite = true;
    pn = 0.0;
    en = 0.0;
    hn = 0.0;
#pragma unroll
    for (int i = 0; i < 18; ++i) {
        hb[i] = 0;
        const int k = c0 + i;
        if (i < CH && k < dim && in_rows) {
            const double x = (double)xf[i];
            finite = finite && (fabs(x) < 1.0e30);  // also false for NaN
            const double c = x - (double)mu[k];  // centred coordinate (header: translation)
            const float cf = (float)c;
            hb[i] = (fabsf(cf) < 8.67361737988403547e-19f) ? (uint16_t)0 : bf_rne(cf);  // 2^-60
            const double xh = (double)bf_f(hb[i]);
            pn += c * c;
            en += (c - xh) * (c - xh);
            hn += xh * xh;
        }
    }
    uint32_t fin = finite ? 1u : 0u;
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {
        pn += __shfl_xor(pn, d);
        en += __shfl_xor(en, d);
        hn += __shfl_xor(hn, d);
        fin &= (uint32_t)__shfl_xor((int)fin, d);
    }
    return fin != 0u;
}

// narrow rows: the image of row r is CP = 2 KS + 1 chunks of 8 bf16 -- 16 KS data columns, then the padding chunk (CI:
// the f32 norms of the tile's rows 4 rr .. 4 rr + 3 in the padding chunk of its row rr < 16)
template <typename T>
__global__ void bf16_pack_corpus8_kernel(const T *__restrict__ P, const float *__restrict__ mu, size_t n, int dim,
                                         size_t ld, int KS, uint16_t *__restrict__ img, size_t n_rows_img,
                                         uint32_t *__restrict__ bad, int ci) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t r = t >> 3;
    const int sub = (int)(t & 7);
    if (r >= n_rows_img) return;  // (whole groups of eight leave together: n_rows_img * 8 is a multiple of the block size)
    const int CP = 2 * KS + 1, CH = 2 * KS, E = bf16_extra_col(dim);
    const int c0 = sub * CH;
    uint16_t v[18];
    double pn, en, hn;
    const bool in_rows = r < n;
    const bool finite = bf_row_part8<T>(P + r * ld, mu, dim, ld, c0, CH, in_rows, v, pn, en, hn);
    const bool ok = in_rows && finite && (pn < 1.2676506002282294e30);  // 2^100
    if (in_rows && !ok && sub == 0) atomicOr(bad, 1u);
    uint16_t *row = img + r * (size_t)CP * 8;
    if (!ci) {  // the five extra columns: |p|^2 (1 - g) rounded down in three truncated bf16 pieces, then the error terms
        uint16_t x0 = 0, x1 = 0, x2 = 0, x3 = 0, x4 = 0;
        if (!in_rows) {
            x0 = 0x7F00u;  // 1.7e38: never among the k' smallest of real rows (select.hip drops rows >= n anyway)
        } else if (!ok) {
            x0 = 0x7F80u;
        } else {
            double rem = pn * (1.0 - kG) / kUp;
            x0 = bf_trunc(f_down(rem));
            rem -= (double)bf_f(x0);
            x1 = bf_trunc(f_down(rem));
            rem -= (double)bf_f(x1);
            x2 = bf_trunc(f_down(rem));
            const double e_n = sqrt(en) * kUp, h_n = sqrt(hn) * kUp, p_n = sqrt(pn) * kUp;
            x3 = bf_up(f_up((2.0 * e_n + 2.0 * kG * h_n) * (1.0 + 2.0 * kG)));
            x4 = bf_up(f_up(2.0 * p_n * (1.0 + 2.0 * kG)));
        }
#pragma unroll
        for (int i = 0; i < 18; ++i) {
            const int k = c0 + i;
            if (i < CH) {
                if (k == E + 0) v[i] = x0;
                if (k == E + 1) v[i] = x1;
                if (k == E + 2) v[i] = x2;
                if (k == E + 3) v[i] = x3;
                if (k == E + 4) v[i] = x4;
            }
        }
    }
    uint16_t *dst = row + c0;
#pragma unroll
    for (int i = 0; i < 18; i += 2)
        if (i + 2 <= CH) *reinterpret_cast<uint32_t *>(dst + i) = (uint32_t)v[i] | ((uint32_t)v[i + 1] << 16);
    // the padding chunk: zero, except that (CI) the tile's first 16 rows carry the 64 row norms, written by those rows
    const size_t rr = r % kBP;
    if (sub == 1 && !(ci && rr < 16)) {
        typedef uint32_t u4_ __attribute__((ext_vector_type(4)));
        *reinterpret_cast<u4_ *>(row + (size_t)(CP - 1) * 8) = u4_{0u, 0u, 0u, 0u};
    }
    if (ci && sub == 0) {  // |p|^2 (1 - g), rounded down to f32: the chain's initial accumulator value
        const size_t tl = r / kBP;
        float *norm_slot = reinterpret_cast<float *>(img + ((tl * kBP + rr / 4) * (size_t)CP + (size_t)(CP - 1)) * 8) + (rr % 4);
        *norm_slot = ok ? f_down(pn * (1.0 - kG) / kUp) : 1.7e38f;
    }
}

// the row statistics (below), eight lanes per row; a grid-stride loop and one set of atomics per WORKGROUP (a set per
// wave -- 125 k waves on four addresses -- took 5.9 ms for 1M rows, more than the thread-per-row kernel it replaced)
template <typename T>
__global__ __launch_bounds__(256) void bf16_row_stats8_kernel(const T *__restrict__ P, const float *__restrict__ mu,
                                                              size_t n, int dim, size_t ld, int KS, size_t rows,
                                                              double *__restrict__ out) {
    const int sub = (int)(threadIdx.x & 7);
    const int CH = 2 * KS;
    double bm = 0.0, dm = 0.0, bs = 0.0, ds = 0.0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;  // a multiple of 64: whole waves take every trip together
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < rows * 8; t += stride) {
        const size_t r = t >> 3;
        uint16_t v[18];
        double pn, en, hn;
        const bool in_rows = r < n;
        const bool finite = bf_row_part8<T>(P + (in_rows ? r : 0) * ld, mu, dim, ld, sub * CH, CH, in_rows, v, pn, en, hn);
        if (in_rows && sub == 0 && finite && pn < 1.2676506002282294e30) {
            const double bp = (2.0 * sqrt(en) * kUp + 2.0 * kG * sqrt(hn) * kUp) * (1.0 + 2.0 * kG) * kUp;
            const double dp = 2.0 * sqrt(pn) * kUp * (1.0 + 2.0 * kG) * kUp;
            bm = fmax(bm, bp);
            dm = fmax(dm, dp);
            bs += bp;
            ds += dp;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        bm = fmax(bm, __shfl_xor(bm, d));
        dm = fmax(dm, __shfl_xor(dm, d));
        bs += __shfl_xor(bs, d);
        ds += __shfl_xor(ds, d);
    }
    __shared__ double red[4][4];
    const int wave = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0) {
        red[wave][0] = bm;
        red[wave][1] = dm;
        red[wave][2] = bs;
        red[wave][3] = ds;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            bm = fmax(bm, red[w][0]);
            dm = fmax(dm, red[w][1]);
            bs += red[w][2];
            ds += red[w][3];
        }
        atomicMax(reinterpret_cast<unsigned long long *>(out), (unsigned long long)__double_as_longlong(bm));
        atomicMax(reinterpret_cast<unsigned long long *>(out + 1), (unsigned long long)__double_as_longlong(dm));
        atomicAdd(out + 2, bs);
        atomicAdd(out + 3, ds);
    }
}

// The per-row constants Bp, Dp of the bound over the whole corpus (f64, before their bf16 rounding): out[0] = max Bp,
// out[1] = max Dp (bit patterns of non-negative doubles order like integers), out[2] = sum Bp, out[3] = sum Dp.
// Decides whether the CI layout serves this corpus and provides the maxima E(q) is built from.
template <typename T>
__global__ void bf16_row_stats_kernel(const T *__restrict__ P, const float *__restrict__ mu, size_t n, int dim,
                                      size_t ld, double *__restrict__ out) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    double bp = 0.0, dp = 0.0;
    if (r < n) {
        double pn = 0.0, en = 0.0, hn = 0.0;
        bool finite = true;
        const T *src = P + r * ld;
        for (int k = 0; k < dim; ++k) {
            const double x = (double)src[k];
            finite = finite && (fabs(x) < 1.0e30);
            const double c = x - (double)mu[k];
            const float cf = (float)c;
            const uint16_t hb = (fabsf(cf) < 8.67361737988403547e-19f) ? (uint16_t)0 : bf_rne(cf);
            const double xh = (double)bf_f(hb);
            pn += c * c;
            en += (c - xh) * (c - xh);
            hn += xh * xh;
        }
        if (finite && pn < 1.2676506002282294e30) {
            bp = (2.0 * sqrt(en) * kUp + 2.0 * kG * sqrt(hn) * kUp) * (1.0 + 2.0 * kG) * kUp;
            dp = 2.0 * sqrt(pn) * kUp * (1.0 + 2.0 * kG) * kUp;
        }
    }
    double bm = bp, dm = dp, bs = bp, ds = dp;
    for (int d = 32; d > 0; d >>= 1) {
        bm = fmax(bm, __shfl_xor(bm, d));
        dm = fmax(dm, __shfl_xor(dm, d));
        bs += __shfl_xor(bs, d);
        ds += __shfl_xor(ds, d);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(reinterpret_cast<unsigned long long *>(out), (unsigned long long)__double_as_longlong(bm));
        atomicMax(reinterpret_cast<unsigned long long *>(out + 1), (unsigned long long)__double_as_longlong(dm));
        atomicAdd(out + 2, bs);
        atomicAdd(out + 3, ds);
    }
}

// Wide rows (corpus and queries share the K-chunked layout), EIGHT lanes per row: lane `sub` packs the 16-byte slots
// sub, sub + 8, ... (8 columns each: two 16-byte loads, one 16-byte store at the slot's swizzled place), the three f64
// sums go through an 8-lane butterfly, and the slot(s) holding the five extra values are stored last, by their owners,
// with the values in place.  The thread-per-row kernels before this one wrote every row twice in 2-byte stores: 1M x 768
// took 21.4 ms to pack, 10^4 queries 0.28 ms of every step.
template <typename T, bool QRY>
__global__ void bf16_pack_wide8_kernel(const T *__restrict__ X, const float *__restrict__ mu, size_t n_valid,
                                       size_t n_rows_img, int dim, size_t ld, uint16_t *__restrict__ img,
                                       double *__restrict__ qn, uint32_t *__restrict__ qbad, uint32_t *__restrict__ bad,
                                       Bf16SeedModel sm) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t r = t >> 3;
    const int sub = (int)(t & 7);
    if (r >= n_rows_img) return;  // (whole groups of eight leave together)
    double sm_mean = 0.0, sm_var = 0.0;  // (queries, seed model: see bf16_pack_queries8_kernel)
    const int n_slots = 8 * bf16_wide_nkc(dim) + (bf16_wide_has_x(dim) ? 2 : 0);
    const int E = bf16_extra_col(dim);
    const int gx0 = E >> 3, gx1 = (E + 4) >> 3;  // the slot(s) of the extra columns
    const bool in_rows = r < n_valid;
    const T *src = X + r * ld;
    double s = 0.0, en = 0.0, hn = 0.0;
    bool finite = true;
    typedef uint32_t u4_ __attribute__((ext_vector_type(4)));
    auto pack8 = [](const uint16_t (&v)[8]) {
        return u4_{(uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16),
                   (uint32_t)v[4] | ((uint32_t)v[5] << 16), (uint32_t)v[6] | ((uint32_t)v[7] << 16)};
    };
    uint16_t vx[2][8];  // this lane's extras slot(s), stored after the totals are known
#pragma unroll
    for (int j = 0; j < 8; ++j) { vx[0][j] = 0; vx[1][j] = 0; }
    for (int g = sub; g < n_slots; g += 8) {
        const int k0 = 8 * g;
        uint16_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0;
        if (in_rows && k0 < dim) {
            T xf[8];
            constexpr int VE = 16 / (int)sizeof(T);
            typedef T tv_ __attribute__((ext_vector_type(VE)));
#pragma unroll
            for (int i = 0; i < 8; i += VE) {  // (rows are zero padded to ld >= 64 nkc columns, 32-byte aligned)
                const tv_ tt = *reinterpret_cast<const tv_ *>(src + k0 + i);
#pragma unroll
                for (int j = 0; j < VE; ++j) xf[i + j] = tt[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (k0 + j < dim) {
                    const double x = (double)xf[j];
                    finite = finite && (fabs(x) < 1.0e30);  // also false for NaN
                    const double c = x - (double)mu[k0 + j];
                    const float cf = (float)c;
                    const uint16_t hb = (fabsf(cf) < 8.67361737988403547e-19f) ? (uint16_t)0 : bf_rne(cf);  // 2^-60
                    const float xh = bf_f(hb);
                    v[j] = QRY ? bf_rne(-2.0f * xh) : hb;  // (queries: exact, a power-of-two multiple of a bf16 value)
                    s += c * c;
                    const double e = c - (double)xh;
                    en += e * e;
                    hn += (double)xh * (double)xh;
                    if (QRY && sm.seed_out) {
                        sm_mean += c * (double)sm.m1[k0 + j];
                        sm_var += c * (c * (double)sm.a[k0 + j] - (double)sm.b[k0 + j]);
                    }
                }
            }
        }
        if (g == gx0 || g == gx1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) vx[g == gx0 ? 0 : 1][j] = v[j];
        } else {
            *reinterpret_cast<u4_ *>(img + bf_wide_at(r, k0, dim)) = pack8(v);
        }
    }
    uint32_t fin = finite ? 1u : 0u;
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {
        s += __shfl_xor(s, d);
        en += __shfl_xor(en, d);
        hn += __shfl_xor(hn, d);
        fin &= (uint32_t)__shfl_xor((int)fin, d);
    }
    const bool ok = fin != 0u && (s < 1.2676506002282294e30);  // 2^100 (padding rows: sums of nothing)
    uint16_t x[5] = {0, 0, 0, 0, 0};
    if (QRY) {
        x[0] = x[1] = x[2] = 0x3F80u;  // 1.0
        if (ok) {
            x[3] = (uint16_t)(bf_up(f_up(sqrt(hn) * kUp)) | 0x8000u);  // -Aq
            x[4] = (uint16_t)(bf_up(f_up(sqrt(en) * kUp)) | 0x8000u);  // -Cq
        }
    } else if (!in_rows) {
        x[0] = 0x7F00u;  // 1.7e38: never among the k' smallest of real rows (select.hip drops rows >= n anyway)
    } else if (!ok) {
        x[0] = 0x7F80u;
    } else {  // |p|^2 (1 - g), rounded down, in three truncated bf16 pieces, then the two error terms
        double rem = s * (1.0 - kG) / kUp;
        x[0] = bf_trunc(f_down(rem));
        rem -= (double)bf_f(x[0]);
        x[1] = bf_trunc(f_down(rem));
        rem -= (double)bf_f(x[1]);
        x[2] = bf_trunc(f_down(rem));
        const double e_n = sqrt(en) * kUp, h_n = sqrt(hn) * kUp, p_n = sqrt(s) * kUp;
        x[3] = bf_up(f_up((2.0 * e_n + 2.0 * kG * h_n) * (1.0 + 2.0 * kG)));
        x[4] = bf_up(f_up(2.0 * p_n * (1.0 + 2.0 * kG)));
    }
    const bool zero_data = QRY && !ok;  // keep the arithmetic finite; the query is re-run exactly
    if (zero_data)
        for (int g = sub; g < n_slots; g += 8)
            if (g != gx0 && g != gx1) *reinterpret_cast<u4_ *>(img + bf_wide_at(r, 8 * g, dim)) = u4_{0u, 0u, 0u, 0u};
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const int g = w == 0 ? gx0 : gx1;
        if ((w == 1 && gx1 == gx0) || (g & 7) != sub || g >= n_slots) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * g + j;
            if (zero_data) vx[w][j] = 0;
            if (k >= E && k < E + 5) vx[w][j] = x[k - E];
        }
        *reinterpret_cast<u4_ *>(img + bf_wide_at(r, 8 * g, dim)) = pack8(vx[w]);
    }
    if (QRY && sm.seed_out) {
#pragma unroll
        for (int d = 1; d < 8; d <<= 1) {
            sm_mean += __shfl_xor(sm_mean, d);
            sm_var += __shfl_xor(sm_var, d);
        }
    }
    if (sub == 0) {
        if (QRY) {
            qn[r] = ok ? s / kUp : 0.0;
            qbad[r] = ok ? 0u : 1u;
            if (sm.seed_out) {  // starting threshold from the index's seed model; padding and bad queries: -inf
                float sd = __uint_as_float(0xFF800000u);
                if (in_rows && ok) {
                    const double var = sm.v0 + sm_var;
                    sd = f_up_signed(sm.c0 - 2.0 * sm_mean - sm.z * sqrt(var > 0.0 ? var : 0.0));
                }
                const uint32_t key = f2s(sd);
                sm.seed_out[r] = (sd == sd && key != 0xFFFFFFFFu && in_rows && ok) ? key + 1u : f2s(__uint_as_float(0xFF800000u));
            }
        } else if (in_rows && !ok) {
            atomicOr(bad, 1u);
        }
    }
}

// The same for narrow rows with EIGHT lanes per query, each packing a contiguous eighth of the K columns (2 KS of
// them): coalesced 16-byte loads and stores instead of one thread walking 128 coordinates and storing them two bytes at
// a time (C2: 37 -> ~8 us per batch).  The three f64 sums are reduced over the eight lanes; their rounding differs
// from the sequential sums' by ~1e-16 relative, which the factors kUp (1 + 2^-40) cover as before.
// Qp (nullable): the call's FIRST kernel -- Q then is the caller's query array itself (row stride ld, at least dim
// columns), and this kernel also writes the zero-padded f32 copy Qp[nq_pad][ldq] that the re-rank and the next tier read
// (pack_rows_kernel's job) and zeroes the call's 16 counter words `misc` (a memset's job): one launch instead of three.
template <typename T>
__global__ void bf16_pack_queries8_kernel(const T *__restrict__ Q, const float *__restrict__ mu, size_t nq,
                                          size_t nq_pad, int dim, size_t ld, int KS, uint16_t *__restrict__ B,
                                          double *__restrict__ qn, uint32_t *__restrict__ qbad, int ci, double bmax,
                                          double dmax, T *__restrict__ Qp, size_t ldq,
                                          uint32_t *__restrict__ misc, Bf16SeedModel sm) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t q = t >> 3;
    const int sub = (int)(t & 7);
    if (misc && t < 16) misc[t] = 0u;
    if (q >= nq_pad) return;  // (whole groups of eight leave together: nq_pad * 8 is a multiple of the block size)
    const int K = 16 * KS, CH = 2 * KS, E = bf16_extra_col(dim);
    const int c0 = sub * CH;
    uint16_t v[18];  // CH <= 18 (KS <= 9)
    double s = 0.0, en = 0.0, hn = 0.0, sm_mean = 0.0, sm_var = 0.0;
    bool finite = true;
    const T *src = Q + q * ld;
    if (Qp) {  // columns of the padded copy that no lane's eighth of the K columns covers (ldq > K, e.g. D = 100)
        for (int k = K + sub; k < (int)ldq; k += 8) Qp[q * ldq + k] = (T)0;
    }
    // this lane's CH coordinates: 16-byte loads when the source rows allow it (the usual case: a contiguous array
    // with a multiple of four columns), and 16- or 8-byte stores into the padded copy (its rows are 32-byte aligned)
    T xf[18];
    const bool in_rows = q < nq;
    constexpr int VE = 16 / (int)sizeof(T);  // elements per 16-byte access
    const bool vec = (CH % 4) == 0 && ((reinterpret_cast<uintptr_t>(Q) | (ld * sizeof(T))) & 15u) == 0 &&
                     c0 + CH <= dim;
#pragma unroll
    for (int i = 0; i < 18; ++i) xf[i] = (T)0;
    if (in_rows) {
        if (vec) {
#pragma unroll
            for (int i = 0; i < 18; i += VE)
                if (i + VE <= CH) {
                    typedef T tv_ __attribute__((ext_vector_type(VE)));
                    const tv_ t4 = *reinterpret_cast<const tv_ *>(src + c0 + i);
#pragma unroll
                    for (int j = 0; j < VE; ++j) xf[i + j] = t4[j];
                }
        } else {
#pragma unroll
            for (int i = 0; i < 18; ++i)
                if (i < CH && c0 + i < dim) xf[i] = src[c0 + i];
        }
    }
    if (Qp) {
        T *qd = Qp + q * ldq + c0;
#pragma unroll
        for (int i = 0; i < 18; i += 2)
            if (i + 2 <= CH && c0 + i + 2 <= (int)ldq) {  // (CH and ldq are even: pairs never straddle the row end)
                typedef T tp_ __attribute__((ext_vector_type(2)));
                tp_ pr;
                pr[0] = xf[i];
                pr[1] = xf[i + 1];
                *reinterpret_cast<tp_ *>(qd + i) = pr;
            }
    }
    // the translation vector and the seed model's words of this lane's columns: 16-byte loads where the columns allow
    // it (hipMalloc'ed arrays, c0 a multiple of four)
    float muv[18], m1v[18], av[18], bv[18];
    const bool vecm = (CH % 4) == 0 && c0 + CH <= dim;
#pragma unroll
    for (int i = 0; i < 18; i += 4) {
        if (i + 4 <= CH && vecm) {
            typedef float f4_ __attribute__((ext_vector_type(4)));
            const f4_ t4 = *reinterpret_cast<const f4_ *>(mu + c0 + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) muv[i + j] = t4[j];
            if (sm.seed_out) {
                const f4_ x4 = *reinterpret_cast<const f4_ *>(sm.m1 + c0 + i);
                const f4_ y4 = *reinterpret_cast<const f4_ *>(sm.a + c0 + i);
                const f4_ z4 = *reinterpret_cast<const f4_ *>(sm.b + c0 + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    m1v[i + j] = x4[j];
                    av[i + j] = y4[j];
                    bv[i + j] = z4[j];
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = c0 + i + j;
                const bool in = i + j < 18 && i + j < CH && k < dim;
                if (i + j < 18) {
                    muv[i + j] = in ? mu[k] : 0.0f;
                    m1v[i + j] = in && sm.seed_out ? sm.m1[k] : 0.0f;
                    av[i + j] = in && sm.seed_out ? sm.a[k] : 0.0f;
                    bv[i + j] = in && sm.seed_out ? sm.b[k] : 0.0f;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 18; ++i) {
        v[i] = 0;
        const int k = c0 + i;
        if (i < CH && k < dim && q < nq) {
            const double x = (double)xf[i];
            finite = finite && (fabs(x) < 1.0e30);
            const double c = x - (double)muv[i];
            const float cf = (float)c;
            const uint16_t hb = (fabsf(cf) < 8.67361737988403547e-19f) ? (uint16_t)0 : bf_rne(cf);
            const float xh = bf_f(hb);
            v[i] = bf_rne(-2.0f * xh);  // exact: a power-of-two multiple of a bf16 value
            s += c * c;
            const double e = c - (double)xh;
            en += e * e;
            hn += (double)xh * (double)xh;
            if (sm.seed_out) {  // seed model: this coordinate's share of the bound's mean and variance over the corpus
                sm_mean += c * (double)m1v[i];
                sm_var += c * (c * (double)av[i] - (double)bv[i]);
            }
        }
    }
    uint32_t fin = finite ? 1u : 0u;
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {
        s += __shfl_xor(s, d);
        en += __shfl_xor(en, d);
        hn += __shfl_xor(hn, d);
        fin &= (uint32_t)__shfl_xor((int)fin, d);
    }
    if (sm.seed_out) {
#pragma unroll
        for (int d = 1; d < 8; d <<= 1) {
            sm_mean += __shfl_xor(sm_mean, d);
            sm_var += __shfl_xor(sm_var, d);
        }
    }
    const bool ok = fin != 0u && (s < 1.2676506002282294e30);
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 18; ++i)
            if (c0 + i < dim) v[i] = 0;  // keep the arithmetic finite; the query is re-run exactly
    }
    if (!ci) {
#pragma unroll
        for (int i = 0; i < 18; ++i) {
            const int k = c0 + i;
            if (i < CH) {
                if (k == E + 0 || k == E + 1 || k == E + 2) v[i] = 0x3F80u;  // 1.0
                if (ok && k == E + 3) v[i] = (uint16_t)(bf_up(f_up(sqrt(hn) * kUp)) | 0x8000u);  // -Aq
                if (ok && k == E + 4) v[i] = (uint16_t)(bf_up(f_up(sqrt(en) * kUp)) | 0x8000u);  // -Cq
            }
        }
    }
    uint16_t *dst = B + q * (size_t)K + c0;
#pragma unroll
    for (int i = 0; i < 18; ++i)
        if (i < CH) dst[i] = v[i];
    if (sub == 0) {
        if (ci) {
            const double eq = (sqrt(hn) * kUp * bmax + sqrt(en) * kUp * dmax) * kUp;
            qn[q] = ok ? s / kUp - eq : 0.0;
        } else {
            qn[q] = ok ? s / kUp : 0.0;
        }
        qbad[q] = ok ? 0u : 1u;
        if (sm.seed_out) {
            // Starting threshold from the index's seed model (Bf16SeedModel): over the corpus rows p the bound
            // L'(q, p) ~ sum_k (u_k^2 - 2 a_k u_k), u = p - t, a = q - t, has mean c0 - 2 sum a_k M1_k and variance
            // v0 + sum (A_k a_k^2 - B_k a_k) (coordinates taken as independent; z is CALIBRATED against the scout's
            // own seeds on corpus rows at index build, so what the model gets wrong on average is inside z).  ANY
            // threshold is valid: a seed that is too low only sends the query to the next tier (and switches the
            // model off), one that is too high costs appends.  Padding queries and bad ones: -inf (nothing passes).
            float sd = __uint_as_float(0xFF800000u);
            if (q < nq && ok) {
                const double var = sm.v0 + sm_var;
                const double S = sm.c0 - 2.0 * sm_mean - sm.z * sqrt(var > 0.0 ? var : 0.0);
                sd = f_up_signed(S);
            }
            const uint32_t key = f2s(sd);
            sm.seed_out[q] = (sd == sd && key != 0xFFFFFFFFu && q < nq && ok) ? key + 1u : f2s(__uint_as_float(0xFF800000u));
        }
    }
}

// ---------------------------------------------------------------------------
// Cosine indexes (round 4; SURVEY.md 8 f3: "normalise rows once, then the same contraction").  In real arithmetic
// |q/|q| - p/|p||^2 = 2 (1 - cos(q, p)) = twice Cosine::distance, so the Euclidean bound over NORMALISED vectors orders
// rows as the Cosine distance does.  This kernel writes the normalised rows in f64 -- x~_k = x_k * (1 / sqrt(sum x^2)),
// every operation in f64 -- and everything downstream (column sums, row statistics, tile images, the query pack) is
// the f64 instantiation of the Euclidean tier's kernels over them: the bound is a statement about these f64 vectors,
// and select.hip (cos_proof_lb) accounts for what separates them from the reference's float arithmetic.
// Eight lanes per row.  A row whose squared norm is not inside [2^-100, 2^100] (zero rows, non-finite coordinates: the
// reference's distance is NaN or meaningless there) raises *bad (corpus: the index keeps the exact scan) or, nan_rows,
// becomes a row of NaNs (queries: the pack kernel then flags that query for the exact engine).
template <typename T>
__global__ __launch_bounds__(256) void cos_normalize_rows_kernel(const T *__restrict__ X, size_t n_valid, size_t n_out,
                                                                 int dim, size_t ld_in, double *__restrict__ out,
                                                                 size_t ld_out, uint32_t *__restrict__ bad, int nan_rows) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t r = t >> 3;
    const int sub = (int)(t & 7);
    if (r >= n_out) return;  // (whole groups of eight leave together)
    const int CH = (int)(ld_out / 8), c0 = sub * CH;
    double *o = out + r * ld_out + c0;
    if (r >= n_valid) {
        for (int i = 0; i < CH; ++i) o[i] = 0.0;
        return;
    }
    const T *x = X + r * ld_in;
    double ss = 0.0;
    for (int i = 0; i < CH; ++i)
        if (c0 + i < dim) {
            const double v = (double)x[c0 + i];
            ss += v * v;
        }
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) ss += __shfl_xor(ss, d);
    const bool ok = ss >= 7.888609052210118e-31 && ss <= 1.2676506002282294e30;  // 2^-100 .. 2^100 (false for NaN)
    if (!ok) {
        if (nan_rows) {
            for (int i = 0; i < CH; ++i) o[i] = (c0 + i < dim) ? __longlong_as_double(0x7FF8000000000000ll) : 0.0;
        } else {
            if (sub == 0) atomicOr(bad, 1u);
            for (int i = 0; i < CH; ++i) o[i] = 0.0;
        }
        return;
    }
    const double inv = 1.0 / sqrt(ss);
    for (int i = 0; i < CH; ++i) o[i] = (c0 + i < dim) ? (double)x[c0 + i] * inv : 0.0;
}
template <typename T>
hipError_t launch_cos_normalize_rows(const T *X, size_t n_valid, size_t n_out, int dim, size_t ld_in, double *out,
                                     size_t ld_out, uint32_t *bad, bool nan_rows, hipStream_t s) {
    if (ld_out % 8 != 0 || (size_t)dim > ld_out || (size_t)dim > ld_in) return hipErrorInvalidValue;
    const size_t threads = n_out * 8;
    hipLaunchKernelGGL((cos_normalize_rows_kernel<T>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, X, n_valid,
                       n_out, dim, ld_in, out, ld_out, bad, nan_rows ? 1 : 0);
    return hipGetLastError();
}
template hipError_t launch_cos_normalize_rows<float>(const float *, size_t, size_t, int, size_t, double *, size_t, uint32_t *,
                                                     bool, hipStream_t);
template hipError_t launch_cos_normalize_rows<double>(const double *, size_t, size_t, int, size_t, double *, size_t, uint32_t *,
                                                      bool, hipStream_t);

// ---------------------------------------------------------------------------
// compaction of one query's buffer (<= 64*M entries in HBM) by its wave: keep the kp smallest under
// (key, row); returns the kp-th key T and the new count (wave-uniform).  Same radix select as
// compact_query (topk_buffer.h) but the bookkeeping goes back to registers.
// ---------------------------------------------------------------------------
template <int M>
__device__ __forceinline__ void bf_compact_load(const uint2 *ce, uint32_t n, int lane, uint32_t (&key)[M],
                                                uint32_t (&ix)[M]) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const uint32_t slot = m * 64 + lane;
        uint2 e = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        if (slot < n) e = ce[slot];
        key[m] = e.x;
        ix[m] = e.y;
    }
}
__device__ __forceinline__ void sh_store_entry(uint2 *p, uint32_t key, uint32_t row);
// WT: the kept entries are rewritten write-through (shared thresholds: other XCDs read them from memory)
template <int M, bool WT = false>
__device__ __forceinline__ void bf_compact_finish(uint2 *ce, const uint32_t (&key)[M], const uint32_t (&ix)[M],
                                                  uint32_t n, uint32_t kp, int lane, uint32_t &T_out, uint32_t &n_out);
template <int M, bool WT = false>
__device__ __forceinline__ void bf_compact(uint2 *ce, uint32_t n, uint32_t kp, int lane, uint32_t &T_out,
                                           uint32_t &n_out) {
    uint32_t key[M], ix[M];
    bf_compact_load<M>(ce, n, lane, key, ix);
    bf_compact_finish<M, WT>(ce, key, ix, n, kp, lane, T_out, n_out);
}
template <int M, bool WT>
__device__ __forceinline__ void bf_compact_finish(uint2 *ce, const uint32_t (&key)[M], const uint32_t (&ix)[M],
                                                  uint32_t n, uint32_t kp, int lane, uint32_t &T_out, uint32_t &n_out) {
    bool valid[M];
#pragma unroll
    for (int m = 0; m < M; ++m) valid[m] = (uint32_t)(m * 64 + lane) < n;
    uint32_t T = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = T | (1u << bit);
        uint32_t c = 0;
#pragma unroll
        for (int m = 0; m < M; ++m) c += (uint32_t)__popcll(__ballot(valid[m] && key[m] < cand));
        if (c < kp) T = cand;
    }
    uint32_t n_less = 0, n_eq = 0;
    bool sel[M], eq[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        sel[m] = valid[m] && key[m] < T;
        eq[m] = valid[m] && key[m] == T;
        n_less += (uint32_t)__popcll(__ballot(sel[m]));
        n_eq += (uint32_t)__popcll(__ballot(eq[m]));
    }
    const uint32_t need_eq = kp - n_less;
    uint32_t row_cut = 0xFFFFFFFFu;
    if (n_eq > need_eq) {
        uint32_t I = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = I | (1u << bit);
            uint32_t c = 0;
#pragma unroll
            for (int m = 0; m < M; ++m) c += (uint32_t)__popcll(__ballot(eq[m] && ix[m] < cand));
            if (c < need_eq) I = cand;
        }
        row_cut = I;
    }
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t pos = 0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const bool keep = sel[m] || (eq[m] && ix[m] <= row_cut);
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            if (WT) sh_store_entry(ce + pos + (uint32_t)__popcll(mask & lt), key[m], ix[m]);
            else ce[pos + (uint32_t)__popcll(mask & lt)] = make_uint2(key[m], ix[m]);
        }
        pos += (uint32_t)__popcll(mask);
    }
    T_out = T;
    n_out = pos;
}

// KS-step chain of one 32-row block against the wave's two query blocks, while the VALU takes the
// minimum of the OTHER block's bounds (r0, r1) in the matrix pipe's shadow.  The first kLA fragments
// were read by the caller right behind the barrier; fragment ks + kLA is requested at step ks.
// The vector unit is the scarce resource of this loop, not the matrix pipe: an MFMA leaves room for ~6 vector
// instructions per wave pair, so the fast path does nothing per bound but the v_min3 tree (8 instructions per 16
// bounds); which row a surviving minimum belongs to is found in the rare path (bf_slow) by one compare per register.
// (Round 1 tagged every bound with its register number first -- one v_and_or_b32 each, 2/3 of the fast path's vector
// work -- so that the rare path needed no search; with seeded thresholds the rare path is rare enough to search.)
// CI: the chain starts from c0 (the 16 row norms of this lane's rows) instead of zero.
constexpr int kLA = 3;
// Tags (the register number in a bound's low four mantissa bits) are written inside a rare-path entry (bf_slow).
// Measured alternative: the main loop writes them while it takes the minimum (bf_chain_p), for kernels with buffers of
// 128 slots and more, so that an entry needs no tagging pass.  With survivors frequent (1M x 128, k = 100) that was 2 %
// faster than tagging inside the entry -- but the 32 tagged values per chain cost the kernel ~50 registers (the compiler
// keeps them beside the accumulator tuples they came from), the KS >= 5 variants spill, and on long runs it is 10 %
// slower (10M x 128, 10^5 queries, k = 100: 239 vs 215 ms): not used.
constexpr int kBfFinalKeep = 32;  // 64-slot buffers holding at most this many entries end a run uncut
constexpr int kScoutList = 12;  // smallest block minima a lane keeps during a scout pass
// smallest (mn) and second smallest (sec) of 16 finite values: triples give (min3, med3); the second smallest overall
// is the smaller of {second smallest of the triples' minima, the smallest of the triples' medians} -- 21 instructions.
__device__ __forceinline__ void bf_min2(const f32x16 &v, float &mn, float &sec) {
    const float big = 3.4e38f;
    auto lo3 = [](float a, float b, float c) { return fminf(fminf(a, b), c); };
    auto md3 = [](float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); };
    const float l0 = lo3(v[0], v[1], v[2]), d0 = md3(v[0], v[1], v[2]);
    const float l1 = lo3(v[3], v[4], v[5]), d1 = md3(v[3], v[4], v[5]);
    const float l2 = lo3(v[6], v[7], v[8]), d2 = md3(v[6], v[7], v[8]);
    const float l3 = lo3(v[9], v[10], v[11]), d3 = md3(v[9], v[10], v[11]);
    const float l4 = lo3(v[12], v[13], v[14]), d4 = md3(v[12], v[13], v[14]);
    const float l5 = v[15];
    const float a = lo3(l0, l1, l2), am = md3(l0, l1, l2);
    const float b = lo3(l3, l4, l5), bm = md3(l3, l4, l5);
    mn = fminf(a, b);
    const float sec_lo = lo3(fmaxf(a, b), am, bm);       // second smallest of l0 .. l5
    const float dmin = fminf(lo3(d0, d1, d2), fminf(d3, d4));
    sec = fminf(sec_lo, dmin);
    (void)big;
}

template <int KS, bool CI>
__device__ __forceinline__ void bf_chain(const char *arow, const bf16x8 (&pre)[kLA], const bf16x8 (&b0)[KS],
                                         const bf16x8 (&b1)[KS], const f32x16 &c0, f32x16 &w0, f32x16 &w1, f32x16 &r0,
                                         f32x16 &r1, float &m0, float &m1) {
    bf16x8 f[KS];
#pragma unroll
    for (int i = 0; i < kLA && i < KS; ++i) f[i] = pre[i];
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (ks + kLA < KS) f[ks + kLA] = *reinterpret_cast<const bf16x8 *>(arow + 32 * (ks + kLA));
        if (CI) {
            w0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[ks], b0[ks], ks ? w0 : c0, 0, 0, 0);
            w1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[ks], b1[ks], ks ? w1 : c0, 0, 0, 0);
        } else {
            w0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[ks], b0[ks], ks ? w0 : z, 0, 0, 0);
            w1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[ks], b1[ks], ks ? w1 : z, 0, 0, 0);
        }
        // this step's share of the other block's minimum: registers [16 ks / KS, 16 (ks + 1) / KS)
#pragma unroll
        for (int i = 16 * ks / KS; i < 16 * (ks + 1) / KS; ++i) {
            m0 = i ? fminf(m0, r0[i]) : r0[0];
            m1 = i ? fminf(m1, r1[i]) : r1[0];
        }
        // One step = one fragment read (kLA steps ahead of its use), two MFMAs, a slice of the minimum -- and the
        // scheduler keeps it that way.  Left alone it sinks the reads next to their uses to save registers (the kernel
        // sits just under the two-waves-per-SIMD limit) and waits for them with lgkmcnt(0) in the middle of the chain.
        __builtin_amdgcn_sched_barrier(0);
    }
}

// CI layout: the norms of this lane's 16 rows of 32-row block `blk` (C/D map of the 32x32 MFMA: register r holds row
// (r & 3) + 8 (r >> 2) + 4 h).  The norms of rows 4i .. 4i+3 of a tile sit in the padding chunk of its row i.
template <int CP>
__device__ __forceinline__ f32x16 bf_cinit(const char *tb, int blk, int h) {
    typedef float f32x4_ __attribute__((ext_vector_type(4)));
    f32x16 c;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4_ v = *reinterpret_cast<const f32x4_ *>(tb + ((blk * 8 + 2 * g + h) * CP + (CP - 1)) * 16);
        c[4 * g + 0] = v[0];
        c[4 * g + 1] = v[1];
        c[4 * g + 2] = v[2];
        c[4 * g + 3] = v[3];
    }
    return c;
}

// The chain of the software-pipelined main loop.  It starts from registers -- its first kLA fragments `pre` and its
// accumulator init `c` were requested during the PREVIOUS chain -- and in its own last steps, where it has no
// fragments of its own left to request, it requests the same for the NEXT chain (narow / ntb, nblk: the other block of
// this tile, or block 0 of the next tile).  So no chain waits for LDS at its head, and whatever sits between two
// chains (the survivor check, the barrier, the LDS-DMA issue) does not delay the first MFMA behind it by a round trip.
// MID: something to do in front of step MID::at(KS) (the paired kernel's lagging half meets its workgroup in mid-chain,
// bf16_filter_kernel_pair); nothing for everybody else.
struct BfNoMid {
    static constexpr int at(int) { return -1; }
    __device__ __forceinline__ void operator()() const {}
};
template <int KS, bool CI, int CP, typename MID = BfNoMid>
__device__ __forceinline__ void bf_chain_p(const char *arow, bf16x8 (&pre)[kLA], const bf16x8 (&b0)[KS],
                                           const bf16x8 (&b1)[KS], f32x16 &c, f32x16 &w0, f32x16 &w1, f32x16 &r0,
                                           f32x16 &r1, float &m0, float &m1, const char *narow, const char *ntb,
                                           int nblk, int h, MID mid = MID()) {
    typedef float f32x4_ __attribute__((ext_vector_type(4)));
    bf16x8 f[KS];
#pragma unroll
    for (int i = 0; i < kLA && i < KS; ++i) f[i] = pre[i];
    f32x16 z, nc = c;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (ks == MID::at(KS)) mid();
        if (ks + kLA < KS) f[ks + kLA] = *reinterpret_cast<const bf16x8 *>(arow + 32 * (ks + kLA));
        // the next chain's first fragments: fragment i at step max(0, KS - kLA + i)
#pragma unroll
        for (int i = 0; i < kLA; ++i)
            if (ks == (KS - kLA + i > 0 ? KS - kLA + i : 0))
                pre[i] = *reinterpret_cast<const bf16x8 *>(narow + 32 * (i < KS ? i : 0));
        if (CI) {  // ... and its accumulator init: piece g at step max(0, KS - 4 + g)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (ks == (KS - 4 + g > 0 ? KS - 4 + g : 0)) {
                    const f32x4_ v =
                        *reinterpret_cast<const f32x4_ *>(ntb + ((nblk * 8 + 2 * g + h) * CP + (CP - 1)) * 16);
                    nc[4 * g + 0] = v[0];
                    nc[4 * g + 1] = v[1];
                    nc[4 * g + 2] = v[2];
                    nc[4 * g + 3] = v[3];
                }
            w0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[ks], b0[ks], ks ? w0 : c, 0, 0, 0);
            w1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[ks], b1[ks], ks ? w1 : c, 0, 0, 0);
            // c outlives both MFMAs that read it: otherwise the second one accumulates IN c's registers, its proper
            // registers serve as fragment space meanwhile, and sixteen moves that wait for the matrix pipe bring the
            // result home before the last step
            if (ks == 0) asm volatile("" ::"v"(c));
        } else {
            w0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[ks], b0[ks], ks ? w0 : z, 0, 0, 0);
            w1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[ks], b1[ks], ks ? w1 : z, 0, 0, 0);
        }
#pragma unroll
        for (int i = 16 * ks / KS; i < 16 * (ks + 1) / KS; ++i) {  // this step's share of the other block's minimum
            m0 = i ? fminf(m0, r0[i]) : r0[0];
            m1 = i ? fminf(m1, r1[i]) : r1[0];
        }
        __builtin_amdgcn_sched_barrier(0);  // a step stays a step (see bf_chain)
    }
    c = nc;
}

// ---------------------------------------------------------------------------
// Shared thresholds (SH): the segments of a query tighten each other's thresholds DURING the run.
//
// A segment's buffer of a k = 10 call takes ~19 appends into 64 slots, never compacts inside the run, and so its
// threshold stays where the scout's seed put it (the 2.4e-4 quantile) while ~24 rows per query matter: the seed, not k',
// sets the appends -- and every append is a rare-path entry that the whole workgroup waits for at the tile barrier.
// What the segments of a query hold TOGETHER says much more: the r-th smallest bound over the union of their buffers
// is an upper bound of the r-th smallest bound of the whole corpus (the r-th smallest of any subset is), so with
// r > (rows whose bound lies below the k-th neighbour's distance) it is a valid threshold for every segment -- and the
// proof in select.hip does not even need that: rows are only ever dropped against the threshold finally reported.
//  * main workgroups store their entries write-through (sc1) and, every kShPeriod tiles, publish their fill counts
//    (word = epoch | tile tag | count, sc1) after a vmcnt(0): what a published count covers has reached memory;
//  * REFRESHER workgroups -- the grid's last blocks, in the workgroup slots the aligned partition leaves idle (C2: 480
//    of 512) -- loop over the queries: read the segments' words, gather the keys (sc1 loads: the writers sit on other
//    XCDs, whose L2 is not coherent with this one), re-read the words (a word that changed means a buffer may have
//    been rewritten meanwhile: skip), radix-select the r-th smallest in registers, atomicMin it into the query's
//    shared threshold word (the seed array the run started from);
//  * main waves re-read their queries' shared words at the same cadence (issued behind the LDS-DMA, consumed a tile
//    later: nothing waits) and lower their thresholds.
// Nothing waits for another workgroup: a refresher that never runs, runs late or reads stale words only leaves the
// thresholds where they were.  Refreshers leave when every main workgroup has counted itself done (or after a bounded
// number of passes).  Racy or stale reads cannot make an answer wrong -- at worst a threshold drops below the k-th
// neighbour's bound and the query goes to the next tier.
// ---------------------------------------------------------------------------
constexpr uint32_t kShPeriod = 32;      // tiles between two publish / re-read points of a main wave
constexpr uint32_t kShMaxPass = 1u << 14;  // a refresher's pass limit (termination does not depend on the mains)
__device__ __forceinline__ uint32_t sh_load(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sh_store(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sh_store_entry(uint2 *p, uint32_t key, uint32_t row) {  // one 8-byte write-through store
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), ((unsigned long long)row << 32) | key, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
// published word: [31:20] epoch of the launch (1 .. 4095), [19:12] tag = the publishing wave's compaction count so far
// (mod 256): words of one launch with equal tags describe one append-only history of the buffer; [11:0] count
__device__ __forceinline__ uint32_t sh_tag(uint32_t epoch, uint32_t ncomp) { return (epoch << 20) | ((ncomp & 0xFFu) << 12); }

template <int M>
__device__ __forceinline__ void bf_refresher(const uint2 *__restrict__ cand, const uint32_t *pcnt, uint32_t *gtau,
                                          const uint32_t *done, uint32_t n_main, size_t nq_pad, uint32_t nseg,
                                          uint32_t epoch, uint32_t rank, uint32_t wv, uint32_t n_wv, int lane) {
    constexpr uint32_t CAP = 64u * M;
    constexpr int NK = 8;  // keys per lane: up to 512 entries of a query's union (more: the first 512, a subset)
    // lanes 0 .. nseg-1: the segments' published words of a query; lane 63: the mains' done counter
    auto words_of = [&](size_t q) -> uint32_t {
        uint32_t x = 0;
        if (lane < (int)nseg) x = sh_load(pcnt + (size_t)lane * nq_pad + q);
        else if (lane == 63) x = sh_load(done);
        return x;
    };
    for (uint32_t pass = 0; pass < kShMaxPass; ++pass) {
        uint32_t x_next = words_of(wv < nq_pad ? wv : 0);
        for (size_t q = wv; q < nq_pad; q += n_wv) {
            const uint32_t x = x_next;
            x_next = words_of(q + n_wv < nq_pad ? q + n_wv : q);  // the next query's words travel while this one is merged
            if ((uint32_t)__builtin_amdgcn_readlane((int)x, 63) >= n_main) return;
#ifdef PN_DIAG_BF_COUNT
            if (lane == 0) atomicAdd(&g_bfdbg[12], 1ull);
#endif
            uint32_t c = (lane < (int)nseg && (x >> 20) == epoch) ? (x & 0xFFFu) : 0u;
            if (c > CAP) c = 0;
            uint32_t inc = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)inc, d);
                if (lane >= d) inc += t;
            }
            uint32_t U = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
            if (U < rank) continue;
            if (U > 64u * NK) U = 64u * NK;
            const uint32_t excl = inc - c;
            uint32_t key[NK];
#pragma unroll
            for (int i = 0; i < NK; ++i) key[i] = 0xFFFFFFFFu;
            const int nk = (int)((U + 63u) / 64u);  // wave-uniform
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                if (i < nk) {
                    const uint32_t e = (uint32_t)lane + 64u * (uint32_t)i;
                    uint32_t sg = 0, pos = 0;
                    for (uint32_t sgi = 0; sgi < nseg; ++sgi) {
                        const uint32_t os = (uint32_t)__builtin_amdgcn_readlane((int)excl, (int)sgi);
                        const uint32_t cs = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)sgi);
                        if (e >= os && e < os + cs) {
                            sg = sgi;
                            pos = e - os;
                        }
                    }
                    if (e < U) key[i] = sh_load(&cand[((size_t)sg * nq_pad + q) * CAP + pos].x);
                }
            }
            // A buffer is append-only between two compactions of its wave, and a compaction first publishes the buffer
            // as empty under a new tag: if the word read again now has the same epoch and tag and no smaller count, the
            // c entries read in between were not rewritten.  Otherwise skip the query this pass.
            uint32_t x2 = x;
            if (lane < (int)nseg) x2 = sh_load(pcnt + (size_t)lane * nq_pad + q);
            if (__any(lane < (int)nseg && c != 0u && ((x2 >> 12) != (x >> 12) || (x2 & 0xFFFu) < c))) {
#ifdef PN_DIAG_BF_COUNT
                if (lane == 0) atomicAdd(&g_bfdbg[15], 1ull);
#endif
                continue;
            }
#ifdef PN_DIAG_BF_COUNT
            if (lane == 0) atomicAdd(&g_bfdbg[13], 1ull);
#endif
            uint32_t T = 0;
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t cnd = T | (1u << bit);
                uint32_t n_lt = 0;
#pragma unroll
                for (int i = 0; i < NK; ++i)
                    if (i < nk) n_lt += (uint32_t)__popcll(__ballot(key[i] < cnd));
                if (n_lt < rank) T = cnd;
            }
            // T = the rank-th smallest key; rows with a bound EQUAL to it must still pass the strict '<': T + 1
            if (lane == 0 && T < 0xFFFFFFFEu)
                (void)__hip_atomic_fetch_min(gtau + q, T + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#ifdef PN_DIAG_BF_COUNT
        if (lane == 0) atomicAdd(&g_bfdbg[14], 1ull);
#endif
        __builtin_amdgcn_s_sleep(32);
    }
}

// append this lane's survivors of one (32-row block, query block) and compact the buffers that filled up.
// cnt is the fill count of the lane's query (identical in lanes j and j+32, which hold different rows).
// ns counts the vector-memory instructions this wave has issued since its last LDS-DMA (wave-uniform): the
// wait in front of the tile barrier must cover the DMA but not these younger stores (see bf_wait_dma).
// One compare per accumulator register, each answered for the whole wave as a scalar mask; a register without a
// survivor in any lane costs that compare and a scalar branch, the (typically one) register with survivors a short
// append block.  The threshold is laundered through an empty asm first: the compiler otherwise hoists these compares
// into the hot loop, where they cost what the whole fast path costs.
// RAD (radius queries): the threshold is the query's fixed radius bound and every row below it must be kept, so
// a buffer that would need compacting is marked overflowed instead (count > capacity; the host re-runs the call
// on the exact engine) and its threshold drops to -inf so that nothing more is stored.
// SH (shared thresholds, above): entries are stored write-through, and a buffer about to be compacted is first
// published as empty under the wave's next tag (pc_blk = the published words of this query block's 32 buffers, pc_tag =
// epoch | the wave's compaction count, advanced here).
template <int M, bool RAD, bool SH = false>
__device__ __forceinline__ void bf_slow(const f32x16 &acc, float mn, float &tau, uint32_t &cnt, uint32_t row0, int h,
                                        int jq, int lane, uint32_t kp, uint2 *ceq, uint2 *ce_blk,
                                        uint32_t &ns BF_DBG_ARG, uint32_t *pc_blk = nullptr, uint32_t *pc_ncomp = nullptr,
                                        uint32_t pc_epoch = 0) {
    constexpr uint32_t CAP = 64u * M;
    BF_COUNT(0, 1);
#ifdef PN_DIAG_BF_COUNT
    const unsigned long long t0_ = bf_stamp();
    unsigned long long tc_ = 0;
#endif
    float t = tau;
    asm volatile("" : "+v"(t));  // opaque from here on: nothing below can be speculated above the caller's branch
    // The siblings of this wave meet it at the next tile barrier, so its detour is the workgroup's: it outranks the
    // SIMD's other wave (another workgroup, in its chain) for vector issue while it lasts.  Measured on one device:
    // C2 -1 %, 1M x 128 k = 100 -2.5 %; raising the priority of the whole stretch between two chains instead: no gain.
    __builtin_amdgcn_s_setprio(1);
    const uint32_t rowb = row0 + 4 * h;
    // Which registers survive.  Nearly always (C2: 99.7 % of the entries) no lane has more than one -- then the lane's
    // survivor IS its block minimum mn, already known -- so the search is straight-line: sixteen compares whose lane
    // masks are folded on the scalar unit into "some lane has two" (dup) and, per lane, the index of the register that
    // passed.  One store instruction then appends for every surviving lane at once.  (The version before this one
    // branched per register -- sixteen vector-compare -> scalar-branch round trips, 1130 cycles per entry at ~0.4
    // entries per tile and wave; measured alternative to that: all compares first, then a scalar loop over the
    // registers with survivors and a switch to read them, 1320 cycles.)
    // The bounds are tagged here -- each register's number into the low four mantissa bits of a copy -- so that the
    // minimum names its register, the sixteen values are distinct, and "some lane has two survivors" is "its second
    // smallest passes": 16 + 21 instructions (bf_min2) instead of 16 compares + 47 scalar + 16 selects.  An entry is
    // ~100 dependent instructions otherwise, and priced like a 950-cycle sleep (calibrated against timing-only builds
    // whose entries sleep: 256 cycles +0.08 ms on C2, 512 cycles +0.24 ms, the real thing +0.52 ms).
    f32x16 v;
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = __uint_as_float((__float_as_uint(acc[r]) & 0xFFFFFFF0u) | (uint32_t)r);
    float sec;
    bf_min2(v, mn, sec);
    const unsigned long long dup = __ballot(sec < t);
    // (a bound within 15 ulp of the threshold may pass or fail differently tagged: either is a valid filter --
    // the thresholds reported to the proof are tagged values' thresholds minus the allowance, select.hip)
    const uint32_t ridx = (mn < t) ? (__float_as_uint(mn) & 15u) : 16u;
    const unsigned long long seen = __ballot(mn < t);  // (only the counting builds read it)
    (void)seen;
    if (dup == 0ull) {
        const bool p = ridx < 16u;
        const uint32_t pp = p ? 1u : 0u;
        const auto sw = __builtin_amdgcn_permlane32_swap(pp, pp, false, false);
        const uint32_t other = h ? sw[0] : sw[1];  // the other half's lane of the same query
        if (p) {
            const uint32_t o = cnt + (h ? other : 0u);  // half 0 writes first
            // C/D map of the 32x32 MFMA: row = (r & 3) + 8 (r >> 2) + 4 h
            if (SH) sh_store_entry(ceq + o, f2s(mn), rowb + (ridx & 3u) + 8u * (ridx >> 2));
            else ceq[o] = make_uint2(f2s(mn), rowb + (ridx & 3u) + 8u * (ridx >> 2));
        }
        BF_COUNT(1, __popcll(seen));
        cnt += pp + other;
        ns += 1;
    } else
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = acc[r];
        const bool p = v < t;
        if (__any(p)) {
            const uint32_t pp = p ? 1u : 0u;
            const auto sw = __builtin_amdgcn_permlane32_swap(pp, pp, false, false);
            const uint32_t other = h ? sw[0] : sw[1];  // the other half's lane of the same query
            if (p) {
                const uint32_t o = cnt + (h ? other : 0u);  // half 0 writes first
                // C/D map of the 32x32 MFMA: row = (r & 3) + 8 (r >> 2) + 4 h
                if (SH) sh_store_entry(ceq + o, f2s(v), rowb + (uint32_t)((r & 3) + 8 * (r >> 2)));
                else ceq[o] = make_uint2(f2s(v), rowb + (uint32_t)((r & 3) + 8 * (r >> 2)));
            }
            BF_COUNT(1, __popcll(__ballot(p)));
            cnt += pp + other;
            ns += 1;
        }
    }
    if (RAD) {
        if (cnt > CAP - 32) {  // would need compacting: overflow, and nothing more is stored
            cnt = CAP + 1;
            tau = __uint_as_float(0xFF800000u);
        }
        __builtin_amdgcn_s_setprio(0);
        return;
    }
    unsigned long long need = __ballot(h == 0 && cnt > CAP - 32);
    if (need) {
#ifdef PN_DIAG_BF_COUNT
        tc_ = bf_stamp();
#endif
        if (SH) {  // the buffers about to be rewritten read "empty" to the refreshers from here to the next publish
            *pc_ncomp += 1u;
            if (h == 0 && ((need >> jq) & 1ull)) sh_store(pc_blk + jq, sh_tag(pc_epoch, *pc_ncomp));
        }
        // the entries were stored by both halves of the wave: they must have left before they are read back
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ns = 0;
        do {
            const int j = __builtin_ctzll(need);
            need &= need - 1;
            const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane((int)cnt, j);
            uint32_t T, nn;
            BF_COUNT(2, 1);
            bf_compact<M, SH>(ce_blk + (size_t)j * CAP, cj, kp, lane, T, nn);
            if (jq == j) {
                tau = fminf(tau, s2f(T));  // never RAISED (a shared word may have lowered tau below entries stored earlier): what is
                                           // reported must be <= every value rows were dropped against
                cnt = nn;
            }
        } while (need);
        ns += 16;  // at least: forces the plain wait at the next barrier
    }
    __builtin_amdgcn_s_setprio(0);
#ifdef PN_DIAG_BF_COUNT
    {
        const unsigned long long t3_ = bf_stamp();
        BF_COUNT(3, t3_ - t0_);
        if (tc_) BF_COUNT(4, t3_ - tc_);
    }
#endif
}

// Wait until this wave's LDS-DMA has landed WITHOUT waiting for the youngest candidate stores: vector-memory
// operations of a wave retire in order, so "at most N outstanding" is enough for any N <= ns when ns store
// instructions were issued after the DMA.  s_waitcnt takes an immediate; three cases (N = min(ns, 2)) cover what
// matters -- the one or two stores of a rare-path entry right in front of the barrier are not waited for, older ones
// (half a tile ago or more) have long landed.  (A 16-way switch on ns compiled into a tree of ~10 scalar branches on
// every tile's critical path.)
template <bool EXACT = false>
__device__ __forceinline__ void bf_wait_dma(uint32_t ns) {
    if (ns == 0u)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (ns == 1u)
        asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if (!EXACT || ns == 2u)
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else  // the wide kernel filters eight blocks right in front of a chunk barrier: up to 16 stores just issued
        switch (ns < 15u ? ns : 15u) {
            case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
            case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
            case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
            case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
            case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
            case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
            case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
            case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
            case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
            case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
            case 13: asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); break;
            case 14: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
            default: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
        }
}

// cand: [nseg][nq_pad][64*M] (key, row) pairs; ccnt/ctau: [nseg][nq_pad], pre-initialised to 0 / sortable(+inf)
// MODE 0: a run may scout for itself, then filters (plans without a shared scout); 1: scout-only launch (scout_out
// given, no buffers touched); 2: filter with the thresholds in tau_init (no scout code: the scout pass's lists and
// accumulators would otherwise set the kernel's register count, and main-loop values would live in scratch).
// SH (MODE 2 only): shared thresholds -- the first n_main blocks are the main workgroups, the rest refreshers; sh =
// {pcnt, done, epoch, rank} (see "Shared thresholds" above); tau_init is then also the array of shared words.
struct BfShared {
    uint32_t *pcnt;   // published fill counts [nseg][nq_pad]
    uint32_t *done;   // main workgroups that have finished (zeroed by the host before the launch)
    uint32_t n_main;  // main workgroups (the grid has more blocks: the refreshers)
    uint32_t epoch;   // 1 .. 4095, different from the previous launch on these buffers
    uint32_t rank;    // r: the shared threshold is the r-th smallest bound of the union
    uint32_t nseg;    // segments per query
    // seed in the kernel (Bf16SeedLists in pn_internal.h): lists of the scout launch -> starting thresholds (main launch);
    // words the scout launch sets to +inf
    const float *seed_lists;
    uint32_t seed_rank, seed_nq;
    uint32_t *seed_words;
};

// Starting threshold of query q from the scout launch's lists (what bf16_seed_kernel computes, in the main launch's
// prologue: a lane per query).  Every (segment, lane half) list is sorted ascending; the rank-th smallest of the union
// of their first kSeedTake entries is the rank-th smallest of the whole union unless one list holds more than
// kSeedTake of the rank smallest, and then it is larger -- a looser start, never an invalid one (ANY start is valid).
typedef float f32x4_t __attribute__((ext_vector_type(4)));
constexpr int kSeedTake = 3;
__device__ __forceinline__ float bf_seed_lane(const float *__restrict__ lists, size_t nq_pad, uint32_t nseg, uint32_t rank,
                                              size_t q) {
    const float inf = __uint_as_float(0x7F800000u);
    float l[kScoutList];
#pragma unroll
    for (int i = 0; i < kScoutList; ++i) l[i] = inf;
    auto insert = [&](float x) {  // keep the kScoutList smallest, ascending
        float c = x;
#pragma unroll
        for (int i = 0; i < kScoutList; ++i) {
            const float lo = fminf(l[i], c);
            c = fmaxf(l[i], c);
            l[i] = lo;
        }
    };
    static_assert(kScoutList % 4 == 0 && kSeedTake <= 4, "list heads are read as one 16-byte load");
    const f32x4_t *p = reinterpret_cast<const f32x4_t *>(lists + q * (size_t)(2 * kScoutList));
    const size_t seg_stride = nq_pad * (size_t)(2 * kScoutList) / 4;  // in 16-byte words
#pragma unroll 4
    for (uint32_t sg = 0; sg < nseg; ++sg) {
        const f32x4_t a = p[(size_t)sg * seg_stride], b = p[(size_t)sg * seg_stride + kScoutList / 4];
#pragma unroll
        for (int i = 0; i < kSeedTake; ++i) {
            insert(a[i]);
            insert(b[i]);
        }
    }
    float r = l[0];
#pragma unroll
    for (int i = 1; i < kScoutList; ++i) r = (uint32_t)i + 1u == rank ? l[i] : r;
    return r;
}
template <int KS, int M, bool RAD, bool CI, int MODE, bool SH = false>
__global__ __launch_bounds__(256, 2) void bf16_filter_kernel(const char *__restrict__ img, uint32_t n_tiles,
                                                             const u32x4 *__restrict__ Bq, uint32_t q_tiles,
                                                             uint32_t kp_keep, uint2 *__restrict__ cand,
                                                             uint32_t *__restrict__ ccnt,
                                                             uint32_t *__restrict__ ctau, size_t nq_pad,
                                                             uint32_t split, uint32_t seg_per_part,
                                                             uint32_t scout_max,
                                                             const uint32_t *tau_init,
                                                             float *__restrict__ scout_out, BfShared sh) {
    static_assert(!SH || (MODE == 2 && !RAD), "shared thresholds: main pass of a k-NN call only");
    // k' in the low half; the high half: entries up to which a buffer ends its run uncut (0: k'; see the end of a run)
    const uint32_t kp = kp_keep & 0xFFFFu, keep_arg = kp_keep >> 16;
    constexpr int C = 2 * KS, CP = C + 1;
    constexpr uint32_t CAP = 64u * M;
    constexpr int TB = kBP * CP * 16;  // bytes per tile image
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    char *tiles = reinterpret_cast<char *>(smem_raw);  // [NBUF][TB] (the scout pass uses two of them)
    // the workgroup's arrival counter of the split tile barrier (main loop), behind the three tile buffers
    constexpr int NBUF = 3;
    // Split tile barrier (below) for the kernels whose survivors are frequent (buffers of 128 slots and more: k' > 16).
    // Measured on one device, full s_barrier vs split: 1M x 128 k = 100 3.62 -> 3.46 ms per step; C2 (64-slot buffers,
    // shared thresholds) 2.29 vs 2.31-2.36: not there.  A fourth tile buffer (landing waited for 1.5 tiles after the
    // request instead of 0.5) made C2 4 % slower and changed nothing at k = 100: the wait is not LDS-DMA latency.
    constexpr bool kSplit = M >= 2;
    volatile uint32_t *arrive = reinterpret_cast<volatile uint32_t *>(tiles + NBUF * TB);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int jq = lane & 31, h = lane >> 5;
    BF_DBG_DECL;
    if (SH && blockIdx.x >= sh.n_main) {  // a refresher workgroup: four waves over the queries, until the mains are done
        const uint32_t n_wv = (gridDim.x - sh.n_main) * 4u, wv = (blockIdx.x - sh.n_main) * 4u + (uint32_t)wave;
        bf_refresher<M>(cand, sh.pcnt, const_cast<uint32_t *>(tau_init), sh.done, sh.n_main, nq_pad, sh.nseg, sh.epoch,
                        sh.rank, wv, n_wv, lane);
        return;
    }

    // Work list: (query tile, row part, tile within the part) in that order; `split` row parts per query tile
    // (1 unless the host wants more, shorter segments per query: see bf16_slots in index.hip), tps tiles each
    // (the last part may be shorter: its tail units are empty).  Workgroup w owns the contiguous slice
    // [w U / W, (w+1) U / W) and walks it in runs that stay inside one (query tile, part).
    const uint32_t tps = (n_tiles + split - 1) / split;
    const unsigned long long U = (unsigned long long)q_tiles * split * tps;
    const unsigned long long W = SH ? sh.n_main : gridDim.x;
    unsigned long long w = blockIdx.x;
    // Which slice a hardware block takes (aligned grids: c = W / q_tiles whole workgroups per query tile, slice
    // q c + p = row range p of query tile q).  Hardware block b runs on XCD b % 8 and every XCD has its own L2, so
    // the blocks of one XCD take a contiguous range of the RANGE-MAJOR order (p, q): the workgroups resident on an
    // XCD at any time -- 2 per CU, started together or as their predecessors finish together -- are different query
    // tiles walking the SAME row range, and a tile image one of them brought into L2 serves the others.  In
    // query-major order the residents of an XCD walk c different ranges, and in a grid that runs in rounds a
    // finished workgroup's successor starts a range from its beginning, alone (10M x 128, 10^5 queries: L2 hit
    // rate 9 %, 0.98 TB from HBM per step, 3.9 TB/s).
    if (split == 1 && W >= q_tiles && W % q_tiles == 0) {
        const uint32_t b = blockIdx.x, x = b & 7u, base = (uint32_t)W >> 3, rem = (uint32_t)W & 7u;
        const uint32_t L = x * base + (x < rem ? x : rem) + (b >> 3);  // XCDs 0 .. rem-1 run base + 1 blocks
        const uint32_t c = (uint32_t)W / q_tiles;
        w = (unsigned long long)(L % q_tiles) * c + L / q_tiles;
    }
    unsigned long long u0 = w * U / W;
    const unsigned long long u1 = (w + 1) * U / W;

    // wave w moves the consecutive pieces [w P, w P + P) of a tile
    constexpr int P = (CP + 3) / 4;
    const int n_mine = CP - wave * P < P ? (CP - wave * P > 0 ? CP - wave * P : 0) : P;  // (the last wave may have fewer)
    auto dma_tile = [&](uint32_t rt, int buf) {
        const char *src = img + (size_t)rt * (size_t)TB + lane * 16;
        char *dst = tiles + buf * TB;
        // one address register and one M0 value serve four pieces through the instruction's immediate offset (which
        // advances the global and the LDS address alike)
        const char *ws = src + wave * (P * 1024);
        char *wd = dst + wave * (P * 1024);
        static_assert(P <= 5, "piece schedule written out for up to five pieces per wave");
        if (0 < n_mine) __builtin_amdgcn_global_load_lds((glb_void_b *)ws, (lds_void_b *)wd, 16, 0, 0);
        if (P > 1 && 1 < n_mine) __builtin_amdgcn_global_load_lds((glb_void_b *)ws, (lds_void_b *)wd, 16, 1024, 0);
        if (P > 2 && 2 < n_mine) __builtin_amdgcn_global_load_lds((glb_void_b *)ws, (lds_void_b *)wd, 16, 2048, 0);
        if (P > 3 && 3 < n_mine) __builtin_amdgcn_global_load_lds((glb_void_b *)ws, (lds_void_b *)wd, 16, 3072, 0);
        if (P > 4 && 4 < n_mine)
            __builtin_amdgcn_global_load_lds((glb_void_b *)(ws + 4096), (lds_void_b *)(wd + 4096), 16, 0, 0);
    };

    while (u0 < u1) {
        const unsigned long long v = u0 / tps;  // (query tile, part)
        const uint32_t qt = (uint32_t)(v / split), part = (uint32_t)(v % split);
        const unsigned long long v_begin = v * tps, v_end = v_begin + tps;
        const unsigned long long run_end = u1 < v_end ? u1 : v_end;
        const uint32_t rt0 = part * tps + (uint32_t)(u0 - v_begin);
        uint32_t rt1 = part * tps + (uint32_t)(run_end - v_begin);
        if (rt1 > n_tiles) rt1 = n_tiles;
        if (rt0 >= rt1) {  // empty tail of the last part
            u0 = run_end;
            continue;
        }
        // ordinal of this workgroup among those touching (query tile, part) v
        unsigned long long wf = v_begin * W / U;
        while ((wf + 1) * U / W <= v_begin) ++wf;
        while (wf > 0 && wf * U / W > v_begin) --wf;
        const uint32_t seg = part * seg_per_part + (uint32_t)(w - wf);
        const size_t q0 = (size_t)qt * kBQ + (size_t)wave * 64;  // first query of this wave
        const size_t cell0 = (size_t)seg * nq_pad + q0;          // its (segment, query) cell
#if defined(PN_DIAG_BF_COUNT)
        const unsigned long long trun0_ = bf_stamp();
        unsigned long long treal0_;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(treal0_)::"memory");
#endif

        // ---- per-run state: B fragments, thresholds and counts in registers
        bf16x8 b0[KS], b1[KS];
        {
            const u32x4 *br0 = Bq + (q0 + jq) * (size_t)C + h;
            const u32x4 *br1 = br0 + (size_t)32 * C;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const u32x4 v0 = br0[2 * ks], v1 = br1[2 * ks];
                b0[ks] = __builtin_bit_cast(bf16x8, v0);
                b1[ks] = __builtin_bit_cast(bf16x8, v1);
            }
        }
        float tau0 = __uint_as_float(0x7F800000u), tau1 = tau0;
        uint32_t cnt0 = 0, cnt1 = 0;

        // ---- scout pass.  A buffer that starts from tau = +inf admits ~k' ln(n/k') rows before its threshold
        // has converged, and with 2048 waves x 64 buffers warming up at once those appends, not the MFMAs, set
        // the kernel's time.  So the first t tiles of the run are first contracted WITHOUT buffers: each lane
        // keeps the 5 smallest of its block minima (16 rows each); the 5th smallest of both lane halves' lists is
        // the starting threshold of the real pass (about the 1e-3 quantile of the segment's bounds: ~30x fewer
        // rows pass it than pass a cold buffer, and it is far above the k-th neighbour's bound).  ANY starting
        // value is valid -- rows are only ever dropped against the threshold that is finally reported -- a
        // threshold that turns out too low merely sends the query to the next tier.
        const uint32_t run_len = rt1 - rt0;
        uint32_t t_scout = run_len / 16u < 64u ? run_len / 16u : 64u;
        if (t_scout > scout_max) t_scout = scout_max;  // host: keeps the scouted rows' share of true neighbours tiny
        if (t_scout < 4u) t_scout = 0;
        if (MODE == 2 || tau_init) {  // thresholds given by the caller (radius queries, shared seed): no scouting
            t_scout = 0;
            if (MODE == 2 && !RAD && sh.seed_lists) {
                // lane L derives query q0 + L's threshold (bf_seed_lane); the lanes (jq, h) then pick up their two.
                // A padding query of the last tile gets -inf: nothing passes, it costs no appends.
                const size_t ql = q0 + (size_t)lane;
                float sd = __uint_as_float(0xFF800000u);
                if (ql < (size_t)sh.seed_nq) {
                    const uint32_t key = f2s(bf_seed_lane(sh.seed_lists, nq_pad, sh.nseg, sh.seed_rank, ql));
                    sd = s2f(key == 0xFFFFFFFFu ? key : key + 1u);  // rows with a bound EQUAL to it still pass the strict '<'
                }
                tau0 = __shfl(sd, jq);
                tau1 = __shfl(sd, 32 + jq);
            } else {
                tau0 = s2f(SH ? sh_load(tau_init + q0 + jq) : tau_init[q0 + jq]);
                tau1 = s2f(SH ? sh_load(tau_init + q0 + 32 + jq) : tau_init[q0 + 32 + jq]);
            }
        }
        if (MODE == 1 || (MODE == 0 && scout_out)) {  // scout-only launch: every run contributes its lists
            t_scout = run_len < scout_max ? run_len : scout_max;
            if (t_scout < 1u) t_scout = 1u;
        }
        if (MODE != 2 && t_scout) {
            const float inf = __uint_as_float(0x7F800000u);
            float s0[kScoutList], s1[kScoutList];
#pragma unroll
            for (int i = 0; i < kScoutList; ++i) { s0[i] = inf; s1[i] = inf; }
            auto insert = [](float (&l)[kScoutList], float x) {  // keep the kScoutList smallest, ascending
                float c = x;
#pragma unroll
                for (int i = 0; i < kScoutList; ++i) {
                    const float lo = fminf(l[i], c);
                    c = fmaxf(l[i], c);
                    l[i] = lo;
                }
            };
            __syncthreads();
            dma_tile(rt0, 0);
            __syncthreads();
            f32x16 x00, x01, x10, x11;
#pragma unroll
            for (int r = 0; r < 16; ++r) { x00[r] = inf; x01[r] = inf; x10[r] = inf; x11[r] = inf; }
            int cs = 0;
            for (uint32_t rt = rt0; rt < rt0 + t_scout; ++rt, cs ^= 1) {
                const char *tb = tiles + cs * TB;
                const char *arow0 = tb + (jq * CP + h) * 16;
                const char *arow1 = arow0 + 32 * CP * 16;
                bf16x8 pre0[kLA], pre1[kLA];
#pragma unroll
                for (int i = 0; i < kLA; ++i) {
                    pre0[i] = *reinterpret_cast<const bf16x8 *>(arow0 + 32 * (i < KS ? i : 0));
                    pre1[i] = *reinterpret_cast<const bf16x8 *>(arow1 + 32 * (i < KS ? i : 0));
                }
                f32x16 c0 = x00, c1 = x00;  // (placeholders unless CI)
                if (CI) {
                    c0 = bf_cinit<CP>(tb, 0, h);
                    c1 = bf_cinit<CP>(tb, 1, h);
                }
                if (rt + 1 < rt0 + t_scout) dma_tile(rt + 1, cs ^ 1);
                float m0, m1;
                bf_chain<KS, CI>(arow0, pre0, b0, b1, c0, x00, x01, x10, x11, m0, m1);
                insert(s0, m0);
                insert(s1, m1);
                bf_chain<KS, CI>(arow1, pre1, b0, b1, c1, x10, x11, x00, x01, m0, m1);
                insert(s0, m0);
                insert(s1, m1);
                __syncthreads();
            }
            float m0 = x10[0], m1 = x11[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) {
                m0 = fminf(m0, x10[i]);
                m1 = fminf(m1, x11[i]);
            }
            insert(s0, m0);
            insert(s1, m1);
            if (MODE == 1 || (MODE == 0 && scout_out)) {
                // publish this lane's lists: [cell][half][kScoutList]; bf16_seed_kernel merges the cells of a query
                float *o0 = scout_out + ((cell0 + jq) * 2 + h) * kScoutList;
                float *o1 = scout_out + ((cell0 + 32 + jq) * 2 + h) * kScoutList;
#pragma unroll
                for (int i = 0; i < kScoutList; ++i) {
                    o0[i] = s0[i];
                    o1[i] = s1[i];
                }
                // seed in the kernel: the words the main launch's refreshers lower start at +inf (the main waves
                // derive their own starting thresholds from the lists)
                if (sh.seed_words && seg == 0u) sh_store(sh.seed_words + q0 + (size_t)lane, 0xFF800000u);
                u0 = run_end;
                continue;
            }
            // 5th smallest of the UNION of the two lane halves' lists (both sorted ascending):
            // min(b5, max(a1,b4), max(a2,b3), max(a3,b2), max(a4,b1), a5)
            auto union5 = [](const float (&a)[kScoutList]) {
                const float b1 = __shfl_xor(a[0], 32), b2 = __shfl_xor(a[1], 32), b3 = __shfl_xor(a[2], 32),
                            b4 = __shfl_xor(a[3], 32), b5 = __shfl_xor(a[4], 32);
                const float x = fminf(fminf(a[4], b5), fminf(fmaxf(a[0], b4), fmaxf(a[3], b1)));
                return fminf(x, fminf(fmaxf(a[1], b3), fmaxf(a[2], b2)));
            };
            tau0 = union5(s0);
            tau1 = union5(s1);
        }
        if (MODE == 1) {  // (a scout-only run always left through the `continue` above)
            u0 = run_end;
            continue;
        }
        uint2 *ce_blk0 = cand + cell0 * CAP;              // query block 0: 32 buffers
        uint2 *ce_blk1 = ce_blk0 + (size_t)32 * CAP;      // query block 1
        uint2 *ceq0 = ce_blk0 + (size_t)jq * CAP, *ceq1 = ce_blk1 + (size_t)jq * CAP;
        uint32_t ns = 0;

        // The survivors of a (32-row block, query block) check: a branch into bf_slow, which finds the survivors' registers
        // and appends them at once (a check finds a survivor in ~20 % of the cases at small k').  Measured alternative:
        // branch-free capture into two pending register slots per lane inside the next chain's shadow, appended in
        // batches -- ~80 vector instructions more per chain whether anything survives or not, ~25 registers over the
        // budget of two workgroups per CU.  Measured on one device, 1M rows: k = 10 2.79 (branch) vs 3.14 ms (capture) at
        // D = 128, 2.10 vs 2.24 at D = 64; k = 100 4.50 vs 4.20 at D = 128, 3.98 vs 3.18 at D = 64 -- but the spills cost
        // more than that on the plans that scout for themselves (configs[2] at full size: 250 -> 335 ms): not used.
        // Software pipeline over the tiles of the run, three LDS buffers (tile rt in buffer (rt - rt0) % 3):
        //   chain A: block 0 of tile rt -> a0x, the VALU takes the minima of a1x (block 1 of tile rt-1) in its shadow;
        //            its last steps request block 1's first fragments and accumulator init
        //   survivors of a1x (rare path)
        //   barrier -- in the MIDDLE of the tile: every wave's pieces of tile rt+1 have landed (they were issued a whole
        //            tile ago, so the wait is over before it starts) and nobody reads tile rt-1 any more; LDS-DMA of
        //            tile rt+2 into that buffer.  What follows the barrier needs nothing the barrier provides:
        //   chain B: block 1 of tile rt -> a1x, minima of a0x; its last steps request block 0 of tile rt+1
        //   survivors of a0x (rare path)
        // With two buffers and the barrier at the end of a tile (round 1) every tile began cold behind the barrier:
        // fragment and norm reads, their round trip, the DMA issue -- a quarter of a wave's time with no MFMA in it
        // (measured with per-section stamps, rare path compiled out: 628 of 2 630 cycles per tile).
        __syncthreads();  // previous run's readers are done with the buffers
        dma_tile(rt0, 0);
        if (rt0 + 1 < rt1) dma_tile(rt0 + 1, 1);
        if (tid == 0) *arrive = 0u;
        __syncthreads();  // carries the vmcnt(0): the first NBUF - 1 tiles are in LDS
        f32x16 a00, a01, a10, a11;
#pragma unroll
        for (int r = 0; r < 16; ++r) {  // "nothing here yet": above every threshold
            a00[r] = 3.0e38f;
            a01[r] = 3.0e38f;
            a10[r] = 3.0e38f;
            a11[r] = 3.0e38f;
        }
        bf16x8 pre[kLA];
        f32x16 cc = a00;  // (placeholder unless CI)
        {
            const char *ar = tiles + (jq * CP + h) * 16;
#pragma unroll
            for (int i = 0; i < kLA; ++i) pre[i] = *reinterpret_cast<const bf16x8 *>(ar + 32 * (i < KS ? i : 0));
            if (CI) cc = bf_cinit<CP>(tiles, 0, h);
        }
        ns = 0;
        int cur = 0;
        // shared thresholds: this wave's published words / shared words, the values re-read at the last publish point
        uint32_t *pc_blk0 = SH ? sh.pcnt + cell0 : nullptr, *pc_blk1 = SH ? sh.pcnt + cell0 + 32 : nullptr;
        const uint32_t *gw0 = tau_init + q0 + jq, *gw1 = gw0 + 32;
        uint32_t g0 = 0, g1 = 0, sh_ncomp = 0;  // sh_ncomp: this wave's compactions so far (wave-uniform)
        bool g_pending = false;  // (wave-uniform)
        for (uint32_t rt = rt0; rt < rt1; ++rt) {
            const int nxt = cur == NBUF - 1 ? 0 : cur + 1, prv = cur == 0 ? NBUF - 1 : cur - 1;
            const bool sh_point = SH && ((rt - rt0) % kShPeriod) == kShPeriod - 1;  // (wave-uniform)
            const char *tb = tiles + cur * TB;
            const char *arow0 = tb + (jq * CP + h) * 16;
            const char *arow1 = arow0 + 32 * CP * 16;
            float m0, m1, p0, p1;
            // SPLIT TILE BARRIER (kSplit).  What the workgroup's one meeting per tile certifies -- every wave's LDS-DMA pieces of
            // tile rt+1 have landed, and nobody reads tile rt-1 any more (its buffer takes tile rt+2) -- is true of THIS
            // wave here, at the top of tile rt, and is needed only in the middle of the tile, a whole MFMA chain and a
            // survivor check later.  So the wave ARRIVES here (its pieces have landed: the counted vmcnt wait; its reads
            // of tile rt-1 are older LDS operations than the add, and LDS operations of a wave execute in order) and
            // WAITS in the middle, for a count instead of at an s_barrier: a sibling delayed by up to a chain -- the one
            // rare-path entry that made the other three wait at every such barrier (a wave's time at the barrier was
            // 26 % of its run, most of it waiting for siblings' detours) -- no longer stops anybody.
            if (kSplit && rt > rt0) {
                bf_wait_dma(ns);
                if (lane == 0) __hip_atomic_fetch_add(const_cast<uint32_t *>(arrive), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
#if defined(PN_DIAG_BF_COUNT)
            unsigned long long tc0_ = bf_stamp_nw();
#endif
            bf_chain_p<KS, CI, CP>(arow0, pre, b0, b1, cc, a00, a01, a10, a11, m0, m1, arow1, tb, 1, h);
#if defined(PN_DIAG_BF_COUNT)
            {
                unsigned long long tc1_ = bf_stamp_nw();
                bf_settle(tc1_);
                bf_settle(tc0_);
                BF_COUNT(9, tc1_ - tc0_);
            }
#endif
            if (rt == rt0) { m0 = __uint_as_float(0x7F800000u); m1 = m0; }  // nothing precedes the first tile
            if (__any(m0 < tau0 || m1 < tau1)) {
                const uint32_t row0 = (rt - 1) * kBP + 32;
                if (__any(m0 < tau0)) bf_slow<M, RAD, SH>(a10, m0, tau0, cnt0, row0, h, jq, lane, kp, ceq0, ce_blk0, ns BF_DBG_PASS, pc_blk0, &sh_ncomp, sh.epoch);
                if (__any(m1 < tau1)) bf_slow<M, RAD, SH>(a11, m1, tau1, cnt1, row0, h, jq, lane, kp, ceq1, ce_blk1, ns BF_DBG_PASS, pc_blk1, &sh_ncomp, sh.epoch);
            }
            // mid-tile barrier
#if defined(PN_DIAG_BF_COUNT)
            const unsigned long long tb0_ = bf_stamp();
#endif
            if (!kSplit) {  // everything at one s_barrier in the middle of the tile
                if (sh_point) ns = 0;  // a publish point: every entry stored so far must have reached memory (vmcnt(0))
                bf_wait_dma(ns);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            } else {
                if (rt > rt0) {  // all four waves have arrived at tile rt (see the top of the loop)
                    const uint32_t want = 4u * (rt - rt0);
                    while (*arrive < want) __builtin_amdgcn_s_sleep(1);
                }
                asm volatile("" ::: "memory");
                // a publish point: every entry stored so far must have reached memory before the counts that cover it
                if (sh_point) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
#if defined(PN_DIAG_BF_COUNT)
            BF_COUNT(6, bf_stamp() - tb0_);
#endif
            if (SH) {
                if (g_pending) {  // the shared words requested a tile ago (older than everything still in flight)
                    tau0 = fminf(tau0, s2f(g0));
                    tau1 = fminf(tau1, s2f(g1));
                    g_pending = false;
                }
            }
            if (rt + 2 < rt1) {
                dma_tile(rt + 2, prv);
                ns = 0;
            }
            if (SH) {
                if (sh_point) {  // publish the fill counts (what they cover has landed: vmcnt(0) above), re-read the shared words
                    if (h == 0) {
                        sh_store(pc_blk0 + jq, sh_tag(sh.epoch, sh_ncomp) | cnt0);
                        sh_store(pc_blk1 + jq, sh_tag(sh.epoch, sh_ncomp) | cnt1);
                    }
                    g0 = sh_load(gw0);
                    g1 = sh_load(gw1);
                    g_pending = true;
                    ns += 4;
                }
            }
            const bool last = rt + 1 >= rt1;  // (then the requests below are never used: any valid LDS address)
            const char *ntb = last ? tb : tiles + nxt * TB;
#if defined(PN_DIAG_BF_COUNT)
            unsigned long long tc2_ = bf_stamp_nw();
#endif
            bf_chain_p<KS, CI, CP>(arow1, pre, b0, b1, cc, a10, a11, a00, a01, p0, p1, ntb + (jq * CP + h) * 16, ntb, 0, h);
#if defined(PN_DIAG_BF_COUNT)
            {
                unsigned long long tc3_ = bf_stamp_nw();
                bf_settle(tc3_);
                bf_settle(tc2_);
                BF_COUNT(10, tc3_ - tc2_);
            }
#endif
            if (__any(p0 < tau0 || p1 < tau1)) {
                const uint32_t row0 = rt * kBP;
                if (__any(p0 < tau0)) bf_slow<M, RAD, SH>(a00, p0, tau0, cnt0, row0, h, jq, lane, kp, ceq0, ce_blk0, ns BF_DBG_PASS, pc_blk0, &sh_ncomp, sh.epoch);
                if (__any(p1 < tau1)) bf_slow<M, RAD, SH>(a01, p1, tau1, cnt1, row0, h, jq, lane, kp, ceq1, ce_blk1, ns BF_DBG_PASS, pc_blk1, &sh_ncomp, sh.epoch);
            }
            cur = nxt;
        }
        if (SH) {
            if (g_pending) {
                tau0 = fminf(tau0, s2f(g0));
                tau1 = fminf(tau1, s2f(g1));
            }
        }
        {  // drain: block 1 of the last tile
            float m0 = a10[0], m1 = a11[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) {
                m0 = fminf(m0, a10[i]);
                m1 = fminf(m1, a11[i]);
            }
            const uint32_t row0 = (rt1 - 1) * kBP + 32;
            if (__any(m0 < tau0)) bf_slow<M, RAD, SH>(a10, m0, tau0, cnt0, row0, h, jq, lane, kp, ceq0, ce_blk0, ns BF_DBG_PASS, pc_blk0, &sh_ncomp, sh.epoch);
            if (__any(m1 < tau1)) bf_slow<M, RAD, SH>(a11, m1, tau1, cnt1, row0, h, jq, lane, kp, ceq1, ce_blk1, ns BF_DBG_PASS, pc_blk1, &sh_ncomp, sh.epoch);
            if (SH) {  // the run is over: its buffers are cut below and read "empty" to the refreshers from now on
                if (h == 0) {
                    sh_store(pc_blk0 + jq, sh_tag(sh.epoch, sh_ncomp + 1u));
                    sh_store(pc_blk1 + jq, sh_tag(sh.epoch, sh_ncomp + 1u));
                }
            }
        }
        // ---- end of run: at most kp candidates per query stay; publish count and threshold
        {
#if defined(PN_DIAG_BF_COUNT)
            const unsigned long long te0_ = bf_stamp();
#endif
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            // A buffer is cut to its k' smallest bounds here only when it holds more than kfin entries.  Handing a
            // buffer over as it is is always valid (the proof only gets a looser threshold); what it costs is re-rank
            // LDS, which is sized for what a cell can hold.  Measured (round 3, one device, a 125 k-row shard of C2 /
            // C2): every buffer cut to k' = 13: kernel 0.530 / 2.34 ms, step 0.644 / 2.48; none cut
            // (cells of up to 64 entries): kernel 0.467 / 2.34, step 0.659 / 2.50 --
            // the serial tail of up to 128 compactions per wave (16 % of a shard's run) is gone but the re-rank's waves
            // per CU halve with 9 KB of LDS each.  So the host names the count up to which a buffer stays uncut
            // (bf16_cell_max: 32 of 64 slots while the re-rank's LDS stays near 5 KB; a buffer holds 18 entries on
            // average at the end of a run): DESIGN.md 4.0.
            const uint32_t kfin = keep_arg > kp ? keep_arg : kp;
            // 64-slot buffers four at a time: their entries are requested together, then selected one after the other
            // (a buffer at a time pays a memory round trip per buffer: up to 128 in a row at the end of every run;
            // larger buffers stay one at a time -- four of them in registers made the kernel spill)
            constexpr int NB = M == 1 ? 4 : 1;
            auto final_compact = [&](uint2 *ce_blk, float &tau, uint32_t &cnt) {
                unsigned long long need = RAD ? 0ull : __ballot(h == 0 && cnt > kfin);
                while (need) {
                    int jj[NB];
                    uint32_t cj[NB], key[NB][M], ixs[NB][M];
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        jj[b] = need ? __builtin_ctzll(need) : -1;
                        if (need) need &= need - 1;
                        cj[b] = jj[b] >= 0 ? (uint32_t)__builtin_amdgcn_readlane((int)cnt, jj[b] >= 0 ? jj[b] : 0) : 0u;
                        if (jj[b] >= 0) bf_compact_load<M>(ce_blk + (size_t)jj[b] * CAP, cj[b], lane, key[b], ixs[b]);
                    }
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        if (jj[b] >= 0) {
                            uint32_t T, nn;
                            bf_compact_finish<M>(ce_blk + (size_t)jj[b] * CAP, key[b], ixs[b], cj[b], kp, lane, T, nn);
                            if (jq == jj[b]) { tau = fminf(tau, s2f(T)); cnt = nn; }
                        }
                    }
                }
            };
            final_compact(ce_blk0, tau0, cnt0);
            final_compact(ce_blk1, tau1, cnt1);
            if (h == 0) {
                ccnt[cell0 + jq] = cnt0;
                ctau[cell0 + jq] = f2s(tau0);
                ccnt[cell0 + 32 + jq] = cnt1;
                ctau[cell0 + 32 + jq] = f2s(tau1);
            }
#if defined(PN_DIAG_BF_COUNT)
            {
                const unsigned long long te1_ = bf_stamp();
                BF_COUNT(5, te1_ - te0_);
                BF_COUNT(7, te1_ - trun0_);
                {
                    unsigned long long treal1_;
                    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(treal1_)::"memory");
                    BF_COUNT(11, treal1_ - treal0_);  // 100 MHz ticks: in-kernel clock = slot 7 / slot 11 x 100 MHz
                }
            }
            BF_DBG_FLUSH(lane);
#endif
        }
        u0 = run_end;
    }
    if (SH) {  // this main workgroup is done: the refreshers leave once all are
        __syncthreads();
        if (tid == 0) (void)__hip_atomic_fetch_add(sh.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------------------
// bf16_filter8_kernel (round 4) -- the main pass of a k-NN call with FOUR waves per SIMD.
//
// bf16_filter_kernel keeps 64 queries per wave (two 32-query MFMA column blocks, 16 KS B-fragment registers + four
// accumulator tuples): 203-215 VGPRs, two waves per SIMD, and the two are both outside their MFMA chains 29 % of the
// time (rare-path entries, the tile barrier, LDS-DMA issue) -- the matrix pipe idles although work is
// queued.  Here a wave owns ONE column block (32 queries; lanes j and j + 32 hold the same query and different rows,
// as before): 8 KS B-fragment registers, two accumulator tuples, <= 128 VGPRs, so a workgroup is EIGHT waves over the
// same 256 queries and the same tile stream, two workgroups per CU = four waves per SIMD.  Nothing else changes: the
// tile images, the (segment, query) candidate buffers, thresholds in registers, shared thresholds, seeds from the scout
// launch, the software pipeline over three tile buffers (one chain per 32-row block: KS MFMAs), the end of a run.  The
// price is LDS bandwidth -- every A fragment read feeds one MFMA instead of two: 1.5 ds_read_b128 per MFMA and SIMD
// with the row norms, 75 % of what the LDS delivers (MI355X_MICROARCH.md, LDS: two per MFMA gap still fit).
// Main pass only (thresholds given: MODE 2 of bf16_filter_kernel), 64- and 128-slot buffers, k-NN; the scout launch,
// radius queries and 256-slot buffers keep the 4-wave kernel.
// ---------------------------------------------------------------------------
// One chain of the 8-wave kernel: KS MFMAs of one 32-row block against the wave's query block while the VALU takes the
// minimum of the other block's bounds (r).  This variant starts from registers -- its first fragments `pre` and its
// accumulator init `c` were requested during the PREVIOUS chain, as in bf_chain_p.
template <int KS, bool CI, int CP, int LA>
__device__ __forceinline__ void bf_chain1(const char *arow, bf16x8 (&pre)[LA], const bf16x8 (&b)[KS], f32x16 &c,
                                          f32x16 &w, f32x16 &r, float &m, const char *narow, const char *ntb, int nblk,
                                          int h) {
    typedef float f32x4_ __attribute__((ext_vector_type(4)));
    bf16x8 f[KS];
#pragma unroll
    for (int i = 0; i < LA && i < KS; ++i) f[i] = pre[i];
    f32x16 z, nc = c;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (ks + LA < KS) f[ks + LA] = *reinterpret_cast<const bf16x8 *>(arow + 32 * (ks + LA));
        // the next chain's first fragments: fragment i at step max(0, KS - LA + i)
#pragma unroll
        for (int i = 0; i < LA; ++i)
            if (ks == (KS - LA + i > 0 ? KS - LA + i : 0))
                pre[i] = *reinterpret_cast<const bf16x8 *>(narow + 32 * (i < KS ? i : 0));
        if (CI) {  // ... and its accumulator init: piece g at step max(0, KS - 4 + g)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (ks == (KS - 4 + g > 0 ? KS - 4 + g : 0)) {
                    const f32x4_ v =
                        *reinterpret_cast<const f32x4_ *>(ntb + ((nblk * 8 + 2 * g + h) * CP + (CP - 1)) * 16);
                    nc[4 * g + 0] = v[0];
                    nc[4 * g + 1] = v[1];
                    nc[4 * g + 2] = v[2];
                    nc[4 * g + 3] = v[3];
                }
            w = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[ks], b[ks], ks ? w : c, 0, 0, 0);
        } else {
            w = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[ks], b[ks], ks ? w : z, 0, 0, 0);
        }
#pragma unroll
        for (int i = 16 * ks / KS; i < 16 * (ks + 1) / KS; ++i)  // this step's share of the other block's minimum
            m = i ? fminf(m, r[i]) : r[0];
        __builtin_amdgcn_sched_barrier(0);  // a step stays a step (see bf_chain)
    }
    c = nc;
}

// The same chain starting COLD: its first fragments and its accumulator init are requested at its head.  With four
// waves per SIMD the other waves' chains cover that LDS round trip, and nothing of the NEXT chain is held across the
// survivor check and the barrier: 24 registers less than bf_chain1 (kBf8Prefetch picks the variant; measured A/B).
template <int KS, bool CI, int CP, int LA>
__device__ __forceinline__ void bf_chain1c(const char *arow, const char *tb, int blk, int h, const bf16x8 (&b)[KS], f32x16 &w,
                                           f32x16 &r, float &m) {
    bf16x8 f[KS];
#pragma unroll
    for (int i = 0; i < LA && i < KS; ++i) f[i] = *reinterpret_cast<const bf16x8 *>(arow + 32 * i);
    f32x16 c;
    if (CI) c = bf_cinit<CP>(tb, blk, h);
    else {
#pragma unroll
        for (int i = 0; i < 16; ++i) c[i] = 0.0f;
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (ks + LA < KS) f[ks + LA] = *reinterpret_cast<const bf16x8 *>(arow + 32 * (ks + LA));
        w = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[ks], b[ks], ks ? w : c, 0, 0, 0);
#pragma unroll
        for (int i = 16 * ks / KS; i < 16 * (ks + 1) / KS; ++i)  // this step's share of the other block's minimum
            m = i ? fminf(m, r[i]) : r[0];
        __builtin_amdgcn_sched_barrier(0);  // a step stays a step (see bf_chain)
    }
}

constexpr bool kBf8Prefetch = false;  // bf_chain1 (true) or bf_chain1c (false)
template <int KS, bool CI, bool SH, int M = 1>
__global__ __launch_bounds__(512, 4) void bf16_filter8_kernel(const char *__restrict__ img, uint32_t n_tiles,
                                                              const u32x4 *__restrict__ Bq, uint32_t q_tiles,
                                                              uint32_t kp_keep, uint2 *__restrict__ cand,
                                                              uint32_t *__restrict__ ccnt, uint32_t *__restrict__ ctau,
                                                              size_t nq_pad, const uint32_t *tau_init, BfShared sh) {
    const uint32_t kp = kp_keep & 0xFFFFu, keep_arg = kp_keep >> 16;
    constexpr int C = 2 * KS, CP = C + 1;
    constexpr uint32_t CAP = 64u * M;
    constexpr int TB = kBP * CP * 16;  // bytes per tile image
    constexpr int NBUF = 3, NW = 8;
    constexpr int LA = 3;  // fragment lookahead (the 4-wave kernel: kLA = 3)
    constexpr bool PREF = kBf8Prefetch;  // chains start from registers requested during the previous chain
    constexpr bool kSplit8 = false;  // arrive at the top of a tile, wait for the count in mid-tile (bf16_filter_kernel, kSplit)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    char *tiles = reinterpret_cast<char *>(smem_raw);  // [NBUF][TB]
    volatile uint32_t *arrive = reinterpret_cast<volatile uint32_t *>(tiles + NBUF * TB);  // split barrier's arrival counter
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int jq = lane & 31, h = lane >> 5;
    BF_DBG_DECL;
    if (SH && blockIdx.x >= sh.n_main) {  // a refresher workgroup: eight waves over the queries, until the mains are done
        const uint32_t n_wv = (gridDim.x - sh.n_main) * (uint32_t)NW, wv = (blockIdx.x - sh.n_main) * (uint32_t)NW + (uint32_t)wave;
        bf_refresher<M>(cand, sh.pcnt, const_cast<uint32_t *>(tau_init), sh.done, sh.n_main, nq_pad, sh.nseg, sh.epoch,
                        sh.rank, wv, n_wv, lane);
        return;
    }
    // Aligned partition only (the host guarantees it): W = c q_tiles workgroups, workgroup w = run p of query tile q in
    // the range-major, XCD-contiguous order of bf16_filter_kernel (blocks of one XCD walk the same row range)
    const uint32_t W = SH ? sh.n_main : gridDim.x;
    uint32_t w = blockIdx.x;
    const uint32_t c_per = W / q_tiles;
    {
        const uint32_t b = blockIdx.x, x = b & 7u, base = W >> 3, rem = W & 7u;
        const uint32_t L = x * base + (x < rem ? x : rem) + (b >> 3);  // XCDs 0 .. rem-1 run base + 1 blocks
        w = (L % q_tiles) * c_per + L / q_tiles;
    }
    const uint32_t qt = w / c_per, seg = w % c_per;
    const uint32_t rt0 = (uint32_t)((unsigned long long)seg * n_tiles / c_per);
    const uint32_t rt1 = (uint32_t)((unsigned long long)(seg + 1) * n_tiles / c_per);
    const size_t q0 = (size_t)qt * kBQ + (size_t)wave * 32;   // first query of this wave
    const size_t cell0 = (size_t)seg * nq_pad + q0;           // its (segment, query) cell

    // wave w moves the consecutive pieces [w P, w P + P) of a tile
    constexpr int P = (CP + NW - 1) / NW;
    static_assert(P <= 3, "piece schedule written out for up to three pieces per wave");
    const int n_mine = CP - wave * P < P ? (CP - wave * P > 0 ? CP - wave * P : 0) : P;
    // (addresses as a wave-uniform base + a 32-bit lane offset, recomputed per tile: 64-bit per-lane pointers kept across
    // the loop were what the register allocator spilled -- and reloaded behind a vmcnt(0) on every tile)
    const uint32_t lane_off = (uint32_t)lane * 16u;
    auto dma_tile = [&](uint32_t rt, int buf) {
        const char *wbase = img + ((size_t)rt * (size_t)TB + (size_t)(wave * (P * 1024)));  // wave-uniform
        const char *ws = wbase + lane_off;
        char *wd = tiles + buf * TB + wave * (P * 1024);
        if (0 < n_mine) __builtin_amdgcn_global_load_lds((glb_void_b *)ws, (lds_void_b *)wd, 16, 0, 0);
        if (P > 1 && 1 < n_mine) __builtin_amdgcn_global_load_lds((glb_void_b *)ws, (lds_void_b *)wd, 16, 1024, 0);
        if (P > 2 && 2 < n_mine) __builtin_amdgcn_global_load_lds((glb_void_b *)ws, (lds_void_b *)wd, 16, 2048, 0);
    };

    if (rt0 < rt1) {
        // ---- per-run state: B fragments, threshold and count in registers
        bf16x8 b[KS];
        {
            const u32x4 *br = Bq + (q0 + jq) * (size_t)C + h;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b[ks] = __builtin_bit_cast(bf16x8, br[2 * ks]);
        }
        float tau;
        uint32_t cnt = 0;
        if (sh.seed_lists) {
            // every lane derives its own query's threshold from the scout launch's lists (both halves the same one); a
            // padding query of the last tile gets -inf: nothing passes, it costs no appends
            const size_t ql = q0 + (size_t)jq;
            tau = __uint_as_float(0xFF800000u);
            if (ql < (size_t)sh.seed_nq) {
                const uint32_t key = f2s(bf_seed_lane(sh.seed_lists, nq_pad, sh.nseg, sh.seed_rank, ql));
                tau = s2f(key == 0xFFFFFFFFu ? key : key + 1u);  // rows with a bound EQUAL to it still pass the strict '<'
            }
        } else {
            tau = s2f(SH ? sh_load(tau_init + q0 + jq) : tau_init[q0 + jq]);
        }
        uint2 *ce_blk = cand + cell0 * CAP;           // this wave's 32 buffers
        uint2 *ceq = ce_blk + (size_t)jq * CAP;
        uint32_t ns = 0;
        // software pipeline over the tiles of the run, three LDS buffers: see bf16_filter_kernel
        dma_tile(rt0, 0);
        if (rt0 + 1 < rt1) dma_tile(rt0 + 1, 1);
        if (tid == 0) *arrive = 0u;
        __syncthreads();  // carries the vmcnt(0): the first NBUF - 1 tiles are in LDS
        f32x16 a0, a1;
#pragma unroll
        for (int r = 0; r < 16; ++r) {  // "nothing here yet": above every threshold
            a0[r] = 3.0e38f;
            a1[r] = 3.0e38f;
        }
        bf16x8 pre[LA];
        f32x16 cc = a0;  // (placeholder unless CI)
        if (PREF) {
            const char *ar = tiles + (jq * CP + h) * 16;
#pragma unroll
            for (int i = 0; i < LA; ++i) pre[i] = *reinterpret_cast<const bf16x8 *>(ar + 32 * (i < KS ? i : 0));
            if (CI) cc = bf_cinit<CP>(tiles, 0, h);
        }
        int cur = 0;
        uint32_t *pc_blk = SH ? sh.pcnt + cell0 : nullptr;
        const uint32_t *gw = tau_init + q0 + jq;
        uint32_t g0 = 0, sh_ncomp = 0;
        bool g_pending = false;  // (wave-uniform)
        for (uint32_t rt = rt0; rt < rt1; ++rt) {
            const int nxt = cur == NBUF - 1 ? 0 : cur + 1, prv = cur == 0 ? NBUF - 1 : cur - 1;
            const bool sh_point = SH && ((rt - rt0) % kShPeriod) == kShPeriod - 1;  // (wave-uniform)
            const char *tb = tiles + cur * TB;
            const char *arow0 = tb + (jq * CP + h) * 16;
            const char *arow1 = arow0 + 32 * CP * 16;
            float m, p;
            if (kSplit8 && rt > rt0) {
                bf_wait_dma(ns);
                if (lane == 0) __hip_atomic_fetch_add(const_cast<uint32_t *>(arrive), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            if (PREF) bf_chain1<KS, CI, CP, LA>(arow0, pre, b, cc, a0, a1, m, arow1, tb, 1, h);
            else bf_chain1c<KS, CI, CP, LA>(arow0, tb, 0, h, b, a0, a1, m);
            if (rt == rt0) m = __uint_as_float(0x7F800000u);  // nothing precedes the first tile
            if (__any(m < tau))
                bf_slow<M, false, SH>(a1, m, tau, cnt, (rt - 1) * kBP + 32, h, jq, lane, kp, ceq, ce_blk, ns BF_DBG_PASS,
                                      pc_blk, &sh_ncomp, sh.epoch);
            // mid-tile barrier: every wave's pieces of tile rt + 1 have landed, nobody reads tile rt - 1 any more
            if (!kSplit8) {
                if (sh_point) ns = 0;  // a publish point: every entry stored so far must have reached memory (vmcnt(0))
                bf_wait_dma(ns);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            } else {
                if (rt > rt0) {  // all eight waves have arrived at tile rt (see the top of the loop)
                    const uint32_t want = (uint32_t)NW * (rt - rt0);
                    while (*arrive < want) __builtin_amdgcn_s_sleep(1);
                }
                asm volatile("" ::: "memory");
                if (sh_point) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            if (SH) {
                if (g_pending) {  // the shared word requested a tile ago
                    tau = fminf(tau, s2f(g0));
                    g_pending = false;
                }
            }
            if (rt + 2 < rt1) {
                dma_tile(rt + 2, prv);
                ns = 0;
            }
            if (SH) {
                if (sh_point) {  // publish the fill count (what it covers has landed), re-read the shared word
                    if (h == 0) sh_store(pc_blk + jq, sh_tag(sh.epoch, sh_ncomp) | cnt);
                    g0 = sh_load(gw);
                    g_pending = true;
                    ns += 2;
                }
            }
            const bool last = rt + 1 >= rt1;  // (then the requests below are never used: any valid LDS address)
            const char *ntb = last ? tb : tiles + nxt * TB;
            if (PREF) bf_chain1<KS, CI, CP, LA>(arow1, pre, b, cc, a1, a0, p, ntb + (jq * CP + h) * 16, ntb, 0, h);
            else bf_chain1c<KS, CI, CP, LA>(arow1, tb, 1, h, b, a1, a0, p);
            if (__any(p < tau))
                bf_slow<M, false, SH>(a0, p, tau, cnt, rt * kBP, h, jq, lane, kp, ceq, ce_blk, ns BF_DBG_PASS, pc_blk,
                                      &sh_ncomp, sh.epoch);
            cur = nxt;
        }
        if (SH) {
            if (g_pending) tau = fminf(tau, s2f(g0));
        }
        {  // drain: block 1 of the last tile
            float m = a1[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) m = fminf(m, a1[i]);
            if (__any(m < tau))
                bf_slow<M, false, SH>(a1, m, tau, cnt, (rt1 - 1) * kBP + 32, h, jq, lane, kp, ceq, ce_blk, ns BF_DBG_PASS,
                                      pc_blk, &sh_ncomp, sh.epoch);
            if (SH) {  // the run is over: its buffers may be cut below and read "empty" to the refreshers from now on
                if (h == 0) sh_store(pc_blk + jq, sh_tag(sh.epoch, sh_ncomp + 1u));
            }
        }
        // ---- end of run: a buffer holding more than kfin entries is cut to its k' smallest; publish count and threshold
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t kfin = keep_arg > kp ? keep_arg : kp;
        unsigned long long need = __ballot(h == 0 && cnt > kfin);
        constexpr int NB = M == 1 ? 4 : 1;  // (larger buffers one at a time: four of them in registers spill)
        while (need) {
            int jj[NB];
            uint32_t cj[NB], key[NB][M], ixs[NB][M];
#pragma unroll
            for (int bb = 0; bb < NB; ++bb) {
                jj[bb] = need ? __builtin_ctzll(need) : -1;
                if (need) need &= need - 1;
                cj[bb] = jj[bb] >= 0 ? (uint32_t)__builtin_amdgcn_readlane((int)cnt, jj[bb] >= 0 ? jj[bb] : 0) : 0u;
                if (jj[bb] >= 0) bf_compact_load<M>(ce_blk + (size_t)jj[bb] * CAP, cj[bb], lane, key[bb], ixs[bb]);
            }
#pragma unroll
            for (int bb = 0; bb < NB; ++bb) {
                if (jj[bb] >= 0) {
                    uint32_t T, nn;
                    bf_compact_finish<M>(ce_blk + (size_t)jj[bb] * CAP, key[bb], ixs[bb], cj[bb], kp, lane, T, nn);
                    if (jq == jj[bb]) { tau = fminf(tau, s2f(T)); cnt = nn; }
                }
            }
        }
        if (h == 0) {
            ccnt[cell0 + jq] = cnt;
            ctau[cell0 + jq] = f2s(tau);
        }
        BF_DBG_FLUSH(lane);
    }
    if (SH) {  // this main workgroup is done: the refreshers leave once all are
        __syncthreads();
        if (tid == 0) (void)__hip_atomic_fetch_add(sh.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------------------
// bf16_filter_kernel_pair (round 5) -- the main pass of a k-NN call with ONE 8-wave workgroup per CU whose SIMD
// partners run in ANTI-PHASE.
//
// In bf16_filter_kernel the two waves of a SIMD belong to two independent workgroups, and what each does outside its
// MFMA chains (survivor check, tile barrier, LDS-DMA issue) falls wherever chance puts it against the other's: both
// are outside their chains 29 % of the time and the matrix pipe idles.  Here the partners are the two
// halves of one workgroup -- waves 0-3 serve query tile 2t, waves 4-7 query tile 2t + 1, over the SAME row range, tile
// stream and three LDS tile buffers -- so that the one s_barrier per tile ties their phases together.  A wave is
// exactly the 4-wave kernel's wave (two 32-query column blocks, B fragments in 8 KS registers, bf_chain_p, bf_slow,
// the end-of-run cut, one writer per (segment, query) cell); the 2 KS + 1 pieces of a tile are spread over the eight
// waves as in bf16_filter8_kernel.
//
// Schedule of tile rt (chain A: row block 0, chain B: row block 1; "survivors" is the rare-path check):
//   waves 0-3 (LEAD):  chain A | survivors | DMA wait + s_barrier | DMA issue rt+2 | chain B | survivors
//   waves 4-7 (LAG):   chain A, first KS/2 steps | DMA wait + s_barrier | rest of chain A | survivors | DMA issue rt+2
//                      | chain B | survivors
// Both do the same work between two barriers, the lagging half displaced by half a chain: its gaps (survivors and DMA
// issue after chain A, survivors after chain B) fall into the leading half's chains and the other way round.
//
// What the barrier B(rt) certifies is what it certifies in the 4-wave kernel, and three buffers still suffice:
//  * tile rt+1 has landed: every wave's pieces of it were issued behind B(rt-1) and are waited for (the counted
//    vmcnt of bf_wait_dma) before the wave arrives at B(rt); its first readers are the last steps of chain B of tile
//    rt (the requests for the next chain), behind B(rt) in both roles;
//  * nobody reads tile rt-1 any more, so its buffer can take tile rt+2 (issued behind B(rt) in both roles): the last
//    reads of tile rt-1 are the fragment requests of chain B of tile rt-1.  The leading half has finished chain A of
//    tile rt since and waits lgkmcnt(0).  The lagging half finished that chain half a chain before it arrives; it
//    does not wait for its LDS reads in flight (fragments of tile rt, kLA steps ahead), and need not: LDS reads of a
//    wave return in order, and the MFMAs of the steps before the barrier have consumed fragments requested AFTER the
//    last request into tile rt-1.
// Barrier counts are the same in both roles by construction: the prologue's __syncthreads is executed before the
// roles part, and the roles are two instantiations of ONE loop (bf_pair_run) over the same rt0 .. rt1 with exactly one
// s_barrier per iteration and none behind the loop.
//
// Main pass only (thresholds given), 64-slot buffers, aligned partition, no refreshers.  With an odd number of
// query tiles the upper half of the last pair has no queries: it moves its DMA pieces, meets every barrier and runs its
// chains against zero B fragments with thresholds of -inf -- nothing survives, it reads and writes no query data.
// STAG (diagnostic builds: -DPN_DIAG_PAIR_STAGGER=0 / 2): 0 = both halves in the leading placement, 2 = the lagging
// half displaced by a whole chain (barrier in front of chain A), where the gaps coincide again.
// ---------------------------------------------------------------------------
#ifndef PN_DIAG_PAIR_STAGGER
#define PN_DIAG_PAIR_STAGGER 1
#endif
constexpr int kPairStagger = PN_DIAG_PAIR_STAGGER;  // 1: half a chain
#ifndef PN_DIAG_PAIR_MID4
#define PN_DIAG_PAIR_MID4 2
#endif
struct BfPairMeet {  // the lagging half's tile barrier, inside chain A: after KS / 2 steps (diagnostic builds: KS MID4 / 4),
    uint32_t ns;     // at least one -- the argument above needs an MFMA of this chain in front of the barrier
    static constexpr int at(int ks) { return ks * PN_DIAG_PAIR_MID4 / 4 > 1 ? ks * PN_DIAG_PAIR_MID4 / 4 : 1; }
#ifdef PN_DIAG_BF_COUNT
    unsigned long long *st;  // two stamps that do not wait (the caller settles them behind the chain): arrival, departure
#endif
    __device__ __forceinline__ void operator()() const {
#ifdef PN_DIAG_BF_COUNT
        st[0] = bf_stamp_nw();
#endif
        bf_wait_dma(ns);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#ifdef PN_DIAG_BF_COUNT
        st[1] = bf_stamp_nw();
#endif
    }
};
#ifdef PN_DIAG_BF_COUNT
#define BF_PAIR_MEET(ns) BfPairMeet{ns, tmeet_}
#else
#define BF_PAIR_MEET(ns) BfPairMeet{ns}
#endif
#ifndef PN_DIAG_PAIR_DMA_LATE
#define PN_DIAG_PAIR_DMA_LATE 0  // diagnostic builds, 1: the second tile's pieces are issued one tile later, in that tile's gap
#endif

//
// MEET (tiles per meeting; 1: the schedule above, 2: bf16_filter_kernel_meet_pair<KS, CI, 2>).  At C2 a wave takes ~0.36
// rare-path entries per tile, so nearly every tile has one of the CU's eight waves in a detour and a meeting per tile
// is paid at the pace of the slowest of eight.  With MEET = 2 an iteration covers the two tiles of SUPER-TILE s = tiles
// (2s, 2s+1) of the run -- chain A, chain B of tile 2s, chain A, chain B of tile 2s+1 -- with ONE s_barrier, placed
// where MEET = 1 places it in the first of them (leading half: between the first tile's chains; lagging half: inside
// its chain A at BfPairMeet::at).  The ring holds 3 MEET tiles, tile t of the run in buffer t mod 6; the prologue
// brings super-tiles 0 and 1.  The argument above holds with "tile" read as "pair of tiles":
//  * B(s) certifies that super-tile s+1 has landed: every wave issued its pieces of both tiles behind B(s-1) (or in
//    the prologue) and waits for them with bf_wait_dma before it arrives.  Its first readers are the last steps of
//    chain B of tile 2s+1, behind B(s) in both roles.  `pre` and `nc` cross from tile 2s to tile 2s+1 WITHOUT a
//    barrier: both tiles landed together, certified by B(s-1);
//  * nobody reads super-tile s-1 any more, so its two buffers take super-tile s+2, issued behind B(s) in the wave's
//    own gap: the last reads of super-tile s-1 are the fragment requests of chain B of tile 2s-1.  The leading half
//    has finished chain A of tile 2s since and waits lgkmcnt(0); the lagging half has executed BfPairMeet::at >= 1
//    steps of that chain, whose MFMAs consumed fragments requested AFTER the last request into tile 2s-1, and LDS
//    reads of a wave return in order: it still needs no lgkmcnt(0) in mid-chain.
// ns and bf_wait_dma: up to four survivor checks now lie between a wave's DMA issue and its next meeting, so ns can be
// larger -- the wait's three cases stay correct for ANY ns: vector-memory operations retire in order, all ns stores
// are younger than the DMA pieces (both tiles' pieces are issued back to back and ns restarts behind the last), and
// "at most min(ns, 2) outstanding" therefore never leaves a piece in flight.
// A run of odd length ends with a half super-tile: the iteration skips the second tile's chains and requests and
// still executes its one barrier -- ceil(n / 2) barriers in both roles for every run length n, by construction (two
// instantiations of one loop).  Cells, writers, thresholds, the order of a wave's appends and the end-of-run cut do not
// depend on MEET: candidates, counters and answers are the same bits.
// -DPN_DIAG_PAIR_MEET=1 (diagnostic builds) gives the two-tile kernel's entry today's schedule from this same source.
#ifndef PN_DIAG_PAIR_MEET
#define PN_DIAG_PAIR_MEET 2
#endif
constexpr int kPairMeet = PN_DIAG_PAIR_MEET;  // tiles per meeting of the two-tile kernel (Bf16Kernel::PairTwo)
static_assert(kPairMeet == 1 || kPairMeet == 2, "PN_DIAG_PAIR_MEET");

template <int KS, bool CI, int STAG, int MEET>
__device__ __forceinline__ void bf_pair_run(const char *__restrict__ img, char *tiles, uint32_t kp, uint32_t kfin, uint2 *__restrict__ cand,
                                            uint32_t *__restrict__ ccnt, uint32_t *__restrict__ ctau,
                                            const bf16x8 (&b0)[KS], const bf16x8 (&b1)[KS], float tau0, float tau1,
                                            uint32_t rt0, uint32_t rt1, size_t cell0, bool active, int wave, int lane) {
    constexpr int C = 2 * KS, CP = C + 1;
    constexpr uint32_t CAP = 64u;
    constexpr int TB = kBP * CP * 16;  // bytes per tile image
    constexpr int NBUF = 3 * MEET, NW = 8;
    const int jq = lane & 31, h = lane >> 5;
    BF_DBG_DECL;
    // wave w moves the consecutive pieces [w P, w P + P) of a tile (bf16_filter8_kernel)
    constexpr int P = (CP + NW - 1) / NW;
    static_assert(P <= 3, "piece schedule written out for up to three pieces per wave");
    const int n_mine = CP - wave * P < P ? (CP - wave * P > 0 ? CP - wave * P : 0) : P;
    const uint32_t lane_off = (uint32_t)lane * 16u;
    auto dma_tile = [&](uint32_t rt, int buf) {
        const char *wbase = img + ((size_t)rt * (size_t)TB + (size_t)(wave * (P * 1024)));  // wave-uniform
        const char *ws = wbase + lane_off;
        char *wd = tiles + buf * TB + wave * (P * 1024);
        if (0 < n_mine) __builtin_amdgcn_global_load_lds((glb_void_b *)ws, (lds_void_b *)wd, 16, 0, 0);
        if (P > 1 && 1 < n_mine) __builtin_amdgcn_global_load_lds((glb_void_b *)ws, (lds_void_b *)wd, 16, 1024, 0);
        if (P > 2 && 2 < n_mine) __builtin_amdgcn_global_load_lds((glb_void_b *)ws, (lds_void_b *)wd, 16, 2048, 0);
    };

    uint32_t cnt0 = 0, cnt1 = 0;
    uint2 *ce_blk0 = cand + cell0 * CAP;          // query block 0: 32 buffers
    uint2 *ce_blk1 = ce_blk0 + (size_t)32 * CAP;  // query block 1
    uint2 *ceq0 = ce_blk0 + (size_t)jq * CAP, *ceq1 = ce_blk1 + (size_t)jq * CAP;
    uint32_t ns = 0;

    f32x16 a00, a01, a10, a11;
#pragma unroll
    for (int r = 0; r < 16; ++r) {  // "nothing here yet": above every threshold
        a00[r] = 3.0e38f;
        a01[r] = 3.0e38f;
        a10[r] = 3.0e38f;
        a11[r] = 3.0e38f;
    }
    bf16x8 pre[kLA];
    f32x16 cc = a00;  // (placeholder unless CI)
    {
        const char *ar = tiles + (jq * CP + h) * 16;
#pragma unroll
        for (int i = 0; i < kLA; ++i) pre[i] = *reinterpret_cast<const bf16x8 *>(ar + 32 * (i < KS ? i : 0));
        if (CI) cc = bf_cinit<CP>(tiles, 0, h);
    }
    int cur = 0;  // the buffer of the tile at hand: tile t of the run sits in buffer t mod NBUF
    auto ring = [](int b) { return b >= NBUF ? b - NBUF : b; };
    constexpr bool LATE = MEET == 2 && PN_DIAG_PAIR_DMA_LATE != 0;
#ifdef PN_DIAG_BF_COUNT
    const unsigned long long trun0_ = bf_stamp();
    unsigned long long tmeet_[2] = {0, 0};
#endif
    // One tile.  meets: the first tile of an iteration -- the workgroup's meeting and the wave's DMA issue lie in it.
    auto tile = [&](uint32_t rt, auto meets) {
        constexpr bool MT = decltype(meets)::value;
        const int nxt = ring(cur + 1);
        const char *tb = tiles + cur * TB;
        const char *arow0 = tb + (jq * CP + h) * 16;
        const char *arow1 = arow0 + 32 * CP * 16;
        float m0, m1, p0, p1;
#ifdef PN_DIAG_BF_COUNT
        unsigned long long tc0_ = bf_stamp_nw();
#endif
        if (MT && STAG == 2) BF_PAIR_MEET(ns)();
        if (MT && STAG == 1)
            bf_chain_p<KS, CI, CP>(arow0, pre, b0, b1, cc, a00, a01, a10, a11, m0, m1, arow1, tb, 1, h, BF_PAIR_MEET(ns));
        else
            bf_chain_p<KS, CI, CP>(arow0, pre, b0, b1, cc, a00, a01, a10, a11, m0, m1, arow1, tb, 1, h);
#ifdef PN_DIAG_BF_COUNT
        {  // chain A, without the meeting inside it (lagging half); the meeting itself
            unsigned long long tc1_ = bf_stamp_nw();
            bf_settle(tc1_);
            bf_settle(tc0_);
            bf_settle(tmeet_[0]);
            bf_settle(tmeet_[1]);
            BF_COUNT(9, tc1_ - tc0_ - (tmeet_[1] - tmeet_[0]));
            BF_COUNT(6, tmeet_[1] - tmeet_[0]);
            tmeet_[0] = tmeet_[1] = 0;
        }
#endif
        if (MT && rt == rt0) { m0 = __uint_as_float(0x7F800000u); m1 = m0; }  // nothing precedes the first tile
        if (__any(m0 < tau0 || m1 < tau1)) {
            const uint32_t row0 = (rt - 1) * kBP + 32;
            if (__any(m0 < tau0)) bf_slow<1, false>(a10, m0, tau0, cnt0, row0, h, jq, lane, kp, ceq0, ce_blk0, ns BF_DBG_PASS);
            if (__any(m1 < tau1)) bf_slow<1, false>(a11, m1, tau1, cnt1, row0, h, jq, lane, kp, ceq1, ce_blk1, ns BF_DBG_PASS);
        }
        if (MT && STAG == 0) {  // the leading placement: between the tile's two chains
#ifdef PN_DIAG_BF_COUNT
            const unsigned long long tb0_ = bf_stamp();
#endif
            bf_wait_dma(ns);
#ifndef PN_DIAG_PAIR_NOLGKM
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
#ifdef PN_DIAG_BF_COUNT
            BF_COUNT(6, bf_stamp() - tb0_);
#endif
        }
        // the wave's pieces of the super-tile after next, into the buffers of the one before this: behind the meeting,
        // in the wave's own gap (MEET = 1: tile rt + 2 into the buffer of tile rt - 1)
        if (MT) {
#pragma unroll
            for (int j = 0; j < (LATE ? 1 : MEET); ++j)
                if (rt + 2 * MEET + j < rt1) {
                    dma_tile(rt + 2 * MEET + j, ring(cur + 2 * MEET + j));
                    ns = 0;
                }
        } else if (LATE && rt + 2 * MEET < rt1) {  // (this tile is the iteration's second: its number is one higher)
            dma_tile(rt + 2 * MEET, ring(cur + 2 * MEET));
            ns = 0;
        }
        const bool last = rt + 1 >= rt1;  // (then the requests below are never used: any valid LDS address)
        const char *ntb = last ? tb : tiles + nxt * TB;
#ifdef PN_DIAG_BF_COUNT
        unsigned long long tc2_ = bf_stamp_nw();
#endif
        bf_chain_p<KS, CI, CP>(arow1, pre, b0, b1, cc, a10, a11, a00, a01, p0, p1, ntb + (jq * CP + h) * 16, ntb, 0, h);
#ifdef PN_DIAG_BF_COUNT
        {
            unsigned long long tc3_ = bf_stamp_nw();
            bf_settle(tc3_);
            bf_settle(tc2_);
            BF_COUNT(10, tc3_ - tc2_);
        }
#endif
        if (__any(p0 < tau0 || p1 < tau1)) {
            const uint32_t row0 = rt * kBP;
            if (__any(p0 < tau0)) bf_slow<1, false>(a00, p0, tau0, cnt0, row0, h, jq, lane, kp, ceq0, ce_blk0, ns BF_DBG_PASS);
            if (__any(p1 < tau1)) bf_slow<1, false>(a01, p1, tau1, cnt1, row0, h, jq, lane, kp, ceq1, ce_blk1, ns BF_DBG_PASS);
        }
        cur = nxt;
    };
    for (uint32_t rt = rt0; rt < rt1; rt += MEET) {  // ONE s_barrier per iteration, whatever STAG and MEET
        tile(rt, std::true_type{});
        if (MEET == 2 && rt + 1 < rt1) tile(rt + 1, std::false_type{});  // (a run of odd length ends with half a super-tile)
    }
    {  // drain: block 1 of the last tile
        float m0 = a10[0], m1 = a11[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) {
            m0 = fminf(m0, a10[i]);
            m1 = fminf(m1, a11[i]);
        }
        const uint32_t row0 = (rt1 - 1) * kBP + 32;
        if (__any(m0 < tau0)) bf_slow<1, false>(a10, m0, tau0, cnt0, row0, h, jq, lane, kp, ceq0, ce_blk0, ns BF_DBG_PASS);
        if (__any(m1 < tau1)) bf_slow<1, false>(a11, m1, tau1, cnt1, row0, h, jq, lane, kp, ceq1, ce_blk1, ns BF_DBG_PASS);
    }
    // ---- end of run (no barrier from here on): a buffer holding more than kfin entries is cut to its k' smallest, four
    // buffers' entries requested together (bf16_filter_kernel); publish count and threshold
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    auto final_compact = [&](uint2 *ce_blk, float &tau, uint32_t &cnt) {
        constexpr int NB = 4;
        unsigned long long need = __ballot(h == 0 && cnt > kfin);
        while (need) {
            int jj[NB];
            uint32_t cj[NB], key[NB][1], ixs[NB][1];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                jj[b] = need ? __builtin_ctzll(need) : -1;
                if (need) need &= need - 1;
                cj[b] = jj[b] >= 0 ? (uint32_t)__builtin_amdgcn_readlane((int)cnt, jj[b] >= 0 ? jj[b] : 0) : 0u;
                if (jj[b] >= 0) bf_compact_load<1>(ce_blk + (size_t)jj[b] * CAP, cj[b], lane, key[b], ixs[b]);
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (jj[b] >= 0) {
                    uint32_t T, nn;
                    bf_compact_finish<1>(ce_blk + (size_t)jj[b] * CAP, key[b], ixs[b], cj[b], kp, lane, T, nn);
                    if (jq == jj[b]) { tau = fminf(tau, s2f(T)); cnt = nn; }
                }
            }
        }
    };
    final_compact(ce_blk0, tau0, cnt0);
    final_compact(ce_blk1, tau1, cnt1);
    if (active && h == 0) {
        ccnt[cell0 + jq] = cnt0;
        ctau[cell0 + jq] = f2s(tau0);
        ccnt[cell0 + 32 + jq] = cnt1;
        ctau[cell0 + 32 + jq] = f2s(tau1);
    }
#ifdef PN_DIAG_BF_COUNT
    BF_COUNT(7, bf_stamp() - trun0_);
    if (lane == 0)  // per role: the leading half's sums in g_bfdbg, the lagging half's in g_bfdbg_lag
        for (int i = 0; i < 12; ++i) atomicAdd(STAG ? &g_bfdbg_lag[i] : &g_bfdbg[i], dbg_[i]);
#endif
}

// The body of both paired kernels (tiles: the ring of 3 MEET tile buffers in dynamic LDS)
template <int KS, bool CI, int MEET>
__device__ __forceinline__ void bf_pair_body(char *tiles, const char *__restrict__ img, uint32_t n_tiles,
                                             const u32x4 *__restrict__ Bq, uint32_t q_tiles, uint32_t kp_keep,
                                             uint2 *__restrict__ cand, uint32_t *__restrict__ ccnt,
                                             uint32_t *__restrict__ ctau, size_t nq_pad, const uint32_t *tau_init,
                                             const BfShared &sh) {
    const uint32_t kp = kp_keep & 0xFFFFu, keep_arg = kp_keep >> 16;
    const uint32_t kfin = keep_arg > kp ? keep_arg : kp;
    constexpr int CP = 2 * KS + 1;
    constexpr int TB = kBP * CP * 16;  // bytes per tile image
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int jq = lane & 31, h = lane >> 5;
    constexpr int C = 2 * KS;
    // Aligned partition (the host guarantees it), counted in PAIRS of query tiles: W = c n_pairs workgroups, workgroup
    // w = row range p of pair t in the range-major, XCD-contiguous order of bf16_filter_kernel (the blocks of one XCD
    // walk the same row range).  The c row ranges are the 4-wave kernel's: every (segment, query) cell keeps its writer.
    const uint32_t W = gridDim.x, n_pairs = (q_tiles + 1u) >> 1, c_per = W / n_pairs;
    uint32_t w;
    {
        const uint32_t b = blockIdx.x, x = b & 7u, base = W >> 3, rem = W & 7u;
        const uint32_t L = x * base + (x < rem ? x : rem) + (b >> 3);  // XCDs 0 .. rem-1 run base + 1 blocks
        w = (L % n_pairs) * c_per + L / n_pairs;
    }
    const uint32_t pt = w / c_per, seg = w % c_per;
    const uint32_t rt0 = (uint32_t)((unsigned long long)seg * n_tiles / c_per);
    const uint32_t rt1 = (uint32_t)((unsigned long long)(seg + 1) * n_tiles / c_per);
    if (rt0 >= rt1) return;  // (workgroup-uniform)
    const uint32_t qt = 2u * pt + (uint32_t)(wave >> 2);
    const bool active = qt < q_tiles;  // odd q_tiles: the last pair's upper half has no queries
    const size_t q0 = active ? (size_t)qt * kBQ + (size_t)(wave & 3) * 64 : 0;  // first query of this wave
    const size_t cell0 = (size_t)seg * nq_pad + q0;                             // its (segment, query) cell

    // ---- per-run state: B fragments and thresholds in registers (requested in front of the prologue's barrier, whose
    // vmcnt(0) covers them: the tile loop then never waits for vector memory at its top)
    bf16x8 b0[KS], b1[KS];
    float tau0 = __uint_as_float(0xFF800000u), tau1 = tau0;  // (a half without queries keeps -inf)
    if (active) {
        const u32x4 *br0 = Bq + (q0 + jq) * (size_t)C + h;
        const u32x4 *br1 = br0 + (size_t)32 * C;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const u32x4 v0 = br0[2 * ks], v1 = br1[2 * ks];
            b0[ks] = __builtin_bit_cast(bf16x8, v0);
            b1[ks] = __builtin_bit_cast(bf16x8, v1);
        }
        if (sh.seed_lists) {  // as the 4-wave kernel: lane L derives query q0 + L's threshold, the lanes pick up their two
            const size_t ql = q0 + (size_t)lane;
            float sd = __uint_as_float(0xFF800000u);
            if (ql < (size_t)sh.seed_nq) {
                const uint32_t key = f2s(bf_seed_lane(sh.seed_lists, nq_pad, sh.nseg, sh.seed_rank, ql));
                sd = s2f(key == 0xFFFFFFFFu ? key : key + 1u);  // rows with a bound EQUAL to it still pass the strict '<'
            }
            tau0 = __shfl(sd, jq);
            tau1 = __shfl(sd, 32 + jq);
        } else {
            tau0 = s2f(tau_init[q0 + jq]);
            tau1 = s2f(tau_init[q0 + 32 + jq]);
        }
    } else {
        const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            b0[ks] = __builtin_bit_cast(bf16x8, zero);
            b1[ks] = b0[ks];
        }
    }
    // prologue, the same instructions for both halves: the run's first 2 MEET tiles, one barrier (it carries the vmcnt(0))
    {
        constexpr int P = (CP + 7) / 8;
        const int n_mine = CP - wave * P < P ? (CP - wave * P > 0 ? CP - wave * P : 0) : P;
        // (rt0 + t < rt1, and `rt + 2 MEET + j < rt1` / `last` in bf_pair_run: the guards of the shortest runs.  No call
        // reaches them -- the plan's shortest aligned run is ~9-12 tiles, tests/test_gpu_bf16_pair.py -- so they are
        // argued, not exercised: a one-tile run loads one tile, meets its one barrier and requests nothing further.)
        for (uint32_t t = 0; t < 2u * MEET && rt0 + t < rt1; ++t) {
            const char *ws = img + ((size_t)(rt0 + t) * (size_t)TB + (size_t)(wave * (P * 1024))) + (uint32_t)lane * 16u;
            char *wd = tiles + t * TB + wave * (P * 1024);
            if (0 < n_mine) __builtin_amdgcn_global_load_lds((glb_void_b *)ws, (lds_void_b *)wd, 16, 0, 0);
            if (P > 1 && 1 < n_mine) __builtin_amdgcn_global_load_lds((glb_void_b *)ws, (lds_void_b *)wd, 16, 1024, 0);
            if (P > 2 && 2 < n_mine) __builtin_amdgcn_global_load_lds((glb_void_b *)ws, (lds_void_b *)wd, 16, 2048, 0);
        }
    }
    __syncthreads();
    // the two roles: one loop, two placements of its barrier; split by wave number >= 4, the SIMD partner of wave w is
    // wave w + 4 (MI355X_MICROARCH.md, "Two waves per SIMD", item 9)
    if (wave >= 4)
        bf_pair_run<KS, CI, kPairStagger, MEET>(img, tiles, kp, kfin, cand, ccnt, ctau, b0, b1, tau0, tau1, rt0, rt1,
                                                cell0, active, wave, lane);
    else
        bf_pair_run<KS, CI, 0, MEET>(img, tiles, kp, kfin, cand, ccnt, ctau, b0, b1, tau0, tau1, rt0, rt1, cell0, active,
                                     wave, lane);
}

template <int KS, bool CI>
__global__ __launch_bounds__(512, 2) void bf16_filter_kernel_pair(const char *__restrict__ img, uint32_t n_tiles,
                                                                  const u32x4 *__restrict__ Bq, uint32_t q_tiles,
                                                                  uint32_t kp_keep, uint2 *__restrict__ cand,
                                                                  uint32_t *__restrict__ ccnt,
                                                                  uint32_t *__restrict__ ctau, size_t nq_pad,
                                                                  const uint32_t *tau_init, BfShared sh) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];  // [3][TB]
    bf_pair_body<KS, CI, 1>(reinterpret_cast<char *>(smem_raw), img, n_tiles, Bq, q_tiles, kp_keep, cand, ccnt, ctau, nq_pad,
                            tau_init, sh);
}
// ... and with MEET tiles per meeting (kPairMeet = 2; Bf16Kernel::PairTwo)
template <int KS, bool CI, int MEET>
__global__ __launch_bounds__(512, 2) void bf16_filter_kernel_meet_pair(const char *__restrict__ img, uint32_t n_tiles,
                                                                       const u32x4 *__restrict__ Bq, uint32_t q_tiles,
                                                                       uint32_t kp_keep, uint2 *__restrict__ cand,
                                                                       uint32_t *__restrict__ ccnt,
                                                                       uint32_t *__restrict__ ctau, size_t nq_pad,
                                                                       const uint32_t *tau_init, BfShared sh) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];  // [3 MEET][TB]
    bf_pair_body<KS, CI, MEET>(reinterpret_cast<char *>(smem_raw), img, n_tiles, Bq, q_tiles, kp_keep, cand, ccnt, ctau,
                               nq_pad, tau_init, sh);
}

// ---------------------------------------------------------------------------
// Wide rows (128 < D <= 1024): the query operand no longer fits the register file, so the contraction is a
// K-chunked tile product with BOTH operands streamed through LDS:
//  * a workgroup is 8 waves and owns a 256-row x 256-query tile; wave (rh, qg) computes the 128 x 64 sub-tile of
//    row half rh and query group qg in 4 x 2 accumulator blocks (128 VGPRs): per MFMA step 4 + 2 ds_read_b128 feed
//    8 MFMAs (0.75 LDS reads per MFMA; the LDS sustains 2);
//  * a stage is one chunk (4 steps = 64 columns) of both operands, 2 x 32 KiB, two stages; the eight waves issue the
//    64 LDS-DMA pieces of the next stage (waves 0-3 the corpus piece, 4-7 the query piece) right behind the one
//    barrier per chunk; the query chunks are re-streamed for every row tile from L2, where the XCD-aware block order
//    below keeps them (and shares every corpus tile between the workgroups of an XCD);
//  * after the last chunk of a row tile the eight blocks are reduced and filtered exactly as in the narrow
//    kernel (bf_slow, bf_compact); the other wave of the SIMD keeps the matrix pipe busy meanwhile;
//  * the two row halves of a workgroup are two SEGMENTS of the query (own buffers, own thresholds); the partition is
//    the balanced persistent one of the narrow kernel (equal slices of the (query tile, row tile) list, one
//    workgroup per CU), so a query has 2 x (workgroups touching its tile) segments;
//  * thresholds start from a scout pass over the run's first tiles: the wave's own seed, or -- shared scout, as for
//    narrow rows -- a scout-only launch whose lists bf16_seed_kernel merges per query over all segments.
// ---------------------------------------------------------------------------
template <int M, bool RAD>
__global__ __launch_bounds__(512, 1) void bf16_wide_kernel(const char *__restrict__ img, uint32_t n_tiles,
                                                           const char *__restrict__ Bimg, uint32_t nkc,
                                                           uint32_t tile_bytes, uint32_t has_x, uint32_t kp,
                                                           uint2 *__restrict__ cand, uint32_t *__restrict__ ccnt,
                                                           uint32_t *__restrict__ ctau, size_t nq_pad,
                                                           uint32_t scout_max,
                                                           const uint32_t *__restrict__ tau_init,
                                                           float *__restrict__ scout_out) {
    constexpr uint32_t CAP = 64u * M;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    char *lds = reinterpret_cast<char *>(smem_raw);  // [2][kWStage]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int jq = lane & 31, h = lane >> 5;
    const int qg = wave & 3, rh = wave >> 2;
    BF_DBG_DECL;

    // Logical workgroup: hardware block b runs on XCD b % 8.  Giving each XCD a contiguous range of logical
    // workgroups puts a few query tiles' row ranges on one L2 (their chunks are re-read from there) and lets
    // workgroups of different query tiles that walk the same rows share each corpus tile.
    uint32_t w = blockIdx.x;
    const uint32_t W = gridDim.x;
    {   // XCD x runs the blocks b = x, x + 8, ...: it gets the logical range that starts where XCD x - 1's ends
        const uint32_t x = blockIdx.x & 7u, base = W >> 3, rem = W & 7u;  // XCDs 0 .. rem-1 run base + 1 blocks
        w = x * base + (x < rem ? x : rem) + (blockIdx.x >> 3);
    }
    // Balanced persistent partition (as bf16_filter_kernel): the work is the list of (query tile, row tile) units in
    // query-major order, workgroup w owns the contiguous slice [w U / W, (w+1) U / W) and walks it in runs that stay
    // inside one query tile.  Segment of a run = ordinal of the workgroup among those touching that query tile.
    const unsigned long long U = (unsigned long long)(nq_pad / kWR) * n_tiles, Wn = W;
    unsigned long long u0 = (unsigned long long)w * U / Wn;
    const unsigned long long u1 = (unsigned long long)(w + 1) * U / Wn;
    const float inf = __uint_as_float(0x7F800000u);

    int slot_off[4];  // byte offset of this lane's fragment of step s inside its row (swizzled slot 2s + h)
#pragma unroll
    for (int s = 0; s < 4; ++s) slot_off[s] = (int)(((unsigned)(2 * s + h) ^ bf_wide_swz((size_t)jq)) * 16u);
    int st = 0;       // stage that holds (or is receiving) the next chunk to contract
    uint32_t ns = 0;  // vector-memory instructions issued since this wave's last LDS-DMA (bf_wait_dma)
    f32x16 acc[4][2];

    while (u0 < u1) {
    const uint32_t qt = (uint32_t)(u0 / n_tiles);
    const unsigned long long v_begin = (unsigned long long)qt * n_tiles, v_end = v_begin + n_tiles;
    const unsigned long long run_end = u1 < v_end ? u1 : v_end;
    const uint32_t rt0 = (uint32_t)(u0 - v_begin), rt1 = (uint32_t)(run_end - v_begin);
    unsigned long long wf = v_begin * Wn / U;  // first workgroup touching query tile qt
    while ((wf + 1) * U / Wn <= v_begin) ++wf;
    while (wf > 0 && wf * U / Wn > v_begin) --wf;
    const uint32_t sg = (uint32_t)(w - wf);
    const size_t q0 = (size_t)qt * kWR + (size_t)qg * 64;                 // first query of this wave
    const size_t cell0 = (size_t)(sg * 2 + rh) * nq_pad + q0;             // its (segment, query) cell
    float tau0 = inf, tau1 = inf;
    uint32_t cnt0 = 0, cnt1 = 0;

    // LDS-DMA of one stage: 64 pieces of 1 KiB, eight per wave
    const bool is_a = wave < 4;
    const char *src0 = (is_a ? img : Bimg + (size_t)qt * tile_bytes) + (size_t)(wave & 3) * (kWDma * 1024) + lane * 16;
    char *dst0 = lds + (is_a ? 0 : kWPiece) + (wave & 3) * (kWDma * 1024);
    auto src_of = [&](uint32_t rt, uint32_t c) {
        return src0 + (is_a ? (size_t)rt * tile_bytes + (size_t)c * kWPiece : (size_t)c * kWPiece);
    };
    // extras piece of row tile rt -> LDS area [rt & 1] behind the stages: eight pieces, one per wave
    char *ldsx = lds + 2 * kWStage;
    auto issue_x = [&](uint32_t rt) {
        const char *src = img + (size_t)rt * tile_bytes + (size_t)nkc * kWPiece + wave * 1024 + lane * 16;
        __builtin_amdgcn_global_load_lds((glb_void_b *)src, (lds_void_b *)(ldsx + (rt & 1u) * kWXPiece + wave * 1024), 16, 0,
                                         0);
    };
    auto issue = [&](uint32_t rt, uint32_t c, int stage) {
        const char *src = src_of(rt, c);
        char *dst = dst0 + stage * kWStage;
#pragma unroll
        for (int i = 0; i < kWDma; ++i)
            __builtin_amdgcn_global_load_lds((glb_void_b *)(src + i * 1024), (lds_void_b *)(dst + i * 1024), 16, 0, 0);
        if (has_x && c == 0) issue_x(rt);
    };
    // the wave's query extras (two fragments): loaded once per run, before any LDS-DMA of the run is in flight
    bf16x8 bx0, bx1;
    {
        u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
        if (has_x) {
            const char *bxp = Bimg + (size_t)qt * tile_bytes + (size_t)nkc * kWPiece;
            const size_t r0 = (size_t)(qg * 64 + jq), r1 = r0 + 32;
            v0 = *reinterpret_cast<const u32x4 *>(bxp + r0 * 32 + ((unsigned)h ^ bf_wide_xswz(r0)) * 16);
            v1 = *reinterpret_cast<const u32x4 *>(bxp + r1 * 32 + ((unsigned)h ^ bf_wide_xswz(r1)) * 16);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("" : "+v"(v0), "+v"(v1));
        bx0 = __builtin_bit_cast(bf16x8, v0);
        bx1 = __builtin_bit_cast(bf16x8, v1);
    }

    // contraction of row tile rt (its chunk 0 is already on its way into stage st); rt_end: end of the tile sequence
    auto contract = [&](uint32_t rt, uint32_t rt_end) {
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                acc[rb][0][i] = 0.0f;
                acc[rb][1][i] = 0.0f;
            }
        for (uint32_t c = 0; c < nkc; ++c) {
            // chunk barrier: every wave's share of this stage has landed and nobody still reads the other stage
            bf_wait_dma<true>(ns);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            // the nine LDS-DMA pieces of the next stage are issued one at a time between the first MFMA pairs: a
            // burst of nine right behind the barrier keeps all eight waves in the memory pipeline's queue at once
            // while the matrix pipe idles
            const bool more = c + 1 < nkc || rt + 1 < rt_end;
            const char *nsrc = c + 1 < nkc ? src_of(rt, c + 1) : src_of(rt + 1 < rt_end ? rt + 1 : rt, 0);
            char *ndst = dst0 + (st ^ 1) * kWStage;
            ns = 0;
            // row (rh*128 + rb*32 + jq) and query (qg*64 + qb*32 + jq) share the swizzle key of jq
            const char *A = lds + st * kWStage + (rh * 128 + jq) * kWPitch;
            const char *B = lds + st * kWStage + kWPiece + (qg * 64 + jq) * kWPitch;
            // Fragments one step ahead: the next step's B pair and last A fragment are requested when a step begins,
            // its other A fragments as this step's die (two MFMAs each) -- 12 registers more than one step's set, and
            // no step but a chunk's first waits for LDS.  (Requested at the head of their own step, as before, every
            // step began with a round trip: the loop alone, operands already in LDS, ran at 0.60 of the peak.)
            bf16x8 a[4], b[2];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) a[rb] = *reinterpret_cast<const bf16x8 *>(A + rb * 32 * kWPitch + slot_off[0]);
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) b[qb] = *reinterpret_cast<const bf16x8 *>(B + qb * 32 * kWPitch + slot_off[0]);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                bf16x8 na[4], nb[2];
                if (s < 3) {
#pragma unroll
                    for (int qb = 0; qb < 2; ++qb)
                        nb[qb] = *reinterpret_cast<const bf16x8 *>(B + qb * 32 * kWPitch + slot_off[s < 3 ? s + 1 : s]);
                    na[3] = *reinterpret_cast<const bf16x8 *>(A + 3 * 32 * kWPitch + slot_off[s < 3 ? s + 1 : s]);
                }
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) {
#pragma unroll
                    for (int qb = 0; qb < 2; ++qb) {
                        acc[rb][qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rb], b[qb], acc[rb][qb], 0, 0, 0);
                        const int m = (s * 4 + rb) * 2 + qb;  // MFMA number within the chunk
                        const int piece = m / 3;
                        if (m == 26) {  // ninth piece: the extras of the next row tile travel with its chunk 0
                            __builtin_amdgcn_sched_barrier(0);
                            if (has_x && c + 1 == nkc && rt + 1 < rt_end) issue_x(rt + 1);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        if (m % 3 == 2 && piece < kWDma) {
                            __builtin_amdgcn_sched_barrier(0);
                            if (more)
                                __builtin_amdgcn_global_load_lds((glb_void_b *)(nsrc + piece * 1024),
                                                                 (lds_void_b *)(ndst + piece * 1024), 16, 0, 0);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                    if (s < 3 && rb < 3) {  // a[rb] is dead: the next step's fragment may land in its registers
                        __builtin_amdgcn_sched_barrier(0);
                        na[rb] = *reinterpret_cast<const bf16x8 *>(A + rb * 32 * kWPitch + slot_off[s < 3 ? s + 1 : s]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if (s < 3) {
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb) a[rb] = na[rb];
                    b[0] = nb[0];
                    b[1] = nb[1];
                }
            }
            st ^= 1;
        }
        if (has_x) {  // the extras step: landed with the tile's chunk 0, read by this wave only now
            const char *X = ldsx + (rt & 1u) * kWXPiece + (rh * 128 + jq) * 32 + (((unsigned)h ^ bf_wide_xswz((size_t)jq)) * 16);
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const bf16x8 ax = *reinterpret_cast<const bf16x8 *>(X + rb * 32 * 32);
                acc[rb][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ax, bx0, acc[rb][0], 0, 0, 0);
                acc[rb][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ax, bx1, acc[rb][1], 0, 0, 0);
            }
        }
    };

    // ---- scout pass (see bf16_filter_kernel): the first tiles contracted without buffers, thresholds seeded with
    // the 5th smallest block minimum of the wave's rows
    const uint32_t run_len = rt1 - rt0;
    uint32_t t_scout = run_len / 32u < scout_max ? run_len / 32u : scout_max;
    if (tau_init) {  // thresholds given by the caller (radius: each query's fixed bound; k-NN: the shared seed)
        t_scout = 0;
        tau0 = s2f(tau_init[q0 + jq]);
        tau1 = s2f(tau_init[q0 + 32 + jq]);
    }
    if (scout_out) {  // scout-only launch: every run contributes its lists, however short it is
        t_scout = run_len < scout_max ? run_len : scout_max;
        if (t_scout < 1u) t_scout = 1u;
    }
    if (t_scout) {
        float s0[kScoutList], s1[kScoutList];
#pragma unroll
        for (int i = 0; i < kScoutList; ++i) { s0[i] = inf; s1[i] = inf; }
        auto insert = [](float (&l)[kScoutList], float x) {
            float c = x;
#pragma unroll
            for (int i = 0; i < kScoutList; ++i) {
                const float lo = fminf(l[i], c);
                c = fmaxf(l[i], c);
                l[i] = lo;
            }
        };
        __syncthreads();
        issue(rt0, 0, st);
        for (uint32_t rt = rt0; rt < rt0 + t_scout; ++rt) {
            contract(rt, rt0 + t_scout);
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                float m0 = acc[rb][0][0], m1 = acc[rb][1][0];
#pragma unroll
                for (int i = 1; i < 16; ++i) {
                    m0 = fminf(m0, acc[rb][0][i]);
                    m1 = fminf(m1, acc[rb][1][i]);
                }
                insert(s0, m0);
                insert(s1, m1);
            }
        }
        if (scout_out) {  // publish this lane's lists: [cell][half][kScoutList]; bf16_seed_kernel merges a query's cells
            float *o0 = scout_out + ((cell0 + jq) * 2 + h) * kScoutList;
            float *o1 = scout_out + ((cell0 + 32 + jq) * 2 + h) * kScoutList;
#pragma unroll
            for (int i = 0; i < kScoutList; ++i) {
                o0[i] = s0[i];
                o1[i] = s1[i];
            }
            u0 = run_end;
            continue;
        }
        auto union5 = [](const float (&a)[kScoutList]) {
            const float b1 = __shfl_xor(a[0], 32), b2 = __shfl_xor(a[1], 32), b3 = __shfl_xor(a[2], 32),
                        b4 = __shfl_xor(a[3], 32), b5 = __shfl_xor(a[4], 32);
            const float x = fminf(fminf(a[4], b5), fminf(fmaxf(a[0], b4), fmaxf(a[3], b1)));
            return fminf(x, fminf(fmaxf(a[1], b3), fmaxf(a[2], b2)));
        };
        tau0 = union5(s0);
        tau1 = union5(s1);
    }

    uint2 *ce_blk0 = cand + cell0 * CAP;
    uint2 *ce_blk1 = ce_blk0 + (size_t)32 * CAP;
    uint2 *ceq0 = ce_blk0 + (size_t)jq * CAP, *ceq1 = ce_blk1 + (size_t)jq * CAP;

    // ---- main pass
    __syncthreads();
    issue(rt0, 0, st);
    ns = 0;
    for (uint32_t rt = rt0; rt < rt1; ++rt) {
        contract(rt, rt1);
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            float m0 = acc[rb][0][0], m1 = acc[rb][1][0];
#pragma unroll
            for (int i = 1; i < 16; ++i) {
                m0 = fminf(m0, acc[rb][0][i]);
                m1 = fminf(m1, acc[rb][1][i]);
            }
            const uint32_t row0 = rt * (uint32_t)kWR + (uint32_t)(rh * 128 + rb * 32);
            if (__any(m0 < tau0))
                bf_slow<M, RAD>(acc[rb][0], m0, tau0, cnt0, row0, h, jq, lane, kp, ceq0, ce_blk0, ns BF_DBG_PASS);
            if (__any(m1 < tau1))
                bf_slow<M, RAD>(acc[rb][1], m1, tau1, cnt1, row0, h, jq, lane, kp, ceq1, ce_blk1, ns BF_DBG_PASS);
        }
    }
    // ---- end of run: at most kp candidates per query stay; publish count and threshold
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned long long need = RAD ? 0ull : __ballot(h == 0 && cnt0 > kp);
    while (need) {
        const int j = __builtin_ctzll(need);
        need &= need - 1;
        const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane((int)cnt0, j);
        uint32_t T, nn;
        bf_compact<M>(ce_blk0 + (size_t)j * CAP, cj, kp, lane, T, nn);
        if (jq == j) { tau0 = fminf(tau0, s2f(T)); cnt0 = nn; }
    }
    need = RAD ? 0ull : __ballot(h == 0 && cnt1 > kp);
    while (need) {
        const int j = __builtin_ctzll(need);
        need &= need - 1;
        const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane((int)cnt1, j);
        uint32_t T, nn;
        bf_compact<M>(ce_blk1 + (size_t)j * CAP, cj, kp, lane, T, nn);
        if (jq == j) { tau1 = fminf(tau1, s2f(T)); cnt1 = nn; }
    }
    if (h == 0) {
        ccnt[cell0 + jq] = cnt0;
        ctau[cell0 + jq] = f2s(tau0);
        ccnt[cell0 + 32 + jq] = cnt1;
        ctau[cell0 + 32 + jq] = f2s(tau1);
    }
    u0 = run_end;
    }  // runs
}

#ifdef PN_DIAG_BF_COUNT
extern "C" int pn_debug_read_bf(unsigned long long *out, int reset) {
    unsigned long long z[16] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bfdbg), sizeof(z)) != hipSuccess) return 1;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_bfdbg), z, sizeof(z)) != hipSuccess) return 1;
    return 0;
}
extern "C" int pn_debug_read_bf_lag(unsigned long long *out, int reset) {
    unsigned long long z[16] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bfdbg_lag), sizeof(z)) != hipSuccess) return 1;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_bfdbg_lag), z, sizeof(z)) != hipSuccess) return 1;
    return 0;
}
#endif

// ---------------------------------------------------------------------------
// The one hardware assumption of the bound, checked by the PRODUCT (round 4; VERDICT r3: "a product that silently depends
// on a test being run is weak").  g = 2^-13 allows the matrix core's f32 accumulation of a chain an error of g * sum|terms|
// -- a property of v_mfma_f32_32x32x16_bf16 that the ISA documents do not state and tests/test_gpu_bf16*.py measure
// (<= 0.0016 of the allowance on gfx950).  Before the first index of a process on a device gets its bf16 tier, this
// kernel contracts synthetic operands of mixed signs and scales over chains of 8, 65 and 257 steps from a non-zero
// accumulator (the narrow kernel's chain, the wide kernel's at D = 1024 and at its limit D = 4096), rebuilds every term in f64 -- bf16 x bf16
// products are exact there, and 1041 of them sum with a relative error below 2^-42 -- and reports the largest
// |delivered - exact| / (g * sum|terms|).  The host refuses the tier above 0.02 (what the tests assert).  One wave,
// ~0.5 ms, once per process and device (rocprofv3, round 4: 1.2 ms with twice the checked outputs).
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint16_t bf_selftest_val(uint32_t i, uint32_t k, uint32_t salt) {
    uint32_t x = (i * 0x9E3779B1u) ^ (k * 0x85EBCA77u) ^ (salt * 0xC2B2AE3Du);
    x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12; x *= 0x297A2D39u; x ^= x >> 15;
    const uint32_t sign = x & 1u, mant = (x >> 1) & 0x7Fu, e = 127u - 4u + ((x >> 8) % 9u);  // 2^-4 .. 2^4
    return (uint16_t)((sign << 15) | (e << 7) | mant);
}
__global__ __launch_bounds__(64) void bf16_selftest_kernel(float *__restrict__ out) {
    const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    float worst = 0.0f;
    constexpr int NR = 2;                       // registers checked per lane (128 of the 1024 outputs of a block; the f64
    const int regs[NR] = {3, 12};               // reference, not the MFMAs, is this kernel's time: ~0.5 ms once per device)
    for (int pass = 0; pass < 3; ++pass) {
        const int steps = pass == 0 ? 8 : pass == 1 ? 65 : 257;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) {  // C/D map: register r of lane (j, h) = row (r & 3) + 8 (r >> 2) + 4 h, column j
            const uint32_t row = (uint32_t)((r & 3) + 8 * (r >> 2) + 4 * h);
            acc[r] = bf_f(bf_selftest_val(row, 4096u + (uint32_t)j, 7u + (uint32_t)pass)) * 5.0f;
        }
        double ref[NR], mag[NR];
#pragma unroll
        for (int c = 0; c < NR; ++c) {
            ref[c] = (double)acc[regs[c]];
            mag[c] = fabs(ref[c]);
        }
        for (int ks = 0; ks < steps; ++ks) {
            // A: lane (i = j, half h) holds A[i][16 ks + 8 h .. + 8); B: lane (j, half h) holds B[16 ks + 8 h .. + 8)[j]
            uint16_t av[8], bv[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const uint32_t k = (uint32_t)(16 * ks + 8 * h + t);
                av[t] = bf_selftest_val((uint32_t)j, k, 1u + (uint32_t)pass);
                bv[t] = bf_selftest_val(1000u + (uint32_t)j, k, 3u + (uint32_t)pass);
            }
            u32x4 au, bu;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                au[t] = (uint32_t)av[2 * t] | ((uint32_t)av[2 * t + 1] << 16);
                bu[t] = (uint32_t)bv[2 * t] | ((uint32_t)bv[2 * t + 1] << 16);
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, au), __builtin_bit_cast(bf16x8, bu), acc, 0, 0, 0);
            for (int k = 16 * ks; k < 16 * ks + 16; ++k) {
                const double bk = (double)bf_f(bf_selftest_val(1000u + (uint32_t)j, (uint32_t)k, 3u + (uint32_t)pass));
#pragma unroll
                for (int c = 0; c < NR; ++c) {
                    const uint32_t row = (uint32_t)((regs[c] & 3) + 8 * (regs[c] >> 2) + 4 * h);
                    const double p = (double)bf_f(bf_selftest_val(row, (uint32_t)k, 1u + (uint32_t)pass)) * bk;
                    ref[c] += p;
                    mag[c] += fabs(p);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < NR; ++c) {
            const double ratio = fabs((double)acc[regs[c]] - ref[c]) / (kG * mag[c]);
            worst = fmaxf(worst, (float)ratio);
            if (!(ratio == ratio)) worst = 3.0e38f;  // a NaN anywhere: refuse
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) worst = fmaxf(worst, __shfl_xor(worst, d));
    if (lane == 0) out[0] = worst;
}
hipError_t launch_bf16_selftest(float *out, hipStream_t s) {
    hipLaunchKernelGGL(bf16_selftest_kernel, dim3(1), dim3(64), 0, s, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int bf16_ks_for(int dim, bool ci) { return bf16_steps_for(dim, ci); }
bool bf16_ci_candidate(int dim) { return bf16_ci_dim(dim); }
// D <= 128: operand-stationary kernel (bf16_filter_kernel); 128 < D <= 4096: K-chunked kernel (bf16_wide_kernel).
// The accumulation-error allowance g = 2^-13 is a measured property of the hardware: checked against chains of up to 65
// MFMA steps (tests/test_gpu_bf16.py, tests/test_gpu_bf16_wide.py: error <= 0.0016 of the allowance, not growing with the
// chain; bf16_selftest_kernel checks chains of 8, 65 and 257 steps on the device the index lives on).
// (round 4: 1024 -> 4096 columns, 257 MFMA steps -- chains of that length are part of the product's self-test)
bool bf16_supported(int dim) { return dim >= 1 && dim <= 4096; }
bool bf16_is_wide(int dim) { return dim > 128; }
size_t bf16_image_bytes(size_t n, int dim, bool ci) {
    if (bf16_is_wide(dim))
        return (n + kWR - 1) / kWR * bf16_wide_tile_bytes(dim);
    const size_t n_tiles = (n + kBP - 1) / kBP;
    return n_tiles * (size_t)kBP * (size_t)(2 * bf16_ks_for(dim, ci) + 1) * 16;
}
size_t bf16_query_bytes(size_t nq_pad, int dim, bool ci) {
    if (bf16_is_wide(dim))
        return (nq_pad + kWR - 1) / kWR * bf16_wide_tile_bytes(dim);
    return nq_pad * (size_t)bf16_ks_for(dim, ci) * 32;
}
// a buffer is compacted once fewer than 32 free slots remain; a compaction is also what refreshes the threshold,
// so small k' take the small buffer (measured: k' = 12, 64 slots 4.7 ms vs 128 slots 5.2 ms on the headline config)
int bf16_cap_for(int kp) { return kp <= 16 ? 64 : kp <= 64 ? 128 : 256; }
int bf16_query_tile() { return kBQ; }
// entries a (segment, query) cell holds at most when a k-NN launch has finished: every run ends with a cut to k'
int bf16_cell_max(int kp, int cap, int nseg, bool wide) {
    const int cut = kp < cap ? kp : cap;
    // (128-slot buffers ending their runs uncut as well: measured at 1M x 128, k = 100 (k' = 42, 65 entries per buffer at
    // the end of a run, the cut 4.9 % of a wave's run): kernel 2.86 -> 2.81 / 2.75 ms at 64 / 96 entries, step 3.29 ->
    // 3.35 / 3.54 -- the re-rank's LDS and gather lose more: not used.)
    if (wide || cap != 64 || nseg < 1) return cut;
    // 64-slot buffers of the narrow kernel end a run uncut up to `keep` entries (CandBuf::final_keep; the kernel's end of
    // run has the measurements): as many as keep the re-rank's LDS -- 12 bytes per slot a query's cells can hold -- near
    // 4.6 KB, i.e. 32 of its one-wave workgroups on a CU
    int keep = 384 / nseg;
    if (keep > kBfFinalKeep) keep = kBfFinalKeep;
    return keep > cut ? keep : cut;
}

// per-dimension sums of the corpus in f64 (any translation vector is valid; the mean minimises the norms);
// sums[dim] receives the sum of all squares
template <typename T>
__global__ void bf16_column_sums_kernel(const T *__restrict__ P, size_t n, int dim, size_t ld, double *__restrict__ sums) {
    const size_t r0 = (size_t)blockIdx.x * 1024;
    const size_t r1 = r0 + 1024 < n ? r0 + 1024 : n;
    for (int k = threadIdx.x; k < dim; k += blockDim.x) {
        double a = 0.0, b = 0.0;
        for (size_t r = r0; r < r1; ++r) {
            const double x = (double)P[r * ld + k];
            const double v = (fabs(x) < 1.0e30) ? x : 0.0;
            a += v;
            b += v * v;
        }
        atomicAdd(&sums[k], a);
        atomicAdd(&sums[dim], b);
    }
}
template <typename T>
hipError_t launch_bf16_column_sums(const T *P, size_t n, int dim, size_t ld, double *sums, hipStream_t s) {
    hipLaunchKernelGGL(bf16_column_sums_kernel<T>, dim3((unsigned)((n + 1023) / 1024)), dim3(128), 0, s, P, n, dim, ld, sums);
    return hipGetLastError();
}
template hipError_t launch_bf16_column_sums<float>(const float *, size_t, int, size_t, double *, hipStream_t);
template hipError_t launch_bf16_column_sums<double>(const double *, size_t, int, size_t, double *, hipStream_t);

// The translation vector, decided on the device (round 4: finish_index read the sums back and decided on the host -- one
// of six stream synchronisations of an index build).  sums = bf16_column_sums_kernel's output (dim column sums, then the
// sum of all squares): mu = the per-dimension mean as f32, kept when translating shrinks the sum of squared norms by
// `factor` (16; wide rows 2: DESIGN.md 4.0b), else zero.  words[0] = 1 when the corpus is translated.  One thread.
__global__ void bf16_decide_mu_kernel(const double *__restrict__ sums, size_t n, int dim, double factor, int never,
                                      float *__restrict__ mu, uint32_t *__restrict__ words) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double mu2 = 0.0;
    for (int k = 0; k < dim; ++k) {
        const double m = sums[k] / (double)n;
        const float f = (m == m && fabs(m) < 1e30) ? (float)m : 0.0f;
        mu[k] = f;
        mu2 += (double)f * (double)f;
    }
    // sum |p - mu|^2 = sum |p|^2 - n |mu|^2
    const double s2 = sums[dim], s2c = s2 - (double)n * mu2;
    const bool centered = !never && s2 > 0.0 && s2c < s2 / factor;
    if (!centered)
        for (int k = 0; k < dim; ++k) mu[k] = 0.0f;
    words[0] = centered ? 1u : 0u;
}
hipError_t launch_bf16_decide_mu(const double *sums, size_t n, int dim, bool never, float *mu, uint32_t *words, hipStream_t s) {
    hipLaunchKernelGGL(bf16_decide_mu_kernel, dim3(1), dim3(64), 0, s, sums, n, dim, bf16_is_wide(dim) ? 2.0 : 16.0,
                       never ? 1 : 0, mu, words);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_bf16_row_stats(const T *P, const float *mu, size_t n, int dim, size_t ld, double *out4,
                                 hipStream_t s) {
    if (!bf16_is_wide(dim)) {  // (row statistics decide about the CI layout: its step count bounds the columns a lane owns)
        const size_t rows = (n + 31) / 32 * 32;  // whole blocks of 256 threads = 32 rows
        const size_t blocks = rows * 8 / 256;
        hipLaunchKernelGGL(bf16_row_stats8_kernel<T>, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, P, mu,
                           n, dim, ld, bf16_ks_for(dim, false), rows, out4);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(bf16_row_stats_kernel<T>, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, s, P, mu, n, dim, ld, out4);
    return hipGetLastError();
}
template hipError_t launch_bf16_row_stats<float>(const float *, const float *, size_t, int, size_t, double *, hipStream_t);
template hipError_t launch_bf16_row_stats<double>(const double *, const float *, size_t, int, size_t, double *, hipStream_t);

template <typename T>
hipError_t launch_bf16_pack_corpus(const T *P, const float *mu, size_t n, int dim, size_t ld, void *img,
                                   uint32_t *bad, bool ci, hipStream_t s) {
    const bool wide = bf16_is_wide(dim);
    if (wide && ci) return hipErrorInvalidValue;
    const size_t rows = wide ? (n + kWR - 1) / kWR * kWR : (n + kBP - 1) / kBP * kBP;
    if (wide) {  // rows is a multiple of 256
        hipLaunchKernelGGL((bf16_pack_wide8_kernel<T, false>), dim3((unsigned)(rows * 8 / 256)), dim3(256), 0, s, P, mu, n, rows,
                           dim, ld, static_cast<uint16_t *>(img), (double *)nullptr, (uint32_t *)nullptr, bad, Bf16SeedModel{});
        return hipGetLastError();
    }
    // narrow rows: rows is a multiple of 64 -- whole blocks of 256 threads = 32 rows
    hipLaunchKernelGGL(bf16_pack_corpus8_kernel<T>, dim3((unsigned)(rows * 8 / 256)), dim3(256), 0, s, P, mu, n, dim, ld,
                       bf16_ks_for(dim, ci), static_cast<uint16_t *>(img), rows, bad, ci ? 1 : 0);
    return hipGetLastError();
}
template hipError_t launch_bf16_pack_corpus<float>(const float *, const float *, size_t, int, size_t, void *, uint32_t *, bool, hipStream_t);
template hipError_t launch_bf16_pack_corpus<double>(const double *, const float *, size_t, int, size_t, void *, uint32_t *, bool, hipStream_t);

bool bf16_pack_fused_supported(int dim) { return !bf16_is_wide(dim); }
template <typename T>
hipError_t launch_bf16_pack_queries(const T *Q, const float *mu, size_t nq, size_t nq_pad, int dim, size_t ld,
                                    void *B, double *qn, uint32_t *qbad, bool ci, double bmax, double dmax,
                                    hipStream_t s, T *Qp, size_t ldq, uint32_t *misc, const Bf16SeedModel *smp) {
    if ((Qp || misc) && !bf16_pack_fused_supported(dim)) return hipErrorInvalidValue;
    Bf16SeedModel sm{};
    if (smp) sm = *smp;
    if (sm.seed_out && (!sm.m1 || !sm.a || !sm.b)) return hipErrorInvalidValue;
    if (!bf16_is_wide(dim)) {  // nq_pad is a multiple of 256: whole blocks
        hipLaunchKernelGGL(bf16_pack_queries8_kernel<T>, dim3((unsigned)(nq_pad * 8 / 256)), dim3(256), 0, s, Q, mu, nq,
                           nq_pad, dim, ld, bf16_ks_for(dim, ci), static_cast<uint16_t *>(B), qn, qbad, ci ? 1 : 0,
                           bmax, dmax, Qp, ldq, misc, sm);
        return hipGetLastError();
    }
    // wide rows: no CI layout, and whole blocks of 32 queries (every caller pads nq_pad to a multiple of 256)
    if (ci || nq_pad % 32 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL((bf16_pack_wide8_kernel<T, true>), dim3((unsigned)(nq_pad * 8 / 256)), dim3(256), 0, s, Q, mu, nq, nq_pad,
                       dim, ld, static_cast<uint16_t *>(B), qn, qbad, (uint32_t *)nullptr, sm);
    return hipGetLastError();
}
// Per-dimension power sums of the corpus translated by mu: out[j * dim + k] = sum over rows of (p_k - mu_k)^(j + 1),
// j = 0 .. 3, in f64 (the seed model's moments; zeroed by the caller).  Non-finite coordinates count as zero.
template <typename T>
__global__ void bf16_column_moments_kernel(const T *__restrict__ P, const float *__restrict__ mu, size_t n, int dim, size_t ld,
                                           double *__restrict__ out) {
    const size_t r0 = (size_t)blockIdx.x * 1024;
    const size_t r1 = r0 + 1024 < n ? r0 + 1024 : n;
    for (int k = threadIdx.x; k < dim; k += blockDim.x) {
        const double m = (double)mu[k];
        double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
        for (size_t r = r0; r < r1; ++r) {
            const double x = (double)P[r * ld + k];
            const double u = (fabs(x) < 1.0e30) ? x - m : 0.0;
            const double u2 = u * u;
            s1 += u;
            s2 += u2;
            s3 += u2 * u;
            s4 += u2 * u2;
        }
        atomicAdd(&out[k], s1);
        atomicAdd(&out[dim + k], s2);
        atomicAdd(&out[2 * dim + k], s3);
        atomicAdd(&out[3 * dim + k], s4);
    }
}
template <typename T>
hipError_t launch_bf16_column_moments(const T *P, const float *mu, size_t n, int dim, size_t ld, double *out, hipStream_t s) {
    hipLaunchKernelGGL(bf16_column_moments_kernel<T>, dim3((unsigned)((n + 1023) / 1024)), dim3(128), 0, s, P, mu, n, dim, ld, out);
    return hipGetLastError();
}
template hipError_t launch_bf16_column_moments<float>(const float *, const float *, size_t, int, size_t, double *, hipStream_t);
template hipError_t launch_bf16_column_moments<double>(const double *, const float *, size_t, int, size_t, double *, hipStream_t);

template hipError_t launch_bf16_pack_queries<float>(const float *, const float *, size_t, size_t, int, size_t, void *, double *,
                                                    uint32_t *, bool, double, double, hipStream_t, float *, size_t, uint32_t *,
                                                    const Bf16SeedModel *);
template hipError_t launch_bf16_pack_queries<double>(const double *, const float *, size_t, size_t, int, size_t, void *, double *,
                                                     uint32_t *, bool, double, double, hipStream_t, double *, size_t, uint32_t *,
                                                     const Bf16SeedModel *);

// ---- launchers of the filter kernels: they run what the descriptor (Bf16Launch, pn_internal.h) names or refuse it --
// which main-pass kernel serves a call is bf16_main_kernel's decision (bf16_launch.h), made by the plan in index.hip
static_assert(kBQ == (int)kBf16QueryTile && kBP == (int)kBf16RowTile && kWR == (int)kBf16WideTile, "bf16_launch.h");
// PN_DEBUG_PLAN: one line per main-pass launch of a k-NN call -- which kernel (4 / 8 / pair / pair2) and its grid
static void bf_debug_kernel(const char *which, unsigned grid, unsigned block) {
    if (debug_plan()) std::fprintf(stderr, "bf16 main pass: kernel %s grid %u x %u\n", which, grid, block);
}
template <auto Kern, typename... A>
static hipError_t bf_go(unsigned grid, unsigned block, size_t sh, hipStream_t s, A... args) {
    static LdsAttrOnce lds_attr;  // per instantiation
    const hipError_t e = lds_attr.ensure(reinterpret_cast<const void *>(Kern), sh);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kern, dim3(grid), dim3(block), sh, s, args...);
    return hipGetLastError();
}
// What both launchers ask of a descriptor: buffers that fit the grid, a grid that is bf16_grid's, and the pointers
// its pass needs -- no others.
static bool bf_launch_valid(const Bf16Launch &l, bool wide) {
    const CandBuf &cb = l.cb;
    const Bf16Grid &g = l.grid, w = bf16_grid(l.n, cb.nq_pad, g.n_wg, g.split, wide);
    if (!bf16_supported(l.dim) || bf16_is_wide(l.dim) != wide || cb.nq_pad % kBQ || l.kp < 1 || l.kp + 32 > cb.cap ||
        (cb.cap != 64 && cb.cap != 128 && cb.cap != 256) || cb.idx_stride != 2 ||
        cb.idx != static_cast<uint32_t *>(cb.keys) + 1 || g.n_wg < 1 || g.split < 1 || l.scout_tiles < 0)
        return false;
    if (g.q_tiles < 1 || g.q_tiles != w.q_tiles || g.n_tiles != w.n_tiles || g.aligned != w.aligned || g.nseg != w.nseg ||
        g.run_tiles != w.run_tiles || cb.nseg < g.nseg || (wide ? g.split != 1 : (uint32_t)g.split > g.n_tiles))
        return false;
    const bool thresholds = l.pass == Bf16Pass::Seeded || l.pass == Bf16Pass::Radius;
    if (thresholds != (l.tau != nullptr) || (l.pass == Bf16Pass::ScoutOnly) != (l.scout_out != nullptr)) return false;
    return l.pass != Bf16Pass::Radius || (cb.cap == 256 && !l.refresh);  // (fixed thresholds: nothing to share)
}
template <int KS, int M, bool RAD, bool CI>
static hipError_t launch_bf16_t(const Bf16Launch &l, hipStream_t s) {
    const CandBuf &cb = l.cb;
    const Bf16Grid &g = l.grid;
    const size_t sh = (size_t)3 * kBP * (2 * KS + 1) * 16 + 16;  // three tile buffers (software-pipelined main loop) + the arrival counter
    const uint32_t kp = (uint32_t)l.kp, split = (uint32_t)g.split, scout = (uint32_t)l.scout_tiles;
    const uint32_t kp_keep = kp | ((uint32_t)(M <= 2 && !RAD && cb.final_keep > (int)kp ? cb.final_keep : 0) << 16);
    const uint32_t spp = (uint32_t)bf16_touching((size_t)g.q_tiles * split, g.n_wg);  // segments per row part
    const unsigned n_wg = (unsigned)g.n_wg, n_all = n_wg + (unsigned)(l.refresh ? l.refresh->n_refresh : 0);
    BfShared a{};
    a.nseg = (uint32_t)cb.nseg;
    if (l.seed) {
        a.seed_lists = l.seed->lists;
        a.seed_rank = l.seed->rank;
        a.seed_nq = l.seed->nq;
        a.seed_words = l.seed->words;
    }
    if (l.refresh) {  // shared thresholds: refresher workgroups behind the n_wg main ones
        a.pcnt = l.refresh->pcnt;
        a.done = l.refresh->done;
        a.n_main = n_wg;
        a.epoch = l.refresh->epoch;
        a.rank = l.refresh->rank;
    }
    const char *img = static_cast<const char *>(l.img);
    const u32x4 *B = static_cast<const u32x4 *>(l.B);
    uint2 *keys = static_cast<uint2 *>(cb.keys);
    uint32_t *tau = static_cast<uint32_t *>(cb.tau);
    if constexpr (!RAD) {  // the kernels of the main pass alone
        if constexpr (M == 1)
            if (l.kernel == Bf16Kernel::Pair || l.kernel == Bf16Kernel::PairTwo) {
                const unsigned grid = (unsigned)(((g.q_tiles + 1u) / 2u) * (n_wg / g.q_tiles));
                if (l.kernel == Bf16Kernel::Pair) {
                    bf_debug_kernel("pair", grid, 512);
                    return bf_go<bf16_filter_kernel_pair<KS, CI>>(grid, 512, sh, s, img, g.n_tiles, B, g.q_tiles, kp_keep,
                                                                     keys, cb.cnt, tau, cb.nq_pad, l.tau, a);
                }
                // two tiles per meeting: a ring of 3 kPairMeet tile buffers (KS = 8: 104 448 B, KS = 9: 116 736 B of
                // the CU's 160 KiB -- bf_go raises the kernel's dynamic-LDS limit to it); one workgroup per CU as before
                const size_t sh2 = kPairMeet == 1 ? sh : (size_t)3 * kPairMeet * kBP * (2 * KS + 1) * 16;
                bf_debug_kernel("pair2", grid, 512);
                return bf_go<bf16_filter_kernel_meet_pair<KS, CI, kPairMeet>>(grid, 512, sh2, s, img, g.n_tiles, B, g.q_tiles,
                                                                         kp_keep, keys, cb.cnt, tau, cb.nq_pad, l.tau, a);
            }
        if (l.kernel == Bf16Kernel::Eight) {
            bf_debug_kernel("8", n_all, 512);
            return l.refresh ? bf_go<bf16_filter8_kernel<KS, CI, true, M>>(n_all, 512, sh, s, img, g.n_tiles, B, g.q_tiles, kp_keep,
                                                                          keys, cb.cnt, tau, cb.nq_pad, l.tau, a)
                             : bf_go<bf16_filter8_kernel<KS, CI, false, M>>(n_all, 512, sh, s, img, g.n_tiles, B, g.q_tiles, kp_keep,
                                                                           keys, cb.cnt, tau, cb.nq_pad, l.tau, a);
        }
        if constexpr (M <= 2)
            if (l.refresh) {
                bf_debug_kernel("4", n_all, 256);
                return bf_go<bf16_filter_kernel<KS, M, false, CI, 2, true>>(n_all, 256, sh, s, img, g.n_tiles, B, g.q_tiles, kp_keep,
                                                                           keys, cb.cnt, tau, cb.nq_pad, split, spp, scout, l.tau,
                                                                           l.scout_out, a);
            }
    }
#define PN_BF_LAUNCH_MODE(MD)                                                                                            \
    bf_go<bf16_filter_kernel<KS, M, RAD, CI, MD>>(n_wg, 256, sh, s, img, g.n_tiles, B, g.q_tiles, kp_keep, keys, cb.cnt, tau, \
                                                  cb.nq_pad, split, spp, scout, l.tau, l.scout_out, a)
    if (l.pass == Bf16Pass::ScoutOnly) return PN_BF_LAUNCH_MODE(1);
    if (l.pass != Bf16Pass::SelfScout) {
        if (!RAD) bf_debug_kernel("4", n_wg, 256);
        return PN_BF_LAUNCH_MODE(2);
    }
    return PN_BF_LAUNCH_MODE(0);
#undef PN_BF_LAUNCH_MODE
}

template <int KS, bool CI>
static hipError_t launch_bf16_m(const Bf16Launch &l, hipStream_t s) {
    if (l.pass == Bf16Pass::Radius) return launch_bf16_t<KS, 4, true, CI>(l, s);
    switch (l.cb.cap) {
        case 64: return launch_bf16_t<KS, 1, false, CI>(l, s);
        case 128: return launch_bf16_t<KS, 2, false, CI>(l, s);
        default: return launch_bf16_t<KS, 4, false, CI>(l, s);
    }
}

bool bf16_shared_supported(int cap) {
    return cap == 64 || cap == 128;
}
// cb: keys = (key, row) pairs [nseg][nq_pad][cap] (cb.idx = keys + 1, cb.idx_stride = 2), cap = bf16_cap_for(kp);
// cnt/tau PRE-INITIALISED to 0 / sortable(+inf) where the partition is not aligned
hipError_t launch_bf16_filter(const Bf16Launch &l, hipStream_t s) {
    const CandBuf &cb = l.cb;
    if (!bf_launch_valid(l, false) || (l.ci && !bf16_ci_dim(l.dim)) ||
        !bf16_kernel_applies(l.kernel, l.grid, cb.cap, l.pass, l.refresh.has_value()))
        return hipErrorInvalidValue;
    if (l.refresh) {  // shared thresholds need the main pass of an aligned partition (exactly nseg cells per query)
        const Bf16Refresh &r = *l.refresh;
        if (l.pass != Bf16Pass::Seeded || !l.grid.aligned || !bf16_shared_supported(cb.cap) || r.n_refresh < 1 ||
            r.epoch < 1 || r.epoch > 4095 || r.rank < 1 || !r.pcnt || !r.done)
            return hipErrorInvalidValue;
    }
    if (l.seed && (!l.seed->lists || l.seed->rank < 1 || l.seed->rank > (uint32_t)kScoutList || !bf16_seed_in_kernel(cb.nseg)))
        return hipErrorInvalidValue;
#define PN_BF_CASE(K, C) \
    case K: return launch_bf16_m<K, C>(l, s);
#ifdef PN_DEV_KS8_ONLY  // development builds: only the D = 128 CI instantiation (compiles in a fraction of the time)
    if (l.ci) {
        switch (bf16_ks_for(l.dim, true)) {
            PN_BF_CASE(8, true)
            default: return hipErrorInvalidValue;
        }
    }
    return hipErrorInvalidValue;
#else
    if (l.ci) {
        switch (bf16_ks_for(l.dim, true)) {
            PN_BF_CASE(2, true) PN_BF_CASE(3, true) PN_BF_CASE(4, true) PN_BF_CASE(5, true) PN_BF_CASE(6, true)
            PN_BF_CASE(7, true) PN_BF_CASE(8, true)
            default: return hipErrorInvalidValue;
        }
    }
    switch (bf16_ks_for(l.dim, false)) {
        PN_BF_CASE(2, false) PN_BF_CASE(3, false) PN_BF_CASE(4, false) PN_BF_CASE(5, false) PN_BF_CASE(6, false)
        PN_BF_CASE(7, false) PN_BF_CASE(8, false) PN_BF_CASE(9, false)
        default: return hipErrorInvalidValue;
    }
#endif
#undef PN_BF_CASE
}

// Shared scout (few queries, many segments per query): a scout-only launch leaves, per (segment, query) cell and
// lane half, the kScoutList smallest block minima of that segment's first tiles.  The rows scouted by ALL segments
// of a query form one sample of the corpus; its rank-th smallest bound is a far better starting threshold for every
// segment than each segment's own list could give (rank from the host: the sample holds Poisson(lambda) of the rows
// that matter, the seed must stay above them).  out[q] = sortable key just above that bound.  One wave per query.
__global__ __launch_bounds__(64) void bf16_seed_kernel(const float *__restrict__ lists, size_t nq_pad, int nseg,
                                                       uint32_t rank, uint32_t *__restrict__ out, size_t nq) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint32_t *sk = reinterpret_cast<uint32_t *>(smem_raw);
    const int lane = threadIdx.x;
    const size_t q = blockIdx.x;
    if (q >= nq) {  // a padding query of the last tile: nothing passes its threshold (-inf), so it costs no appends
        if (lane == 0) out[q] = f2s(__uint_as_float(0xFF800000u));
        return;
    }
    const uint32_t per = 2 * kScoutList, n = (uint32_t)nseg * per;
    uint32_t T = 0;
    if (n <= 512u) {  // up to eight words per lane, in registers: no LDS round trip per bit (C2: 288 values per query)
        uint32_t v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t e = (uint32_t)lane + 64u * (uint32_t)i;
            v[i] = e < n ? f2s(lists[((size_t)(e / per) * nq_pad + q) * per + e % per]) : 0xFFFFFFFFu;
        }
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cnd = T | (1u << bit);
            uint32_t c = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) c += (uint32_t)__popcll(__ballot(v[i] < cnd));
            if (c < rank) T = cnd;
        }
        if (lane == 0) out[q] = T == 0xFFFFFFFFu ? T : T + 1;
        return;
    }
    // Many segments (a handful of queries spread over every workgroup slot: 512 segments x 24 values): a radix select
    // over all n values in LDS is 32 x n/64 dependent LDS round trips -- 0.3 ms for ONE query's wave.  Instead: the
    // rank-th smallest of the 64 lanes' minima is an upper bound U of the answer (rank lanes hold a value at or below
    // it, rank <= 24 < 64); only the values at or below U -- a few times rank of them -- go to LDS and are selected from.
    // (every (segment, lane half) list is sorted ascending: its first entry is its minimum, and the entries at or below
    // U are a prefix -- a lane walks its lists' heads, 2 nseg / 64 loads, instead of all n values)
    const uint32_t n_lists = 2u * (uint32_t)nseg;
    auto list_at = [&](uint32_t li) { return lists + ((size_t)(li >> 1) * nq_pad + q) * per + (size_t)(li & 1u) * kScoutList; };
    uint32_t lmin = 0xFFFFFFFFu;
    for (uint32_t li = lane; li < n_lists; li += 64) {
        const uint32_t v = f2s(list_at(li)[0]);
        lmin = v < lmin ? v : lmin;
    }
    uint32_t U = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cnd = U | (1u << bit);
        if ((uint32_t)__popcll(__ballot(lmin < cnd)) < rank) U = cnd;
    }
    __shared__ uint32_t s_w;
    if (lane == 0) s_w = 0u;
    __syncthreads();
    const uint32_t cap_lds = (uint32_t)nseg * per;  // (the launch sized LDS for all n values)
    for (uint32_t li = lane; li < n_lists; li += 64) {
        const float *l = list_at(li);
        for (int i = 0; i < kScoutList; ++i) {
            const uint32_t v = f2s(l[i]);
            if (v > U) break;
            const uint32_t pos = atomicAdd(&s_w, 1u);
            if (pos < cap_lds) sk[pos] = v;
        }
    }
    __syncthreads();
    const uint32_t w = s_w;
    const uint32_t nn = w < cap_lds ? w : cap_lds;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cnd = T | (1u << bit);
        uint32_t c = 0;
        for (uint32_t e0 = 0; e0 < nn; e0 += 64) {
            const uint32_t e = e0 + lane;
            c += (uint32_t)__popcll(__ballot(e < nn && sk[e] < cnd));
        }
        if (c < rank) T = cnd;
    }
    if (lane == 0) out[q] = T == 0xFFFFFFFFu ? T : T + 1;  // rows with a bound EQUAL to it still pass the strict '<'
}

hipError_t launch_bf16_seed(const float *lists, size_t nq_pad, int nseg, int rank, uint32_t *out, hipStream_t s,
                            size_t nq) {
    const size_t sh = (size_t)nseg * 2 * kScoutList * sizeof(uint32_t);
    if (sh > 64 * 1024 || rank < 1 || (size_t)rank > (size_t)nseg * 2 * kScoutList) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf16_seed_kernel, dim3((unsigned)nq_pad), dim3(64), sh, s, lists, nq_pad, nseg, (uint32_t)rank,
                       out, nq ? nq : nq_pad);
    return hipGetLastError();
}
int bf16_scout_list() { return kScoutList; }
// the main launch derives its starting thresholds from the scout launch's lists itself when a lane can walk them all
bool bf16_seed_in_kernel(int nseg) { return nseg >= 1 && nseg <= 32; }

// radius queries: per-query threshold of the filter.  A row can only be within the radius when its exact squared
// distance is below tau_r (computed by the host with the rounding allowances of select.hip's proof), hence when
// L' < tau_r - |q|^2_down.  out[q] = sortable key of that bound, widened by a 2^-18 margin, rounded up to f32 and
// one step beyond (strict <).
__global__ void bf16_radius_tau_kernel(const double *__restrict__ qn, size_t nq_pad, double tau_r,
                                       uint32_t *__restrict__ out) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq_pad) return;
    // A margin of |t| 2^-18 on top of the rounding below (round 1's kernels compared bounds whose low four mantissa
    // bits carried a row tag; the margin was sized for that and is kept: it costs a handful of exact checks).
    double t = tau_r - qn[q];
    t += fabs(t) * 3.814697265625e-06;
    float f = (float)t;
    if ((double)f < t) f = nextafterf(f, __uint_as_float(0x7F800000u));
    f = nextafterf(f, __uint_as_float(0x7F800000u));
    out[q] = f2s(f);
}

hipError_t launch_bf16_radius_tau(const double *qn, size_t nq_pad, double tau_r, uint32_t *out, hipStream_t s) {
    hipLaunchKernelGGL(bf16_radius_tau_kernel, dim3((unsigned)((nq_pad + 255) / 256)), dim3(256), 0, s, qn, nq_pad, tau_r,
                       out);
    return hipGetLastError();
}

// debug / test entry: L'(q, p) for every pair of a small problem, straight from the MFMA (one wave per
// 32 x 32 block), so tests can check L' <= |q-p|^2 - |q|^2 against f64 and measure the accumulation error.
template <int KS, bool CI>
__global__ __launch_bounds__(64) void bf16_bound_kernel(const char *__restrict__ img, const u32x4 *__restrict__ Bq,
                                                        uint32_t n_rows, uint32_t nq, float *__restrict__ out) {
    constexpr int C = 2 * KS, CP = C + 1;
    const int lane = threadIdx.x, jq = lane & 31, h = lane >> 5;
    const uint32_t rb = blockIdx.x, qb = blockIdx.y;  // 32-row block, 32-query block
    const uint32_t row = rb * 32 + jq;
    const char *arow = img + ((size_t)(row / kBP) * kBP * CP + (size_t)(row % kBP) * CP + h) * 16;
    const u32x4 *br = Bq + ((size_t)qb * 32 + jq) * C + h;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    if (CI) acc = bf_cinit<CP>(img + (size_t)(rb * 32 / kBP) * kBP * CP * 16, (int)((rb * 32 % kBP) / 32), h);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const u32x4 av = *reinterpret_cast<const u32x4 *>(arow + 32 * ks);
        const u32x4 bv = br[2 * ks];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv),
                                                      acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t i = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const uint32_t q = qb * 32 + jq;
        if (i < n_rows && q < nq) out[(size_t)q * n_rows + i] = acc[r];
    }
}

__global__ void bf16_wide_bound_kernel(const char *__restrict__ img, const char *__restrict__ Bimg, uint32_t nkc,
                                       uint32_t tile_bytes, uint32_t has_x, uint32_t n_rows, uint32_t nq,
                                       float *__restrict__ out);
hipError_t launch_bf16_bound(const void *img, const void *B, size_t n_rows, size_t nq, int dim, float *out, bool ci,
                             hipStream_t s) {
    // img covers round_up(n_rows, 64) rows and B round_up(nq, 32) queries at least
    const dim3 grid((unsigned)((n_rows + 31) / 32), (unsigned)((nq + 31) / 32));
    const char *im = static_cast<const char *>(img);
    if (bf16_is_wide(dim)) {  // img covers round_up(n_rows, 256) rows, B round_up(nq, 256) queries
        if (!bf16_supported(dim) || ci) return hipErrorInvalidValue;
        hipLaunchKernelGGL(bf16_wide_bound_kernel, grid, dim3(64), 0, s, im, static_cast<const char *>(B),
                           (uint32_t)bf16_wide_nkc(dim), (uint32_t)bf16_wide_tile_bytes(dim),
                           bf16_wide_has_x(dim) ? 1u : 0u, (uint32_t)n_rows, (uint32_t)nq, out);
        return hipGetLastError();
    }
    const u32x4 *b = static_cast<const u32x4 *>(B);
#define PN_BOUND_CASE(K, C)                                                                                       \
    case K:                                                                                                       \
        hipLaunchKernelGGL((bf16_bound_kernel<K, C>), grid, dim3(64), 0, s, im, b, (uint32_t)n_rows, (uint32_t)nq, out); \
        break;
    if (ci) {
        switch (bf16_ks_for(dim, true)) {
            PN_BOUND_CASE(2, true) PN_BOUND_CASE(3, true) PN_BOUND_CASE(4, true) PN_BOUND_CASE(5, true)
            PN_BOUND_CASE(6, true) PN_BOUND_CASE(7, true) PN_BOUND_CASE(8, true)
            default: return hipErrorInvalidValue;
        }
    } else {
        switch (bf16_ks_for(dim, false)) {
            PN_BOUND_CASE(2, false) PN_BOUND_CASE(3, false) PN_BOUND_CASE(4, false) PN_BOUND_CASE(5, false)
            PN_BOUND_CASE(6, false) PN_BOUND_CASE(7, false) PN_BOUND_CASE(8, false) PN_BOUND_CASE(9, false)
            default: return hipErrorInvalidValue;
        }
    }
#undef PN_BOUND_CASE
    return hipGetLastError();
}

// ---- wide rows: launcher.  The kernel reads its pass off its arguments (l.tau, l.scout_out: bf_launch_valid ties
// them to l.pass); cells without a writer must read "empty" (cnt 0, tau +inf, lists +inf) unless the grid is aligned
template <int M, bool RAD>
static hipError_t launch_bf16_wide_t(const Bf16Launch &l, hipStream_t s) {
    const size_t sh = (size_t)2 * kWStage + 2 * kWXPiece;  // two stages + two extras pieces
    return bf_go<bf16_wide_kernel<M, RAD>>((unsigned)l.grid.n_wg, 512, sh, s, static_cast<const char *>(l.img), l.grid.n_tiles,
                                           static_cast<const char *>(l.B), (uint32_t)bf16_wide_nkc(l.dim),
                                           (uint32_t)bf16_wide_tile_bytes(l.dim), bf16_wide_has_x(l.dim) ? 1u : 0u,
                                           (uint32_t)l.kp, static_cast<uint2 *>(l.cb.keys), l.cb.cnt,
                                           static_cast<uint32_t *>(l.cb.tau), l.cb.nq_pad, (uint32_t)l.scout_tiles, l.tau,
                                           l.scout_out);
}
hipError_t launch_bf16_wide_filter(const Bf16Launch &l, hipStream_t s) {
    if (!bf_launch_valid(l, true) || l.kernel != Bf16Kernel::Wide || l.seed || l.refresh ||
        (unsigned long long)l.grid.n_wg > (unsigned long long)l.grid.q_tiles * l.grid.n_tiles)
        return hipErrorInvalidValue;
    if (l.pass == Bf16Pass::Radius) return launch_bf16_wide_t<4, true>(l, s);
    switch (l.cb.cap) {
        case 64: return launch_bf16_wide_t<1, false>(l, s);
        case 128: return launch_bf16_wide_t<2, false>(l, s);
        default: return launch_bf16_wide_t<4, false>(l, s);
    }
}

// debug / test entry for wide rows: the same MFMA chain, step by step in the kernel's order
__global__ __launch_bounds__(64) void bf16_wide_bound_kernel(const char *__restrict__ img, const char *__restrict__ Bimg,
                                                             uint32_t nkc, uint32_t tile_bytes, uint32_t has_x,
                                                             uint32_t n_rows, uint32_t nq, float *__restrict__ out) {
    const int lane = threadIdx.x, jq = lane & 31, h = lane >> 5;
    const uint32_t rb = blockIdx.x, qb = blockIdx.y;
    const size_t row = (size_t)rb * 32 + jq, q = (size_t)qb * 32 + jq;
    const char *pa = img + (row / kWR) * (size_t)tile_bytes, *pb = Bimg + (q / kWR) * (size_t)tile_bytes;
    const size_t ra = row % kWR, rq = q % kWR;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (uint32_t ks = 0; ks < 4 * nkc; ++ks) {  // the kernel's order: all steps of the data chunks, zero ones included
        const size_t c = ks >> 2;
        const unsigned slot = (unsigned)((ks & 3) * 2 + h);
        const u32x4 av = *reinterpret_cast<const u32x4 *>(pa + (c * kWR + ra) * kWPitch + (slot ^ bf_wide_swz(ra)) * 16);
        const u32x4 bv = *reinterpret_cast<const u32x4 *>(pb + (c * kWR + rq) * kWPitch + (slot ^ bf_wide_swz(rq)) * 16);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv),
                                                      acc, 0, 0, 0);
    }
    if (has_x) {  // then the extras step
        const u32x4 av = *reinterpret_cast<const u32x4 *>(pa + (size_t)nkc * kWPiece + ra * 32 +
                                                          ((unsigned)h ^ bf_wide_xswz(ra)) * 16);
        const u32x4 bv = *reinterpret_cast<const u32x4 *>(pb + (size_t)nkc * kWPiece + rq * 32 +
                                                          ((unsigned)h ^ bf_wide_xswz(rq)) * 16);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv),
                                                      acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t i = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const uint32_t qq = qb * 32 + jq;
        if (i < n_rows && qq < nq) out[(size_t)qq * n_rows + i] = acc[r];
    }
}

}  // namespace pn
