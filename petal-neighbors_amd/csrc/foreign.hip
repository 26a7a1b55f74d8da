// foreign.hip -- the first tier of the masked nearest-foreign-row scan (pn_nearest_foreign_*, the rounds of pn_mst_*): on
// Euclidean indexes and, below under "Cosine", on Cosine indexes.  For every listed row i the exact scan (exact_scan.hip, mst_scan_kernel) wants the
// least (key(w(i, j)), j) over the rows j of another group, w = max(d(i, j), core[i], core[j]) on the sortable keys, and
// pays 3 VALU operations per coordinate of every pair for it.  Here the matrix cores look at every pair first.
//
// Pack (once per call, km_pack.h): the rows are centred at the corpus mean mu and split into two bf16 images, x - mu =
// x^ + x~ + e; per row xn <= |x - mu|^2 and bounds of |x^|, |x~|, |e|; over all rows the maxima Ch, Cl, Ce, B of |x^|, |x~|,
// |e|, |x - mu|.  A distance does not see the translation, so any mu is sound; the mean makes the norms, and with them the
// slack, as small as a translation can.
//
// Filter (fr_filter_kernel): a self-join.  With S(i, j) the f32 MFMA accumulation of x^_j . x^_i + x^_j . x~_i + x~_j . x^_i
// (three MFMAs per 16 columns, one chain) kmeans.hip's bound reads, the partner j in the place of the centre,
//   L(i, j) = xn(i) + fl32(cn(j) - 2 S(i, j)) - E(i) <= |x_i - x_j|^2,     E(i) = km_row_slack of row i over the maxima.
// The reference's fold delivers s >= |x_i - x_j|^2 (1 - (D + 3) u) - D 2^-149 and d = rn(sqrt(s)), both
// monotone, so with a32 <= xn(i) - E(i) in f32 and
//   L' = fl32(fl32(a32 + key) * shrink - 1e-36),  shrink <= 1 - (D + 4) u - 2^-20   (the two roundings are inside 2^-20)
//   l  = v_sqrt_f32(L') * (1 - 2^-21)  (the instruction is within one ulp; 0 where L' < 1e-30)
// l <= d(i, j) as the fold computes it, in either element type.  In the key domain (K = the index's keys)
//   lifted(i, j) = max(key(l), ckey[i], ckey[j]) <= key(w(i, j)),
// because key() is monotone and the maximum is taken on the keys on both sides.  Per listed row the kernel keeps the M
// smallest (lifted, j) over the rows of other groups and tau = the (M + 1)-th smallest, in registers.
//
// Re-rank and proof (fr_rerank_kernel): the M candidates' edges in the reference's fold, best = the least (key(w), j) among
// them.  Every row j' that is no candidate has (key(w(i, j')), j') >= (lifted(i, j'), j') >= tau, and the row of tau is
// not the row of best: best <= tau (lexicographic) therefore proves best < every non-candidate, ties at equal keys
// included -- they are decided by j on both sides.  No strict slack is needed, and a row whose candidates all sit on the
// floor core[i] (a cored call is full of them) is proven as soon as one of them truly weighs core[i].  A row that is not
// proven -- or any row of a call in which some row is not finite or has a squared norm beyond 2^100 -- is listed for the
// exact scan, which answers it alone: results never depend on this tier.
//
// Cosine (COS instantiations; the candidates, tau, the proof in key order and the fallback are the ones above).  The rows
// are packed NORMALISED and not translated -- a translation changes angles -- by km_pack.h's NORM front: x- = x / |x| in
// f64, two bf16 images; no mean is summed.  Over the packed unit vectors the same chain and the same slack give
//   L(i, j) = xn(i) + fl32(cn(j) - 2 S(i, j)) - E(i) <= |x-_i - x-_j|^2,
// and every packed vector has norm 1 to rounding, so E(i) is about 2.9e-4 for every row (spherical_kmeans.hip).  With
// DESIGN.md 4.8's two inequalities (select.hip, cos_proof_lb; D = dim, u = 2^-24 | 2^-53 by the index's type)
//   | |x-_i - x-_j|^2 - 2 d* | <= eps1 = (4.5 D + 45) 2^-53,      | d_ref - d* | <= E' = (2 D + 16) u
// the distance the reference computes obeys d_ref(i, j) >= (L - eps1) / 2 - E'.  The kernel evaluates, per accumulator
// element and in f32, with a32 <= xn(i) - E(i) (fr_row_offset) and key = fl32(cn(j) - 2 S), so a32 + key <= L exactly,
//   t = fl32(a32 + key),      l = fmaf(t, 0.5, -c),      c >= eps1 / 2 + E' + 2^-21      (c folded on the host, rounded up)
// one add and one fused multiply-add, no square root.  The allowance 2^-21: |x^| <= 1 + 2^-8 and |x~| <= 2^-8 bound |S| by
// 1.02, cn <= 1 and -0.01 < a32 <= 1 give |a32 + key| < 4.1 and |t / 2 - c| < 2.1, so both results lie below 8 in magnitude,
// where a float's half ulp is at most 2^-22: t <= (a32 + key) + 2^-22, l <= (t / 2 - c) + 2^-22, together
//   l <= (a32 + key) / 2 - c + 2^-23 + 2^-22 < (L - eps1) / 2 - E' <= d_ref(i, j).
// l may be negative: its key is the signed order-preserving map of exact_scan.hip (dist_key_signed) -- of l for an f32
// index, of (double)l for an f64 one, an exact and hence monotone conversion.  l is never -0 (c > 0: a fused result is
// zero only when t / 2 = c exactly, and round-to-nearest makes that +0) and, for an unflagged call, never NaN.  So
//   lifted(i, j) = max(key(l), ckey[i], ckey[j]) <= key(w(i, j))
// as above.  Without cores ckey is (K)0 everywhere (mst.hip, fr_keys_kernel), which is the least key of the signed map too
// -- the key of the negative NaN of all bits set, below every number -- so the maximum leaves key(l) as it is.  The padding's
// cn is +inf and its core key kMax: never kept.  The re-rank evaluates a candidate by the reference's Cosine::distance
// in T -- the sequential unfused dot, 1 - dot / (norm_i * norm_j) with the index's own row norms, the expression and the
// operands of mst_scan_kernel, so both paths deliver the same bits -- on the signed keys.  A call with a flagged row (not
// finite, or a squared norm outside [2^-100, 2^100]: a zero row) goes to the exact scan as a whole, as above: such a row
// is a partner of every other row and its reference distance need not be NaN.
//
// Layout of the filter.  A workgroup of 4 waves holds 128 listed rows, gathered through the list: their two images lie in
// LDS ([2][128][dp + 8]) and are the B operands of v_mfma_f32_32x32x16_bf16; wave w owns rows 32 w .. 32 w + 31, the ROW on
// the lane (lane & 31), 16 partners in the lane's accumulator.  Every row of the index streams past as the A operand in
// stages of 32 SUB rows (SUB = 4, 2, 1 by the row width): a stage is read from HBM once per workgroup into registers while
// the previous stage is contracted, stored to the other of two LDS buffers, and shared by the four waves.  With it travel
// the stage's meta data -- cn, the group code and the core key of its rows -- in three small buffers, because the register
// scan of a tile runs one tile late: the MFMA chain of tile t + 1 is issued before the accumulator of tile t is scanned, so
// the VALU works while the matrix core does.  One barrier per stage.  K runs over the whole padded row in one chain: dp <=
// 160 keeps it at 30 MFMAs (the allowance g = 2^-13 is checked up to 65, pn_bf16_selftest) and the LDS at 130,560 bytes.
// The stream is cut into segments (grid.y) so that a short list still fills the device; the segments' lists are merged by
// the re-rank kernel.  Keys are integers and every reduction is a minimum of (key, j); the corpus mean is summed in a
// fixed shape (blocks of 4096 rows in row order, the blocks in order; Euclidean only): no floating-point atomics anywhere, so the images,
// the lists and the counters of pn_stats depend on the data alone.
//
// This translation unit is compiled with -ffp-contract=off: every operation outside the MFMA is plain IEEE, unfused, and
// the one fused multiply-add of the bound is written as such.
#include "../../include/petal_mi355x.h"
#include "pn_internal.h"
#include "km_filter.h"  // the packing and E(x), the MFMA chain, the gathered row tile, the fold's sqrt and key

namespace pn {

namespace {

// M = 3 candidates per row: with it the measured MST calls (10^5 and 10^6 rows of 16 columns, 10^5 of 128, uniform and
// blobs, with and without cores) leave 0 to 0.47 % of their listed rows to the exact scan, at three folds
// per row.  At
// that rate the exact scan's share of a call is already small, so no other M was measured; the list costs 3 (M + 1)
// registers per lane in f64 and the kernel has room (152 of 256).
constexpr int kFrM = 3, kFrM1 = kFrM + 1;
constexpr int kFrRows = 128;    // listed rows per workgroup
constexpr int kFrMaxDp = 160;   // the widest padded row: 30 MFMAs per chain, 130,560 bytes of LDS
constexpr int kFrPrefetch = 6;  // 16-byte chunks a thread carries from HBM to LDS per stage, at most
constexpr uint32_t kFrNoRow = 0xFFFFFFFFu;
constexpr size_t kFrMaxLds = 131072;

__host__ __device__ inline int fr_sub(int dp) { return dp <= 48 ? 4 : dp <= 96 ? 2 : 1; }  // 8 SUB dp <= 256 kFrPrefetch

template <typename K> __device__ __forceinline__ K fr_key_of_f32(float l);  // key of a finite l >= +0
template <> __device__ __forceinline__ uint32_t fr_key_of_f32<uint32_t>(float l) { return __float_as_uint(l); }
template <> __device__ __forceinline__ uint64_t fr_key_of_f32<uint64_t>(float l) {
    return (uint64_t)__double_as_longlong((double)l);
}
// Cosine: the signed key (exact_scan.hip, dist_key_signed) of a float l that is neither -0 nor NaN, and of a distance in T
template <typename K> __device__ __forceinline__ K fr_signed_key_of_f32(float l);
template <> __device__ __forceinline__ uint32_t fr_signed_key_of_f32<uint32_t>(float l) {
    const uint32_t b = __float_as_uint(l);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);  // (negative: every bit; else: the sign bit)
}
template <> __device__ __forceinline__ uint64_t fr_signed_key_of_f32<uint64_t>(float l) {
    const uint64_t b = (uint64_t)__double_as_longlong((double)l);
    return b ^ ((uint64_t)((int64_t)b >> 63) | 0x8000000000000000ull);
}
__device__ __forceinline__ uint32_t fr_signed_key(float d) {
    return d != d ? 0xFFC00000u : fr_signed_key_of_f32<uint32_t>(d == 0.0f ? 0.0f : d);
}
__device__ __forceinline__ uint64_t fr_signed_key(double d) {
    if (d != d) return 0xFFF8000000000000ull;
    const uint64_t b = (uint64_t)__double_as_longlong(d == 0.0 ? 0.0 : d);
    return b ^ ((uint64_t)((int64_t)b >> 63) | 0x8000000000000000ull);
}
template <typename K>
__device__ __forceinline__ bool fr_before(K ka, uint32_t ja, K kb, uint32_t jb) {
    return ka < kb || (ka == kb && ja < jb);
}
// (k, j) into the ascending list lk / lj [kFrM1], which it is known to precede the last entry of
template <typename K>
__device__ __forceinline__ void fr_insert(K (&lk)[kFrM1], uint32_t (&lj)[kFrM1], K k, uint32_t j) {
    lk[kFrM] = k;
    lj[kFrM] = j;
#pragma unroll
    for (int p = kFrM; p > 0; --p) {
        if (fr_before<K>(lk[p], lj[p], lk[p - 1], lj[p - 1])) {
            const K tk = lk[p];
            const uint32_t tj = lj[p];
            lk[p] = lk[p - 1];
            lj[p] = lj[p - 1];
            lk[p - 1] = tk;
            lj[p - 1] = tj;
        }
    }
}

// the corpus mean in a fixed shape: sums[b][k] <- column k over rows 4096 b .. in row order; mu[k] <- the blocks in order / n
constexpr size_t kFrSumRows = 4096;
template <typename T>
__global__ __launch_bounds__(256) void fr_colsum_kernel(const T *__restrict__ X, size_t n, size_t ld, int dim,
                                                        double *__restrict__ sums) {
    const int k = threadIdx.x;
    if (k >= dim) return;
    const size_t r0 = (size_t)blockIdx.x * kFrSumRows, r1 = r0 + kFrSumRows < n ? r0 + kFrSumRows : n;
    double s = 0.0;
    for (size_t r = r0; r < r1; ++r) s = s + (double)X[r * ld + k];
    sums[(size_t)blockIdx.x * dim + k] = s;
}
__global__ void fr_mean_kernel(const double *__restrict__ sums, size_t nblk, size_t n, int dim, float *__restrict__ mu) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= dim) return;
    double s = 0.0;
    for (size_t b = 0; b < nblk; ++b) s = s + sums[b * dim + k];
    const float m = (float)(s / (double)n);
    mu[k] = fabsf(m) < 1.0e30f ? m : 0.0f;  // (NaN, inf: the rows are flagged by the packing anyway)
}

// a32 <= xn - E in f32 (NaN for a flagged row: nothing of it is kept, and the re-rank lists it)
__device__ __forceinline__ float fr_row_offset(double xn, double xh, double xl, double xe,
                                               const unsigned long long *__restrict__ cc) {
    const double a = xn - km_row_slack(xh, xl, xe, cc);
    const float f = (float)(a - fabs(a) * 1.0e-15);
    return f - fabsf(f) * 2.4e-7f - 1.0e-37f;  // (two ulps below the nearest float: below a)
}

template <typename K>
struct FrMeta {  // a stage's rows: |x - mu|^2 rounded down (+inf: padding), group code, core key (kMax: padding)
    float *cn;
    uint32_t *comp;
    K *ck;
};

// grid (listed-row tiles, segments), 256 threads.  seg_key / seg_j [seg][nq_pad][kFrM1]
// fc: the constant of the bound folded on the host -- `shrink` (Euclidean), -c (COS); the metric enters in scan() alone
template <typename K, bool COS>
__global__ __launch_bounds__(256) void fr_filter_kernel(
    const uint16_t *__restrict__ img, const uint16_t *__restrict__ lo, const float *__restrict__ cn, size_t n, int dp,
    const uint32_t *__restrict__ list, int nq, size_t n_stages, size_t seg_stages, const uint32_t *__restrict__ comp,
    const K *__restrict__ ckey, const double *__restrict__ xn, const float *__restrict__ xh, const float *__restrict__ xl,
    const float *__restrict__ xe, const unsigned long long *__restrict__ cc, float fc, K *__restrict__ seg_key,
    uint32_t *__restrict__ seg_j, size_t nq_pad) {
    constexpr K KMAX = ~(K)0;
    extern __shared__ __align__(16) unsigned char fr_smem[];
    const int pitch = dp + 8, chunks = dp >> 3, ksteps = dp >> 4, sub = fr_sub(dp), srows = 32 * sub;
    uint16_t *btile = (uint16_t *)fr_smem, *btile_lo = btile + (size_t)kFrRows * pitch;
    uint16_t *abuf = btile_lo + (size_t)kFrRows * pitch;  // [2 buffers][2 images][srows][pitch]
    unsigned char *mbase = (unsigned char *)(abuf + (size_t)4 * srows * pitch);
    const size_t mbytes = (size_t)srows * (8 + sizeof(K));
    auto meta_at = [&](int b) {
        FrMeta<K> m;
        m.ck = (K *)(mbase + (size_t)b * mbytes);  // (8-byte aligned: every part before it is a multiple of 16 bytes)
        m.cn = (float *)(m.ck + srows);
        m.comp = (uint32_t *)(m.cn + srows);
        return m;
    };
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 31, h = lane >> 5;
    const size_t pos0 = (size_t)blockIdx.x * kFrRows;
    const size_t st_begin = (size_t)blockIdx.y * seg_stages;
    const size_t st_end = st_begin + seg_stages < n_stages ? st_begin + seg_stages : n_stages;

    // ---- the listed rows' images, gathered through the list (positions at and beyond nq: zeros)
    km_gather_row_tile<256>(btile, btile_lo, img, lo, list, pos0, (size_t)nq, kFrRows, dp, t);
    // ---- this lane's row
    const size_t my_pos = pos0 + (size_t)(w * 32 + r);
    const bool mine = my_pos < (size_t)nq;
    uint32_t comp_i = 0;
    K ck_i = KMAX;  // (no row: every lifted key is kMax, nothing is kept)
    float a32 = 0.0f;
    if (mine) {
        const size_t i = list[my_pos];
        comp_i = comp[i];
        ck_i = ckey[i];
        a32 = fr_row_offset(xn[i], (double)xh[i], (double)xl[i], (double)xe[i], cc);
        if (a32 != a32) ck_i = KMAX;
    }
    K lk[kFrM1];
    uint32_t lj[kFrM1];
#pragma unroll
    for (int e = 0; e < kFrM1; ++e) {
        lk[e] = KMAX;
        lj[e] = kFrNoRow;
    }

    // ---- the stream.  Stage s lies in data buffer s & 1 and meta buffer s % 3.
    const int per_img = srows * chunks, total = 2 * per_img;  // 16-byte chunks of a stage
    u32x4 pf[kFrPrefetch];
    float pm_cn = 0.0f;
    uint32_t pm_comp = 0;
    K pm_ck = KMAX;
    auto fetch = [&](size_t stage) {  // HBM -> registers
        const size_t row0 = stage * (size_t)srows;
#pragma unroll
        for (int e = 0; e < kFrPrefetch; ++e) {
            const int q = t + 256 * e;
            if (q < total) {
                const int im = q >= per_img ? 1 : 0, rem = q - im * per_img, rr = rem / chunks, ch = rem - rr * chunks;
                const size_t src = (row0 + (size_t)rr) * (size_t)dp + (size_t)ch * 8;  // (row0 + rr < n_img)
                pf[e] = *(const u32x4 *)((im ? lo : img) + src);
            }
        }
        if (t < srows) {
            const size_t j = row0 + (size_t)t;
            pm_cn = cn[j];  // (j < n_img)
            pm_comp = j < n ? comp[j] : 0u;
            pm_ck = j < n ? ckey[j] : KMAX;
        }
    };
    auto store = [&](size_t stage) {  // registers -> LDS
        uint16_t *dst = abuf + (size_t)(stage & 1) * 2 * srows * pitch;
#pragma unroll
        for (int e = 0; e < kFrPrefetch; ++e) {
            const int q = t + 256 * e;
            if (q < total) {
                const int im = q >= per_img ? 1 : 0, rem = q - im * per_img, rr = rem / chunks, ch = rem - rr * chunks;
                *(u32x4 *)(dst + ((size_t)im * srows + rr) * pitch + ch * 8) = pf[e];
            }
        }
        if (t < srows) {
            const FrMeta<K> m = meta_at((int)(stage % 3));
            m.cn[t] = pm_cn;
            m.comp[t] = pm_comp;
            m.ck[t] = pm_ck;
        }
    };
    const uint16_t *brow = btile + (size_t)(w * 32 + r) * pitch + h * 8;
    const uint16_t *brow_lo = btile_lo + (size_t)(w * 32 + r) * pitch + h * 8;
    auto chain = [&](size_t stage, int v) {
        const uint16_t *a0 = abuf + (size_t)(stage & 1) * 2 * srows * pitch + (size_t)(v * 32 + r) * pitch + h * 8;
        return km_mfma_chain(a0, a0 + (size_t)srows * pitch, brow, brow_lo, ksteps);
    };
    // registers 4 g .. 4 g + 3 of the accumulator are the tile's rows 8 g + 4 h + 0 .. 3 (km_mfma_chain): a lane meets its
    // partners in ascending j, so a strict '<' on the key keeps the smaller j among equal keys
    auto scan = [&](const f32x16 &acc, size_t stage, int v) {
        const FrMeta<K> m = meta_at((int)(stage % 3));
        const size_t j0 = stage * (size_t)srows + (size_t)(v * 32);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int a = v * 32 + 8 * g + 4 * h + jj;
                const float key = m.cn[a] - 2.0f * acc[4 * g + jj];
                K lifted;
                if constexpr (COS) {
                    lifted = fr_signed_key_of_f32<K>(__builtin_fmaf(a32 + key, 0.5f, fc));
                } else {
                    const float lp = __builtin_fmaf(a32 + key, fc, -1.0e-36f);
                    const float l = lp > 1.0e-30f ? __builtin_amdgcn_sqrtf(lp) * 0.99999952f : 0.0f;
                    lifted = fr_key_of_f32<K>(l);
                }
                const K cj = m.ck[a];
                lifted = lifted > ck_i ? lifted : ck_i;
                lifted = lifted > cj ? lifted : cj;
                if (lifted < lk[kFrM] && m.comp[a] != comp_i) fr_insert<K>(lk, lj, lifted, (uint32_t)(j0 + (size_t)(8 * g + 4 * h + jj)));
            }
        }
    };

    if (st_begin < st_end) {
        fetch(st_begin);
        store(st_begin);
    }
    f32x16 acc_prev;
    size_t prev_stage = 0;
    int prev_v = -1;  // (-1: no tile waits for its scan)
    for (size_t s = st_begin; s < st_end; ++s) {
        __syncthreads();  // stage s is in LDS; the buffers stage s + 1 goes to are no longer read (its meta: see above)
        if (s + 1 < st_end) fetch(s + 1);
        for (int v = 0; v < sub; ++v) {
            const f32x16 acc = chain(s, v);
            if (prev_v >= 0) scan(acc_prev, prev_stage, prev_v);
            acc_prev = acc;
            prev_stage = s;
            prev_v = v;
        }
        if (s + 1 < st_end) store(s + 1);
    }
    if (prev_v >= 0) scan(acc_prev, prev_stage, prev_v);

    // ---- the other half of the row's partners: the lane 32 away
    K ok[kFrM1];
    uint32_t oj[kFrM1];
#pragma unroll
    for (int e = 0; e < kFrM1; ++e) {
        ok[e] = __shfl_xor(lk[e], 32, 64);
        oj[e] = (uint32_t)__shfl_xor((int)lj[e], 32, 64);
    }
#pragma unroll
    for (int e = 0; e < kFrM1; ++e)
        if (fr_before<K>(ok[e], oj[e], lk[kFrM], lj[kFrM])) fr_insert<K>(lk, lj, ok[e], oj[e]);
    if (h == 0) {  // (positions beyond nq: empty lists, inside the padded row of the buffers)
        const size_t o = ((size_t)blockIdx.y * nq_pad + my_pos) * kFrM1;
#pragma unroll
        for (int e = 0; e < kFrM1; ++e) {
            seg_key[o + e] = lk[e];
            seg_j[o + e] = lj[e];
        }
    }
}

// ---- merge of the segments' lists, re-rank and proof: one thread per listed row.  ctr[0]: the rows listed for the exact
// scan (sel[slot]), ctr[1]: the candidates evaluated.  COS: the edge is Cosine::distance with the index's row norms
// cnorm [n] on the signed keys (mst_scan_kernel's expression: the same bits); else cnorm is not read.
template <typename T, bool COS>
__global__ __launch_bounds__(64) void fr_rerank_kernel(const T *__restrict__ X, size_t ld, int dim,
                                                       const uint32_t *__restrict__ list, size_t nq, size_t nq_pad, int nseg,
                                                       const typename KeyOf<T>::type *__restrict__ seg_key,
                                                       const uint32_t *__restrict__ seg_j,
                                                       const typename KeyOf<T>::type *__restrict__ ckey,
                                                       const double *__restrict__ xn,
                                                       const unsigned long long *__restrict__ cc,
                                                       typename KeyOf<T>::type *__restrict__ cand_key,
                                                       uint32_t *__restrict__ cand_j, uint32_t *__restrict__ sel,
                                                       uint32_t *__restrict__ ctr, const T *__restrict__ cnorm) {
#pragma clang fp contract(off)
    using K = typename KeyOf<T>::type;
    constexpr K KMAX = KeyOf<T>::kMax;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t evaluated = 0;
    if (p < nq) {
        const size_t i = list[p];
        K lk[kFrM1];
        uint32_t lj[kFrM1];
#pragma unroll
        for (int e = 0; e < kFrM1; ++e) {
            lk[e] = seg_key[p * kFrM1 + e];
            lj[e] = seg_j[p * kFrM1 + e];
        }
        for (int sg = 1; sg < nseg; ++sg) {
            const size_t o = ((size_t)sg * nq_pad + p) * kFrM1;
            for (int e = 0; e < kFrM1; ++e) {  // (a segment's list ascends: the first entry that fails ends it)
                const K k = seg_key[o + e];
                const uint32_t j = seg_j[o + e];
                if (!fr_before<K>(k, j, lk[kFrM], lj[kFrM])) break;
                fr_insert<K>(lk, lj, k, j);
            }
        }
        const double xni = xn[i];
        bool ok = cc[4] == 0 && xni == xni;
        K bk = KMAX;
        uint32_t bj = kFrNoRow;
        if (ok) {
            const T *xi = X + i * ld;
            const K ci = ckey[i];
            T ni = (T)0;
            if constexpr (COS) ni = cnorm[i];
#pragma unroll
            for (int e = 0; e < kFrM; ++e) {
                const uint32_t j = lj[e];
                if (j == kFrNoRow) break;
                const T *xj = X + (size_t)j * ld;
                T sum = (T)0;
                K kk;
                if constexpr (COS) {
                    for (int k = 0; k < dim; ++k) {
                        const T pr = xi[k] * xj[k];
                        sum = sum + pr;
                    }
                    const T den = ni * cnorm[j];
                    kk = fr_signed_key((T)1 - sum / den);
                } else {
                    for (int k = 0; k < dim; ++k) {
                        const T diff = xi[k] - xj[k];
                        const T sq = diff * diff;
                        sum = sum + sq;
                    }
                    kk = km_dist_key<T>(km_sqrt<T>(sum));
                }
                const K cj = ckey[j];
                kk = kk > ci ? kk : ci;
                kk = kk > cj ? kk : cj;
                if (fr_before<K>(kk, j, bk, bj)) {
                    bk = kk;
                    bj = j;
                }
                ++evaluated;
            }
            // (no entry at all: tau is (kMax, none) and so is best -- the row has no foreign row, proven)
            ok = !fr_before<K>(lk[kFrM], lj[kFrM], bk, bj);
        }
        if (ok) {
            cand_key[i] = bk;
            cand_j[i] = bj;
        } else {
            sel[atomicAdd(ctr, 1u)] = (uint32_t)i;  // (slot < nq: a position is listed at most once)
        }
    }
    for (int o = 32; o > 0; o >>= 1) evaluated += (uint32_t)__shfl_xor((int)evaluated, o, 64);
    if (threadIdx.x == 0 && evaluated) atomicAdd(ctr + 1, evaluated);
}

// the most (listed-row tile, segment) cells a launch makes for nq listed rows, and its plan
struct FrPlan {
    size_t qt, nseg, seg_stages, n_stages;
};
FrPlan fr_plan(size_t n, int dp, size_t nq, int n_cu) {
    FrPlan p;
    p.qt = (nq + kFrRows - 1) / kFrRows;
    const size_t srows = (size_t)32 * fr_sub(dp), target = (size_t)4 * (size_t)n_cu;
    p.n_stages = (n + srows - 1) / srows;
    size_t nseg = target / (p.qt ? p.qt : 1);
    nseg = nseg < 1 ? 1 : (nseg > p.n_stages ? p.n_stages : nseg);
    p.seg_stages = (p.n_stages + nseg - 1) / nseg;
    p.nseg = (p.n_stages + p.seg_stages - 1) / p.seg_stages;
    return p;
}
size_t fr_sum_blocks(size_t n) { return (n + kFrSumRows - 1) / kFrSumRows; }
size_t fr_seg_entries(size_t batch, int n_cu) {
    const size_t qt = (batch + kFrRows - 1) / kFrRows, target = (size_t)4 * (size_t)n_cu;
    return (qt > target ? qt : target) * kFrRows * kFrM1;
}

}  // namespace

bool foreign_filter_supported(int dim) { return dim >= 8 && (dim + 15) / 16 * 16 <= kFrMaxDp; }

// xn [n4] (8 bytes) | seg_key [seg_entries] (elem_bytes) | cc [8], sums [ceil(n / 4096)][dim] (8) | xh, xl, xe [n4], cn [n_img], mu
// [dp], seg_j [seg_entries], sel [batch], ctr [4] (4 bytes) | img, lo [n_img][dp] (2 bytes), every part 16-byte aligned
size_t foreign_tier_bytes(size_t n, int dim, int elem_bytes, size_t batch, int n_cu) {
    const size_t dp = (size_t)(dim + 15) / 16 * 16, n_img = round_up(n, (size_t)kFrRows), n4 = round_up(n, (size_t)4);
    const size_t se = fr_seg_entries(batch, n_cu);
    return n4 * 8 + round_up(se * (size_t)elem_bytes, (size_t)16) + round_up((8 + fr_sum_blocks(n) * (size_t)dim) * 8, (size_t)16) +
           (3 * n4 + n_img + dp + se + round_up(batch, (size_t)4) + 4) * 4 + 2 * n_img * dp * 2;
}
void foreign_tier_at(void *buf, size_t n, int dim, int elem_bytes, size_t batch, int n_cu, ForeignTier *t) {
    const size_t dp = (size_t)(dim + 15) / 16 * 16, n_img = round_up(n, (size_t)kFrRows), n4 = round_up(n, (size_t)4);
    const size_t se = fr_seg_entries(batch, n_cu);
    char *b = (char *)buf;
    t->xn = (double *)b;
    b += n4 * 8;
    t->seg_key = b;
    b += round_up(se * (size_t)elem_bytes, (size_t)16);
    t->cc = (unsigned long long *)b;
    t->sums = (double *)(t->cc + 8);
    b += round_up((8 + fr_sum_blocks(n) * (size_t)dim) * 8, (size_t)16);
    t->xh = (float *)b;
    t->xl = t->xh + n4;
    t->xe = t->xl + n4;
    t->cn = t->xe + n4;
    t->mu = t->cn + n_img;
    t->seg_j = (uint32_t *)(t->mu + dp);
    t->sel = t->seg_j + se;
    t->ctr = t->sel + round_up(batch, (size_t)4);
    t->img = (uint16_t *)(t->ctr + 4);
    t->lo = t->img + n_img * dp;
    t->n_img = n_img;
    t->dp = (int)dp;
    t->seg_entries = se;
    t->n_cu = n_cu;
}

template <typename T>
hipError_t foreign_pack(const ForeignTier &t, const T *X, size_t n, size_t ld, int dim, bool cosine, hipStream_t s) {
    // (kernels, not memsets: the words are cleared in stream order whatever the caller's stream is captured into)
    const size_t nblk = fr_sum_blocks(n);
    km_zero_words(t.cc, 8, s);
    if (cosine) {  // normalised, not translated: no mean (t.mu and t.sums stay unused)
        hipLaunchKernelGGL((km_pack_kernel<T, true, true>), dim3((unsigned)((t.n_img + 3) / 4)), dim3(256), 0, s, X, n, t.n_img,
                           ld, dim, t.dp, t.img, t.lo, t.xn, t.xh, t.xl, t.xe, t.cn, t.cc, (const float *)nullptr);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((fr_colsum_kernel<T>), dim3((unsigned)nblk), dim3(256), 0, s, X, n, ld, dim, t.sums);
    hipLaunchKernelGGL(fr_mean_kernel, dim3((unsigned)((dim + 63) / 64)), dim3(64), 0, s, t.sums, nblk, n, dim, t.mu);
    hipLaunchKernelGGL((km_pack_kernel<T, true>), dim3((unsigned)((t.n_img + 3) / 4)), dim3(256), 0, s, X, n, t.n_img, ld, dim,
                       t.dp, t.img, t.lo, t.xn, t.xh, t.xl, t.xe, t.cn, t.cc, (const float *)t.mu);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_foreign_filter(const ForeignTier &t, const T *X, size_t n, size_t ld, int dim, const uint32_t *list,
                                 size_t nq, const uint32_t *comp, const typename KeyOf<T>::type *ckey, const T *cnorm,
                                 typename KeyOf<T>::type *cand_key, uint32_t *cand_j, hipStream_t s) {
    using K = typename KeyOf<T>::type;
    if (nq == 0) return hipSuccess;
    const FrPlan p = fr_plan(n, t.dp, nq, t.n_cu);
    const size_t nq_pad = p.qt * kFrRows;
    if (p.nseg * nq_pad * kFrM1 > t.seg_entries) return hipErrorInvalidValue;
    const int sub = fr_sub(t.dp), srows = 32 * sub, pitch = t.dp + 8;
    const size_t lds = ((size_t)2 * kFrRows + (size_t)4 * srows) * pitch * 2 + (size_t)3 * srows * (8 + sizeof(K));
    const double u = sizeof(T) == 4 ? 5.9604644775390625e-08 : 1.1102230246251565e-16;
    km_zero_words(t.ctr, 2, s);
    auto run = [&](auto cos, float fc) -> hipError_t {  // (one instantiation, and one LDS attribute, per metric)
        constexpr bool COS = decltype(cos)::value;
        static LdsAttrOnce once;
        if (lds > 64 * 1024) {
            const hipError_t e = once.ensure((const void *)fr_filter_kernel<K, COS>, kFrMaxLds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL((fr_filter_kernel<K, COS>), dim3((unsigned)p.qt, (unsigned)p.nseg), dim3(256), lds, s, t.img, t.lo,
                           t.cn, n, t.dp, list, (int)nq, p.n_stages, p.seg_stages, comp, ckey, t.xn, t.xh, t.xl, t.xe, t.cc, fc,
                           (K *)t.seg_key, t.seg_j, nq_pad);
        hipLaunchKernelGGL((fr_rerank_kernel<T, COS>), dim3((unsigned)((nq + 63) / 64)), dim3(64), 0, s, X, ld, dim, list, nq,
                           nq_pad, (int)p.nseg, (const K *)t.seg_key, t.seg_j, ckey, t.xn, t.cc, cand_key, cand_j, t.sel, t.ctr,
                           cnorm);
        return hipGetLastError();
    };
    if (cnorm) {  // -c of the header: c >= eps1 / 2 + E' + 2^-21, and the conversion to float rounds it up
        const double c = 0.5 * (4.5 * (double)dim + 45.0) * 1.1102230246251565e-16 + (2.0 * (double)dim + 16.0) * u +
                         4.76837158203125e-07;
        return run(std::true_type{}, -(float)(c * (1.0 + 2.4e-7)));
    }
    return run(std::false_type{}, (float)(1.0 - (double)(dim + 4) * u - 1.0e-6));
}

#define PN_FR_INSTANTIATE(T)                                                                                          \
    template hipError_t foreign_pack<T>(const ForeignTier &, const T *, size_t, size_t, int, bool, hipStream_t);      \
    template hipError_t launch_foreign_filter<T>(const ForeignTier &, const T *, size_t, size_t, int, const uint32_t *, \
                                                 size_t, const uint32_t *, const KeyOf<T>::type *, const T *,          \
                                                 KeyOf<T>::type *, uint32_t *, hipStream_t);
PN_FR_INSTANTIATE(float)
PN_FR_INSTANTIATE(double)
#undef PN_FR_INSTANTIATE

}  // namespace pn
