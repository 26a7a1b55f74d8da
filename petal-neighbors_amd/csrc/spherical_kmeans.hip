// spherical_kmeans.hip -- spherical k-means on Cosine indexes (pn_spherical_kmeans_*, pn_spherical_kmeans_assign_*): the
// assignment of every indexed row to the centre of the least Cosine::distance behind a bf16 MFMA filter, and the update of
// the centres as normalised sums of their members' directions in a fixed shape.  The contract is in the header
// (petal_mi355x.h) and DESIGN.md 4.28.
//
// Distance.  d(i, c) = the reference's Cosine::distance (src/distance.rs:86-107) in T: dot = the sequential unfused fold of
// x_k c_k, den = norm_c * norm_row (each norm the correctly rounded sqrt of its own sequential fold; the rows' come from the
// index, the centres' are folded once per assignment), d = 1 - dot / den.  Products and the denominator commute exactly:
// the value does not depend on the order of the arguments.  Keys are the signed order-preserving map of DESIGN.md 4.8.
//
// Bound.  Rows and centres are packed NORMALISED in f64 (km_pack.h, NORM): x- = x / |x|, c- = c / |c|, each split into two
// bf16 images.  kmeans.hip's bound over those vectors,
//   L(x, c) = xn(x) + fl32(cn(c) - 2 S(x, c)) - E(x) <= |x- - c-|^2,
// is a bound of 2 (1 - cos) = twice the real Cosine distance d*.  Every packed vector has norm 1 to rounding, so the maxima
// Ch, Cl, Ce, B over the centres that E(x) is made of are those of EVERY centre: E(x) is about 2^-12 for every row and no
// far-away or long centre inflates it, as one does in the Euclidean filter.  The filter keeps per row the centre of the
// smallest key and tau = the second smallest key: every other centre has |x- - c-|^2 >= tau' = xn + tau - E.  With
//   | |x- - c-|^2 - 2 d* | <= eps1 = (4.5 D + 45) 2^-53      (x-, c- are f64 roundings of the true directions)
//   | d_ref - d* |         <= E'   = (2 D + 16) u            (the reference's arithmetic; u = 2^-24 | 2^-53)
// (select.hip cos_proof_lb) every other centre's reference distance is at least (tau' - eps1) / 2 - E', and a
// row is PROVEN when that, pushed down by the roundings of its own evaluation, is strictly above the candidate's d: then
// no other centre ties or beats it.  A tie of two centres is never proven: the exact kernel alone decides (key, number).
// Rows that are not proven -- and every row of a call with a flagged centre -- are listed on the device and answered by
// the exact kernel.  Flagged: not finite, or a squared norm outside [2^-100, 2^100].
//
// Layout of the filter (the frame of foreign.hip).  A workgroup of WAVES waves holds 32 WAVES rows: their
// two images lie in LDS ([2][rows][dp + 8], 16 bytes of padding per row) and are the B operands of
// v_mfma_f32_32x32x16_bf16; a wave owns 32 rows, the ROW on the lane (lane & 31), 16 centres in the lane's accumulator.
// The centres stream past as the A operands in stages of 32 SUB centres (SUB = 4, 2, 1 by the row width): a stage is read
// from HBM / L2 once per WORKGROUP into registers while the previous stage is contracted, stored to the other of two LDS
// buffers and shared by the waves; cn travels with it in three small buffers, because the scan of a tile's accumulator
// runs one tile late -- the chain of tile t + 1 is issued before tile t is scanned, so the VALU works while the matrix
// core does.  One barrier per stage.  Three MFMAs per 16 columns on one chain: dp <= 304 keeps it at 57, inside the 65
// the allowance g is checked for (pn_bf16_selftest).  WAVES = 4 up to dp = 192 (153,984 bytes of LDS at most), 2 up to
// dp = 304 (160,128 bytes); wider rows take the exact kernel.
//
// This translation unit is compiled with -ffp-contract=off: every operation outside the MFMA is plain IEEE, unfused.
#include "../../include/petal_mi355x.h"
#include "pn_internal.h"
#include "km_pack.h"

namespace pn {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kSkmMaxDp = 304, kSkmWideDp = 192;  // four waves up to kSkmWideDp padded columns, two beyond
constexpr int kSkmLabelRows = 64, kSkmLabelPitch = 65;
constexpr int kSkmSeg = 4096;

__host__ __device__ inline int skm_sub(int dp) { return dp <= 48 ? 4 : dp <= 96 ? 2 : 1; }  // 32-centre tiles per stage

__device__ __forceinline__ void skm_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

template <typename T> __device__ __forceinline__ T skm_nan();
template <> __device__ __forceinline__ float skm_nan<float>() { return __uint_as_float(0x7FC00000u); }
template <> __device__ __forceinline__ double skm_nan<double>() { return __longlong_as_double(0x7FF8000000000000ll); }

// the order-preserving map of ALL floats (select.hip, sel_key_signed): -0 as +0, NaN above +inf
template <typename T> struct SkmKey;
template <> struct SkmKey<float> {
    static constexpr uint32_t kNaN = 0xFFC00000u, kInf = 0xFF800000u;
    static __device__ __forceinline__ uint32_t of(float d) {
        if (d != d) return kNaN;
        const uint32_t b = __float_as_uint(d == 0.0f ? 0.0f : d);
        return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
};
template <> struct SkmKey<double> {
    static constexpr uint64_t kNaN = 0xFFF8000000000000ull, kInf = 0xFFF0000000000000ull;
    static __device__ __forceinline__ uint64_t of(double d) {
        if (d != d) return kNaN;
        const uint64_t b = (uint64_t)__double_as_longlong(d == 0.0 ? 0.0 : d);
        return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
    }
};

__global__ void skm_zero_kernel(unsigned long long *p, int words) {
    if ((int)threadIdx.x < words) p[threadIdx.x] = 0ull;
}

// ---- the filter.  grid: the row tiles; PF = the 16-byte chunks a thread carries from HBM to LDS per stage, at most
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void skm_filter_kernel(const uint16_t *__restrict__ ximg,
                                                                const uint16_t *__restrict__ xlo, size_t n, int dp,
                                                                const uint16_t *__restrict__ cimg,
                                                                const uint16_t *__restrict__ clo,
                                                                const float *__restrict__ cn, size_t nc_pad,
                                                                uint32_t *__restrict__ cand, float *__restrict__ tau) {
    constexpr int kRows = 32 * WAVES, kThreads = 64 * WAVES, PF = WAVES == 4 ? 6 : 19;
    extern __shared__ __align__(16) unsigned char skm_smem[];
    const int pitch = dp + 8, chunks = dp >> 3, ksteps = dp >> 4, sub = WAVES == 4 ? skm_sub(dp) : 1, srows = 32 * sub;
    uint16_t *btile = (uint16_t *)skm_smem, *btile_lo = btile + (size_t)kRows * pitch;
    uint16_t *abuf = btile_lo + (size_t)kRows * pitch;     // [2 buffers][2 images][srows][pitch]
    float *meta = (float *)(abuf + (size_t)4 * srows * pitch);  // [3][srows]: the stage's cn
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 31, h = lane >> 5;
    const size_t row0 = (size_t)blockIdx.x * kRows;  // (the images have whole tiles of 128 rows: rows beyond n are zeros)
    const size_t n_stages = (nc_pad + (size_t)srows - 1) / (size_t)srows;

    // ---- the workgroup's rows
    for (int q = t; q < kRows * chunks; q += kThreads) {
        const int rr = q / chunks, ch = q - rr * chunks;
        const size_t src = (row0 + (size_t)rr) * (size_t)dp + (size_t)ch * 8;
        *(u32x4 *)(btile + (size_t)rr * pitch + ch * 8) = *(const u32x4 *)(ximg + src);
        *(u32x4 *)(btile_lo + (size_t)rr * pitch + ch * 8) = *(const u32x4 *)(xlo + src);
    }

    // ---- the stream of the centres.  Stage s lies in data buffer s & 1 and meta buffer s % 3.
    const int per_img = srows * chunks, total = 2 * per_img;  // 16-byte chunks of a stage: total <= PF kThreads
    u32x4 pf[PF];
    float pm_cn = 0.0f;
    auto fetch = [&](size_t stage) {  // HBM / L2 -> registers
        const size_t c0 = stage * (size_t)srows;
#pragma unroll
        for (int e = 0; e < PF; ++e) {
            const int q = t + kThreads * e;
            pf[e] = u32x4{0u, 0u, 0u, 0u};
            if (q < total) {
                const int im = q >= per_img ? 1 : 0, rem = q - im * per_img, rr = rem / chunks, ch = rem - rr * chunks;
                if (c0 + (size_t)rr < nc_pad)  // (the last stage may reach beyond the padded centres: zeros, never scanned)
                    pf[e] = *(const u32x4 *)((im ? clo : cimg) + (c0 + (size_t)rr) * (size_t)dp + (size_t)ch * 8);
            }
        }
        if (t < srows) pm_cn = c0 + (size_t)t < nc_pad ? cn[c0 + (size_t)t] : __uint_as_float(0x7F800000u);
    };
    auto store = [&](size_t stage) {  // registers -> LDS
        uint16_t *dst = abuf + (size_t)(stage & 1) * 2 * srows * pitch;
#pragma unroll
        for (int e = 0; e < PF; ++e) {
            const int q = t + kThreads * e;
            if (q < total) {
                const int im = q >= per_img ? 1 : 0, rem = q - im * per_img, rr = rem / chunks, ch = rem - rr * chunks;
                *(u32x4 *)(dst + ((size_t)im * srows + rr) * pitch + ch * 8) = pf[e];
            }
        }
        if (t < srows) meta[(int)(stage % 3) * srows + t] = pm_cn;
    };
    const uint16_t *brow = btile + (size_t)(w * 32 + r) * pitch + h * 8;
    const uint16_t *brow_lo = btile_lo + (size_t)(w * 32 + r) * pitch + h * 8;
    auto chain = [&](size_t stage, int v) {
        const uint16_t *a0 = abuf + (size_t)(stage & 1) * 2 * srows * pitch + (size_t)(v * 32 + r) * pitch + h * 8;
        const uint16_t *a1 = a0 + (size_t)srows * pitch;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
        for (int ks = 0; ks < ksteps; ++ks) {
            const bf16x8 a = *(const bf16x8 *)(a0 + ks * 16);
            const bf16x8 al = *(const bf16x8 *)(a1 + ks * 16);
            const bf16x8 b = *(const bf16x8 *)(brow + ks * 16);
            const bf16x8 bl = *(const bf16x8 *)(brow_lo + ks * 16);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, b, acc, 0, 0, 0);
        }
        return acc;
    };
    // registers 4 g .. 4 g + 3 of the accumulator are the tile's centres 8 g + 4 h + 0 .. 3 (the C layout of the
    // instruction); the padding's cn is +inf, so its keys never pass the strict '<'
    const float inf = __uint_as_float(0x7F800000u);
    float k1 = inf, k2 = inf;
    uint32_t c1 = 0xFFFFFFFFu;
    auto scan = [&](const f32x16 &acc, size_t stage, int v) {
        const float *m = meta + (int)(stage % 3) * srows + v * 32 + 4 * h;
        const uint32_t j0 = (uint32_t)(stage * (size_t)srows) + (uint32_t)(v * 32 + 4 * h);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 cn4 = *(const float4 *)(m + 8 * g);
            const float cnv[4] = {cn4.x, cn4.y, cn4.z, cn4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float key = cnv[j] - 2.0f * acc[4 * g + j];
                if (key < k2) {
                    if (key < k1) {
                        k2 = k1;
                        k1 = key;
                        c1 = j0 + (uint32_t)(8 * g + j);
                    } else {
                        k2 = key;
                    }
                }
            }
        }
    };

    if (n_stages) {
        fetch(0);
        store(0);
    }
    f32x16 acc_prev;
    size_t prev_stage = 0;
    int prev_v = -1;  // (-1: no tile waits for its scan)
    for (size_t s = 0; s < n_stages; ++s) {
        __syncthreads();  // stage s is in LDS (the first time: the rows too); the buffers of stage s + 1 are no longer read
        if (s + 1 < n_stages) fetch(s + 1);
        for (int v = 0; v < sub; ++v) {
            if (s * (size_t)srows + (size_t)(v * 32) >= nc_pad) break;  // (the whole workgroup: tiles beyond the centres)
            const f32x16 acc = chain(s, v);
            if (prev_v >= 0) scan(acc_prev, prev_stage, prev_v);
            acc_prev = acc;
            prev_stage = s;
            prev_v = v;
        }
        if (s + 1 < n_stages) store(s + 1);
    }
    if (prev_v >= 0) scan(acc_prev, prev_stage, prev_v);

    // ---- the other half of the row's centres: the lane 32 away
    const float p1 = __shfl_xor(k1, 32, 64), p2 = __shfl_xor(k2, 32, 64);
    const uint32_t pc = (uint32_t)__shfl_xor((int)c1, 32, 64);
    if (p1 < k2) {
        if (p1 < k1) {
            k2 = k1;
            k1 = p1;
            c1 = pc;
        } else {
            k2 = p1;
        }
    }
    if (p2 < k2) k2 = p2;  // (p2 >= p1 >= k1 by now: it can only be the runner-up)
    const size_t my_row = row0 + (size_t)(w * 32 + r);
    if (h == 0 && my_row < n) {
        cand[my_row] = c1;
        tau[my_row] = k2;
    }
}

// ---- staging of a wave's 64 rows, transposed, in LDS (kmeans.hip, km_stage_rows); sel: the listed rows
template <typename T>
__device__ __forceinline__ void skm_stage_rows(const T *__restrict__ X, size_t ld, int dim, const uint32_t *__restrict__ sel,
                                               size_t first, int rows, int lane, T *__restrict__ tile) {
    for (int r = 0; r < rows; ++r) {
        const size_t i = sel ? (size_t)sel[first + r] : first + (size_t)r;
        for (int k = lane; k < dim; k += kSkmLabelRows) tile[k * kSkmLabelPitch + r] = X[i * ld + k];
    }
    __syncthreads();
}

// ---- the exact kernel: Cosine::distance of every centre for thread j's row (sel / nsel as in km_exact_kernel), the
// least (signed key, centre number); a row whose least key is the NaN key is a member of nothing
template <typename T, bool STAGED>
__global__ __launch_bounds__(kSkmLabelRows) void skm_exact_kernel(const T *__restrict__ X, size_t n, size_t ld, int dim,
                                                                  const T *__restrict__ rnorm,
                                                                  const T *__restrict__ centres,
                                                                  const T *__restrict__ cnorm, size_t nc,
                                                                  const uint32_t *__restrict__ sel,
                                                                  const uint32_t *__restrict__ nsel,
                                                                  int64_t *__restrict__ labels, T *__restrict__ dist) {
#pragma clang fp contract(off)
    using K = typename KeyOf<T>::type;
    extern __shared__ __align__(16) unsigned char skm_smem[];
    T *tile = (T *)skm_smem;
    const int lane = threadIdx.x;
    const size_t count = sel ? (size_t)*nsel : n;
    const size_t first = (size_t)blockIdx.x * kSkmLabelRows, j = first + lane;
    if (first >= count) return;  // (the whole workgroup)
    if (STAGED) {
        const int rows = count - first < (size_t)kSkmLabelRows ? (int)(count - first) : kSkmLabelRows;
        skm_stage_rows<T>(X, ld, dim, sel, first, rows, lane, tile);
    }
    if (j >= count) return;
    const size_t i = sel ? (size_t)sel[j] : j;
    const T *row = X + i * ld;
    const T rn = rnorm[i];
    K best = SkmKey<T>::kNaN;  // (only keys below the NaN key make a member)
    int64_t lab = -1;
    T best_d = skm_nan<T>();
    for (size_t c = 0; c < nc; c += 4) {
        const T *cp[4];
        T dot[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            cp[u] = centres + (c + u < nc ? c + u : nc - 1) * (size_t)dim;  // (past the end: the last centre again, not used)
            dot[u] = (T)0;
        }
        for (int k = 0; k < dim; ++k) {
            const T x = STAGED ? tile[k * kSkmLabelPitch + lane] : row[k];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const T pr = cp[u][k] * x;
                dot[u] = dot[u] + pr;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const T den = cnorm[c + u < nc ? c + u : nc - 1] * rn;
            const T d = (T)1 - dot[u] / den;
            const K key = SkmKey<T>::of(d);
            if (c + u < nc && key < best) {
                best = key;
                lab = (int64_t)(c + u);
                best_d = d;
            }
        }
    }
    labels[i] = lab;
    if (dist) dist[i] = best_d;
}

// ---- re-rank and proof: one thread per row, the wave's rows staged as above.  The candidate's distance in the
// reference's arithmetic; proven rows are answered here, the others are listed: slot = atomicAdd(nsel), sel[slot] = row.
template <typename T, bool STAGED>
__global__ __launch_bounds__(kSkmLabelRows) void skm_rerank_kernel(const T *__restrict__ X, size_t n, size_t ld, int dim,
                                                                   const T *__restrict__ rnorm,
                                                                   const T *__restrict__ centres,
                                                                   const T *__restrict__ cnorm, size_t nc,
                                                                   const uint32_t *__restrict__ cand,
                                                                   const float *__restrict__ tau,
                                                                   const double *__restrict__ xn,
                                                                   const float *__restrict__ xh,
                                                                   const float *__restrict__ xl,
                                                                   const float *__restrict__ xe,
                                                                   const unsigned long long *__restrict__ cc,
                                                                   uint32_t *__restrict__ sel, uint32_t *__restrict__ nsel,
                                                                   int64_t *__restrict__ labels, T *__restrict__ dist) {
#pragma clang fp contract(off)
    using K = typename KeyOf<T>::type;
    extern __shared__ __align__(16) unsigned char skm_smem[];
    T *tile = (T *)skm_smem;
    const int lane = threadIdx.x;
    const size_t first = (size_t)blockIdx.x * kSkmLabelRows, i = first + lane;
    if (STAGED) {
        const int rows = n - first < (size_t)kSkmLabelRows ? (int)(n - first) : kSkmLabelRows;
        skm_stage_rows<T>(X, ld, dim, nullptr, first, rows, lane, tile);
    }
    if (i >= n) return;
    const uint32_t c = cand[i];
    const double xnr = xn[i];
    const float tv = tau[i];
    // (a flagged centre, a flagged row, no candidate, no finite runner-up: the exact kernel)
    bool ok = cc[4] == 0 && xnr == xnr && (size_t)c < nc && tv < __uint_as_float(0x7F800000u);
    T d = (T)0;
    if (ok) {
        const T *cp = centres + (size_t)c * (size_t)dim;
        const T *row = X + i * ld;
        T dot = (T)0;
        for (int k = 0; k < dim; ++k) {
            const T x = STAGED ? tile[k * kSkmLabelPitch + lane] : row[k];
            const T pr = cp[k] * x;
            dot = dot + pr;
        }
        const T den = cnorm[c] * rnorm[i];
        d = (T)1 - dot / den;
        const K kk = SkmKey<T>::of(d);
        if (kk >= SkmKey<T>::kInf) {
            ok = false;  // an infinite or NaN distance: the exact kernel orders it
        } else {
            const double u = sizeof(T) == 4 ? 5.9604644775390625e-08 : 1.1102230246251565e-16;
            const double slack = km_row_slack((double)xh[i], (double)xl[i], (double)xe[i], cc);
            // tau' = xn + tau - E, pushed down by the roundings of its own evaluation
            double lb = (xnr + (double)tv) - slack;
            lb = lb - (xnr + fabs((double)tv) + slack) * 1.7763568394002505e-15;  // 2^-49
            // (tau' - eps1) / 2 - E' - guard: cos_proof_lb's constants (select.hip)
            const double eps1 = (4.5 * (double)dim + 45.0) * 1.1102230246251565e-16;
            const double e = (2.0 * (double)dim + 16.0) * u;
            lb = 0.5 * (lb - eps1) - e - (fabs(lb) + 1.0) * 1.0e-15;
            ok = lb > (double)d;
        }
    }
    if (ok) {
        labels[i] = (int64_t)c;
        if (dist) dist[i] = d;
    } else {
        const uint32_t slot = atomicAdd(nsel, 1u);
        sel[slot] = (uint32_t)i;  // (slot < n: every row is listed at most once)
    }
}

// ---- the update.  km_segment_sums_kernel (kmeans.hip) with the member's term x / |x|: (double)x[i][col] / (double)rnorm[i]
template <typename T, int COLS>
__global__ __launch_bounds__(64) void skm_segment_sums_kernel(const uint64_t *__restrict__ key,
                                                              const uint64_t *__restrict__ off,
                                                              const uint64_t *__restrict__ seg_off, size_t nc,
                                                              const T *__restrict__ X, size_t ld, int dim,
                                                              const T *__restrict__ rnorm, double *__restrict__ segsum) {
#pragma clang fp contract(off)
    __shared__ double s_part[COLS][65];
    const int lane = threadIdx.x;
    const uint64_t b = blockIdx.x;
    if (b >= seg_off[nc]) return;
    size_t lo = 0, hi = nc;  // the cluster: the last c with seg_off[c] <= b
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (seg_off[mid] <= b)
            lo = mid;
        else
            hi = mid;
    }
    const size_t c = lo;
    const uint64_t s = b - seg_off[c];
    const uint64_t beg = off[c] + s * kSkmSeg, rest = off[c + 1] - beg;
    const uint64_t len = rest < (uint64_t)kSkmSeg ? rest : (uint64_t)kSkmSeg;
    for (int c0 = 0; c0 < dim; c0 += COLS) {
        double P[COLS];
#pragma unroll
        for (int k = 0; k < COLS; ++k) P[k] = 0.0;
        for (uint64_t j = lane; j < len; j += 64) {
            // (c0 + COLS <= ld: the row's padding is read, and never used)
            const size_t i = (size_t)(uint32_t)key[beg + j];
            const T *__restrict__ row = X + i * ld + c0;
            const double rn = (double)rnorm[i];
            T v[COLS];
#pragma unroll
            for (int k = 0; k < COLS; ++k) v[k] = row[k];
#pragma unroll
            for (int k = 0; k < COLS; ++k) {
                const double q = (double)v[k] / rn;
                P[k] = P[k] + q;
            }
        }
#pragma unroll
        for (int k = 0; k < COLS; ++k) s_part[k][lane] = P[k];
        skm_lds_fence();
        const int col = c0 + lane;
        if (lane < COLS && col < dim) {
            double S = s_part[lane][0];
#pragma unroll 9
            for (int l = 1; l < 64; ++l) S = S + s_part[lane][l];
            segsum[b * (uint64_t)dim + col] = S;
        }
        skm_lds_fence();
    }
}
// One wave per centre: S_col = the segments in order; Q = the sum of S_col^2 in the 64-partial shape; the new centre
// (T)(S_col / sqrt(Q)); tc[c] <- the sum of the squared moves in the same shape.  A centre without members, or whose Q is
// 0 or not finite, is unchanged.
template <typename T>
__global__ __launch_bounds__(64) void skm_move_kernel(const uint64_t *__restrict__ off, const uint64_t *__restrict__ seg_off,
                                                      const double *__restrict__ segsum, int dim, T *__restrict__ centres,
                                                      double *__restrict__ tc) {
#pragma clang fp contract(off)
    __shared__ double s_t[64];
    const int lane = threadIdx.x;
    const size_t c = blockIdx.x;
    const uint64_t m = off[c + 1] - off[c];
    const uint64_t s0 = seg_off[c], s1 = seg_off[c + 1];
    auto column = [&](int col) {
        double S = segsum[s0 * (uint64_t)dim + col];
        for (uint64_t s = s0 + 1; s < s1; ++s) S = S + segsum[s * (uint64_t)dim + col];
        return S;
    };
    double q = 0.0;
    if (m)
        for (int col = lane; col < dim; col += 64) {
            const double S = column(col);
            const double sq = S * S;
            q = q + sq;
        }
    s_t[lane] = q;
    __syncthreads();
    double Q = s_t[0];
    for (int l = 1; l < 64; ++l) Q = Q + s_t[l];  // (every lane the same fold)
    __syncthreads();
    const bool move = m != 0 && Q > 0.0 && Q < __longlong_as_double(0x7FF0000000000000ll);
    const double rq = sqrt(Q);
    double part = 0.0;
    for (int col = lane; col < dim; col += 64) {
        const T old = centres[c * (size_t)dim + col];
        T nw = old;
        if (move) {
            nw = (T)(column(col) / rq);
            centres[c * (size_t)dim + col] = nw;
        }
        const double dd = (double)nw - (double)old;
        const double sq = dd * dd;
        part = part + sq;
    }
    s_t[lane] = part;
    __syncthreads();
    if (lane == 0) {
        double S = s_t[0];
        for (int l = 1; l < 64; ++l) S = S + s_t[l];
        tc[c] = S;
    }
}

}  // namespace

bool skm_filter_supported(int dim) { return dim >= 8 && (dim + 15) / 16 * 16 <= kSkmMaxDp; }

template <typename T>
hipError_t launch_skm_pack_rows(const T *X, size_t n, size_t ld, int dim, const KmRowImage &r, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL((km_pack_kernel<T, true, true>), dim3((unsigned)((r.n_img + 3) / 4)), dim3(256), 0, s, X, n, r.n_img, ld,
                       dim, r.dp, r.img, r.lo, r.xn, r.xh, r.xl, r.xe, (float *)nullptr, (unsigned long long *)nullptr,
                       (const float *)nullptr);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_skm_pack_centres(const T *centres, size_t nc, int dim, const KmCentreImage &c, hipStream_t s) {
    const int dp = (dim + 15) / 16 * 16;
    hipLaunchKernelGGL(skm_zero_kernel, dim3(1), dim3(64), 0, s, c.cc, 8);
    hipLaunchKernelGGL((km_pack_kernel<T, false, true>), dim3((unsigned)((c.nc_pad + 3) / 4)), dim3(256), 0, s, centres, nc,
                       c.nc_pad, (size_t)dim, dim, dp, c.img, c.lo, (double *)nullptr, (float *)nullptr, (float *)nullptr,
                       (float *)nullptr, c.cn, c.cc, (const float *)nullptr);
    return hipGetLastError();
}

hipError_t launch_skm_filter(const KmRowImage &r, size_t n, const KmCentreImage &c, size_t nc, uint32_t *cand, float *tau,
                             hipStream_t s) {
    if (n == 0 || nc == 0) return hipSuccess;
    if (r.dp > kSkmMaxDp) return hipErrorInvalidValue;
    static LdsAttrOnce once4, once2;
    const bool wide = r.dp > kSkmWideDp;
    const int rows = wide ? 64 : 128, srows = 32 * (wide ? 1 : skm_sub(r.dp));
    const size_t lds = ((size_t)2 * rows + (size_t)4 * srows) * (size_t)(r.dp + 8) * 2 + (size_t)3 * srows * 4;
    if (lds > 64 * 1024) {
        const hipError_t e = wide ? once2.ensure((const void *)skm_filter_kernel<2>, (size_t)256 * (kSkmMaxDp + 8) * 2 + 384)
                                  : once4.ensure((const void *)skm_filter_kernel<4>, (size_t)384 * (kSkmWideDp + 8) * 2 + 384);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)(r.n_img / rows));
    if (wide)
        hipLaunchKernelGGL((skm_filter_kernel<2>), grid, dim3(128), lds, s, r.img, r.lo, n, r.dp, c.img, c.lo, c.cn, c.nc_pad,
                           cand, tau);
    else
        hipLaunchKernelGGL((skm_filter_kernel<4>), grid, dim3(256), lds, s, r.img, r.lo, n, r.dp, c.img, c.lo, c.cn, c.nc_pad,
                           cand, tau);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_skm_rerank(const T *X, size_t n, size_t ld, int dim, const T *rnorm, const T *centres, const T *cnorm,
                             size_t nc, const uint32_t *cand, const float *tau, const KmRowImage &r, const KmCentreImage &c,
                             uint32_t *sel, uint32_t *nsel, int64_t *labels, T *dist, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + kSkmLabelRows - 1) / kSkmLabelRows)), blk(kSkmLabelRows);
    const size_t tile = (size_t)dim * kSkmLabelPitch * sizeof(T);
    hipLaunchKernelGGL(skm_zero_kernel, dim3(1), dim3(64), 0, s, (unsigned long long *)nsel, 1);
    if (tile <= 64 * 1024)
        hipLaunchKernelGGL((skm_rerank_kernel<T, true>), grid, blk, tile, s, X, n, ld, dim, rnorm, centres, cnorm, nc, cand, tau,
                           r.xn, r.xh, r.xl, r.xe, c.cc, sel, nsel, labels, dist);
    else
        hipLaunchKernelGGL((skm_rerank_kernel<T, false>), grid, blk, 0, s, X, n, ld, dim, rnorm, centres, cnorm, nc, cand, tau,
                           r.xn, r.xh, r.xl, r.xe, c.cc, sel, nsel, labels, dist);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_skm_exact(const T *X, size_t n, size_t ld, int dim, const T *rnorm, const T *centres, const T *cnorm,
                            size_t nc, const uint32_t *sel, const uint32_t *nsel, int64_t *labels, T *dist, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + kSkmLabelRows - 1) / kSkmLabelRows)), blk(kSkmLabelRows);
    const size_t tile = (size_t)dim * kSkmLabelPitch * sizeof(T);
    if (tile <= 64 * 1024)
        hipLaunchKernelGGL((skm_exact_kernel<T, true>), grid, blk, tile, s, X, n, ld, dim, rnorm, centres, cnorm, nc, sel, nsel,
                           labels, dist);
    else  // (rows too long for LDS: read in place)
        hipLaunchKernelGGL((skm_exact_kernel<T, false>), grid, blk, 0, s, X, n, ld, dim, rnorm, centres, cnorm, nc, sel, nsel,
                           labels, dist);
    return hipGetLastError();
}

template <typename T>
hipError_t skm_update_enqueue(const T *X, size_t n, size_t ld, int dim, const T *rnorm, const int64_t *labels, size_t nc,
                              void *buf, T *centres, uint64_t *counts, double tol, int last, double **stop_out,
                              hipStream_t s) {
    KmMembers m;
    const hipError_t e = km_members_enqueue(labels, n, nc, dim, buf, centres != nullptr, counts, &m, s);
    if (e != hipSuccess) return e;
    if (stop_out) *stop_out = m.stop;
    if (!centres) return hipGetLastError();
    const dim3 grid((unsigned)m.max_segments);
    if (ld % 16 == 0)
        hipLaunchKernelGGL((skm_segment_sums_kernel<T, 16>), grid, dim3(64), 0, s, m.key, m.off, m.seg_off, nc, X, ld, dim, rnorm,
                           m.segsum);
    else
        hipLaunchKernelGGL((skm_segment_sums_kernel<T, 8>), grid, dim3(64), 0, s, m.key, m.off, m.seg_off, nc, X, ld, dim, rnorm,
                           m.segsum);
    hipLaunchKernelGGL((skm_move_kernel<T>), dim3((unsigned)nc), dim3(64), 0, s, m.off, m.seg_off, m.segsum, dim, centres, m.tc);
    return launch_km_stop(m.tc, nc, tol, last, m.stop, s);
}

#define PN_SKM_INSTANTIATE(T)                                                                                              \
    template hipError_t launch_skm_pack_rows<T>(const T *, size_t, size_t, int, const KmRowImage &, hipStream_t);          \
    template hipError_t launch_skm_pack_centres<T>(const T *, size_t, int, const KmCentreImage &, hipStream_t);            \
    template hipError_t launch_skm_rerank<T>(const T *, size_t, size_t, int, const T *, const T *, const T *, size_t,      \
                                             const uint32_t *, const float *, const KmRowImage &, const KmCentreImage &,   \
                                             uint32_t *, uint32_t *, int64_t *, T *, hipStream_t);                         \
    template hipError_t launch_skm_exact<T>(const T *, size_t, size_t, int, const T *, const T *, const T *, size_t,       \
                                            const uint32_t *, const uint32_t *, int64_t *, T *, hipStream_t);              \
    template hipError_t skm_update_enqueue<T>(const T *, size_t, size_t, int, const T *, const int64_t *, size_t, void *,  \
                                              T *, uint64_t *, double, int, double **, hipStream_t);
PN_SKM_INSTANTIATE(float)
PN_SKM_INSTANTIATE(double)
#undef PN_SKM_INSTANTIATE

}  // namespace pn
