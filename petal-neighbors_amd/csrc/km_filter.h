// km_filter.h -- what the small MFMA filters share beyond their packing (km_pack.h): k-means (kmeans.hip),
// the m nearest centres (kmeans_nearest.hip, 4.27), spherical k-means (spherical_kmeans.hip, 4.28) and the nearest-foreign
// tier (foreign.hip, 4.25).  The slack E(x) of km_pack.h is a bound of ONE accumulation shape and feeds ONE proof; both
// live here, once: the three-MFMA chain, the load of a row tile, the
// exact-side helpers of the re-rank (the reference's fold, tau' and the proof's right-hand side), and the kernels and
// launchers of an assignment that differ by metric only, the metric being a policy (KmMetric) each unit defines for
// itself.  The anonymous part has internal linkage, as km_pack.h: each unit compiles its own copy.  Every unit that
// includes this header is compiled with -ffp-contract=off.
#pragma once
#include "km_pack.h"

namespace pn {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void km_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// (a kernel, not a memset: the words are cleared in stream order whatever the caller's stream is captured into)
__global__ void km_zero_kernel(unsigned long long *p, int words) {
    if ((int)threadIdx.x < words) p[threadIdx.x] = 0ull;
}
inline void km_zero_words(void *p, int words, hipStream_t s) {  // words <= 64, p 8-byte aligned
    hipLaunchKernelGGL(km_zero_kernel, dim3(1), dim3(64), 0, s, (unsigned long long *)p, words);
}

// ---- the chain: S = a^ . b^ + a^ . b~ + a~ . b^ over ksteps steps of 16 columns, three MFMAs per step on one f32
// accumulator that starts at zero -- the shape the allowance g = 2^-13 of km_pack.h's bound is checked for, up to 65
// MFMAs (pn_bf16_selftest).  a_hi / a_lo, b_hi / b_lo: this lane's 8 elements of the first step in the
// two images of its A row (lane & 31) and of its B row, i.e. row start + 8 (lane >> 5).  The accumulator has the B row on
// the lane and 16 A rows in the registers: registers 4 g .. 4 g + 3 are the tile's A rows 8 g + 4 (lane >> 5) + 0 .. 3
// (the C layout of the instruction).
__device__ __forceinline__ f32x16 km_mfma_chain(const uint16_t *a_hi, const uint16_t *a_lo, const uint16_t *b_hi,
                                                const uint16_t *b_lo, int ksteps) {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (int ks = 0; ks < ksteps; ++ks) {
        const bf16x8 a = *(const bf16x8 *)(a_hi + ks * 16);
        const bf16x8 al = *(const bf16x8 *)(a_lo + ks * 16);
        const bf16x8 b = *(const bf16x8 *)(b_hi + ks * 16);
        const bf16x8 bl = *(const bf16x8 *)(b_lo + ks * 16);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, b, acc, 0, 0, 0);
    }
    return acc;
}

// ---- a workgroup's B operands: `rows` rows of the two images into LDS, tile / tile_lo [rows][pitch] (pitch = dp + 8: the
// 16 bytes of padding spread the rows over the banks), in 16-byte chunks.  The contiguous form reads rows row0 .. of
// img / lo [..][dp] (whole tiles exist: rows beyond n are zeros); the gathered form reads row list[pos0 + rr] and fills
// positions at and beyond nq with zeros.
template <int THREADS>
__device__ __forceinline__ void km_load_row_tile(uint16_t *tile, uint16_t *tile_lo, const uint16_t *__restrict__ img,
                                                 const uint16_t *__restrict__ lo, size_t row0, int rows, int dp, int t) {
    const int chunks = dp >> 3, pitch = dp + 8;
    for (int q = t; q < rows * chunks; q += THREADS) {
        const int rr = q / chunks, ch = q - rr * chunks;
        const size_t src = (row0 + (size_t)rr) * (size_t)dp + (size_t)ch * 8;
        *(u32x4 *)(tile + (size_t)rr * pitch + ch * 8) = *(const u32x4 *)(img + src);
        *(u32x4 *)(tile_lo + (size_t)rr * pitch + ch * 8) = *(const u32x4 *)(lo + src);
    }
}
template <int THREADS>
__device__ __forceinline__ void km_gather_row_tile(uint16_t *tile, uint16_t *tile_lo, const uint16_t *__restrict__ img,
                                                   const uint16_t *__restrict__ lo, const uint32_t *__restrict__ list,
                                                   size_t pos0, size_t nq, int rows, int dp, int t) {
    const int chunks = dp >> 3, pitch = dp + 8;
    for (int q = t; q < rows * chunks; q += THREADS) {
        const int rr = q / chunks, ch = q - rr * chunks;
        u32x4 vh = {0u, 0u, 0u, 0u}, vl = {0u, 0u, 0u, 0u};
        if (pos0 + (size_t)rr < nq) {
            const size_t src = (size_t)list[pos0 + rr] * (size_t)dp + (size_t)ch * 8;
            vh = *(const u32x4 *)(img + src);
            vl = *(const u32x4 *)(lo + src);
        }
        *(u32x4 *)(tile + (size_t)rr * pitch + ch * 8) = vh;
        *(u32x4 *)(tile_lo + (size_t)rr * pitch + ch * 8) = vl;
    }
}

// ---- the exact side: the reference's fold, and the proof that a folded candidate beats everything the filter set aside
template <typename T>
__device__ __forceinline__ T km_sqrt(T x);
template <>
__device__ __forceinline__ float km_sqrt<float>(float x) { return sqrtf(x); }  // correctly rounded (build flags)
template <>
__device__ __forceinline__ double km_sqrt<double>(double x) { return sqrt(x); }

// the sortable key of a distance >= +0 (KeyOf: its bits; every NaN the one NaN key)
template <typename T>
__device__ __forceinline__ typename KeyOf<T>::type km_dist_key(T d) {
    using K = typename KeyOf<T>::type;
    if constexpr (sizeof(T) == 4)
        return d != d ? KeyOf<T>::kNaN : (K)__float_as_uint(d);
    else
        return d != d ? KeyOf<T>::kNaN : (K)__double_as_longlong(d);
}
template <typename T> __device__ __forceinline__ T km_nan();
template <> __device__ __forceinline__ float km_nan<float>() { return __uint_as_float(0x7FC00000u); }
template <> __device__ __forceinline__ double km_nan<double>() { return __longlong_as_double(0x7FF8000000000000ll); }

// staging of a wave's 64 rows, transposed, in LDS (ms_labels_kernel says why); sel: the listed rows
constexpr int kKmLabelRows = 64, kKmLabelPitch = 65;
template <typename T>
__device__ __forceinline__ void km_stage_rows(const T *__restrict__ X, size_t ld, int dim, const uint32_t *__restrict__ sel,
                                              size_t first, int rows, int lane, T *__restrict__ tile) {
    for (int r = 0; r < rows; ++r) {
        const size_t i = sel ? (size_t)sel[first + r] : first + (size_t)r;
        for (int k = lane; k < dim; k += kKmLabelRows) tile[k * kKmLabelPitch + r] = X[i * ld + k];
    }
    __syncthreads();
}
inline size_t km_stage_bytes(int dim, size_t elem) { return (size_t)dim * kKmLabelPitch * elem; }

// tau' = xn + tau - E <= |x - c|^2 of every centre whose key is at least tau, pushed down by the roundings of its own
// evaluation (2^-49 of the magnitudes that met)
__device__ __forceinline__ double km_tau_floor(double xn, double tau, double slack) {
    const double lb = (xn + tau) - slack;
    return lb - (xn + fabs(tau) + slack) * 1.7763568394002505e-15;
}
// lb <= |x - c|^2 -> a bound of the SQUARE of the reference's folded Euclidean distance before its final rounding: the
// fold of D terms loses at most (D + 4) u relatively (u = 2^-24 | 2^-53), and an absolute guard
template <typename T>
__device__ __forceinline__ double km_euclid_push_down(double lb, int dim) {
    if constexpr (sizeof(T) == 4)
        return lb * (1.0 - (double)(dim + 4) * 5.9604644775390625e-08) - 1e-37;
    else
        return lb * (1.0 - (double)(dim + 4) * 1.1102230246251565e-16) * (1.0 - 8.881784197001252e-16) - 1e-300;
}
// the proof's right-hand side: everything at or below it may still round to d (key kk, finite) and tie (select.hip)
template <typename T> __device__ __forceinline__ double km_proof_rhs(typename KeyOf<T>::type kk);
template <> __device__ __forceinline__ double km_proof_rhs<float>(uint32_t kk) {
    const double dk = (double)__uint_as_float(kk), dn = (double)__uint_as_float(kk + 1);  // succ(d): the next float up
    const double mid = 0.5 * (dk + dn);
    return mid * mid * (1.0 + 4.5e-16);
}
template <> __device__ __forceinline__ double km_proof_rhs<double>(uint64_t kk) {
    const double dn = __longlong_as_double((long long)(kk + 1));
    return dn * dn * (1.0 + 4.440892098500626e-16);
}
// the Euclidean proof: no centre of key >= tau can tie or beat a candidate folded to the key kk,
//   (xn + tau - E) (1 - (D + 4) u) - guard > ((d + succ d) / 2)^2.
// Never proven: an infinite or NaN kk, a NaN tau; tau = +inf: no other centre exists.  tau_floor(): tau', asked for at most once.
template <typename T, typename TauFloor>
__device__ __forceinline__ bool km_euclid_proven(typename KeyOf<T>::type kk, float tau, int dim, TauFloor tau_floor) {
    using K = typename KeyOf<T>::type;
    constexpr K kInf = sizeof(T) == 4 ? (K)0x7F800000u : (K)0x7FF0000000000000ull;
    if (kk >= kInf || tau != tau) return false;  // (the exact kernel orders it)
    if (!(tau < __uint_as_float(0x7F800000u))) return true;
    return km_euclid_push_down<T>(tau_floor(), dim) > km_proof_rhs<T>(kk);
}

// ---- the metric of an assignment, a policy each unit defines for its own: KmMetric<T, false> Euclidean (kmeans.hip),
// KmMetric<T, true> Cosine (spherical_kmeans.hip).  With K = KeyOf<T>::type and norms = the call's KmNorms<T>:
//   term(c, x)                      one column's term of the fold (the fold adds the terms in column order)
//   row_norm(norms, i)              what finish() wants of row i, read once per row
//   finish(sum, norms, c, rn) -> d  the distance to centre c from the folded sum
//   key(d) -> K                     the order of the answers; kNoKey: a best that every member's key is below
//   no_dist()                       the distance of a row that is a member of nothing
//   admits(tau, i)                  false: row i is listed whatever its candidate is (tau [n] need not be read)
//   proven(d, tau, dim, tau_floor)  the proof inequality (tau_floor(): km_tau_floor of the row, evaluated on demand)
//   launch_move(m, nc, dim, centres, s)   the segments' sums -> the new centres and their squared moves
template <typename T, bool SPH> struct KmMetric;

// ---- the exact kernel: the metric's fold of every centre for thread j's row, the least (key, centre number).  sel / nsel
// (nullable together): thread j of the launch answers row sel[j], j < *nsel (the grid is sized for n).
// (norms is the last argument: the unrolled fold holds 32 scalar registers of centre columns, and with the norms in
// front of the outputs the compiler keeps labels and dist alive in VGPR lanes across it -- an SGPR spill)
template <typename T, typename METRIC, bool STAGED>
__global__ __launch_bounds__(kKmLabelRows) void km_exact_kernel(const T *__restrict__ X, size_t n, size_t ld, int dim,
                                                                const T *__restrict__ centres, size_t nc,
                                                                const uint32_t *__restrict__ sel,
                                                                const uint32_t *__restrict__ nsel,
                                                                int64_t *__restrict__ labels, T *__restrict__ dist,
                                                                KmNorms<T> norms) {
#pragma clang fp contract(off)
    using K = typename KeyOf<T>::type;
    extern __shared__ __align__(16) unsigned char km_smem[];
    T *tile = (T *)km_smem;
    const int lane = threadIdx.x;
    const size_t count = sel ? (size_t)*nsel : n;
    const size_t first = (size_t)blockIdx.x * kKmLabelRows, j = first + lane;
    if (first >= count) return;  // (the whole workgroup)
    if (STAGED) {
        const int rows = count - first < (size_t)kKmLabelRows ? (int)(count - first) : kKmLabelRows;
        km_stage_rows<T>(X, ld, dim, sel, first, rows, lane, tile);
    }
    if (j >= count) return;
    const size_t i = sel ? (size_t)sel[j] : j;
    const T *row = X + i * ld;
    const T rn = METRIC::row_norm(norms, i);
    K best = METRIC::kNoKey;
    int64_t lab = -1;
    T best_d = METRIC::no_dist();
    for (size_t c = 0; c < nc; c += 4) {
        const T *cp[4];
        T sum[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            cp[u] = centres + (c + u < nc ? c + u : nc - 1) * (size_t)dim;  // (past the end: the last centre again, not used)
            sum[u] = (T)0;
        }
        for (int k = 0; k < dim; ++k) {
            const T x = STAGED ? tile[k * kKmLabelPitch + lane] : row[k];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const T term = METRIC::term(cp[u][k], x);
                sum[u] = sum[u] + term;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const T d = METRIC::finish(sum[u], norms, c + u < nc ? c + u : nc - 1, rn);
            const K key = METRIC::key(d);
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
// Listed whatever the candidate is: every row of a call with a flagged centre, a flagged row, a row without a candidate.
template <typename T, typename METRIC, bool STAGED>
__global__ __launch_bounds__(kKmLabelRows) void km_rerank_kernel(const T *__restrict__ X, size_t n, size_t ld, int dim,
                                                                 KmNorms<T> norms, const T *__restrict__ centres, size_t nc,
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
    extern __shared__ __align__(16) unsigned char km_smem[];
    T *tile = (T *)km_smem;
    const int lane = threadIdx.x;
    const size_t first = (size_t)blockIdx.x * kKmLabelRows, i = first + lane;
    if (STAGED) {
        const int rows = n - first < (size_t)kKmLabelRows ? (int)(n - first) : kKmLabelRows;
        km_stage_rows<T>(X, ld, dim, nullptr, first, rows, lane, tile);
    }
    if (i >= n) return;
    const uint32_t c = cand[i];
    const double xnr = xn[i];
    const bool admitted = METRIC::admits(tau, i);
    bool ok = cc[4] == 0 && xnr == xnr && (size_t)c < nc && admitted;
    T d = (T)0;
    if (ok) {
        const T *cp = centres + (size_t)c * (size_t)dim;
        const T *row = X + i * ld;
        T sum = (T)0;
        for (int k = 0; k < dim; ++k) {
            const T x = STAGED ? tile[k * kKmLabelPitch + lane] : row[k];
            const T term = METRIC::term(cp[k], x);
            sum = sum + term;
        }
        d = METRIC::finish(sum, norms, (size_t)c, METRIC::row_norm(norms, i));
        const float tv = tau[i];
        ok = METRIC::proven(d, tv, dim, [&] {
            return km_tau_floor(xnr, (double)tv, km_row_slack((double)xh[i], (double)xl[i], (double)xe[i], cc));
        });
    }
    if (ok) {
        labels[i] = (int64_t)c;
        if (dist) dist[i] = d;
    } else {
        const uint32_t slot = atomicAdd(nsel, 1u);
        sel[slot] = (uint32_t)i;  // (slot < n: every row is listed at most once)
    }
}

// nc == 0: every label -1, every distance NaN
template <typename T>
__global__ __launch_bounds__(256) void km_none_kernel(size_t n, int64_t *__restrict__ labels, T *__restrict__ dist) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    labels[i] = -1;
    if (dist) dist[i] = km_nan<T>();
}

// ---- the update's sums.  One wave per (cluster, segment): workgroup b is segment b of the enumeration seg_off (the
// exclusive scan of nseg); the grid is sized for the most segments a call can have and the surplus exits.  Lane l strides
// the segment's members by 64 and reads COLS consecutive columns of each row; the 64 partials of a column are transposed
// through LDS and lane c folds column c's in lane order (ms_step_kernel).  segsum [segments][dim].
// NORMED: the term of a member is its direction, (double)x[i][col] / (double)rnorm[i]; else (double)x[i][col], and rnorm
// is not read.
constexpr int kKmSeg = 4096;
template <typename T, int COLS, bool NORMED>
__global__ __launch_bounds__(64) void km_segment_sums_kernel(const uint64_t *__restrict__ key,
                                                             const uint64_t *__restrict__ off,
                                                             const uint64_t *__restrict__ seg_off, size_t nc,
                                                             const T *__restrict__ X, size_t ld, int dim,
                                                             double *__restrict__ segsum, const T *__restrict__ rnorm) {
#pragma clang fp contract(off)
    __shared__ double s_part[COLS][65];
    const int lane = threadIdx.x;
    const uint64_t b = blockIdx.x;
    if (b >= seg_off[nc]) return;
    // the cluster: the last c with seg_off[c] <= b (clusters without members have no segment and are skipped by the search)
    size_t lo = 0, hi = nc;
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (seg_off[mid] <= b)
            lo = mid;
        else
            hi = mid;
    }
    const size_t c = lo;
    const uint64_t s = b - seg_off[c];
    const uint64_t beg = off[c] + s * kKmSeg, rest = off[c + 1] - beg;
    const uint64_t len = rest < (uint64_t)kKmSeg ? rest : (uint64_t)kKmSeg;
    for (int c0 = 0; c0 < dim; c0 += COLS) {
        double P[COLS];
#pragma unroll
        for (int k = 0; k < COLS; ++k) P[k] = 0.0;
        for (uint64_t j = lane; j < len; j += 64) {
            // (c0 + COLS <= ld: the row's padding is read, and never used)
            const size_t i = (size_t)(uint32_t)key[beg + j];
            const T *__restrict__ row = X + i * ld + c0;
            double rn = 1.0;
            if constexpr (NORMED) rn = (double)rnorm[i];
            T v[COLS];
#pragma unroll
            for (int k = 0; k < COLS; ++k) v[k] = row[k];
#pragma unroll
            for (int k = 0; k < COLS; ++k) {
                double q = (double)v[k];
                if constexpr (NORMED) q = q / rn;
                P[k] = P[k] + q;
            }
        }
#pragma unroll
        for (int k = 0; k < COLS; ++k) s_part[k][lane] = P[k];
        km_lds_fence();
        const int col = c0 + lane;
        if (lane < COLS && col < dim) {
            double S = s_part[lane][0];
#pragma unroll 9
            for (int l = 1; l < 64; ++l) S = S + s_part[lane][l];
            segsum[b * (uint64_t)dim + col] = S;
        }
        km_lds_fence();
    }
}

}  // namespace

// ---- the launchers that differ by metric only (the declarations and their contracts: pn_internal.h).  Each unit
// instantiates them for its own metric.
template <typename T, bool SPH>
hipError_t launch_km_pack_rows(const T *X, size_t n, size_t ld, int dim, const KmRowImage &r, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL((km_pack_kernel<T, true, SPH>), dim3((unsigned)((r.n_img + 3) / 4)), dim3(256), 0, s, X, n, r.n_img, ld,
                       dim, r.dp, r.img, r.lo, r.xn, r.xh, r.xl, r.xe, (float *)nullptr, (unsigned long long *)nullptr,
                       (const float *)nullptr);
    return hipGetLastError();
}
template <typename T, bool SPH>
hipError_t launch_km_pack_centres(const T *centres, size_t nc, int dim, const KmCentreImage &c, hipStream_t s) {
    const int dp = (dim + 15) / 16 * 16;
    km_zero_words(c.cc, 8, s);
    hipLaunchKernelGGL((km_pack_kernel<T, false, SPH>), dim3((unsigned)((c.nc_pad + 3) / 4)), dim3(256), 0, s, centres, nc,
                       c.nc_pad, (size_t)dim, dim, dp, c.img, c.lo, (double *)nullptr, (float *)nullptr, (float *)nullptr,
                       (float *)nullptr, c.cn, c.cc, (const float *)nullptr);
    return hipGetLastError();
}
template <typename T, bool SPH>
hipError_t launch_km_rerank(const T *X, size_t n, size_t ld, int dim, const KmNorms<T> &norms, const T *centres, size_t nc,
                            const uint32_t *cand, const float *tau, const KmRowImage &r, const KmCentreImage &c,
                            uint32_t *sel, uint32_t *nsel, int64_t *labels, T *dist, hipStream_t s) {
    if (n == 0) return hipSuccess;
    using M = KmMetric<T, SPH>;
    const dim3 grid((unsigned)((n + kKmLabelRows - 1) / kKmLabelRows)), blk(kKmLabelRows);
    const size_t tile = km_stage_bytes(dim, sizeof(T));
    km_zero_words(nsel, 1, s);
    if (tile <= 64 * 1024)
        hipLaunchKernelGGL((km_rerank_kernel<T, M, true>), grid, blk, tile, s, X, n, ld, dim, norms, centres, nc, cand, tau,
                           r.xn, r.xh, r.xl, r.xe, c.cc, sel, nsel, labels, dist);
    else  // (rows too long for LDS: read in place)
        hipLaunchKernelGGL((km_rerank_kernel<T, M, false>), grid, blk, 0, s, X, n, ld, dim, norms, centres, nc, cand, tau, r.xn,
                           r.xh, r.xl, r.xe, c.cc, sel, nsel, labels, dist);
    return hipGetLastError();
}
template <typename T, bool SPH>
hipError_t launch_km_exact(const T *X, size_t n, size_t ld, int dim, const KmNorms<T> &norms, const T *centres, size_t nc,
                           const uint32_t *sel, const uint32_t *nsel, int64_t *labels, T *dist, hipStream_t s) {
    if (n == 0) return hipSuccess;
    using M = KmMetric<T, SPH>;
    if (nc == 0) {
        hipLaunchKernelGGL((km_none_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, labels, dist);
        return hipGetLastError();
    }
    const dim3 grid((unsigned)((n + kKmLabelRows - 1) / kKmLabelRows)), blk(kKmLabelRows);
    const size_t tile = km_stage_bytes(dim, sizeof(T));
    if (tile <= 64 * 1024)
        hipLaunchKernelGGL((km_exact_kernel<T, M, true>), grid, blk, tile, s, X, n, ld, dim, centres, nc, sel, nsel, labels,
                           dist, norms);
    else  // (rows too long for LDS: read in place)
        hipLaunchKernelGGL((km_exact_kernel<T, M, false>), grid, blk, 0, s, X, n, ld, dim, centres, nc, sel, nsel, labels, dist,
                           norms);
    return hipGetLastError();
}
template <typename T, bool SPH>
hipError_t km_update_enqueue(const T *X, size_t n, size_t ld, int dim, const T *rnorm, const int64_t *labels, size_t nc,
                             void *buf, T *centres, uint64_t *counts, double tol, int last, double **stop_out,
                             hipStream_t s) {
    KmMembers m;
    const hipError_t e = km_members_enqueue(labels, n, nc, dim, buf, centres != nullptr, counts, &m, s);
    if (e != hipSuccess) return e;
    if (stop_out) *stop_out = m.stop;
    if (!centres) return hipGetLastError();
    const dim3 grid((unsigned)m.max_segments);
    if (ld % 16 == 0)
        hipLaunchKernelGGL((km_segment_sums_kernel<T, 16, SPH>), grid, dim3(64), 0, s, m.key, m.off, m.seg_off, nc, X, ld, dim,
                           m.segsum, rnorm);
    else
        hipLaunchKernelGGL((km_segment_sums_kernel<T, 8, SPH>), grid, dim3(64), 0, s, m.key, m.off, m.seg_off, nc, X, ld, dim,
                           m.segsum, rnorm);
    KmMetric<T, SPH>::launch_move(m, nc, dim, centres, s);
    return launch_km_stop(m.tc, nc, tol, last, m.stop, s);
}

#define PN_KM_INSTANTIATE(T, SPH)                                                                                            \
    template hipError_t launch_km_pack_rows<T, SPH>(const T *, size_t, size_t, int, const KmRowImage &, hipStream_t);        \
    template hipError_t launch_km_pack_centres<T, SPH>(const T *, size_t, int, const KmCentreImage &, hipStream_t);          \
    template hipError_t launch_km_rerank<T, SPH>(const T *, size_t, size_t, int, const KmNorms<T> &, const T *, size_t,      \
                                                 const uint32_t *, const float *, const KmRowImage &, const KmCentreImage &, \
                                                 uint32_t *, uint32_t *, int64_t *, T *, hipStream_t);                       \
    template hipError_t launch_km_exact<T, SPH>(const T *, size_t, size_t, int, const KmNorms<T> &, const T *, size_t,       \
                                                const uint32_t *, const uint32_t *, int64_t *, T *, hipStream_t);            \
    template hipError_t km_update_enqueue<T, SPH>(const T *, size_t, size_t, int, const T *, const int64_t *, size_t,        \
                                                  void *, T *, uint64_t *, double, int, double **, hipStream_t);

}  // namespace pn
