// kmeans_nearest.hip -- the m nearest centres of every indexed row (pn_kmeans_nearest_*), 1 <= m <= 8, behind the bf16
// MFMA filter of k-means.  The contract is in the header (petal_mi355x.h), the design in DESIGN.md 4.27.
//
// Slot j of row i holds the centre that is j-th by (distance key, centre number), the distance being the reference
// metric's sequential fold in T: column 0 is pn_kmeans_assign_*'s answer.  The operands, the MFMA chain and hence the
// bound are those of kmeans.hip (its header states them): key(x, c) = fl32(cn(c) - 2 S(x, c)) and
//   L(x, c) = xn(x) + key(x, c) - E(x) <= |x - c|^2.
// What is new is what the filter keeps.  Per lane it carries the M + 1 smallest keys seen so far, ascending, the first M
// with their centre (M = m rounded up to 2, 4 or 8).  For the caller's m it hands over the centres of the m smallest
// keys and tau = the (m + 1)-th smallest key: every centre outside those m has key >= tau, so L >= xn + tau - E.  The re-rank
// folds the m candidates in the reference's order, sorts them by (key, number) and takes d_m, the largest of them; the
// row is PROVEN when
//   (xn + tau - E) (1 - (D + 4) u) - 1e-37 > ((d_m + succ d_m) / 2)^2          (u = 2^-24 | 2^-53)
// -- then no centre outside the list can tie or beat the m-th, and the order inside the list is exact because every
// member was folded.  Rows that are not proven are listed on the device and the exact kernel, a fold of every centre
// with a register top-M, answers them; it is also the whole engine where the filter is not used.
//
// The filter stages every tile of 32 centres in LDS once per workgroup (kmeans.hip has each wave read it from L1 / L2),
// in two buffers where they fit: the next tile's global loads are issued before the current tile's chain and land in
// registers behind it.
//
// This translation unit is compiled with -ffp-contract=off: every operation outside the MFMA is plain IEEE, unfused.
#include "../../include/petal_mi355x.h"
#include "pn_internal.h"
#include "km_filter.h"  // the MFMA chain, the row tile, the fold's helpers and the proof

namespace pn {

namespace {

constexpr int kKnCentreTile = 32, kKnMaxDp = 320, kKnFourWaveDp = 240;
constexpr size_t kKnLdsMax = 160 * 1024;
constexpr uint32_t kKnNone = 0xFFFFFFFFu;

// the distance of a key (a NaN comes back as the canonical one)
__device__ __forceinline__ float kn_dist(uint32_t k) { return __uint_as_float(k); }
__device__ __forceinline__ double kn_dist(uint64_t k) { return __longlong_as_double((long long)k); }

// A sorted list in registers: NK keys ascending, the first NC of them with a number.  The caller has seen
// key < k[NK - 1]; a key equal to one in the list goes behind it.  Fully unrolled, no index is a runtime value.
template <typename KT, int NK, int NC>
__device__ __forceinline__ void kn_insert(KT (&k)[NK], uint32_t (&c)[NC], KT key, uint32_t id) {
#pragma unroll
    for (int j = NK - 1; j >= 1; --j) {
        const bool up = key < k[j - 1], here = key < k[j];
        if (j < NC) c[j] = up ? c[j - 1] : (here ? id : c[j]);
        k[j] = up ? k[j - 1] : (here ? key : k[j]);
    }
    const bool first = key < k[0];
    c[0] = first ? id : c[0];
    k[0] = first ? key : k[0];
}

// ---- the filter.  A workgroup of WAVES waves takes 32 WAVES rows, a wave 32 of them.  LDS: the rows' two images
// [2][32 WAVES][dp + 8] (the B operands), then nbuf centre buffers [2][32][dp + 8] (the A operands: both images of one
// tile of 32 centres, in the rows' padded pitch).  The accumulator has the ROW on the lane (column lane & 31) and 16
// centres in the registers, as in km_assign_filter_kernel; K runs in steps of 16 columns, three MFMAs per step on one
// accumulator, at most 60 in a chain (dp <= 320).
// A tile's 64 (dp / 8) chunks of 16 bytes are spread over the threads, at most kPre per thread: the loads of tile t + 1
// are issued before the chain of tile t, held in registers, and written to the other buffer behind the scan (one
// buffer: behind a barrier).  cand [n][M] <- the centres of the row's M smallest keys, ascending by key (0xFFFFFFFF: an
// empty slot); tau [n] <- the (m + 1)-th smallest key, +inf where there is none.  1 <= m <= M.
template <int M, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void km_nearest_filter_kernel(const uint16_t *__restrict__ ximg,
                                                                       const uint16_t *__restrict__ xlo, size_t n, int dp,
                                                                       const uint16_t *__restrict__ cimg,
                                                                       const uint16_t *__restrict__ clo,
                                                                       const float *__restrict__ cn, size_t nc_pad, int nbuf,
                                                                       int m, uint32_t *__restrict__ cand,
                                                                       float *__restrict__ tau) {
    extern __shared__ __align__(16) unsigned char kn_smem[];
    constexpr int kRows = 32 * WAVES, kThreads = 64 * WAVES;
    constexpr int kPre = (64 * ((WAVES == 4 ? kKnFourWaveDp : kKnMaxDp) / 8) + kThreads - 1) / kThreads;
    const int pitch = dp + 8;  // elements
    uint16_t *tile = (uint16_t *)kn_smem, *tile_lo = tile + (size_t)kRows * pitch;
    uint16_t *cbuf = tile_lo + (size_t)kRows * pitch;
    const int cbuf_len = 64 * pitch;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 31, h = lane >> 5;
    const size_t row0 = (size_t)blockIdx.x * kRows;  // (the images have whole tiles of 128 rows: rows beyond n are zeros)
    const int chunks = dp >> 3, half = 32 * chunks, total = 64 * chunks;
    km_load_row_tile<kThreads>(tile, tile_lo, ximg, xlo, row0, kRows, dp, t);
    // this thread's chunks of a centre tile: chunk q of the 64 image rows [hi 0 .. 31 | lo 0 .. 31] lies at q * 8 of the
    // packed tile (whole rows, contiguous) and at (q + q / chunks) * 8 of a buffer (the pitch)
    int dst[kPre];
    u32x4 pre[kPre];
#pragma unroll
    for (int i = 0; i < kPre; ++i) {
        const int q = t + i * kThreads;
        dst[i] = (q + q / chunks) * 8;
    }
    auto fetch = [&](size_t ct) {
#pragma unroll
        for (int i = 0; i < kPre; ++i) {
            const int q = t + i * kThreads;
            if (q < total) {
                const uint16_t *src = q < half ? cimg + ct * (size_t)dp + (size_t)q * 8
                                               : clo + ct * (size_t)dp + (size_t)(q - half) * 8;
                pre[i] = *(const u32x4 *)src;
            }
        }
    };
    auto stash = [&](uint16_t *buf) {
#pragma unroll
        for (int i = 0; i < kPre; ++i)
            if (t + i * kThreads < total) *(u32x4 *)(buf + dst[i]) = pre[i];
    };
    fetch(0);
    stash(cbuf);
    __syncthreads();
    const uint16_t *brow = tile + (size_t)(w * 32 + r) * pitch + h * 8;
    const uint16_t *brow_lo = tile_lo + (size_t)(w * 32 + r) * pitch + h * 8;
    const int ksteps = dp >> 4;
    const float inf = __uint_as_float(0x7F800000u);
    float k[M + 1];
    uint32_t c[M];
#pragma unroll
    for (int j = 0; j <= M; ++j) k[j] = inf;
#pragma unroll
    for (int j = 0; j < M; ++j) c[j] = kKnNone;
    int cur = 0;
    for (size_t ct = 0; ct < nc_pad; ct += kKnCentreTile) {
        const bool more = ct + kKnCentreTile < nc_pad;
        if (more) fetch(ct + kKnCentreTile);
        const uint16_t *arow = cbuf + (size_t)cur * cbuf_len + (size_t)r * pitch + h * 8;
        const f32x16 acc = km_mfma_chain(arow, arow + (size_t)32 * pitch, brow, brow_lo, ksteps);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const size_t cb = ct + (size_t)(8 * g + 4 * h);
            const float4 cn4 = *(const float4 *)(cn + cb);
            const float cnv[4] = {cn4.x, cn4.y, cn4.z, cn4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float key = cnv[j] - 2.0f * acc[4 * g + j];
                if (key < k[M]) kn_insert<float, M + 1, M>(k, c, key, (uint32_t)(cb + j));
            }
        }
        if (nbuf == 1) __syncthreads();  // (every wave has read the one buffer)
        const int nxt = nbuf == 2 ? cur ^ 1 : 0;
        if (more) stash(cbuf + (size_t)nxt * cbuf_len);  // (two buffers: the other one was last read before the barrier below)
        __syncthreads();
        cur = nxt;
    }
    // the other half of the row's centres: the list of the lane 32 away, key by key.  Its last key has no centre, and
    // needs none: its own M keys go in before it, so it can only become the last key here.
    float pk[M + 1];
    uint32_t pc[M];
#pragma unroll
    for (int j = 0; j <= M; ++j) pk[j] = __shfl_xor(k[j], 32, 64);
#pragma unroll
    for (int j = 0; j < M; ++j) pc[j] = (uint32_t)__shfl_xor((int)c[j], 32, 64);
#pragma unroll
    for (int j = 0; j < M; ++j)
        if (pk[j] < k[M]) kn_insert<float, M + 1, M>(k, c, pk[j], pc[j]);
    if (pk[M] < k[M]) k[M] = pk[M];
    const size_t my_row = row0 + (size_t)(w * 32 + r);
    if (h == 0 && my_row < n) {
        float tv = k[M];
#pragma unroll
        for (int j = 1; j < M; ++j)
            if (j == m) tv = k[j];
#pragma unroll
        for (int j = 0; j < M; ++j) cand[my_row * M + j] = c[j];
        tau[my_row] = tv;
    }
}

// slot j of a row's answer; id 0xFFFFFFFF: there is no such centre (label -1, NaN)
template <typename T>
__device__ __forceinline__ void kn_write(int64_t *__restrict__ labels, T *__restrict__ dist, size_t at, uint32_t id,
                                         typename KeyOf<T>::type key) {
    labels[at] = id == kKnNone ? (int64_t)-1 : (int64_t)id;
    if (dist) dist[at] = kn_dist(id == kKnNone ? KeyOf<T>::kNaN : key);
}

// ---- the exact kernel: the fold of km_exact_kernel with a register top-M by (key, number) -- the centres come in
// ascending number and a key equal to one in the list goes behind it.  sel / nsel (nullable together): thread j of the
// launch answers row sel[j], j < *nsel (the grid is sized for n).  labels / dist [n][m], m <= M; slots at and beyond nc:
// -1 and NaN (nc == 0: every slot).
template <typename T, int M>
__global__ __launch_bounds__(kKmLabelRows) void km_nearest_exact_kernel(const T *__restrict__ X, size_t n, size_t ld, int dim,
                                                                   const T *__restrict__ centres, size_t nc, int m,
                                                                   int staged, const uint32_t *__restrict__ sel,
                                                                   const uint32_t *__restrict__ nsel,
                                                                   int64_t *__restrict__ labels, T *__restrict__ dist) {
#pragma clang fp contract(off)
    using K = typename KeyOf<T>::type;
    extern __shared__ __align__(16) unsigned char kn_smem[];
    T *tile = (T *)kn_smem;
    const int lane = threadIdx.x;
    const size_t count = sel ? (size_t)*nsel : n;
    const size_t first = (size_t)blockIdx.x * kKmLabelRows, j = first + lane;
    if (first >= count) return;  // (the whole workgroup)
    if (staged) {
        const int rows = count - first < (size_t)kKmLabelRows ? (int)(count - first) : kKmLabelRows;
        km_stage_rows<T>(X, ld, dim, sel, first, rows, lane, tile);
    }
    if (j >= count) return;
    const size_t i = sel ? (size_t)sel[j] : j;
    const T *row = X + i * ld;
    K key[M];
    uint32_t id[M];
#pragma unroll
    for (int s = 0; s < M; ++s) {
        key[s] = KeyOf<T>::kMax;
        id[s] = kKnNone;
    }
    for (size_t c = 0; c < nc; c += 4) {
        const T *cp[4];
        T sum[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            cp[u] = centres + (c + u < nc ? c + u : nc - 1) * (size_t)dim;  // (past the end: the last centre again, not used)
            sum[u] = (T)0;
        }
        // (one loop per source of the row, chosen outside it)
        auto fold = [&](auto in_lds) {
            for (int k = 0; k < dim; ++k) {
                const T x = decltype(in_lds)::value ? tile[k * kKmLabelPitch + lane] : row[k];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const T diff = cp[u][k] - x;
                    const T sq = diff * diff;
                    sum[u] = sum[u] + sq;
                }
            }
        };
        if (staged)
            fold(std::true_type{});
        else
            fold(std::false_type{});
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const K kk = km_dist_key<T>(km_sqrt<T>(sum[u]));
            if (c + u < nc && kk < key[M - 1]) kn_insert<K, M, M>(key, id, kk, (uint32_t)(c + u));
        }
    }
#pragma unroll
    for (int s = 0; s < M; ++s)
        if (s < m) kn_write<T>(labels, dist, i * (size_t)m + s, id[s], key[s]);
}

// ---- re-rank and proof: one thread per row, the wave's rows staged as above.  The row's m candidates in the
// reference's fold, all at once (slots m .. M - 1 fold the first candidate again and are not used), sorted by (key,
// number) in an odd-even network; proven rows are answered here, the others are listed: slot = atomicAdd(nsel),
// sel[slot] = row.  Never proven: a flagged row or call, an empty slot among the m, an infinite or NaN d_m.
template <typename T, int M>
__global__ __launch_bounds__(kKmLabelRows) void km_nearest_rerank_kernel(const T *__restrict__ X, size_t n, size_t ld, int dim,
                                                                    const T *__restrict__ centres, size_t nc, int m,
                                                                    int staged, const uint32_t *__restrict__ cand,
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
    extern __shared__ __align__(16) unsigned char kn_smem[];
    T *tile = (T *)kn_smem;
    const int lane = threadIdx.x;
    const size_t first = (size_t)blockIdx.x * kKmLabelRows, i = first + lane;
    if (staged) {
        const int rows = n - first < (size_t)kKmLabelRows ? (int)(n - first) : kKmLabelRows;
        km_stage_rows<T>(X, ld, dim, nullptr, first, rows, lane, tile);
    }
    if (i >= n) return;
    const double xnr = xn[i];
    bool ok = cc[4] == 0 && xnr == xnr;
    uint32_t id[M];
#pragma unroll
    for (int s = 0; s < M; ++s) {
        id[s] = s < m ? cand[i * M + s] : kKnNone;
        if (s < m && (size_t)id[s] >= nc) ok = false;
    }
    if (ok) {
        const T *row = X + i * ld;
        const T *cp[M];
        T sum[M];
        K key[M];
#pragma unroll
        for (int s = 0; s < M; ++s) {
            cp[s] = centres + (size_t)(s < m ? id[s] : id[0]) * (size_t)dim;
            sum[s] = (T)0;
        }
        auto fold = [&](auto in_lds) {
            for (int k = 0; k < dim; ++k) {
                const T x = decltype(in_lds)::value ? tile[k * kKmLabelPitch + lane] : row[k];
#pragma unroll
                for (int s = 0; s < M; ++s) {
                    const T diff = cp[s][k] - x;
                    const T sq = diff * diff;
                    sum[s] = sum[s] + sq;
                }
            }
        };
        if (staged)
            fold(std::true_type{});
        else
            fold(std::false_type{});
#pragma unroll
        for (int s = 0; s < M; ++s) key[s] = s < m ? km_dist_key<T>(km_sqrt<T>(sum[s])) : KeyOf<T>::kMax;
        // (the slots beyond m: the largest key and the largest number, so they stay behind)
#pragma unroll
        for (int round = 0; round < M; ++round) {
#pragma unroll
            for (int s = round & 1; s + 1 < M; s += 2) {
                const bool swap = key[s + 1] < key[s] || (key[s + 1] == key[s] && id[s + 1] < id[s]);
                const K ka = key[s], kb = key[s + 1];
                const uint32_t ia = id[s], ib = id[s + 1];
                key[s] = swap ? kb : ka;
                key[s + 1] = swap ? ka : kb;
                id[s] = swap ? ib : ia;
                id[s + 1] = swap ? ia : ib;
            }
        }
        K kk = key[0];  // d_m: the largest of the m
#pragma unroll
        for (int s = 1; s < M; ++s)
            if (s == m - 1) kk = key[s];
        const float tv = tau[i];
        ok = km_euclid_proven<T>(kk, tv, dim, [&] {
            return km_tau_floor(xnr, (double)tv, km_row_slack((double)xh[i], (double)xl[i], (double)xe[i], cc));
        });
        if (ok) {
#pragma unroll
            for (int s = 0; s < M; ++s)
                if (s < m) kn_write<T>(labels, dist, i * (size_t)m + s, id[s], key[s]);
        }
    }
    if (!ok) {
        const uint32_t slot = atomicAdd(nsel, 1u);
        sel[slot] = (uint32_t)i;  // (slot < n: every row is listed at most once)
    }
}

// waves per workgroup, centre buffers and the LDS of a launch: the most that fits 160 KiB
struct KnPlan {
    int waves, nbuf;
    size_t lds;
};
inline KnPlan kn_plan(int dp) {
    const size_t p = (size_t)(dp + 8);  // (a row of 128 rows' two images: 512 p bytes; a centre buffer: 128 p)
    if (768 * p <= kKnLdsMax) return {4, 2, 768 * p};
    if (640 * p <= kKnLdsMax) return {4, 1, 640 * p};
    if (512 * p <= kKnLdsMax) return {2, 2, 512 * p};
    return {2, 1, 384 * p};
}
static_assert(640 * (size_t)(kKnFourWaveDp + 8) <= kKnLdsMax && 640 * (size_t)(kKnFourWaveDp + 24) > kKnLdsMax,
              "kKnFourWaveDp is the widest row four waves take");
static_assert(384 * (size_t)(kKnMaxDp + 8) <= kKnLdsMax, "the widest row fits two waves and one buffer");

template <int M, int WAVES>
hipError_t kn_filter_launch(const KmRowImage &r, size_t n, const KmCentreImage &c, const KnPlan &plan, int m, uint32_t *cand,
                            float *tau, hipStream_t s) {
    static LdsAttrOnce once;
    if (plan.lds > 64 * 1024) {
        // (the most a plan of these waves asks for: 640 * 248 at four, 512 * 312 at two)
        const hipError_t e = once.ensure((const void *)km_nearest_filter_kernel<M, WAVES>,
                                         WAVES == 4 ? 640 * (size_t)(kKnFourWaveDp + 8) : 512 * (size_t)(kKnMaxDp - 8));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((km_nearest_filter_kernel<M, WAVES>), dim3((unsigned)(r.n_img / (32 * WAVES))), dim3(64 * WAVES),
                       plan.lds, s, r.img, r.lo, n, r.dp, c.img, c.lo, c.cn, c.nc_pad, plan.nbuf, m, cand, tau);
    return hipGetLastError();
}

template <int M>
hipError_t kn_filter_width(const KmRowImage &r, size_t n, const KmCentreImage &c, int m, uint32_t *cand, float *tau,
                           hipStream_t s) {
    const KnPlan plan = kn_plan(r.dp);
    return plan.waves == 4 ? kn_filter_launch<M, 4>(r, n, c, plan, m, cand, tau, s)
                           : kn_filter_launch<M, 2>(r, n, c, plan, m, cand, tau, s);
}

}  // namespace

int km_nearest_width(size_t m) { return m <= 2 ? 2 : m <= 4 ? 4 : 8; }

hipError_t launch_km_nearest_filter(const KmRowImage &r, size_t n, const KmCentreImage &c, size_t nc, int m, uint32_t *cand,
                                    float *tau, hipStream_t s) {
    if (n == 0 || nc == 0) return hipSuccess;
    if (r.dp > kKnMaxDp || r.n_img % 128 != 0 || c.nc_pad % kKnCentreTile != 0) return hipErrorInvalidValue;
    switch (km_nearest_width((size_t)m)) {
        case 2: return kn_filter_width<2>(r, n, c, m, cand, tau, s);
        case 4: return kn_filter_width<4>(r, n, c, m, cand, tau, s);
        default: return kn_filter_width<8>(r, n, c, m, cand, tau, s);
    }
}

template <typename T>
hipError_t launch_km_nearest_rerank(const T *X, size_t n, size_t ld, int dim, const T *centres, size_t nc, int m,
                                    const uint32_t *cand, const float *tau, const KmRowImage &r, const KmCentreImage &c,
                                    uint32_t *sel, uint32_t *nsel, int64_t *labels, T *dist, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + kKmLabelRows - 1) / kKmLabelRows)), blk(kKmLabelRows);
    const size_t bytes = km_stage_bytes(dim, sizeof(T));
    const int staged = bytes <= 64 * 1024;  // (rows too long for LDS: read in place)
    const size_t lds = staged ? bytes : 0;
    km_zero_words(nsel, 1, s);
#define PN_KN_RERANK(M)                                                                                                      \
    hipLaunchKernelGGL((km_nearest_rerank_kernel<T, M>), grid, blk, lds, s, X, n, ld, dim, centres, nc, m, staged, cand, tau, \
                       r.xn, r.xh, r.xl, r.xe, c.cc, sel, nsel, labels, dist)
    switch (km_nearest_width((size_t)m)) {
        case 2: PN_KN_RERANK(2); break;
        case 4: PN_KN_RERANK(4); break;
        default: PN_KN_RERANK(8); break;
    }
#undef PN_KN_RERANK
    return hipGetLastError();
}

template <typename T>
hipError_t launch_km_nearest_exact(const T *X, size_t n, size_t ld, int dim, const T *centres, size_t nc, int m,
                                   const uint32_t *sel, const uint32_t *nsel, int64_t *labels, T *dist, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + kKmLabelRows - 1) / kKmLabelRows)), blk(kKmLabelRows);
    const size_t bytes = km_stage_bytes(dim, sizeof(T));
    const int staged = bytes <= 64 * 1024;
    const size_t lds = staged ? bytes : 0;
#define PN_KN_EXACT(M)                                                                                                     \
    hipLaunchKernelGGL((km_nearest_exact_kernel<T, M>), grid, blk, lds, s, X, n, ld, dim, centres, nc, m, staged, sel, nsel, \
                       labels, dist)
    switch (km_nearest_width((size_t)m)) {
        case 2: PN_KN_EXACT(2); break;
        case 4: PN_KN_EXACT(4); break;
        default: PN_KN_EXACT(8); break;
    }
#undef PN_KN_EXACT
    return hipGetLastError();
}

#define PN_KN_INSTANTIATE(T)                                                                                                 \
    template hipError_t launch_km_nearest_rerank<T>(const T *, size_t, size_t, int, const T *, size_t, int, const uint32_t *, \
                                                    const float *, const KmRowImage &, const KmCentreImage &, uint32_t *,    \
                                                    uint32_t *, int64_t *, T *, hipStream_t);                                \
    template hipError_t launch_km_nearest_exact<T>(const T *, size_t, size_t, int, const T *, size_t, int, const uint32_t *,  \
                                                   const uint32_t *, int64_t *, T *, hipStream_t);
PN_KN_INSTANTIATE(float)
PN_KN_INSTANTIATE(double)
#undef PN_KN_INSTANTIATE

}  // namespace pn
