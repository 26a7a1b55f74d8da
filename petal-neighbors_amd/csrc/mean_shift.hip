// mean_shift.hip -- mean shift over the radius lists (pn_mean_shift_*): the step kernel, the bookkeeping of the active set,
// the merge of the converged modes and the labelling of the rows.  The contract is in the header (petal_mi355x.h) and
// DESIGN.md 4.21; in short, one step of a seed at p with bandwidth h:
//   L    = the list of pn_query_radii_*(p, h), flags 0: ascending row index, strict '<';  m = its length (0: dead)
//   P_l  = (...((0.0 + (double)x[L_l][c]) + (double)x[L_{l+64}][c]) + ...)   for l = 0 .. 63, per column c
//   S_c  = (...((P_0 + P_1) + P_2) ... + P_63)
//   p'_c = (T)(S_c / (double)m)
//   t_c  = ((double)p'_c - (double)p_c)^2, summed in the same 64-partial shape (column c to partial c mod 64); shift = sqrt
// One wave serves one seed.  Lane l strides the list by 64 and reads COLS consecutive columns of each row (8 where the
// rows are padded to 8 elements, else 16), so narrow rows (D = 2 .. 16, the common case) keep every lane busy; wider rows
// take ceil(D / COLS) passes over the list.  The 64 partials of a column are transposed through LDS and lane c folds
// column c's in lane order.
//
// This translation unit is compiled with -ffp-contract=off: every operation is plain IEEE f64 (or T for the distances of
// the merge and the labels, which are the reference metric's fold), unfused.
#include "../../include/petal_mi355x.h"
#include "pn_internal.h"

namespace pn {

namespace {

// columns per pass = f64 partials per lane: rows are padded to 8 elements (D <= 8) or to a multiple of 16 (pick_ld, index.hip)
constexpr int kMsColsNarrow = 8, kMsColsWide = 16;

// (one wave's LDS traffic: the hardware executes a wave's LDS instructions in order, the clobber stops the compiler)
__device__ __forceinline__ void ms_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

template <typename T>
__device__ __forceinline__ T ms_sqrt(T x);
template <>
__device__ __forceinline__ float ms_sqrt<float>(float x) { return sqrtf(x); }  // correctly rounded (build flags)
template <>
__device__ __forceinline__ double ms_sqrt<double>(double x) { return sqrt(x); }

// Euclidean::distance of the reference metric: the bits of pn_euclidean_*
template <typename T>
__device__ __forceinline__ T ms_dist(const T *__restrict__ a, const T *__restrict__ b, int dim) {
#pragma clang fp contract(off)
    T sum = (T)0;
    for (int k = 0; k < dim; ++k) {
        const T diff = a[k] - b[k];
        const T sq = diff * diff;
        sum = sum + sq;
    }
    return ms_sqrt<T>(sum);
}

template <typename T>
__global__ __launch_bounds__(256) void ms_init_kernel(const T *__restrict__ seeds, size_t s_stride, size_t ns, int dim,
                                                      const T *__restrict__ h, size_t n_h, T *__restrict__ pos,
                                                      T *__restrict__ hq, uint32_t *__restrict__ slot) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ns * (size_t)dim) return;
    const size_t i = t / (size_t)dim, c = t - i * (size_t)dim;
    pos[t] = seeds[i * s_stride + c];
    if (c == 0) {
        hq[i] = h[n_h == 1 ? 0 : i];
        slot[i] = (uint32_t)i;
    }
}

// the finish of a dead seed: the position it was queried at, no points, the iterations before this one, NaN
template <typename T>
__device__ __forceinline__ void ms_finish_dead(const MsStep<T> &a, size_t q, int lane) {
    const size_t slot = a.slot[q];
    const T *p = a.pos + q * (size_t)a.dim;
    for (int c = lane; c < a.dim; c += 64) a.modes[slot * (size_t)a.dim + c] = p[c];
    if (lane == 0) {
        a.keep[q] = 0;
        a.points[slot] = 0;
        if (a.iters) a.iters[slot] = a.iter - 1;
        if (a.shift) a.shift[slot] = __longlong_as_double(0x7FF8000000000000ll);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ms_dead_kernel(MsStep<T> a) {
    const int lane = threadIdx.x & 63;
    const size_t q = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.nq) return;
    ms_finish_dead<T>(a, q, lane);
}

// One wave per active seed, four seeds per workgroup; the waves share nothing (no workgroup barrier).
template <typename T, int kMsCols>
__global__ __launch_bounds__(256) void ms_step_kernel(MsStep<T> a) {
#pragma clang fp contract(off)
    __shared__ double s_part[4][kMsCols][65];  // (65: lane c's fold reads column c's row, the rows in different banks)
    __shared__ double s_shift[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t q = (size_t)blockIdx.x * 4 + w;
    if (q >= a.nq) return;  // (the whole wave)
    const uint64_t beg = a.off[q], m = a.off[q + 1] - beg;
    if (m == 0) {
        ms_finish_dead<T>(a, q, lane);
        return;
    }
    const int dim = a.dim;
    T *p = a.pos + q * (size_t)dim;
    const double md = (double)m;
    s_shift[w][lane] = 0.0;
    ms_lds_fence();
    for (int c0 = 0; c0 < dim; c0 += kMsCols) {
        double P[kMsCols];
#pragma unroll
        for (int c = 0; c < kMsCols; ++c) P[c] = 0.0;
        for (uint64_t j = lane; j < m; j += 64) {
            // (c0 + kMsCols <= ld: the row's padding is read, and never used)
            const T *__restrict__ row = a.X + (size_t)(a.idx[beg + j] - a.index_base) * a.ld + c0;
            T v[kMsCols];
#pragma unroll
            for (int c = 0; c < kMsCols; ++c) v[c] = row[c];
#pragma unroll
            for (int c = 0; c < kMsCols; ++c) P[c] = P[c] + (double)v[c];
        }
#pragma unroll
        for (int c = 0; c < kMsCols; ++c) s_part[w][c][lane] = P[c];
        ms_lds_fence();
        const int col = c0 + lane;
        if (lane < kMsCols && col < dim) {
            double S = s_part[w][lane][0];
#pragma unroll 9
            for (int l = 1; l < 64; ++l) S = S + s_part[w][lane][l];
            const T pn = (T)(S / md);
            const double dd = (double)pn - (double)p[col];
            const double t = dd * dd;
            p[col] = pn;
            s_shift[w][col & 63] = s_shift[w][col & 63] + t;
        }
        ms_lds_fence();
    }
    // (every lane folds the same 64 words: LDS broadcasts, and the stop decision is wave-uniform without a readlane)
    double S = s_shift[w][0];
#pragma unroll 9
    for (int l = 1; l < 64; ++l) S = S + s_shift[w][l];
    const double shift = sqrt(S);
    const bool stop = shift <= a.tol || a.last;
    if (lane == 0) a.keep[q] = stop ? 0u : 1u;
    if (stop) {
        __threadfence();  // the new position was written by the column lanes
        const size_t slot = a.slot[q];
        for (int c = lane; c < dim; c += 64) a.modes[slot * (size_t)dim + c] = p[c];
        if (lane == 0) {
            a.points[slot] = m;
            if (a.iters) a.iters[slot] = a.iter;
            if (a.shift) a.shift[slot] = shift;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ms_gather_kernel(const uint32_t *__restrict__ sel, const uint32_t *__restrict__ nsel,
                                                        int dim, const T *__restrict__ pos_in, const T *__restrict__ h_in,
                                                        const uint32_t *__restrict__ slot_in, T *__restrict__ pos_out,
                                                        T *__restrict__ h_out, uint32_t *__restrict__ slot_out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i = t / (size_t)dim, c = t - i * (size_t)dim;
    if (i >= (size_t)*nsel) return;
    const size_t from = sel[i];
    pos_out[t] = pos_in[from * (size_t)dim + c];
    if (c == 0) {
        h_out[i] = h_in[from];
        slot_out[i] = slot_in[from];
    }
}

// ---- the merge.  Ranks: the live seeds by (points_within descending, seed ascending), one 64-bit key; the dead ones
// (points_within = 0) and the padding sort behind them with the all-ones key.
constexpr unsigned long long kMsDeadKey = ~0ull;
constexpr int64_t kMsOpen = -2;  // state of a rank no centre has claimed yet

__global__ __launch_bounds__(256) void ms_rank_keys_kernel(const uint64_t *__restrict__ points, size_t ns, size_t N,
                                                           uint64_t *__restrict__ key, unsigned long long *__restrict__ pair) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    unsigned long long k = kMsDeadKey;
    if (i < ns) {
        const uint64_t pw = points[i];
        if (pw) k = ((unsigned long long)(0x7FFFFFFFull - (pw < 0x7FFFFFFFull ? pw : 0x7FFFFFFFull)) << 32) | (unsigned long long)i;
    }
    key[i] = k;
    pair[i] = i < ns ? (unsigned long long)i : ~0ull;
}
// state[r] <- open (a live rank) or -1 (dead); counters[0] (the number of centres) <- 0
__global__ __launch_bounds__(256) void ms_merge_init_kernel(const uint64_t *__restrict__ key, size_t ns,
                                                            int64_t *__restrict__ state, uint64_t *__restrict__ counters) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r == 0) counters[0] = counters[1] = counters[2] = 0;
    if (r < ns) state[r] = key[r] == kMsDeadKey ? -1 : kMsOpen;
}
// One round's ranks [r0, r0 + kMsMergeRound), one workgroup, thread t for rank r0 + t.  Walking the ranks in order, an
// open rank that no earlier centre of this round claimed is a centre (centres of earlier rounds have claimed theirs in
// their sweeps); it claims the later open ranks of the round within h.  counters: [0] the number of centres, [1] / [2]
// the round's first centre / one past its last.
template <typename T>
__global__ __launch_bounds__(kMsMergeRound) void ms_resolve_kernel(size_t r0, size_t ns,
                                                                   const unsigned long long *__restrict__ pair,
                                                                   const T *__restrict__ modes, int dim, T h,
                                                                   int64_t *__restrict__ state,
                                                                   uint32_t *__restrict__ centre_seed,
                                                                   uint64_t *__restrict__ counters) {
    __shared__ int s_open[kMsMergeRound];
    const int t = threadIdx.x;
    const size_t r = r0 + (size_t)t;
    const bool mine = r < ns && state[r] == kMsOpen;
    const T *my = mine ? modes + (size_t)pair[r] * (size_t)dim : nullptr;
    s_open[t] = mine ? 1 : 0;
    uint64_t nc = counters[0];
    const uint64_t first = nc;
    int64_t claimed = kMsOpen;
    __syncthreads();
    const int lim = ns - r0 < (size_t)kMsMergeRound ? (int)(ns - r0) : kMsMergeRound;
    for (int j = 0; j < lim; ++j) {
        if (s_open[j]) {  // (uniform: settled by the barrier that ended step j - 1)
            if (t == j) {
                claimed = (int64_t)nc;
                centre_seed[nc] = (uint32_t)pair[r];
            } else if (t > j && mine && claimed == kMsOpen) {
                const T d = ms_dist<T>(modes + (size_t)pair[r0 + (size_t)j] * (size_t)dim, my, dim);
                if (d < h) {
                    claimed = (int64_t)nc;
                    s_open[t] = 0;
                }
            }
            ++nc;
        }
        __syncthreads();
    }
    if (mine) state[r] = claimed;
    if (t == 0) {
        counters[0] = nc;
        counters[1] = first;
        counters[2] = nc;
    }
}
// every open rank behind the round against the round's new centres, in centre order: the first within h claims it
template <typename T>
__global__ __launch_bounds__(256) void ms_sweep_kernel(size_t r_from, size_t ns, const unsigned long long *__restrict__ pair,
                                                       const T *__restrict__ modes, int dim, T h,
                                                       int64_t *__restrict__ state, const uint32_t *__restrict__ centre_seed,
                                                       const uint64_t *__restrict__ counters) {
    const uint64_t lo = counters[1], hi = counters[2];
    if (lo == hi) return;  // the round made no centre
    const size_t r = r_from + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ns || state[r] != kMsOpen) return;
    const T *my = modes + (size_t)pair[r] * (size_t)dim;
    for (uint64_t c = lo; c < hi; ++c) {
        const T d = ms_dist<T>(modes + (size_t)centre_seed[c] * (size_t)dim, my, dim);
        if (d < h) {
            state[r] = (int64_t)c;
            return;
        }
    }
}
// the outputs: centre_of_seed by seed, the centres' rows and points compacted in centre order, the count
template <typename T>
__global__ __launch_bounds__(256) void ms_merge_out_kernel(size_t ns, int dim, const unsigned long long *__restrict__ pair,
                                                           const int64_t *__restrict__ state,
                                                           const uint32_t *__restrict__ centre_seed,
                                                           const uint64_t *__restrict__ counters, const T *__restrict__ modes,
                                                           const uint64_t *__restrict__ points, T *__restrict__ centres,
                                                           uint64_t *__restrict__ centre_points,
                                                           int64_t *__restrict__ centre_of_seed,
                                                           uint64_t *__restrict__ n_centres) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nc = counters[0];
    if (i == 0) *n_centres = nc;
    if (i >= ns) return;
    if (centre_of_seed) centre_of_seed[pair[i]] = state[i];
    if (i < nc) {
        const size_t seed = centre_seed[i];
        for (int c = 0; c < dim; ++c) centres[i * (size_t)dim + c] = modes[seed * (size_t)dim + c];
        if (centre_points) centre_points[i] = points[seed];
    }
}

// ---- the labels: one thread per row against every centre, the k-NN pipeline's order of (distance key, index) -- a NaN
// distance is the canonical NaN key, above +inf.  One wave per 64 rows.  STAGED: the wave's rows lie transposed in LDS
// ([dim][65] of T: filled with coalesced reads, read without bank conflicts) -- a thread that reads its row from HBM
// strides by the row length and at 10^6 x 128 against 10^3 centres the call is 2 s of cache misses.  Four centres at a
// time give four independent chains; each distance is still the reference metric's sequential fold.
template <typename T>
__device__ __forceinline__ typename KeyOf<T>::type ms_key(T d) {
    using K = typename KeyOf<T>::type;
    if constexpr (sizeof(T) == 4)
        return d != d ? KeyOf<T>::kNaN : (K)__float_as_uint(d);
    else
        return d != d ? KeyOf<T>::kNaN : (K)__double_as_longlong(d);
}
constexpr int kMsLabelRows = 64, kMsLabelPitch = 65;
template <typename T, bool STAGED>
__global__ __launch_bounds__(kMsLabelRows) void ms_labels_kernel(const T *__restrict__ X, size_t n, size_t ld, int dim,
                                                                 const T *__restrict__ centres, size_t nc, T h, bool orphans,
                                                                 int64_t *__restrict__ labels) {
#pragma clang fp contract(off)
    using K = typename KeyOf<T>::type;
    extern __shared__ __align__(8) unsigned char ms_smem[];
    T *tile = (T *)ms_smem;
    const int lane = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * kMsLabelRows, i = row0 + lane;
    if (STAGED) {
        const int rows = n - row0 < (size_t)kMsLabelRows ? (int)(n - row0) : kMsLabelRows;
        for (int r = 0; r < rows; ++r)
            for (int k = lane; k < dim; k += kMsLabelRows) tile[k * kMsLabelPitch + r] = X[(row0 + r) * ld + k];
        __syncthreads();
    }
    if (i >= n) return;
    const T *row = X + i * ld;
    K best = KeyOf<T>::kMax;
    int64_t lab = -1;
    T best_d = (T)0;
    for (size_t c = 0; c < nc; c += 4) {
        const T *cp[4];
        T sum[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            cp[u] = centres + (c + u < nc ? c + u : nc - 1) * (size_t)dim;  // (past the end: the last centre again, not used)
            sum[u] = (T)0;
        }
        for (int k = 0; k < dim; ++k) {
            const T x = STAGED ? tile[k * kMsLabelPitch + lane] : row[k];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const T diff = cp[u][k] - x;
                const T sq = diff * diff;
                sum[u] = sum[u] + sq;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const T d = ms_sqrt<T>(sum[u]);
            const K key = ms_key<T>(d);
            if (c + u < nc && key < best) {
                best = key;
                lab = (int64_t)(c + u);
                best_d = d;
            }
        }
    }
    if (orphans && lab >= 0 && !(best_d < h)) lab = -1;
    labels[i] = lab;
}

inline dim3 ms_grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
inline size_t ms_sort_len(size_t ns) { return sort_key_pair_len(ns); }

}  // namespace

template <typename T>
hipError_t launch_ms_init(const T *seeds, size_t s_stride, size_t ns, int dim, const T *h, size_t n_h, T *pos, T *hq,
                          uint32_t *slot, hipStream_t s) {
    if (ns == 0) return hipSuccess;
    hipLaunchKernelGGL((ms_init_kernel<T>), ms_grid(ns * (size_t)dim), dim3(256), 0, s, seeds, s_stride, ns, dim, h, n_h, pos,
                       hq, slot);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_ms_step(const MsStep<T> &a, hipStream_t s) {
    if (a.nq == 0) return hipSuccess;
    const dim3 grid((unsigned)((a.nq + 3) / 4));
    if (a.ld % kMsColsWide == 0)
        hipLaunchKernelGGL((ms_step_kernel<T, kMsColsWide>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((ms_step_kernel<T, kMsColsNarrow>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_ms_dead(const MsStep<T> &a, hipStream_t s) {
    if (a.nq == 0) return hipSuccess;
    hipLaunchKernelGGL((ms_dead_kernel<T>), dim3((unsigned)((a.nq + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_ms_gather(const uint32_t *sel, const uint32_t *nsel, size_t n_in, int dim, const T *pos_in, const T *h_in,
                            const uint32_t *slot_in, T *pos_out, T *h_out, uint32_t *slot_out, hipStream_t s) {
    if (n_in == 0) return hipSuccess;
    hipLaunchKernelGGL((ms_gather_kernel<T>), ms_grid(n_in * (size_t)dim), dim3(256), 0, s, sel, nsel, dim, pos_in, h_in,
                       slot_in, pos_out, h_out, slot_out);
    return hipGetLastError();
}

// scratch: key [N], pair [N] (N = sort_key_pair_len(ns)), state [ns], counters [4] (64-bit words), then centre_seed [ns]
// (32-bit): 16 N + 12 ns + 40 bytes
size_t ms_merge_bytes(size_t ns) { return (2 * ms_sort_len(ns) + ns + 4) * 8 + (ns + 2) * 4; }

template <typename T>
hipError_t ms_merge_enqueue(const T *modes, size_t ns, int dim, const uint64_t *points, T h, void *buf, T *centres,
                            uint64_t *centre_points, int64_t *centre_of_seed, uint64_t *n_centres, hipStream_t s) {
    if (ns == 0) return hipMemsetAsync(n_centres, 0, sizeof(uint64_t), s);
    const size_t N = ms_sort_len(ns);
    uint64_t *key = (uint64_t *)buf;
    unsigned long long *pair = (unsigned long long *)(key + N);
    int64_t *state = (int64_t *)(pair + N);
    uint64_t *counters = (uint64_t *)(state + ns);
    uint32_t *centre_seed = (uint32_t *)(counters + 4);
    hipLaunchKernelGGL(ms_rank_keys_kernel, ms_grid(N), dim3(256), 0, s, points, ns, N, key, pair);
    hipError_t e = launch_sort_key_pair_u64(key, pair, N, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ms_merge_init_kernel, ms_grid(ns), dim3(256), 0, s, key, ns, state, counters);
    for (size_t r0 = 0; r0 < ns; r0 += kMsMergeRound) {
        hipLaunchKernelGGL((ms_resolve_kernel<T>), dim3(1), dim3(kMsMergeRound), 0, s, r0, ns, pair, modes, dim, h, state,
                           centre_seed, counters);
        const size_t r_from = r0 + kMsMergeRound;
        if (r_from < ns)
            hipLaunchKernelGGL((ms_sweep_kernel<T>), ms_grid(ns - r_from), dim3(256), 0, s, r_from, ns, pair, modes, dim, h,
                               state, centre_seed, counters);
    }
    hipLaunchKernelGGL((ms_merge_out_kernel<T>), ms_grid(ns), dim3(256), 0, s, ns, dim, pair, state, centre_seed, counters,
                       modes, points, centres, centre_points, centre_of_seed, n_centres);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_ms_labels(const T *X, size_t n, size_t ld, int dim, const T *centres, size_t nc, T h, bool orphans,
                            int64_t *labels, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + kMsLabelRows - 1) / kMsLabelRows)), blk(kMsLabelRows);
    const size_t tile = (size_t)dim * kMsLabelPitch * sizeof(T);
    if (tile <= 64 * 1024)
        hipLaunchKernelGGL((ms_labels_kernel<T, true>), grid, blk, tile, s, X, n, ld, dim, centres, nc, h, orphans, labels);
    else  // (rows too long for LDS: read in place)
        hipLaunchKernelGGL((ms_labels_kernel<T, false>), grid, blk, 0, s, X, n, ld, dim, centres, nc, h, orphans, labels);
    return hipGetLastError();
}

#define PN_MS_INSTANTIATE(T)                                                                                                \
    template hipError_t launch_ms_init<T>(const T *, size_t, size_t, int, const T *, size_t, T *, T *, uint32_t *,          \
                                          hipStream_t);                                                                     \
    template hipError_t launch_ms_step<T>(const MsStep<T> &, hipStream_t);                                                  \
    template hipError_t launch_ms_dead<T>(const MsStep<T> &, hipStream_t);                                                  \
    template hipError_t launch_ms_gather<T>(const uint32_t *, const uint32_t *, size_t, int, const T *, const T *,          \
                                            const uint32_t *, T *, T *, uint32_t *, hipStream_t);                           \
    template hipError_t ms_merge_enqueue<T>(const T *, size_t, int, const uint64_t *, T, void *, T *, uint64_t *, int64_t *, \
                                            uint64_t *, hipStream_t);                                                       \
    template hipError_t launch_ms_labels<T>(const T *, size_t, size_t, int, const T *, size_t, T, bool, int64_t *, hipStream_t);
PN_MS_INSTANTIATE(float)
PN_MS_INSTANTIATE(double)
#undef PN_MS_INSTANTIATE

}  // namespace pn
