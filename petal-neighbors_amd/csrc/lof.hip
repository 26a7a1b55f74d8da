// lof.hip -- Local Outlier Factor over the self-k-NN graph (pn_lof_*, pn_lof_score_*): everything above the k-NN
// pipeline.  The contract is in the header (petal_mi355x.h) and DESIGN.md 4.18; in short, for row i with the list
// (j_0 .. j_{k-1}, d_0 .. d_{k-1}) of pn_query_self_*(k):
//   kdist[i] = d_{k-1}
//   v_t      = NaN if d_t or kdist[j_t] is NaN, else max((double)d_t, (double)kdist[j_t], +0.0)
//   lrd[i]   = 1 / ((0 + v_0 + v_1 + ... + v_{k-1}) / k + 1e-10)           (added in list order)
//   lof[i]   = (0 + lrd[j_0] / lrd[i] + ... + lrd[j_{k-1}] / lrd[i]) / k   (added in list order)
// and a query's score is the same two steps over its pn_query_*(q, k) list, with lrd and kdist of the fitted rows.
//
// The store: the whole graph as [n][k] uint32 ids (no index base) and [n][k] distances of T, packed chunk by chunk from
// the self-query's answers.  Three passes then stream it: pack (write), lrd (read ids + distances, gather kdist), lof
// (read ids, gather lrd).  All of it is HBM-bound copy / gather work; no floating-point atomics, no reduction whose
// shape depends on the launch: every sum is the sequential fold in list order, whatever the group width.
//
// This translation unit is compiled with -ffp-contract=off: the sums and quotients are plain IEEE f64 operations.
#include "pn_internal.h"

namespace pn {

// np.maximum's NaN rule (a NaN operand wins), then the clamp at +0.0 (a Cosine distance a few ulp below 0)
__device__ __forceinline__ double lof_reach(double d, double kd) {
    if (d != d || kd != kd) return __longlong_as_double(0x7FF8000000000000ll);
    const double m = d > kd ? d : kd;
    return m > 0.0 ? m : 0.0;
}

// acc + x_0 + x_1 + ... over the first `cnt` lanes of the caller's group of L lanes, in lane order; every lane of the
// wave runs it with the same cnt, every lane of a group ends with the same sum
__device__ __forceinline__ double lof_fold(double acc, double x, int cnt, int L) {
    for (int u = 0; u < cnt; ++u) {
        const double xu = __shfl(x, u, L);
        acc = acc + xu;
    }
    return acc;
}

// One element per thread: the chunk's answer [nq][k] (ids with the index base, as the self-query writes them) into the
// store at the chunk's rows; the last column is kdist.
template <typename T>
__global__ __launch_bounds__(256) void lof_pack_kernel(const uint64_t *__restrict__ in_idx, const T *__restrict__ in_dist,
                                                       size_t nq, int k, uint64_t index_base, uint32_t *__restrict__ ids,
                                                       T *__restrict__ dist, T *__restrict__ kdist) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nq * (size_t)k) return;
    const T d = in_dist[e];
    ids[e] = (uint32_t)(in_idx[e] - index_base);
    dist[e] = d;
    const size_t q = e / (size_t)k;
    if (e - q * (size_t)k == (size_t)(k - 1)) kdist[q] = d;
}

// Groups of L lanes (a power of two <= 64, groups aligned inside the wave) serve one row each: lane g of a group takes
// the list entries g, g + L, ... -- the store is read coalesced and L gathers per row are in flight at once -- and the
// group's values are then added in list order by lof_fold.  k and L are uniform, so every lane runs the same trips.
template <typename T>
__global__ __launch_bounds__(256) void lof_lrd_kernel(const uint32_t *__restrict__ ids, const T *__restrict__ dist,
                                                      const T *__restrict__ kdist, size_t n, int k, int L,
                                                      double *__restrict__ lrd) {
#pragma clang fp contract(off)
    const int g = threadIdx.x & (L - 1);
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / (size_t)L;
    const bool valid = i < n;
    const size_t row = (valid ? i : 0) * (size_t)k;
    double S = 0.0;
    for (int t0 = 0; t0 < k; t0 += L) {
        const int t = t0 + g;
        double v = 0.0;
        if (valid && t < k) {
            const uint32_t j = ids[row + t];
            const double d = (double)dist[row + t];
            // (an id outside the rows cannot come out of the self-query; it reads nothing and scores NaN)
            const double kd = j < n ? (double)kdist[j] : __longlong_as_double(0x7FF8000000000000ll);
            v = lof_reach(d, kd);
        }
        S = lof_fold(S, v, k - t0 < L ? k - t0 : L, L);
    }
    if (valid && g == 0) lrd[i] = 1.0 / (S / (double)k + 1e-10);
}

__global__ __launch_bounds__(256) void lof_lof_kernel(const uint32_t *__restrict__ ids, const double *__restrict__ lrd,
                                                      size_t n, int k, int L, double *__restrict__ lof) {
#pragma clang fp contract(off)
    const int g = threadIdx.x & (L - 1);
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / (size_t)L;
    const bool valid = i < n;
    const size_t row = (valid ? i : 0) * (size_t)k;
    const double own = lrd[valid ? i : 0];
    double S = 0.0;
    for (int t0 = 0; t0 < k; t0 += L) {
        const int t = t0 + g;
        double v = 0.0;
        if (valid && t < k) {
            const uint32_t j = ids[row + t];
            const double lj = j < n ? lrd[j] : __longlong_as_double(0x7FF8000000000000ll);
            v = lj / own;
        }
        S = lof_fold(S, v, k - t0 < L ? k - t0 : L, L);
    }
    if (valid && g == 0) lof[i] = S / (double)k;
}

// Scoring: the queries' k-NN answer [nq][k] (ids with the index base) against the fit's lrd and kdist.  Both gathers are
// issued together; the first fold gives the query's lrd, the second its score.
template <typename T>
__global__ __launch_bounds__(256) void lof_score_kernel(const uint64_t *__restrict__ q_idx, const T *__restrict__ q_dist,
                                                        size_t nq, int k, int L, uint64_t index_base, size_t n,
                                                        const double *__restrict__ lrd, const T *__restrict__ kdist,
                                                        double *__restrict__ score) {
#pragma clang fp contract(off)
    const int g = threadIdx.x & (L - 1);
    const size_t q = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / (size_t)L;
    const bool valid = q < nq;
    const size_t row = (valid ? q : 0) * (size_t)k;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double S = 0.0;
    for (int t0 = 0; t0 < k; t0 += L) {
        const int t = t0 + g;
        double v = 0.0;
        if (valid && t < k) {
            const uint64_t j = q_idx[row + t] - index_base;
            v = lof_reach((double)q_dist[row + t], j < n ? (double)kdist[j] : nan);
        }
        S = lof_fold(S, v, k - t0 < L ? k - t0 : L, L);
    }
    const double own = 1.0 / (S / (double)k + 1e-10);
    double R = 0.0;
    for (int t0 = 0; t0 < k; t0 += L) {
        const int t = t0 + g;
        double v = 0.0;
        if (valid && t < k) {
            const uint64_t j = q_idx[row + t] - index_base;
            v = (j < n ? lrd[j] : nan) / own;
        }
        R = lof_fold(R, v, k - t0 < L ? k - t0 : L, L);
    }
    if (valid && g == 0) score[q] = R / (double)k;
}

// the smallest power of two that holds the list, at most a wave: one trip for k <= 64
static int lof_group(int k) {
    int L = 1;
    while (L < 64 && L < k) L <<= 1;
    return L;
}
static unsigned lof_grid(size_t rows, int L) {
    const size_t rows_per_block = 256 / (size_t)L;
    return (unsigned)((rows + rows_per_block - 1) / rows_per_block);
}

template <typename T>
hipError_t launch_lof_pack(const uint64_t *in_idx, const T *in_dist, size_t nq, int k, uint64_t index_base,
                           uint32_t *ids, T *dist, T *kdist, hipStream_t s) {
    if (nq == 0 || k <= 0) return hipSuccess;
    hipLaunchKernelGGL((lof_pack_kernel<T>), dim3((unsigned)((nq * (size_t)k + 255) / 256)), dim3(256), 0, s, in_idx,
                       in_dist, nq, k, index_base, ids, dist, kdist);
    return hipGetLastError();
}
template hipError_t launch_lof_pack<float>(const uint64_t *, const float *, size_t, int, uint64_t, uint32_t *, float *,
                                           float *, hipStream_t);
template hipError_t launch_lof_pack<double>(const uint64_t *, const double *, size_t, int, uint64_t, uint32_t *,
                                            double *, double *, hipStream_t);

template <typename T>
hipError_t launch_lof_lrd(const uint32_t *ids, const T *dist, const T *kdist, size_t n, int k, double *lrd,
                          hipStream_t s) {
    if (n == 0 || k <= 0) return hipSuccess;
    const int L = lof_group(k);
    hipLaunchKernelGGL((lof_lrd_kernel<T>), dim3(lof_grid(n, L)), dim3(256), 0, s, ids, dist, kdist, n, k, L, lrd);
    return hipGetLastError();
}
template hipError_t launch_lof_lrd<float>(const uint32_t *, const float *, const float *, size_t, int, double *,
                                          hipStream_t);
template hipError_t launch_lof_lrd<double>(const uint32_t *, const double *, const double *, size_t, int, double *,
                                           hipStream_t);
hipError_t launch_lof_lof(const uint32_t *ids, const double *lrd, size_t n, int k, double *lof, hipStream_t s) {
    if (n == 0 || k <= 0) return hipSuccess;
    const int L = lof_group(k);
    hipLaunchKernelGGL(lof_lof_kernel, dim3(lof_grid(n, L)), dim3(256), 0, s, ids, lrd, n, k, L, lof);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_lof_score(const uint64_t *q_idx, const T *q_dist, size_t nq, int k, uint64_t index_base, size_t n,
                            const double *lrd, const T *kdist, double *score, hipStream_t s) {
    if (nq == 0 || k <= 0) return hipSuccess;
    const int L = lof_group(k);
    hipLaunchKernelGGL((lof_score_kernel<T>), dim3(lof_grid(nq, L)), dim3(256), 0, s, q_idx, q_dist, nq, k, L, index_base, n,
                       lrd, kdist, score);
    return hipGetLastError();
}
template hipError_t launch_lof_score<float>(const uint64_t *, const float *, size_t, int, uint64_t, size_t,
                                            const double *, const float *, double *, hipStream_t);
template hipError_t launch_lof_score<double>(const uint64_t *, const double *, size_t, int, uint64_t, size_t,
                                             const double *, const double *, double *, hipStream_t);

}  // namespace pn
