// kde.hip -- kernel density sums over the radius lists (pn_kde_*): everything above the radius pipeline.  The contract is
// in the header (petal_mi355x.h) and DESIGN.md 4.20; in short, for query q with bandwidth h_q:
//   c_q  = the cutoff: h_q for the compact kernels, h_q * f rounded upward for the smooth ones (f from n and atol)
//   L_q  = the list of pn_query_radii_with_distance_*(q, c_q), flags 0: ascending row index, strict '<'
//   t_j  = the kernel's term of list entry j, in f64, d = max((double)dist, +0.0), h = (double)h_q
//   P_l  = (...((0.0 + t_l) + t_{l+64}) + t_{l+128} ...)    for l = 0 .. 63
//   S    = (...((P_0 + P_1) + P_2) ... + P_63)
// One wave serves one query: lane l strides the list by 64, then the 64 partials are folded in lane order.  The shape of
// the sum depends on the list's length alone -- no floating-point atomics, no reduction that depends on the launch.
//
// This translation unit is compiled with -ffp-contract=off: terms and sums are plain IEEE f64 operations, exp is the
// device library's double-precision exp.
#include "pn_internal.h"

namespace pn {

// c_q and the broadcast h_q.  mode: 0 = compact kernel (c = h); 1 = smooth kernel with a finite positive factor f
// (c = the smallest T >= (double)h * f); 2 = atol >= n (c = 0, the list is empty); 3 = atol = 0 (c = +inf).  A bandwidth
// that is not positive (or NaN) is its own cutoff in every mode: such a radius gives an empty list.
template <typename T>
__global__ __launch_bounds__(256) void kde_cutoff_kernel(const T *__restrict__ h, size_t n_h, size_t nq, int mode, double f,
                                                         T *__restrict__ hq, T *__restrict__ cut) {
#pragma clang fp contract(off)
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const T hv = h[n_h == 1 ? 0 : q];
    T c = hv;
    if (hv > (T)0) {
        if (mode == 1) {
            const double x = (double)hv * f;
            c = (T)x;  // (to nearest; a product beyond T's range gives +inf)
            if ((double)c < x) {
                if constexpr (sizeof(T) == 4)
                    c = nextafterf(c, __uint_as_float(0x7F800000u));
                else
                    c = nextafter(c, __longlong_as_double(0x7FF0000000000000ll));
            }
        } else if (mode == 2) {
            c = (T)0;
        } else if (mode == 3) {
            if constexpr (sizeof(T) == 4)
                c = __uint_as_float(0x7F800000u);
            else
                c = __longlong_as_double(0x7FF0000000000000ll);
        }
    }
    hq[q] = hv;
    cut[q] = c;
}

// count[q] = off[q + 1] - off[q]
__global__ __launch_bounds__(256) void kde_counts_kernel(const uint64_t *__restrict__ off, size_t nq,
                                                         uint64_t *__restrict__ count) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) count[q] = off[q + 1] - off[q];
}

__device__ __forceinline__ double kde_term(int kernel, double d, double h) {
#pragma clang fp contract(off)
    switch (kernel) {
        case 1: return 1.0;                                  // tophat
        case 2: return 1.0 - (d * d) / (h * h);              // epanechnikov
        case 4: return 1.0 - d / h;                          // linear
        case 3: return exp(-(d / h));                        // exponential
        default: return exp(-((d * d) / (2.0 * (h * h))));   // gaussian
    }
}

// lane l's value of x, as a wave-uniform double (l is uniform)
__device__ __forceinline__ double kde_lane(double x, int l) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// One wave per query, four queries per workgroup.  off [nq + 1]: the piece's own offsets into dist / idx (the inner radius
// call's).  own_first != ~0: query q is indexed row own_first + q (ids with the index base) and its own entry is left
// out of the list -- the list is in ascending row index, so the entry is found by bisection and the positions behind it
// move up by one.  count (nullable) gets the number of terms.
template <typename T>
__global__ __launch_bounds__(256) void kde_sum_kernel(const uint64_t *__restrict__ off, const uint64_t *__restrict__ idx,
                                                      const T *__restrict__ dist, const T *__restrict__ hq, size_t nq,
                                                      int kernel, uint64_t own_first, double *__restrict__ sum,
                                                      uint64_t *__restrict__ count) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const size_t q = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;  // (the whole wave)
    const uint64_t beg = off[q], end = off[q + 1];
    uint64_t m = end - beg, skip = m;  // skip: the raw position left out (m: none)
    if (own_first != ~0ull) {
        const uint64_t own = own_first + q;
        uint64_t lo = 0, hi = m;  // the first position whose id is >= own
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (idx[beg + mid] < own)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lo < m && idx[beg + lo] == own) {
            skip = lo;
            m -= 1;
        }
    }
    const double h = (double)hq[q];
    double P = 0.0;
    for (uint64_t j = lane; j < m; j += 64) {
        const double dv = (double)dist[beg + j + (j >= skip ? 1 : 0)];
        const double d = dv > 0.0 ? dv : 0.0;  // (a Cosine distance a few ulp below 0; -0.0 becomes +0.0)
        P = P + kde_term(kernel, d, h);
    }
    // (lanes 1 .. 63 in nine trips of seven: unrolled whole, the 128 scalar registers of the partials are all live at once
    // and spill)
    double S = kde_lane(P, 0);
#pragma unroll 1
    for (int l0 = 1; l0 < 64; l0 += 7) {
#pragma unroll
        for (int l = 0; l < 7; ++l) S = S + kde_lane(P, l0 + l);
    }
    if (lane == 0) {
        sum[q] = S;
        if (count) count[q] = m;
    }
}

template <typename T>
hipError_t launch_kde_cutoff(const T *h, size_t n_h, size_t nq, int mode, double f, T *hq, T *cut, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL((kde_cutoff_kernel<T>), dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, h, n_h, nq, mode, f, hq,
                       cut);
    return hipGetLastError();
}
template hipError_t launch_kde_cutoff<float>(const float *, size_t, size_t, int, double, float *, float *, hipStream_t);
template hipError_t launch_kde_cutoff<double>(const double *, size_t, size_t, int, double, double *, double *, hipStream_t);

hipError_t launch_kde_counts(const uint64_t *off, size_t nq, uint64_t *count, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(kde_counts_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, off, nq, count);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_kde_sum(const uint64_t *off, const uint64_t *idx, const T *dist, const T *hq, size_t nq, int kernel,
                          uint64_t own_first, double *sum, uint64_t *count, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL((kde_sum_kernel<T>), dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s, off, idx, dist, hq, nq, kernel,
                       own_first, sum, count);
    return hipGetLastError();
}
template hipError_t launch_kde_sum<float>(const uint64_t *, const uint64_t *, const float *, const float *, size_t, int,
                                          uint64_t, double *, uint64_t *, hipStream_t);
template hipError_t launch_kde_sum<double>(const uint64_t *, const uint64_t *, const double *, const double *, size_t, int,
                                           uint64_t, double *, uint64_t *, hipStream_t);

}  // namespace pn
