// knn_predict.hip -- k-NN classification and regression over the k-NN lists (pn_knn_classify_*, pn_knn_regress_*): the
// vote and the weighted mean above the k-NN pipeline.  The contract is in the header (petal_mi355x.h) and DESIGN.md 4.23;
// in short, for a list (j_0 .. j_{k-1}, d_0 .. d_{k-1}) of pn_query_*(q, k) or pn_query_self_*(k):
//   v_t  = d_t > 0 ? (double)d_t : +0.0
//   w_t  = 1                                              (uniform)
//        = some v_u == 0 ? (v_t == 0 ? 1 : 0) : 1 / v_t   (PN_KNN_WEIGHT_DISTANCE)
//   S    = 0 + w_0 + w_1 + ... + w_{k-1}                  (added in list order)
//   W_c  = 0 + the w_t with labels[j_t] == c              (added in list order)
//   pred = the c with the largest W_c, the smallest such c;  proba[c] = W_c / S
//   out[o] = (0 + w_0 * y[j_0][o] + w_1 * y[j_1][o] + ...) / S   (each product rounded, added in list order)
// and a list with a NaN distance -- or, classifying, a label outside [0, n_classes) -- answers -1 / a NaN row.
//
// Everything here is gather work behind the k-NN answer of one pipeline chunk; no floating-point atomics, no reduction
// whose shape depends on the launch: every sum is the sequential fold in list order, whatever the lane layout.  The only
// order-independent step is the winner's comparison on (W descending, class ascending), which is a total order.
//
// This translation unit is compiled with -ffp-contract=off: the sums, products and quotients are plain IEEE f64 operations.
#include "pn_internal.h"

namespace pn {

namespace {

constexpr int kKnnMaxK = 1024;          // the longest list served (the header's limit)
constexpr int kKnnWaveM = kKnnMaxK / 64;  // list entries per lane of the one-wave-per-list kernel

__device__ __forceinline__ double knn_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
// the clamp LOF uses: a Cosine distance a few ulp below 0 (and -0.0) counts as +0.0
__device__ __forceinline__ double knn_clamp(double d) { return d > 0.0 ? d : 0.0; }
// scikit-learn's _get_weights: a list with a zero distance counts its zero-distance entries alone
__device__ __forceinline__ double knn_weight(double v, bool distance, bool zero) {
    if (!distance) return 1.0;
    if (zero) return v == 0.0 ? 1.0 : 0.0;
    return 1.0 / v;
}
// the winner's order: the larger sum, then the smaller class (total: no two candidates of different classes are equal)
__device__ __forceinline__ bool knn_better(double wa, int ca, double wb, int cb) {
    return wa > wb || (wa == wb && ca < cb);
}
// the bits of a wave-wide ballot that belong to the caller's group of L lanes (L a power of two <= 64, groups aligned)
__device__ __forceinline__ bool knn_group_any(bool x, int lane, int L) {
    const unsigned long long m = (L == 64 ? ~0ull : ((1ull << L) - 1ull)) << (lane & ~(L - 1));
    return (__ballot(x) & m) != 0ull;
}

// ---- the vote, k <= 64.  Groups of L lanes (the smallest power of two >= k, groups aligned inside the wave) serve one
// list each; lane g holds entry g: (class, weight).  One serial fold over u broadcasts entry u, and a lane adds w_u where
// the class is its own -- so every lane ends with its own class's W in list order -- and the same loop folds S.  The lane
// that holds a class's first occurrence stores its share into the proba row (zeroed by the launcher).
template <typename T>
__global__ __launch_bounds__(256) void knn_vote_group_kernel(const uint64_t *__restrict__ q_idx, const T *__restrict__ q_dist,
                                                             size_t nq, int k, int L, uint64_t index_base, size_t n,
                                                             const int64_t *__restrict__ labels, int64_t n_classes,
                                                             int distance, int64_t *__restrict__ pred,
                                                             double *__restrict__ proba) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int g = lane & (L - 1);
    const size_t q = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / (size_t)L;
    const bool valid = q < nq;
    const bool has = valid && g < k;
    int c = -1;
    double v = 0.0;
    bool bad = false;
    if (has) {
        const size_t e = q * (size_t)k + (size_t)g;
        const uint64_t j = q_idx[e] - index_base;
        const double d = (double)q_dist[e];
        // (an id outside the rows cannot come out of the query; it reads nothing and poisons the list)
        const int64_t lab = j < n ? labels[j] : -1;
        bad = d != d || lab < 0 || lab >= n_classes;
        c = bad ? -1 : (int)lab;
        v = knn_clamp(d);
    }
    const bool poisoned = knn_group_any(bad, lane, L);
    const bool zero = knn_group_any(has && v == 0.0, lane, L);
    const double w = has ? knn_weight(v, distance != 0, zero) : 0.0;
    double W = 0.0, S = 0.0;
    bool first = true;
    for (int u = 0; u < k; ++u) {
        const int cu = __shfl(c, u, L);
        const double wu = __shfl(w, u, L);
        S = S + wu;
        if (cu == c) {
            W = W + wu;
            if (u < g) first = false;
        }
    }
    double bw = has ? W : -1.0;
    int bc = has ? c : 0x7FFFFFFF;
    for (int m = L >> 1; m > 0; m >>= 1) {
        const double ow = __shfl_xor(bw, m, L);
        const int oc = __shfl_xor(bc, m, L);
        if (knn_better(ow, oc, bw, bc)) {
            bw = ow;
            bc = oc;
        }
    }
    if (!valid) return;
    if (g == 0) pred[q] = poisoned ? (int64_t)-1 : (int64_t)bc;
    if (proba) {
        double *row = proba + q * (size_t)n_classes;
        if (poisoned) {
            for (int64_t cc = g; cc < n_classes; cc += L) row[cc] = knn_nan();
        } else if (has && first) {
            row[c] = W / S;  // (0 <= c < n_classes: a label outside poisons the list and stores nothing here)
        }
    }
}

// ---- the vote, 64 < k <= 1024.  One wave per list; classes and weights staged in LDS (12 bytes per entry, at most 12 KB
// per list).  Lane g owns the entries g, g + 64, ... and walks the whole list once for all of them: the order of every
// sum is the list's, as above.
template <typename T>
__global__ __launch_bounds__(256) void knn_vote_wave_kernel(const uint64_t *__restrict__ q_idx, const T *__restrict__ q_dist,
                                                            size_t nq, int k, uint64_t index_base, size_t n,
                                                            const int64_t *__restrict__ labels, int64_t n_classes,
                                                            int distance, int64_t *__restrict__ pred,
                                                            double *__restrict__ proba) {
#pragma clang fp contract(off)
    __shared__ double s_w[4][kKnnMaxK];
    __shared__ int s_c[4][kKnnMaxK];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t q = (size_t)blockIdx.x * 4 + (size_t)wv;
    const bool valid = q < nq;
    const size_t row0 = (valid ? q : 0) * (size_t)k;
    double *sw = s_w[wv];
    int *sc = s_c[wv];
    bool bad = false, z = false;
    for (int t = lane; t < k; t += 64) {
        int c = -1;
        double v = 0.0;
        if (valid) {
            const uint64_t j = q_idx[row0 + t] - index_base;
            const double d = (double)q_dist[row0 + t];
            const int64_t lab = j < n ? labels[j] : -1;
            const bool b = d != d || lab < 0 || lab >= n_classes;
            bad = bad || b;
            c = b ? -1 : (int)lab;
            v = knn_clamp(d);
            z = z || v == 0.0;
        }
        sc[t] = c;
        sw[t] = v;
    }
    const bool poisoned = __any(bad) != 0;
    const bool zero = __any(z) != 0;
    for (int t = lane; t < k; t += 64) sw[t] = knn_weight(sw[t], distance != 0, zero);  // (the lane's own entries)
    __syncthreads();
    const int nm = (k + 63) >> 6;
    double W[kKnnWaveM];
    int C[kKnnWaveM];
    unsigned later = 0;  // bit m: an earlier entry holds entry m's class
#pragma unroll
    for (int m = 0; m < kKnnWaveM; ++m) {
        const int t = lane + 64 * m;
        C[m] = t < k ? sc[t] : -1;
        W[m] = 0.0;
    }
    double S = 0.0;
    for (int u = 0; u < k; ++u) {
        const int cu = sc[u];
        const double wu = sw[u];
        S = S + wu;
#pragma unroll
        for (int m = 0; m < kKnnWaveM; ++m)
            if (m < nm && cu == C[m]) {
                W[m] = W[m] + wu;
                if (u < lane + 64 * m) later |= 1u << m;
            }
    }
    double bw = -1.0;
    int bc = 0x7FFFFFFF;
#pragma unroll
    for (int m = 0; m < kKnnWaveM; ++m)
        if (lane + 64 * m < k && knn_better(W[m], C[m], bw, bc)) {
            bw = W[m];
            bc = C[m];
        }
    for (int m = 32; m > 0; m >>= 1) {
        const double ow = __shfl_xor(bw, m, 64);
        const int oc = __shfl_xor(bc, m, 64);
        if (knn_better(ow, oc, bw, bc)) {
            bw = ow;
            bc = oc;
        }
    }
    if (!valid) return;
    if (lane == 0) pred[q] = poisoned ? (int64_t)-1 : (int64_t)bc;
    if (proba) {
        double *row = proba + q * (size_t)n_classes;
        if (poisoned) {
            for (int64_t cc = lane; cc < n_classes; cc += 64) row[cc] = knn_nan();
        } else {
#pragma unroll
            for (int m = 0; m < kKnnWaveM; ++m)
                if (lane + 64 * m < k && !(later & (1u << m))) row[C[m]] = W[m] / S;
        }
    }
}

// ---- the mean.  Groups of G lanes (the smallest power of two >= n_out, at most a wave) serve one list each, lanes
// across the outputs: a target row is read coalesced, and the list is walked eight entries at a time -- their gathers are
// issued together, then the products are added one by one.  The first pass finds the NaN and zero distances and folds S.
// One output per list is one lane per list with eight gathers in flight; the vote's group layout (one gather per lane,
// shuffle fold) was measured against this one at n_out = 1 .. 16 and was never faster.
template <typename T>
__global__ __launch_bounds__(256) void knn_mean_row_kernel(const uint64_t *__restrict__ q_idx, const T *__restrict__ q_dist,
                                                           size_t nq, int k, int G, uint64_t index_base, size_t n,
                                                           const double *__restrict__ y, size_t n_out, int distance,
                                                           double *__restrict__ out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int g = lane & (G - 1);
    const size_t q = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / (size_t)G;
    const bool valid = q < nq;
    const size_t row0 = (valid ? q : 0) * (size_t)k;
    bool bad = false, z = false;
    for (int t0 = 0; t0 < k; t0 += G) {
        const int t = t0 + g;
        if (valid && t < k) {
            const uint64_t j = q_idx[row0 + t] - index_base;
            const double d = (double)q_dist[row0 + t];
            bad = bad || d != d || j >= n;
            z = z || knn_clamp(d) == 0.0;
        }
    }
    const bool poisoned = knn_group_any(bad, lane, G);
    const bool zero = knn_group_any(z, lane, G);
    double S = 0.0;
    for (int t0 = 0; t0 < k; t0 += G) {
        const int t = t0 + g;
        const double w = valid && t < k ? knn_weight(knn_clamp((double)q_dist[row0 + t]), distance != 0, zero) : 0.0;
        const int cnt = k - t0 < G ? k - t0 : G;
        for (int u = 0; u < cnt; ++u) S = S + __shfl(w, u, G);
    }
    if (!valid) return;
    for (size_t o = (size_t)g; o < n_out; o += (size_t)G) {
        double N = 0.0;
        if (!poisoned) {
            for (int t0 = 0; t0 < k; t0 += 8) {
                double x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    x[u] = 0.0;
                    if (t0 + u < k) {
                        const size_t j = (size_t)(q_idx[row0 + t0 + u] - index_base);
                        const double w = knn_weight(knn_clamp((double)q_dist[row0 + t0 + u]), distance != 0, zero);
                        x[u] = w * y[j * n_out + o];
                    }
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (t0 + u < k) N = N + x[u];
            }
        }
        out[q * n_out + o] = poisoned ? knn_nan() : N / S;
    }
}

// the smallest power of two that holds `x`, at most a wave
int knn_group(size_t x) {
    int L = 1;
    while (L < 64 && (size_t)L < x) L <<= 1;
    return L;
}
unsigned knn_grid(size_t lists, int L) {
    const size_t per_block = 256 / (size_t)L;
    return (unsigned)((lists + per_block - 1) / per_block);
}

}  // namespace

template <typename T>
hipError_t launch_knn_vote(const uint64_t *q_idx, const T *q_dist, size_t nq, int k, uint64_t index_base, size_t n,
                           const int64_t *labels, size_t n_classes, unsigned flags, int64_t *pred, double *proba,
                           hipStream_t s) {
    if (nq == 0 || k <= 0) return hipSuccess;
    if (k > kKnnMaxK) return hipErrorInvalidValue;
    if (proba) {  // the kernels store the classes a list holds; every other share is 0
        hipError_t e = hipMemsetAsync(proba, 0, nq * n_classes * sizeof(double), s);
        if (e != hipSuccess) return e;
    }
    const int distance = (int)(flags & 1u);
    if (k <= 64) {
        const int L = knn_group((size_t)k);
        hipLaunchKernelGGL((knn_vote_group_kernel<T>), dim3(knn_grid(nq, L)), dim3(256), 0, s, q_idx, q_dist, nq, k, L,
                           index_base, n, labels, (int64_t)n_classes, distance, pred, proba);
    } else {
        hipLaunchKernelGGL((knn_vote_wave_kernel<T>), dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s, q_idx, q_dist, nq, k,
                           index_base, n, labels, (int64_t)n_classes, distance, pred, proba);
    }
    return hipGetLastError();
}
template hipError_t launch_knn_vote<float>(const uint64_t *, const float *, size_t, int, uint64_t, size_t, const int64_t *,
                                           size_t, unsigned, int64_t *, double *, hipStream_t);
template hipError_t launch_knn_vote<double>(const uint64_t *, const double *, size_t, int, uint64_t, size_t,
                                            const int64_t *, size_t, unsigned, int64_t *, double *, hipStream_t);

template <typename T>
hipError_t launch_knn_mean(const uint64_t *q_idx, const T *q_dist, size_t nq, int k, uint64_t index_base, size_t n,
                           const double *targets, size_t n_out, unsigned flags, double *out, hipStream_t s) {
    if (nq == 0 || k <= 0 || n_out == 0) return hipSuccess;
    const int distance = (int)(flags & 1u);
    const int G = knn_group(n_out);
    hipLaunchKernelGGL((knn_mean_row_kernel<T>), dim3(knn_grid(nq, G)), dim3(256), 0, s, q_idx, q_dist, nq, k, G, index_base,
                       n, targets, n_out, distance, out);
    return hipGetLastError();
}
template hipError_t launch_knn_mean<float>(const uint64_t *, const float *, size_t, int, uint64_t, size_t, const double *,
                                           size_t, unsigned, double *, hipStream_t);
template hipError_t launch_knn_mean<double>(const uint64_t *, const double *, size_t, int, uint64_t, size_t, const double *,
                                            size_t, unsigned, double *, hipStream_t);

}  // namespace pn
