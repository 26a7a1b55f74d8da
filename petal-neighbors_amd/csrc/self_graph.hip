// self_graph.hip -- self-queries of an index (pn_query_self_*, pn_query_radius_self_*): every indexed row asked against
// its own index, the row itself left out of its answer.
//
// The queries are the index's own rows (d_pts, read in place by the ordinary k-NN / radius pipeline); what is new is
// the exclusion, done here on the pipeline's answers:
//   k-NN:   the chunk's [nqc][k + 1] answer -> [nqc][k]: the entry equal to the row's own index is dropped, else the last
//           one.  The answer is ordered by (distance, index), so this is exactly "the first k entries of the list of the
//           other rows" -- whatever the row's own position in it (duplicates, NaN rows, Cosine self-distances != 0).
//   radius: a row is in its own list iff metric.distance(p_i, p_i) < r -- evaluated here in the reference's arithmetic,
//           which is the arithmetic the pipeline compares with r (exact_scan.hip, select.hip) -- so the adjusted counts
//           need none of the lists (a count-only call has none); each chunk's counts are scanned and placed behind the
//           rows before it, and its lists compacted under the capacity.
// All of it is HBM-bound integer / copy work over the answers, plus one read of the rows for the radius flags.
//
// This translation unit is compiled with -ffp-contract=off: the self-distance must be the reference's unfused fold.
#include "pn_internal.h"

namespace pn {

// Groups of L lanes (a power of two <= 64, groups aligned inside the wave) serve one row each.  Every lane of a wave runs
// the same trip counts (kin, kout are uniform), so the width-L shuffles see all lanes.
template <typename T>
__global__ __launch_bounds__(256) void knn_self_exclude_kernel(const uint64_t *__restrict__ in_idx,
                                                               const T *__restrict__ in_dist, size_t nq, int kin, int kout,
                                                               int L, uint64_t self0, uint64_t *__restrict__ out_idx,
                                                               T *__restrict__ out_dist) {
    const int g = threadIdx.x & (L - 1);
    const size_t q = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / (size_t)L;
    const bool valid = q < nq;
    const uint64_t self = self0 + q;
    const uint64_t *ri = in_idx + (valid ? q : 0) * (size_t)kin;
    const T *rd = in_dist + (valid ? q : 0) * (size_t)kin;
    // the row's own position, else the last entry
    int pos = kin - 1;
    for (int j0 = 0; j0 < kin; j0 += L) {
        const int j = j0 + g;
        int c = (valid && j < kin && ri[j] == self) ? j : kin - 1;
        for (int m = 1; m < L; m <<= 1) {
            const int o = __shfl_xor(c, m, L);
            c = o < c ? o : c;
        }
        pos = c < pos ? c : pos;
    }
    if (!valid) return;
    uint64_t *oi = out_idx + q * (size_t)kout;
    T *od = out_dist + q * (size_t)kout;
    for (int r = g; r < kout; r += L) {
        const int src = r + (r >= pos ? 1 : 0);  // src <= kout = kin - 1
        oi[r] = ri[src];
        od[r] = rd[src];
    }
}

__device__ __forceinline__ float self_sqrt(float x) { return sqrtf(x); }  // correctly rounded (default hipcc)
__device__ __forceinline__ double self_sqrt(double x) { return sqrt(x); }

// flag[i] = exclude && metric.distance(p_i, p_i) < r (the reference's arithmetic: Euclidean sqrt of the fold of
// (a - a)^2 -- 0 for a finite row, NaN otherwise; Cosine 1 - dot / (|a| |a|) with dot the fold of a * a and |a| = cnorm[i],
// the norm the pipeline divides by); cnt[i] = the row's list length without it.  The pipeline compares the same value
// with r for every r -- r <= 0 included: a Cosine self-distance a few ulp below 0 is listed at r = 0 -- and NaN compares
// false on both sides, so a flagged row always has a list of at least one entry.  A flagged row with an empty list would
// be a disagreement between the two: it is counted in *bad (the host entry points fail on it) and the row keeps its
// count, so the offsets stay well formed.
template <typename T, bool COS>
__global__ __launch_bounds__(256) void radius_self_counts_kernel(const T *__restrict__ P, size_t n, int dim, size_t ld,
                                                                 const T *__restrict__ cnorm, T r, bool exclude,
                                                                 const uint64_t *__restrict__ in_off,
                                                                 uint32_t *__restrict__ flag, uint32_t *__restrict__ cnt,
                                                                 uint32_t *__restrict__ bad, const T *__restrict__ radii) {
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t len = in_off[i + 1] - in_off[i];
    uint32_t f = 0;
    if (exclude) {
        const T *p = P + i * ld;
        T acc = (T)0;
        for (int k = 0; k < dim; ++k) {
            const T a = p[k];
            if (COS) {
                const T pr = a * a;
                acc = acc + pr;
            } else {
                const T diff = a - a;
                const T sq = diff * diff;
                acc = acc + sq;
            }
        }
        const T d = COS ? (T)1 - acc / (cnorm[i] * cnorm[i]) : self_sqrt(acc);
        f = d < (radii ? radii[i] : r) ? 1u : 0u;  // NaN distances never match (radii: pn_query_radii_self_*, row i's own)
        if (f && len == 0) {
            atomicAdd(bad, 1u);
            f = 0;
        }
    }
    flag[i] = f;
    cnt[i] = (uint32_t)(len - f);
}

// out[r0 + 1 + j] <- out[r0] + part[j + 1], j < nq: a chunk's exclusive scan (part) placed behind the rows before it
__global__ __launch_bounds__(256) void radius_self_place_kernel(const uint64_t *__restrict__ part, size_t nq,
                                                                uint64_t *__restrict__ out) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nq) out[1 + j] = out[0] + part[j + 1];
}

// out[out_off[i] + t] <- row i's inner list (in_off[i] .. in_off[i + 1], written below in_cap, ascending index) without its
// own index self0 + i when flag[i]; positions below `cap` only.  The own index is found by binary search in the written
// part; a flagged row whose whole list is written and does not hold it is counted in *bad.
template <typename T>
__global__ __launch_bounds__(256) void radius_self_compact_kernel(const uint64_t *__restrict__ in_off,
                                                                  const uint64_t *__restrict__ in_idx,
                                                                  const T *__restrict__ in_dist, uint64_t in_cap,
                                                                  const uint32_t *__restrict__ flag,
                                                                  const uint64_t *__restrict__ out_off, size_t n, int L,
                                                                  uint64_t self0, uint64_t *__restrict__ out_idx,
                                                                  T *__restrict__ out_dist, uint64_t cap,
                                                                  uint32_t *__restrict__ bad) {
    const int g = threadIdx.x & (L - 1);
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / (size_t)L;
    if (i >= n) return;
    const uint64_t o = out_off[i], m = out_off[i + 1] - o;
    if (o >= cap || m == 0) return;
    const uint64_t a = in_off[i], b = in_off[i + 1];
    const uint64_t end = b < in_cap ? b : in_cap;
    uint64_t pos = ~0ull;  // none: every written entry lies before it
    if (flag[i]) {
        const uint64_t self = self0 + i;
        uint64_t lo = a, hi = end;  // first entry >= self in [a, end)
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (in_idx[mid] < self) lo = mid + 1; else hi = mid;
        }
        if (lo < end && in_idx[lo] == self)
            pos = lo - a;
        else if (end == b && g == 0)
            atomicAdd(bad, 1u);
    }
    for (uint64_t t = g; t < m; t += (uint64_t)L) {
        const uint64_t dst = o + t;
        if (dst >= cap) break;
        const uint64_t src = a + t + (t >= pos ? 1 : 0);
        if (src >= end) break;  // (never for dst below cap: see radius_self_enqueue)
        out_idx[dst] = in_idx[src];
        if (out_dist) out_dist[dst] = in_dist[src];
    }
}

static int pick_group(size_t len) {
    int L = 1;
    while (L < 64 && (size_t)L < len) L <<= 1;
    return L;
}

template <typename T>
hipError_t launch_knn_self_exclude(const uint64_t *in_idx, const T *in_dist, size_t nq, int kin, int kout,
                                   uint64_t self0, uint64_t *out_idx, T *out_dist, hipStream_t s) {
    if (nq == 0 || kout <= 0) return hipSuccess;
    const int L = pick_group((size_t)kin);
    const size_t rows_per_block = 256 / (size_t)L;
    hipLaunchKernelGGL((knn_self_exclude_kernel<T>), dim3((unsigned)((nq + rows_per_block - 1) / rows_per_block)), dim3(256),
                       0, s, in_idx, in_dist, nq, kin, kout, L, self0, out_idx, out_dist);
    return hipGetLastError();
}
template hipError_t launch_knn_self_exclude<float>(const uint64_t *, const float *, size_t, int, int, uint64_t,
                                                   uint64_t *, float *, hipStream_t);
template hipError_t launch_knn_self_exclude<double>(const uint64_t *, const double *, size_t, int, int, uint64_t,
                                                    uint64_t *, double *, hipStream_t);

template <typename T>
hipError_t launch_radius_self_counts(const T *P, size_t n, int dim, size_t ld, const T *cnorm, T r, bool exclude,
                                     const uint64_t *in_off, uint32_t *flag, uint32_t *cnt, uint32_t *bad,
                                     hipStream_t s, const T *radii) {
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (cnorm)
        hipLaunchKernelGGL((radius_self_counts_kernel<T, true>), grid, block, 0, s, P, n, dim, ld, cnorm, r, exclude, in_off,
                           flag, cnt, bad, radii);
    else
        hipLaunchKernelGGL((radius_self_counts_kernel<T, false>), grid, block, 0, s, P, n, dim, ld, cnorm, r, exclude, in_off,
                           flag, cnt, bad, radii);
    return hipGetLastError();
}
template hipError_t launch_radius_self_counts<float>(const float *, size_t, int, size_t, const float *, float, bool,
                                                     const uint64_t *, uint32_t *, uint32_t *, uint32_t *, hipStream_t,
                                                     const float *);
template hipError_t launch_radius_self_counts<double>(const double *, size_t, int, size_t, const double *, double, bool,
                                                      const uint64_t *, uint32_t *, uint32_t *, uint32_t *, hipStream_t,
                                                      const double *);
hipError_t launch_radius_self_place(const uint64_t *part, size_t nq, uint64_t *out, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(radius_self_place_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, part, nq, out);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_radius_self_compact(const uint64_t *in_off, const uint64_t *in_idx, const T *in_dist, uint64_t in_cap,
                                      const uint32_t *flag, const uint64_t *out_off, size_t n, uint64_t self0,
                                      uint64_t *out_idx, T *out_dist, uint64_t cap, uint32_t *bad, hipStream_t s) {
    if (n == 0 || cap == 0) return hipSuccess;
    constexpr int L = 32;  // lists average tens of entries in the intended use; longer ones take more trips
    const size_t rows_per_block = 256 / L;
    hipLaunchKernelGGL((radius_self_compact_kernel<T>), dim3((unsigned)((n + rows_per_block - 1) / rows_per_block)),
                       dim3(256), 0, s, in_off, in_idx, in_dist, in_cap, flag, out_off, n, L, self0, out_idx, out_dist, cap,
                       bad);
    return hipGetLastError();
}
template hipError_t launch_radius_self_compact<float>(const uint64_t *, const uint64_t *, const float *, uint64_t,
                                                      const uint32_t *, const uint64_t *, size_t, uint64_t, uint64_t *,
                                                      float *, uint64_t, uint32_t *, hipStream_t);
template hipError_t launch_radius_self_compact<double>(const uint64_t *, const uint64_t *, const double *, uint64_t,
                                                       const uint32_t *, const uint64_t *, size_t, uint64_t, uint64_t *,
                                                       double *, uint64_t, uint32_t *, hipStream_t);

}  // namespace pn
