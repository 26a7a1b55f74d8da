// csr_sort.hip -- segmented sort of a radius answer (CSR of (index, distance) lists) by (distance, index) (gfx950).
//
// pn_query_radius_with_distance_* with PN_RADIUS_SORTED orders each query's list nearest-first under the same total
// order as the k-NN answers: distance ascending, index ascending among equal distances.  The lists are complete on the
// device when this runs (every tier, host and device entry points); they are sorted in place.
//
// Two regimes, split at kSortTile entries per list:
//   short lists  one workgroup per list: (distance, index) pairs in LDS, a bitonic network padded to the next power of
//                two (padding compares above every real entry), written back in place;
//   long lists   (a list can be the whole corpus: r = +inf) spread over many workgroups: every kSortTile-entry chunk is
//                sorted in LDS by a workgroup of its own, then log2(chunks) merge passes, each output tile of
//                kSortTile entries merged by one workgroup from the two sorted runs it draws on (merge path: every
//                thread finds its start on the diagonal by a binary search, then merges 8 entries), ping-pong between
//                the output and a scratch copy.  A list that ends its passes in the scratch copy is copied back.
// The chunks of the long lists are enumerated on the device (a count per list, an exclusive scan), so the device entry
// point never reads anything back; the grids are fixed and the workgroups stride over the chunks.
// Lists that do not lie wholly below `limit` (the device entry point's capacity) are left as they are.
#include "pn_internal.h"

namespace pn {

constexpr int kSortThreads = 256;
constexpr int kMergePerThread = kSortTile / kSortThreads;  // 8 outputs per thread and merge tile

// the k-NN order's key, KeyOf<T>::type wide: the order-preserving map of every float (-0 as +0) that the shard merge
// uses for Cosine indexes (select.hip, sel_key_signed) -- KeyOf's raw bits would misplace Cosine distances a few ulp
// below zero; for distances >= 0 it orders exactly as the raw bits do
template <typename T>
__device__ __forceinline__ typename KeyOf<T>::type sort_key(T d) {
    using K = typename KeyOf<T>::type;
    constexpr K sign = (K)1 << (sizeof(K) * 8 - 1);
    K b;
    const T z = d == (T)0 ? (T)0 : d;
    __builtin_memcpy(&b, &z, sizeof b);
    return (b & sign) ? ~b : (b | sign);
}
template <typename T>
__device__ __forceinline__ bool entry_less(T da, uint64_t ia, T db, uint64_t ib) {
    const auto ka = sort_key<T>(da), kb = sort_key<T>(db);
    return ka < kb || (ka == kb && ia < ib);
}

// bitonic sort of `len` (<= kSortTile) entries at idx / dist in place; sd / si: LDS of kSortTile entries
template <typename T>
__device__ void lds_sort(uint64_t *idx, T *dist, uint32_t len, T *sd, uint64_t *si, bool *spad) {
    const int tid = threadIdx.x;
    uint32_t p2 = 2;
    while (p2 < len) p2 <<= 1;
    for (uint32_t e = tid; e < p2; e += kSortThreads) {
        const bool real = e < len;
        sd[e] = real ? dist[e] : (T)0;
        si[e] = real ? idx[e] : 0;
        spad[e] = !real;  // padding ranks above every real entry
    }
    __syncthreads();
    for (uint32_t k = 2; k <= p2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < p2; i += kSortThreads) {
                const uint32_t l = i ^ j;
                if (l <= i) continue;
                // does entry l rank before entry i?
                const bool pl = spad[l], pi = spad[i];
                const bool l_first = pi ? !pl : (!pl && entry_less<T>(sd[l], si[l], sd[i], si[i]));
                const bool i_first = pl ? !pi : (!pi && entry_less<T>(sd[i], si[i], sd[l], si[l]));
                const bool asc = (i & k) == 0;
                if (asc ? l_first : i_first) {
                    const T td = sd[i];
                    sd[i] = sd[l];
                    sd[l] = td;
                    const uint64_t ti = si[i];
                    si[i] = si[l];
                    si[l] = ti;
                    spad[i] = pl;
                    spad[l] = pi;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t e = tid; e < len; e += kSortThreads) {
        dist[e] = sd[e];
        idx[e] = si[e];
    }
}

__device__ __forceinline__ uint32_t merge_passes(uint64_t len) {  // ceil(log2(chunks)) of a long list
    const uint64_t nch = (len + kSortTile - 1) / kSortTile;
    return nch <= 1 ? 0u : 64u - (uint32_t)__clzll(nch - 1);
}

// short lists: sorted here; long lists: nch[q] = their chunk count (0 otherwise)
template <typename T>
__global__ __launch_bounds__(kSortThreads) void csr_sort_short_kernel(const uint64_t *__restrict__ offsets, int nq,
                                                                     uint64_t *__restrict__ idx, T *__restrict__ dist,
                                                                     uint64_t limit, uint32_t *__restrict__ nch) {
    __shared__ T sd[kSortTile];
    __shared__ uint64_t si[kSortTile];
    __shared__ bool spad[kSortTile];
    const int q = blockIdx.x;
    const uint64_t o0 = offsets[q], o1 = offsets[q + 1], len = o1 - o0;
    const bool whole = o1 <= limit;
    if (threadIdx.x == 0) nch[q] = (whole && len > (uint64_t)kSortTile) ? (uint32_t)((len + kSortTile - 1) / kSortTile) : 0u;
    if (!whole || len <= 1 || len > (uint64_t)kSortTile) return;
    lds_sort<T>(idx + o0, dist + o0, (uint32_t)len, sd, si, spad);
}

// chunk g of the long lists -> (list q, chunk c): the last q with chunk_off[q] <= g (lists without chunks share their
// successor's offset and lose the search)
__device__ __forceinline__ int chunk_owner(const uint64_t *chunk_off, int nq, uint64_t g) {
    int lo = 0, hi = nq;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_off[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <typename T>
__global__ __launch_bounds__(kSortThreads) void csr_sort_chunks_kernel(const uint64_t *__restrict__ offsets, int nq,
                                                                      const uint64_t *__restrict__ chunk_off,
                                                                      uint64_t *__restrict__ idx, T *__restrict__ dist) {
    __shared__ T sd[kSortTile];
    __shared__ uint64_t si[kSortTile];
    __shared__ bool spad[kSortTile];
    const uint64_t total = chunk_off[nq];
    for (uint64_t g = blockIdx.x; g < total; g += gridDim.x) {
        const int q = chunk_owner(chunk_off, nq, g);
        const uint64_t c = g - chunk_off[q];
        const uint64_t o0 = offsets[q], len = offsets[q + 1] - o0;
        const uint64_t b = c * kSortTile, e = b + kSortTile < len ? b + kSortTile : len;
        lds_sort<T>(idx + o0 + b, dist + o0 + b, (uint32_t)(e - b), sd, si, spad);
        __syncthreads();
    }
}

// merge pass p: runs of W = kSortTile << p entries of every long list that still needs the pass, pairwise, from the
// buffer the list's previous pass wrote (even p: the output) into the other one; one kSortTile-entry output tile per
// workgroup and trip
template <typename T>
__global__ __launch_bounds__(kSortThreads) void csr_merge_kernel(const uint64_t *__restrict__ offsets, int nq,
                                                                const uint64_t *__restrict__ chunk_off, uint32_t p,
                                                                uint64_t *__restrict__ idx, T *__restrict__ dist,
                                                                uint64_t *__restrict__ sidx, T *__restrict__ sdist) {
    const uint64_t total = chunk_off[nq];
    const uint64_t W = (uint64_t)kSortTile << p;
    const uint64_t *src_i = (p & 1) ? sidx : idx;
    const T *src_d = (p & 1) ? sdist : dist;
    uint64_t *dst_i = (p & 1) ? idx : sidx;
    T *dst_d = (p & 1) ? dist : sdist;
    for (uint64_t g = blockIdx.x; g < total; g += gridDim.x) {
        const int q = chunk_owner(chunk_off, nq, g);
        const uint64_t o0 = offsets[q], len = offsets[q + 1] - o0;
        if (p >= merge_passes(len)) continue;
        const uint64_t c = g - chunk_off[q];
        const uint64_t t0 = c * kSortTile, t1 = t0 + kSortTile < len ? t0 + kSortTile : len;  // this tile's outputs
        const uint64_t b = t0 / (2 * W) * (2 * W);                                              // its pair of runs
        const uint64_t na = len - b < W ? len - b : W;
        const uint64_t nb = len - b - na < W ? len - b - na : W;
        const uint64_t *ai = src_i + o0 + b, *bi = ai + na;
        const T *ad = src_d + o0 + b, *bd = ad + na;
        uint64_t k = t0 - b + (uint64_t)threadIdx.x * kMergePerThread;  // this thread's first output, on the pair's diagonal
        if (b + k >= t1) continue;
        uint64_t kend = k + kMergePerThread;
        if (b + kend > t1) kend = t1 - b;
        // merge path: i entries from A and k - i from B precede output k
        uint64_t lo = k > nb ? k - nb : 0, hi = k < na ? k : na;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (entry_less<T>(bd[k - 1 - mid], bi[k - 1 - mid], ad[mid], ai[mid])) hi = mid;
            else lo = mid + 1;
        }
        uint64_t i = lo, j = k - lo;
        for (; k < kend; ++k) {
            const bool take_a = j >= nb || (i < na && !entry_less<T>(bd[j], bi[j], ad[i], ai[i]));
            if (take_a) {
                dst_i[o0 + b + k] = ai[i];
                dst_d[o0 + b + k] = ad[i];
                ++i;
            } else {
                dst_i[o0 + b + k] = bi[j];
                dst_d[o0 + b + k] = bd[j];
                ++j;
            }
        }
    }
}

// lists whose last pass wrote the scratch copy: back to the output
template <typename T>
__global__ __launch_bounds__(kSortThreads) void csr_copy_back_kernel(const uint64_t *__restrict__ offsets, int nq,
                                                                    const uint64_t *__restrict__ chunk_off,
                                                                    uint64_t *__restrict__ idx, T *__restrict__ dist,
                                                                    const uint64_t *__restrict__ sidx,
                                                                    const T *__restrict__ sdist) {
    const uint64_t total = chunk_off[nq];
    for (uint64_t g = blockIdx.x; g < total; g += gridDim.x) {
        const int q = chunk_owner(chunk_off, nq, g);
        const uint64_t o0 = offsets[q], len = offsets[q + 1] - o0;
        if (!(merge_passes(len) & 1)) continue;
        const uint64_t t0 = (g - chunk_off[q]) * kSortTile, t1 = t0 + kSortTile < len ? t0 + kSortTile : len;
        for (uint64_t e = t0 + threadIdx.x; e < t1; e += kSortThreads) {
            idx[o0 + e] = sidx[o0 + e];
            dist[o0 + e] = sdist[o0 + e];
        }
    }
}

size_t csr_sort_scratch_entries(size_t nq, size_t max_row, size_t limit) {
    if (max_row <= (size_t)kSortTile) return 0;  // no list can be long
    const size_t all = nq > 0 && max_row > SIZE_MAX / nq ? SIZE_MAX : nq * max_row;
    return all < limit ? all : limit;
}

template <typename T>
hipError_t launch_csr_sort(const uint64_t *offsets, int nq, uint64_t *idx, T *dist, uint64_t limit, size_t max_row,
                           const CsrSortScratch &w, int n_cu, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(csr_sort_short_kernel<T>, dim3((unsigned)nq), dim3(kSortThreads), 0, s, offsets, nq, idx, dist, limit,
                       w.nch);
    const size_t entries = csr_sort_scratch_entries((size_t)nq, max_row, (size_t)limit);
    if (!entries) return hipGetLastError();  // no long list: nothing more to launch
    if (!w.chunk_off || !w.scan || !w.idx || !w.dist) return hipErrorInvalidValue;
    hipError_t e = launch_exclusive_scan_u32(w.nch, (size_t)nq, w.chunk_off, w.scan, nullptr, s);
    if (e != hipSuccess) return e;
    // chunks of the long lists: at most 2 * entries / kSortTile (each has more than kSortTile entries)
    const size_t chunks = 2 * ((entries + kSortTile - 1) / kSortTile) + 1;
    const size_t cap_wg = (size_t)(n_cu > 0 ? n_cu : 256) * 8;
    const unsigned grid = (unsigned)(chunks < cap_wg ? chunks : cap_wg);
    hipLaunchKernelGGL(csr_sort_chunks_kernel<T>, dim3(grid), dim3(kSortThreads), 0, s, offsets, nq,
                       (const uint64_t *)w.chunk_off, idx, dist);
    const size_t longest = max_row < entries ? max_row : entries;
    uint32_t passes = 0;
    while (((size_t)kSortTile << passes) < longest) ++passes;
    for (uint32_t p = 0; p < passes; ++p)
        hipLaunchKernelGGL(csr_merge_kernel<T>, dim3(grid), dim3(kSortThreads), 0, s, offsets, nq,
                           (const uint64_t *)w.chunk_off, p, idx, dist, w.idx, (T *)w.dist);
    if (passes)
        hipLaunchKernelGGL(csr_copy_back_kernel<T>, dim3(grid), dim3(kSortThreads), 0, s, offsets, nq,
                           (const uint64_t *)w.chunk_off, idx, dist, (const uint64_t *)w.idx, (const T *)w.dist);
    return hipGetLastError();
}
template hipError_t launch_csr_sort<float>(const uint64_t *, int, uint64_t *, float *, uint64_t, size_t,
                                           const CsrSortScratch &, int, hipStream_t);
template hipError_t launch_csr_sort<double>(const uint64_t *, int, uint64_t *, double *, uint64_t, size_t,
                                            const CsrSortScratch &, int, hipStream_t);

}  // namespace pn
