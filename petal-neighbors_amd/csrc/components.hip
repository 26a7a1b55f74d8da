// components.hip -- DBSCAN on the device (pn_dbscan_*): the consumer of the radius self-lists.  The lists themselves are
// the pipeline's (radius_device_enqueue over a piece of the rows, index.hip); what is here turns them into labels:
//   init:    core[i] = |N(i)| >= min_samples from the counting pass' offsets, parent[i] = i, and the length of the side
//            list a non-core row will need (|N(i)|, 0 for a core row);
//   union:   a piece's lists, read in the workspace scratch they were written to.  A core row is united with every core
//            row of its list (lock-free union-find over parent[]); a non-core row copies its list to its side list, the
//            non-core entries replaced by kNone, so that its cluster can be chosen once every root is final;
//   finish:  root[i] = find(i), the roots of core rows flagged, scanned (radius_device.hip's scan) into cluster numbers;
//            a core row takes its root's number, a non-core row the number of the SMALLEST root in its side list, else -1.
//
// Why the labels depend on nothing but the data.  Every hook (union_find.h) links the larger of two roots under the
// smaller, so parent[x] <= x always, the forest has no cycle, and a finished component's root is its lowest core index
// whatever order the unions ran in.  Clusters are numbered by ascending root, so "the lowest-numbered cluster among a border row's core
// neighbours" is the smallest root among them: an order-free minimum.
//
// Visibility: the agent-scope-atomics rule of union_find.h holds inside the union and flatten kernels.  core[] and the
// offsets are written by earlier launches only and are read plainly.
//
// Work distribution: groups of L lanes (a power of two <= 64, aligned inside the wave) serve one row, L picked per piece
// from its mean list length.  The alternative -- one lane per entry with a binary search for its row in the piece's
// offsets -- balances skewed lists perfectly but pays log2(rows) = 18 dependent loads per entry, more than the union of
// an entry costs once the roots agree; with lists of mean 24 and maximum 300-odd a group of 32 lanes idles a quarter of
// its lanes on the mean row and takes ten trips on the longest, which tools/bench_dbscan.py shows to be a small share of
// the call (the radius pipeline that makes the lists dominates it).
#include "pn_internal.h"
#include "union_find.h"

namespace pn {

constexpr uint32_t kNone = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void dbscan_init_kernel(const uint64_t *__restrict__ off, size_t n, uint64_t min_samples,
                                                          uint8_t *__restrict__ core, uint32_t *__restrict__ parent,
                                                          uint32_t *__restrict__ side_len) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t len = off[i + 1] - off[i];  // <= n < 2^31
    const bool c = len >= min_samples;
    core[i] = c ? 1 : 0;
    parent[i] = (uint32_t)i;
    side_len[i] = c ? 0u : (uint32_t)len;
}

// rows [r0, r0 + nq) of the index: list of row r0 + q = in_idx[in_off[q] .. in_off[q + 1]) (entries base + j, j < n; the
// piece's capacity is its exact total, so every entry is written).  side / side_off: the side lists of ALL rows.
__global__ __launch_bounds__(256) void dbscan_union_kernel(const uint64_t *__restrict__ in_off,
                                                           const uint64_t *__restrict__ in_idx, uint64_t in_cap, size_t nq,
                                                           size_t r0, size_t n, uint64_t base, int L,
                                                           const uint8_t *__restrict__ core, uint32_t *parent,
                                                           const uint64_t *__restrict__ side_off,
                                                           uint32_t *__restrict__ side) {
    const int g = threadIdx.x & (L - 1);
    const size_t q = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / (size_t)L;
    if (q >= nq) return;
    const uint64_t a = in_off[q], b = in_off[q + 1] < in_cap ? in_off[q + 1] : in_cap;
    const uint32_t i = (uint32_t)(r0 + q);
    if (core[i]) {
        uint32_t ri = i;
        for (uint64_t t = a + g; t < b; t += (uint64_t)L) {
            const uint64_t j = in_idx[t] - base;
            if (j >= n || j == i || !core[j]) continue;
            ri = uf_unite(parent, ri, (uint32_t)j);
        }
    } else {
        const uint64_t so = side_off[i], room = side_off[i + 1] - so;  // = the list's length (dbscan_init_kernel)
        for (uint64_t t = a + g; t < b; t += (uint64_t)L) {
            if (t - a >= room) break;
            const uint64_t j = in_idx[t] - base;
            side[so + (t - a)] = (j < n && core[j]) ? (uint32_t)j : kNone;
        }
    }
}

// root[i] <- find(i) for core rows (kNone otherwise); is_root[i] <- core[i] && root[i] == i
__global__ __launch_bounds__(256) void dbscan_flatten_kernel(uint32_t *parent, const uint8_t *__restrict__ core, size_t n,
                                                             uint32_t *__restrict__ root, uint32_t *__restrict__ is_root) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t r = kNone;
    if (core[i]) r = uf_find(parent, (uint32_t)i);
    root[i] = r;
    is_root[i] = r == (uint32_t)i ? 1u : 0u;
}

// num[r] = the number of the cluster rooted at r (exclusive scan of is_root)
__global__ __launch_bounds__(256) void dbscan_label_kernel(const uint32_t *__restrict__ root,
                                                           const uint64_t *__restrict__ num,
                                                           const uint8_t *__restrict__ core,
                                                           const uint64_t *__restrict__ side_off,
                                                           const uint32_t *__restrict__ side, size_t n,
                                                           int64_t *__restrict__ labels) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t r = kNone;
    if (core[i]) {
        r = root[i];
    } else {
        for (uint64_t t = side_off[i]; t < side_off[i + 1]; ++t) {
            const uint32_t j = side[t];
            if (j >= n) continue;  // kNone
            const uint32_t rj = root[j];
            r = rj < r ? rj : r;
        }
    }
    labels[i] = r == kNone ? (int64_t)-1 : (int64_t)num[r];
}

// every row noise (eps <= 0 or NaN): labels -1, core 0 (nullable), n_clusters 0 (nullable)
__global__ __launch_bounds__(256) void dbscan_noise_kernel(size_t n, int64_t *__restrict__ labels, uint8_t *__restrict__ core,
                                                           uint64_t *__restrict__ n_clusters) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && n_clusters) *n_clusters = 0;
    if (i >= n) return;
    labels[i] = -1;
    if (core) core[i] = 0;
}

static dim3 rows_grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

hipError_t launch_dbscan_init(const uint64_t *off, size_t n, uint64_t min_samples, uint8_t *core, uint32_t *parent,
                              uint32_t *side_len, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(dbscan_init_kernel, rows_grid(n), dim3(256), 0, s, off, n, min_samples, core, parent, side_len);
    return hipGetLastError();
}
hipError_t launch_dbscan_union(const uint64_t *in_off, const uint64_t *in_idx, uint64_t in_cap, size_t nq, size_t r0,
                               size_t n, uint64_t base, const uint8_t *core, uint32_t *parent, const uint64_t *side_off,
                               uint32_t *side, hipStream_t s) {
    if (nq == 0 || in_cap == 0) return hipSuccess;
    const size_t mean = (size_t)(in_cap / nq);
    int L = 4;
    while (L < 64 && (size_t)L < mean) L <<= 1;
    const size_t rows_per_block = 256 / (size_t)L;
    hipLaunchKernelGGL(dbscan_union_kernel, dim3((unsigned)((nq + rows_per_block - 1) / rows_per_block)), dim3(256), 0, s,
                       in_off, in_idx, in_cap, nq, r0, n, base, L, core, parent, side_off, side);
    return hipGetLastError();
}
hipError_t launch_dbscan_flatten(uint32_t *parent, const uint8_t *core, size_t n, uint32_t *root, uint32_t *is_root,
                                 hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(dbscan_flatten_kernel, rows_grid(n), dim3(256), 0, s, parent, core, n, root, is_root);
    return hipGetLastError();
}
hipError_t launch_dbscan_label(const uint32_t *root, const uint64_t *num, const uint8_t *core, const uint64_t *side_off,
                               const uint32_t *side, size_t n, int64_t *labels, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(dbscan_label_kernel, rows_grid(n), dim3(256), 0, s, root, num, core, side_off, side, n, labels);
    return hipGetLastError();
}
hipError_t launch_dbscan_noise(size_t n, int64_t *labels, uint8_t *core, uint64_t *n_clusters, hipStream_t s) {
    hipLaunchKernelGGL(dbscan_noise_kernel, rows_grid(n ? n : 1), dim3(256), 0, s, n, labels, core, n_clusters);
    return hipGetLastError();
}

}  // namespace pn
