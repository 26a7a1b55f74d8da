// optics.hip -- OPTICS over the max_eps self-graph (pn_optics_*) and the DBSCAN-at-eps extraction from an ordering
// (pn_optics_dbscan_*): everything above the k-NN and radius pipelines.  The contract is in the header
// (petal_mi355x.h) and DESIGN.md 4.19; in short
//   core[i]  = the min_samples-th nearest OTHER row's distance if that is < max_eps, else +inf
//   N(i)     = { j != i : d(i, j) < max_eps }, stored only for the rows with a finite core (only they relax anything)
//   n times: p = the unprocessed row with the smallest (reach, row); append it; if core[p] is finite, every unprocessed
//            q in N(p) with max(d(p, q), core[p]) < reach[q] takes that value and the predecessor p.
//
// The n steps depend on each other, so the ordering is ONE launch of ONE workgroup that runs them all: no launch per
// step, no host round trip and nothing that waits for another workgroup -- __syncthreads is the only synchronisation,
// so the kernel cannot hang on the schedule.  The priority structure is a 64-ary tournament tree over packed keys
// (monotone bits of reach, row): a node holds the smallest key of its 64 children, a processed row's leaf holds all
// ones, the root names the next row.  A step retires the root's leaf, relaxes N(p) one entry per thread (each q occurs
// once in N(p): plain stores), and re-reduces only the groups it touched, level by level, one wave64 reduction per
// group -- O(|N(p)| + depth) work per step, depth = ceil(log64 n) <= 4 up to 16 M rows.  The levels above the leaves
// live in LDS from the top down as far as 128 KiB go (all of them up to about 10^6 rows in f32); the rest, and the
// leaves, in global memory, which the L2 holds.
//
// Every comparison is on keys or IEEE '<', every store is to a location a single thread owns within its phase, and two
// waves that re-reduce the same group write the same value: the result is a function of the data alone.
#include "../../include/petal_mi355x.h"
#include "pn_internal.h"

namespace pn {

constexpr int kOptThreads = 1024;            // the ordering workgroup: 16 waves
constexpr int kOptWaves = kOptThreads / 64;
constexpr uint32_t kOptChunk = kOptThreads;  // list entries relaxed between two re-reductions
constexpr uint32_t kOptLdsWords = 16384;     // 64-bit words of LDS for the upper levels: 128 KiB of the CU's 160
constexpr uint32_t kOptNone = 0xFFFFFFFFu;
constexpr int kOptMaxLevels = 8;

template <typename T> struct OptKey;
template <> struct OptKey<float> {
    typedef uint64_t K;
    static constexpr uint32_t kWords = 1;  // 64-bit words per key
    static __device__ __forceinline__ K done() { return ~0ull; }
    static __device__ __forceinline__ K make(float r, uint32_t row) {
        r = r == 0.0f ? 0.0f : r;  // (-0 ties with +0 under IEEE '<')
        uint32_t u = __float_as_uint(r);
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        return ((uint64_t)u << 32) | row;
    }
    static __device__ __forceinline__ bool less(K a, K b) { return a < b; }
    static __device__ __forceinline__ bool is_done(K a) { return a == ~0ull; }
    static __device__ __forceinline__ uint32_t row(K a) { return (uint32_t)a; }
    static __device__ __forceinline__ K shfl_xor(K a, int m) { return __shfl_xor(a, m, 64); }
};
template <> struct OptKey<double> {
    struct __attribute__((aligned(16))) K {
        uint64_t k, row;
    };
    static constexpr uint32_t kWords = 2;
    static __device__ __forceinline__ K done() { return K{~0ull, ~0ull}; }
    static __device__ __forceinline__ K make(double r, uint32_t row) {
        r = r == 0.0 ? 0.0 : r;
        uint64_t u = (uint64_t)__double_as_longlong(r);
        u = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
        return K{u, row};
    }
    static __device__ __forceinline__ bool less(K a, K b) { return a.k < b.k || (a.k == b.k && a.row < b.row); }
    static __device__ __forceinline__ bool is_done(K a) { return a.row == ~0ull; }
    static __device__ __forceinline__ uint32_t row(K a) { return (uint32_t)a.row; }
    static __device__ __forceinline__ K shfl_xor(K a, int m) {
        return K{__shfl_xor(a.k, m, 64), __shfl_xor(a.row, m, 64)};
    }
};

// the tree's shape, the same on the host and in the kernel: sz[0] = n, sz[l + 1] = ceil(sz[l] / 64) down to 1; every level
// is padded to a multiple of 64 keys (the padding holds "processed"), so a group read never leaves its level
struct OptShape {
    int depth;
    uint32_t sz[kOptMaxLevels];
};
__host__ __device__ inline OptShape opt_shape(uint32_t n) {
    OptShape s;
    s.depth = 0;
    s.sz[0] = n;
    while (s.sz[s.depth] > 1 && s.depth + 1 < kOptMaxLevels) {
        s.sz[s.depth + 1] = (s.sz[s.depth] + 63u) >> 6;
        ++s.depth;
    }
    return s;
}
__host__ __device__ inline uint32_t opt_pad(uint32_t x) { return (x + 63u) & ~63u; }

size_t optics_tree_keys(size_t n) {  // leaves + every upper level, padded: what the caller allocates (in keys)
    const OptShape s = opt_shape((uint32_t)n);
    size_t t = 0;
    for (int l = 0; l <= s.depth; ++l) t += opt_pad(s.sz[l]);
    return t;
}

// core[i] = v < max_eps ? v : +inf with v = row i's last self-query column (in_dist == nullptr: undefined everywhere);
// radii[i] = the radius row i's list is asked with: max_eps where the core is defined, 0 (an empty list) elsewhere
template <typename T>
__global__ __launch_bounds__(256) void optics_core_kernel(const T *__restrict__ in_dist, size_t nq, size_t k, T max_eps,
                                                          T *__restrict__ core, T *__restrict__ radii) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const T inf = (T)INFINITY;
    const T v = in_dist ? in_dist[i * k + (k - 1)] : inf;
    const T c = v < max_eps ? v : inf;  // (a NaN value is not < max_eps)
    core[i] = c;
    radii[i] = c < inf ? max_eps : (T)0;
}

// One wave per row of a fill piece: the piece's lists as the radius pipeline wrote them (64-bit ids with the index base,
// the row itself among them wherever its own distance is below its radius) into the graph store at the row's final
// offset, as 32-bit ids without the base and without the row itself.  Nothing is assumed about the order inside a list.
template <typename T>
__global__ __launch_bounds__(256) void optics_repack_kernel(const uint64_t *__restrict__ in_off, const uint64_t *__restrict__ in_idx,
                                                            const T *__restrict__ in_dist, uint64_t in_cap, size_t rows,
                                                            size_t row0, uint64_t index_base, const uint64_t *__restrict__ off,
                                                            uint32_t *__restrict__ ids, T *__restrict__ dist) {
    const int lane = threadIdx.x & 63;
    const size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= rows) return;  // (wave-uniform)
    const uint64_t b = in_off[r], e = in_off[r + 1];
    const uint64_t o0 = off[row0 + r], o1 = off[row0 + r + 1];
    const uint64_t self = index_base + row0 + r;
    uint64_t dropped = 0;
    for (uint64_t t0 = b; t0 < e; t0 += 64) {
        const uint64_t t = t0 + lane;
        const bool live = t < e && t < in_cap;
        const uint64_t j = live ? in_idx[t] : self;
        const bool keep = live && j != self;
        const unsigned long long drops = __ballot(live && j == self);
        const uint64_t before = dropped + __popcll(drops & ((1ull << lane) - 1ull));
        const uint64_t pos = o0 + (t - b) - before;
        if (keep && pos < o1) {
            ids[pos] = (uint32_t)(j - index_base);
            dist[pos] = in_dist[t];
        }
        dropped += __popcll(drops);
    }
}

// ---- the ordering kernel: one workgroup, all n steps
template <typename T>
__global__ __launch_bounds__(kOptThreads) void optics_order_kernel(uint32_t n, const uint64_t *__restrict__ off,
                                                                   const uint32_t *__restrict__ ids,
                                                                   const T *__restrict__ dist, uint64_t n_entries,
                                                                   const T *__restrict__ core, void *tree_mem,
                                                                   uint64_t *__restrict__ ordering, T *reach, int64_t *pred) {
    typedef OptKey<T> KT;
    typedef typename KT::K K;
    __shared__ __attribute__((aligned(16))) uint64_t s_words[kOptLdsWords];
    __shared__ uint32_t s_slot[kOptChunk + 1];  // the groups a chunk's relaxations touched; [kOptChunk]: the group of p
    __shared__ K *s_lvl[kOptMaxLevels];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const OptShape sh = opt_shape(n);
    const int depth = sh.depth;
    const T inf = (T)INFINITY;

    // ---- place the levels (every thread computes the same table; thread 0 publishes it) and fill them
    if (tid == 0) {
        K *g = (K *)tree_mem;
        s_lvl[0] = g;
        g += opt_pad(sh.sz[0]);
        uint32_t used = 0;  // keys of LDS taken
        for (int l = depth; l >= 1; --l) {
            const uint32_t pad = opt_pad(sh.sz[l]);
            if ((used + pad) * KT::kWords <= kOptLdsWords) {
                s_lvl[l] = (K *)s_words + used;
                used += pad;
            } else {
                s_lvl[l] = g;
                g += pad;
            }
        }
    }
    __syncthreads();
    {
        // with every reach at +inf the smallest key under a node is its lowest row
        uint64_t stride = 1;
        for (int l = 0; l <= depth; ++l) {
            K *lv = s_lvl[l];
            const uint32_t pad = opt_pad(sh.sz[l]);
            for (uint32_t g = tid; g < pad; g += kOptThreads) {
                const uint64_t row = (uint64_t)g * stride;
                lv[g] = row < n ? KT::make(inf, (uint32_t)row) : KT::done();
            }
            stride <<= 6;
        }
        for (uint32_t i = tid; i < n; i += kOptThreads) {
            reach[i] = inf;
            if (pred) pred[i] = -1;
        }
    }
    __syncthreads();
    if (depth == 0) {  // a single row
        if (tid == 0 && n) ordering[0] = 0;
        return;
    }
    K *const leaf = s_lvl[0];
    const K *const root = s_lvl[depth];

    for (uint32_t t = 0; t < n; ++t) {
        const K top = root[0];  // (the same value in every thread: written before the last barrier)
        const uint32_t p = KT::row(top);
        if (KT::is_done(top) || p >= n) break;  // (cannot happen before n steps; never index with it)
        if (tid == 0) {
            ordering[t] = p;
            leaf[p] = KT::done();
        }
        const T c = core[p];
        uint64_t beg = 0, end = 0;
        if (c < inf) {
            beg = off[p];
            end = off[p + 1];
            if (end > n_entries) end = n_entries;
            if (beg > end) beg = end;
        }
        bool first = true;
        do {
            const uint64_t left = end - beg;
            const uint32_t m = left < kOptChunk ? (uint32_t)left : kOptChunk;
            uint32_t slot = kOptNone;
            if (tid < m) {
                const uint32_t q = ids[beg + tid];
                const T d = dist[beg + tid];
                if (q < n && q != p && !KT::is_done(leaf[q])) {
                    const T nw = d > c ? d : c;
                    if (nw < reach[q]) {
                        reach[q] = nw;
                        if (pred) pred[q] = (int64_t)p;
                        leaf[q] = KT::make(nw, q);
                        slot = q >> 6;
                    }
                }
            }
            s_slot[tid] = slot;
            if (tid == 0) s_slot[kOptChunk] = first ? (p >> 6) : kOptNone;
            __syncthreads();
            for (int l = 1; l <= depth; ++l) {
                const K *child = s_lvl[l - 1];
                K *node = s_lvl[l];
                for (uint32_t i = wave; i <= m; i += kOptWaves) {
                    const uint32_t g = i == m ? s_slot[kOptChunk] : s_slot[i];
                    if (g == kOptNone) continue;
                    if (i > 0 && i < m && s_slot[i - 1] == g) continue;  // (its left neighbour re-reduces the same group)
                    K v = child[(size_t)g * 64 + lane];
                    for (int x = 32; x; x >>= 1) {
                        const K o = KT::shfl_xor(v, x);
                        if (KT::less(o, v)) v = o;
                    }
                    if (lane == 0) node[g] = v;
                }
                __syncthreads();
                if (l < depth) {
                    if (tid < m && s_slot[tid] != kOptNone) s_slot[tid] >>= 6;
                    if (tid == 0 && s_slot[kOptChunk] != kOptNone) s_slot[kOptChunk] >>= 6;
                    __syncthreads();
                }
            }
            beg += m;
            first = false;
        } while (beg < end);
    }
}

// ---- extraction (pn_optics_dbscan_*): flag pass, one prefix sum over the ordering, scatter
// flag[t] = far && near at ordering[t]; seen[] (zeroed by the caller) counts each row's appearances: a row outside
// [0, n) or a second appearance raises *err
template <typename T>
__global__ __launch_bounds__(256) void optics_flag_kernel(const uint64_t *__restrict__ ordering, const T *__restrict__ reach,
                                                          const T *__restrict__ core, size_t n, T eps, uint32_t *__restrict__ flag,
                                                          uint32_t *seen, uint32_t *err) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint64_t i = ordering[t];
    uint32_t f = 0;
    if (i >= n) {
        atomicOr(err, 1u);
    } else {
        if (atomicAdd(&seen[i], 1u) != 0) atomicOr(err, 1u);
        const bool far = !(reach[i] < eps), near = core[i] < eps;
        f = far && near ? 1u : 0u;
    }
    flag[t] = f;
}
template <typename T>
__global__ __launch_bounds__(256) void optics_label_kernel(const uint64_t *__restrict__ ordering, const T *__restrict__ reach,
                                                           const T *__restrict__ core, size_t n, T eps,
                                                           const uint32_t *__restrict__ flag, const uint64_t *__restrict__ excl,
                                                           int64_t *__restrict__ labels, uint64_t *n_clusters,
                                                           const uint32_t *err, int32_t *d_error) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) {
        if (n_clusters) *n_clusters = excl[n];
        if (d_error) *d_error = *err ? PN_ERR_INVALID : PN_OK;
    }
    if (t >= n) return;
    const uint64_t i = ordering[t];
    if (i >= n) return;
    const bool far = !(reach[i] < eps), near = core[i] < eps;
    labels[i] = far && !near ? -1 : (int64_t)(excl[t] + flag[t]) - 1;
}

// ---- launchers
template <typename T>
hipError_t launch_optics_core(const T *in_dist, size_t nq, size_t k, T max_eps, T *core, T *radii, hipStream_t s) {
    if (!nq) return hipSuccess;
    hipLaunchKernelGGL((optics_core_kernel<T>), dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, in_dist, nq, k, max_eps, core,
                       radii);
    return hipGetLastError();
}
template hipError_t launch_optics_core<float>(const float *, size_t, size_t, float, float *, float *, hipStream_t);
template hipError_t launch_optics_core<double>(const double *, size_t, size_t, double, double *, double *, hipStream_t);
template <typename T>
hipError_t launch_optics_repack(const uint64_t *in_off, const uint64_t *in_idx, const T *in_dist, uint64_t in_cap,
                                size_t rows, size_t row0, uint64_t index_base, const uint64_t *off, uint32_t *ids,
                                T *dist, hipStream_t s) {
    if (!rows) return hipSuccess;
    hipLaunchKernelGGL((optics_repack_kernel<T>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, in_off, in_idx, in_dist, in_cap,
                       rows, row0, index_base, off, ids, dist);
    return hipGetLastError();
}
template hipError_t launch_optics_repack<float>(const uint64_t *, const uint64_t *, const float *, uint64_t, size_t,
                                                size_t, uint64_t, const uint64_t *, uint32_t *, float *, hipStream_t);
template hipError_t launch_optics_repack<double>(const uint64_t *, const uint64_t *, const double *, uint64_t, size_t,
                                                 size_t, uint64_t, const uint64_t *, uint32_t *, double *, hipStream_t);
size_t optics_tree_bytes(size_t n, int elem_bytes) { return optics_tree_keys(n) * (elem_bytes == 4 ? 8 : 16); }
template <typename T>
hipError_t launch_optics_order(size_t n, const uint64_t *off, const uint32_t *ids, const T *dist, uint64_t n_entries,
                               const T *core, void *tree, uint64_t *ordering, T *reach, int64_t *pred, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL((optics_order_kernel<T>), dim3(1), dim3(kOptThreads), 0, s, (uint32_t)n, off, ids, dist, n_entries, core,
                       tree, ordering, reach, pred);
    return hipGetLastError();
}
template hipError_t launch_optics_order<float>(size_t, const uint64_t *, const uint32_t *, const float *, uint64_t,
                                               const float *, void *, uint64_t *, float *, int64_t *, hipStream_t);
template hipError_t launch_optics_order<double>(size_t, const uint64_t *, const uint32_t *, const double *, uint64_t,
                                                const double *, void *, uint64_t *, double *, int64_t *, hipStream_t);
// buf: optics_extract_bytes(n) bytes of scratch
size_t optics_extract_bytes(size_t n) { return (n + 1 + n / 4096 + 2) * sizeof(uint64_t) + (2 * n + 2) * sizeof(uint32_t); }
template <typename T>
hipError_t launch_optics_extract(const uint64_t *ordering, const T *reach, const T *core, size_t n, T eps, void *buf,
                                 int64_t *labels, uint64_t *n_clusters, int32_t *d_error, hipStream_t s) {
    uint64_t *excl = (uint64_t *)buf, *scan = excl + n + 1;
    uint32_t *flag = (uint32_t *)(scan + n / 4096 + 2), *seen = flag + n, *err = seen + n;
    hipError_t e = hipMemsetAsync(seen, 0, (n + 1) * sizeof(uint32_t), s);  // (seen and the error word behind it)
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL((optics_flag_kernel<T>), dim3(grid), dim3(256), 0, s, ordering, reach, core, n, eps, flag, seen, err);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_exclusive_scan_u32(flag, n, excl, scan, nullptr, s)) != hipSuccess) return e;
    hipLaunchKernelGGL((optics_label_kernel<T>), dim3(grid), dim3(256), 0, s, ordering, reach, core, n, eps, flag, excl, labels,
                       n_clusters, err, d_error);
    return hipGetLastError();
}
template hipError_t launch_optics_extract<float>(const uint64_t *, const float *, const float *, size_t, float, void *,
                                                 int64_t *, uint64_t *, int32_t *, hipStream_t);
template hipError_t launch_optics_extract<double>(const uint64_t *, const double *, const double *, size_t, double,
                                                  void *, int64_t *, uint64_t *, int32_t *, hipStream_t);

}  // namespace pn
