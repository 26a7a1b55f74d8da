// mst.hip -- the exact minimum spanning tree of the indexed rows under mutual reachability (pn_mst_*): Boruvka rounds
// under a strict edge order.  The distances come from exact_scan.hip's masked scan (mst_scan_kernel); what is here is the
// bookkeeping between scans, the round loop and the final sort.
//
// The graph is complete over the n rows; the edge {i, j}, i < j, weighs w = max(d(i, j), core[i], core[j]), the maximum
// taken on the library's sortable keys (NaN above +inf, -0 as +0; signed keys for Cosine, and a negative core value of a
// Euclidean index counts as 0).  Edges are ordered by (key(w), i, j): a STRICT total order, so the minimum spanning tree is
// unique (the cut property picks one edge per cut, never one of several) and every choice below is a pure minimum --
// the result depends on nothing but the data.
//
// State: comp[i] (the row's component = the lowest row in it), a cached candidate (cand_key[i], cand_j[i]) = the least edge
// from row i to a row outside its component as of the round it was scanned in, and the core keys ckey[i].  For a fixed i
// the edge order over j is ascending (key(w(i, j)), j) (exact_scan.hip), so one (key, j) per row is enough.
//
// A round:
//   list     which rows must be scanned.  (1) Components only grow, so a cached candidate whose partner is still outside
//            the row's component is still the row's minimum: only rows whose partner has joined them ("invalid" rows) can
//            need a scan.  (2) Every edge out of row i weighs at least core[i]: an invalid row whose core key is strictly
//            above the least cached key of its component's valid rows cannot supply the component's edge; it is left out
//            and stays invalid.  A component without a valid row lists all its rows.  (3) Round 0 of an un-cored call is
//            the 1-NN self-query, answered by the k-NN pipeline and its filter tiers (index.hip); it counts n rows.
//   scan     the listed rows, at most `batch` per launch; the segments' minima are reduced into the cache.
//   choose   per component the least (key, lo, hi) over its valid rows: two order-free minima, first the key
//            (cmin_key), then the packed pair among the rows that attain it (cmin_pair).
//   emit     every component's edge, once where both ends chose it (the lower component writes), united through
//            union_find.h; then comp[i] = find(i) and the components are counted.
// The host reads {listed rows, components, edges so far} once per round; with a strict order the chosen edges cannot
// close a cycle, so edges == n - components always -- a mismatch ends the call with PN_ERR_DEVICE instead of a loop.
// At the end the n - 1 edges are sorted by (key, lo, hi) with a bitonic network (padded to a power of two, 1024-element
// blocks in LDS, the wider strides in HBM): the order is strict, so an unstable network gives one answer.
//
// Visibility: parent[] by union_find.h's rule inside the emit and relabel kernels; cmin_key / cmin_pair / counters are
// only ever touched by agent-scope atomics inside the kernel that builds them and read plainly by LATER launches;
// everything else is written by one launch and read by later ones.
#include "../../include/petal_mi355x.h"
#include "pn_internal.h"
#include "union_find.h"

namespace pn {

namespace {

constexpr uint32_t kNoRow = 0xFFFFFFFFu;
constexpr uint64_t kNoPair = ~0ull;
constexpr int kSortBlock = 1024;  // elements one workgroup sorts in LDS

// sortable keys of values / values of keys (exact_scan.hip's dist_key, dist_key_signed and their inverses); the unsigned
// map is for distances (>= +0 or NaN): anything at or below zero, -0 included, is the key of +0
template <typename T> struct Bits;
template <> struct Bits<float> {
    static __device__ __forceinline__ uint32_t of(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ float to(uint32_t b) { return __uint_as_float(b); }
    static constexpr uint32_t kSign = 0x80000000u, kNaNSigned = 0xFFC00000u;
};
template <> struct Bits<double> {
    static __device__ __forceinline__ uint64_t of(double v) { return (uint64_t)__double_as_longlong(v); }
    static __device__ __forceinline__ double to(uint64_t b) { return __longlong_as_double((long long)b); }
    static constexpr uint64_t kSign = 0x8000000000000000ull, kNaNSigned = 0xFFF8000000000000ull;
};
template <typename T>
__device__ __forceinline__ typename KeyOf<T>::type key_of(T v, bool signed_keys) {
    using K = typename KeyOf<T>::type;
    if (signed_keys) {
        if (v != v) return Bits<T>::kNaNSigned;
        const K b = Bits<T>::of(v == (T)0 ? (T)0 : v);
        return (b & Bits<T>::kSign) ? ~b : (b | Bits<T>::kSign);
    }
    if (v != v) return KeyOf<T>::kNaN;
    return v <= (T)0 ? (K)0 : Bits<T>::of(v);
}
template <typename T>
__device__ __forceinline__ T value_of(typename KeyOf<T>::type k, bool signed_keys) {
    if (signed_keys) return Bits<T>::to((k & Bits<T>::kSign) ? (k ^ Bits<T>::kSign) : ~k);
    return Bits<T>::to(k);
}

// one atomic per wave: the lanes with pred get consecutive slots from *ctr (every lane of the wave must call)
__device__ __forceinline__ uint32_t wave_slots(uint32_t *ctr, bool pred) {
    const unsigned long long m = __ballot(pred);
    if (!m) return 0;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(ctr, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

template <typename T>
__global__ __launch_bounds__(256) void mst_init_kernel(size_t n, const T *__restrict__ core, bool signed_keys,
                                                       uint32_t *__restrict__ comp, uint32_t *__restrict__ parent,
                                                       uint32_t *__restrict__ cand_j, uint32_t *__restrict__ list,
                                                       typename KeyOf<T>::type *__restrict__ ckey) {
    using K = typename KeyOf<T>::type;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    comp[i] = parent[i] = list[i] = (uint32_t)i;
    cand_j[i] = kNoRow;
    ckey[i] = core ? key_of<T>(core[i], signed_keys) : (K)0;  // (no cores: the least key of either map, w = d)
}

// round 0 from the 1-NN self-query: the nearest other row by (distance, index) IS the row's least edge while every row
// is its own component and the cores are zero
template <typename T>
__global__ __launch_bounds__(256) void mst_seed_kernel(size_t n, const uint64_t *__restrict__ nn_idx,
                                                       const T *__restrict__ nn_dist, uint64_t base, bool signed_keys,
                                                       uint32_t *__restrict__ cand_j,
                                                       typename KeyOf<T>::type *__restrict__ cand_key) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t j = nn_idx[i] - base;
    cand_j[i] = j < n ? (uint32_t)j : kNoRow;
    cand_key[i] = key_of<T>(nn_dist[i], signed_keys);
}

// the segments' minima of listed row r -> the row's cache
template <typename K>
__global__ __launch_bounds__(256) void mst_reduce_kernel(const uint32_t *__restrict__ qsel, size_t nq, size_t nq_pad,
                                                         int nseg, const K *__restrict__ seg_key,
                                                         const uint32_t *__restrict__ seg_j, K *__restrict__ cand_key,
                                                         uint32_t *__restrict__ cand_j) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nq) return;
    K bk = seg_key[r];
    uint32_t bj = seg_j[r];
    for (int sg = 1; sg < nseg; ++sg) {
        const K k = seg_key[(size_t)sg * nq_pad + r];
        const uint32_t j = seg_j[(size_t)sg * nq_pad + r];
        if (k < bk || (k == bk && j < bj)) {
            bk = k;
            bj = j;
        }
    }
    const uint32_t row = qsel[r];
    cand_key[row] = bk;
    cand_j[row] = bj;
}

__device__ __forceinline__ void key_min(uint32_t *p, uint32_t v) { atomicMin(p, v); }
__device__ __forceinline__ void key_min(uint64_t *p, uint64_t v) {
    atomicMin(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}
__device__ __forceinline__ bool cache_valid(const uint32_t *comp, const uint32_t *cand_j, size_t i) {
    const uint32_t j = cand_j[i];
    return j != kNoRow && comp[j] != comp[i];
}

// cmin_key[c] <- the least cached key over the valid rows of component c (pre-set to kMax)
template <typename K>
__global__ __launch_bounds__(256) void mst_minkey_kernel(size_t n, const uint32_t *__restrict__ comp,
                                                         const uint32_t *__restrict__ cand_j,
                                                         const K *__restrict__ cand_key, K *cmin_key) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (cache_valid(comp, cand_j, i)) key_min(cmin_key + comp[i], cand_key[i]);
}
// flag[i] <- row i must be scanned this round
template <typename K>
__global__ __launch_bounds__(256) void mst_flag_kernel(size_t n, const uint32_t *__restrict__ comp,
                                                       const uint32_t *__restrict__ cand_j, const K *__restrict__ ckey,
                                                       const K *__restrict__ cmin_key, uint32_t *__restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t f = 0;
    if (!cache_valid(comp, cand_j, i)) {
        const K m = cmin_key[comp[i]];  // kMax: no valid row in the component (no key is kMax)
        f = ckey[i] <= m ? 1u : 0u;
    }
    flag[i] = f;
}
__global__ __launch_bounds__(256) void mst_list_kernel(size_t n, const uint32_t *__restrict__ flag,
                                                       const uint64_t *__restrict__ off, uint32_t *__restrict__ list) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) list[off[i]] = (uint32_t)i;
}
// cmin_pair[c] <- the least (lo, hi) among the valid rows of c that attain cmin_key[c] (pre-set to all ones)
template <typename K>
__global__ __launch_bounds__(256) void mst_minpair_kernel(size_t n, const uint32_t *__restrict__ comp,
                                                          const uint32_t *__restrict__ cand_j,
                                                          const K *__restrict__ cand_key, const K *__restrict__ cmin_key,
                                                          unsigned long long *cmin_pair) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!cache_valid(comp, cand_j, i)) return;
    const uint32_t c = comp[i], j = cand_j[i];
    if (cand_key[i] != cmin_key[c]) return;
    const uint32_t lo = j < (uint32_t)i ? j : (uint32_t)i, hi = j < (uint32_t)i ? (uint32_t)i : j;
    atomicMin(cmin_pair + c, ((unsigned long long)lo << 32) | hi);
}
// every component root writes its edge -- unless the component at the other end chose the same edge and is the lower
// one -- and unites the two ends.  ctr[1]: edges so far.
template <typename K>
__global__ __launch_bounds__(256) void mst_emit_kernel(size_t n, const uint32_t *__restrict__ comp,
                                                       const K *__restrict__ cmin_key,
                                                       const unsigned long long *__restrict__ cmin_pair, uint32_t *parent,
                                                       K *__restrict__ e_key, unsigned long long *__restrict__ e_pair,
                                                       uint32_t *ctr) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool root = i < n && comp[i] == (uint32_t)i;
    unsigned long long pair = kNoPair;
    if (root) pair = cmin_pair[i];
    root = root && pair != kNoPair;
    uint32_t lo = 0, hi = 0;
    bool write = false;
    if (root) {
        lo = (uint32_t)(pair >> 32);
        hi = (uint32_t)pair;
        const uint32_t c2 = comp[lo] == (uint32_t)i ? comp[hi] : comp[lo];
        write = !(cmin_pair[c2] == pair && c2 < (uint32_t)i);
    }
    const uint32_t slot = wave_slots(ctr + 1, write);
    if (write && (size_t)slot + 1 < n) {
        e_key[slot] = cmin_key[i];
        e_pair[slot] = pair;
    }
    if (root) (void)uf_unite(parent, lo, hi);
}
// comp[i] <- find(i); ctr[0] (zeroed by the caller) <- components
__global__ __launch_bounds__(256) void mst_relabel_kernel(size_t n, uint32_t *parent, uint32_t *__restrict__ comp,
                                                          uint32_t *ctr) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t r = kNoRow;
    if (i < n) {
        r = uf_find(parent, (uint32_t)i);
        comp[i] = r;
    }
    const unsigned long long m = __ballot(i < n && r == (uint32_t)i);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(ctr, (uint32_t)__popcll(m));
}

// ---- the final sort: bitonic network over (key, pair), ascending
template <typename K>
__device__ __forceinline__ bool edge_after(K ka, unsigned long long pa, K kb, unsigned long long pb) {
    return ka > kb || (ka == kb && pa > pb);
}
template <typename K>
__global__ __launch_bounds__(256) void mst_sort_pad_kernel(size_t from, size_t to, K *__restrict__ e_key,
                                                           unsigned long long *__restrict__ e_pair) {
    const size_t i = from + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= to) return;
    e_key[i] = ~(K)0;  // kMax
    e_pair[i] = kNoPair;
}
// stages k = k_lo .. k_hi (doubling), of each the strides min(k / 2, kSortBlock / 2) .. 1, on one block's elements in LDS
template <typename K>
__global__ __launch_bounds__(kSortBlock / 2) void mst_sort_local_kernel(K *__restrict__ e_key,
                                                                        unsigned long long *__restrict__ e_pair, size_t k_lo,
                                                                        size_t k_hi) {
    __shared__ K sk[kSortBlock];
    __shared__ unsigned long long sp[kSortBlock];
    const size_t base = (size_t)blockIdx.x * kSortBlock;
    const int t = threadIdx.x;
    sk[t] = e_key[base + t];
    sp[t] = e_pair[base + t];
    sk[t + kSortBlock / 2] = e_key[base + t + kSortBlock / 2];
    sp[t + kSortBlock / 2] = e_pair[base + t + kSortBlock / 2];
    for (size_t k = k_lo; k <= k_hi; k <<= 1) {
        for (int j = (int)(k / 2 < (size_t)(kSortBlock / 2) ? k / 2 : (size_t)(kSortBlock / 2)); j >= 1; j >>= 1) {
            __syncthreads();
            const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
            const bool asc = ((base + (size_t)i) & k) == 0;
            const K ka = sk[i], kb = sk[l];
            const unsigned long long pa = sp[i], pb = sp[l];
            if (edge_after<K>(ka, pa, kb, pb) == asc) {
                sk[i] = kb; sp[i] = pb;
                sk[l] = ka; sp[l] = pa;
            }
        }
    }
    __syncthreads();
    e_key[base + t] = sk[t];
    e_pair[base + t] = sp[t];
    e_key[base + t + kSortBlock / 2] = sk[t + kSortBlock / 2];
    e_pair[base + t + kSortBlock / 2] = sp[t + kSortBlock / 2];
}
// one compare-exchange step of stage k at stride j (>= kSortBlock), N / 2 threads
template <typename K>
__global__ __launch_bounds__(256) void mst_sort_step_kernel(K *__restrict__ e_key, unsigned long long *__restrict__ e_pair,
                                                            size_t half, size_t k, size_t j) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= half) return;
    const size_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const bool asc = (i & k) == 0;
    const K ka = e_key[i], kb = e_key[l];
    const unsigned long long pa = e_pair[i], pb = e_pair[l];
    if (edge_after<K>(ka, pa, kb, pb) == asc) {
        e_key[i] = kb; e_pair[i] = pb;
        e_key[l] = ka; e_pair[l] = pa;
    }
}
template <typename T>
__global__ __launch_bounds__(256) void mst_output_kernel(size_t ne, const typename KeyOf<T>::type *__restrict__ e_key,
                                                         const unsigned long long *__restrict__ e_pair, uint64_t base,
                                                         bool signed_keys, uint64_t *__restrict__ src,
                                                         uint64_t *__restrict__ dst, T *__restrict__ weight) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const unsigned long long p = e_pair[e];
    src[e] = base + (p >> 32);
    dst[e] = base + (p & 0xFFFFFFFFull);
    weight[e] = value_of<T>(e_key[e], signed_keys);
}

dim3 rows_grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
size_t sort_len(size_t n) { return sort_key_pair_len(n - 1); }  // the n - 1 edges padded for the network

// the network over N (a power of two >= kSortBlock) padded elements: also mean_shift.hip's rank sort
template <typename K>
hipError_t sort_key_pair(K *e_key, unsigned long long *e_pair, size_t N2, hipStream_t s) {
    const dim3 lg((unsigned)(N2 / kSortBlock)), lb(kSortBlock / 2), blk(256);
    hipLaunchKernelGGL((mst_sort_local_kernel<K>), lg, lb, 0, s, e_key, e_pair, (size_t)2, (size_t)kSortBlock);
    for (size_t k = 2 * (size_t)kSortBlock; k <= N2; k <<= 1) {
        for (size_t j = k / 2; j >= (size_t)kSortBlock; j >>= 1)
            hipLaunchKernelGGL((mst_sort_step_kernel<K>), rows_grid(N2 / 2), blk, 0, s, e_key, e_pair, N2 / 2, k, j);
        hipLaunchKernelGGL((mst_sort_local_kernel<K>), lg, lb, 0, s, e_key, e_pair, k, k);
    }
    return hipGetLastError();
}

// the scratch of a call, carved from one buffer: 64-bit arrays first
struct Layout {
    size_t n = 0, n_pad = 0, N2 = 0, scan_words = 0, seg_entries = 0, key_bytes = 0;
    size_t o_pair = 0, o_off = 0, o_scan = 0, o_epair = 0, o_keys = 0, o_u32 = 0, total = 0;
    Layout(size_t n_, int elem_bytes, size_t batch, int n_cu) {
        n = n_;
        n_pad = round_up(n, (size_t)kRowPad);
        N2 = sort_len(n);
        scan_words = n / 4096 + 2;
        key_bytes = (size_t)elem_bytes;
        const size_t bmax = batch < n ? batch : n, qt = (bmax + kTileQ - 1) / kTileQ, target = (size_t)8 * (size_t)n_cu;
        seg_entries = (qt > target ? qt : target) * kTileQ;
        o_pair = 0;
        o_off = o_pair + n * 8;
        o_scan = o_off + (n + 1) * 8;
        o_epair = o_scan + scan_words * 8;
        o_keys = o_epair + N2 * 8;  // ckey [n_pad], cand_key [n], cmin_key [n], e_key [N2], seg_key [seg_entries]
        o_u32 = o_keys + round_up((n_pad + 2 * n + N2 + seg_entries) * key_bytes, (size_t)8);
        // comp [n_pad], parent, cand_j, list, flag [n each], seg_j [seg_entries], counters [4]
        total = o_u32 + (n_pad + 4 * n + seg_entries + 4) * 4;
    }
};

#define MSTCHK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return set_error(e_ == hipErrorOutOfMemory ? PN_ERR_NOMEM : PN_ERR_DEVICE, "%s: %s", #expr,      \
                             hipGetErrorString(e_));                                                         \
    } while (0)

}  // namespace

template <typename T>
int mst_enqueue(MstArgs &a, hipStream_t s) {
    using K = typename KeyOf<T>::type;
    const size_t n = a.n;
    a.work[0] = a.work[1] = 0;
    if (n < 2) return PN_OK;
    const size_t batch = a.batch ? a.batch : 1;
    const Layout L(n, (int)sizeof(T), batch, a.n_cu);
    char *b = (char *)a.buf;
    unsigned long long *cmin_pair = (unsigned long long *)(b + L.o_pair), *e_pair = (unsigned long long *)(b + L.o_epair);
    uint64_t *off = (uint64_t *)(b + L.o_off), *scan = (uint64_t *)(b + L.o_scan);
    K *ckey = (K *)(b + L.o_keys), *cand_key = ckey + L.n_pad, *cmin_key = cand_key + n, *e_key = cmin_key + n,
      *seg_key = e_key + L.N2;
    uint32_t *comp = (uint32_t *)(b + L.o_u32), *parent = comp + L.n_pad, *cand_j = parent + n, *list = cand_j + n,
             *flag = list + n, *seg_j = flag + n, *ctr = seg_j + L.seg_entries;
    const bool cosm = a.cnorm != nullptr;
    const T *P = (const T *)a.P, *cnorm = (const T *)a.cnorm;
    const dim3 g = rows_grid(n), blk(256);
    const size_t row_tiles = (n + kTileP - 1) / kTileP, target = (size_t)8 * (size_t)a.n_cu;

    MSTCHK(hipMemsetAsync(ctr, 0, 4 * sizeof(uint32_t), s));
    hipLaunchKernelGGL((mst_init_kernel<T>), g, blk, 0, s, n, (const T *)a.d_core, cosm, comp, parent, cand_j, list, ckey);
    MSTCHK(hipGetLastError());

    // the listed rows list[0 .. nlist), `batch` per launch; segments sized so that a short list still fills the device
    auto scan_listed = [&](size_t nlist) -> int {
        for (size_t r0 = 0; r0 < nlist; r0 += batch) {
            const size_t nq = nlist - r0 < batch ? nlist - r0 : batch;
            const size_t qt = (nq + kTileQ - 1) / kTileQ;
            size_t nseg = target / qt;
            nseg = nseg < 1 ? 1 : (nseg > row_tiles ? row_tiles : nseg);
            const size_t seg_tiles = (row_tiles + nseg - 1) / nseg;
            nseg = (row_tiles + seg_tiles - 1) / seg_tiles;
            if (nseg * qt * kTileQ > L.seg_entries) return set_error(PN_ERR_DEVICE, "MST scan plan exceeds its scratch (internal error)");
            MSTCHK(launch_mst_scan<T>(P, n, a.dim, a.ld, list + r0, (int)nq, seg_tiles * kTileP, (int)nseg, comp, ckey, cnorm,
                                      seg_key, seg_j, s));
            hipLaunchKernelGGL((mst_reduce_kernel<K>), rows_grid(nq), blk, 0, s, list + r0, nq, qt * kTileQ, (int)nseg, seg_key,
                               seg_j, cand_key, cand_j);
            MSTCHK(hipGetLastError());
        }
        return PN_OK;
    };
    auto min_keys = [&]() -> int {
        MSTCHK(hipMemsetAsync(cmin_key, 0xFF, n * sizeof(K), s));
        hipLaunchKernelGGL((mst_minkey_kernel<K>), g, blk, 0, s, n, comp, cand_j, cand_key, cmin_key);
        MSTCHK(hipGetLastError());
        return PN_OK;
    };
    auto choose_emit_relabel = [&]() -> int {
        int rc = min_keys();
        if (rc != PN_OK) return rc;
        MSTCHK(hipMemsetAsync(cmin_pair, 0xFF, n * sizeof(unsigned long long), s));
        hipLaunchKernelGGL((mst_minpair_kernel<K>), g, blk, 0, s, n, comp, cand_j, cand_key, cmin_key, cmin_pair);
        hipLaunchKernelGGL((mst_emit_kernel<K>), g, blk, 0, s, n, comp, cmin_key, cmin_pair, parent, e_key, e_pair, ctr);
        MSTCHK(hipMemsetAsync(ctr, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(mst_relabel_kernel, g, blk, 0, s, n, parent, comp, ctr);
        MSTCHK(hipGetLastError());
        return PN_OK;
    };

    uint64_t rounds = 0, scanned = 0;
    // ---- round 0: every row is listed (or answered by the 1-NN self-query)
    if (a.nn_idx && a.nn_dist) {
        hipLaunchKernelGGL((mst_seed_kernel<T>), g, blk, 0, s, n, a.nn_idx, (const T *)a.nn_dist, a.index_base, cosm, cand_j,
                           cand_key);
        MSTCHK(hipGetLastError());
    } else {
        int rc = scan_listed(n);
        if (rc != PN_OK) return rc;
    }
    scanned += n;
    {
        int rc = choose_emit_relabel();
        if (rc != PN_OK) return rc;
    }
    rounds = 1;
    size_t ncomp_prev = n;
    for (;;) {
        // the next round's list, enqueued before the host looks: one wait per round
        int rc = min_keys();
        if (rc != PN_OK) return rc;
        hipLaunchKernelGGL((mst_flag_kernel<K>), g, blk, 0, s, n, comp, cand_j, ckey, cmin_key, flag);
        MSTCHK(hipGetLastError());
        MSTCHK(launch_exclusive_scan_u32(flag, n, off, scan, nullptr, s));
        hipLaunchKernelGGL(mst_list_kernel, g, blk, 0, s, n, flag, off, list);
        MSTCHK(hipGetLastError());
        uint64_t nlist = 0;
        uint32_t h_ctr[2] = {0, 0};
        MSTCHK(hipMemcpyAsync(&nlist, off + n, sizeof nlist, hipMemcpyDeviceToHost, s));
        MSTCHK(hipMemcpyAsync(h_ctr, ctr, sizeof h_ctr, hipMemcpyDeviceToHost, s));
        MSTCHK(hipStreamSynchronize(s));
        const size_t ncomp = h_ctr[0];
        if (ncomp < 1 || ncomp >= ncomp_prev || (size_t)h_ctr[1] != n - ncomp || nlist > n)
            return set_error(PN_ERR_DEVICE, "MST round %llu: %u edges for %zu -> %zu components (internal error)",
                             (unsigned long long)rounds, h_ctr[1], ncomp_prev, ncomp);
        if (ncomp == 1) break;
        ncomp_prev = ncomp;
        rc = scan_listed((size_t)nlist);
        if (rc != PN_OK) return rc;
        scanned += nlist;
        rc = choose_emit_relabel();
        if (rc != PN_OK) return rc;
        ++rounds;
    }
    // ---- the n - 1 edges in edge order
    const size_t ne = n - 1, N2 = L.N2;
    if (N2 > ne) {
        hipLaunchKernelGGL((mst_sort_pad_kernel<K>), rows_grid(N2 - ne), blk, 0, s, ne, N2, e_key, e_pair);
        MSTCHK(hipGetLastError());
    }
    MSTCHK(sort_key_pair<K>(e_key, e_pair, N2, s));
    hipLaunchKernelGGL((mst_output_kernel<T>), rows_grid(ne), blk, 0, s, ne, e_key, e_pair, a.index_base, cosm, a.d_src, a.d_dst,
                       (T *)a.d_weight);
    MSTCHK(hipGetLastError());
    a.work[0] = rounds;
    a.work[1] = scanned;
    return PN_OK;
}

size_t mst_buffer_bytes(size_t n, int elem_bytes, size_t batch, int n_cu) {
    if (n < 2) return 0;
    return Layout(n, elem_bytes, batch ? batch : 1, n_cu).total;
}
size_t sort_key_pair_len(size_t count) {
    size_t N = kSortBlock;
    while (N < count) N <<= 1;
    return N;
}
hipError_t launch_sort_key_pair_u64(uint64_t *key, unsigned long long *pair, size_t N, hipStream_t s) {
    return sort_key_pair<uint64_t>(key, pair, N, s);
}
template int mst_enqueue<float>(MstArgs &, hipStream_t);
template int mst_enqueue<double>(MstArgs &, hipStream_t);

}  // namespace pn
