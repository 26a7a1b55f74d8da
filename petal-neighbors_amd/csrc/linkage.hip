// linkage.hip -- the single-linkage dendrogram of a sorted spanning tree (pn_linkage_*) and HDBSCAN's cluster extraction
// from it (pn_hdbscan_*): condensed tree, stability, excess-of-mass selection, labels and probabilities, all in HBM and
// without a host wait.  No step walks the dendrogram: its height can be n - 1.
//
// ---- Part 1: the dendrogram.  Edge r (rank r of the n - 1 sorted edges) makes node n + r; its children are the current
// components of its two ends.  A component is NAMED by a row (a singleton) or by n + q, q = its highest edge so far, so a
// name is a node id.  a[r], b[r] hold the names of edge r's ends, initially the rows themselves.  Divide and conquer on
// the rank: S = the least power of two above n - 1; for half = S / 2, S / 4, ..., 1 the ranks fall into aligned segments
// of 2 * half, and all segments of a level run in the same four launches over the edges:
//   hook     low-half edges ((r & half) == 0) unite a[r] and b[r] in a union-find over the 2n - 1 names (union_find.h)
//   claim    per low-half edge: root = find(a[r]); top[root] <- max r; each end's name, the first time it is met this
//            level (mark), adds its size to acc[root]
//   rename   the low-half edge with top[root] == r writes sz[n + r] = acc[root]; a high-half edge replaces an end's name
//            x, if marked, by n + top[find(x)]
//   reset    low-half edges put parent / top / acc / mark of their ends' names back
// Invariant: at the start of a level the names of every edge of a segment [lo, hi) are the components under the edges of
// rank < lo.  The level's low half unites exactly the names that the edges [lo, mid) touch, so afterwards the high half
// holds the components under rank < mid and the low half is unchanged.  After half = 1 the names of edge r are the
// components under rank < r: the children of node n + r.  Names of different segments of a level are disjoint (an end
// that a lower segment touches has, for any higher segment, been merged into a component with a higher top), so one
// parent[] serves all segments.  Node n + r is the top of its low half's component at the level whose
// midpoint is r + 1 (S > n - 1: every r + 1 is a midpoint), so every size is written, from sizes written at coarser
// levels; a later level may write the same value again.  All sums are integer atomics: the result depends on the edges
// alone.  Edges that are no spanning tree leave the root short of n rows: the error word.
//
// ---- Part 2: the extraction (the contract: petal_mi355x.h).  With m = min_cluster_size, a node is big when it holds
// >= m rows, a true split when both children are big; cluster tops are the root and the children of true splits.  The big
// nodes of one cluster are a PATH from its top down to its bottom (a true split, or a node with two small children), and
// all rows that fall out at a big node share its lambda, so
//     stability(c) = sum over the path of  w(v) * (lambda(v) - birth(c)),   w = rows in v's small children, or size(v)
// at the ending split -- a sum along a path, done by pointer doubling over double-buffered (sum, up) pairs: its shape is
// fixed by the tree, no floating-point atomics.  Edge ranks ascend in key order and lambda falls with the key, so the
// largest lambda of a cluster is its bottom's: death(c) = lambda(bottom(c)).
//   jump     nearest ancestor-or-self with a flag, in place, ceil(log2(2n)) rounds: jA (big: a(p)), jC (cluster top);
//            a racing read sees an older or a newer pointer, both on the path and not past the flag
//   select   bottom-up over the cluster tree: a leaf cluster's thread climbs while it is the second child to arrive
//            (arrival counter per split; a + b commutes, so the order of arrival does not matter)
//   jF, jS   nearest flagged cluster, then nearest SELECTED (flagged, no flagged ancestor) over the cluster parents
//   number   minrow[c] <- atomic min of member rows; a flag at each such row; exclusive scan
// Visibility: parent[] by union_find.h's rule; top / acc / mark / minrow / arrive / best are touched by agent-scope
// atomics inside the kernel that builds them and read plainly by later launches only; the jump arrays as said above.
#include "../../include/petal_mi355x.h"
#include "pn_internal.h"
#include "union_find.h"

#include <utility>

namespace pn {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

dim3 grid_of(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
int rounds_for(size_t len) {  // the least k with 2^k >= len
    int k = 0;
    while (((size_t)1 << k) < len) ++k;
    return k;
}

// ------------------------------------------------------------------------------------------------ part 1: linkage
template <typename T>
__global__ __launch_bounds__(256) void lk_init_kernel(size_t n, const uint64_t *__restrict__ src,
                                                      const uint64_t *__restrict__ dst, const T *w_in, uint64_t base,
                                                      uint32_t *__restrict__ a, uint32_t *__restrict__ b,
                                                      uint32_t *__restrict__ parent, uint32_t *__restrict__ top,
                                                      uint32_t *__restrict__ acc, uint32_t *__restrict__ mark,
                                                      uint32_t *__restrict__ sz, T *w_out, uint32_t *__restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * n - 1) return;
    parent[i] = (uint32_t)i;
    top[i] = acc[i] = mark[i] = 0;
    sz[i] = i < n ? 1u : 0u;
    if (i + 1 < n) {
        uint64_t s = src[i] - base, d = dst[i] - base;
        if (s >= n || d >= n) {  // not a row: the call fails; the edge is kept harmless
            *bad = 1;
            s = d = 0;
        }
        a[i] = (uint32_t)s;
        b[i] = (uint32_t)d;
        if (w_out && w_out != w_in) w_out[i] = w_in[i];
    }
}
__global__ __launch_bounds__(256) void lk_hook_kernel(size_t ne, size_t half, const uint32_t *__restrict__ a,
                                                      const uint32_t *__restrict__ b, uint32_t *parent) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ne || (r & half)) return;
    (void)uf_unite(parent, a[r], b[r]);
}
__global__ __launch_bounds__(256) void lk_claim_kernel(size_t ne, size_t half, const uint32_t *__restrict__ a,
                                                       const uint32_t *__restrict__ b, const uint32_t *__restrict__ sz,
                                                       uint32_t *parent, uint32_t *top, uint32_t *acc, uint32_t *mark) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ne || (r & half)) return;
    const uint32_t x = a[r], y = b[r];
    const uint32_t root = uf_find(parent, x);
    atomicMax(top + root, (uint32_t)r);
    if (atomicExch(mark + x, 1u) == 0u) atomicAdd(acc + root, sz[x]);
    if (atomicExch(mark + y, 1u) == 0u) atomicAdd(acc + root, sz[y]);
}
__global__ __launch_bounds__(256) void lk_rename_kernel(size_t n, size_t ne, size_t half, uint32_t *__restrict__ a,
                                                        uint32_t *__restrict__ b, uint32_t *parent,
                                                        const uint32_t *__restrict__ top, const uint32_t *__restrict__ acc,
                                                        const uint32_t *__restrict__ mark, uint32_t *sz) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ne) return;
    if (!(r & half)) {
        const uint32_t root = uf_find(parent, a[r]);
        if (top[root] == (uint32_t)r) sz[n + r] = acc[root];
        return;
    }
    const uint32_t x = a[r], y = b[r];
    if (mark[x]) a[r] = (uint32_t)n + top[uf_find(parent, x)];
    if (mark[y]) b[r] = (uint32_t)n + top[uf_find(parent, y)];
}
__global__ __launch_bounds__(256) void lk_reset_kernel(size_t ne, size_t half, const uint32_t *__restrict__ a,
                                                       const uint32_t *__restrict__ b, uint32_t *parent, uint32_t *top,
                                                       uint32_t *acc, uint32_t *mark) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ne || (r & half)) return;
    const uint32_t x = a[r], y = b[r];
    parent[x] = x;
    parent[y] = y;
    top[x] = top[y] = 0;
    acc[x] = acc[y] = 0;
    mark[x] = mark[y] = 0;
}
__global__ __launch_bounds__(256) void lk_output_kernel(size_t n, const uint32_t *__restrict__ a,
                                                        const uint32_t *__restrict__ b, const uint32_t *__restrict__ sz,
                                                        const uint32_t *__restrict__ bad, uint64_t *__restrict__ left,
                                                        uint64_t *__restrict__ right, uint64_t *__restrict__ size,
                                                        int32_t *__restrict__ err) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r + 1 >= n) return;
    if (left) {
        left[r] = a[r];
        right[r] = b[r];
        size[r] = sz[n + r];
    }
    if (err && r + 2 == n) *err = (*bad || sz[n + r] != (uint32_t)n) ? PN_ERR_INVALID : PN_OK;
}

// the scratch of part 1, u32 words: a, b [n - 1]; parent, top, acc, mark, sz [2n - 1]; bad [1]
struct LinkLayout {
    size_t ne, N, words;
    explicit LinkLayout(size_t n) : ne(n - 1), N(2 * n - 1), words(2 * (n - 1) + 5 * (2 * n - 1) + 1) {}
};

#define LKCHK(expr)                                                                                          \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return set_error(e_ == hipErrorOutOfMemory ? PN_ERR_NOMEM : PN_ERR_DEVICE, "%s: %s", #expr,      \
                             hipGetErrorString(e_));                                                         \
    } while (0)

}  // namespace

template <typename T>
int linkage_enqueue(const LinkageArgs &g, hipStream_t s) {
    const size_t n = g.n;
    if (n < 2) return PN_OK;
    const LinkLayout L(n);
    const size_t ne = L.ne, N = L.N;
    uint32_t *a = (uint32_t *)g.buf, *b = a + ne, *parent = b + ne, *top = parent + N, *acc = top + N, *mark = acc + N,
             *sz = mark + N, *bad = sz + N;
    const dim3 blk(256), ge = grid_of(ne);
    LKCHK(hipMemsetAsync(bad, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL((lk_init_kernel<T>), grid_of(N), blk, 0, s, n, g.d_src, g.d_dst, (const T *)g.d_weight, g.index_base, a, b,
                       parent, top, acc, mark, sz, (T *)g.d_weight_out, bad);
    size_t S = 2;
    while (S <= ne) S <<= 1;
    for (size_t half = S / 2; half >= 1; half >>= 1) {
        hipLaunchKernelGGL(lk_hook_kernel, ge, blk, 0, s, ne, half, a, b, parent);
        hipLaunchKernelGGL(lk_claim_kernel, ge, blk, 0, s, ne, half, a, b, sz, parent, top, acc, mark);
        hipLaunchKernelGGL(lk_rename_kernel, ge, blk, 0, s, n, ne, half, a, b, parent, top, acc, mark, sz);
        if (half > 1) hipLaunchKernelGGL(lk_reset_kernel, ge, blk, 0, s, ne, half, a, b, parent, top, acc, mark);
    }
    LKCHK(hipGetLastError());
    if (g.d_left || g.d_err) {
        hipLaunchKernelGGL(lk_output_kernel, ge, blk, 0, s, n, a, b, sz, bad, g.d_left, g.d_right, g.d_size, g.d_err);
        LKCHK(hipGetLastError());
    }
    return PN_OK;
}
template int linkage_enqueue<float>(const LinkageArgs &, hipStream_t);
template int linkage_enqueue<double>(const LinkageArgs &, hipStream_t);

namespace {
// --------------------------------------------------------------------------------------------- part 2: extraction
// lambda of a merge weight, in f64: 1 / w above 2^-100, 2^100 at or below it (duplicates, Cosine's non-positive weights:
// finite, so no inf - inf), 0 for NaN
__device__ __forceinline__ double lambda_of(double w) {
    if (w != w) return 0.0;
    return w > 0x1p-100 ? 1.0 / w : 0x1p100;
}

// the dendrogram as the kernels see it: node v >= n is merge v - n with children l / r; sz over all 2n - 1 nodes
template <typename T>
struct Dendro {
    size_t n;
    uint32_t m;
    const uint32_t *l, *r, *sz, *par;
    const T *w;
    __device__ __forceinline__ uint32_t root() const { return (uint32_t)(2 * n - 2); }
    __device__ __forceinline__ bool big(uint32_t v) const { return sz[v] >= m; }
    __device__ __forceinline__ bool split(uint32_t v) const { return v >= n && sz[l[v - n]] >= m && sz[r[v - n]] >= m; }
    __device__ __forceinline__ bool is_top(uint32_t v) const { return v == root() || split(par[v]); }
    __device__ __forceinline__ double lambda(uint32_t v) const { return lambda_of((double)w[v - n]); }
    __device__ __forceinline__ double birth(uint32_t c) const { return c == root() ? 0.0 : lambda(par[c]); }
};

__global__ __launch_bounds__(256) void hx_parent_kernel(size_t n, const uint32_t *__restrict__ l,
                                                        const uint32_t *__restrict__ r, uint32_t *__restrict__ par) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e + 1 >= n) return;
    par[l[e]] = par[r[e]] = (uint32_t)(n + e);
    if (e + 2 == n) par[n + e] = (uint32_t)(n + e);
}
// jA[v]: v itself when big (or the root), else its parent; jC[v]: v itself when a cluster top, else its parent
template <typename T>
__global__ __launch_bounds__(256) void hx_jump_init_kernel(Dendro<T> t, uint32_t *__restrict__ jA, uint32_t *__restrict__ jC) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= 2 * t.n - 1) return;
    const uint32_t p = t.par[v];
    jA[v] = t.big((uint32_t)v) ? (uint32_t)v : p;
    jC[v] = t.is_top((uint32_t)v) ? (uint32_t)v : p;
}
// one doubling round, in place (x nullable / y nullable)
__global__ __launch_bounds__(256) void hx_jump_kernel(size_t N, uint32_t *x, uint32_t *y) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    if (x) {
        const uint32_t p = x[v], q = x[p];
        if (q != p) x[v] = q;
    }
    if (y) {
        const uint32_t p = y[v], q = y[p];
        if (q != p) y[v] = q;
    }
}
// the path sums' start: sum[v] = v's own term, up[v] = the next node of its cluster's path (kNone at the top)
template <typename T>
__global__ __launch_bounds__(256) void hx_term_kernel(Dendro<T> t, const uint32_t *__restrict__ jC, double *__restrict__ sum,
                                                      uint32_t *__restrict__ up) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 >= t.n) return;
    const uint32_t v = (uint32_t)(t.n + i);
    double term = 0.0;
    uint32_t u = kNone;
    if (t.big(v)) {
        const uint32_t sl = t.sz[t.l[i]], sr = t.sz[t.r[i]];
        const uint32_t cnt = (sl >= t.m && sr >= t.m) ? t.sz[v] : (sl < t.m ? sl : 0u) + (sr < t.m ? sr : 0u);
        term = (double)cnt * (t.lambda(v) - t.birth(jC[v]));
        if (!t.is_top(v)) u = t.par[v];
    }
    sum[v] = term;
    up[v] = u;
}
__global__ __launch_bounds__(256) void hx_sum_kernel(size_t n, const double *__restrict__ s_in, const uint32_t *__restrict__ u_in,
                                                     double *__restrict__ s_out, uint32_t *__restrict__ u_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 >= n) return;
    const size_t v = n + i;
    const uint32_t u = u_in[v];
    if (u == kNone) {
        s_out[v] = s_in[v];
        u_out[v] = kNone;
    } else {
        s_out[v] = s_in[v] + s_in[u];
        u_out[v] = u_in[u];
    }
}
// every cluster's bottom hands its path sum to the cluster: stab[top], bot[top]
template <typename T>
__global__ __launch_bounds__(256) void hx_bottom_kernel(Dendro<T> t, const uint32_t *__restrict__ jC,
                                                        const double *__restrict__ sum, double *__restrict__ stab,
                                                        uint32_t *__restrict__ bot) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 >= t.n) return;
    const uint32_t v = (uint32_t)(t.n + i);
    if (!t.big(v)) return;
    const bool bl = t.big(t.l[i]), br = t.big(t.r[i]);
    if (bl != br) return;  // one big child: the path goes on
    const uint32_t c = jC[v];
    stab[c] = sum[v];
    bot[c] = v;
}
__device__ __forceinline__ void best_store(double *p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), (unsigned long long)__double_as_longlong(v),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double best_load(double *p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long *>(p), __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
}
// excess of mass, bottom-up: one thread per leaf cluster; at a split the second child to arrive goes on with the parent
template <typename T>
__global__ __launch_bounds__(256) void hx_select_kernel(Dendro<T> t, const uint32_t *__restrict__ jC,
                                                        const double *__restrict__ stab, double *best, uint32_t *arrive,
                                                        uint32_t *flagged) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 >= t.n) return;
    const uint32_t v = (uint32_t)(t.n + i), root = t.root();
    if (!t.big(v) || t.big(t.l[i]) || t.big(t.r[i])) return;
    uint32_t c = jC[v];
    if (c == root) return;
    flagged[c] = 1;  // (no children: their sum, 0, is not above a stability)
    double mine = stab[c];
    for (;;) {
        const uint32_t sp = t.par[c];
        best_store(best + c, mine);
        if (__hip_atomic_fetch_add(arrive + sp, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
        const uint32_t sib = t.l[sp - t.n] == c ? t.r[sp - t.n] : t.l[sp - t.n];
        const double kids = mine + best_load(best + sib);
        c = jC[sp];
        if (c == root) return;  // never flagged
        const double own = stab[c];
        if (kids > own) {
            mine = kids;
        } else {
            flagged[c] = 1;
            mine = own;
        }
    }
}
// over the cluster tops: jF[c] = c when flagged (or the root), else the parent cluster; other nodes point at themselves
template <typename T>
__global__ __launch_bounds__(256) void hx_flag_init_kernel(Dendro<T> t, const uint32_t *__restrict__ jC,
                                                           const uint32_t *__restrict__ flagged, uint32_t *__restrict__ jF) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= 2 * t.n - 1) return;
    uint32_t to = (uint32_t)v;
    if (v != t.root() && t.big((uint32_t)v) && t.is_top((uint32_t)v) && !flagged[v]) to = jC[t.par[v]];
    jF[v] = to;
}
// jS[c] = c when selected -- flagged, and no flagged cluster above -- (or the root), else the parent cluster
template <typename T>
__global__ __launch_bounds__(256) void hx_sel_init_kernel(Dendro<T> t, const uint32_t *__restrict__ jC,
                                                          const uint32_t *__restrict__ flagged, const uint32_t *__restrict__ jF,
                                                          uint32_t *__restrict__ jS) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= 2 * t.n - 1) return;
    uint32_t to = (uint32_t)v;
    if (v != t.root() && t.big((uint32_t)v) && t.is_top((uint32_t)v)) {
        const uint32_t cp = jC[t.par[v]];
        if (!flagged[v] || flagged[jF[cp]]) to = cp;
    }
    jS[v] = to;
}
__global__ __launch_bounds__(256) void hx_minrow_kernel(size_t n, const uint32_t *__restrict__ jC,
                                                        const uint32_t *__restrict__ jS, uint32_t *minrow) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t c = jS[jC[p]];
    if (c != (uint32_t)(2 * n - 2)) atomicMin(minrow + c, (uint32_t)p);
}
__global__ __launch_bounds__(256) void hx_rowflag_kernel(size_t n, const uint32_t *__restrict__ minrow,
                                                         uint32_t *__restrict__ rowflag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 >= n) return;
    const uint32_t p = minrow[n + i];
    if (p != kNone) rowflag[p] = 1;
}
template <typename T>
__global__ __launch_bounds__(256) void hx_label_kernel(Dendro<T> t, const uint32_t *__restrict__ jA,
                                                       const uint32_t *__restrict__ jC, const uint32_t *__restrict__ jS,
                                                       const uint32_t *__restrict__ minrow, const uint32_t *__restrict__ bot,
                                                       const uint64_t *__restrict__ num, int64_t *__restrict__ labels,
                                                       T *__restrict__ prob) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= t.n) return;
    const uint32_t c = jS[jC[p]];
    if (c == t.root()) {
        labels[p] = -1;
        if (prob) prob[p] = (T)0;
        return;
    }
    labels[p] = (int64_t)num[minrow[c]];
    if (prob) {
        const double death = t.lambda(bot[c]), lp = t.lambda(jA[p]);
        prob[p] = death == 0.0 ? (T)1 : (T)((lp < death ? lp : death) / death);
    }
}

// the scratch of part 2 after part 1's: f64 sum0, sum1, best [N]; u64 num [n + 1], scan; u32 par, jA, jC, up0, up1, bot,
// minrow [N], rowflag [n].  jF / arrive / flagged / jS reuse part 1's parent / top / acc / mark.
struct ExtractLayout {
    size_t link_bytes, N, scan_words, o_f64, o_u64, o_u32, total;
    explicit ExtractLayout(size_t n) {
        link_bytes = round_up(LinkLayout(n).words * 4, (size_t)16);
        N = 2 * n - 1;
        scan_words = n / 4096 + 2;
        o_f64 = link_bytes;
        o_u64 = o_f64 + 3 * N * 8;
        o_u32 = o_u64 + (n + 1 + scan_words) * 8;
        total = o_u32 + (7 * N + n) * 4;
    }
};

}  // namespace

template <typename T>
int hdbscan_extract_enqueue(const HdbscanArgs &g, hipStream_t s) {
    const size_t n = g.n, N = 2 * n - 1, ne = n - 1;
    const LinkLayout L(n);
    const ExtractLayout X(n);
    char *buf = (char *)g.buf;
    uint32_t *a = (uint32_t *)buf, *b = a + ne, *parent = b + ne, *top = parent + N, *acc = top + N, *mark = acc + N,
             *sz = mark + N;
    double *sum0 = (double *)(buf + X.o_f64), *sum1 = sum0 + N, *best = sum1 + N;
    uint64_t *num = (uint64_t *)(buf + X.o_u64), *scan = num + n + 1;
    uint32_t *par = (uint32_t *)(buf + X.o_u32), *jA = par + N, *jC = jA + N, *up0 = jC + N, *up1 = up0 + N, *bot = up1 + N,
             *minrow = bot + N, *rowflag = minrow + N;
    uint32_t *jF = parent, *arrive = top, *flagged = acc, *jS = mark;
    const dim3 blk(256), gN = grid_of(N), ge = grid_of(ne), gn = grid_of(n);
    const Dendro<T> t{n, (uint32_t)g.min_cluster_size, a, b, sz, par, (const T *)g.d_weight};

    hipLaunchKernelGGL(hx_parent_kernel, ge, blk, 0, s, n, a, b, par);
    hipLaunchKernelGGL((hx_jump_init_kernel<T>), gN, blk, 0, s, t, jA, jC);
    const int full = rounds_for(N);
    for (int k = 0; k < full; ++k) hipLaunchKernelGGL(hx_jump_kernel, gN, blk, 0, s, N, jA, jC);
    LKCHK(hipGetLastError());
    // stability: the sums along the clusters' paths
    hipLaunchKernelGGL((hx_term_kernel<T>), ge, blk, 0, s, t, jC, sum0, up0);
    double *si = sum0, *so = sum1;
    uint32_t *ui = up0, *uo = up1;
    for (int k = 0; k < full; ++k) {
        hipLaunchKernelGGL(hx_sum_kernel, ge, blk, 0, s, n, si, ui, so, uo);
        std::swap(si, so);
        std::swap(ui, uo);
    }
    hipLaunchKernelGGL((hx_bottom_kernel<T>), ge, blk, 0, s, t, jC, si, so, bot);  // stab = so from here on
    LKCHK(hipGetLastError());
    // selection
    LKCHK(hipMemsetAsync(arrive, 0, N * sizeof(uint32_t), s));
    LKCHK(hipMemsetAsync(flagged, 0, N * sizeof(uint32_t), s));
    hipLaunchKernelGGL((hx_select_kernel<T>), ge, blk, 0, s, t, jC, so, best, arrive, flagged);
    // (a path of the cluster tree passes at most n / m true splits)
    const int few = rounds_for(n / g.min_cluster_size + 2);
    hipLaunchKernelGGL((hx_flag_init_kernel<T>), gN, blk, 0, s, t, jC, flagged, jF);
    for (int k = 0; k < few; ++k) hipLaunchKernelGGL(hx_jump_kernel, gN, blk, 0, s, N, jF, (uint32_t *)nullptr);
    hipLaunchKernelGGL((hx_sel_init_kernel<T>), gN, blk, 0, s, t, jC, flagged, jF, jS);
    for (int k = 0; k < few; ++k) hipLaunchKernelGGL(hx_jump_kernel, gN, blk, 0, s, N, jS, (uint32_t *)nullptr);
    LKCHK(hipGetLastError());
    // numbering and the outputs
    LKCHK(hipMemsetAsync(minrow, 0xFF, N * sizeof(uint32_t), s));
    LKCHK(hipMemsetAsync(rowflag, 0, n * sizeof(uint32_t), s));
    hipLaunchKernelGGL(hx_minrow_kernel, gn, blk, 0, s, n, jC, jS, minrow);
    hipLaunchKernelGGL(hx_rowflag_kernel, ge, blk, 0, s, n, minrow, rowflag);
    LKCHK(launch_exclusive_scan_u32(rowflag, n, num, scan, g.d_n_clusters, s));
    hipLaunchKernelGGL((hx_label_kernel<T>), gn, blk, 0, s, t, jA, jC, jS, minrow, bot, num, g.d_labels, (T *)g.d_prob);
    LKCHK(hipGetLastError());
    return PN_OK;
}
template int hdbscan_extract_enqueue<float>(const HdbscanArgs &, hipStream_t);
template int hdbscan_extract_enqueue<double>(const HdbscanArgs &, hipStream_t);

namespace {
template <typename T>
__global__ __launch_bounds__(256) void last_column_kernel(const T *__restrict__ d, size_t rows, size_t k, T *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) out[i] = d[i * k + k - 1];
}

}  // namespace

size_t linkage_buffer_bytes(size_t n) { return n < 2 ? 0 : round_up(LinkLayout(n).words * 4, (size_t)16); }

size_t hdbscan_buffer_bytes(size_t n) { return n < 2 ? 0 : ExtractLayout(n).total; }

template <typename T>
hipError_t launch_last_column(const T *d, size_t rows, size_t k, T *out, hipStream_t s) {
    if (rows) hipLaunchKernelGGL((last_column_kernel<T>), grid_of(rows), dim3(256), 0, s, d, rows, k, out);
    return hipGetLastError();
}
template hipError_t launch_last_column<float>(const float *, size_t, size_t, float *, hipStream_t);
template hipError_t launch_last_column<double>(const double *, size_t, size_t, double *, hipStream_t);

}  // namespace pn
