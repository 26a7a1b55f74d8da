// kmeans_init.hip -- greedy k-means++ seeding of the indexed rows (pn_kmeans_init_*): nc rows chosen by D^2 sampling,
// every round trying L candidates and keeping the one that lowers the potential most.  The contract is in the header
// (petal_mi355x.h) and DESIGN.md 4.26; in short, with u_j = (mix32(seed, j) >> 8) * 2^-24:
//   round 0:  the one candidate is row floor(u_0 * n)
//   round t:  L candidates, each picked with the draw u_(1 + (t - 1) L + c) from the weights w_i = (double)m_i^2 (NaN: 0.0),
//             m_i the smallest distance (by key) of row i to the rows chosen so far; candidate c's potential is the
//             TREE256 sum of (double)min(m_i, d(i, c))^2; the smallest potential wins by a strict '<' in trial order
//   TREE256:  blocks of 256 rows summed by the halving tree (t[0:128] + t[128:256], 64 + 64, ... 1), 256 block sums summed
//             by the same tree into a group, the groups added in order
//   a pick:   r = (double)u * total; the first group whose sequential prefix exceeds r, then with r - the prefix before it
//             the first of its 256 block sums, then the first of the block's 256 terms; where rounding leaves no prefix
//             above r, the last entry that is not zero
// Every distance is the fold of km_exact_kernel (diff = c - x; sq = diff * diff; sum += sq in ascending k, the correctly
// rounded sqrt): the bits of pn_euclidean_*.  No floating-point atomics, nothing waits for the host.
//
// The chain of a call, 2 nc launches: sweep_0, (pick_t, sweep_t) for t = 1 .. nc - 1, and a last pick that only decides the
// last round and gathers the chosen rows.  sweep_t reads the corpus once: one 256-thread workgroup per 256-row block, a
// thread per row with its L running sums in registers; it first applies round t - 1's outcome to m (the commit is fused:
// the winner's number is read from device memory), and leaves the L distances per row and the L block sums.  pick_t is
// one workgroup: the group trees (one wave per tree, no barrier inside), the L totals, the winner, then the L three-level
// picks against the winner's sums and the gather of the picked rows into the candidate image of sweep_t.
//
// No MFMA: a potential is a sum of the distances themselves, at the bits of pn_euclidean_*; a bound on a distance is not
// a term of it, and there is nothing to filter (DESIGN.md 4.24 makes the same argument for the silhouette).
//
// This translation unit is compiled with -ffp-contract=off: subtract, multiply and add are separately rounded.
#include "../../include/petal_mi355x.h"
#include "pn_internal.h"

namespace pn {

namespace {

constexpr int kKppRows = 256;      // rows per block of TREE256 = rows per workgroup of the sweep = block sums per group
constexpr int kKppPickThreads = 1024;
constexpr int kKppStateWords = 4 + kKppMaxTrials;  // {winner, error word, -, -, the round's candidate rows}

// K-chunks of 128 bytes per row: eight 16-byte pieces.  The staged chunk is [k][row] with PAD elements behind the 256
// rows: the four (two) coordinates of a piece go to rows k of the chunk that lie 4 (2) PITCH elements apart, so the eight
// pieces p of a row land 8 p banks apart (f32; f64: 16 p, two banks per element) and the eight rows a wave writes at once
// fill the gaps: a wave's 64 stores of one coordinate take the fewest cycles 64 lanes can.  The reads are [k][row] with
// the row on the lane: consecutive addresses, no conflict whatever the pitch.
template <typename T> struct KppShape;
template <> struct KppShape<float> { static constexpr int KC = 32, PAD = 2; };
template <> struct KppShape<double> { static constexpr int KC = 16, PAD = 4; };

typedef unsigned int kpp_u4 __attribute__((ext_vector_type(4)));  // 16 bytes moved as they lie

__device__ __forceinline__ float kpp_sqrt(float x) { return sqrtf(x); }  // correctly rounded (the build's flags)
__device__ __forceinline__ double kpp_sqrt(double x) { return sqrt(x); }
template <typename T> __device__ __forceinline__ T kpp_nan();
template <> __device__ __forceinline__ float kpp_nan<float>() { return __uint_as_float(KeyOf<float>::kNaN); }
template <> __device__ __forceinline__ double kpp_nan<double>() { return __longlong_as_double((long long)KeyOf<double>::kNaN); }
template <typename T>
__device__ __forceinline__ typename KeyOf<T>::type kpp_key(T d) {
    using K = typename KeyOf<T>::type;
    if constexpr (sizeof(T) == 4)
        return d != d ? KeyOf<T>::kNaN : (K)__float_as_uint(d);
    else
        return d != d ? KeyOf<T>::kNaN : (K)__double_as_longlong(d);
}
// the smaller of two distances by the key of pn_kmeans_assign_* (NaN above +inf); a tie keeps m
template <typename T> __device__ __forceinline__ T kpp_min(T m, T d) { return kpp_key<T>(d) < kpp_key<T>(m) ? d : m; }
// the term of a row whose nearest chosen row is e away
template <typename T> __device__ __forceinline__ double kpp_term(T e) {
    const double w = (double)e * (double)e;
    return w != w ? 0.0 : w;
}
// the pieces of a 16-byte load as elements
__device__ __forceinline__ void kpp_split(const kpp_u4 &v, float (&o)[4]) {
    o[0] = __uint_as_float(v.x), o[1] = __uint_as_float(v.y), o[2] = __uint_as_float(v.z), o[3] = __uint_as_float(v.w);
}
__device__ __forceinline__ void kpp_split(const kpp_u4 &v, double (&o)[2]) {
    o[0] = __hiloint2double((int)v.y, (int)v.x), o[1] = __hiloint2double((int)v.w, (int)v.z);
}

// ---- the sweep of one round.  grid: the 256-row blocks; 256 threads, thread r owns row blockIdx.x * 256 + r.
// cand: the round's L candidate rows, candidate c at cand + c * cand_ld (ld elements each, zero beyond dim).  first: round
// 0 -- m starts as NaN, which the key order puts above every distance, and the error word is cleared.  Otherwise the
// commit of the round before: m_i <- min(m_i, cdist[winner][i]), the winner's number read from state[0].
// Out: cdist[c][i] (row stride n), bsum[c][block] (row stride nblocks).
template <typename T, int L>
__global__ __launch_bounds__(kKppRows) void kpp_sweep_kernel(const T *__restrict__ X, size_t n, size_t ld, int nkc,
                                                             const T *__restrict__ cand, size_t cand_ld,
                                                             uint32_t *__restrict__ state, int first, T *__restrict__ m,
                                                             T *__restrict__ cdist, double *__restrict__ bsum,
                                                             size_t nblocks) {
#pragma clang fp contract(off)
    constexpr int KC = KppShape<T>::KC, PITCH = kKppRows + KppShape<T>::PAD;
    constexpr int EPP = 16 / (int)sizeof(T);  // elements per 16-byte piece
    constexpr int PPR = KC / EPP;             // pieces per row of a chunk (8)
    constexpr int XV = PPR;                   // pieces per thread of a chunk of the rows (256 rows x 8 / 256 threads)
    constexpr int UNROLL = L >= 8 ? 1 : L >= 4 ? 2 : 4;  // steps of the fold unrolled together
    extern __shared__ __attribute__((aligned(16))) unsigned char kpp_smem[];
    T *Xs = reinterpret_cast<T *>(kpp_smem);         // [2][KC][PITCH]
    T *Cs = Xs + 2 * KC * PITCH;                     // [2][L][KC]
    double *Ts = reinterpret_cast<double *>(kpp_smem);  // [L][256], once the chunks are folded

    const int tid = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * kKppRows, row = row0 + (size_t)tid;
    const bool live = row < n;

    // the commit of the round before
    T mi = kpp_nan<T>();
    if (first) {
        if (blockIdx.x == 0 && tid == 0) state[1] = 0;
    } else if (live) {
        const uint32_t w = state[0];
        mi = kpp_min<T>(m[row], cdist[(size_t)w * n + row]);
    }
    if (live) m[row] = mi;

    // piece i of a thread: element offset of its row in X, row and first coordinate in the chunk
    const T *xsrc[XV];
    int xdst[XV], xk[XV];
#pragma unroll
    for (int i = 0; i < XV; ++i) {
        const int idx = tid + kKppRows * i, r = idx / PPR, p = idx % PPR;
        xsrc[i] = X + (row0 + (size_t)r) * ld + p * EPP;  // (rows up to n_pad, a multiple of 256, exist)
        xk[i] = p * EPP;
        xdst[i] = p * EPP * PITCH + r;
    }
    const bool has_c = tid < L * PPR;
    const int cc = tid / PPR, cp = (tid % PPR) * EPP;
    const T *csrc = cand + (size_t)(has_c ? cc : 0) * cand_ld + cp;

    kpp_u4 rx[XV], rc;
    const kpp_u4 zero = {0u, 0u, 0u, 0u};
    auto fetch = [&](int kc) {
        const int k0 = kc * KC;
#pragma unroll
        for (int i = 0; i < XV; ++i)
            rx[i] = (size_t)(k0 + xk[i]) < ld ? *reinterpret_cast<const kpp_u4 *>(xsrc[i] + k0) : zero;
        if (has_c) rc = (size_t)(k0 + cp) < ld ? *reinterpret_cast<const kpp_u4 *>(csrc + k0) : zero;
    };
    auto stage = [&](int b) {
        T *xs = Xs + b * (KC * PITCH);
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            T e[EPP];
            kpp_split(rx[i], e);
#pragma unroll
            for (int j = 0; j < EPP; ++j) xs[xdst[i] + j * PITCH] = e[j];
        }
        if (has_c) *reinterpret_cast<kpp_u4 *>(Cs + b * (L * KC) + cc * KC + cp) = rc;
    };

    T acc[L];
#pragma unroll
    for (int c = 0; c < L; ++c) acc[c] = (T)0;

    fetch(0);
    stage(0);
    __syncthreads();
    for (int kc = 0; kc < nkc; ++kc) {
        const bool more = kc + 1 < nkc;
        if (more) fetch(kc + 1);  // (in flight while this chunk is folded)
        const T *xs = Xs + (kc & 1) * (KC * PITCH) + tid;
        const T *cs = Cs + (kc & 1) * (L * KC);
        // (a step holds L pieces of candidate values in registers: unrolled only as far as they leave room)
#pragma unroll UNROLL
        for (int k0 = 0; k0 < KC; k0 += EPP) {
            T x[EPP];
#pragma unroll
            for (int j = 0; j < EPP; ++j) x[j] = xs[(k0 + j) * PITCH];
#pragma unroll
            for (int c = 0; c < L; ++c) {
                T cv[EPP];
                kpp_split(*reinterpret_cast<const kpp_u4 *>(cs + c * KC + k0), cv);  // (one address per wave: a broadcast)
#pragma unroll
                for (int j = 0; j < EPP; ++j) {
                    const T diff = cv[j] - x[j];
                    const T sq = diff * diff;
                    acc[c] = acc[c] + sq;
                }
            }
        }
        if (more) stage((kc + 1) & 1);
        __syncthreads();  // the next chunk is staged, and this one fully read
    }

    // the distances, and the terms into LDS over the staging buffers
#pragma unroll
    for (int c = 0; c < L; ++c) {
        const T d = kpp_sqrt(acc[c]);
        if (live) cdist[(size_t)c * n + row] = d;
        Ts[c * kKppRows + tid] = live ? kpp_term<T>(kpp_min<T>(mi, d)) : 0.0;
    }
    for (int w = kKppRows / 2; w > 0; w >>= 1) {
        __syncthreads();
        if (tid < w) {
#pragma unroll
            for (int c = 0; c < L; ++c) Ts[c * kKppRows + tid] = Ts[c * kKppRows + tid] + Ts[c * kKppRows + tid + w];
        }
    }
    if (tid == 0) {
#pragma unroll
        for (int c = 0; c < L; ++c) bsum[(size_t)c * nblocks + blockIdx.x] = Ts[c * kKppRows];
    }
}

// One level of a pick: the first entry whose sequential prefix exceeds r, else the last entry that is not zero (else 0);
// *before <- the prefix in front of it.
template <typename F>
__device__ __forceinline__ size_t kpp_walk(F get, size_t count, double r, double *before) {
#pragma clang fp contract(off)
    double p = 0.0, p_last = 0.0;
    size_t last = 0;
    for (size_t i = 0; i < count; ++i) {
        const double s = get(i);
        if (s != 0.0) last = i, p_last = p;
        const double pn = p + s;
        if (pn > r) {
            *before = p;
            return i;
        }
        p = pn;
    }
    *before = p_last;
    return last;
}

struct KppBufs {
    double *bsum, *gsum;  // [kKppMaxTrials][nblocks], [kKppMaxTrials][ngroups]
    uint32_t *state;      // [kKppStateWords]
    uint32_t *chosen;     // [nc]
    size_t nblocks, ngroups;
};

// ---- the pick in front of round t (1 <= t < nc), or behind the last round (t = nc: last).  One workgroup.
// l_prev: the candidates of round t - 1, whose block sums and distances lie in bsum / cdist; l_next: those to pick.
template <typename T>
__global__ __launch_bounds__(kKppPickThreads) void kpp_pick_kernel(const T *__restrict__ X, size_t n, size_t ld, int dim,
                                                                   KppBufs b, const T *__restrict__ m,
                                                                   const T *__restrict__ cdist, T *__restrict__ cimg,
                                                                   size_t t, int l_prev, int l_next, uint64_t seed,
                                                                   uint32_t first_row, int last, size_t nc,
                                                                   uint64_t index_base, T *__restrict__ centres,
                                                                   uint64_t *__restrict__ rows, int32_t *__restrict__ err) {
#pragma clang fp contract(off)
    __shared__ double tot[kKppMaxTrials], sh_r[kKppMaxTrials];
    __shared__ size_t sh_blk[kKppMaxTrials], sh_row[kKppMaxTrials];
    __shared__ uint32_t sh_w;
    __shared__ double Ts[kKppMaxTrials * kKppRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // the group trees: a wave per (candidate, group), lane l holding entries l, l + 64, l + 128, l + 192
    for (size_t q = (size_t)wave; q < (size_t)l_prev * b.ngroups; q += kKppPickThreads / 64) {
        const size_t c = q / b.ngroups, g = q % b.ngroups, base = g * kKppRows + (size_t)lane;
        const double *src = b.bsum + c * b.nblocks;
        double v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = base + 64 * j < b.nblocks ? src[base + 64 * j] : 0.0;
        double s = (v[0] + v[2]) + (v[1] + v[3]);  // the steps of width 128 and 64
        for (int w = 32; w > 0; w >>= 1) s = s + __shfl_down(s, w);  // (lanes at and beyond w hold what nobody reads)
        if (lane == 0) b.gsum[c * b.ngroups + g] = s;
    }
    __syncthreads();
    if (tid < l_prev) {
        double s = 0.0;
        for (size_t g = 0; g < b.ngroups; ++g) s = s + b.gsum[(size_t)tid * b.ngroups + g];
        tot[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t w = 0;
        for (int c = 1; c < l_prev; ++c)
            if (tot[c] < tot[w]) w = (uint32_t)c;
        sh_w = w;
        b.chosen[t - 1] = t == 1 ? first_row : b.state[4 + w];
        b.state[0] = w;
        if (!last && !(tot[w] > 0.0)) b.state[1] = 1;  // fewer distinct rows than centres
    }
    __syncthreads();
    const uint32_t w = sh_w;

    if (last) {
        const bool bad = b.state[1] != 0;
        for (size_t q = (size_t)tid; q < nc * (size_t)dim; q += kKppPickThreads)
            centres[q] = bad ? kpp_nan<T>() : X[(size_t)b.chosen[q / (size_t)dim] * ld + q % (size_t)dim];
        if (rows)
            for (size_t q = (size_t)tid; q < nc; q += kKppPickThreads) rows[q] = bad ? ~0ull : index_base + b.chosen[q];
        if (err && tid == 0) *err = bad ? PN_ERR_INVALID : PN_OK;
        return;
    }

    // levels one and two of the picks: the group, then the block
    if (tid < l_next) {
        const uint64_t j = 1 + (uint64_t)(t - 1) * (uint64_t)l_next + (uint64_t)tid;
        const float u = (float)(mix32(seed, j) >> 8) * (1.0f / 16777216.0f);
        const double r = (double)u * tot[w];
        const double *gs = b.gsum + (size_t)w * b.ngroups, *bs = b.bsum + (size_t)w * b.nblocks;
        double before = 0.0;
        const size_t g = kpp_walk([&](size_t i) { return gs[i]; }, b.ngroups, r, &before);
        const double r2 = r - before;
        const size_t b0 = g * kKppRows;
        const size_t blk = kpp_walk([&](size_t i) { return b0 + i < b.nblocks ? bs[b0 + i] : 0.0; }, kKppRows, r2, &before);
        sh_blk[tid] = b0 + blk;  // (below nblocks: an entry beyond is zero and never taken, and entry 0 exists)
        sh_r[tid] = r2 - before;
    }
    __syncthreads();
    // the picked blocks' terms, as the next sweep's commit will leave them
    for (int q = tid; q < l_next * kKppRows; q += kKppPickThreads) {
        const size_t i = sh_blk[q / kKppRows] * kKppRows + (size_t)(q % kKppRows);
        Ts[q] = i < n ? kpp_term<T>(kpp_min<T>(m[i], cdist[(size_t)w * n + i])) : 0.0;
    }
    __syncthreads();
    if (tid < l_next) {
        const double *ts = Ts + tid * kKppRows;
        double before = 0.0;
        size_t r = sh_blk[tid] * kKppRows + kpp_walk([&](size_t i) { return ts[i]; }, kKppRows, sh_r[tid], &before);
        if (r >= n) r = n - 1;  // (never: a row beyond n has the term zero)
        sh_row[tid] = r;
        b.state[4 + tid] = (uint32_t)r;
    }
    __syncthreads();
    for (size_t q = (size_t)tid; q < (size_t)l_next * ld; q += kKppPickThreads) cimg[q] = X[sh_row[q / ld] * ld + q % ld];
}

size_t kpp_up16(size_t b) { return round_up(b, (size_t)16); }

// the carve of KppArgs::buf (every piece 16-byte aligned)
struct KppCarve {
    size_t nblocks, ngroups;
    size_t o_m, o_cdist, o_bsum, o_gsum, o_state, o_chosen, o_cimg, total;
    KppCarve(size_t n, size_t ld, size_t nc, int trials, size_t eb) {
        nblocks = (n + kKppRows - 1) / kKppRows;
        ngroups = (nblocks + kKppRows - 1) / kKppRows;
        size_t o = 0;
        o_m = o, o += kpp_up16(n * eb);
        o_cdist = o, o += kpp_up16((size_t)trials * n * eb);
        o_bsum = o, o += kpp_up16((size_t)trials * nblocks * 8);
        o_gsum = o, o += kpp_up16((size_t)trials * ngroups * 8);
        o_state = o, o += kpp_up16(kKppStateWords * 4);
        o_chosen = o, o += kpp_up16(nc * 4);
        o_cimg = o, o += kpp_up16((size_t)trials * ld * eb);
        total = o;
    }
};

template <typename T, int L>
hipError_t kpp_launch_sweep(const T *X, size_t n, size_t ld, int nkc, const T *cand, uint32_t *state, int first, T *m,
                            T *cdist, double *bsum, size_t nblocks, hipStream_t s) {
    constexpr int KC = KppShape<T>::KC, PITCH = kKppRows + KppShape<T>::PAD;
    // LDS: the two staging buffers of the rows and of the candidates (the block's terms lie over them afterwards)
    constexpr size_t lds = (size_t)2 * KC * (PITCH + L) * sizeof(T);
    static_assert(lds >= (size_t)L * kKppRows * sizeof(double), "the terms fit over the staging buffers");
    static LdsAttrOnce once;
    const hipError_t e = once.ensure((const void *)kpp_sweep_kernel<T, L>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((kpp_sweep_kernel<T, L>), dim3((unsigned)nblocks), dim3(kKppRows), lds, s, X, n, ld, nkc, cand, ld, state,
                       first, m, cdist, bsum, nblocks);
    return hipSuccess;
}
template <typename T, int L = kKppMaxTrials>
hipError_t kpp_sweep(int trials, const T *X, size_t n, size_t ld, int nkc, const T *cand, uint32_t *state, int first, T *m,
                     T *cdist, double *bsum, size_t nblocks, hipStream_t s) {
    if (trials == L) return kpp_launch_sweep<T, L>(X, n, ld, nkc, cand, state, first, m, cdist, bsum, nblocks, s);
    if constexpr (L > 1) return kpp_sweep<T, L - 1>(trials, X, n, ld, nkc, cand, state, first, m, cdist, bsum, nblocks, s);
    return hipErrorInvalidValue;
}

}  // namespace

size_t kpp_buffer_bytes(size_t n, size_t ld, size_t nc, int trials, int elem_bytes) {
    return KppCarve(n, ld, nc, trials, (size_t)elem_bytes).total;
}

template <typename T>
hipError_t kpp_enqueue(const KppArgs &a, hipStream_t s) {
    const size_t n = a.n, nc = a.nc;
    const int L = a.trials, KC = KppShape<T>::KC;
    const KppCarve cv(n, a.ld, nc, L, sizeof(T));
    char *base = (char *)a.buf;
    T *m = (T *)(base + cv.o_m), *cdist = (T *)(base + cv.o_cdist), *cimg = (T *)(base + cv.o_cimg);
    KppBufs b;
    b.bsum = (double *)(base + cv.o_bsum), b.gsum = (double *)(base + cv.o_gsum);
    b.state = (uint32_t *)(base + cv.o_state), b.chosen = (uint32_t *)(base + cv.o_chosen);
    b.nblocks = cv.nblocks, b.ngroups = cv.ngroups;
    const T *X = (const T *)a.X;
    int nkc = (a.dim + KC - 1) / KC;
    if (nkc < 1) nkc = 1;

    const float u0 = (float)(mix32(a.seed, 0) >> 8) * (1.0f / 16777216.0f);
    size_t first_row = (size_t)((double)u0 * (double)n);  // (below n: u0 <= 1 - 2^-24 and n < 2^31)
    if (first_row >= n) first_row = n - 1;

    hipError_t e = kpp_sweep<T>(1, X, n, a.ld, nkc, X + first_row * a.ld, b.state, 1, m, cdist, b.bsum, cv.nblocks, s);
    if (e != hipSuccess) return e;
    for (size_t t = 1; t <= nc; ++t) {
        const int last = t == nc;
        hipLaunchKernelGGL((kpp_pick_kernel<T>), dim3(1), dim3(kKppPickThreads), 0, s, X, n, a.ld, a.dim, b, (const T *)m,
                           (const T *)cdist, cimg, t, t == 1 ? 1 : L, L, a.seed, (uint32_t)first_row, last, nc, a.index_base,
                           (T *)a.centres, a.rows, a.err);
        if (last) break;
        e = kpp_sweep<T>(L, X, n, a.ld, nkc, cimg, b.state, 0, m, cdist, b.bsum, cv.nblocks, s);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}
template hipError_t kpp_enqueue<float>(const KppArgs &, hipStream_t);
template hipError_t kpp_enqueue<double>(const KppArgs &, hipStream_t);

}  // namespace pn
