// silhouette.hip -- silhouette values of a labelling of the indexed rows (pn_silhouette_*): every (scored row, member)
// distance in the reference's fold, reduced per (row, cluster) on the fly.  O(n) results, no n x n matrix.  The contract
// is in the header (petal_mi355x.h) and DESIGN.md 4.24; in short, with the members (rows with a code in [0, n_clusters))
// sorted by (code, row number) into positions 0 .. M - 1, cut into spans of L = sil_span_len(n) positions:
//   d(i, j)  = sqrt(((0 + (x_i0 - x_j0)^2) + (x_i1 - x_j1)^2) + ...) in T, the bits of pn_pairwise_*, widened to f64
//   Q(i,C,t) = ((0.0 + d(i, j_0)) + d(i, j_1)) + ...  over the members j != i of C at positions [128 t, 128 t + 128)
//   P(i,C,s) = ((0.0 + Q(i,C,t_0)) + Q(i,C,t_1)) + ... over the tiles t of span s that hold members of C, ascending
//   S(i, C)  = (P(i,C,s_0) + P(i,C,s_1)) + ...         over the spans that hold members of C, ascending
// (three levels, so that the rounding of a 10^5-member sum stays a few ulp: a plain sequential fold would show in f64)
//   a(i) = S(i, A) / (|A| - 1),  b(i) = min over C != A of S(i, C) / |C| (ties: the lowest C),  s = (b - a) / max(a, b)
// A span is a fixed range of positions, so the shape of every sum follows from the codes and n alone: not from the
// device, the grid, the row tile a row falls into or the rows asked for.  No floating-point atomics.
//
// The chain of a call: keys (code << 32 | row, excluded rows behind every cluster) -> one sort -> M and the validation
// word -> the members gathered into the cluster-ordered image, the scored rows into theirs -> the sweep, one workgroup
// per (tile of scored rows, span) -> the finish, one thread per scored row over its spans -> the mean.
//
// The images are stored the way the sweep stages them: [tile][K-chunk][k][row of the tile], so a K-chunk of a tile is one
// contiguous block that goes to LDS in 16-byte pieces as it lies, and the per-coordinate reads of a thread are whole
// 16-byte LDS reads without bank conflicts (see sil_sweep_kernel).
//
// This translation unit is compiled with -ffp-contract=off: subtract, multiply and add are separately rounded.
#include "../../include/petal_mi355x.h"
#include "pn_internal.h"

namespace pn {

namespace {

constexpr int kSilTC = 128;                 // members (columns) per tile of the sweep
constexpr int kSilKC = 16;                  // coordinates per staged chunk
constexpr uint32_t kSilNone = 0xFFFFFFFFu;  // no cluster (padding, nothing open)
constexpr uint32_t kSilExcl = 0x7FFFFFFFu;  // an excluded row's key code: behind every cluster (n_clusters <= 2^31 - 1)
constexpr size_t kSilMinSpan = 8192, kSilMaxSpans = 16;
constexpr unsigned long long kSilErrCode = 1, kSilErrClusters = 2, kSilErrRow = 4;  // bits of meta[1]

__device__ __forceinline__ double sil_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ double sil_inf() { return __longlong_as_double(0x7FF0000000000000ll); }
__device__ __forceinline__ float sil_sqrt(float x) { return sqrtf(x); }  // correctly rounded (the build's flags)
__device__ __forceinline__ double sil_sqrt(double x) { return sqrt(x); }

typedef unsigned int sil_u4 __attribute__((ext_vector_type(4)));  // 16 bytes moved as they lie
// four consecutive elements of LDS, as whole 16-byte reads / writes (p 16-byte aligned)
__device__ __forceinline__ void sil_ld4(const float *p, float (&o)[4]) {
    const float4 v = *reinterpret_cast<const float4 *>(p);
    o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
}
__device__ __forceinline__ void sil_ld4(const double *p, double (&o)[4]) {
    const double2 u = *reinterpret_cast<const double2 *>(p), v = *reinterpret_cast<const double2 *>(p + 2);
    o[0] = u.x, o[1] = u.y, o[2] = v.x, o[3] = v.y;
}
__device__ __forceinline__ void sil_st4(float *p, const float (&o)[4]) {
    *reinterpret_cast<float4 *>(p) = make_float4(o[0], o[1], o[2], o[3]);
}
__device__ __forceinline__ void sil_st4(double *p, const double (&o)[4]) {
    *reinterpret_cast<double2 *>(p) = make_double2(o[0], o[1]);
    *reinterpret_cast<double2 *>(p + 2) = make_double2(o[2], o[3]);
}

// ---- preparation
// key[i] <- code << 32 | i (a code outside [0, nc): the excluded code; i >= n: all ones), pair[i] <- i; a code >= nc
// raises the validation word
__global__ __launch_bounds__(256) void sil_keys_kernel(const int64_t *__restrict__ codes, size_t n, size_t N, uint64_t nc,
                                                       uint64_t *__restrict__ key, unsigned long long *__restrict__ pair,
                                                       unsigned long long *__restrict__ meta) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    uint64_t k = ~0ull;
    if (i < n) {
        const int64_t c = codes[i];
        uint64_t code = kSilExcl;
        if (c >= 0) {
            if ((uint64_t)c < nc)
                code = (uint64_t)c;
            else
                atomicOr(meta + 1, kSilErrCode);
        }
        k = (code << 32) | (uint64_t)i;
    }
    key[i] = k;
    pair[i] = (unsigned long long)i;
}
// meta[0] <- M, the members' count (the first sorted position of an excluded row); fewer than two clusters among them
// raises the validation word
__global__ void sil_meta_kernel(const uint64_t *__restrict__ key, size_t n, unsigned long long *__restrict__ meta) {
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t want = (uint64_t)kSilExcl << 32;
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (key[mid] < want)
            lo = mid + 1;
        else
            hi = mid;
    }
    meta[0] = (unsigned long long)lo;
    if (lo == 0 || (key[0] >> 32) == (key[lo - 1] >> 32)) atomicOr(meta + 1, kSilErrClusters);
}
// One (tile, K-chunk) block of an image: img[((tile * nkc + kc) * kSilKC + k) * TILE + r] <- coordinate kc * kSilKC + k of
// the tile's row r, zero beyond dim and for a slot without a row.
//   MEMBERS: slot p of the image is sorted position p (a member where p < M); bcode[p] <- its code or kSilNone,
//            pos_of_row[row] <- p for every row, excluded ones too (their positions are >= M); tiles at or beyond M stay
//            unwritten (the sweep never reads them)
//   else:    slot r is the r-th row asked for (rows[r], or r itself); a_code[r] <- its code or kSilExcl, a_pos[r] <- its
//            sorted position; a row number >= n raises the validation word and leaves an empty, excluded slot
template <typename T, int TILE, bool MEMBERS>
__global__ __launch_bounds__(256) void sil_gather_kernel(const T *__restrict__ X, size_t n, size_t ld, int dim, int nkc,
                                                         const uint64_t *__restrict__ key, const uint64_t *__restrict__ rows,
                                                         size_t m, const int64_t *__restrict__ codes, uint64_t nc,
                                                         uint32_t *__restrict__ code_out, uint32_t *__restrict__ pos,
                                                         unsigned long long *__restrict__ meta, T *__restrict__ img) {
    constexpr int KPT = kSilKC * TILE / 256;  // coordinates per thread
    const int r = threadIdx.x % TILE, k0 = (threadIdx.x / TILE) * KPT;
    const size_t tile = blockIdx.x, slot = tile * TILE + (size_t)r;
    const int kc = blockIdx.y;
    const bool first = kc == 0 && k0 == 0;  // one thread per slot writes the slot's words
    size_t row = n;                          // (n: no row)
    if (MEMBERS) {
        const size_t M = (size_t)meta[0];
        if (slot < n) {
            const uint64_t k = key[slot];
            if (first) pos[(uint32_t)k] = (uint32_t)slot;
            if (slot < M) row = (size_t)(uint32_t)k;
            if (first && tile * TILE < M) code_out[slot] = slot < M ? (uint32_t)(k >> 32) : kSilNone;
        } else if (first && tile * TILE < M) {
            code_out[slot] = kSilNone;
        }
        if (tile * TILE >= M) return;
    } else {
        uint32_t code = kSilExcl, p = kSilNone;
        if (slot < m) {
            const uint64_t want = rows ? rows[slot] : (uint64_t)slot;
            if (want < (uint64_t)n) {
                row = (size_t)want;
                const int64_t c = codes[row];
                if (c >= 0 && (uint64_t)c < nc) code = (uint32_t)c;
                p = pos[row];
            } else if (first) {
                atomicOr(meta + 1, kSilErrRow);
            }
        }
        if (first) code_out[slot] = code, pos[n + slot] = p;  // (a_pos lies behind pos_of_row: see the carve)
    }
    T *dst = img + (((size_t)tile * nkc + kc) * kSilKC + k0) * TILE + r;
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const int k = kc * kSilKC + k0 + j;
        dst[(size_t)j * TILE] = (row < n && k < dim) ? X[row * ld + k] : (T)0;
    }
}

// what a (row, span) leaves for the finish, [span][m_pad] each
struct SilParts {
    double *head;         // P of the first cluster of the span
    double *tail;         // P of the last cluster of the span, where it is not the first
    double *own;          // S of the row's own cluster, where it lies strictly between the two (own_in)
    double *best;         // the smallest mean of the other clusters strictly between the two (+inf: none)
    uint32_t *best_code;  // its cluster
    uint32_t *own_in;
    size_t stride;        // m_pad
};

// ---- the sweep.  grid (tiles of scored rows, spans), 256 threads.  A workgroup owns TR = 16 * RM scored rows (128 for
// f32, 64 for f64) and walks its span one tile of 128 members at a time.
//
// The tile: thread (tr, tc) = (tid / 16, tid % 16) holds RM x 8 accumulators, rows tr * 4 + {0 .. 3} (f32: and 64 + the
// same), members tc * 4 + {0 .. 3} and 64 + the same.  Per coordinate it reads RM + 8 values of LDS for RM * 8 pairs --
// for f32 16 values per 64 pairs, half of what the 4 x 4 tile of the exact scan reads per pair -- as 16-byte reads: the
// staged chunk is [k][row], so a thread's four rows are contiguous; the 16 tc of a wave read 256 contiguous bytes, its 4
// tr four pieces 16 bytes apart, and lanes that share a tr (or a tc) read the same address: no bank conflict.
//
// Staging: the images are stored as the chunks are staged, so chunk kc + 1 of both operands is read from HBM in 16-byte
// pieces into registers while chunk kc is folded, then written to the other LDS buffer: one barrier per chunk.  The
// accumulators persist across the chunks; each pair's chain is the sequential fold in k (the zero padding beyond dim adds
// +0.0 to a sum that is >= +0.0 or NaN: the same bits).
//
// After the last chunk the tile's distances go to LDS transposed, Dt[member][row] (over the staging buffers), and thread
// r < TR walks row r's 128 distances in member order, adding each to the tile's f64 sum of the open cluster (Q above).  Where a cluster
// starts is a 128-bit mask of the tile, built from the members' codes once per tile and read as scalars: the walk has no
// per-member load but the distance.  When a cluster ends inside the span, its sum becomes the span's head (the first
// cluster, which may have begun in an earlier span), the row's own sum, or a candidate mean for b.
template <typename T, int RM>
__global__ __launch_bounds__(256) void sil_sweep_kernel(const T *__restrict__ Aimg, const T *__restrict__ Bimg, int nkc,
                                                        const uint32_t *__restrict__ bcode,
                                                        const uint32_t *__restrict__ a_code,
                                                        const uint32_t *__restrict__ a_pos,
                                                        const unsigned long long *__restrict__ meta, size_t span_len,
                                                        SilParts out) {
#pragma clang fp contract(off)
    constexpr int TR = 16 * RM, TC = kSilTC, KC = kSilKC;
    constexpr int DS = TR + 16 / (int)sizeof(T);                  // row stride of Dt: 16 bytes of padding
    constexpr int AV = KC * TR * (int)sizeof(T) / 16 / 256;        // 16-byte pieces per thread of a chunk of A
    constexpr int BV = KC * TC * (int)sizeof(T) / 16 / 256;        // ... of B
    extern __shared__ __attribute__((aligned(16))) unsigned char sil_smem[];
    __shared__ uint32_t scode[TC];
    __shared__ unsigned long long smask[2];
    T *As = reinterpret_cast<T *>(sil_smem);  // [2][KC][TR]
    T *Bs = As + 2 * KC * TR;                 // [2][KC][TC]
    T *Dt = reinterpret_cast<T *>(sil_smem);  // [TC][DS], once the chunks are folded

    const size_t M = (size_t)meta[0];
    const size_t p_begin = (size_t)blockIdx.y * span_len;
    if (p_begin >= M) return;  // (the finish reads the spans below M only)
    const size_t p_end = p_begin + span_len < M ? p_begin + span_len : M;
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const T *Arow = Aimg + (size_t)blockIdx.x * nkc * (KC * TR);

    // the walk's state of row tid (threads below TR)
    const size_t slot = (size_t)blockIdx.x * TR + (size_t)(tid < TR ? tid : 0);
    const uint32_t own = a_code[slot];
    const size_t self = (size_t)a_pos[slot];  // (kSilNone or a position >= M: meets no member)
    double cur = 0.0, head = 0.0, tail = 0.0, own_sum = 0.0, best = sil_inf();
    uint32_t best_code = kSilNone, own_in = 0, cur_code = kSilNone;
    size_t cur_start = p_begin;
    bool first = true;

    for (size_t t0 = p_begin; t0 < p_end; t0 += TC) {
        // the tile's codes and where its clusters start (consumed behind the barriers of the chunk loop)
        if (tid < TC) {
            const size_t p = t0 + (size_t)tid;
            const uint32_t c = bcode[p];  // (the image's tiles are whole: p < tiles * 128)
            scode[tid] = c;
            const bool start = p > p_begin && p < p_end && c != bcode[p - 1];
            const unsigned long long bal = __ballot(start);
            if ((tid & 63) == 0) smask[tid >> 6] = bal;
        }
        T acc[RM][8];
#pragma unroll
        for (int a = 0; a < RM; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[a][b] = (T)0;

        const T *Btile = Bimg + (t0 / TC) * (size_t)nkc * (KC * TC);
        sil_u4 ra[AV], rb[BV];
#pragma unroll
        for (int i = 0; i < AV; ++i) ra[i] = reinterpret_cast<const sil_u4 *>(Arow)[tid + 256 * i];
#pragma unroll
        for (int i = 0; i < BV; ++i) rb[i] = reinterpret_cast<const sil_u4 *>(Btile)[tid + 256 * i];
#pragma unroll
        for (int i = 0; i < AV; ++i) reinterpret_cast<sil_u4 *>(As)[tid + 256 * i] = ra[i];
#pragma unroll
        for (int i = 0; i < BV; ++i) reinterpret_cast<sil_u4 *>(Bs)[tid + 256 * i] = rb[i];
        __syncthreads();

        for (int kc = 0; kc < nkc; ++kc) {
            const bool more = kc + 1 < nkc;
            if (more) {
                const sil_u4 *an = reinterpret_cast<const sil_u4 *>(Arow + (size_t)(kc + 1) * (KC * TR));
                const sil_u4 *bn = reinterpret_cast<const sil_u4 *>(Btile + (size_t)(kc + 1) * (KC * TC));
#pragma unroll
                for (int i = 0; i < AV; ++i) ra[i] = an[tid + 256 * i];
#pragma unroll
                for (int i = 0; i < BV; ++i) rb[i] = bn[tid + 256 * i];
            }
            const T *Ac = As + (kc & 1) * (KC * TR) + tr * 4;
            const T *Bc = Bs + (kc & 1) * (KC * TC) + tc * 4;
#pragma unroll 4
            for (int k = 0; k < KC; ++k) {
                T av[RM], bv[8];
                {
                    T v[4];
                    sil_ld4(Ac + k * TR, v);
#pragma unroll
                    for (int j = 0; j < 4; ++j) av[j] = v[j];
                    if (RM == 8) {
                        sil_ld4(Ac + k * TR + 64, v);
#pragma unroll
                        for (int j = 0; j < 4; ++j) av[(RM == 8 ? 4 : 0) + j] = v[j];
                    }
                    sil_ld4(Bc + k * TC, v);
#pragma unroll
                    for (int j = 0; j < 4; ++j) bv[j] = v[j];
                    sil_ld4(Bc + k * TC + 64, v);
#pragma unroll
                    for (int j = 0; j < 4; ++j) bv[4 + j] = v[j];
                }
#pragma unroll
                for (int a = 0; a < RM; ++a)
#pragma unroll
                    for (int b = 0; b < 8; ++b) {
                        const T diff = av[a] - bv[b];
                        const T sq = diff * diff;
                        acc[a][b] = acc[a][b] + sq;
                    }
            }
            if (more) {
                sil_u4 *aw = reinterpret_cast<sil_u4 *>(As + ((kc + 1) & 1) * (KC * TR));
                sil_u4 *bw = reinterpret_cast<sil_u4 *>(Bs + ((kc + 1) & 1) * (KC * TC));
#pragma unroll
                for (int i = 0; i < AV; ++i) aw[tid + 256 * i] = ra[i];
#pragma unroll
                for (int i = 0; i < BV; ++i) bw[tid + 256 * i] = rb[i];
            }
            __syncthreads();  // the next chunk is staged, and this one fully read
        }

        // the distances, transposed into LDS over the staging buffers
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int col = (b < 4 ? 0 : 64) + tc * 4 + (b & 3);
#pragma unroll
            for (int g = 0; g < RM / 4; ++g) {
                T d[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] = sil_sqrt(acc[g * 4 + j][b]);
                sil_st4(Dt + col * DS + g * 64 + tr * 4, d);
            }
        }
        __syncthreads();

        // the walk: thread r folds row r's distances of the tile in member order
        if (tid < TR) {
            const int ncols = p_end - t0 < (size_t)TC ? (int)(p_end - t0) : TC;
            if (t0 == p_begin) cur_code = scode[0];
            double q = 0.0;  // the open cluster's sum over this tile
            for (int h = 0; h < 2; ++h) {
                const unsigned long long mk = smask[h];
                const unsigned mlo = __builtin_amdgcn_readfirstlane((unsigned)mk);
                const unsigned mhi = __builtin_amdgcn_readfirstlane((unsigned)(mk >> 32));
                const unsigned long long mask = ((unsigned long long)mhi << 32) | mlo;
                const int c_end = ncols < 64 * (h + 1) ? ncols : 64 * (h + 1);
                for (int c = 64 * h; c < c_end; ++c) {
                    const size_t p = t0 + (size_t)c;
                    if ((mask >> (c & 63)) & 1ull) {  // a cluster ends before member c (uniform over the workgroup)
                        cur = cur + q;
                        q = 0.0;
                        if (first) {
                            head = cur;
                            first = false;
                        } else if (cur_code == own) {
                            own_sum = cur;
                            own_in = 1;
                        } else {
                            const double mean = cur / (double)(p - cur_start);
                            if (mean < best) {
                                best = mean;
                                best_code = cur_code;
                            }
                        }
                        cur = 0.0;
                        cur_start = p;
                        cur_code = scode[c];
                    }
                    const double d = (double)Dt[c * DS + tid];
                    if (p != self) q = q + d;
                }
            }
            cur = cur + q;
        }
        __syncthreads();  // Dt, the codes and the mask are free again
    }
    if (tid < TR) {
        if (first)
            head = cur;
        else
            tail = cur;
        const size_t o = (size_t)blockIdx.y * out.stride + slot;
        out.head[o] = head;
        out.tail[o] = tail;
        out.own[o] = own_sum;
        out.best[o] = best;
        out.best_code[o] = best_code;
        out.own_in[o] = own_in;
    }
}

// the positions [lo, hi) of a code among the members' sorted codes
__device__ __forceinline__ size_t sil_bound(const uint32_t *__restrict__ bcode, size_t M, uint64_t code) {
    size_t lo = 0, hi = M;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)bcode[mid] < code)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
// ---- the finish: one thread per scored row folds its spans in order.  The first cluster of a span continues the last
// one of the span before where the codes agree (S = (P_s0 + P_s1) + ...); a cluster is closed -- compared as a mean, or
// kept as the row's own sum -- when another one follows it.  Clusters are met in ascending order and a mean wins by a
// strict '<': ties go to the lowest cluster.
__global__ __launch_bounds__(256) void sil_finish_kernel(const uint32_t *__restrict__ bcode,
                                                         const uint32_t *__restrict__ a_code,
                                                         const unsigned long long *__restrict__ meta, size_t m,
                                                         size_t span_len, SilParts in, double *__restrict__ s_out,
                                                         double *__restrict__ a_out, double *__restrict__ b_out,
                                                         int64_t *__restrict__ nearest_out) {
#pragma clang fp contract(off)
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    const uint32_t own = a_code[r];
    const size_t M = (size_t)meta[0];
    double a = sil_nan(), b = sil_nan(), s = sil_nan();
    int64_t nearest = -1;
    if (own != kSilExcl && M > 0) {
        double a_sum = 0.0, best = sil_inf(), open_sum = 0.0;
        uint32_t best_code = kSilNone, open_code = kSilNone;
        auto close = [&]() {
            if (open_code == own) {
                a_sum = open_sum;
            } else {
                const size_t cnt = sil_bound(bcode, M, (uint64_t)open_code + 1) - sil_bound(bcode, M, open_code);
                const double mean = open_sum / (double)cnt;
                if (mean < best) {
                    best = mean;
                    best_code = open_code;
                }
            }
        };
        size_t sp = 0;
        for (size_t p0 = 0; p0 < M; p0 += span_len, ++sp) {
            const size_t p1 = p0 + span_len < M ? p0 + span_len : M;
            const uint32_t fc = bcode[p0], lc = bcode[p1 - 1];
            const size_t o = sp * in.stride + r;
            if (sp > 0 && fc == open_code) {
                open_sum = open_sum + in.head[o];
            } else {
                if (sp > 0) close();
                open_code = fc;
                open_sum = in.head[o];
            }
            if (lc != fc) {
                close();
                if (in.own_in[o]) a_sum = in.own[o];
                const double bm = in.best[o];
                if (bm < best) {
                    best = bm;
                    best_code = in.best_code[o];
                }
                open_code = lc;
                open_sum = in.tail[o];
            }
        }
        close();
        const size_t na = sil_bound(bcode, M, (uint64_t)own + 1) - sil_bound(bcode, M, own);
        a = na > 1 ? a_sum / (double)(na - 1) : 0.0;
        b = best;
        nearest = best_code == kSilNone ? (int64_t)-1 : (int64_t)best_code;
        const double mx = a > b ? a : b;
        s = (na == 1 || mx == 0.0) ? 0.0 : (b - a) / mx;
    }
    s_out[r] = s;
    if (a_out) a_out[r] = a;
    if (b_out) b_out[r] = b;
    if (nearest_out) nearest_out[r] = nearest;
}
// ---- the mean and the validation word.  One workgroup: lane l folds the scored values among rows l, l + 256, ... of the
// rows asked for, in that order; the 256 partials are added by the halving tree (lane l += lane l + w, w = 128, 64, .. 1).
__global__ __launch_bounds__(256) void sil_score_kernel(const double *__restrict__ s, const uint32_t *__restrict__ a_code,
                                                        size_t m, const unsigned long long *__restrict__ meta,
                                                        double *__restrict__ score, uint64_t *__restrict__ n_scored,
                                                        int32_t *__restrict__ err) {
#pragma clang fp contract(off)
    __shared__ double sh[256];
    __shared__ unsigned long long shc[256];
    const int t = threadIdx.x;
    double sum = 0.0;
    unsigned long long cnt = 0;
    for (size_t r = (size_t)t; r < m; r += 256)
        if (a_code[r] != kSilExcl) {
            sum = sum + s[r];
            cnt += 1;
        }
    sh[t] = sum;
    shc[t] = cnt;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            sh[t] = sh[t] + sh[t + w];
            shc[t] += shc[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        if (score) *score = shc[0] ? sh[0] / (double)shc[0] : sil_nan();
        if (n_scored) *n_scored = (uint64_t)shc[0];
        if (err) *err = meta[1] ? PN_ERR_INVALID : PN_OK;
    }
}

size_t sil_up16(size_t b) { return round_up(b, (size_t)16); }
dim3 sil_grid(size_t items) { return dim3((unsigned)((items + 255) / 256)); }

// the carve of SilArgs::buf (every piece 16-byte aligned)
template <typename T, int TR>
struct SilCarve {
    size_t N, tiles_b, tiles_a, m_pad, nspans, span_len;
    int nkc;
    size_t o_key, o_pair, o_meta, o_pos, o_bcode, o_acode, o_bimg, o_aimg, o_parts, total;
    SilCarve(size_t n, size_t m, int dim) {
        N = sort_key_pair_len(n);
        tiles_b = (n + kSilTC - 1) / kSilTC;
        tiles_a = (m + TR - 1) / TR;
        m_pad = tiles_a * TR;
        span_len = sil_span_len(n);
        nspans = n ? (n + span_len - 1) / span_len : 1;
        nkc = (dim + kSilKC - 1) / kSilKC;
        if (nkc < 1) nkc = 1;
        size_t o = 0;
        o_key = o, o += sil_up16(N * 8);
        o_pair = o, o += sil_up16(N * 8);
        o_meta = o, o += 32;
        o_pos = o, o += sil_up16((n + m_pad) * 4);  // pos_of_row [n] | a_pos [m_pad]
        o_bcode = o, o += sil_up16(tiles_b * kSilTC * 4);
        o_acode = o, o += sil_up16(m_pad * 4);
        o_bimg = o, o += sil_up16(tiles_b * nkc * kSilKC * kSilTC * sizeof(T));
        o_aimg = o, o += sil_up16(tiles_a * nkc * kSilKC * TR * sizeof(T));
        o_parts = o, o += nspans * m_pad * 40;
        total = o;
    }
};
template <typename T> struct SilShape;
template <> struct SilShape<float> { static constexpr int RM = 8; };
template <> struct SilShape<double> { static constexpr int RM = 4; };

}  // namespace

size_t sil_span_len(size_t n) {
    const size_t per = round_up((n + kSilMaxSpans - 1) / kSilMaxSpans, (size_t)kSilTC);
    return per > kSilMinSpan ? per : kSilMinSpan;
}
size_t sil_buffer_bytes(size_t n, size_t m, int dim, int elem_bytes) {
    return elem_bytes == 4 ? SilCarve<float, 16 * SilShape<float>::RM>(n, m, dim).total
                           : SilCarve<double, 16 * SilShape<double>::RM>(n, m, dim).total;
}

template <typename T>
hipError_t sil_enqueue(const SilArgs &g, hipStream_t s) {
    constexpr int RM = SilShape<T>::RM, TR = 16 * RM;
    const size_t n = g.n, m = g.m;
    const SilCarve<T, TR> cv(n, m, g.dim);
    char *base = (char *)g.buf;
    uint64_t *key = (uint64_t *)(base + cv.o_key);
    unsigned long long *pair = (unsigned long long *)(base + cv.o_pair), *meta = (unsigned long long *)(base + cv.o_meta);
    uint32_t *pos = (uint32_t *)(base + cv.o_pos), *bcode = (uint32_t *)(base + cv.o_bcode);
    uint32_t *a_code = (uint32_t *)(base + cv.o_acode);
    T *bimg = (T *)(base + cv.o_bimg), *aimg = (T *)(base + cv.o_aimg);
    SilParts parts;
    const size_t cells = cv.nspans * cv.m_pad;
    parts.head = (double *)(base + cv.o_parts);
    parts.tail = parts.head + cells;
    parts.own = parts.tail + cells;
    parts.best = parts.own + cells;
    parts.best_code = (uint32_t *)(parts.best + cells);
    parts.own_in = parts.best_code + cells;
    parts.stride = cv.m_pad;
    const T *X = (const T *)g.X;
    const uint64_t nc = (uint64_t)g.n_clusters;

    hipError_t e = hipMemsetAsync(meta, 0, 32, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sil_keys_kernel, sil_grid(cv.N), dim3(256), 0, s, g.codes, n, cv.N, nc, key, pair, meta);
    e = launch_sort_key_pair_u64(key, pair, cv.N, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sil_meta_kernel, dim3(1), dim3(64), 0, s, key, n, meta);
    if (cv.tiles_b)
        hipLaunchKernelGGL((sil_gather_kernel<T, kSilTC, true>), dim3((unsigned)cv.tiles_b, (unsigned)cv.nkc), dim3(256), 0, s, X,
                           n, g.ld, g.dim, cv.nkc, key, (const uint64_t *)nullptr, (size_t)0, (const int64_t *)nullptr, nc,
                           bcode, pos, meta, bimg);
    if (cv.tiles_a) {
        hipLaunchKernelGGL((sil_gather_kernel<T, TR, false>), dim3((unsigned)cv.tiles_a, (unsigned)cv.nkc), dim3(256), 0, s, X, n,
                           g.ld, g.dim, cv.nkc, (const uint64_t *)nullptr, g.rows, m, g.codes, nc, a_code, pos, meta, aimg);
        // LDS: the two staging buffers of both operands, or the transposed tile of distances over them
        constexpr size_t stage = 2 * kSilKC * (TR + kSilTC) * sizeof(T);
        constexpr size_t dump = (size_t)kSilTC * (TR + 16 / sizeof(T)) * sizeof(T);
        constexpr size_t lds = stage > dump ? stage : dump;
        static LdsAttrOnce once;
        e = once.ensure((const void *)sil_sweep_kernel<T, RM>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((sil_sweep_kernel<T, RM>), dim3((unsigned)cv.tiles_a, (unsigned)cv.nspans), dim3(256), lds, s, aimg,
                           bimg, cv.nkc, bcode, a_code, pos + n, meta, cv.span_len, parts);
        hipLaunchKernelGGL(sil_finish_kernel, sil_grid(m), dim3(256), 0, s, bcode, a_code, meta, m, cv.span_len, parts, g.samples,
                           g.a, g.b, g.nearest);
    }
    hipLaunchKernelGGL(sil_score_kernel, dim3(1), dim3(256), 0, s, g.samples, a_code, m, meta, g.score, g.n_scored, g.err);
    return hipGetLastError();
}
template hipError_t sil_enqueue<float>(const SilArgs &, hipStream_t);
template hipError_t sil_enqueue<double>(const SilArgs &, hipStream_t);

}  // namespace pn
