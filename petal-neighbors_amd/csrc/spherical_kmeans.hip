// spherical_kmeans.hip -- spherical k-means on Cosine indexes (pn_spherical_kmeans_*, pn_spherical_kmeans_assign_*): the
// assignment of every indexed row to the centre of the least Cosine::distance behind a bf16 MFMA filter, and the update of
// the centres as normalised sums of their members' directions in a fixed shape.  The contract is in the header
// (petal_mi355x.h) and DESIGN.md 4.28.
//
// Distance.  d(i, c) = the reference's Cosine::distance (src/distance.rs:86-107) in T: dot = the sequential unfused fold of
// x_k c_k, den = norm_c * norm_row (each norm the correctly rounded sqrt of its own sequential fold; the rows' come from the
// index, the centres' are folded once per assignment), d = 1 - dot / den.  Products and the denominator commute exactly:
// the value does not depend on the order of the arguments.  Keys are the signed order-preserving map of DESIGN.md 4.8.
//
// Bound.  Rows and centres are packed NORMALISED in f64 (km_pack.h, NORM): x- = x / |x|, c- = c / |c|, each split into two
// bf16 images.  kmeans.hip's bound over those vectors,
//   L(x, c) = xn(x) + fl32(cn(c) - 2 S(x, c)) - E(x) <= |x- - c-|^2,
// is a bound of 2 (1 - cos) = twice the real Cosine distance d*.  Every packed vector has norm 1 to rounding, so the maxima
// Ch, Cl, Ce, B over the centres that E(x) is made of are those of EVERY centre: E(x) is about 2^-12 for every row and no
// far-away or long centre inflates it, as one does in the Euclidean filter.  The filter keeps per row the centre of the
// smallest key and tau = the second smallest key: every other centre has |x- - c-|^2 >= tau' = xn + tau - E.  With
//   | |x- - c-|^2 - 2 d* | <= eps1 = (4.5 D + 45) 2^-53      (x-, c- are f64 roundings of the true directions)
//   | d_ref - d* |         <= E'   = (2 D + 16) u            (the reference's arithmetic; u = 2^-24 | 2^-53)
// (select.hip cos_proof_lb) every other centre's reference distance is at least (tau' - eps1) / 2 - E', and a
// row is PROVEN when that, pushed down by the roundings of its own evaluation, is strictly above the candidate's d: then
// no other centre ties or beats it.  A tie of two centres is never proven: the exact kernel alone decides (key, number).
// Rows that are not proven -- and every row of a call with a flagged centre -- are listed on the device and answered by
// the exact kernel.  Flagged: not finite, or a squared norm outside [2^-100, 2^100].
//
// Layout of the filter (the frame of foreign.hip).  A workgroup of WAVES waves holds 32 WAVES rows: their
// two images lie in LDS ([2][rows][dp + 8], 16 bytes of padding per row) and are the B operands of
// v_mfma_f32_32x32x16_bf16; a wave owns 32 rows, the ROW on the lane (lane & 31), 16 centres in the lane's accumulator.
// The centres stream past as the A operands in stages of 32 SUB centres (SUB = 4, 2, 1 by the row width): a stage is read
// from HBM / L2 once per WORKGROUP into registers while the previous stage is contracted, stored to the other of two LDS
// buffers and shared by the waves; cn travels with it in three small buffers, because the scan of a tile's accumulator
// runs one tile late -- the chain of tile t + 1 is issued before tile t is scanned, so the VALU works while the matrix
// core does.  One barrier per stage.  Three MFMAs per 16 columns on one chain: dp <= 304 keeps it at 57, inside the 65
// the allowance g is checked for (pn_bf16_selftest).  WAVES = 4 up to dp = 192 (153,984 bytes of LDS at most), 2 up to
// dp = 304 (160,128 bytes); wider rows take the exact kernel.
//
// This translation unit is compiled with -ffp-contract=off: every operation outside the MFMA is plain IEEE, unfused.
#include "../../include/petal_mi355x.h"
#include "pn_internal.h"
#include "km_filter.h"  // the chain, the row tile, the proof's tau', the kernels and launchers shared with kmeans.hip

namespace pn {

namespace {

constexpr int kSkmMaxDp = 304, kSkmWideDp = 192;  // four waves up to kSkmWideDp padded columns, two beyond
__host__ __device__ inline int skm_sub(int dp) { return dp <= 48 ? 4 : dp <= 96 ? 2 : 1; }  // 32-centre tiles per stage

// the order-preserving map of ALL floats (select.hip, sel_key_signed): -0 as +0, NaN above +inf
template <typename T> struct SkmKey;
template <> struct SkmKey<float> {
    static constexpr uint32_t kNaN = 0xFFC00000u, kInf = 0xFF800000u;
    static __device__ __forceinline__ uint32_t of(float d) {
        if (d != d) return kNaN;
        const uint32_t b = __float_as_uint(d == 0.0f ? 0.0f : d);
        return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
};
template <> struct SkmKey<double> {
    static constexpr uint64_t kNaN = 0xFFF8000000000000ull, kInf = 0xFFF0000000000000ull;
    static __device__ __forceinline__ uint64_t of(double d) {
        if (d != d) return kNaN;
        const uint64_t b = (uint64_t)__double_as_longlong(d == 0.0 ? 0.0 : d);
        return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
    }
};

// ---- the filter.  grid: the row tiles; PF = the 16-byte chunks a thread carries from HBM to LDS per stage, at most
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void skm_filter_kernel(const uint16_t *__restrict__ ximg,
                                                                const uint16_t *__restrict__ xlo, size_t n, int dp,
                                                                const uint16_t *__restrict__ cimg,
                                                                const uint16_t *__restrict__ clo,
                                                                const float *__restrict__ cn, size_t nc_pad,
                                                                uint32_t *__restrict__ cand, float *__restrict__ tau) {
    constexpr int kRows = 32 * WAVES, kThreads = 64 * WAVES, PF = WAVES == 4 ? 6 : 19;
    extern __shared__ __align__(16) unsigned char skm_smem[];
    const int pitch = dp + 8, chunks = dp >> 3, ksteps = dp >> 4, sub = WAVES == 4 ? skm_sub(dp) : 1, srows = 32 * sub;
    uint16_t *btile = (uint16_t *)skm_smem, *btile_lo = btile + (size_t)kRows * pitch;
    uint16_t *abuf = btile_lo + (size_t)kRows * pitch;     // [2 buffers][2 images][srows][pitch]
    float *meta = (float *)(abuf + (size_t)4 * srows * pitch);  // [3][srows]: the stage's cn
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 31, h = lane >> 5;
    const size_t row0 = (size_t)blockIdx.x * kRows;  // (the images have whole tiles of 128 rows: rows beyond n are zeros)
    const size_t n_stages = (nc_pad + (size_t)srows - 1) / (size_t)srows;

    km_load_row_tile<kThreads>(btile, btile_lo, ximg, xlo, row0, kRows, dp, t);

    // ---- the stream of the centres.  Stage s lies in data buffer s & 1 and meta buffer s % 3.
    const int per_img = srows * chunks, total = 2 * per_img;  // 16-byte chunks of a stage: total <= PF kThreads
    u32x4 pf[PF];
    float pm_cn = 0.0f;
    auto fetch = [&](size_t stage) {  // HBM / L2 -> registers
        const size_t c0 = stage * (size_t)srows;
#pragma unroll
        for (int e = 0; e < PF; ++e) {
            const int q = t + kThreads * e;
            pf[e] = u32x4{0u, 0u, 0u, 0u};
            if (q < total) {
                const int im = q >= per_img ? 1 : 0, rem = q - im * per_img, rr = rem / chunks, ch = rem - rr * chunks;
                if (c0 + (size_t)rr < nc_pad)  // (the last stage may reach beyond the padded centres: zeros, never scanned)
                    pf[e] = *(const u32x4 *)((im ? clo : cimg) + (c0 + (size_t)rr) * (size_t)dp + (size_t)ch * 8);
            }
        }
        if (t < srows) pm_cn = c0 + (size_t)t < nc_pad ? cn[c0 + (size_t)t] : __uint_as_float(0x7F800000u);
    };
    auto store = [&](size_t stage) {  // registers -> LDS
        uint16_t *dst = abuf + (size_t)(stage & 1) * 2 * srows * pitch;
#pragma unroll
        for (int e = 0; e < PF; ++e) {
            const int q = t + kThreads * e;
            if (q < total) {
                const int im = q >= per_img ? 1 : 0, rem = q - im * per_img, rr = rem / chunks, ch = rem - rr * chunks;
                *(u32x4 *)(dst + ((size_t)im * srows + rr) * pitch + ch * 8) = pf[e];
            }
        }
        if (t < srows) meta[(int)(stage % 3) * srows + t] = pm_cn;
    };
    const uint16_t *brow = btile + (size_t)(w * 32 + r) * pitch + h * 8;
    const uint16_t *brow_lo = btile_lo + (size_t)(w * 32 + r) * pitch + h * 8;
    auto chain = [&](size_t stage, int v) {
        const uint16_t *a0 = abuf + (size_t)(stage & 1) * 2 * srows * pitch + (size_t)(v * 32 + r) * pitch + h * 8;
        return km_mfma_chain(a0, a0 + (size_t)srows * pitch, brow, brow_lo, ksteps);
    };
    // (the padding's cn is +inf, so its keys never pass the strict '<')
    const float inf = __uint_as_float(0x7F800000u);
    float k1 = inf, k2 = inf;
    uint32_t c1 = 0xFFFFFFFFu;
    auto scan = [&](const f32x16 &acc, size_t stage, int v) {
        const float *m = meta + (int)(stage % 3) * srows + v * 32 + 4 * h;
        const uint32_t j0 = (uint32_t)(stage * (size_t)srows) + (uint32_t)(v * 32 + 4 * h);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 cn4 = *(const float4 *)(m + 8 * g);
            const float cnv[4] = {cn4.x, cn4.y, cn4.z, cn4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float key = cnv[j] - 2.0f * acc[4 * g + j];
                if (key < k2) {
                    if (key < k1) {
                        k2 = k1;
                        k1 = key;
                        c1 = j0 + (uint32_t)(8 * g + j);
                    } else {
                        k2 = key;
                    }
                }
            }
        }
    };

    if (n_stages) {
        fetch(0);
        store(0);
    }
    f32x16 acc_prev;
    size_t prev_stage = 0;
    int prev_v = -1;  // (-1: no tile waits for its scan)
    for (size_t s = 0; s < n_stages; ++s) {
        __syncthreads();  // stage s is in LDS (the first time: the rows too); the buffers of stage s + 1 are no longer read
        if (s + 1 < n_stages) fetch(s + 1);
        for (int v = 0; v < sub; ++v) {
            if (s * (size_t)srows + (size_t)(v * 32) >= nc_pad) break;  // (the whole workgroup: tiles beyond the centres)
            const f32x16 acc = chain(s, v);
            if (prev_v >= 0) scan(acc_prev, prev_stage, prev_v);
            acc_prev = acc;
            prev_stage = s;
            prev_v = v;
        }
        if (s + 1 < n_stages) store(s + 1);
    }
    if (prev_v >= 0) scan(acc_prev, prev_stage, prev_v);

    // ---- the other half of the row's centres: the lane 32 away
    const float p1 = __shfl_xor(k1, 32, 64), p2 = __shfl_xor(k2, 32, 64);
    const uint32_t pc = (uint32_t)__shfl_xor((int)c1, 32, 64);
    if (p1 < k2) {
        if (p1 < k1) {
            k2 = k1;
            k1 = p1;
            c1 = pc;
        } else {
            k2 = p1;
        }
    }
    if (p2 < k2) k2 = p2;  // (p2 >= p1 >= k1 by now: it can only be the runner-up)
    const size_t my_row = row0 + (size_t)(w * 32 + r);
    if (h == 0 && my_row < n) {
        cand[my_row] = c1;
        tau[my_row] = k2;
    }
}

// ---- the Cosine metric of km_filter.h's kernels: Cosine::distance as the header of this file states it -- the unfused
// fold of x_k c_k, 1 - dot / (norm_c * norm_row) -- on the signed keys; a row whose least key is the NaN key is a member of
// nothing (label -1, distance NaN).  A row without a finite runner-up is listed.  PROVEN: every other centre's reference
// distance is at least (tau' - eps1) / 2 - E' (cos_proof_lb's constants, select.hip), pushed down by the roundings of its
// own evaluation, and that is strictly above the candidate's d.
template <typename T>
struct KmMetric<T, true> {
    using K = typename KeyOf<T>::type;
    static constexpr K kNoKey = SkmKey<T>::kNaN;  // (only keys below the NaN key make a member)
    static __device__ __forceinline__ T no_dist() { return km_nan<T>(); }
    static __device__ __forceinline__ T term(T c, T x) { return c * x; }
    static __device__ __forceinline__ T row_norm(const KmNorms<T> &norms, size_t i) { return norms.rnorm[i]; }
    static __device__ __forceinline__ T finish(T dot, const KmNorms<T> &norms, size_t c, T rn) {
        const T den = norms.cnorm[(uint32_t)c] * rn;  // (nc < 2^31: a 32-bit index keeps the exact kernel's scalars in registers)
        return (T)1 - dot / den;
    }
    static __device__ __forceinline__ K key(T d) { return SkmKey<T>::of(d); }
    static __device__ __forceinline__ bool admits(const float *tau, size_t i) { return tau[i] < __uint_as_float(0x7F800000u); }
    template <typename TauFloor>
    static __device__ __forceinline__ bool proven(T d, float, int dim, TauFloor tau_floor) {
        if (key(d) >= SkmKey<T>::kInf) return false;  // an infinite or NaN distance: the exact kernel orders it
        const double u = sizeof(T) == 4 ? 5.9604644775390625e-08 : 1.1102230246251565e-16;
        double lb = tau_floor();
        const double eps1 = (4.5 * (double)dim + 45.0) * 1.1102230246251565e-16;
        const double e = (2.0 * (double)dim + 16.0) * u;
        lb = 0.5 * (lb - eps1) - e - (fabs(lb) + 1.0) * 1.0e-15;
        return lb > (double)d;
    }
    static void launch_move(const KmMembers &m, size_t nc, int dim, T *centres, hipStream_t s);
};

// One wave per centre: S_col = the segments in order; Q = the sum of S_col^2 in the 64-partial shape; the new centre
// (T)(S_col / sqrt(Q)); tc[c] <- the sum of the squared moves in the same shape.  A centre without members, or whose Q is
// 0 or not finite, is unchanged.
template <typename T>
__global__ __launch_bounds__(64) void skm_move_kernel(const uint64_t *__restrict__ off, const uint64_t *__restrict__ seg_off,
                                                      const double *__restrict__ segsum, int dim, T *__restrict__ centres,
                                                      double *__restrict__ tc) {
#pragma clang fp contract(off)
    __shared__ double s_t[64];
    const int lane = threadIdx.x;
    const size_t c = blockIdx.x;
    const uint64_t m = off[c + 1] - off[c];
    const uint64_t s0 = seg_off[c], s1 = seg_off[c + 1];
    auto column = [&](int col) {
        double S = segsum[s0 * (uint64_t)dim + col];
        for (uint64_t s = s0 + 1; s < s1; ++s) S = S + segsum[s * (uint64_t)dim + col];
        return S;
    };
    double q = 0.0;
    if (m)
        for (int col = lane; col < dim; col += 64) {
            const double S = column(col);
            const double sq = S * S;
            q = q + sq;
        }
    s_t[lane] = q;
    __syncthreads();
    double Q = s_t[0];
    for (int l = 1; l < 64; ++l) Q = Q + s_t[l];  // (every lane the same fold)
    __syncthreads();
    const bool move = m != 0 && Q > 0.0 && Q < __longlong_as_double(0x7FF0000000000000ll);
    const double rq = sqrt(Q);
    double part = 0.0;
    for (int col = lane; col < dim; col += 64) {
        const T old = centres[c * (size_t)dim + col];
        T nw = old;
        if (move) {
            nw = (T)(column(col) / rq);
            centres[c * (size_t)dim + col] = nw;
        }
        const double dd = (double)nw - (double)old;
        const double sq = dd * dd;
        part = part + sq;
    }
    s_t[lane] = part;
    __syncthreads();
    if (lane == 0) {
        double S = s_t[0];
        for (int l = 1; l < 64; ++l) S = S + s_t[l];
        tc[c] = S;
    }
}

}  // namespace

bool skm_filter_supported(int dim) { return dim >= 8 && (dim + 15) / 16 * 16 <= kSkmMaxDp; }

template <>
hipError_t launch_km_filter<true>(const KmRowImage &r, size_t n, const KmCentreImage &c, size_t nc, uint32_t *cand,
                                  float *tau, hipStream_t s) {
    if (n == 0 || nc == 0) return hipSuccess;
    if (r.dp > kSkmMaxDp) return hipErrorInvalidValue;
    static LdsAttrOnce once4, once2;
    const bool wide = r.dp > kSkmWideDp;
    const int rows = wide ? 64 : 128, srows = 32 * (wide ? 1 : skm_sub(r.dp));
    const size_t lds = ((size_t)2 * rows + (size_t)4 * srows) * (size_t)(r.dp + 8) * 2 + (size_t)3 * srows * 4;
    if (lds > 64 * 1024) {
        const hipError_t e = wide ? once2.ensure((const void *)skm_filter_kernel<2>, (size_t)256 * (kSkmMaxDp + 8) * 2 + 384)
                                  : once4.ensure((const void *)skm_filter_kernel<4>, (size_t)384 * (kSkmWideDp + 8) * 2 + 384);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)(r.n_img / rows));
    if (wide)
        hipLaunchKernelGGL((skm_filter_kernel<2>), grid, dim3(128), lds, s, r.img, r.lo, n, r.dp, c.img, c.lo, c.cn, c.nc_pad,
                           cand, tau);
    else
        hipLaunchKernelGGL((skm_filter_kernel<4>), grid, dim3(256), lds, s, r.img, r.lo, n, r.dp, c.img, c.lo, c.cn, c.nc_pad,
                           cand, tau);
    return hipGetLastError();
}

template <typename T>
void KmMetric<T, true>::launch_move(const KmMembers &m, size_t nc, int dim, T *centres, hipStream_t s) {
    hipLaunchKernelGGL((skm_move_kernel<T>), dim3((unsigned)nc), dim3(64), 0, s, m.off, m.seg_off, m.segsum, dim, centres, m.tc);
}

PN_KM_INSTANTIATE(float, true)
PN_KM_INSTANTIATE(double, true)
#undef PN_KM_INSTANTIATE

}  // namespace pn
