// kmeans.hip -- k-means on the device (pn_kmeans_*, pn_kmeans_assign_*): the assignment of every indexed row to its
// nearest centre behind a bf16 MFMA filter, and the update of the centres as means of a fixed shape.  The contract is in
// the header (petal_mi355x.h) and DESIGN.md 4.22.
//
// Assignment.  labels[i] = the centre nearest to row i by (distance key, centre number), the distance being the reference
// metric's sequential fold in T -- what ms_labels_kernel (mean_shift.hip) computes on the VALU against every centre.  Here
// the matrix cores look at every (row, centre) pair first:
//   x = x^ + x~ + e_x, c = c^ + c~ + e_c: x^ the bf16 rounding of x, x~ the bf16 rounding of what is left (each element
//       below 2^-60 in magnitude rounds to 0) -- two bf16 images per operand, |e| about 2^-17 |x|;
//   S(x,c) = the f32 MFMA accumulation of x^ . c^ + x^ . c~ + x~ . c^ (three MFMAs per step of 16 columns, one chain):
//       |S - those products| <= g (|x^| |c^| + |x^| |c~| + |x~| |c^|), g = 2^-13;
//   |x . c - S| <= (|x^| + |x~|) |e_c| + |e_x| |c| + |x~| |c~| + g ((|x^| + |x~|) |c^| + |x^| |c~|);
//   key(x,c) = fl32(cn(c) - 2 S), cn(c) <= |c|^2;  the subtraction's rounding is at most 2^-24 (|c|^2 + 2 |S|);
//   E(x) = 2 ((xh + xl) Ce + xe B + xl Cl + g ((xh + xl) Ch + xh Cl)) + 2^-23 (B^2 + 2.001 ((xh + xl) Ch + xh Cl)) + 1e-37
//          with xh, xl, xe >= |x^|, |x~|, |e_x| and the maxima over the centres Ch, Cl, Ce, B of |c^|, |c~|, |e_c|, |c|:
//          a constant of the ROW, so it does not disturb the ranking of the centres for one row;
//   L(x,c) = xn(x) + key(x,c) - E(x) <= |x - c|^2,  xn(x) <= |x|^2,
// for finite operands with squared norms below 2^100; anything else is flagged and answered by the exact kernel.  The
// filter keeps, per row, the centre of the smallest key (m = 1 candidate) and tau = the second smallest key: every other
// centre has L >= xn + tau - E.  The candidate is evaluated in the reference's fold and the row is PROVEN when
//   (xn + tau - E) (1 - (D + 4) u) - 1e-37 > ((d + succ d) / 2)^2      (u = 2^-24 | 2^-53)
// -- then no other centre's folded distance can tie or beat d.  Rows that are not proven are listed on the device and the
// exact kernel answers them.  m = 1: the re-rank costs one fold per row whatever nc is, a tie of two centres is always
// refused (so the (key, number) order is decided by the exact kernel alone), and the state the MFMA loop carries per
// lane is three registers.  One bf16 image per operand would do for the bound, but its slack, 2^-7 |x| |c|, is as large
// as the gaps between neighbouring centres of real problems; the split leaves the accumulation allowance, 2^-12 |x| |c|.
//
// Update.  A cluster's members in ascending row order come from one sort of the keys (label << 32 | row); one wave per
// (cluster, segment of 4096 members) sums the members' columns in f64 in the 64-lane shape of ms_step_kernel, and the
// fold kernel adds the segments in order, divides, moves the centre and sums the squared moves.
//
// This translation unit is compiled with -ffp-contract=off: every operation outside the MFMA is plain IEEE, unfused.
#include "../../include/petal_mi355x.h"
#include "pn_internal.h"
#include "km_filter.h"  // the packing and E(x), the MFMA chain, the proof, the kernels and launchers shared with the Cosine twin

namespace pn {

namespace {

// ---- the filter.  A workgroup of WAVES waves takes 32 WAVES rows, a wave 32 of them: the rows' two bf16 images lie in LDS
// ([2][rows][dp + 8], the 16 bytes of padding spread the rows over the banks) and are the B operands of
// v_mfma_f32_32x32x16_bf16, a tile of 32 centres read from the packed centres (L1 / L2) the A operands: the accumulator has
// the ROW on the lane (column lane & 31) and 16 centres in the registers, so the reduction over the centres is a scan of
// the lane's own registers, and the two lanes of a row (lane >> 5) merge once at the end.  K runs in steps of 16 columns
// over the whole padded row; dp <= kKmMaxDp = 320 keeps a chain at 60 MFMAs, inside the 65 the allowance g is checked for
// (DESIGN.md 4.11).  WAVES = 4 up to dp = 256 (135,168 bytes of LDS at most), 2 beyond (83,968 bytes).
// BOUNDS: the diagnostic of pn_kmeans_bounds_f32 -- L(x, c) for every pair instead of the reduction.
constexpr int kKmRowTile = 128, kKmCentreTile = 32, kKmMaxDp = 320, kKmWideDp = 256;
template <bool BOUNDS, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void km_assign_filter_kernel(const uint16_t *__restrict__ ximg,
                                                                      const uint16_t *__restrict__ xlo, size_t n, int dp,
                                                                      const uint16_t *__restrict__ cimg,
                                                                      const uint16_t *__restrict__ clo,
                                                                      const float *__restrict__ cn, size_t nc, size_t nc_pad,
                                                                      uint32_t *__restrict__ cand, float *__restrict__ tau,
                                                                      const double *__restrict__ xn,
                                                                      const float *__restrict__ xh,
                                                                      const float *__restrict__ xl,
                                                                      const float *__restrict__ xe,
                                                                      const unsigned long long *__restrict__ cc,
                                                                      double *__restrict__ bounds) {
    extern __shared__ __align__(16) unsigned char km_smem[];
    constexpr int kRows = 32 * WAVES;
    const int pitch = dp + 8;  // elements
    uint16_t *tile = (uint16_t *)km_smem, *tile_lo = tile + (size_t)kRows * pitch;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 31, h = lane >> 5;
    const size_t row0 = (size_t)blockIdx.x * kRows;  // (the images have whole tiles of 128 rows: rows beyond n are zeros)
    km_load_row_tile<64 * WAVES>(tile, tile_lo, ximg, xlo, row0, kRows, dp, t);
    __syncthreads();
    const uint16_t *brow = tile + (size_t)(w * 32 + r) * pitch + h * 8;
    const uint16_t *brow_lo = tile_lo + (size_t)(w * 32 + r) * pitch + h * 8;
    const int ksteps = dp >> 4;
    const float inf = __uint_as_float(0x7F800000u);
    float k1 = inf, k2 = inf;
    uint32_t c1 = 0xFFFFFFFFu;
    const size_t my_row = row0 + (size_t)(w * 32 + r);
    double xnr = 0.0, slack = 0.0;
    if (BOUNDS && my_row < n) {
        xnr = xn[my_row];
        slack = cc[4] ? __longlong_as_double(0x7FF8000000000000ll)  // (a centre is flagged: no bound is claimed)
                      : km_row_slack((double)xh[my_row], (double)xl[my_row], (double)xe[my_row], cc);
    }
    for (size_t ct = 0; ct < nc_pad; ct += kKmCentreTile) {
        const size_t aoff = (ct + (size_t)r) * (size_t)dp + h * 8;
        const f32x16 acc = km_mfma_chain(cimg + aoff, clo + aoff, brow, brow_lo, ksteps);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const size_t cb = ct + (size_t)(8 * g + 4 * h);
            const float4 cn4 = *(const float4 *)(cn + cb);
            const float cnv[4] = {cn4.x, cn4.y, cn4.z, cn4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float key = cnv[j] - 2.0f * acc[4 * g + j];
                if (BOUNDS) {
                    // (the proof's tau' with this pair's key in the place of tau)
                    if (my_row < n && cb + j < nc) bounds[my_row * nc + cb + j] = km_tau_floor(xnr, (double)key, slack);
                } else if (key < k2) {
                    if (key < k1) {
                        k2 = k1;
                        k1 = key;
                        c1 = (uint32_t)(cb + j);
                    } else {
                        k2 = key;
                    }
                }
            }
        }
    }
    if (BOUNDS) return;
    // the other half of the row's centres: the lane 32 away
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
    if (h == 0 && my_row < n) {
        cand[my_row] = c1;
        tau[my_row] = k2;
    }
}

// ---- the Euclidean metric of km_filter.h's kernels: the fold of ms_labels_kernel, (c - x)^2 summed in column order and
// the correctly rounded sqrt; keys are the bits of the distance.  A row is PROVEN by km_euclid_proven.  m = 1 candidate:
// a row without a second centre (tau = +inf) is proven by its candidate alone.
template <typename T>
struct KmMetric<T, false> {
    using K = typename KeyOf<T>::type;
    static constexpr K kNoKey = KeyOf<T>::kMax;
    static __device__ __forceinline__ T no_dist() { return (T)0; }
    static __device__ __forceinline__ T term(T c, T x) {
        const T diff = c - x;
        return diff * diff;
    }
    static __device__ __forceinline__ T row_norm(const KmNorms<T> &, size_t) { return (T)0; }
    static __device__ __forceinline__ T finish(T sum, const KmNorms<T> &, size_t, T) { return km_sqrt<T>(sum); }
    static __device__ __forceinline__ K key(T d) { return km_dist_key<T>(d); }
    static __device__ __forceinline__ bool admits(const float *, size_t) { return true; }
    template <typename TauFloor>
    static __device__ __forceinline__ bool proven(T d, float tau, int dim, TauFloor tau_floor) {
        return km_euclid_proven<T>(key(d), tau, dim, tau_floor);
    }
    // One wave per centre: the segments in order, the division, the move; tc[c] <- the sum of the squared moves
    static void launch_move(const KmMembers &m, size_t nc, int dim, T *centres, hipStream_t s);
};

// ---- SUM4096 of the squared distances: one wave per segment of 4096 rows, then one thread over the segments
// SQUARED: the term of a member is d * d (k-means); else d itself (spherical k-means)
template <typename T, bool SQUARED>
__global__ __launch_bounds__(64) void km_inertia_seg_kernel(const int64_t *__restrict__ labels, const T *__restrict__ dist,
                                                            size_t n, double *__restrict__ seg) {
#pragma clang fp contract(off)
    __shared__ double s_p[64];
    const int lane = threadIdx.x;
    const size_t beg = (size_t)blockIdx.x * kKmSeg;
    const size_t len = n - beg < (size_t)kKmSeg ? n - beg : (size_t)kKmSeg;
    double P = 0.0;
    for (size_t j = lane; j < len; j += 64) {
        const double d = (double)dist[beg + j];
        const double t = labels[beg + j] < 0 ? 0.0 : SQUARED ? d * d : d;
        P = P + t;
    }
    s_p[lane] = P;
    __syncthreads();
    if (lane == 0) {
        double S = s_p[0];
        for (int l = 1; l < 64; ++l) S = S + s_p[l];
        seg[blockIdx.x] = S;
    }
}
__global__ void km_fold_segments_kernel(const double *__restrict__ seg, size_t nseg, double *__restrict__ out) {
#pragma clang fp contract(off)
    if (threadIdx.x || blockIdx.x) return;
    double S = 0.0;
    if (nseg) {
        S = seg[0];
        for (size_t s = 1; s < nseg; ++s) S = S + seg[s];
    }
    *out = S;
}

// ---- the update
__global__ __launch_bounds__(256) void km_member_keys_kernel(const int64_t *__restrict__ labels, size_t n, size_t N,
                                                             uint64_t *__restrict__ key,
                                                             unsigned long long *__restrict__ pair) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    uint64_t k = ~0ull;
    if (i < n) k = ((uint64_t)(uint32_t)labels[i] << 32) | (uint64_t)i;  // (label -1: behind every cluster)
    key[i] = k;
    pair[i] = (unsigned long long)i;
}
// off[c] <- the first sorted position whose label is >= c (c <= nc); nseg[c] <- the cluster's segments of 4096 members
__global__ __launch_bounds__(256) void km_offsets_kernel(const uint64_t *__restrict__ key, size_t N, size_t nc,
                                                         uint64_t *__restrict__ off) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > nc) return;
    const uint64_t want = (uint64_t)c << 32;
    size_t lo = 0, hi = N;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (key[mid] < want)
            lo = mid + 1;
        else
            hi = mid;
    }
    off[c] = lo;
}
__global__ __launch_bounds__(256) void km_counts_kernel(const uint64_t *__restrict__ off, size_t nc,
                                                        uint32_t *__restrict__ nseg, uint64_t *__restrict__ counts) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const uint64_t m = off[c + 1] - off[c];
    if (nseg) nseg[c] = (uint32_t)((m + kKmSeg - 1) / kKmSeg);
    if (counts) counts[c] = m;
}
// One wave per centre: the segments in order, the division, the move; tc[c] <- the sum of the squared moves in the
// 64-partial shape (column col to partial col mod 64).  A centre without members is unchanged.
template <typename T>
__global__ __launch_bounds__(64) void km_move_kernel(const uint64_t *__restrict__ off, const uint64_t *__restrict__ seg_off,
                                                     const double *__restrict__ segsum, int dim, T *__restrict__ centres,
                                                     double *__restrict__ tc) {
#pragma clang fp contract(off)
    __shared__ double s_t[64];
    const int lane = threadIdx.x;
    const size_t c = blockIdx.x;
    const uint64_t m = off[c + 1] - off[c];
    const uint64_t s0 = seg_off[c], s1 = seg_off[c + 1];
    const double md = (double)m;
    double part = 0.0;
    for (int col = lane; col < dim; col += 64) {
        const T old = centres[c * (size_t)dim + col];
        T nw = old;
        if (m) {
            double S = segsum[s0 * (uint64_t)dim + col];
            for (uint64_t s = s0 + 1; s < s1; ++s) S = S + segsum[s * (uint64_t)dim + col];
            nw = (T)(S / md);
            centres[c * (size_t)dim + col] = nw;
        }
        const double dd = (double)nw - (double)old;
        part = part + dd * dd;
    }
    s_t[lane] = part;
    __syncthreads();
    if (lane == 0) {
        double S = s_t[0];
        for (int l = 1; l < 64; ++l) S = S + s_t[l];
        tc[c] = S;
    }
}
// shift2 = (((0.0 + t_0) + t_1) + ...) in centre order; out[0] <- shift2, the word at out[1] <- shift2 <= tol || last
__global__ __launch_bounds__(64) void km_stop_kernel(const double *__restrict__ tc, size_t nc, double tol, int last,
                                                     double *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_t[64];
    const int lane = threadIdx.x;
    double S = 0.0;
    for (size_t c0 = 0; c0 < nc; c0 += 64) {
        s_t[lane] = c0 + lane < nc ? tc[c0 + lane] : 0.0;
        __syncthreads();
        if (lane == 0) {
            const int lim = nc - c0 < 64 ? (int)(nc - c0) : 64;
            for (int l = 0; l < lim; ++l) S = S + s_t[l];
        }
        __syncthreads();
    }
    if (lane == 0) {
        out[0] = S;
        ((unsigned long long *)out)[1] = (S <= tol || last) ? 1ull : 0ull;
    }
}

inline dim3 km_grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

bool km_filter_supported(int dim) { return dim >= 8 && (dim + 15) / 16 * 16 <= kKmMaxDp; }
int km_row_tile() { return kKmRowTile; }
int km_centre_tile() { return kKmCentreTile; }

// rows: xn [n] (8 bytes), xh, xl, xe [n] (4 each), img and lo [round_up(n, 128)][dp] (2 each)
size_t km_row_image_bytes(size_t n, int dim) {
    const size_t dp = (size_t)(dim + 15) / 16 * 16;
    return round_up(n, (size_t)kKmRowTile) * dp * 4 + round_up(n, (size_t)4) * 20;
}
// centres: cc [8] (8 bytes), img and lo [round_up(nc, 32)][dp], cn [round_up(nc, 32)] (4)
size_t km_centre_image_bytes(size_t nc, int dim) {
    const size_t dp = (size_t)(dim + 15) / 16 * 16;
    return round_up(nc, (size_t)kKmCentreTile) * (dp * 4 + 4) + 64;
}

KmRowImage km_row_image_at(void *buf, size_t n, int dim) {
    const size_t dp = (size_t)(dim + 15) / 16 * 16, n_img = round_up(n, (size_t)kKmRowTile), n4 = round_up(n, (size_t)4);
    KmRowImage r;
    r.xn = (double *)buf;
    r.xh = (float *)(r.xn + n4);
    r.xl = r.xh + n4;
    r.xe = r.xl + n4;
    r.img = (uint16_t *)(r.xe + n4);  // (16-byte aligned: 20 n4 bytes in, n4 a multiple of 4, and buf is)
    r.lo = r.img + n_img * dp;
    r.n_img = n_img;
    r.dp = (int)dp;
    return r;
}
KmCentreImage km_centre_image_at(void *buf, size_t nc, int dim) {
    const size_t dp = (size_t)(dim + 15) / 16 * 16, nc_pad = round_up(nc, (size_t)kKmCentreTile);
    KmCentreImage c;
    c.cc = (unsigned long long *)buf;
    c.img = (uint16_t *)(c.cc + 8);
    c.lo = c.img + nc_pad * dp;
    c.cn = (float *)(c.lo + nc_pad * dp);
    c.nc_pad = nc_pad;
    return c;
}

// the two instantiations of a launch: four waves per workgroup up to dp = 256, two beyond
template <bool BOUNDS>
static hipError_t km_filter_launch(const KmRowImage &r, size_t n, const KmCentreImage &c, size_t nc, uint32_t *cand,
                                   float *tau, double *bounds, hipStream_t s) {
    if (n == 0 || nc == 0) return hipSuccess;
    static LdsAttrOnce once4, once2;
    const bool wide = r.dp > kKmWideDp;
    const int rows = wide ? 64 : 128;
    const size_t lds = 2 * (size_t)rows * (size_t)(r.dp + 8) * 2;
    if (lds > 64 * 1024) {
        const hipError_t e = wide ? once2.ensure((const void *)km_assign_filter_kernel<BOUNDS, 2>,
                                                 2 * (size_t)64 * (kKmMaxDp + 8) * 2)
                                  : once4.ensure((const void *)km_assign_filter_kernel<BOUNDS, 4>,
                                                 2 * (size_t)128 * (kKmWideDp + 8) * 2);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)(r.n_img / rows));
    if (wide)
        hipLaunchKernelGGL((km_assign_filter_kernel<BOUNDS, 2>), grid, dim3(128), lds, s, r.img, r.lo, n, r.dp, c.img, c.lo,
                           c.cn, nc, c.nc_pad, cand, tau, r.xn, r.xh, r.xl, r.xe, c.cc, bounds);
    else
        hipLaunchKernelGGL((km_assign_filter_kernel<BOUNDS, 4>), grid, dim3(256), lds, s, r.img, r.lo, n, r.dp, c.img, c.lo,
                           c.cn, nc, c.nc_pad, cand, tau, r.xn, r.xh, r.xl, r.xe, c.cc, bounds);
    return hipGetLastError();
}
template <>
hipError_t launch_km_filter<false>(const KmRowImage &r, size_t n, const KmCentreImage &c, size_t nc, uint32_t *cand,
                                   float *tau, hipStream_t s) {
    return km_filter_launch<false>(r, n, c, nc, cand, tau, nullptr, s);
}
hipError_t launch_km_bounds(const KmRowImage &r, size_t n, const KmCentreImage &c, size_t nc, double *bounds,
                            hipStream_t s) {
    return km_filter_launch<true>(r, n, c, nc, nullptr, nullptr, bounds, s);
}

size_t km_inertia_bytes(size_t n) { return ((n + kKmSeg - 1) / kKmSeg + 1) * sizeof(double); }
template <typename T>
hipError_t launch_km_inertia(const int64_t *labels, const T *dist, size_t n, void *buf, double *out, hipStream_t s,
                             bool squared) {
    const size_t nseg = (n + kKmSeg - 1) / kKmSeg;
    double *seg = (double *)buf;
    if (nseg && squared)
        hipLaunchKernelGGL((km_inertia_seg_kernel<T, true>), dim3((unsigned)nseg), dim3(64), 0, s, labels, dist, n, seg);
    else if (nseg)
        hipLaunchKernelGGL((km_inertia_seg_kernel<T, false>), dim3((unsigned)nseg), dim3(64), 0, s, labels, dist, n, seg);
    hipLaunchKernelGGL(km_fold_segments_kernel, dim3(1), dim3(64), 0, s, seg, nseg, out);
    return hipGetLastError();
}

// scratch of the update: key [N], pair [N] (N = sort_key_pair_len(n)), off [nc + 1], seg_off [nc + 1], scan scratch
// [nc / 4096 + 2], tc [nc], stop [2], segsum [n / 4096 + nc][dim] (64-bit words), nseg [nc] (32-bit)
size_t km_max_segments(size_t n, size_t nc) { return n / kKmSeg + nc; }
size_t km_update_bytes(size_t n, size_t nc, int dim) {
    return (2 * sort_key_pair_len(n) + 3 * nc + 2 + (nc / 4096 + 2) + 2 + km_max_segments(n, nc) * (size_t)dim) * 8 +
           round_up(nc, (size_t)2) * 4;
}
// the front half of an update, shared with spherical_kmeans.hip: the sort, the offsets, the counts and, with segments,
// the (cluster, segment) enumeration; m <- where the parts of buf are
hipError_t km_members_enqueue(const int64_t *labels, size_t n, size_t nc, int dim, void *buf, bool segments,
                              uint64_t *counts, KmMembers *m, hipStream_t s) {
    const size_t N = sort_key_pair_len(n);
    uint64_t *key = (uint64_t *)buf;
    unsigned long long *pair = (unsigned long long *)(key + N);
    uint64_t *off = (uint64_t *)(pair + N), *seg_off = off + nc + 1, *scan = seg_off + nc + 1;
    double *tc = (double *)(scan + nc / 4096 + 2), *stop = tc + nc, *segsum = stop + 2;
    uint32_t *nseg = (uint32_t *)(segsum + km_max_segments(n, nc) * (size_t)dim);
    *m = KmMembers{key, off, seg_off, tc, stop, segsum, km_max_segments(n, nc)};
    hipLaunchKernelGGL(km_member_keys_kernel, km_grid(N), dim3(256), 0, s, labels, n, N, key, pair);
    hipError_t e = launch_sort_key_pair_u64(key, pair, N, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(km_offsets_kernel, km_grid(nc + 1), dim3(256), 0, s, key, N, nc, off);
    hipLaunchKernelGGL(km_counts_kernel, km_grid(nc), dim3(256), 0, s, off, nc, segments ? nseg : (uint32_t *)nullptr, counts);
    if (!segments) return hipGetLastError();
    return launch_exclusive_scan_u32(nseg, nc, seg_off, scan, nullptr, s);
}
hipError_t launch_km_stop(const double *tc, size_t nc, double tol, int last, double *stop, hipStream_t s) {
    hipLaunchKernelGGL(km_stop_kernel, dim3(1), dim3(64), 0, s, tc, nc, tol, last, stop);
    return hipGetLastError();
}
template <typename T>
void KmMetric<T, false>::launch_move(const KmMembers &m, size_t nc, int dim, T *centres, hipStream_t s) {
    hipLaunchKernelGGL((km_move_kernel<T>), dim3((unsigned)nc), dim3(64), 0, s, m.off, m.seg_off, m.segsum, dim, centres, m.tc);
}

PN_KM_INSTANTIATE(float, false)
PN_KM_INSTANTIATE(double, false)
#undef PN_KM_INSTANTIATE
template hipError_t launch_km_inertia<float>(const int64_t *, const float *, size_t, void *, double *, hipStream_t, bool);
template hipError_t launch_km_inertia<double>(const int64_t *, const double *, size_t, void *, double *, hipStream_t, bool);

}  // namespace pn
