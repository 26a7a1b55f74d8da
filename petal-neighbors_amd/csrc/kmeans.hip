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

namespace pn {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr double kKmG = 1.0 / 8192.0;                    // g = 2^-13
constexpr double kKmUp = 1.0 + 1.0 / 1099511627776.0;   // 1 + 2^-40: covers the f64 rounding of the norm sums
constexpr double kKmDown = 1.0 - 1.0 / 1099511627776.0;
constexpr double kKmNormMax = 1.2676506002282294e30;    // 2^100
constexpr int kKmLabelRows = 64, kKmLabelPitch = 65;

__device__ __forceinline__ void km_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

template <typename T>
__device__ __forceinline__ T km_sqrt(T x);
template <>
__device__ __forceinline__ float km_sqrt<float>(float x) { return sqrtf(x); }  // correctly rounded (build flags)
template <>
__device__ __forceinline__ double km_sqrt<double>(double x) { return sqrt(x); }

template <typename T>
__device__ __forceinline__ typename KeyOf<T>::type km_key(T d) {
    using K = typename KeyOf<T>::type;
    if constexpr (sizeof(T) == 4)
        return d != d ? KeyOf<T>::kNaN : (K)__float_as_uint(d);
    else
        return d != d ? KeyOf<T>::kNaN : (K)__double_as_longlong(d);
}

__device__ __forceinline__ uint16_t km_bf_rne(float x) {  // finite x
    const uint32_t u = __float_as_uint(x);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float km_f_down(double x) {  // largest float <= x (0 <= x < 2^127)
    float f = (float)x;
    if ((double)f > x) f = __uint_as_float(__float_as_uint(f) - 1u);
    return f;
}
__device__ __forceinline__ double km_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

// ---- packing: one wave per row of X [n][ld] (rows at and beyond n: zeros).  img / lo [n_img][dp] bf16 bits.
// ROWS: xn[r] <- |x|^2 rounded down (NaN: the row is flagged), xh[r] / xl[r] / xe[r] <- upper bounds of |x^| / |x~| / |e_x|.
// !ROWS (centres): cn[r] <- |c|^2 rounded down to f32 (+inf for the padding), cc[0..3] <- the maxima Ce, B, Ch, Cl (as the
// bits of non-negative doubles, by integer max), cc[4] <- nonzero when a centre is flagged.
template <typename T, bool ROWS>
__global__ __launch_bounds__(256) void km_pack_kernel(const T *__restrict__ X, size_t n, size_t n_img, size_t ld, int dim,
                                                      int dp, uint16_t *__restrict__ img, uint16_t *__restrict__ lo,
                                                      double *__restrict__ xn, float *__restrict__ xh,
                                                      float *__restrict__ xl, float *__restrict__ xe,
                                                      float *__restrict__ cn, unsigned long long *__restrict__ cc) {
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_img) return;  // (the whole wave)
    double s2 = 0.0, h2 = 0.0, l2 = 0.0, e2 = 0.0;
    bool bad = false;
    for (int k = lane; k < dp; k += 64) {
        uint16_t hb = 0, lb = 0;
        if (r < n && k < dim) {
            const double x = (double)X[r * ld + k];
            if (!(fabs(x) < 1.0e30)) {  // (NaN, inf, or beyond what a squared norm below 2^100 allows)
                bad = true;
            } else {
                const float xf = (float)x;
                hb = fabsf(xf) < 8.67361737988403547e-19f ? (uint16_t)0 : km_bf_rne(xf);  // 2^-60
                const double xhat = (double)__uint_as_float((uint32_t)hb << 16), r1 = x - xhat;
                const float rf = (float)r1;
                lb = fabsf(rf) < 8.67361737988403547e-19f ? (uint16_t)0 : km_bf_rne(rf);
                const double xlo = (double)__uint_as_float((uint32_t)lb << 16), e = r1 - xlo;
                s2 = s2 + x * x;
                h2 = h2 + xhat * xhat;
                l2 = l2 + xlo * xlo;
                e2 = e2 + e * e;
            }
        }
        img[r * (size_t)dp + k] = hb;
        lo[r * (size_t)dp + k] = lb;
    }
    bad = __any(bad);
    s2 = km_wave_sum(s2);
    h2 = km_wave_sum(h2);
    l2 = km_wave_sum(l2);
    e2 = km_wave_sum(e2);
    if (!(s2 < kKmNormMax)) bad = true;
    if (lane != 0) return;
    // (x - x^ in f64 may itself round, by at most 2^-53 |x|: the norm of e is widened by 2^-50 |x| for it)
    const double nx = sqrt(s2 * kKmUp) * kKmUp, nh = sqrt(h2 * kKmUp) * kKmUp, nl = sqrt(l2 * kKmUp) * kKmUp,
                 ne = sqrt(e2 * kKmUp) * kKmUp + nx * 8.881784197001252e-16;
    if (ROWS) {
        if (r < n) {
            xn[r] = bad ? __longlong_as_double(0x7FF8000000000000ll) : s2 * kKmDown;
            // (float upper bounds: the conversion rounds to nearest, one more factor covers it; + 1e-44: never below a
            // positive value that underflows)
            xh[r] = (float)(nh * (1.0 + 1.0 / 4194304.0));
            xl[r] = (float)(nl * (1.0 + 1.0 / 4194304.0) + 1e-40);
            xe[r] = (float)(ne * (1.0 + 1.0 / 4194304.0) + 1e-40);
        }
    } else {
        cn[r] = r < n && !bad ? km_f_down(s2 * kKmDown) : __uint_as_float(0x7F800000u);
        if (r < n) {
            if (bad) {
                atomicMax(&cc[4], 1ull);
            } else {
                atomicMax(&cc[0], (unsigned long long)__double_as_longlong(ne));
                atomicMax(&cc[1], (unsigned long long)__double_as_longlong(nx));
                atomicMax(&cc[2], (unsigned long long)__double_as_longlong(nh));
                atomicMax(&cc[3], (unsigned long long)__double_as_longlong(nl));
            }
        }
    }
}

// E(x) of the header, rounded upward
__device__ __forceinline__ double km_row_slack(double xh, double xl, double xe, const unsigned long long *__restrict__ cc) {
    const double Ce = __longlong_as_double((long long)cc[0]), B = __longlong_as_double((long long)cc[1]),
                 Ch = __longlong_as_double((long long)cc[2]), Cl = __longlong_as_double((long long)cc[3]);
    const double xs = xh + xl, prod = xs * Ch + xh * Cl;
    const double e = 2.0 * (xs * Ce + xe * B + xl * Cl + kKmG * prod) + 1.1920928955078125e-07 * (B * B + 2.001 * prod);
    return e * kKmUp + 1e-37;
}

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
    const int chunks = dp >> 3;                      // 16-byte chunks per row
    for (int q = t; q < kRows * chunks; q += 64 * WAVES) {
        const int rr = q / chunks, ch = q - rr * chunks;
        const size_t src = (row0 + (size_t)rr) * (size_t)dp + (size_t)ch * 8;
        *(u32x4 *)(tile + (size_t)rr * pitch + ch * 8) = *(const u32x4 *)(ximg + src);
        *(u32x4 *)(tile_lo + (size_t)rr * pitch + ch * 8) = *(const u32x4 *)(xlo + src);
    }
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
        const uint16_t *arow = cimg + aoff, *arow_lo = clo + aoff;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
        for (int ks = 0; ks < ksteps; ++ks) {
            const bf16x8 a = *(const bf16x8 *)(arow + ks * 16);
            const bf16x8 al = *(const bf16x8 *)(arow_lo + ks * 16);
            const bf16x8 b = *(const bf16x8 *)(brow + ks * 16);
            const bf16x8 bl = *(const bf16x8 *)(brow_lo + ks * 16);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            // registers 4 g .. 4 g + 3 are the centres ct + 8 g + 4 h + 0 .. 3 (the C layout of the instruction)
            const size_t cb = ct + (size_t)(8 * g + 4 * h);
            const float4 cn4 = *(const float4 *)(cn + cb);
            const float cnv[4] = {cn4.x, cn4.y, cn4.z, cn4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float key = cnv[j] - 2.0f * acc[4 * g + j];
                if (BOUNDS) {
                    if (my_row < n && cb + j < nc) {
                        // (pushed down by the roundings of its own evaluation, as the proof's tau' is)
                        const double lb = (xnr + (double)key) - slack;
                        bounds[my_row * nc + cb + j] = lb - (xnr + fabs((double)key) + slack) * 1.7763568394002505e-15;
                    }
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

// ---- staging of a wave's 64 rows, transposed, in LDS (ms_labels_kernel says why); sel: the listed rows
template <typename T>
__device__ __forceinline__ void km_stage_rows(const T *__restrict__ X, size_t ld, int dim, const uint32_t *__restrict__ sel,
                                              size_t first, int rows, int lane, T *__restrict__ tile) {
    for (int r = 0; r < rows; ++r) {
        const size_t i = sel ? (size_t)sel[first + r] : first + (size_t)r;
        for (int k = lane; k < dim; k += kKmLabelRows) tile[k * kKmLabelPitch + r] = X[i * ld + k];
    }
    __syncthreads();
}

// ---- the exact kernel: the fold of ms_labels_kernel with a distance output and an optional row list.  sel / nsel
// (nullable together): thread j of the launch answers row sel[j], j < *nsel (the grid is sized for n).
template <typename T, bool STAGED>
__global__ __launch_bounds__(kKmLabelRows) void km_exact_kernel(const T *__restrict__ X, size_t n, size_t ld, int dim,
                                                                const T *__restrict__ centres, size_t nc,
                                                                const uint32_t *__restrict__ sel,
                                                                const uint32_t *__restrict__ nsel,
                                                                int64_t *__restrict__ labels, T *__restrict__ dist) {
#pragma clang fp contract(off)
    using K = typename KeyOf<T>::type;
    extern __shared__ __align__(16) unsigned char km_smem[];
    T *tile = (T *)km_smem;
    const int lane = threadIdx.x;
    const size_t count = sel ? (size_t)*nsel : n;
    const size_t first = (size_t)blockIdx.x * kKmLabelRows, j = first + lane;
    if (first >= count) return;  // (the whole workgroup)
    if (STAGED) {
        const int rows = count - first < (size_t)kKmLabelRows ? (int)(count - first) : kKmLabelRows;
        km_stage_rows<T>(X, ld, dim, sel, first, rows, lane, tile);
    }
    if (j >= count) return;
    const size_t i = sel ? (size_t)sel[j] : j;
    const T *row = X + i * ld;
    K best = KeyOf<T>::kMax;
    int64_t lab = -1;
    T best_d = (T)0;
    for (size_t c = 0; c < nc; c += 4) {
        const T *cp[4];
        T sum[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            cp[u] = centres + (c + u < nc ? c + u : nc - 1) * (size_t)dim;  // (past the end: the last centre again, not used)
            sum[u] = (T)0;
        }
        for (int k = 0; k < dim; ++k) {
            const T x = STAGED ? tile[k * kKmLabelPitch + lane] : row[k];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const T diff = cp[u][k] - x;
                const T sq = diff * diff;
                sum[u] = sum[u] + sq;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const T d = km_sqrt<T>(sum[u]);
            const K key = km_key<T>(d);
            if (c + u < nc && key < best) {
                best = key;
                lab = (int64_t)(c + u);
                best_d = d;
            }
        }
    }
    labels[i] = lab;
    if (dist) dist[i] = best_d;
}

// the proof's right-hand side: everything at or below it may still round to d (key kk, finite) and tie (select.hip)
template <typename T> __device__ __forceinline__ double km_proof_rhs(typename KeyOf<T>::type kk);
template <> __device__ __forceinline__ double km_proof_rhs<float>(uint32_t kk) {
    const double dk = (double)__uint_as_float(kk), dn = (double)__uint_as_float(kk + 1);  // succ(d): the next float up
    const double mid = 0.5 * (dk + dn);
    return mid * mid * (1.0 + 4.5e-16);
}
template <> __device__ __forceinline__ double km_proof_rhs<double>(uint64_t kk) {
    const double dn = __longlong_as_double((long long)(kk + 1));
    return dn * dn * (1.0 + 4.440892098500626e-16);
}

// ---- re-rank and proof: one thread per row, the wave's rows staged as above.  The candidate's distance in the
// reference's fold; proven rows are answered here, the others are listed: slot = atomicAdd(nsel), sel[slot] = row.
template <typename T, bool STAGED>
__global__ __launch_bounds__(kKmLabelRows) void km_rerank_kernel(const T *__restrict__ X, size_t n, size_t ld, int dim,
                                                                 const T *__restrict__ centres, size_t nc,
                                                                 const uint32_t *__restrict__ cand,
                                                                 const float *__restrict__ tau,
                                                                 const double *__restrict__ xn,
                                                                 const float *__restrict__ xh,
                                                                 const float *__restrict__ xl,
                                                                 const float *__restrict__ xe,
                                                                 const unsigned long long *__restrict__ cc,
                                                                 uint32_t *__restrict__ sel, uint32_t *__restrict__ nsel,
                                                                 int64_t *__restrict__ labels, T *__restrict__ dist) {
#pragma clang fp contract(off)
    using K = typename KeyOf<T>::type;
    extern __shared__ __align__(16) unsigned char km_smem[];
    T *tile = (T *)km_smem;
    const int lane = threadIdx.x;
    const size_t first = (size_t)blockIdx.x * kKmLabelRows, i = first + lane;
    if (STAGED) {
        const int rows = n - first < (size_t)kKmLabelRows ? (int)(n - first) : kKmLabelRows;
        km_stage_rows<T>(X, ld, dim, nullptr, first, rows, lane, tile);
    }
    if (i >= n) return;
    const uint32_t c = cand[i];
    const double xnr = xn[i];
    bool ok = cc[4] == 0 && xnr == xnr && (size_t)c < nc;
    T d = (T)0;
    if (ok) {
        const T *cp = centres + (size_t)c * (size_t)dim;
        const T *row = X + i * ld;
        T sum = (T)0;
        for (int k = 0; k < dim; ++k) {
            const T x = STAGED ? tile[k * kKmLabelPitch + lane] : row[k];
            const T diff = cp[k] - x;
            const T sq = diff * diff;
            sum = sum + sq;
        }
        d = km_sqrt<T>(sum);
        const K kk = km_key<T>(d);
        constexpr K kInf = sizeof(T) == 4 ? (K)0x7F800000u : (K)0x7FF0000000000000ull;
        const float tv = tau[i];
        if (kk >= kInf || tv != tv) {
            ok = false;  // an infinite or NaN distance: the exact kernel orders it
        } else if (tv < __uint_as_float(0x7F800000u)) {
            const double slack = km_row_slack((double)xh[i], (double)xl[i], (double)xe[i], cc);
            // tau' = xn + tau - E, pushed down by the roundings of its own evaluation
            double lb = (xnr + (double)tv) - slack;
            lb = lb - (xnr + fabs((double)tv) + slack) * 1.7763568394002505e-15;  // 2^-49
            if constexpr (sizeof(T) == 4)
                lb = lb * (1.0 - (double)(dim + 4) * 5.9604644775390625e-08) - 1e-37;
            else
                lb = lb * (1.0 - (double)(dim + 4) * 1.1102230246251565e-16) * (1.0 - 8.881784197001252e-16) - 1e-300;
            ok = lb > km_proof_rhs<T>(kk);
        }  // (tau = +inf: no other centre exists)
    }
    if (ok) {
        labels[i] = (int64_t)c;
        if (dist) dist[i] = d;
    } else {
        const uint32_t slot = atomicAdd(nsel, 1u);
        sel[slot] = (uint32_t)i;  // (slot < n: every row is listed at most once)
    }
}

// nc == 0: every label -1, every distance NaN
template <typename T>
__global__ __launch_bounds__(256) void km_none_kernel(size_t n, int64_t *__restrict__ labels, T *__restrict__ dist) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    labels[i] = -1;
    if (dist) {
        if constexpr (sizeof(T) == 4)
            dist[i] = __uint_as_float(0x7FC00000u);
        else
            dist[i] = __longlong_as_double(0x7FF8000000000000ll);
    }
}

// ---- SUM4096 of the squared distances: one wave per segment of 4096 rows, then one thread over the segments
constexpr int kKmSeg = 4096;
template <typename T>
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
        const double t = labels[beg + j] < 0 ? 0.0 : d * d;
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
// One wave per (cluster, segment): workgroup b is segment b of the enumeration seg_off (the exclusive scan of nseg);
// the grid is sized for the most segments a call can have and the surplus exits.  Lane l strides the segment's members
// by 64 and reads COLS consecutive columns of each row; the 64 partials of a column are transposed through LDS and lane c
// folds column c's in lane order (ms_step_kernel).  segsum [segments][dim].
template <typename T, int COLS>
__global__ __launch_bounds__(64) void km_segment_sums_kernel(const uint64_t *__restrict__ key,
                                                             const uint64_t *__restrict__ off,
                                                             const uint64_t *__restrict__ seg_off, size_t nc,
                                                             const T *__restrict__ X, size_t ld, int dim,
                                                             double *__restrict__ segsum) {
#pragma clang fp contract(off)
    __shared__ double s_part[COLS][65];
    const int lane = threadIdx.x;
    const uint64_t b = blockIdx.x;
    if (b >= seg_off[nc]) return;
    // the cluster: the last c with seg_off[c] <= b (clusters without members have no segment and are skipped by the search)
    size_t lo = 0, hi = nc;
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (seg_off[mid] <= b)
            lo = mid;
        else
            hi = mid;
    }
    const size_t c = lo;
    const uint64_t s = b - seg_off[c];
    const uint64_t beg = off[c] + s * kKmSeg, rest = off[c + 1] - beg;
    const uint64_t len = rest < (uint64_t)kKmSeg ? rest : (uint64_t)kKmSeg;
    for (int c0 = 0; c0 < dim; c0 += COLS) {
        double P[COLS];
#pragma unroll
        for (int k = 0; k < COLS; ++k) P[k] = 0.0;
        for (uint64_t j = lane; j < len; j += 64) {
            // (c0 + COLS <= ld: the row's padding is read, and never used)
            const T *__restrict__ row = X + (size_t)(uint32_t)key[beg + j] * ld + c0;
            T v[COLS];
#pragma unroll
            for (int k = 0; k < COLS; ++k) v[k] = row[k];
#pragma unroll
            for (int k = 0; k < COLS; ++k) P[k] = P[k] + (double)v[k];
        }
#pragma unroll
        for (int k = 0; k < COLS; ++k) s_part[k][lane] = P[k];
        km_lds_fence();
        const int col = c0 + lane;
        if (lane < COLS && col < dim) {
            double S = s_part[lane][0];
#pragma unroll 9
            for (int l = 1; l < 64; ++l) S = S + s_part[lane][l];
            segsum[b * (uint64_t)dim + col] = S;
        }
        km_lds_fence();
    }
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

template <typename T>
hipError_t launch_km_pack_rows(const T *X, size_t n, size_t ld, int dim, const KmRowImage &r, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL((km_pack_kernel<T, true>), dim3((unsigned)((r.n_img + 3) / 4)), dim3(256), 0, s, X, n, r.n_img, ld,
                       dim, r.dp, r.img, r.lo, r.xn, r.xh, r.xl, r.xe, (float *)nullptr, (unsigned long long *)nullptr);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_km_pack_centres(const T *centres, size_t nc, int dim, const KmCentreImage &c, hipStream_t s) {
    const int dp = (dim + 15) / 16 * 16;
    hipError_t e = hipMemsetAsync(c.cc, 0, 8 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((km_pack_kernel<T, false>), dim3((unsigned)((c.nc_pad + 3) / 4)), dim3(256), 0, s, centres, nc,
                       c.nc_pad, (size_t)dim, dim, dp, c.img, c.lo, (double *)nullptr, (float *)nullptr, (float *)nullptr,
                       (float *)nullptr, c.cn, c.cc);
    return hipGetLastError();
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
hipError_t launch_km_filter(const KmRowImage &r, size_t n, const KmCentreImage &c, size_t nc, uint32_t *cand, float *tau,
                            hipStream_t s) {
    return km_filter_launch<false>(r, n, c, nc, cand, tau, nullptr, s);
}
hipError_t launch_km_bounds(const KmRowImage &r, size_t n, const KmCentreImage &c, size_t nc, double *bounds,
                            hipStream_t s) {
    return km_filter_launch<true>(r, n, c, nc, nullptr, nullptr, bounds, s);
}

template <typename T>
hipError_t launch_km_rerank(const T *X, size_t n, size_t ld, int dim, const T *centres, size_t nc, const uint32_t *cand,
                            const float *tau, const KmRowImage &r, const KmCentreImage &c, uint32_t *sel, uint32_t *nsel,
                            int64_t *labels, T *dist, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + kKmLabelRows - 1) / kKmLabelRows)), blk(kKmLabelRows);
    const size_t tile = (size_t)dim * kKmLabelPitch * sizeof(T);
    if (tile <= 64 * 1024)
        hipLaunchKernelGGL((km_rerank_kernel<T, true>), grid, blk, tile, s, X, n, ld, dim, centres, nc, cand, tau, r.xn, r.xh,
                           r.xl, r.xe, c.cc, sel, nsel, labels, dist);
    else
        hipLaunchKernelGGL((km_rerank_kernel<T, false>), grid, blk, 0, s, X, n, ld, dim, centres, nc, cand, tau, r.xn, r.xh,
                           r.xl, r.xe, c.cc, sel, nsel, labels, dist);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_km_exact(const T *X, size_t n, size_t ld, int dim, const T *centres, size_t nc, const uint32_t *sel,
                           const uint32_t *nsel, int64_t *labels, T *dist, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (nc == 0) {
        hipLaunchKernelGGL((km_none_kernel<T>), km_grid(n), dim3(256), 0, s, n, labels, dist);
        return hipGetLastError();
    }
    const dim3 grid((unsigned)((n + kKmLabelRows - 1) / kKmLabelRows)), blk(kKmLabelRows);
    const size_t tile = (size_t)dim * kKmLabelPitch * sizeof(T);
    if (tile <= 64 * 1024)
        hipLaunchKernelGGL((km_exact_kernel<T, true>), grid, blk, tile, s, X, n, ld, dim, centres, nc, sel, nsel, labels, dist);
    else  // (rows too long for LDS: read in place)
        hipLaunchKernelGGL((km_exact_kernel<T, false>), grid, blk, 0, s, X, n, ld, dim, centres, nc, sel, nsel, labels, dist);
    return hipGetLastError();
}

size_t km_inertia_bytes(size_t n) { return ((n + kKmSeg - 1) / kKmSeg + 1) * sizeof(double); }
template <typename T>
hipError_t launch_km_inertia(const int64_t *labels, const T *dist, size_t n, void *buf, double *out, hipStream_t s) {
    const size_t nseg = (n + kKmSeg - 1) / kKmSeg;
    double *seg = (double *)buf;
    if (nseg) hipLaunchKernelGGL((km_inertia_seg_kernel<T>), dim3((unsigned)nseg), dim3(64), 0, s, labels, dist, n, seg);
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
// labels [n] -> the members' lists, the counts (nullable) and, with centres != nullptr, one update of the centres in
// place; stop_out (device, 16 bytes): {shift2, the stop word}
template <typename T>
hipError_t km_update_enqueue(const T *X, size_t n, size_t ld, int dim, const int64_t *labels, size_t nc, void *buf,
                             T *centres, uint64_t *counts, double tol, int last, double **stop_out, hipStream_t s) {
    const size_t N = sort_key_pair_len(n);
    uint64_t *key = (uint64_t *)buf;
    unsigned long long *pair = (unsigned long long *)(key + N);
    uint64_t *off = (uint64_t *)(pair + N), *seg_off = off + nc + 1, *scan = seg_off + nc + 1;
    double *tc = (double *)(scan + nc / 4096 + 2), *stop = tc + nc, *segsum = stop + 2;
    uint32_t *nseg = (uint32_t *)(segsum + km_max_segments(n, nc) * (size_t)dim);
    if (stop_out) *stop_out = stop;
    hipLaunchKernelGGL(km_member_keys_kernel, km_grid(N), dim3(256), 0, s, labels, n, N, key, pair);
    hipError_t e = launch_sort_key_pair_u64(key, pair, N, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(km_offsets_kernel, km_grid(nc + 1), dim3(256), 0, s, key, N, nc, off);
    hipLaunchKernelGGL(km_counts_kernel, km_grid(nc), dim3(256), 0, s, off, nc, centres ? nseg : (uint32_t *)nullptr, counts);
    if (!centres) return hipGetLastError();
    e = launch_exclusive_scan_u32(nseg, nc, seg_off, scan, nullptr, s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)km_max_segments(n, nc));
    if (ld % 16 == 0)
        hipLaunchKernelGGL((km_segment_sums_kernel<T, 16>), grid, dim3(64), 0, s, key, off, seg_off, nc, X, ld, dim, segsum);
    else
        hipLaunchKernelGGL((km_segment_sums_kernel<T, 8>), grid, dim3(64), 0, s, key, off, seg_off, nc, X, ld, dim, segsum);
    hipLaunchKernelGGL((km_move_kernel<T>), dim3((unsigned)nc), dim3(64), 0, s, off, seg_off, segsum, dim, centres, tc);
    hipLaunchKernelGGL(km_stop_kernel, dim3(1), dim3(64), 0, s, tc, nc, tol, last, stop);
    return hipGetLastError();
}

#define PN_KM_INSTANTIATE(T)                                                                                                 \
    template hipError_t launch_km_pack_rows<T>(const T *, size_t, size_t, int, const KmRowImage &, hipStream_t);             \
    template hipError_t launch_km_pack_centres<T>(const T *, size_t, int, const KmCentreImage &, hipStream_t);               \
    template hipError_t launch_km_rerank<T>(const T *, size_t, size_t, int, const T *, size_t, const uint32_t *,             \
                                            const float *, const KmRowImage &, const KmCentreImage &, uint32_t *,            \
                                            uint32_t *, int64_t *, T *, hipStream_t);                                        \
    template hipError_t launch_km_exact<T>(const T *, size_t, size_t, int, const T *, size_t, const uint32_t *,              \
                                           const uint32_t *, int64_t *, T *, hipStream_t);                                   \
    template hipError_t launch_km_inertia<T>(const int64_t *, const T *, size_t, void *, double *, hipStream_t);             \
    template hipError_t km_update_enqueue<T>(const T *, size_t, size_t, int, const int64_t *, size_t, void *, T *,           \
                                             uint64_t *, double, int, double **, hipStream_t);
PN_KM_INSTANTIATE(float)
PN_KM_INSTANTIATE(double)
#undef PN_KM_INSTANTIATE

}  // namespace pn
