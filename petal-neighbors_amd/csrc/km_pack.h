// km_pack.h -- the two-image bf16 packing of rows behind the small MFMA filters: the k-means assignment (kmeans.hip,
// DESIGN.md 4.22) and the nearest-foreign-row tier (foreign.hip).  A row x (optionally translated by mu
// first) is split as x = x^ + x~ + e_x: x^ the bf16 rounding of x, x~ the bf16 rounding of what is left (each element
// below 2^-60 in magnitude rounds to 0), |e_x| about 2^-17 |x|; the kernel writes both images and, per row, bounds of the
// four norms the filters' slack E(x) is made of.  Everything here has internal linkage: each unit that includes the header
// compiles its own copy of the kernel.
#pragma once
#include "pn_internal.h"

namespace pn {

namespace {

constexpr double kKmG = 1.0 / 8192.0;                    // g = 2^-13
constexpr double kKmUp = 1.0 + 1.0 / 1099511627776.0;   // 1 + 2^-40: covers the f64 rounding of the norm sums
constexpr double kKmDown = 1.0 - 1.0 / 1099511627776.0;
constexpr double kKmNormMax = 1.2676506002282294e30;    // 2^100

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
// mu (nullable, [dim] f32): the row is x - mu, the difference taken in f64 (its rounding, at most 2^-53 |x - mu| per
// element, is inside the 2^-50 |x| by which the norm of e is widened below).
// ROWS: xn[r] <- |x|^2 rounded down (NaN: the row is flagged), xh[r] / xl[r] / xe[r] <- upper bounds of |x^| / |x~| / |e_x|.
// cn (nullable) [n_img]: |x|^2 rounded down to f32 (+inf for the padding and for flagged rows); cc (nullable): cc[0..3] <-
// the maxima Ce, B, Ch, Cl of |e|, |x|, |x^|, |x~| over the rows (as the bits of non-negative doubles, by integer max),
// cc[4] <- nonzero when a row is flagged.  The centres of k-means: !ROWS with cn and cc.
// NORM (spherical_kmeans.hip): the normalising front of Cosine indexes.  The row that is packed is
// x / |x| in f64 as cos_normalize_rows_kernel (bf16_filter.hip) forms it -- ss = the sum of the squares, every element
// times 1 / sqrt(ss) -- and a row whose ss is not inside [2^-100, 2^100] (zero, not finite) is flagged.  Every packed
// vector then has norm 1 to rounding.  Without NORM nothing of this is compiled: the other instantiations keep their bits.
template <typename T, bool ROWS, bool NORM = false>
__global__ __launch_bounds__(256) void km_pack_kernel(const T *__restrict__ X, size_t n, size_t n_img, size_t ld, int dim,
                                                      int dp, uint16_t *__restrict__ img, uint16_t *__restrict__ lo,
                                                      double *__restrict__ xn, float *__restrict__ xh,
                                                      float *__restrict__ xl, float *__restrict__ xe,
                                                      float *__restrict__ cn, unsigned long long *__restrict__ cc,
                                                      const float *__restrict__ mu) {
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_img) return;  // (the whole wave)
    double s2 = 0.0, h2 = 0.0, l2 = 0.0, e2 = 0.0;
    bool bad = false;
    double inv = 1.0;
    if constexpr (NORM) {
        double ss = 0.0;
        if (r < n)
            for (int k = lane; k < dim; k += 64) {
                const double v = (double)X[r * ld + k];
                ss = ss + v * v;
            }
        ss = km_wave_sum(ss);  // (the butterfly of commutative additions: the same bits on every lane)
        if (r < n && !(ss >= 7.888609052210118e-31 && ss <= 1.2676506002282294e30)) bad = true;  // 2^-100 .. 2^100, NaN
        inv = bad ? 0.0 : 1.0 / sqrt(ss);
    }
    for (int k = lane; k < dp; k += 64) {
        uint16_t hb = 0, lb = 0;
        if (r < n && k < dim && !(NORM && bad)) {
            double x = (double)X[r * ld + k];
            if (mu) x = x - (double)mu[k];
            if constexpr (NORM) x = x * inv;
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
    if (ROWS && r < n) {
        xn[r] = bad ? __longlong_as_double(0x7FF8000000000000ll) : s2 * kKmDown;
        // (float upper bounds: the conversion rounds to nearest, one more factor covers it; + 1e-44: never below a
        // positive value that underflows)
        xh[r] = (float)(nh * (1.0 + 1.0 / 4194304.0));
        xl[r] = (float)(nl * (1.0 + 1.0 / 4194304.0) + 1e-40);
        xe[r] = (float)(ne * (1.0 + 1.0 / 4194304.0) + 1e-40);
    }
    if (cn) cn[r] = r < n && !bad ? km_f_down(s2 * kKmDown) : __uint_as_float(0x7F800000u);
    if (cc && r < n) {
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

// E(x) of kmeans.hip's header, rounded upward
__device__ __forceinline__ double km_row_slack(double xh, double xl, double xe, const unsigned long long *__restrict__ cc) {
    const double Ce = __longlong_as_double((long long)cc[0]), B = __longlong_as_double((long long)cc[1]),
                 Ch = __longlong_as_double((long long)cc[2]), Cl = __longlong_as_double((long long)cc[3]);
    const double xs = xh + xl, prod = xs * Ch + xh * Cl;
    const double e = 2.0 * (xs * Ce + xe * B + xl * Cl + kKmG * prod) + 1.1920928955078125e-07 * (B * B + 2.001 * prod);
    return e * kKmUp + 1e-37;
}

}  // namespace

}  // namespace pn
