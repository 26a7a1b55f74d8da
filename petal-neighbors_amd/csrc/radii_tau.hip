// radii_tau.hip -- one radius per query (pn_query_radii_*): the first tier's per-query thresholds, on the device.
//
// A scalar radius call routes on the host: radius_bf16_enqueue (index.hip) evaluates tau_r once, in f64, and the whole
// call leaves the filter when the radius cannot be served (not finite positive, Cosine r >= 1, tau_r >= 1e37).  With an
// array of radii in HBM both happen here, per query: the same three tau_r formulas, the same widening and key conversion
// as bf16_radius_tau_kernel (bf16_filter.hip), and a query whose radius the filter cannot serve gets the threshold -inf --
// no row passes it, so it appends nothing and overflows nothing -- and its w_qbad word, which takes it to the exact scan
// through the device-side list (radius_device.hip, rad_list_kernel).  One odd radius costs one query's exact scan.
//
// This unit is built with -ffp-contract=off (build.py): the host evaluates the formulas with one rounding per operation,
// and a constant array must give exactly the scalar call's thresholds.
#include "pn_internal.h"
#include "topk_buffer.h"

namespace pn {

// ut: the unit roundoff of T as a double; den = 1 - (D + 4) ut; c1 = (2 D + 16) ut, c2 = (4.5 D + 45) 2^-53 (Cosine)
template <typename T, bool COS>
__global__ __launch_bounds__(256) void bf16_radii_tau_kernel(const double *__restrict__ qn, const T *__restrict__ radii,
                                                             size_t nq, size_t nq_pad, double den, double c1, double c2,
                                                             uint32_t *__restrict__ out, uint32_t *__restrict__ qbad) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq_pad) return;
    const uint32_t none = f2s(__uint_as_float(0xFF800000u));  // -inf: nothing passes
    if (q >= nq) {
        out[q] = none;
        return;
    }
    const T rt = radii[q];
    const double r = (double)rt;
    bool ok = rt > (T)0 && rt < (T)INFINITY;
    if (COS) ok = ok && rt < (T)1;  // (r >= 1: half the sphere -- exact scan)
    double tr;
    if (COS)
        tr = 2.0 * (r + c1 + 1.0e-14) + c2;
    else if (sizeof(T) == 4)
        tr = (r * r + 1e-37) / den;
    else
        tr = (r * r * (1.0 + 8.881784197001252e-16) + 1e-300) / den;  // (f64: r^2 itself is rounded)
    ok = ok && tr < 1e37;
    if (!ok) {
        out[q] = none;
        qbad[q] = 1u;
        return;
    }
    // (from here: bf16_radius_tau_kernel; |t| 2^-18 is exact, so a fused and an unfused sum round alike)
    double t = tr - qn[q];
    t += fabs(t) * 3.814697265625e-06;
    float f = (float)t;
    if ((double)f < t) f = nextafterf(f, __uint_as_float(0x7F800000u));
    f = nextafterf(f, __uint_as_float(0x7F800000u));
    out[q] = f2s(f);
}

template <typename T>
hipError_t launch_bf16_radii_tau(const double *qn, const T *radii, size_t nq, size_t nq_pad, int dim, bool cosine,
                                 uint32_t *out, uint32_t *qbad, hipStream_t s) {
    const double ut = sizeof(T) == 4 ? 5.9604644775390625e-08 : 1.1102230246251565e-16;
    const double den = 1.0 - (double)(dim + 4) * ut;
    const double c1 = (2.0 * (double)dim + 16.0) * ut, c2 = (4.5 * (double)dim + 45.0) * 1.1102230246251565e-16;
    const dim3 grid((unsigned)((nq_pad + 255) / 256)), block(256);
    if (cosine)
        hipLaunchKernelGGL((bf16_radii_tau_kernel<T, true>), grid, block, 0, s, qn, radii, nq, nq_pad, den, c1, c2, out, qbad);
    else
        hipLaunchKernelGGL((bf16_radii_tau_kernel<T, false>), grid, block, 0, s, qn, radii, nq, nq_pad, den, c1, c2, out, qbad);
    return hipGetLastError();
}
template hipError_t launch_bf16_radii_tau<float>(const double *, const float *, size_t, size_t, int, bool, uint32_t *,
                                                 uint32_t *, hipStream_t);
template hipError_t launch_bf16_radii_tau<double>(const double *, const double *, size_t, size_t, int, bool, uint32_t *,
                                                  uint32_t *, hipStream_t);

__global__ void radii_add_listed_kernel(const uint32_t *__restrict__ nsel, unsigned long long *__restrict__ stats) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && *nsel) atomicAdd(stats, (unsigned long long)*nsel);
}
hipError_t launch_radii_add_listed(const uint32_t *nsel, unsigned long long *stats, hipStream_t s) {
    hipLaunchKernelGGL(radii_add_listed_kernel, dim3(1), dim3(64), 0, s, nsel, stats);
    return hipGetLastError();
}

}  // namespace pn
