// What the kernels on tiles of a stationary ARD kernel share: the row-major lower-triangle tile order, and the prelude of the two fused
// products that never store the kernel matrix (kernels_kmm.hip, kernels_ksyrk.hip) -- the per-feature scales, the kernel's value from
// r^2, and the choice between the matrix-core form behind the far-point scan and the per-pair form alone.
#pragma once
#include "gpcore_internal.h"

// tile t of the row-major lower order: t = bi (bi + 1) / 2 + bj, bj <= bi
__device__ __forceinline__ void gp_tile_lower(int t, int &bi, int &bj) {
    int b = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (b * (b + 1) / 2 > t) --b;
    while ((b + 1) * (b + 2) / 2 <= t) ++b;
    bi = b;
    bj = t - b * (b + 1) / 2;
}

struct ArdScale {
    double scale[64];          // matrix-core form: 1 / l_k; per-pair form: 1 / l_k^2; zero beyond d
};

inline void ard_scales(const double *theta, int d, ArdScale *inv_ls, ArdScale *inv_ls2) {
    for (int k = 0; k < 64; ++k) inv_ls->scale[k] = inv_ls2->scale[k] = 0.0;
    for (int k = 0; k < d; ++k) {
        inv_ls->scale[k] = 1.0 / fabs(theta[1 + k]);
        inv_ls2->scale[k] = 1.0 / (theta[1 + k] * theta[1 + k]);
    }
}

// k / sf^2 from r^2
template <int NU2>
__device__ __forceinline__ double ard_value(double r2) {
    if constexpr (NU2 == 0) {
        return exp(-0.5 * r2);
    } else {
        double k0, h;
        matern_terms<NU2>(r2, k0, h);
        return k0;
    }
}

// The matrix-core form wants a centre, a finite non-zero amplitude and leading dimensions below 2^25 (ld_max: the largest of those the
// kernel indexes with), as the Gram builders' does.  Then the scan over Xa and Xb is enqueued with a fresh *epoch and far_flag comes
// back: both halves run behind the scan.  Else nullptr (*epoch = 0): the per-pair form alone.
inline int *ard_far_scan_or_pair(hipStream_t s, int nu2, const double *Xa, int na, int ldxa, const double *Xb, int nb, int ldxb, int d, const double *theta,
                                 const double *center, int ld_max, int *far_flag, int *epoch) {
    const double sf2 = theta[0] * theta[0];
    *epoch = 0;
    if (!(far_flag && center && std::isfinite(sf2) && sf2 != 0.0 && ld_max < (1 << 25))) return nullptr;
    *epoch = gpk_gram_epoch();
    gpk_ard_far_scan(s, nu2, Xa, na, ldxa, Xb, nb, ldxb, d, theta, center, 1, far_flag, *epoch);
    return far_flag;
}
