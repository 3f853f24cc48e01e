// Device p-value functions of the linear-model scans (k_lm.hip, k_lm2.hip): two-sided Student t through the regularised
// incomplete beta function and the chi-square(1) tail in its erfc form (src/stats/glm.rs:383-500).
#pragma once
#include <cmath>

#include "jx_common.h"

namespace jx {

// ---- p-values (glm.rs:383-500) ------------------------------------------------------------------------------------
__device__ inline double lm_betacf(double a, double b, double x) {
    const int maxit = 200;
    const double eps = 3.0e-14, fpmin = 1.0e-300;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0;
    double d = 1.0 - qab * x / qap;
    if (fabs(d) < fpmin) d = fpmin;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= maxit; ++m) {
        const double fm = (double)m, m2 = 2.0 * fm;
        double aa = fm * (b - fm) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < fpmin) d = fpmin;
        c = 1.0 + aa / c;
        if (fabs(c) < fpmin) c = fpmin;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + fm) * (qab + fm) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < fpmin) d = fpmin;
        c = 1.0 + aa / c;
        if (fabs(c) < fpmin) c = fpmin;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < eps) break;
    }
    return h;
}

__device__ inline double lm_betai(double a, double b, double x, double ln_beta) {
    if (!(x >= 0.0 && x <= 1.0)) return NAN;
    if (x == 0.0) return 0.0;
    if (x == 1.0) return 1.0;
    if (x < (a + 1.0) / (a + b + 2.0)) {
        const double front = exp(a * log(x) + b * log(1.0 - x) - ln_beta) / a;
        return front * lm_betacf(a, b, x);
    }
    const double front = exp(b * log(1.0 - x) + a * log(x) - ln_beta) / b;
    return 1.0 - front * lm_betacf(b, a, 1.0 - x);
}

constexpr double LM_MIN_POS = 2.2250738585072014e-308;

__device__ inline double lm_student_t_two_sided(double t, int df, double ln_beta) {
    if (df <= 0) return NAN;
    if (!isfinite(t)) return isnan(t) ? NAN : LM_MIN_POS;
    const double v = (double)df;
    double p = lm_betai(0.5 * v, 0.5, v / (v + t * t), ln_beta);
    if (!isfinite(p)) p = 1.0;
    return fmin(fmax(p, LM_MIN_POS), 1.0);
}

__device__ inline double lm_chi2_sf_df1(double stat) {
    if (!isfinite(stat) || stat < 0.0) return NAN;
    const double p = erfc(sqrt(0.5 * stat));
    if (!isfinite(p)) return 1.0;
    return fmin(fmax(p, LM_MIN_POS), 1.0);
}

}  // namespace jx
