// The scan-domain bounds of a range search (hr_search_dense_range*): plain C++, no HIP, so that a stand-alone host
// program can compile the very functions prep_queries_kernel calls (tests/test_range_host.py holds them, bit for bit, to
// the numpy restatement in tests/range_yardstick.py, which in turn is held against the exact values).
#pragma once
#include <math.h>

#include "../../include/hbmrag.h"

#if defined(__HIPCC__)
#define HR_HD __host__ __device__
#else
#define HR_HD
#endif

namespace hbmrag {

// The smallest float >= x / the largest float <= x.
HR_HD inline float f32_up(double x) {
    float f = (float)x;
    if ((double)f < x) {
        const unsigned u = __builtin_bit_cast(unsigned, f);
        f = f == 0.f ? __builtin_bit_cast(float, 1u) : __builtin_bit_cast(float, f > 0.f ? u + 1u : u - 1u);
    }
    return f;
}
HR_HD inline float f32_down(double x) { return -f32_up(-x); }

// qn2 = the canonical |q|^2, eps = eps(q), M = the largest row norm.  A zero query, and one whose 1 / |q| is not a normal
// fp32 number, gets no ceiling and no floor: the refine still decides every row.
HR_HD inline void range_scan_bounds(int metric, double qn2, double radius, double range_filter, double eps, double M,
                                         float* hi_a, float* lo_a) {
    const double INF = (double)__builtin_inff();
    *hi_a = __builtin_inff();
    *lo_a = -__builtin_inff();
    if (!(qn2 > 0.0)) return;
    const double nq = sqrt(qn2), c = 1.0 / nq;
    const float cf = (float)c;
    if (!(cf >= 0x1p-126f && cf < __builtin_inff()) || !(eps < 3.0e38)) return;
    double t_hi, t_lo;  // exact domain: t <= t_hi for a row that passes range_filter, t >= t_lo for one that passes radius
    if (metric == HR_METRIC_COSINE) {
        // |score32 - s64| <= 2^-24 |score32|, |score32| <= 1 + 2^-23; |s64 - t| <= 2^-40
        t_hi = range_filter + 0x1p-23;
        t_lo = radius - 0x1p-23;
    } else if (metric == HR_METRIC_IP) {
        // |score32 - S64| <= 2^-24 |score32| (2^-149 below the normal range), |S64 - S| <= 2^-40 |x| |q|, |x| <= M
        const double sl = 0x1p-23 * M * nq * 1.0001 + 0x1p-149;
        t_hi = (range_filter + sl) * c;
        t_lo = (radius - sl) * c;
    } else {
        // D32 = fl32(D64), D64 = D (1 +- 2^-40): a row with D32 >= range_filter has D >= d_lo, one with D32 < radius D <= d_hi
        double d_lo = range_filter * (1.0 - 0x1p-23) - 0x1p-149;
        const double d_hi = radius > 0.0 ? radius * (1.0 + 0x1p-23) + 0x1p-149 : 0.0;
        if (!(range_filter > 0.0)) {
            t_hi = INF;   // every distance passes
        } else {
            d_lo = d_lo > 0.0 ? d_lo : 0.0;
            t_hi = (qn2 - d_lo) * 0.5 * c;
            t_hi += 0x1p-39 * (qn2 + d_lo) * 0.5 * c;   // qn2 against the exact |q|^2, and this conversion's own rounding
        }
        t_lo = (qn2 - d_hi) * 0.5 * c;
        t_lo -= 0x1p-39 * (qn2 + d_hi) * 0.5 * c;
    }
    t_hi += fabs(t_hi) * 0x1p-40;
    t_lo -= fabs(t_lo) * 0x1p-40;
    const double e = eps * (1.0 + 0x1p-20);
    *hi_a = f32_up(t_hi + e);
    *lo_a = f32_down(t_lo - e);
}

}  // namespace hbmrag
