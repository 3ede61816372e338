// de_exact.h -- the exact Mann-Whitney p of the differential-expression step (de_rank.hip), host code only: integers and
// one division, no device call.  Kept apart from de_rank.hip so that tests/host_shim compiles it with g++ and the CPU
// suite compares it with Python integers (tests/test_de_cpu.py).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/nabo_knn.h"

namespace nabo {

int api_fail(int code, const char *fmt, ...);      // api.hip (launch.h)

// 2 * P(U >= u_max) for samples of m and n values without ties, clipped to 1: the number of ways U takes the value k is
// the coefficient of q^k in the Gaussian binomial C(m + n, m)_q = prod_{i=1..m} (1 - q^(n+i)) / (1 - q^i).  Unsigned
// 128-bit arithmetic wraps, and a ring keeps the final coefficients exact as long as they are below 2^128 themselves:
// every one of them, and their partial sum cum, is at most total = C(m + n, m), which is below 2^127 or refused.
inline int de_exact_pvalue(int64_t n1, int64_t n2, int64_t u2, double *p)
{
    typedef unsigned __int128 u128;
    const int64_t m = n1 < n2 ? n1 : n2, n = n1 < n2 ? n2 : n1;      // the distribution is symmetric in (m, n)
    const u128 limit = ((u128)1 << 127) - 1;                         // the largest binomial that is accepted
    u128 total = 1;
    for (int64_t i = 1; i <= m; ++i) {
        // C(n + i, i) = C(n + i - 1, i - 1) * (n + i) / i.  With a / b = (n + i) / i in lowest terms, b divides the old
        // binomial, so (old / b) * a is the new one with no intermediate above it.  The binomials grow with i, so the
        // finished one reaches 2^127 exactly when one of these steps does.
        int64_t g = n + i, r = i;
        while (r) {
            const int64_t t = g % r;
            g = r, r = t;
        }
        const u128 a = (u128)((n + i) / g), q = total / (u128)(i / g);
        if (q > limit / a)
            return api_fail(NABO_E_UNSUPPORTED, "exact Mann-Whitney p for samples of %lld and %lld values without ties: "
                            "C(n1 + n2, n1) does not fit 127 bits", (long long)n1, (long long)n2);
        total = q * a;
    }
    const int64_t mn = m * n, um2 = u2 > 2 * mn - u2 ? u2 : 2 * mn - u2;
    const int64_t K = mn - um2 / 2;                                  // without ties U is an integer
    std::vector<u128> f((size_t)K + 1, 0);
    f[0] = 1;
    for (int64_t i = 1; i <= m; ++i) {
        for (int64_t k = K; k >= n + i; --k) f[k] -= f[k - n - i];
        for (int64_t k = i; k <= K; ++k) f[k] += f[k - i];
    }
    u128 cum = 0;
    for (int64_t k = 0; k <= K; ++k) cum += f[k];
    const double v = 2.0 * ((double)cum / (double)total);
    *p = v > 1.0 ? 1.0 : v;
    return NABO_OK;
}

}  // namespace nabo
