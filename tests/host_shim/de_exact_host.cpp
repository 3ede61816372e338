// de_exact_host.cpp -- TEST INFRASTRUCTURE: nabo_amd/csrc/de_exact.h (the exact Mann-Whitney p of nabo_de_test) behind a C
// entry point, compiled with g++ on a box without a GPU.  tests/test_de_cpu.py compares it with Python integers.
#include <cstdarg>
#include <cstdio>

#include "../../nabo_amd/csrc/de_exact.h"

static thread_local char g_err[512] = "";

namespace nabo {
int api_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace nabo

extern "C" {
const char *nabo_last_error(void) { return g_err; }
int nabo_host_de_exact_pvalue(int64_t n1, int64_t n2, int64_t u2, double *p) { return nabo::de_exact_pvalue(n1, n2, u2, p); }
}
