// euler4_fma_probe.cpp - tests only: PDEHIP_E4_MINUS_TWICE (py-pde_amd/csrc/pdehip_euler4_plan.h), the fused form of x - 2 * c the four-step
// sweep computes with, against the two operations of the reference, bit for bit.  Built by g++ with -ffp-contract=off in
// tests/test_euler4_fma.py.  No HIP, no GPU.
#include <cstdint>
#include <cstring>

#include "../../py-pde_amd/csrc/pdehip_euler4_plan.h"

namespace {
uint64_t bits(double v)
{
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}
}

extern "C" {

// number of pairs whose fused result differs from x[i] - vm with vm = 2 * c[i] (two NaNs count as equal); *first: index of the first such pair
long e4fma_mismatches(const double *x, const double *c, long n, long *first)
{
    long bad = 0;
    for (long i = 0; i < n; i++) {
        volatile double vm = 2 * c[i];          // (volatile: the two operations stay two, whatever the flags)
        const double two = x[i] - vm;
        const double one = PDEHIP_E4_MINUS_TWICE(x[i], c[i]);
        if (bits(one) != bits(two) && !(one != one && two != two)) {
            if (!bad) *first = i;
            bad++;
        }
    }
    return bad;
}

}
