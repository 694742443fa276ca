// chisq_host.cpp — sts::chisq_upper_tail (csrc/arima_chisq.hpp) evaluated on the host: reads lines "L bits" (the
// degrees of freedom and the statistic as the 16 hex digits of its fp64 pattern) and prints the p-value's pattern.
// tests/test_diag_ref.py holds it to tests/diag_ref.py bit for bit: on the host both go through the same libm.
#include <cstdio>
#include <cstring>

#include "arima_chisq.hpp"

int main() {
    int L;
    unsigned long long bits;
    while (scanf("%d %llx", &L, &bits) == 2) {
        double stat, p;
        memcpy(&stat, &bits, sizeof stat);
        p = sts::chisq_upper_tail(L, stat);
        memcpy(&bits, &p, sizeof p);
        printf("%016llx\n", bits);
    }
    return 0;
}
