// Host build of leg-kilo_amd/csrc/lk_horn.h for tests/test_ate_host.py:
//   g++ -O2 -shared -fPIC -ffp-contract=off -o horn_host.so horn_host.cc                      (loaded with ctypes)
//   g++ -O1 -g -fsanitize=address,undefined -DLK_HORN_MAIN -o horn_host horn_host.cc          (a program of its own: prints "horn ok")
#include "../../leg-kilo_amd/csrc/lk_horn.h"
extern "C" void lk_horn_rotation_host_n(const double* S9, double* R9, int n) {
    for (int i = 0; i < n; ++i) lk_horn_rotation(S9 + 9 * i, R9 + 9 * i);
}
#ifdef LK_HORN_MAIN
#include <stdio.h>
static int check(const double* S, const char* name) {
    double R[9];
    lk_horn_rotation(S, R);
    double worst = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double d = (i == j) ? -1.0 : 0.0;
            for (int k = 0; k < 3; ++k) d += R[3 * k + i] * R[3 * k + j];
            worst = fabs(d) > worst ? fabs(d) : worst;
        }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (!(worst <= 1e-14) || !(fabs(det - 1.0) <= 1e-14)) {
        printf("%s: R^T R - I %.3e, det %.17g\n", name, worst, det);
        return 1;
    }
    return 0;
}
int main() {
    const double inf = 1.0 / 0.0, nan = inf - inf;
    const double full[9] = {3.0, 0.2, -0.1, 0.4, 2.0, 0.3, -0.2, 0.1, 1.0}, mirror[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0},
                 rank1[9] = {2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, rank2[9] = {1.0, 0.5, 0.0, -0.5, 1.0, 0.0, 0.0, 0.0, 0.0},
                 zero[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, tiny[9] = {1e-300, 0.0, 0.0, 0.0, 2e-300, 1e-301, 0.0, 0.0, 3e-300},
                 huge[9] = {1e300, 1e299, 0.0, 0.0, 2e300, 0.0, 1e298, 0.0, 3e300}, neg[9] = {-1.0, 0.0, 0.0, 0.0, -2.0, 0.0, 0.0, 0.0, -3.0},
                 bad0[9] = {nan, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, bad1[9] = {1.0, 0.0, 0.0, 0.0, inf, 0.0, 0.0, 0.0, 1.0};
    int rc = check(full, "full") + check(mirror, "mirror") + check(rank1, "rank1") + check(rank2, "rank2") + check(zero, "zero") + check(tiny, "tiny") +
             check(huge, "huge") + check(neg, "neg") + check(bad0, "nan") + check(bad1, "inf");
    if (rc == 0) printf("horn ok\n");
    return rc;
}
#endif
