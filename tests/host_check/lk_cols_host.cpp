// lk_cols_host.cpp -- TEST ONLY.  The vertical-pair samplers of vo_lkmath.h against the horizontal-pair ones and against the
// plain int64 formula, over the vectors of lk_cols_cases.h, as a g++ program (the host text of the wrappers).
//     lk_cols_host [out]     prints "OK <cases> <cases with iw11 < 0>", exit 0; a difference: the first case, exit 1
// out: the ColsOut records of the new composites, for tests/test_gpu_lk_cols.py to compare the device's with.
#include "lk_cols_cases.h"

#include <stdio.h>

int main(int argc, char **argv)
{
    int n_neg = 0;
    const std::vector<ColsCase> cases = cols_cases(&n_neg);
    std::vector<ColsOut> got(cases.size());
    for (size_t i = 0; i < cases.size(); i++) {
        ColsOut old, plain;
        cols_new(cases[i], got[i]);
        cols_old(cases[i], old);
        cols_plain(cases[i], plain);
        if (!cols_same(got[i], old) || !cols_same(got[i], plain)) {
            const ColsCase &c = cases[i];
            printf("case %zu differs (%s): w = %d %d %d %d, pix = %08x %08x %08x %08x\n", i, cols_same(got[i], old) ? "plain formula" : "horizontal pairs",
                   c.w[0], c.w[1], c.w[2], c.w[3], c.pix[0], c.pix[1], c.pix[2], c.pix[3]);
            return 1;
        }
    }
    if (argc > 1) {
        FILE *f = fopen(argv[1], "wb");
        if (!f || fwrite(got.data(), sizeof(ColsOut), got.size(), f) != got.size() || fclose(f) != 0)
            return 2;
    }
    if (n_neg == 0) {
        printf("the grid holds no weight pair with iw11 < 0\n");
        return 4;
    }
    printf("OK %zu %d\n", cases.size(), n_neg);
    return 0;
}
