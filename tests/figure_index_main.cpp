// Stand-alone check of csrc/akb_figure.h's index contract (the case of test_figure_cpu.py's
// test_index_contract, for a host sanitizer build):
//   g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I akbraytracing_amd/csrc tests/figure_index_main.cpp -o figure_index && ./figure_index
// Every table is allocated at its exact size on the heap, so a load outside it is an error under
// AddressSanitizer; the program itself checks every reported offset, the outside reports and the
// zero / NaN values, and returns non-zero on the first violation.
#include <math.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "akb_figure.h"

static int fails = 0;
#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) {                                           \
            printf("FAILED line %d: %s\n", __LINE__, #c);     \
            ++fails;                                          \
        }                                                     \
    } while (0)

int main() {
    const double inf = std::numeric_limits<double>::infinity(), qnan = std::numeric_limits<double>::quiet_NaN();
    const int shapes[4][2] = {{4, 4}, {7, 5}, {1, 9}, {9, 1}};  // (nw, nu)
    long evals = 0;
    for (const auto& sh : shapes) {
        const int nw = sh[0], nu = sh[1];
        std::vector<double> tab((size_t)nw * nu);
        for (size_t k = 0; k < tab.size(); ++k) tab[k] = 1e-9 * (double)(k + 1);
        akb_fig::Map M;
        M.h = tab.data();
        const double o[3] = {0.0, 0.0, 0.0}, eu[3] = {1.0, 0.0, 0.0}, ew[3] = {0.0, 1.0, 0.0};
        for (int k = 0; k < 3; ++k) {
            M.o[k] = o[k];
            M.eu[k] = eu[k];
            M.ew[k] = ew[k];
        }
        M.u0 = -1.0;
        M.du = 0.5;
        M.w0 = 2.0;
        M.dw = 0.25;
        M.nu = nu;
        M.nw = nw;
        const double u_in = M.u0 + 0.5 * M.du * (nu - 1), w_in = M.w0 + 0.5 * M.dw * (nw - 1);
        const double us[] = {qnan, inf, -inf, 1e300, -1e300, M.u0 - M.du, M.u0 + M.du * nu, M.u0, M.u0 + M.du * (nu - 1), u_in};
        const double ws[] = {qnan, inf, -inf, 1e300, -1e300, M.w0 - M.dw, M.w0 + M.dw * nw, M.w0, M.w0 + M.dw * (nw - 1), w_in};
        for (double x : us)
            for (double y : ws) {
                int32_t off[16];
                bool outside = false;
                double h = 0.0;
                const double d = akb_fig::eval(M, x, y, 0.0, 0.25, &outside, &h, off);
                // the map coordinates are the frame's dot products: an infinite or NaN lab coordinate
                // reaches both (inf * 0 is NaN), so the expectation is formed from them
                const double u = (x * 1.0 + y * 0.0) + 0.0 * 0.0, w = (x * 0.0 + y * 1.0) + 0.0 * 0.0;
                ++evals;
                for (int k = 0; k < 16; ++k) CHECK(off[k] >= 0 && off[k] < nw * nu);
                const bool u_used = nu > 1, w_used = nw > 1;
                const bool nan_in = (u_used && u != u) || (w_used && w != w);
                const bool out_u = u_used && (u < M.u0 || u > M.u0 + M.du * (nu - 1));
                const bool out_w = w_used && (w < M.w0 || w > M.w0 + M.dw * (nw - 1));
                CHECK(outside == (out_u || out_w));
                if (out_u || out_w) {
                    CHECK(h == 0.0 && d == 0.0);  // zero, whatever the other axis holds
                } else if (nan_in) {
                    CHECK(h != h && d != d);  // NaN, and no outside report
                } else {
                    CHECK(h > 0.0 && d < 0.0);
                }
            }
    }
    printf("figure index contract: %ld evaluations, %d failures\n", evals, fails);
    return fails ? 1 : 0;
}
