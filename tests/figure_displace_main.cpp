// Stand-alone check of the displacement part of csrc/akb_figure.h (locate + combine + displace) over
// hostile coordinates, for a host sanitizer build:
//   g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I akbraytracing_amd/csrc tests/figure_displace_main.cpp -o figure_displace && ./figure_displace
// Every table is allocated at its exact size on the heap, so a load outside it is an error under
// AddressSanitizer (displace adds no load to the height's sixteen: the offsets are locate()'s); the
// program itself checks every offset, the outside reports, the untouched point and +0 height outside,
// the NaN point without a report for a NaN coordinate, the step's size and side inside, and returns
// non-zero on the first violation.
#include <math.h>
#include <stdio.h>
#include <string.h>

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

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

int main() {
    const double inf = std::numeric_limits<double>::infinity(), qnan = std::numeric_limits<double>::quiet_NaN();
    const int shapes[4][2] = {{4, 4}, {7, 5}, {1, 9}, {9, 1}};  // (nw, nu)
    long evals = 0;
    for (const auto& sh : shapes) {
        const int nw = sh[0], nu = sh[1];
        std::vector<double> tab((size_t)nw * nu);
        for (size_t k = 0; k < tab.size(); ++k) tab[k] = 1e-9 * (double)((k * 7) % 11 + 1);
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
            for (double y : ws)
                for (double dn : {-0.25, 0.25}) {
                    int32_t off[16];
                    double tu, tw, v[16];
                    const bool outside = akb_fig::locate(M, x, y, -0.0, off, tu, tw);
                    for (int k = 0; k < 16; ++k) {
                        CHECK(off[k] >= 0 && off[k] < nw * nu);
                        v[k] = M.h[off[k] < 0 || off[k] >= nw * nu ? 0 : off[k]];
                    }
                    const double h = akb_fig::combine(v, tu, tw, outside);
                    const double nz = dn > 0.0 ? 1.0 : -1.0;  // the unit normal (0, 0, nz), either sign
                    double px = x, py = y, pz = -0.0;
                    akb_fig::displace(px, py, pz, 0.0, 0.0, nz, dn, h, outside);
                    // the whole evaluation takes the same path
                    double qx = x, qy = y, qz = -0.0, qh;
                    const bool qo = akb_fig::eval_displace(M, qx, qy, qz, 0.0, 0.0, dn * nz, 0.0, 0.0, nz, qh);
                    CHECK(qo == outside && same_bits(qx, px) && same_bits(qy, py) && same_bits(qz, pz) && same_bits(qh, h));
                    ++evals;
                    const double u = (x * 1.0 + y * 0.0) + -0.0 * 0.0, w = (x * 0.0 + y * 1.0) + -0.0 * 0.0;
                    const bool u_used = nu > 1, w_used = nw > 1;
                    const bool nan_in = (u_used && u != u) || (w_used && w != w);
                    const bool out_u = u_used && (u < M.u0 || u > M.u0 + M.du * (nu - 1));
                    const bool out_w = w_used && (w < M.w0 || w > M.w0 + M.dw * (nw - 1));
                    CHECK(outside == (out_u || out_w));
                    if (out_u || out_w) {
                        CHECK(h == 0.0 && !signbit(h));
                        CHECK(same_bits(px, x) && same_bits(py, y) && same_bits(pz, -0.0));  // P untouched
                    } else if (nan_in) {
                        CHECK(h != h && pz != pz);  // a NaN height and point, and no outside report
                    } else {
                        CHECK(h == h && fabs(h) <= 13.75e-9);  // samples in [1, 11] nm, |weights| sum to at most 1.25
                        // towards the beam: sigma nz = -sign(dn) nz = -1 in both cases, the step is -h along z
                        CHECK(pz == -h);
                        if (x == x && fabs(x) <= 1e300) CHECK(same_bits(px, x + (dn > 0.0 ? -h : h) * 0.0));
                        if (y == y && fabs(y) <= 1e300) CHECK(same_bits(py, y + (dn > 0.0 ? -h : h) * 0.0));
                    }
                }
    }
    printf("figure displace contract: %ld evaluations, %d failures\n", evals, fails);
    return fails ? 1 : 0;
}
