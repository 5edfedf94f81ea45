// Stand-alone check of the slope part of csrc/akb_figure.h (locate + gradient + deflect) over hostile
// coordinates, for a host sanitizer build:
//   g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I akbraytracing_amd/csrc tests/figure_slope_main.cpp -o figure_slope && ./figure_slope
// Every table is allocated at its exact size on the heap, so a load outside it is an error under
// AddressSanitizer (the gradient adds no load to the height's sixteen: the offsets are locate()'s);
// the program itself checks every offset, the outside reports, the +0 gradients of one-sample axes
// and outside hits, the untouched normal outside and the unit normal inside, and returns non-zero
// on the first violation.
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

static bool pos_zero(double x) { return x == 0.0 && !signbit(x); }

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
                    double tu, tw, v[16], hu, hw;
                    const bool outside = akb_fig::locate(M, x, y, 0.0, off, tu, tw);
                    for (int k = 0; k < 16; ++k) {
                        CHECK(off[k] >= 0 && off[k] < nw * nu);
                        v[k] = M.h[off[k] < 0 || off[k] >= nw * nu ? 0 : off[k]];
                    }
                    akb_fig::gradient(v, tu, tw, M, outside, hu, hw);
                    double nx = 0.0, ny = 0.0, nz = dn > 0.0 ? 1.0 : -1.0;  // the unit normal, either sign
                    const double n0[3] = {nx, ny, nz};
                    akb_fig::deflect(nx, ny, nz, dn, M, hu, hw, outside);
                    ++evals;
                    const double u = (x * 1.0 + y * 0.0) + 0.0 * 0.0, w = (x * 0.0 + y * 1.0) + 0.0 * 0.0;
                    const bool u_used = nu > 1, w_used = nw > 1;
                    const bool nan_in = (u_used && u != u) || (w_used && w != w);
                    const bool out_u = u_used && (u < M.u0 || u > M.u0 + M.du * (nu - 1));
                    const bool out_w = w_used && (w < M.w0 || w > M.w0 + M.dw * (nw - 1));
                    CHECK(outside == (out_u || out_w));
                    if (!u_used) CHECK(pos_zero(hu));
                    if (!w_used) CHECK(pos_zero(hw));
                    if (out_u || out_w) {
                        CHECK(pos_zero(hu) && pos_zero(hw));
                        CHECK(nx == n0[0] && ny == n0[1] && nz == n0[2]);  // N untouched
                    } else if (nan_in) {
                        CHECK(hu != hu || hw != hw);
                        CHECK(nx != nx && ny != ny && nz != nz);  // a NaN normal, and no outside report
                    } else {
                        CHECK(hu == hu && hw == hw && fabs(hu) < 1e-7 && fabs(hw) < 1e-7);
                        CHECK(fabs(((nx * nx + ny * ny) + nz * nz) - 1.0) < 1e-15);
                        // the beam-facing normal sigma N' tips against the gradient; N' stays on N's side
                        const double s = dn > 0.0 ? -1.0 : 1.0;
                        CHECK(s * nx * hu <= 0.0 && s * ny * hw <= 0.0 && nz * n0[2] > 0.0);
                    }
                }
    }
    printf("figure slope contract: %ld evaluations, %d failures\n", evals, fails);
    return fails ? 1 : 0;
}
