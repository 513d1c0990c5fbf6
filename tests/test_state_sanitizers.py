"""The bounds promise of csrc/cbet_mesh_model.h for the state arm: mesh_state reads te, ti and zbar at
the indices mesh_locate produces, which lie inside the arrays whatever the coordinates and the node hold.  As
tests/test_mesh_sanitizers.py: a stand-alone C++ program runs mesh_locate and the state statements on meshes whose coordinate
arrays hold NaN, infinities, descending, constant and random values, te, ti and zbar heap blocks of exactly their size (ti and
zbar once present, once NULL), under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only; nothing is loaded into Python)."""
from helpers.twin_driver import run_driver

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>
#include "cbet_mesh_model.h"

#define REQUIRE(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s: ", #cond); std::fprintf(stderr, __VA_ARGS__); \
                                               std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

static double *block(size_t n) { double *p = (double *)std::malloc(n * sizeof(double)); REQUIRE(p, "malloc"); return p; }

int main()
{
    using namespace cbet;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> uni(-4.0, 4.0);
    const double specials[] = {nan, inf, -inf, 0.0, -0.0, 1e300, -1e300};
    long nodes = 0;
    // kind: how the coordinate arrays are filled -- 0 valid, 1 random (unsorted), 2 descending, 3 constant, 4 all NaN,
    // 5 random with specials sprinkled in
    for (int kind = 0; kind < 6; ++kind)
        for (int nr : {2, 3, 17})
            for (int nth : {1, 2, 9})
                for (int nph : {1, 2, 14}) {
                    double *coord[3] = {block(nr), block(nth), block(nph)};
                    const int n[3] = {nr, nth, nph};
                    const double lo[3] = {0.0, 0.0, -3.0}, hi[3] = {0.2, 3.14, 3.0};
                    for (int c = 0; c < 3; ++c)
                        for (int i = 0; i < n[c]; ++i) {
                            double v = lo[c] + (hi[c] - lo[c]) * (i + 0.5) / n[c];
                            if (kind == 1 || kind == 5) v = uni(rng);
                            if (kind == 2) v = hi[c] - (hi[c] - lo[c]) * (i + 0.5) / n[c];
                            if (kind == 3) v = 1.0;
                            if (kind == 4) v = nan;
                            if (kind == 5 && rng() % 3 == 0) v = specials[rng() % 7];
                            coord[c][i] = v;
                        }
                    const size_t cells = (size_t)nr * nth * nph;
                    double *f = block(cells), *ti = block(cells), *zb = block(cells);
                    for (size_t i = 0; i < cells; ++i) { f[i] = 100.0 + (double)(i % 7); ti[i] = 40.0 + (double)(i % 5); zb[i] = 1.0 + (double)(i % 3); }
                    MeshArgs a{};
                    a.nx = a.ny = a.nz = 7;
                    a.xmin = a.ymin = a.zmin = -0.13;
                    a.dx = a.dy = a.dz = 0.26 / 6;
                    a.dt = 1e-13; a.ncrit = 9e21;
                    a.nr = nr; a.nth = nth; a.nph = nph;
                    a.r = coord[0]; a.theta = coord[1]; a.phi = coord[2];
                    a.ne = a.te = f;
                    a.ti0 = 1000.0; a.z0 = 3.1;
                    a.sc.e2 = 2.3e-19; a.sc.a = 8.1e-18; a.sc.f = 8.4e-3; a.sc.mi_kg = 9.3e-27;
                    for (int centre = 0; centre < 4; ++centre) {
                        a.ox = centre == 1 ? a.xmin + 3 * a.dx : centre == 2 ? nan : centre == 3 ? inf : 0.01;   // 1: on a node's x
                        a.oy = centre == 1 ? a.ymin + 3 * a.dy : -0.02;
                        a.oz = centre == 1 ? a.zmin + 3 * a.dz : 0.005;
                        for (int i = 0; i < a.nx; ++i)
                            for (int j = 0; j < a.ny; ++j)
                                for (int k = 0; k < a.nz; ++k) {
                                    MeshNode m;
                                    mesh_locate(a, a.r, a.theta, a.phi, i, j, k, m);
                                    REQUIRE(m.m0 >= 0 && m.m0 < nr && (m.m1 == m.m0 || m.m1 == m.m0 + 1) && m.m1 < nr, "r bracket %d %d of %d", m.m0, m.m1, nr);
                                    REQUIRE(m.j0 >= 0 && m.j0 < nth && (m.j1 == m.j0 || m.j1 == m.j0 + 1) && m.j1 < nth, "theta bracket %d %d of %d", m.j0, m.j1, nth);
                                    REQUIRE(m.k0 >= 0 && m.k0 < nph && m.k1 >= 0 && m.k1 < nph && (m.k1 == m.k0 + 1 || m.k1 == 0), "phi bracket %d %d of %d", m.k0, m.k1, nph);
                                    REQUIRE(nth > 1 || m.j1 == m.j0, "ntheta == 1 reads one row");
                                    REQUIRE(nph > 1 || m.k1 == m.k0, "nphi == 1 reads one column");
                                    for (int present = 0; present < 2; ++present) {
                                        a.ti = present ? ti : nullptr;
                                        a.zbar = present ? zb : nullptr;
                                        double cs, gc;
                                        mesh_state(a, m, cs, gc);       // reads the field blocks: an index out of range is the sanitizer's
                                        if (kind == 0 && centre < 2) REQUIRE(std::isfinite(cs) && cs > 0.0 && std::isfinite(gc) && gc > 0.0, "valid mesh, node %d %d %d", i, j, k);
                                    }
                                    ++nodes;
                                }
                    }
                    std::free(f); std::free(ti); std::free(zb);
                    for (double *c : coord) std::free(c);
                }
    std::printf("state model ok: %ld nodes\n", nodes);
    return 0;
}
'''


def test_state_model_stays_in_bounds_under_asan_ubsan(tmp_path):
    out = run_driver(tmp_path, DRIVER, sources=())
    assert "state model ok" in out
