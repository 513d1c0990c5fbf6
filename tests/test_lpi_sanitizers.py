"""The bounds promises of csrc/cbet_lpi_model.h: a cell reads ne3d and te3d at its clamped node and, for
the gradient, at two nodes of each axis that the face rule keeps inside the table -- faces and a 2-node axis included --, reads
the fields of its own cell only, finds a cone bin inside [0, NB) for every direction (parallel, antiparallel, a zero gradient),
and writes its seven quantities inside the stack.  As tests/test_gain_model_sanitizers.py: a stand-alone C++ program walks
every haloed cell of a 5 x 4 x 3 grid and of a 5 x 2 x 3 one through the header with NB = 1, 8 and 16, every array a heap
block of exactly its size, under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only; nothing is loaded into Python)."""
from helpers.twin_driver import run_driver

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "cbet_lpi_model.h"

#define REQUIRE(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s: ", #cond); std::fprintf(stderr, __VA_ARGS__); \
                                               std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

using namespace cbet;

static bool same_bits(double x, double y) { return std::memcmp(&x, &y, sizeof x) == 0; }
static double *block(size_t n) { double *p = (double *)std::malloc(n * sizeof(double)); REQUIRE(p, "malloc"); return p; }

static const int NB = 5;       // beams: 0 along +z, 1 along -z, 2 absent (I = 0), 3 present in I but without a direction, 4 oblique
static double checksum = 0.0;
static long band_cells = 0, last_bin = 0, first_bin = 0;

static void walk(int NX, int NY, int NZ, int nbins, bool table_te, bool flat)
{
    const long NODES = (long)NX * NY * NZ, CELLS = (long)(NX + 2) * (NY + 2) * (NZ + 2), total = NB * CELLS;
    LpiArgs a{};
    a.nx = NX; a.ny = NY; a.nz = NZ; a.nbeams = NB;
    a.dx = 0.006; a.dy = 0.005; a.dz = 0.007;
    a.ncrit = 9.05e21; a.lambda_um = 0.351;
    a.frac_lo = 0.10; a.frac_hi = 0.30; a.te_ev = 1800.0;
    a.cone_bins = nbins; a.hx_lo = 0; a.hx_hi = NX + 2; a.hsize = CELLS;
    double *ne3d = block(NODES), *te3d = block(NODES), *fields = block(4 * total), *lpi = block(CBET_LPI_NQ * CELLS);
    for (long n = 0; n < NODES; ++n) {
        // in band but for two nodes; flat: one density everywhere, a zero gradient
        ne3d[n] = flat ? 0.2 * a.ncrit : a.ncrit * (0.12 + 0.15 * (double)((7 * n) % NODES) / NODES);
        te3d[n] = n % 5 == 0 ? 0.0 : 900.0 + 10.0 * n;
    }
    if (!flat) { ne3d[1] = 0.5 * a.ncrit; ne3d[NODES - 2] = 0.01 * a.ncrit; }
    for (long h = 0; h < CELLS; ++h) {
        const double kmag = 1.5e5, t = 0.3 + 0.01 * h;
        const double dir[NB][3] = {{0.0, 0.0, 1.0}, {0.0, 0.0, -1.0}, {0.6, 0.0, 0.8}, {0.0, 0.0, 0.0}, {std::cos(t) * 0.6, std::sin(t) * 0.6, 0.8}};
        const double inten[NB] = {1e14 * (1 + h % 4), 3e13 * (1 + h % 7), 0.0, 5e14, 2e14};
        for (int b = 0; b < NB; ++b) {
            fields[b * CELLS + h] = inten[b];
            for (int x = 0; x < 3; ++x) fields[(x + 1) * total + b * CELLS + h] = kmag * dir[b][x];
        }
    }
    a.fields = fields; a.ne3d = ne3d; a.te3d = table_te ? te3d : nullptr; a.lpi = lpi;
    cbet_lpi_summary s;
    lpi_summary_clear(s);
    for (long h = 0; h < CELLS; ++h) {
        int i, j, k;
        lpi_cell_node(a, h, i, j, k);
        REQUIRE(i >= 0 && i < NX && j >= 0 && j < NY && k >= 0 && k < NZ, "cell %ld -> node %d %d %d", h, i, j, k);
        const double ne = ne3d[((long)i * NY + j) * NZ + k];
        const bool band = lpi_in_band(a, ne / a.ncrit);
        LpiCell c = {0.0, 0.0, 0.0, 0};
        LpiPlasma q = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (band) {
            ++band_cells;
            q = lpi_plasma(a, i, j, k, ne);           // reads the tables: an index out of range is the sanitizer's
            if (NY < 3) REQUIRE(q.gy == 0.0, "cell %ld: a 2-node axis has gradient %g", h, q.gy);
            if (flat) REQUIRE(q.gn == 0.0 && q.Ln == 0.0 && q.T == 0.0, "cell %ld: flat density, gn %g Ln %g T %g", h, q.gn, q.Ln, q.T);
            else REQUIRE(q.Ln > 0.0 && q.T >= 0.0, "cell %ld: Ln %g T %g", h, q.Ln, q.T);
            double bins[CBET_LPI_MAX_BINS] = {};
            const double *fI = fields + h, *fx = fI + total, *fy = fx + total, *fz = fy + total;
            for (int b = 0; b < NB; ++b) {
                const long o = (long)b * CELLS;
                const double kn = lpi_knorm(fx[o], fy[o], fz[o]);
                REQUIRE(lpi_present(fI[o], kn) == (b != 2 && b != 3), "cell %ld beam %d: present %d", h, b, (int)lpi_present(fI[o], kn));
                if (!lpi_present(fI[o], kn)) continue;
                const int bin = lpi_bin(q, fx[o], fy[o], fz[o], kn, nbins);
                REQUIRE(bin >= 0 && bin < nbins, "cell %ld beam %d: bin %d of %d", h, b, bin, nbins);
                if (flat) REQUIRE(bin == 0, "cell %ld beam %d: bin %d without a gradient", h, b, bin);
                if (bin == nbins - 1) ++last_bin;
                if (bin == 0) ++first_bin;
                c.Isum = c.Isum + fI[o];
                if (fI[o] > c.Imax) c.Imax = fI[o];
                c.npresent += 1;
                bins[bin] = bins[bin] + fI[o];
            }
            for (int n = 0; n < nbins; ++n)
                if (bins[n] > c.Icw) c.Icw = bins[n];
            REQUIRE(c.npresent == 3 && c.Imax <= c.Icw && c.Icw <= c.Isum, "cell %ld: %d present, Imax %g Icw %g Isum %g", h, c.npresent, c.Imax, c.Icw, c.Isum);
            if (nbins == 1 || flat) REQUIRE(same_bits(c.Icw, c.Isum), "cell %ld: one bin, Icw %a Isum %a", h, c.Icw, c.Isum);
            lpi_summary_cell(s, h, c, q);
        }
        lpi_store(a, h, band, c, q);                  // writes the stack: likewise
        for (int n = 0; n < CBET_LPI_NQ; ++n) {
            if (!band) REQUIRE(lpi[n * CELLS + h] == 0.0, "cell %ld quantity %d: %g out of band", h, n, lpi[n * CELLS + h]);
            checksum += lpi[n * CELLS + h];
        }
    }
    cbet_lpi_summary m;
    lpi_summary_clear(m);
    lpi_summary_merge(m, s);
    lpi_summary_merge(m, s);
    REQUIRE(m.band_cells == 2 * s.band_cells && m.argmax_cw == s.argmax_cw && same_bits(m.max_eta_cw, s.max_eta_cw), "merge");
    REQUIRE(s.band_cells > 0 && s.argmax_cw >= 0 && s.argmax_cw < CELLS && s.max_present == 3, "summary: %lld band cells, argmax %lld", s.band_cells, s.argmax_cw);
    std::free(ne3d); std::free(te3d); std::free(fields); std::free(lpi);
}

int main()
{
    const int bins[3] = {1, 8, 16};
    for (int n = 0; n < 3; ++n)
        for (int te = 0; te < 2; ++te) {
            walk(5, 4, 3, bins[n], te != 0, false);
            walk(5, 2, 3, bins[n], te != 0, false);   // a 2-node axis: no gradient along it, no read beyond it
            walk(5, 4, 3, bins[n], te != 0, true);
        }
    // along the gradient: the first bin; against it: mu = -1, (1 - mu) NB / 2 = NB, the last bin; across it: the middle
    for (int n = 0; n < 3; ++n) {
        LpiPlasma q = {0.0, 0.0, -2.0e24, 2.0e24, 1.0, 1.0};
        REQUIRE(lpi_bin(q, 0.0, 0.0, -1.5e5, 1.5e5, bins[n]) == 0, "parallel, %d bins", bins[n]);
        REQUIRE(lpi_bin(q, 0.0, 0.0, 1.5e5, 1.5e5, bins[n]) == bins[n] - 1, "antiparallel, %d bins", bins[n]);
        REQUIRE(lpi_bin(q, 1.5e5, 0.0, 0.0, 1.5e5, bins[n]) == bins[n] / 2, "across, %d bins", bins[n]);
        REQUIRE(lpi_bin(q, 0.0, 0.0, -3.1e5, 1.5e5, bins[n]) == 0 && lpi_bin(q, 0.0, 0.0, 3.1e5, 1.5e5, bins[n]) == bins[n] - 1, "clamped, %d bins", bins[n]);
    }
    REQUIRE(band_cells > 0 && first_bin > 0, "%ld band cells, %ld first-bin beams", band_cells, first_bin);
    std::printf("lpi model ok: %ld band cells, %ld beams in the first bin, %ld in the last, checksum %.17g\n", band_cells, first_bin, last_bin, checksum);
    return 0;
}
'''


def test_lpi_model_stays_in_bounds_under_asan_ubsan(tmp_path):
    out = run_driver(tmp_path, DRIVER, sources=())
    assert "lpi model ok" in out and "checksum" in out
