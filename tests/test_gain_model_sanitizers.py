"""The bounds and sign promises of csrc/cbet_gain_model.h: cell_state reads ne3d, the flow table and the
state table at the cell's clamped node, which lies inside the tables for every cell of the haloed grid, halo included; the
ordered pair gain is odd in the pair (g_ji == -g_ij bit for bit, clamped or not); at and above critical density the
prefactor, kap and the saturation limit are exactly 0.  As tests/test_state_sanitizers.py: a stand-alone C++ program walks
every haloed cell of a 5 x 4 x 3 grid for the four FLOW x STATE combinations, the tables heap blocks of exactly their size,
under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only; nothing is loaded into Python)."""
from helpers.twin_driver import run_driver

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "cbet_gain_model.h"
#include "cbet_node_model.h"

#define REQUIRE(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s: ", #cond); std::fprintf(stderr, __VA_ARGS__); \
                                               std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

using namespace cbet;

static bool same_bits(double x, double y) { return std::memcmp(&x, &y, sizeof x) == 0; }
static double *block(size_t n) { double *p = (double *)std::malloc(n * sizeof(double)); REQUIRE(p, "malloc"); return p; }

static const int NX = 5, NY = 4, NZ = 3, NB = 4;
static const long NODES = (long)NX * NY * NZ, CELLS = (long)(NX + 2) * (NY + 2) * (NZ + 2);
static const long CRITICAL = 17, ABOVE = 42;   // nodes (1, 1, 2) and (3, 2, 0)

static double checksum = 0.0;
static long pairs = 0, clamped = 0, dense_cells = 0;

// the four beams of cell h: 0 and 1 parallel (q = 0, different intensities), 2 absent (I = 0), 3 across them
static BeamAtCell beam(const double *fields, int b, long h)
{
    const long total = NB * CELLS;
    const double *fI = fields + h;
    return beam_at(fI, fI + total, fI + 2 * total, fI + 3 * total, b * CELLS);
}

template <bool FLOW, bool STATE>
static void walk(GainArgs a, const double *flow, const double *state, const double *fields)
{
    a.flow = FLOW ? flow : nullptr;
    a.state = STATE ? state : nullptr;
    const double iaw2 = a.iaw * a.iaw;
    for (long h = 0; h < CELLS; ++h) {
        int i, j, k;
        cell_node(a, h, i, j, k);
        REQUIRE(i >= 0 && i < NX && j >= 0 && j < NY && k >= 0 && k < NZ, "cell %ld -> node %d %d %d", h, i, j, k);
        const long node = ((long)i * NY + j) * NZ + k;
        const CellState c = cell_state<FLOW, STATE>(a, h);      // reads the tables: an index out of range is the sanitizer's
        const CellState r = cell_state(a, h);                   // the run-time choice is the same function
        REQUIRE(std::memcmp(&c, &r, sizeof c) == 0, "cell %ld: cell_state(a, h) != cell_state<%d, %d>(a, h)", h, FLOW, STATE);
        const double pref = cell_pref(a, c), kap = cell_kap(a, c), lim = cell_sat_limit(a, c);
        if (node == CRITICAL || node == ABOVE) {
            ++dense_cells;
            REQUIRE(!(c.eps > 0.0) && c.rt == 0.0, "node %ld is not sub-critical: eps %g rt %g", node, c.eps, c.rt);
            REQUIRE(pref == 0.0 && kap == 0.0 && lim == 0.0, "node %ld: pref %g kap %g lim %g", node, pref, kap, lim);
        } else {
            REQUIRE(c.eps > 0.0 && pref > 0.0 && kap > 0.0 && lim > 0.0, "node %ld: eps %g pref %g kap %g lim %g", node, c.eps, pref, kap, lim);
        }
        checksum += c.frac + c.rt + c.ux + c.uy + c.uz + c.cs + c.gc + pref + kap + lim;
        // the limit of this cell's clamp: between the swings of its two exchanging pairs, (0, 3) and (1, 3)
        const BeamAtCell B0 = beam(fields, 0, h), B1 = beam(fields, 1, h), B3 = beam(fields, 3, h);
        const double w0 = pair_swing(pair_gain(c, pref, iaw2, pair_wave(B0, B3)), B0.I, B3.I);
        const double w1 = pair_swing(pair_gain(c, pref, iaw2, pair_wave(B1, B3)), B1.I, B3.I);
        const double mid = 0.5 * (w0 + w1);
        for (int bi = 0; bi < NB; ++bi)
            for (int bj = 0; bj < NB; ++bj) {
                if (bi == bj) continue;
                const BeamAtCell Bi = beam(fields, bi, h), Bj = beam(fields, bj, h);
                const PairWave wij = pair_wave(Bi, Bj), wji = pair_wave(Bj, Bi);
                const bool present = pair_present(Bi, Bj, wij);
                REQUIRE(present == pair_present(Bj, Bi, wji), "cell %ld pair %d %d: presence depends on the order", h, bi, bj);
                REQUIRE(present == ((bi == 3 || bj == 3) && bi != 2 && bj != 2), "cell %ld pair %d %d: present %d", h, bi, bj, (int)present);
                if (!present) continue;
                const double gij = pair_gain(c, pref, iaw2, wij), gji = pair_gain(c, pref, iaw2, wji);
                REQUIRE(same_bits(gji, -gij), "cell %ld pair %d %d: g_ij %a g_ji %a", h, bi, bj, gij, gji);
                const double cij = pair_clamp(gij, Bi.I, Bj.I, mid), cji = pair_clamp(gji, Bj.I, Bi.I, mid);
                REQUIRE(same_bits(cji, -cij), "cell %ld pair %d %d: clamped g_ij %a g_ji %a", h, bi, bj, cij, cji);
                REQUIRE(std::fabs(cij) <= std::fabs(gij), "cell %ld pair %d %d: the clamp raised the gain", h, bi, bj);
                REQUIRE(same_bits(pair_clamp(gji, Bj.I, Bi.I, lim), -pair_clamp(gij, Bi.I, Bj.I, lim)), "cell %ld pair %d %d: cell_sat_limit's clamp", h, bi, bj);
                ++pairs;
                if (cij != gij) ++clamped;
                checksum += gij * Bj.I + cij * Bj.I;
            }
    }
}

int main()
{
    GainArgs a{};
    a.nx = NX; a.ny = NY; a.nz = NZ; a.nbeams = NB;
    a.xmin = -0.012; a.ymin = -0.009; a.zmin = -0.007;
    a.dx = 0.006; a.dy = 0.006; a.dz = 0.007;
    a.dt = 1e-13; a.ncrit = 9.05e21; a.k0 = 1.79e5;
    a.cs = 3.1e7; a.gain_const = 2.7e-19; a.iaw = 0.2;
    a.mach_r0 = 0.004; a.mach_0 = 0.3; a.mach_r1 = 0.013; a.mach_1 = 2.1;
    a.sat = 0.05;
    double *ne3d = block(NODES), *flow = block(3 * NODES), *state = block(2 * NODES), *fields = block(4 * NB * CELLS);
    for (long n = 0; n < NODES; ++n) {
        ne3d[n] = a.ncrit * (0.05 + 0.9 * (double)((7 * n) % NODES) / NODES);
        flow[n] = 1e7 * std::sin(0.7 * n); flow[n + NODES] = 2e7 * std::cos(1.3 * n); flow[n + 2 * NODES] = -1.5e7 * std::sin(2.1 * n + 1.0);
        state[n] = 2e7 + 1e6 * (n % 5); state[n + NODES] = 1e-19 * (1 + n % 3);
    }
    ne3d[CRITICAL] = a.ncrit;          // ne / ncrit == 1: eps == 0
    ne3d[ABOVE] = 2.5 * a.ncrit;
    a.ne3d = ne3d;
    const long total = NB * CELLS;
    for (long h = 0; h < CELLS; ++h) {
        const double t = 0.3 + 0.01 * h, kmag = 1.5e5;
        const double dir[NB][3] = {{std::cos(t), std::sin(t), 0.0}, {std::cos(t), std::sin(t), 0.0}, {0.0, 0.6, 0.8},
                                   {-std::sin(t) * 0.6, std::cos(t) * 0.6, 0.8}};
        const double inten[NB] = {1e14 * (1 + h % 4), 3e13 * (1 + h % 7), 0.0, 2e14};
        for (int b = 0; b < NB; ++b) {
            fields[b * CELLS + h] = inten[b];
            for (int x = 0; x < 3; ++x) fields[(x + 1) * total + b * CELLS + h] = kmag * dir[b][x];
        }
    }
    walk<false, false>(a, flow, state, fields);
    walk<false, true>(a, flow, state, fields);
    walk<true, false>(a, flow, state, fields);
    walk<true, true>(a, flow, state, fields);
    REQUIRE(dense_cells > 0 && 2 * clamped >= pairs / 2 && 2 * clamped <= 3 * pairs / 2, "%ld dense cells, %ld of %ld pairs clamped", dense_cells, clamped, pairs);
    std::free(ne3d); std::free(flow); std::free(state); std::free(fields);
    std::printf("gain model ok: %ld cells, %ld ordered pairs, %ld clamped, checksum %.17g\n", 4 * CELLS, pairs, clamped, checksum);
    return 0;
}
'''


def test_gain_model_stays_in_bounds_and_odd_under_asan_ubsan(tmp_path):
    out = run_driver(tmp_path, DRIVER, sources=())
    assert "gain model ok" in out and "checksum" in out
