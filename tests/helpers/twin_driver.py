"""The stand-alone programs that run the exchange matrix's host twin under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/test_detuning_host.py, test_polarization_host.py, test_bandwidth_host.py): the C++ text the three drivers share --
REQUIRE, block, same and the small world they all run on -- and the one way such a program is compiled and run (run_driver;
the model headers' tests/test_*_sanitizers.py use it too, with no source beside the driver).  Each test keeps its own cases
and its own main(); nothing is loaded into Python."""
import os
import subprocess

from cbet_raytracing_3d_amd import build
from conftest import ROOT

CSRC = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc")
FLAGS = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-D__HIP_PLATFORM_AMD__"]
TWIN_SOURCES = ("cbet_exchange_host.cpp", "cbet_params.cpp")

PRELUDE = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include "cbet_mi355x.h"

#define REQUIRE(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s: ", #cond); std::fprintf(stderr, __VA_ARGS__); \
                                               std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

static double *block(size_t n) { double *p = (double *)std::calloc(n ? n : 1, sizeof(double)); REQUIRE(p, "calloc"); return p; }
static bool same(const double *a, const double *b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

// One 6 x 5 x 7 grid, nb beams: every array a heap block of exactly its size (an index out of range is the sanitizer's to
// catch), freed with the world.  A super-critical node, tables of flow (and a still one) and state, the sixty shifts and their
// negatives, every beam absent from a seventh of the cells, beams 0 and 1 parallel in every cell (they exchange nothing).
// cell_k: every beam has |k| = kmag of its cell, as the normalisation leaves it, and is absent where the cell is
// super-critical; otherwise |k| = 0.8 k0 everywhere.  T, G, T2, G2: four nb x nb matrices for the cases to write.
struct World {
    cbet_params p;
    cbet_gain_params g;
    cbet_derived d;
    const int nb;
    int hx;
    long nodes, cells, total;
    size_t m;
    double *ne3d, *flow, *still, *state, *fields, *shift, *minus, *T, *G, *T2, *G2;

    World(int beams, bool cell_k) : nb(beams)
    {
        REQUIRE(cbet_params_default(&p, 6) == CBET_OK, "%s", cbet_last_error());
        p.ny = 5; p.nz = 7; p.nbeams = nb;
        REQUIRE(cbet_gain_params_default(&g) == CBET_OK, "%s", cbet_last_error());
        REQUIRE(cbet_derive(&p, &d) == CBET_OK, "%s", cbet_last_error());
        const int hy = p.ny + 2, hz = p.nz + 2;
        hx = p.nx + 2;
        nodes = (long)p.nx * p.ny * p.nz; cells = (long)hx * hy * hz; total = nb * cells;
        ne3d = block(nodes); flow = block(3 * nodes); still = block(3 * nodes); state = block(2 * nodes); fields = block(4 * total);
        shift = block(nb); minus = block(nb);
        for (long n = 0; n < nodes; ++n) {
            ne3d[n] = d.ncrit * (0.05 + 0.9 * (double)((7 * n) % nodes) / nodes);
            for (int x = 0; x < 3; ++x) flow[n + x * nodes] = 2e7 * std::sin(0.7 * n + x);
            state[n] = 2e7 + 1e6 * (n % 5); state[n + nodes] = 1e-19 * (1 + n % 3);
        }
        ne3d[17] = 2.5 * d.ncrit;                                   // a super-critical node
        for (int b = 0; b < nb; ++b) { shift[b] = 4.6e12 * (((37 * b) % 60) - 29.5) / 30.0; minus[b] = -shift[b]; }
        const double k0 = d.omega / 29979245800.0;
        auto clampi = [](int v, int n) { return v < 1 ? 0 : (v > n ? n - 1 : v - 1); };
        for (long h = 0; h < cells; ++h) {
            const int hi = (int)(h / ((long)hy * hz)), hj = (int)((h / hz) % hy), hk = (int)(h % hz);
            const long node = ((long)clampi(hi, p.nx) * p.ny + clampi(hj, p.ny)) * p.nz + clampi(hk, p.nz);
            const double eps = 1.0 - ne3d[node] / d.ncrit;
            const double kmag = !cell_k ? 0.8 * k0 : (eps > 0.0 ? k0 * std::sqrt(eps) : 0.0);
            for (int b = 0; b < nb; ++b) {
                const bool absent = (h + 3 * b) % 7 == 0 || (cell_k && !(eps > 0.0));
                const double t = 0.3 + 0.01 * h + 0.9 * (b % 16), s = 0.2 + 0.05 * b;
                fields[b * cells + h] = absent ? 0.0 : 1e14 * (1 + (h + b) % 4);
                fields[total + b * cells + h] = absent ? 0.0 : kmag * std::cos(t) * std::cos(s);
                fields[2 * total + b * cells + h] = absent ? 0.0 : kmag * std::sin(t) * std::cos(s);
                fields[3 * total + b * cells + h] = absent ? 0.0 : kmag * std::sin(s);
            }
        }
        if (nb >= 2)                                                // beams 0 and 1 parallel in every cell
            for (long h = 0; h < cells; ++h)
                for (int x = 1; x < 4; ++x) fields[x * total + cells + h] = fields[x * total + h];
        m = (size_t)nb * nb;
        T = block(m); G = block(m); T2 = block(m); G2 = block(m);
    }
    World(const World &) = delete;
    ~World()
    {
        for (double *a : {ne3d, flow, still, state, fields, shift, minus, T, G, T2, G2}) std::free(a);
    }
};
'''


def run_driver(tmp_path, text, sources=TWIN_SOURCES):
    """Writes the program `text`, compiles it with `sources` of csrc/ under the sanitizers (no HIP library on the link line),
    runs it with leak detection on and returns its stdout; a failed build, a non-zero exit or a sanitizer report fails the test."""
    src = tmp_path / "driver.cpp"
    src.write_text(text)
    exe = str(tmp_path / "driver")
    hip_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "include")
    subprocess.check_call(["g++"] + FLAGS + ["-I", hip_include, "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src)]
                          + [os.path.join(CSRC, s) for s in sources] + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr
    return out.stdout
