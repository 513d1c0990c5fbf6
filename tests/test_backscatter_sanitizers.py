"""The bounds promises of the backscatter twin (csrc/cbet_backscatter_host.cpp and csrc/cbet_sbs_model.h):
an item reads its own samples 0 .. nsamples - 1 of the sample-major array and nothing behind them, a step reads ne3d, the flow
and the state table at the sample's node and the fields at that node's cell only, an idle item reads no sample at all, and the
spectra and records are written inside their arrays.  As tests/test_lpi_sanitizers.py: a stand-alone C++ program (the twin
driver's small world, helpers/twin_driver.py) runs the twin over paths that visit every node of the grid -- faces, corners
and the super-critical node included -- with every array a heap block of exactly its size, under AddressSanitizer +
UndefinedBehaviorSanitizer (CPU only; nothing is loaded into Python)."""
from helpers.twin_driver import PRELUDE, run_driver

DRIVER = PRELUDE + r'''
static void *bytes(size_t n) { void *p = std::calloc(n ? n : 1, 1); REQUIRE(p, "calloc"); return p; }

int main()
{
    World w(3, false);
    const cbet_params &p = w.p;
    const int steps = 30, capacity = steps + 1;
    const long nitems = 9;                     // 7 x 30 + 7 = 217 steps cover the 210 nodes; item 3 is idle, item 5 short
    cbet_path_sample *S = (cbet_path_sample *)bytes(sizeof(cbet_path_sample) * capacity * nitems);
    cbet_ray_turn *T = (cbet_ray_turn *)bytes(sizeof(cbet_ray_turn) * nitems);
    int *beams = (int *)bytes(sizeof(int) * nitems);
    long next = 0;
    for (long k = 0; k < nitems; ++k) {
        beams[k] = (int)(k % w.nb);
        if (k == 3) { beams[k] = -7; continue; }                         // idle: status 0, its beam may be anything
        T[k].status = CBET_RAY_LAUNCHED | CBET_RAY_ESCAPED; T[k].steps = steps; T[k].nsamples = capacity;
        if (k == 5) { T[k].steps = 7; T[k].nsamples = 8; }               // a short ray: samples 8 .. 30 are not its own
        for (int t = 0; t <= T[k].steps; ++t) {
            cbet_path_sample &s = S[(long)t * nitems + k];
            const long node = next % w.nodes;
            if (t > 0) ++next;
            s.ci = (int)(node / ((long)p.ny * p.nz)); s.cj = (int)((node / p.nz) % p.ny); s.ck = (int)(node % p.nz);
            s.x = 1e-3 * t * (k + 1); s.y = -7e-4 * t; s.z = 2e-4 * t * t;
            if (k == 6 && t > 10) { s.x = S[10 * nitems + k].x; s.y = S[10 * nitems + k].y; s.z = S[10 * nitems + k].z; }   // ds == 0.0
            s.uray = 5.0 - 0.1 * t; s.step = t;
        }
        if (k == 5)                                                      // ... and hold nodes far outside the grid
            for (int t = 8; t < capacity; ++t) S[(long)t * nitems + k].ci = 1 << 30;
    }
    REQUIRE(next >= w.nodes, "the paths visit %ld of %ld nodes", next, w.nodes);
    double shifts[CBET_SBS_MAX_SHIFTS];
    for (int m = 0; m < CBET_SBS_MAX_SHIFTS; ++m) shifts[m] = 3e11 * (m - 9.0);
    const int counts[3] = {1, 5, CBET_SBS_MAX_SHIFTS};
    double checksum = 0.0;
    long nonzero = 0;
    for (int c = 0; c < 3; ++c)
        for (int tables = 0; tables < 2; ++tables) {
            const int ns = counts[c];
            double *gamma = block((size_t)ns * nitems), *half = block((size_t)ns * nitems);
            cbet_ray_sbs *rays = (cbet_ray_sbs *)bytes(sizeof(cbet_ray_sbs) * nitems), *rays2 = (cbet_ray_sbs *)bytes(sizeof(cbet_ray_sbs) * nitems);
            const double *flow = tables ? w.flow : nullptr, *state = tables ? w.state : nullptr;
            REQUIRE(cbet_backscatter_host(S, T, beams, nitems, capacity, w.fields, w.ne3d, flow, state, CBET_POL_ALIGNED, shifts, ns, gamma,
                                          rays, &w.p, &w.g) == CBET_OK, "%s", cbet_last_error());
            REQUIRE(cbet_backscatter_host(S, T, beams, nitems, capacity, w.fields, w.ne3d, flow, state, CBET_POL_SMOOTHED, shifts, ns, half,
                                          rays2, &w.p, &w.g) == CBET_OK, "%s", cbet_last_error());
            for (long k = 0; k < nitems; ++k) {
                for (int m = 0; m < ns; ++m) {
                    const double v = gamma[m * nitems + k];
                    REQUIRE(std::isfinite(v) && half[m * nitems + k] == 0.5 * v, "item %ld shift %d: %g, smoothed %g", k, m, v, half[m * nitems + k]);
                    REQUIRE(v <= rays[k].gmax, "item %ld: gmax %g below Gamma_%d = %g", k, rays[k].gmax, m, v);
                    if (k == 3) REQUIRE(v == 0.0, "idle item: Gamma_%d = %g", m, v);
                    checksum += v;
                    nonzero += v != 0.0;
                }
                REQUIRE(rays[k].imax >= 0 && rays[k].imax < ns && gamma[rays[k].imax * nitems + k] == rays[k].gmax, "item %ld: imax %d", k, (int)rays[k].imax);
                REQUIRE(rays[k].steps == T[k].steps && rays[k].status == T[k].status, "item %ld: steps %d status %d", k, rays[k].steps, (int)rays[k].status);
                if (k != 3) REQUIRE(rays[k].uray0 == 5.0 && rays[k].uray_end == 5.0 - 0.1 * T[k].steps, "item %ld: uray0 %g uray_end %g", k, rays[k].uray0, rays[k].uray_end);
            }
            std::free(gamma); std::free(half); std::free(rays); std::free(rays2);
        }
    // the refusals leave the arrays alone and read nothing out of range
    double g1[9] = {0};
    cbet_ray_sbs r1[9];
    std::memset(r1, 0, sizeof r1);
    REQUIRE(cbet_backscatter_host(S, T, beams, nitems, capacity, w.fields, w.ne3d, nullptr, nullptr, 0, shifts, 17, g1, r1, &w.p, &w.g) == CBET_EINVAL, "nshift 17");
    REQUIRE(cbet_backscatter_host(S, T, beams, nitems, 8, w.fields, w.ne3d, nullptr, nullptr, 0, shifts, 1, g1, r1, &w.p, &w.g) == CBET_EINVAL, "capacity below nsamples");
    S[4 * nitems + 2].ck = p.nz;                                          // one node just outside
    REQUIRE(cbet_backscatter_host(S, T, beams, nitems, capacity, w.fields, w.ne3d, nullptr, nullptr, 0, shifts, 1, g1, r1, &w.p, &w.g) == CBET_EINVAL, "node outside");
    S[4 * nitems + 2].ck = 0;
    beams[0] = w.nb;
    REQUIRE(cbet_backscatter_host(S, T, beams, nitems, capacity, w.fields, w.ne3d, nullptr, nullptr, 0, shifts, 1, g1, r1, &w.p, &w.g) == CBET_EINVAL, "beam outside");
    for (int k = 0; k < 9; ++k) REQUIRE(g1[k] == 0.0 && r1[k].status == 0, "a refused call wrote item %d", k);
    REQUIRE(nonzero > 100, "%ld non-zero exponents", nonzero);
    std::printf("backscatter twin ok: %ld non-zero exponents, checksum %.17g\n", nonzero, checksum);
    std::free(S); std::free(T); std::free(beams);
    return 0;
}
'''


def test_backscatter_twin_stays_in_bounds_under_asan_ubsan(tmp_path):
    out = run_driver(tmp_path, DRIVER, sources=("cbet_backscatter_host.cpp", "cbet_exchange_host.cpp", "cbet_params.cpp"))
    assert "backscatter twin ok" in out and "checksum" in out
