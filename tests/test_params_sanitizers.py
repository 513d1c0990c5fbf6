"""csrc/cbet_params.cpp is the host's pure arithmetic -- validation, derivation and the launch-list builder with its
hand-indexed 64-entry patches and bundles -- and makes no HIP call.  Build it alone with AddressSanitizer +
UndefinedBehaviorSanitizer (CPU only, no HIP library on the link line: the link succeeding is part of the test) and drive
every arm of the builder from a C++ program that checks the list's invariants itself."""
import os
import subprocess

from cbet_raytracing_3d_amd import build
from conftest import DATA, ROOT

CSRC = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc")

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "cbet_mi355x.h"

#define REQUIRE(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s: ", #cond); std::fprintf(stderr, __VA_ARGS__); \
                                               std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

static cbet_params defaults(int n)
{
    cbet_params p;
    REQUIRE(cbet_params_default(&p, n) == CBET_OK, "n = %d", n);
    return p;
}

// The list through cbet_live_ray_list into a heap block of exactly `cap` entries (an overrun is the sanitizer's to catch).
static std::vector<int> fetch(const cbet_params &p, long cap, long *count)
{
    int *block = (int *)std::malloc((size_t)cap * sizeof(int));
    REQUIRE(block, "malloc");
    REQUIRE(cbet_live_ray_list(&p, block, cap, count) == CBET_OK, "%s", cbet_last_error());
    std::vector<int> out(block, block + cap);
    std::free(block);
    return out;
}

// Returns the number of bundles.  short_cap: also fetch with cap = count - 64 into a block of that size.
static long check(const char *what, const cbet_params &p, bool short_cap = false)
{
    cbet_derived d;
    REQUIRE(cbet_derive(&p, &d) == CBET_OK, "%s: %s", what, cbet_last_error());
    long count = -1, again = -1;
    REQUIRE(cbet_live_ray_list(&p, NULL, 0, &count) == CBET_OK, "%s: %s", what, cbet_last_error());
    REQUIRE(count > 0 && count % 64 == 0, "%s: count = %ld", what, count);
    const std::vector<int> list = fetch(p, count, &again);
    REQUIRE(again == count, "%s: count %ld then %ld", what, count, again);
    std::vector<char> seen((size_t)d.nrays, 0);
    long live = 0;
    for (long b = 0; b < count; b += 64) {
        int in_bundle = 0;
        for (int l = 0; l < 64; ++l) {
            const int id = list[b + l];
            REQUIRE(id == -1 || (id >= 0 && id < d.nrays), "%s: entry %ld is %d, nrays = %d", what, b + l, id, d.nrays);
            if (id < 0) continue;
            REQUIRE(!seen[id], "%s: ray %d listed twice", what, id);
            seen[id] = 1;
            ++in_bundle;
        }
        REQUIRE(in_bundle > 0, "%s: bundle %ld is all holes", what, b / 64);
        live += in_bundle;
    }
    REQUIRE(live == d.nlive_rays, "%s: %ld live entries, nlive_rays = %ld", what, live, d.nlive_rays);
    REQUIRE(d.ntraced_ids <= d.nrays && d.nlive_rays <= d.ntraced_ids, "%s: nrays %d, traced %ld, live %ld", what, d.nrays,
            d.ntraced_ids, d.nlive_rays);
    if (short_cap) {
        const std::vector<int> head = fetch(p, count - 64, &again);
        REQUIRE(again == count, "%s: short fetch reports %ld, not %ld", what, again, count);
        REQUIRE(count == 64 || std::memcmp(head.data(), list.data(), head.size() * sizeof(int)) == 0, "%s: short fetch differs", what);
    }
    std::printf("%s: %ld bundles, %ld live of %d rays (%ld traced)\n", what, count / 64, live, d.nrays, d.ntraced_ids);
    return count / 64;
}

static void refused(const char *what, const cbet_params *p)
{
    cbet_derived d;
    long count = 0;
    REQUIRE(cbet_derive(p, &d) == CBET_EINVAL && cbet_last_error()[0], "%s: cbet_derive", what);
    REQUIRE(cbet_live_ray_list(p, NULL, 0, &count) == CBET_EINVAL && cbet_last_error()[0], "%s: cbet_live_ray_list", what);
}

int main(int argc, char **argv)
{
    REQUIRE(argc == 2, "usage: driver DATA_DIR");
    // The reference's grid.y = threads_per_beam / threads_per_block truncates (main.cu:161): a beam cross-section of fewer
    // rays than one block is not traced at all and its list is empty.  The two smallest cases shrink the block so that
    // their rays are launched.
    cbet_params p = defaults(3);            // one zone, one ray: a single partial patch
    p.rays_per_zone = 1; p.threads_per_block = 1;
    check("n=3 rpz=1", p);
    p = defaults(24);                       // 5 rays per zone: a ray count that is no multiple of 8 per axis
    p.rays_per_zone = 5;
    check("n=24 rpz=5", p, true);
    p = defaults(9);                        // ragged sides, 12 x 12 rays: four patches, all partial
    p.ny = 7; p.nz = 13; p.rays_per_zone = 4; p.threads_per_block = 16;
    check("9x7x13 rpz=4", p);
    p = defaults(48);                       // nrays_x = 68, nrays_y = 28
    p.ny = 21; p.nz = 134;
    check("48x21x134", p);
    p = defaults(8);                        // the upper limit of rays_per_zone
    p.rays_per_zone = 64;
    check("n=8 rpz=64", p);
    {   // main.cu:161's truncated grid.y: 1000 threads in blocks of 256 start 768 of every 1000 ids.  One beam: with the
        // default 60 the 16 threads per beam fill no block at all and the list would be empty.
        p = defaults(64);
        p.nbeams = 1; p.max_threads = 1000; p.threads_per_block = 256;
        cbet_derived d;
        REQUIRE(cbet_derive(&p, &d) == CBET_OK, "%s", cbet_last_error());
        REQUIRE(d.ntraced_ids > 0 && d.ntraced_ids < d.nrays, "truncated grid.y: %ld of %d ids traced", d.ntraced_ids, d.nrays);
        check("n=64 truncated grid.y", p);
    }
    for (int rim : {0, 2, 16})
        for (int order : {0, 1, 2, 5}) {
            p = defaults(64);
            p.rim_merge = rim; p.patch_order = order;
            check(("n=64 rim_merge=" + std::to_string(rim) + " patch_order=" + std::to_string(order)).c_str(), p);
        }
    p = defaults(256);                      // the one size here at which packing the rim wins: 1620 bundles without it
    REQUIRE(check("n=256", p) < 1620, "rim packing did not win at 256^3");

    // refusals that need no device
    refused("NULL params", NULL);
    p = defaults(2);
    refused("n=2", &p);
    p = defaults(10); p.rays_per_zone = 65;
    refused("rays_per_zone 65", &p);
    p = defaults(10); p.rim_merge = 1;
    refused("rim_merge 1", &p);
    p = defaults(10); p.max_threads = p.nbeams - 1;
    refused("max_threads < nbeams", &p);
    REQUIRE(std::strstr(cbet_last_error(), "no threads per beam"), "got: %s", cbet_last_error());
    p = defaults(10); p.xmin = 0.13; p.xmax = -0.13;
    refused("reversed extent", &p);

    // host tables, each into a heap block of exactly its size
    double *phase = (double *)std::malloc(CBET_NPHASE * sizeof(double)), *pw = (double *)std::malloc(CBET_NPHASE * sizeof(double));
    REQUIRE(cbet_host_power_table(phase, pw) == CBET_OK && phase[0] == 0.0 && pw[0] == 1.0 && pw[CBET_NPHASE - 1] < 1e-3, "power table");
    double *trig = (double *)std::malloc(4 * 60 * sizeof(double));
    REQUIRE(cbet_host_beam_trig(cbet_omega60_beam_norm(), 60, trig) == CBET_OK, "%s", cbet_last_error());
    for (int b = 0; b < 60; ++b)
        REQUIRE(std::fabs(trig[4 * b] * trig[4 * b] + trig[4 * b + 1] * trig[4 * b + 1] - 1.0) < 1e-12 &&
                std::fabs(trig[4 * b + 2] * trig[4 * b + 2] + trig[4 * b + 3] * trig[4 * b + 3] - 1.0) < 1e-12, "beam %d", b);
    const std::string path = std::string(argv[1]) + "/s83177_ne.txt";
    double *r = (double *)std::malloc(443 * sizeof(double)), *v = (double *)std::malloc(443 * sizeof(double));
    REQUIRE(cbet_read_profile(path.c_str(), 443, r, v) == CBET_OK && r[442] > r[0], "%s", cbet_last_error());
    double *r2 = (double *)std::malloc(445 * sizeof(double)), *v2 = (double *)std::malloc(445 * sizeof(double));
    REQUIRE(cbet_read_profile(path.c_str(), 445, r2, v2) == CBET_EINVAL && cbet_last_error()[0], "445 rows were read");
    for (double *block : {phase, pw, trig, r, v, r2, v2}) std::free(block);
    p = defaults(10);
    cbet_gain_params g;
    double c1 = 0, cs = 0, gc = 0;
    REQUIRE(cbet_gain_params_default(&g) == CBET_OK && cbet_gain_constants(&p, &g, &c1, &cs, &gc) == CBET_OK, "%s", cbet_last_error());
    REQUIRE(c1 > 0 && cs > 0 && gc > 0 && std::isfinite(c1) && std::isfinite(cs) && std::isfinite(gc), "%g %g %g", c1, cs, gc);
    std::printf("params ok\n");
    return 0;
}
'''


def test_params_unit_links_without_hip_and_is_clean_under_asan_ubsan(tmp_path):
    src = tmp_path / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "driver")
    hip_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "include")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I", hip_include,
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src),
                           os.path.join(CSRC, "cbet_params.cpp"), "-o", exe])
    out = subprocess.run([exe, DATA], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "params ok" in out.stdout and "ERROR" not in out.stderr and "runtime error" not in out.stderr
