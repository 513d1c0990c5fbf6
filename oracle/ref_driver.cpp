/*
 * ref_driver.cpp -- runs the reference's own kernel source, compiled unmodified as host C++ against
 * oracle/ref_shim/, one CUDA "thread" at a time.  TEST INFRASTRUCTURE ONLY (see oracle/ref_build.py, which
 * builds one binary per case, and DESIGN.md section 2).  Our own text: what it needs of the reference's main.cu
 * (span, the pow_r loop, the four constant lines) is not restated here but extracted by the recipe into the
 * generated include files named below, which exist only in the build directory.
 *
 *   run <profile> <beams> <grid out> <side out> <host threads>
 *
 *   profile   binary, r[nr] ne[nr] te[nr] doubles            (nr and everything else: the case's def.cuh)
 *   beams     binary, nbeams x 3 doubles
 *   grid out  binary, (nx+2)(ny+2)(nz+2) doubles, ONE grid for all "GPUs" (beams deposit in ascending order)
 *   side out  binary, int64 nbeams, int64 ray_steps[nbeams], double phase_r[2001], pow_r[2001], xconst, yconst, zconst
 *
 * Launch shape as main.cu:161-176: b < nGPUs, blockIdx.x < nbeams / nGPUs, blockIdx.y < threads_per_beam /
 * threads_per_block, threadIdx.x < threads_per_block.  With one host thread the run is serial and deterministic;
 * with more, the blockIdx.y loop is shared out and the shim's atomicAdd becomes an "omp atomic" add.
 *
 * def.cuh defines short macros (c, nr, dx, dt, nt, Z, ...): every standard header comes first and every name
 * of this file carries a drv_ prefix.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <omp.h>

#include "def.cuh"

#include "ref_main_span.inc" /* main.cu:24-32 */

static std::vector<double> drv_read(const char *drv_path, size_t drv_count) {
    std::vector<double> drv_v(drv_count);
    FILE *drv_f = fopen(drv_path, "rb");
    if (!drv_f) {
        fprintf(stderr, "ref_driver: cannot open %s\n", drv_path);
        exit(2);
    }
    size_t drv_got = fread(drv_v.data(), sizeof(double), drv_count, drv_f);
    int drv_more = fgetc(drv_f);
    fclose(drv_f);
    if (drv_got != drv_count || drv_more != EOF) {
        fprintf(stderr, "ref_driver: %s does not hold exactly %zu doubles\n", drv_path, drv_count);
        exit(2);
    }
    return drv_v;
}

static void drv_write(FILE *drv_f, const void *drv_p, size_t drv_bytes) {
    if (fwrite(drv_p, 1, drv_bytes, drv_f) != drv_bytes) {
        fprintf(stderr, "ref_driver: short write\n");
        exit(2);
    }
}

int main(int argc, char **argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: %s <profile> <beams> <grid out> <side out> <host threads>\n", argv[0]);
        return 2;
    }
    const int drv_threads = std::max(1, atoi(argv[5]));
    const int drv_nbeams = nbeams, drv_nr = nr;
    std::vector<double> drv_prof = drv_read(argv[1], 3 * (size_t)drv_nr);
    std::vector<double> drv_beams = drv_read(argv[2], 3 * (size_t)drv_nbeams);
    double *drv_r = &drv_prof[0], *drv_ne = &drv_prof[drv_nr], *drv_te = &drv_prof[2 * (size_t)drv_nr];
    std::vector<double> drv_edep((size_t)edep_size, 0.0);
    std::vector<double> drv_bbeam(4 * (size_t)drv_nbeams, 0.0); /* the kernel never reads bbeam_norm */
    std::vector<long long> drv_steps(drv_nbeams, 0);

#include "ref_main_pow_r.inc"  /* main.cu:102-110: phase_r, pow_r */
#include "ref_main_consts.inc" /* main.cu:156-159: grad_const, dedx_const, dedy_const, dedz_const */

    /* the static "shared" tables: one pass over a block's threads, tracing nothing (nindices = 0) */
    blockIdx.x = blockIdx.y = blockIdx.z = 0;
    blockDim.x = threads_per_block;
    for (int drv_t = 0; drv_t < threads_per_block; ++drv_t) {
        threadIdx.x = drv_t;
        launch_ray_XYZ(0, 0u, drv_te, drv_r, drv_ne, &drv_edep[0], &drv_bbeam[0], &drv_beams[0], &pow_r[0],
                       &phase_r[0], dedx_const, dedy_const, dedz_const);
    }

    ref_shim_concurrent = drv_threads > 1;
    const long drv_blocks_x = drv_nbeams / nGPUs, drv_blocks_y = threads_per_beam / threads_per_block;
    for (int drv_g = 0; drv_g < nGPUs; ++drv_g) {
        for (long drv_bx = 0; drv_bx < drv_blocks_x; ++drv_bx) {
            unsigned long long drv_calls = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : drv_calls) num_threads(drv_threads)
            for (long drv_by = 0; drv_by < drv_blocks_y; ++drv_by) {
                const unsigned long long drv_before = ref_shim_atomic_calls;
                blockIdx.x = (unsigned)drv_bx;
                blockIdx.y = (unsigned)drv_by;
                blockDim.x = threads_per_block;
                gridDim.x = (unsigned)drv_blocks_x;
                gridDim.y = (unsigned)drv_blocks_y;
                for (int drv_t = 0; drv_t < threads_per_block; ++drv_t) {
                    threadIdx.x = drv_t;
                    launch_ray_XYZ(drv_g, (unsigned)nindices, drv_te, drv_r, drv_ne, &drv_edep[0], &drv_bbeam[0],
                                   &drv_beams[0], &pow_r[0], &phase_r[0], dedx_const, dedy_const, dedz_const);
                }
                drv_calls += ref_shim_atomic_calls - drv_before;
            }
            if (drv_calls % 8) {
                fprintf(stderr, "ref_driver: %llu atomic adds is no multiple of 8\n", drv_calls);
                return 3;
            }
            drv_steps[drv_g * drv_blocks_x + drv_bx] = (long long)(drv_calls / 8);
        }
    }

    FILE *drv_f = fopen(argv[3], "wb");
    if (!drv_f) return 2;
    drv_write(drv_f, &drv_edep[0], drv_edep.size() * sizeof(double));
    fclose(drv_f);
    drv_f = fopen(argv[4], "wb");
    if (!drv_f) return 2;
    const long long drv_nb = drv_nbeams;
    const double drv_consts[3] = {dedx_const, dedy_const, dedz_const};
    drv_write(drv_f, &drv_nb, sizeof drv_nb);
    drv_write(drv_f, &drv_steps[0], drv_steps.size() * sizeof(long long));
    drv_write(drv_f, &phase_r[0], phase_r.size() * sizeof(double));
    drv_write(drv_f, &pow_r[0], pow_r.size() * sizeof(double));
    drv_write(drv_f, drv_consts, sizeof drv_consts);
    fclose(drv_f);
    return 0;
}
