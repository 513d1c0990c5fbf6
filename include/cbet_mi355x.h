/*
 * cbet_mi355x.h -- C ABI of the MI355X-native ray-integrator path.
 *
 * This is the drop-in boundary for the ONE hot path of abowman6/CBET_RayTracing_3D: the
 * launch_ray_XYZ kernel launch (launch_ray_XZ.cu:117-121, launched at main.cu:166-176), the two
 * multi_gpu helpers around it (multi_gpu.cuh:6-7) and the rayTracing() orchestrator that strings
 * them together (main.cu:96-232).  Plain pointers and sizes only; no C++ or torch types.
 * Citations are into /root/reference/.
 *
 * Conventions
 *   - every function that can fail returns an int status: CBET_OK (0) or a negative CBET_E* code;
 *     cbet_last_error() returns a thread-local message.  (The reference returns bool + prints to
 *     cout and its call sites ignore the result, main.cu:136-151; here nothing is fire-and-forget.)
 *   - "device pointer" = memory of the HIP device the call names; streams are hipStream_t passed
 *     as void* (NULL = the device's default stream).
 *   - all arithmetic is fp64; grids are dense C-order arrays.
 */
#ifndef CBET_MI355X_H_
#define CBET_MI355X_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CBET_OK 0
#define CBET_EINVAL (-1)   /* bad argument / unsupported parameter combination */
#define CBET_EHIP (-2)     /* a HIP runtime call failed (message has hipGetErrorString) */
#define CBET_ENOMEM (-3)   /* device out of memory (safeGPUAlloc's free<size guard) */
#define CBET_ENODEVICE (-4)/* GPUIndex == -1 / no such device (moveToAndFromGPU's guard) */
#define CBET_ECOMM (-5)    /* RCCL failure in the multi-GPU orchestrator */

#define CBET_NPHASE 2001   /* length of pow_r / phase_r, main.cu:102-103 */
#define CBET_MAX_CBET_BEAMS 64 /* the CBET stage keeps a beam-presence bit mask per wavefront */

/* Kernel formulations selectable at run time (cbet_params.kernel_variant). */
#define CBET_KERNEL_DEFAULT 0        /* the library's best parity-exact kernel */
#define CBET_KERNEL_GLOBAL_ATOMICS 1 /* one ray per lane, 8 global fp64 atomics per step */
#define CBET_KERNEL_LDS_COMBINE 2    /* wave-private tagged LDS write-combining of the deposits */
#define CBET_KERNEL_LDS_WINDOW 3     /* wave-private dense LDS windows that follow the ray bundle (the default) */

#define CBET_BEAMS_BY_GPU (-1)       /* cbet_params.beam_hi: no explicit beam range, use the ngpus rule */

/*
 * Run-time counterpart of def.cuh's compile-time configuration (def.cuh:33-131).  Fill with
 * cbet_params_default() and override fields; every launch validates it.
 */
typedef struct cbet_params {
    int nx, ny, nz;              /* def.cuh:35-46 xyz_size (nodes per axis, >= 3)              */
    double xmin, xmax;           /* def.cuh:37-38                                              */
    double ymin, ymax;           /* def.cuh:42-43                                              */
    double zmin, zmax;           /* def.cuh:47-48                                              */
    int nbeams;                  /* def.cuh:58  rows in beam_norm                              */
    int rays_per_zone;           /* def.cuh:71                                                 */
    double courant_mult;         /* def.cuh:80                                                 */
    int absorption;              /* def.cuh:118 (1: absorb; else bookkeeping mode)             */
    int nprofile;                /* def.cuh:33  nr, rows of the radial ne/Te profile           */
    int max_threads;             /* def.cuh:125 (enters the reference's traced-id rule)        */
    int threads_per_block;       /* def.cuh:127 (enters the reference's traced-id rule)        */
    int ngpus;                   /* def.cuh:116 nGPUs: with beam_hi < 0 (unset, the default),  */
                                 /* launch `b` owns beams [b*(nbeams/ngpus), (b+1)*(nbeams/ngpus)), */
                                 /* as at launch_ray_XZ.cu:123                                 */
    int beam_lo, beam_hi;        /* explicit beam range [lo,hi) overriding the ngpus rule;     */
                                 /* beam_hi = CBET_BEAMS_BY_GPU (-1, what cbet_params_default  */
                                 /* sets) = not given.  An empty range [k,k), [0,0) included,  */
                                 /* is an explicit no-op: a rank that owns no beam traces nothing */
    int shard_index, shard_count;/* ray-bundle sharding inside the beam range: the (beam, patch) */
                                 /* list is cut into shard_count contiguous near-equal parts    */
                                 /* and part shard_index is traced (shard_count<=1: everything) */
    int kernel_variant;          /* CBET_KERNEL_*                                              */
    int force_wide_index;        /* test hook: use the 64-bit node-table indexing path that grids  */
                                 /* with 8*nx*ny*nz >= 2^32 bytes (n > 812) need, at any size      */
    int per_beam_grids;          /* 1: beam-resolved deposition -- edep is nbeams grids of            */
                                 /* (nx+2)(ny+2)(nz+2) doubles and beam b adds into grid b (what a    */
                                 /* cross-beam stage needs: every beam's own field); 0: one grid      */
    int patch_order;             /* 1 = longest first: a beam's patches are listed by descending      */
                                 /* launch radius (outer rays take ~3x the steps of central ones);     */
                                 /* 0 = Morton curve; k >= 2 = k radial rings, Morton inside each (all    */
                                 /* measured within 2 % of each other on one device at 256^3).  Part of   */
                                 /* the geometry a context is created for.                               */
    int grid_beam0, grid_beams;  /* beam-resolved arrays (per_beam_grids output, the field pass's output, the  */
                                 /* gain coefficient) that hold only the grids of beams [grid_beam0,          */
                                 /* grid_beam0 + grid_beams): beam b uses grid b - grid_beam0.  grid_beams = 0 */
                                 /* (default): the arrays hold all nbeams grids.  This is how a rank of the    */
                                 /* slab-owned CBET loop keeps only ITS beams' fields and gain.                */
    int rim_merge;               /* patches on the rim of the beam cross-section hold fewer than 64 live rays:  */
                                 /* their rays are pooled, walked by angle around the beam axis and cut into    */
                                 /* bundles of up to 64 rays with a footprint of at most rim_merge launch zones */
                                 /* (= cells) per axis (default 4: 16 rays at 4 rays per zone; 0 = every bundle */
                                 /* is one 8x8 patch).  The same rays are traced; at 256^3 lane utilisation goes from */
                                 /* 0.907 to 0.957 (1620 -> 1552 bundles per beam).  Part of the geometry a     */
                                 /* context is created for.                                                     */
    int edep_zpitch;             /* 0 (default): `edep` has the reference's dense layout, rows of nz+2 doubles   */
                                 /* (launch_ray_XZ.cu:5-7).  p >= nz+2: the caller's grid has rows of p doubles  */
                                 /* -- node (i,j,k) at (i*(ny+2) + j)*p + k; the entries k >= nz+2 of a row are   */
                                 /* padding the launch never touches.  For callers that own their deposit grid's */
                                 /* layout (pipeline.SweepPipeline pads its private grids' rows to whole 64-byte  */
                                 /* lines).  With an earlier kernel the pass time depended on where a dense grid  */
                                 /* landed relative to the record table (16.9 ... 18.6 ms); with the current one  */
                                 /* five fresh dense allocations give 12.53 ... 12.72 ms: the effect is gone, the */
                                 /* padding is harmless.  Plain path only.                */
    int window_stats;            /* 0 (default): a launch of the default kernel counts ray_steps and rays_traced  */
                                 /* only.  1: the instantiation that also counts the deposit windows' diagnostics  */
                                 /* (global_atomics, lds_evictions, wave_steps, wave_steps_miss, wave_steps_wide,  */
                                 /* slabs_retired) -- a few scalar instructions per step that a timed launch does  */
                                 /* not need.  The cross-check kernels (variants 1, 2) always count what they count. */
} cbet_params;

/* Quantities the reference derives in def.cuh / main.cu:156-161, evaluated in the same order. */
typedef struct cbet_derived {
    double dx, dy, dz, dt;       /* def.cuh:39,44,49,81                                        */
    int nt;                      /* def.cuh:83-84                                              */
    int zones_spanned;           /* launch_ray_XZ.cu:69                                        */
    int nrays_x, nrays_y, nrays; /* def.cuh:75-77                                              */
    double omega, ncrit;         /* def.cuh:68-69                                              */
    double uray_mult;            /* def.cuh:92                                                 */
    double xconst, yconst, zconst; /* main.cu:156-159 dedx_const, dedy_const, dedz_const       */
    long threads_per_beam;       /* def.cuh:128                                                */
    int nindices;                /* def.cuh:129                                                */
    int grid_y;                  /* main.cu:161                                                */
    long edep_size;              /* def.cuh:131 (nx+2)(ny+2)(nz+2)                             */
    long ntraced_ids;            /* thread-ray ids per beam the launch shape visits            */
    long nlive_rays;             /* of those, rays inside the beam radius (per beam)           */
} cbet_derived;

/* Counters a launch accumulates on the device (read back with cbet_context_counters).  The default kernel fills
 * ray_steps and rays_traced always; the other six (the deposit windows' diagnostics) only when cbet_params.window_stats
 * is set -- they stay 0 otherwise.  The cross-check kernels (variants 1, 2) fill what applies to them. */
typedef struct cbet_counters {
    unsigned long long ray_steps;        /* integrator iterations that reached the deposition  */
    unsigned long long rays_traced;      /* live rays launched                                 */
    unsigned long long global_atomics;   /* fp64 atomics that went to HBM                      */
    unsigned long long lds_evictions;    /* LDS_COMBINE: slots written back before the end;    */
                                         /* LDS_WINDOW: ray-steps that fell outside the window */
    unsigned long long wave_steps;       /* integrator iterations per wavefront (64 lane slots each) */
    unsigned long long wave_steps_miss;  /* LDS_WINDOW: wave-steps in which some lane missed the window */
    unsigned long long wave_steps_wide;  /* LDS_WINDOW: wave-steps in which the second box was live     */
    unsigned long long slabs_retired;    /* LDS_WINDOW: wave-steps in which a box origin moved (planes / */
                                         /* z-bricks written back to HBM)                               */
} cbet_counters;

typedef struct cbet_context cbet_context; /* per-device workspace: node tables, ray list, counters */

/* ---- configuration ------------------------------------------------------------------------ */
const char *cbet_last_error(void);
const char *cbet_version(void);

/* def.cuh defaults at grid size n (n = 100 is the shipped configuration). */
int cbet_params_default(cbet_params *p, int n);
int cbet_derive(const cbet_params *p, cbet_derived *d);

/*
 * The beam-independent launch list, in the order the trace kernel consumes it.  The beam cross
 * section is cut into 8x8-ray patches (cbet_params.patch_order); 64 consecutive entries = one ray bundle = one
 * wavefront: one patch, or rays of the rim patches packed together (cbet_params.rim_merge; those bundles come first).  An entry is the thread-ray id (launch_ray_XZ.cu:125,156) of that ray,
 * or -1 for a hole: a ray the reference launch shape never visits or one that fails init()'s
 * beam-radius test (:94,114).  Work items g are (beam, patch) pairs, beam by beam, patch by patch;
 * shard s of K traces the items [s T / K, (s + 1) T / K) of the T in the list.
 * Writes min(n, cap) entries to out (may be NULL) and n to *count.
 */
int cbet_live_ray_list(const cbet_params *p, int *out, long cap, long *count);

/* omega_beams.h:1-62 : the 60 OMEGA port normals, double[60][3], row-major. */
const double *cbet_omega60_beam_norm(void);
/* main.cu:24-32 + 102-110 : phase_r = span(0,0.1,2001), pow_r = exp(-((r/sigma)^2)^2.5); host arrays. */
int cbet_host_power_table(double *phase_r, double *pow_r);
/* main.cu:121-129 : better_beam_norm, 4 doubles per beam {cos t1, sin t1, cos t2, sin t2}; host arrays. */
int cbet_host_beam_trig(const double *beam_norm, int nbeams, double *bbeam_norm);
/* main.cu:249-260 : read exactly nprofile rows "r value" of a profile file into r[] and v[]. */
int cbet_read_profile(const char *path, int nprofile, double *r, double *v);

/* ---- multi_gpu.cuh:6-7 helpers -------------------------------------------------------------- */
/*
 * safeGPUAlloc (multi_gpu.cpp:3-28): makes `gpu` current (and leaves it current), fails with
 * CBET_ENOMEM when free < size, otherwise hipMalloc.  Returns CBET_OK where the reference
 * returns true.
 */
int cbet_safeGPUAlloc(void **dst, size_t size, int gpu);
/*
 * moveToAndFromGPU (multi_gpu.cpp:44-59): gpu == -1 -> CBET_ENODEVICE; blocking copy with the
 * direction inferred from the pointers (hipMemcpyDefault); the caller's current device is
 * preserved.
 */
int cbet_moveToAndFromGPU(void *dst, void *src, size_t size, int gpu);
/* cudaFree counterpart for memory from cbet_safeGPUAlloc (main.cu:180-187). */
int cbet_gpuFree(void *ptr, int gpu);

/* ---- workspace ------------------------------------------------------------------------------ */
/*
 * Allocates the per-device workspace a launch needs (node tables ne3d/kappa3d of nx*ny*nz doubles
 * each, the compacted live-ray list, counters) so that cbet_launch_ray_XYZ itself never
 * allocates or synchronises (graph-capturable).  The context is bound to `gpu` and to the grid /
 * ray geometry in *p; sharding, beam range and kernel variant may change per launch.
 */
int cbet_context_create(cbet_context **ctx, const cbet_params *p, int gpu);
int cbet_context_destroy(cbet_context *ctx);
/* Synchronises `stream`, copies the counters to *out and, if reset != 0, zeroes them. */
int cbet_context_counters(cbet_context *ctx, void *stream, cbet_counters *out, int reset);
/*
 * Replace the context's launch list (cbet_live_ray_list's layout: 64 entries per bundle, -1 = idle lane) by a
 * regrouping of the SAME rays -- every live ray exactly once, no empty bundle; anything else is CBET_EINVAL.  For a
 * caller that knows how long its rays live (e.g. from a previous pass) and wants bundles of rays that end together;
 * the trace deposits the same sums in a different order.  Synchronises the device.
 */
int cbet_context_set_launch_list(cbet_context *ctx, const int *list, long n);
/*
 * *length = L, the number of entries of the context's current launch list (holes included; 64 per bundle): the count
 * cbet_live_ray_list reports, or the n of the last cbet_context_set_launch_list.  The per-beam stride of the exit
 * records (cbet_trace_exits).
 */
int cbet_context_list_length(const cbet_context *ctx, long *length);
/*
 * Device pointers of the context's own node tables (for tests / the 3-D plasma entry below).  They are writable:
 * the call marks the tables as modified, so the next launch that uses them (ne3d = kappa3d = NULL) rebuilds the
 * per-node step records it gathers from.  Call it again (or cbet_prepare_step_records) after EVERY later in-place
 * modification -- a launch cannot see a write on its own.
 */
int cbet_context_tables(cbet_context *ctx, double **ne3d, double **kappa3d);
/*
 * For tests: *records = device pointer of the context's per-node step records (nx*ny*nz records of four doubles
 * {kx, ky, kz, kappa}, read-only), *builds = how many launches have written them so far (a launch that finds them
 * current does not).  Either may be NULL.
 */
int cbet_context_step_records(const cbet_context *ctx, const void **records, unsigned long long *builds);

/*
 * Bounds-audit builds only (-DCBET_DEBUG_BOUNDS; tests/test_gpu_bounds_audit.py): number of
 * out-of-range grid atomics / node-table gathers / LDS accumulates the kernels attempted (and
 * skipped) on the current device since the last reset.  Regular builds return CBET_EINVAL.
 */
int cbet_debug_bounds_violations(unsigned long long *out, int reset, void *stream);

/* ---- the hot path ---------------------------------------------------------------------------- */
/*
 * launch_ray_XYZ (launch_ray_XZ.cu:117-121; launch site main.cu:171-174).  Same thirteen
 * arguments, same order and meaning:
 *   b          GPU ordinal of the reference's beam split (see cbet_params.ngpus / beam_lo)
 *   nindices   strided passes per thread (def.cuh:129) -- enters the traced-id rule only
 *   te_data_g, r_data_g, ne_data_g   device, nprofile doubles each (main.cu:149-151)
 *   edep       device, (nx+2)(ny+2)(nz+2) doubles, x-major/z-fastest with a one-cell halo
 *              (launch_ray_XZ.cu:5-7); ACCUMULATED into, never cleared (caller zeroes it).
 *              With params->per_beam_grids: nbeams such grids, beam b's at offset b * grid size.
 *   bbeam_norm device, 4*nbeams doubles from cbet_host_beam_trig; the reference uploads but
 *              ignores it (main.cu:146) -- here it supplies the rotation cos/sin so that launch
 *              points equal the host libm's to the last bit.  NULL: trig evaluated on the device.
 *   beam_norm  device, 3*nbeams doubles
 *   pow_r, phase_r  device, CBET_NPHASE doubles each
 *   xconst, yconst, zconst  main.cu:156-159
 * plus: the run-time parameters, the workspace and the stream.  Work is enqueued on `stream`
 * (node tables and, for the default kernel, the per-node step records in one kernel -> trace; the
 * cross-check kernels: node tables -> trace) and the call returns without synchronising; launch errors are
 * reported through the return value (the reference checks nothing, main.cu:171-175).
 */
int cbet_launch_ray_XYZ(int b, unsigned nindices, double *te_data_g, double *r_data_g,
                        double *ne_data_g, double *edep, double *bbeam_norm, double *beam_norm,
                        double *pow_r, double *phase_r, double xconst, double yconst,
                        double zconst, const cbet_params *p, cbet_context *ctx, void *stream);

/*
 * The two halves of cbet_launch_ray_XYZ, for callers that hold a 3-D plasma state:
 *   cbet_tabulate_plasma : radial profiles -> ctx node tables (values the reference would
 *       interpolate at each node, launch_ray_XZ.cu:254-265, 296-305).
 *   cbet_trace_nodes     : trace using caller-supplied node tables ne3d / kappa3d of nx*ny*nz
 *       doubles (NULL = the context's own), i.e. an arbitrary, not necessarily spherical, plasma.
 *   cbet_prepare_step_records : optional.  The default kernel gathers ONE 32-byte record per node and step
 *       -- the three velocity kicks xconst * (ne(x+1) - ne(x-1)) of launch_ray_XZ.cu:268-270 with the face
 *       rule of :212-238, and kappa3d -- which a launch builds from the tables and xconst / yconst / zconst
 *       when they are not current.  Calling this first moves that pass (0.15 ms at 256^3) out of the launch;
 *       records built from the context's own tables stay valid until the next cbet_tabulate_plasma.
 *   cbet_prepare_plasma  : cbet_tabulate_plasma directly followed by cbet_prepare_step_records(ctx, p, NULL, NULL, ...)
 *       as ONE kernel: ne is evaluated plane by plane into LDS and the records are formed there, instead of reading
 *       back the table the first kernel has just written.  Node tables and records are bit for bit those of the two
 *       calls, and so is what the context remembers about them (the records stay valid until the tables change).
 *       cbet_launch_ray_XYZ with the default kernel, and a pass of the pipeline, prepare their plasma this way.
 */
int cbet_tabulate_plasma(cbet_context *ctx, const cbet_params *p, const double *te_data_g,
                         const double *r_data_g, const double *ne_data_g, void *stream);
int cbet_trace_nodes(int b, unsigned nindices, const double *ne3d, const double *kappa3d,
                     double *edep, const double *bbeam_norm, const double *beam_norm,
                     const double *pow_r, const double *phase_r, double xconst, double yconst,
                     double zconst, const cbet_params *p, cbet_context *ctx, void *stream);
int cbet_prepare_step_records(cbet_context *ctx, const cbet_params *p, const double *ne3d,
                              const double *kappa3d, double xconst, double yconst, double zconst,
                              void *stream);
int cbet_prepare_plasma(cbet_context *ctx, const cbet_params *p, const double *te_data_g,
                        const double *r_data_g, const double *ne_data_g, double xconst, double yconst,
                        double zconst, void *stream);

/* ---- perturbed targets -------------------------------------------------- */
/*
 * The radial profiles evaluated on a target that sits off centre and whose iso-surfaces are distorted by real spherical
 * harmonics: the producer of node tables for cbet_trace_nodes / cbet_trace_exits that is not spherical about the origin.
 *
 * Model.  Node (i, j, k) has cbet_tabulate_plasma's coordinates xc = i*dx + xmin (y, z alike; dx from cbet_derive).  With
 * the target's offset o and coefficients c[(lmax+1)^2], every statement ONE IEEE fp64 operation per written operator, in
 * the written order, no fused multiply-add:
 *     sx = xc - ox,  sy = yc - oy,  sz = zc - oz
 *     rho   = sqrt(sx*sx + sy*sy + sz*sz)                       (squares summed x, y, z)
 *     delta = sum_c c[c] Y_c(s / rho)                           (order below)
 *     rho'  = rho / (1.0 + delta)
 *     ed, etemp = ne, Te interpolated at rho'                   (cbet_tabulate_plasma's bisection and interpolation)
 *     kappa = ed / ncrit * nuei * dt                            (launch_ray_XZ.cu:299-305, cbet_tabulate_plasma's statements)
 * c_lm is a relative radial displacement dR/R of every iso-surface in the direction (theta, phi): the surface that the
 * unperturbed target has at radius R lies at R (1 + delta(theta, phi)) around the point o.  Te follows the same rho'.
 *
 * Harmonics: cbet_sph_modes's -- real, orthonormal, no Condon-Shortley phase, index c = l*l + l + m, m > 0 the cos(m phi)
 * and m < 0 the sin(|m| phi) member.  Their evaluation here is this header's own (cbet_sph_modes fuses the recurrence's
 * multiply-subtract; this one does not), with a table F of factors computed ONCE on the host by correctly rounded sqrt and
 * division and used by the device kernel and the host twin alike:
 *     y00 = 1.0 / sqrt(4.0 * pi),  q2 = sqrt(2.0),  d_k = sqrt((double)(2k+1) / (double)(2k))            (k = 1 .. 16)
 *     a_lm = sqrt((double)(4 l l - 1) / (double)(l l - m m)),
 *     b_lm = sqrt((double)((l-1)(l-1) - m m) / (double)(4 (l-1)(l-1) - 1))                               (0 <= m < l <= 16)
 * Angles:  rxy = sqrt(sx*sx + sy*sy),  ct = sz / rho,  st = rxy / rho,  (c1, s1) = (sx / rxy, sy / rxy); ON THE z AXIS
 * (rxy == 0) (c1, s1) = (1, 0), as cbet_sph_modes takes it.  Then, with L the library's instantiation (the smallest of
 * 0, 2, 8, 16 that covers the highest l with a non-zero coefficient; coefficients beyond the call's lmax count as 0 --
 * their terms add +-0 and change no table entry):
 *     pmm = y00, cr = 1, si = 0
 *     for m = 0 .. L                                              (m outermost)
 *         if m > 0:  pmm = (pmm * d_m) * st;  cn = cr*c1 - si*s1;  si = cr*s1 + si*c1;  cr = cn
 *         p1 = pmm, p2 = 0;  A = c[m*m+m+m] * pmm;  B = c[m*m+m-m] * pmm   (m > 0)
 *         for l = m+1 .. L:   y = a_lm * (ct*p1 - b_lm*p2);  p2 = p1;  p1 = y;
 *                             A = A + c[l*l+l+m] * y;  B = B + c[l*l+l-m] * y   (m > 0)
 *         m == 0:  delta = A;      m > 0:  delta = delta + ((q2*cr) * A + (q2*si) * B)
 * AT rho == 0 (a node exactly at the target's centre, no direction):  delta = c[0] * y00.  L == 0:  delta = c[0] * y00
 * at every node.
 *
 * Limits: 0 <= lmax <= CBET_TARGET_LMAX; offset and coefficients finite; and, so that 1 + delta > 0 everywhere,
 *     sum_c |c[c]| sqrt((2 l_c + 1) / (4 pi)) < 1
 * (sufficient: sum_m Y_lm^2 = (2l+1)/(4 pi), so no |Y_lm| exceeds that root).  Anything else is CBET_EINVAL before any
 * device work.
 *
 * Identity: with o = 0 and all c = 0 every operation above is exact (x - 0, 0 * y00, rho / 1.0): the tables are, bit for
 * bit, cbet_tabulate_plasma's.
 */
#define CBET_TARGET_LMAX 16
typedef struct cbet_target {
    double offset[3];      /* o: the target's centre (cm)                                          */
    int lmax;              /* 0 .. CBET_TARGET_LMAX                                                 */
    const double *coeffs;  /* HOST array of (lmax+1)^2 doubles, or NULL = all zero                  */
} cbet_target;
/*
 * Device profiles (as for cbet_tabulate_plasma) -> the context's ne3d / kappa3d.  Behaves towards the context exactly
 * like cbet_tabulate_plasma: the same validation and geometry check, enqueued on `stream` without allocation or
 * synchronisation (graph-capturable), and the step records are marked stale, so the next launch that uses the context's
 * tables rebuilds them.  The target's host arrays are captured at the call.
 */
int cbet_tabulate_target(cbet_context *ctx, const cbet_params *p, const double *te_data_g, const double *r_data_g,
                         const double *ne_data_g, const cbet_target *target, void *stream);
/* The host twin, plain loops: HOST profiles of p->nprofile rows -> HOST ne3d / kappa3d of nx*ny*nz doubles each. */
int cbet_target_tables(const cbet_params *p, const double *te, const double *r, const double *ne,
                       const cbet_target *target, double *ne3d, double *kappa3d);

/* ---- orchestrator ---------------------------------------------------------------------------- */
/*
 * rayTracing (main.cu:96-232): host profiles in, host edep (caller-owned, (nx+2)(ny+2)(nz+2)
 * doubles) ADDED into.  Uses devices gpus[0..ngpu) (NULL: 0..ngpu-1), one host thread per device;
 * device g of G traces the contiguous part [T g / G, T (g+1) / G) of the beam-major list of T ray bundles
 * (no beam is lost to nbeams/nGPUs truncation), the per-device grids are combined on the devices by one
 * RCCL reduce-scatter into x-slabs, and every device's host thread downloads ITS slab and adds it into
 * edep (replacing the whole-grid D2H copies and the serial host += loop of main.cu:178-210).
 * beam_norm: host double[nbeams][3] (the reference reads the global table of omega_beams.h);
 * NULL = cbet_omega60_beam_norm().  timers (may be NULL) receives {init, tracing, combining,
 * total} seconds as main.cu:219-231 prints; counters (may be NULL) the summed device counters.
 */
int cbet_ray_tracing(const double *te_profile, const double *r_profile, const double *ne_profile,
                     double *edep, const cbet_params *p, const double *beam_norm, const int *gpus,
                     int ngpu, double *timers, cbet_counters *counters);

/* ---- output stage ------------------------------------------------------ */
/*
 * print(std::cout, edep) under -D PRINT (main.cu:6-22, 353-355): the nested "[a,b,...]\n" text
 * at operator<<'s default 6 significant digits -- the format of the reference's golden file
 * truth_100 (Makefile:14-17).  edep: HOST array [d0][d1][d2].  path NULL or "-" = stdout.
 * Returns the number of bytes written, or a negative CBET_E* code.
 */
long long cbet_write_text(const double *edep, int d0, int d1, int d2, const char *path);
/*
 * The 27-point node average of main.cu:334-349 (commented out in the reference):
 * edepavg[nx][ny][nz] from the haloed HOST array edep[nx+2][ny+2][nz+2], same summation order.
 */
int cbet_edep_average(const double *edep, double *edepavg, int nx, int ny, int nz);
/* The same on the current device: edep and edepavg are DEVICE arrays; enqueued on `stream`, same bits. */
int cbet_edep_average_device(const double *edep, double *edepavg, int nx, int ny, int nz, void *stream);
/* main.cu:321-332 (commented out in the reference): HOST arrays x, y, z of [nx][ny][nz] node coordinates. */
int cbet_node_coordinates(const cbet_params *p, double *x, double *y, double *z);
/*
 * Binary output.  The reference's is save2Hdf5 (main.cu:37-94: /Coordinate_x,y,z and /Edepavg, [nx][ny][nz]
 * little-endian fp64) -- dead code there, and libhdf5 does not exist in this image.  The same HOST arrays
 * can be written as NumPy .npy files (format 1.0, C order, '<f8'): data[shape[0]]...[shape[ndim-1]].
 * Returns the number of bytes written, or a negative CBET_E* code.
 */
long long cbet_write_npy(const double *data, int ndim, const long *shape, const char *path);

/* ---- CBET stage ------------------------------------------------------------- */
/*
 * PARITY UNPINNED.  The reference has no cross-beam energy transfer code -- only the unused constants
 * of def.cuh:94-114 (estat, mach, Z, mi, Te, Ti, iaw, kb, constant1, cs, u_flow) -- so this stage has
 * no reference output to match.  It implements the steady-state ion-acoustic gain of the ray-based
 * CBET codes those constants come from, on per-beam FIELDS of the deposit grid:
 *
 *   dI_i/ds = I_i K_i,   K_i = sum_{j != i} G_ij I_j,   G_ij = -G_ji
 *   G_ij = constant1 (8 pi 1e7 / c) (ne/ncrit) (1/iaw) P(eta_ij) / sqrt(1 - ne/ncrit)
 *   eta_ij = -(k_j - k_i).u / (|k_j - k_i| cs + 1e-10),  P = iaw^2 eta / ((eta^2 - 1)^2 + iaw^2 eta^2)
 *
 * with a radial outflow u = Mach(r) cs r_hat (def.cuh:114 refers to an undefined `machnum`).  It is
 * checked against a CPU restatement of the same model (oracle/, tests/test_gpu_cbet.py), by the exact
 * antisymmetry of the exchange and by energy conservation at the fixed point.
 */
typedef struct cbet_gain_params {
    double z_ion;          /* def.cuh:100   Z = 3.1                                             */
    double te_ev, ti_ev;   /* def.cuh:104, 106                                                   */
    double mi_over_me;     /* def.cuh:101-102  10230                                             */
    double iaw;            /* def.cuh:107   ion-acoustic wave damping nu_ia / omega_s            */
    double mach_r0, mach_0, mach_r1, mach_1;  /* Mach number ramps linearly from mach_0 at radius mach_r0 to mach_1 at mach_r1 (clamped outside) */
    double max_exponent;   /* clamp on |K ds| per ray-step, 0 < max_exponent <= 1                */
    double relax;          /* K <- K + relax (K_raw - K) between passes, 0 < relax <= 1          */
    double tolerance;      /* cbet_cbet_solve stops when sum |dK| / sum |K| falls below it       */
    int max_passes;        /* ... or after this many field passes                                */
    int direction_passes;  /* the first direction_passes (>= 1, default 1) field passes deposit all four fields and
                              build the direction field k; later passes deposit the energy field alone and reuse k --
                              gain changes ray energies, not ray paths, so k of the gain-free first pass is kept      */
    int directions_frozen; /* cbet_gain_field*: 1 = the three direction components of `fields` already hold k (an
                              earlier call normalised them): only the energy component is read and normalised       */
    int reserved_;
} cbet_gain_params;

typedef struct cbet_cbet_report {
    int passes;                      /* field passes run                                        */
    int converged;                   /* 1: tolerance reached                                    */
    double change;                   /* last sum |dK| / sum |K|                                 */
    double imbalance;                /* |sum_b gained_b| / sum_b |gained_b| of the final pass   */
    double beam_gain[CBET_MAX_CBET_BEAMS]; /* energy each beam gained in the final pass          */
    unsigned long long ray_steps;    /* all ray-steps traced, field passes included             */
    unsigned long long ray_steps_final; /* ray-steps of the final (deposition) pass              */
} cbet_cbet_report;

int cbet_gain_params_default(cbet_gain_params *g);
/* def.cuh:111 constant1, def.cuh:113 cs, and gain_const = constant1 * 8 pi 1e7 / c (any may be NULL) */
int cbet_gain_constants(const cbet_params *p, const cbet_gain_params *g, double *constant1, double *cs,
                        double *gain_const);
/*
 * cbet_trace_nodes with the CBET hooks.  gain: device [nbeams][(nx+2)(ny+2)(nz+2)] gain coefficient
 * per beam on the deposit grid (1/cm), or NULL; every ray-step gathers it from its eight deposit
 * nodes with the deposit weights and multiplies the ray's energy by exp(K |v| dt) before absorption.
 * quantity says what a step deposits into `out`:
 *   CBET_DEPOSIT_ENERGY  the absorbed energy (the reference's edep; `out` as for cbet_trace_nodes);
 *   CBET_DEPOSIT_FIELD_ENERGY  the first of those four fields alone (out is [nbeams][(n+2)^3], i.e. the head of a
 *                        fields array): what every field pass after the direction-building ones deposits;
 *   CBET_DEPOSIT_FIELDS  the four per-beam fields the gain needs, in ONE trace: out is
 *       [4][nbeams][(n+2)^3] -- component 0 the step-averaged ray energy x path length, spread over the
 *       eight deposit nodes with the deposit weights; components 1..3 that energy x the step's
 *       displacement along x/y/z, at the ray's own (nearest) node.
 * beam_gain: device [nbeams], ADDED into: energy each beam gained (may be NULL).  Default kernel knobs only.
 */
#define CBET_DEPOSIT_ENERGY 0
#define CBET_DEPOSIT_FIELDS 1
#define CBET_DEPOSIT_FIELD_ENERGY 2
int cbet_trace_cbet(int b, unsigned nindices, const double *ne3d, const double *kappa3d,
                    const double *gain, int quantity, double *out, double *beam_gain,
                    const double *bbeam_norm, const double *beam_norm, const double *pow_r,
                    const double *phase_r, double xconst, double yconst, double zconst,
                    const cbet_params *p, const cbet_gain_params *g, cbet_context *ctx, void *stream);
/*
 * fields: device [4][nbeams][(n+2)^3] = what a CBET_DEPOSIT_FIELDS pass deposited;
 * normalised IN PLACE to (intensity, k_x, k_y, k_z) wherever the beam's rays deposited (intensity 0 where the
 * energy is not positive); with g->directions_frozen the k entries are taken as they are and only the energy
 * entries are read and normalised.  gain: device [nbeams][(n+2)^3], updated to
 * gain + relax (K - gain).  change: device double[2], ADDED into: {sum |new - old|, sum |new|}
 * (may be NULL).  scratch: a SELECTOR, kept in the signature for ABI stability: any non-NULL pointer selects
 * the kernel that evaluates every unordered beam pair once with the cell's beams staged in LDS (it is never
 * dereferenced since round 3 -- pass `gain`); NULL selects the ordered kernel (twice the pair evaluations, every
 * statement one IEEE operation in the CPU checker's order; the pair-once kernel's K agrees with it to ~1e-13
 * of the largest |K|).  ne3d NULL = the context's node table.  Needs nbeams <= CBET_MAX_CBET_BEAMS.
 * Alignment: `fields` and `gain` need the alignment of a double only (a view that starts anywhere inside a larger
 * allocation is accepted).  The pair-once kernel cuts a z-row into runs of 16 cells by the cells' ELEMENT INDEX in the
 * arrays ((row start - first stored element) mod 16), not by their address, so the grouping of a cell's pair sums -- and
 * with it every bit of K -- is the same wherever the arrays start; it does follow the STORAGE (whole grid or
 * cbet_gain_field_packed's slab, whose first element is another cell: equal to ~1e-13 of the largest |K|, not bit for
 * bit).  The runs are whole 128-byte lines only when the arrays start on one: other starts cost time, never bits.
 */
int cbet_gain_field(double *fields, const double *ne3d, double *gain, double *scratch, double *change,
                    const cbet_params *p, const cbet_gain_params *g, cbet_context *ctx, void *stream);
/*
 * The same for the x-planes [hx_lo, hx_hi) of the deposit grid only (0 <= hx_lo <= hx_hi <= nx+2): one rank's
 * slab when the gain update is shared between ranks (tracer.cbet_fixed_point_slabs).  The arrays keep their full
 * shape; cells outside the slab are neither read for the update nor written.
 */
int cbet_gain_field_slab(double *fields, const double *ne3d, double *gain, double *scratch, double *change,
                         int hx_lo, int hx_hi, const cbet_params *p, const cbet_gain_params *g,
                         cbet_context *ctx, void *stream);
/*
 * cbet_gain_field_slab on SLAB-PACKED arrays: fields [4][nbeams][slab] and gain [nbeams][slab] hold only
 * the planes [hx_lo, hx_hi) of every beam's haloed grid (slab = (hx_hi - hx_lo)(ny+2)(nz+2) doubles per beam and
 * component) -- what one rank of the slab-owned loop stores: all beams over its own x-slab.
 */
int cbet_gain_field_packed(double *fields, const double *ne3d, double *gain, double *scratch, double *change,
                         int hx_lo, int hx_hi, const cbet_params *p, const cbet_gain_params *g,
                         cbet_context *ctx, void *stream);
/* ---- flow table: the gain kernels on a perturbed target ------------------- */
/*
 * By default both gain kernels compute the flow u of a cell in closed form about the ORIGIN (the radial ramp above, from
 * the cell's node).  A context can instead hold a FLOW TABLE, double [3][nx][ny][nz] on the device, component-major
 * (ux, then uy, then uz, each in ne3d's node order): every entry that updates the gain with that context --
 * cbet_gain_field, cbet_gain_field_slab, cbet_gain_field_packed -- then reads u of a cell from the table at the cell's
 * (clamped) node and evaluates nothing of the ramp.  The trace kernels only gather the gain and need nothing.
 *
 * cbet_tabulate_flow fills the table with the ramp's flow on a perturbed target (cbet_target; NULL = the sphere about the
 * origin).  Model, for node (i, j, k), every statement ONE IEEE fp64 operation per written operator, in the written order,
 * no fused multiply-add; the first five lines are cbet_tabulate_target's, the rest the gain kernels' own ramp:
 *     xc = i*dx + xmin  (y, z alike)
 *     sx = xc - ox,  sy = yc - oy,  sz = zc - oz
 *     rho   = sqrt(sx*sx + sy*sy + sz*sz)
 *     q     = 1.0 + delta,  delta = sum_c c[c] Y_c(s / rho)       (cbet_tabulate_target's recurrence, factors and order)
 *     rho'  = rho if q == 1.0, else rho / q
 *     t     = (rho' - mach_r0) / (mach_r1 - mach_r0),  clamped to [0, 1]   (t < 0 -> 0, then t > 1 -> 1)
 *     um    = (mach_0 + (mach_1 - mach_0) * t) * cs               (cs of cbet_gain_constants)
 *     ux = um * (sx / rho),  uy = um * (sy / rho),  uz = um * (sz / rho);   u = 0 where rho == 0
 * The Mach number follows the distorted iso-surfaces (rho'), the DIRECTION stays radial from the target's centre o: tilting
 * the flow to the normal of the distorted surface is out of scope.
 * Limits and refusals: cbet_tabulate_target's (lmax, finite values, sum |c| sqrt((2l+1)/(4 pi)) < 1) and the gain
 * parameters' (as cbet_gain_field), CBET_EINVAL before any device work.
 * Identity: with o = 0 and all c = 0 every statement is the closed-form ramp's own in its order (x - 0 and the skipped
 * division are exact), so a gain update with that table selected gives, bit for bit, the update with none.
 *
 * cbet_tabulate_flow: fills the context's OWN table and selects it.  The FIRST call on a context allocates the table
 * (3 nx ny nz doubles) and is therefore not graph-capturable; every later call only enqueues the kernel on `stream` (no
 * allocation, no synchronisation).  The target's host arrays and the gain parameters are captured at the call.
 * cbet_context_set_flow: selects a CALLER's device table of the same layout (e.g. a hydro code's 3-D flow field); the
 * caller keeps it alive and unchanged while gain updates that read it are in flight.  NULL = back to the closed-form ramp
 * (the context's own table stays allocated).  Host-side state only: it applies to launches made after it.
 * cbet_context_flow: *out = the table in use, NULL if none (for tests).
 * cbet_flow_table: the host twin of cbet_tabulate_flow, plain loops in node order: HOST out of 3 nx ny nz doubles.
 * cbet_cbet_solve tabulates the radial plasma about the origin itself and returns CBET_EINVAL for a context that has a
 * flow table selected, rather than mixing the two models; the loop above the C ABI (tracer.cbet_solve) runs on a target.
 */
int cbet_tabulate_flow(cbet_context *ctx, const cbet_params *p, const cbet_gain_params *g,
                       const cbet_target *target /* NULL = sphere about the origin */, void *stream);
int cbet_context_set_flow(cbet_context *ctx, const double *flow);
int cbet_context_flow(cbet_context *ctx, void **out);
int cbet_flow_table(const cbet_params *p, const cbet_gain_params *g, const cbet_target *target, double *out);

/* ---- hydro-mesh plasma: node tables and flow from a spherical-polar state -- */
/*
 * The producer of node tables and of the flow table for a plasma that is the state of a hydrodynamics run rather than
 * one radial profile: ne, Te and the fluid velocity on a spherical-polar mesh (r, theta, phi) about a centre o, 1-D, 2-D
 * axisymmetric or 3-D.
 *
 * Mesh.  Node coordinates r[nr] strictly ascending, r[0] >= 0, nr >= 2; theta[ntheta] strictly ascending in [0, pi],
 * ntheta >= 1; phi[nphi] strictly ascending, -pi <= phi[0] < pi, phi[nphi-1] < phi[0] + 2 pi, nphi >= 1;
 * nr + ntheta + nphi <= CBET_MESH_MAX_COORDS.  Fields [nr][ntheta][nphi], phi fastest: ne (cm^-3, >= 0), te (the
 * profile's units, > 0) and optionally ur, uth, uph (cm/s; a NULL component is zero).  ntheta == 1 or nphi == 1: the
 * state does not depend on that angle (its one coordinate value is not used).
 *
 * Model, for node (i, j, k); every statement ONE IEEE fp64 operation per written operator, in the written order, no fused
 * multiply-add; TWO_PI is the literal 6.283185307179586:
 *     xc = i*dx + xmin (y, z alike);  sx = xc - ox,  sy = yc - oy,  sz = zc - oz       (cbet_tabulate_target's statements)
 *     rho = sqrt(sx*sx + sy*sy + sz*sz);   rxy = sqrt(sx*sx + sy*sy)
 *     theta = atan2(rxy, sz)                                                     (skipped when ntheta == 1)
 *     phi   = atan2(sy, sx);  if (phi < phi[0]) phi = phi + TWO_PI               (skipped when nphi == 1)
 * theta bracket: clamped like the profile lookup of cbet_tabulate_plasma -- at or below theta[0] the first row alone, at
 * or above the last the last row alone, else the bisection's j with wt = (theta - theta[j]) / (theta[j+1] - theta[j]).
 * phi bracket, periodic: k = the last index with phi[k] <= phi; for k < nphi - 1 the upper node is k + 1 and
 * wp = (phi - phi[k]) / (phi[k+1] - phi[k]); for k = nphi - 1 the upper node is 0 and
 * wp = (phi - phi[k]) / ((phi[0] + TWO_PI) - phi[k]); wp is clamped to [0, 1] (wp < 0 -> 0, then wp > 1 -> 1).
 * r bracket: cbet_tabulate_plasma's tests and bisection on rho: one clamped shell, or the pair m, m + 1.
 * A field f, the angles first on each shell that is used, the radius last:
 *     a0 = f[s][j][k] + (f[s][j][k'] - f[s][j][k]) * wp,   a1 = the same on row j'
 *     v(s) = a0 + (a1 - a0) * wt                                                 (a clamped theta: v(s) = a0)
 *     f = v(m) + (v(m+1) - v(m)) / (r[m+1] - r[m]) * (rho - r[m])                (a clamped rho: f = v(0) or v(nr-1))
 * For a field that does not depend on the angles v(s) is f[s] exactly, the last statement is cbet_tabulate_plasma's, and
 * the tables equal cbet_tabulate_plasma's (centre 0) / cbet_tabulate_target's (offset = centre, no coefficients) bit for bit.
 * kappa from the interpolated ne and Te: cbet_tabulate_plasma's three statements (launch_ray_XZ.cu:299-305).
 * Velocity: ct = sz/rho, st = rxy/rho, (c1, s1) = (sx/rxy, sy/rxy), (1, 0) where rxy == 0; with the interpolated components
 *     h = ur*st + uth*ct;   ux = h*c1 - uph*s1;   uy = h*s1 + uph*c1;   uz = ur*ct - uth*st;     u = 0 where rho == 0
 * Degenerate nodes: atan2(0, 0) is 0 (host and device), so a node at the centre reads the brackets of theta = 0 and
 * phi = 0 on the innermost shell, and a node on the polar axis those of phi = 0 (with theta = 0 or pi).
 * The device and the host evaluate atan2 with different functions: a node that lies on a bracket's edge may be put into
 * the neighbouring bracket by one of them.  The interpolant is continuous there, so the two sides agree to rounding (the
 * project's bound for two formulations of one quantity, 1e-12 relative), and bit for bit for angle-independent fields.
 * Every index the searches produce lies inside its array whatever the coordinates hold: the device entries, which cannot
 * read a device mesh, check sizes and NULL pointers only, and a bad mesh gives wrong numbers, never a read out of range.
 *
 * cbet_tabulate_mesh: DEVICE mesh arrays -> the context's ne3d / kappa3d; behaves towards the context exactly like
 * cbet_tabulate_target (geometry check, enqueued on `stream`, no allocation, no synchronisation, step records stale).
 * cbet_tabulate_mesh_flow: DEVICE mesh arrays -> the context's OWN flow table, which it selects; behaves exactly like
 * cbet_tabulate_flow (the first call on a context allocates; later calls only enqueue).
 * The struct is captured at the call; the arrays it points to are read when the kernel runs.
 * cbet_mesh_tables / cbet_mesh_flow_table: the host twins, plain loops in node order over HOST mesh arrays into HOST
 * ne3d / kappa3d (nx ny nz doubles each) / flow (3 nx ny nz doubles).  They validate the WHOLE mesh first -- cbet_mesh_check:
 * the rules under "Mesh" above and finite values everywhere -- and return CBET_EINVAL naming the first offence.
 */
#define CBET_MESH_MAX_COORDS 2560
typedef struct cbet_mesh {
    double center[3];                       /* o (cm)                                                             */
    int nr, ntheta, nphi;
    const double *r, *theta, *phi;          /* node coordinates                                                   */
    const double *ne, *te;                  /* [nr][ntheta][nphi]                                                 */
    const double *ur, *uth, *uph;           /* the same shape; each may be NULL = zero                            */
} cbet_mesh;
int cbet_tabulate_mesh(cbet_context *ctx, const cbet_params *p, const cbet_mesh *mesh /* device pointers */, void *stream);
int cbet_tabulate_mesh_flow(cbet_context *ctx, const cbet_params *p, const cbet_mesh *mesh /* device pointers */,
                            void *stream);
int cbet_mesh_check(const cbet_mesh *mesh /* host pointers */);
int cbet_mesh_tables(const cbet_params *p, const cbet_mesh *mesh /* host pointers */, double *ne3d, double *kappa3d);
int cbet_mesh_flow_table(const cbet_params *p, const cbet_mesh *mesh /* host pointers */, double *flow);

/* ---- local plasma state of the gain kernels -------------------------------------------- */
/*
 * By default both gain kernels take the sound speed cs and the prefactor gain_const from cbet_gain_constants: ONE Te, Ti
 * and Z for the whole plasma (cbet_gain_params.te_ev, ti_ev, z_ion).  A context can instead hold a STATE TABLE,
 * double [2][nx][ny][nz] on the device, component-major in ne3d's node order: component 0 is cs (cm/s), component 1 is
 * gain_const.  Every entry that updates the gain with that context -- cbet_gain_field, cbet_gain_field_slab,
 * cbet_gain_field_packed -- then reads both values at the cell's (clamped) node, the node it takes ne3d and the flow from,
 * and uses them wherever the scalars stand otherwise: in eta's denominator |k_j - k_i| cs + 1e-10 and in the cell's
 * prefactor gain_const (ne/ncrit) (1/iaw) / sqrt(1 - ne/ncrit).
 * What stays uniform: iaw, mi_over_me and the Mach ramp's parameters.  The closed-form ramp of the gain kernels and
 * cbet_tabulate_flow keep multiplying the Mach number with the SCALAR cs of cbet_gain_constants, with a state table selected
 * too: a caller who wants the local state throughout supplies the flow as well (cbet_tabulate_mesh_flow,
 * cbet_context_set_flow).  The trace kernels only gather the gain and need nothing.
 *
 * Model, for a node with Te = te, Ti = ti (both eV) and mean charge z; every written operator ONE IEEE fp64 operation in the
 * written order, no fused multiply-add (csrc/cbet_state_model.h, compiled by the kernel and by the host twin):
 *     te_k = te * 11604.5052;   ti_k = ti * 11604.5052
 *     c1   = E2 / ((A * te_k) * (1 + 3 * ti_k / (z * te_k)))
 *     gc   = c1 * F                                                  (component 1)
 *     cs   = 1e2 * sqrt(kEc * (z * te + 3.0 * ti) / mi_kg)           (component 0)
 * with E2 = pow(estat, 2), A = 4 * (1.0e3 * kMe) * kC * omega * kb (left to right), F = 8.0 * M_PI * 1.0e7 / kC and
 * mi_kg = mi_over_me * kMe, all four computed once on the host exactly as cbet_gain_constants computes them.
 * Identity: with te = te_ev, ti = ti_ev and z = z_ion at every node the table holds cbet_gain_constants' cs and gain_const
 * bit for bit, and a gain update with that table selected gives, bit for bit, the update with none.
 *
 * Producer from the hydro mesh: te is the mesh's (cbet_mesh.te, which must be in eV for the state to mean anything), ti and
 * z come from cbet_mesh_ions, each array of the mesh's shape or NULL = cbet_gain_params.ti_ev / z_ion everywhere (ions
 * NULL: both).  The three are interpolated with the mesh's own statement (phi, then theta, r last), then the model above.
 * cbet_tabulate_mesh_state: DEVICE arrays -> the context's OWN state table, which it selects; behaves exactly like
 * cbet_tabulate_mesh_flow: the FIRST call on a context allocates the table (2 nx ny nz doubles: 268 MB at 256^3) and is
 * not graph-capturable, every later call only enqueues the kernel on `stream` (no allocation, no synchronisation).  It
 * checks sizes, NULL pointers and the gain parameters only.
 * cbet_context_set_state: selects a CALLER's device table of the layout above; the caller keeps it alive and unchanged while
 * gain updates that read it are in flight.  NULL = back to the scalars (the context's own table stays allocated).
 * Host-side state only: it applies to launches made after it.
 * cbet_context_state: *out = the table in use, NULL if none (for tests).
 * cbet_mesh_state_table: the host twin, plain loops in node order over HOST arrays into HOST out of 2 nx ny nz doubles.
 * It validates the whole mesh first (cbet_mesh_check's rules), then ti (finite, >= 0) and zbar (finite, > 0), and returns
 * CBET_EINVAL naming the first offence.
 * cbet_cbet_solve takes cs and gain_const from its gain parameters and returns CBET_EINVAL for a context that has a state
 * table selected, as it does for a selected flow; the loop above the C ABI (tracer.cbet_solve) runs with both.
 */
typedef struct cbet_mesh_ions {
    const double *ti;    /* [nr][ntheta][nphi] eV, or NULL: cbet_gain_params.ti_ev everywhere */
    const double *zbar;  /* same shape, or NULL: cbet_gain_params.z_ion everywhere */
} cbet_mesh_ions;
int cbet_tabulate_mesh_state(cbet_context *ctx, const cbet_params *p, const cbet_gain_params *g,
                             const cbet_mesh *mesh /* device pointers */, const cbet_mesh_ions *ions /* device pointers; may be NULL */,
                             void *stream);
int cbet_context_set_state(cbet_context *ctx, const double *state);
int cbet_context_state(cbet_context *ctx, void **out);
int cbet_mesh_state_table(const cbet_params *p, const cbet_gain_params *g, const cbet_mesh *mesh /* host pointers */,
                          const cbet_mesh_ions *ions /* host pointers; may be NULL */, double *out);
/*
 * The sparse exchange of the slab-owned CBET loop (tracer._Exchanger).  A segment is a 64-byte run of 8 doubles aligned
 * to 8 along z; `segments` is a DEVICE array of nseg {row of the array (beam), index of the run inside one beam's
 * [planes][hy][ceil(hz / 8)] run grid} int pairs.  pack: out[8 i .. 8 i + 8) = the i-th run of `src` (rows are
 * beam_stride doubles apart, a row is [planes][hy][hz]; entries beyond the end of a z-row are written as 0);
 * unpack: the inverse scatter (entries beyond the end of a z-row are dropped).  Stream-ordered, no synchronisation.
 */
int cbet_pack_segments(const double *src, long beam_stride, int hy, int hz, const int *segments, long nseg, double *out,
                       void *stream);
int cbet_unpack_segments(double *dst, long beam_stride, int hy, int hz, const int *segments, long nseg, const double *in,
                         void *stream);
/*
 * Device bytes one rank of the slab-owned CBET loop (tracer.cbet_fixed_point_slabs) needs beside the node tables:
 * its own beams' four field components and gain over the whole grid and all beams' fields and gain over its x-slab.
 * The dense exchanges need NO staging: a beam's part over a slab is contiguous in both layouts, so every message is
 * sent from and received into the arrays themselves (one message per beam, peer and component; all peers of a beam
 * in one grouped send/recv).  `_parts`: the rank holds own_beams beams and own_planes planes -- the slabs are cut by
 * gain-update WORK (the central planes, where the beams cross, are the expensive ones), so the outer ranks hold more
 * planes than (nx+2) / W -- plus staging_doubles of exchange staging (0; the optional sparse exchange packs its runs).
 * cbet_cbet_slab_workspace_bytes(p, W, rank): the same with the equal cut of beams and planes (a lower bound for the outer
 * ranks of a balanced cut).  0 on bad arguments.  (512^3, 60 beams, 8 ranks, equal cut: ~86 GB per rank; every rank
 * holding everything, cbet_cbet_workspace_bytes, would be 391 GB.)
 */
size_t cbet_cbet_slab_workspace_bytes(const cbet_params *p, int world_size, int rank);
size_t cbet_cbet_slab_workspace_bytes_parts(const cbet_params *p, int own_beams, int own_planes, size_t staging_doubles);
/* Bytes of device workspace cbet_cbet_solve needs: 5 nbeams (n+2)^3 doubles (four field components + gain) + a few scalars. */
size_t cbet_cbet_workspace_bytes(const cbet_params *p);
/*
 * The whole iteration on the current device: tabulate the plasma; repeat { field pass with the
 * current gain -> normalise -> new gain } until converged; then one deposition pass with the
 * converged gain ADDED into edep (device, (n+2)^3).  Profiles and tables are device pointers as for
 * cbet_launch_ray_XYZ.  workspace: device memory of cbet_cbet_workspace_bytes() or NULL (allocated
 * and freed inside).  Honours shard_index / shard_count only with shard_count == 1 (the multi-rank
 * loop lives above the C ABI: tracer.cbet_solve all-reduces the fields between passes).
 * Synchronises the stream once per pass (it reads the convergence scalars).
 */
int cbet_cbet_solve(double *te_data_g, double *r_data_g, double *ne_data_g, double *edep,
                    double *bbeam_norm, double *beam_norm, double *pow_r, double *phase_r,
                    const cbet_params *p, const cbet_gain_params *g, void *workspace,
                    cbet_context *ctx, void *stream, cbet_cbet_report *report);
/*
 * The converged gain inside a workspace that cbet_cbet_solve has run in: device [nbeams][(nx+2)(ny+2)(nz+2)]
 * doubles at a fixed offset of `workspace` (the four field components come first).  Valid after the solve
 * returns, until the workspace is reused; pass it to cbet_trace_exits to see where the light of that solve went.
 * NULL on bad arguments.
 */
const double *cbet_cbet_workspace_gain(const cbet_params *p, const void *workspace);

/* ---- saturation of the ion-acoustic wave --------------------------------------------------- */
/*
 * The pair gain G_ij = pref P(eta_ij) of the gain kernels is linear: nothing in it limits the ion-acoustic grating a beam
 * pair drives.  (cbet_gain_params.max_exponent is a numerical clamp of the TRACE kernels on |K ds| per ray step; it does not
 * act on the pair gains and is not symmetric between the two beams of a pair.)  A context can hold a limit dn_max > 0 on
 * the grating's relative amplitude.  Scattering off a grating of amplitude dn/n exchanges intensity at the rate
 * kap (dn/n) sqrt(Ii Ij), kap = (k0 / 2) frac / sqrt(eps) with k0 = omega / c, frac = ne / ncrit, eps = 1 - frac; so
 *     A_ij = |G_ij| sqrt(Ii Ij) / kap                       (dimensionless: G I and kap are both 1/cm)
 * is the amplitude this model's gain corresponds to -- no more than that: the model's parity is unpinned (DESIGN.md section
 * 9).  With a limit every pair gain becomes G_ij min(1, dn_max / A_ij).  The factor is the same for (i, j) and (j, i): G
 * stays antisymmetric and a cell's exchange sum_i I_i K_i still cancels.
 *
 * The ordered kernel, every written operator ONE IEEE fp64 operation in the written order, no fused multiply-add:
 *     per cell:  kap = ((0.5 * k0) * frac) / rt             (rt = sqrt(eps), eps > 0;  kap = 0 otherwise)
 *                lim = dn_max * kap
 *     per pair:  g = pref * P
 *                w = fabs(g) * sqrt(Ii * Ij)
 *                if (w > lim) g = g * (lim / w)
 *                acc += g * Ij
 * A pair that does not reach the limit keeps its bits (the update without a limit adds (pref * P) * Ij).  With a state table
 * pref holds the node's gain_const, as without a limit.  The pair-once kernel applies ONE factor per unordered pair to its
 * pair function's value before both addends, comparing squares and scaling by lim rsqrt(w^2) from the hardware estimate
 * (measured: K_i within 4.9 units of 2^-53 S_i of a 200-bit model where the ordered statements reach 4.7 -- S_i the
 * condition-aware scale of DESIGN.md section 9, "Per-pair accuracy"); where the limit is not reached the value is untouched.
 *
 * cbet_context_set_saturation: dn_max > 0 sets the limit, 0 = none (a new context's default); negative, NaN or infinite:
 * CBET_EINVAL naming the offence.  Host-side state only, like cbet_context_set_state: it applies to launches made after it.
 * Every entry that updates the gain with that context honours it -- cbet_gain_field, cbet_gain_field_slab,
 * cbet_gain_field_packed, and cbet_cbet_solve with a caller's context (the limit is uniform: the solve does not refuse it;
 * with ctx == NULL it runs without one).
 * cbet_context_saturation: *out = the limit in use, 0 if none.
 * cbet_pair_amplitude: the map of the UNCLAMPED amplitude.  `fields` are NORMALISED whole-grid device fields
 * [4][nbeams][hsize] (I, kx, ky, kz), as a gain update without `consume` leaves them; `amp` is [hsize] device doubles,
 * whole-grid storage.  For every cell of the planes [hx_lo, hx_hi) it writes max over i < j of A_ij by the statements above
 * (the largest w, divided by kap), 0 where fewer than two beams are present, where no present pair has k_i != k_j, or where
 * kap = 0; other planes are not written.  It reads the context's flow and state tables like the gain kernels (ne3d NULL:
 * the context's), ignores the context's dn_max and changes neither `fields` nor any gain.  Stream-ordered.
 */
int cbet_context_set_saturation(cbet_context *ctx, double dn_max);
int cbet_context_saturation(cbet_context *ctx, double *out);
int cbet_pair_amplitude(const double *fields, const double *ne3d, double *amp, int hx_lo, int hx_hi, const cbet_params *p,
                        const cbet_gain_params *g, cbet_context *ctx, void *stream);

/* ---- pairwise exchange matrix ------------------------------------------------------------- */
/*
 * Which beam feeds which, and how much.  For a cell of the haloed deposit grid and beams i != j both present there
 * (I_i > 0, I_j > 0, k_i != k_j, eps > 0), with the NORMALISED fields (I, kx, ky, kz) a gain update leaves:
 *     x_ij(cell) = ((ds_node * g_ij) * I_i) * I_j           ds_node = (c * rt) * dt, the divisor of the normalisation
 * g_ij is the cell's pair gain exactly as the gain kernels form it, pref * P(eta_ij) with q = k_j - k_i: it reads the
 * context's flow table and state table if selected, and it is scaled by min(1, lim / w) when the context holds a saturation
 * limit -- unlike cbet_pair_amplitude the matrix HONOURS dn_max, because it decomposes the K that the solve uses.
 *     T[i][j]     = sum over cells of x_ij     the energy beam i gains from beam j per field pass, in beam_gain's units;
 *                                              T[j][i] = -T[i][j] and T[i][i] = 0
 *     Gross[i][j] = sum over cells of |x_ij|   symmetric; the scale a tolerance on T[i][j] is taken against
 * Identity: sum_j T[i][j] = sum over cells of ds_node * I_i * K_i, K the unrelaxed sum of the gain kernels.
 *
 * cbet_exchange_matrix: `fields` are NORMALISED whole-grid device fields [4][nbeams][hsize] under cbet_pair_amplitude's
 * contract, never written; the planes [hx_lo, hx_hi) are covered.  `out` is device [nbeams][nbeams]: its upper triangle is
 * ADDED into (slabs and ranks sum; the caller zeroes it before the first call), its lower triangle is rewritten as the
 * negated upper one and its diagonal as 0.  `gross` is the same shape (upper triangle added into, lower mirrored, diagonal
 * 0), or NULL.  ne3d NULL = the context's table.  Stream-ordered, no synchronisation, no allocation.
 * Every unordered pair is evaluated once per cell with the pair-once gain kernel's pair function (and its clamp): the
 * arithmetic of the kernel cbet_cbet_solve runs, per pair within 5.7 units of 2^-53 S of a 200-bit model where the ordered
 * statements stay within 4.7 ("Per-pair accuracy").  Per-workgroup partial
 * tables are written to `work` and summed in workgroup order by a second kernel: no floating-point atomics, so two calls on
 * the same inputs give the same bits, on any device -- the number of workgroups is min(rows, CBET_EXCHANGE_MAX_GROUPS) with
 * rows = (hx_hi - hx_lo) (ny + 2), never the device's size.  `work` holds [groups][2][nbeams (nbeams - 1) / 2] doubles;
 * cbet_exchange_matrix_work_bytes(p) is the size for the whole grid, enough for any slab: at most 768 x 2 x 2016 doubles =
 * 24.8 MB (0 for one beam or bad parameters).
 * CBET_EINVAL naming the offence: nbeams > CBET_MAX_CBET_BEAMS, a slab outside [0, nx + 2] or reversed, NULL fields, out
 * or work.  With nbeams == 1 nothing is launched and `out` keeps the caller's zeros; an empty slab changes nothing.
 *
 * cbet_exchange_matrix_host: the host twin and the reference of the device path at any size.  HOST pointers; no context:
 * ne3d [nx][ny][nz] (required), flow [3][nx][ny][nz] or NULL = the closed-form ramp about the origin, state [2][nx][ny][nz]
 * or NULL = cbet_gain_constants' scalars, dn_max (0 = none) explicit.  It runs the ORDERED kernel's statements, one IEEE
 * operation per written operator (the statements of DESIGN.md sections 9 and 17), cells in index order, every pair's two
 * sums compensated (Neumaier), and makes no HIP call.  out / gross as above.
 */
#define CBET_EXCHANGE_MAX_GROUPS 768
size_t cbet_exchange_matrix_work_bytes(const cbet_params *p);
int cbet_exchange_matrix(const double *fields, const double *ne3d, double *out, double *gross, void *work, int hx_lo, int hx_hi,
                         const cbet_params *p, const cbet_gain_params *g, cbet_context *ctx, void *stream);
int cbet_exchange_matrix_host(const double *fields, const double *ne3d, double *out, double *gross, int hx_lo, int hx_hi,
                              const cbet_params *p, const cbet_gain_params *g, const double *flow, const double *state,
                              double dn_max);

/* ---- wavelength detuning ------------------------------------------------------------------ */
/*
 * Per-beam frequency shifts in the gain stage.  Beam b has the angular frequency omega + w_b, omega the nominal one of
 * cbet_derive and w_b in rad/s (a wavelength shift dl of the nominal l0 = 2 pi c / omega is w = omega l0 / (l0 + dl) - omega:
 * a red shift, dl > 0, is a negative w).  The ion-acoustic wave of the ordered pair (i, j), q = k_j - k_i, is driven at the
 * beat frequency, so the resonance of the pair gain G_ij = pref P(eta_ij) becomes
 *     eta_ij = ((0.0 - (qx*ux + qy*uy + qz*uz)) + (w_j - w_i)) / (kiaw*cs + 1e-10)
 * in the ordered kernel -- every written operator ONE IEEE fp64 operation in the written order, no fused multiply-add --
 * and N = -(q . u) + (w_j - w_i) in the pair function of the pair-once kernels (measured: both within 4.3 units of 2^-53 S of
 * a 200-bit model, as without shifts: DESIGN.md section 9, "Per-pair accuracy").
 * Identities: beam i gains where its frequency in the plasma frame is the lower one, so in still plasma the red-shifted beam
 * gains; (w_i - w_j) = -(w_j - w_i) exactly, so G_ji = -G_ij stays exact and a cell's exchange sum_i I_i K_i still cancels,
 * with or without a saturation limit; equal shifts add an exact zero and give the bits of no shifts; two exactly parallel
 * beams exchange nothing whatever their colours (the pair-once kernels count the beat frequency only where q != 0).
 * Out of scope: only the beat frequency enters.  Each beam's own k0, ncrit and refraction keep the nominal wavelength (the
 * relative change is ~1e-3 at +-3 Angstrom of 351 nm), and the Manley-Rowe photon-number correction of the same order is
 * left out.  The trace kernels only gather K and do not see the shifts.
 *
 * cbet_context_set_detuning: domega[nbeams] HOST doubles.  NULL, or all shifts equal to the first, selects none (a new
 * context's default); otherwise the values are copied to a device table of CBET_MAX_CBET_BEAMS doubles that the context owns
 * (the first such call allocates it).  The call synchronises `stream` before it overwrites the table and copies
 * synchronously: a SET-UP call, not capturable in a graph, and launches on other streams that still read the table are the
 * caller's to wait for.  It applies to launches made after it.  CBET_EINVAL naming the offence: a NaN or infinite shift,
 * nbeams above CBET_MAX_CBET_BEAMS or below 1, nbeams different from the context's parameters, a NULL context; a refused call
 * changes nothing.  Every entry that builds its gain arguments from that context honours the shifts -- cbet_gain_field,
 * cbet_gain_field_slab, cbet_gain_field_packed, cbet_pair_amplitude (the amplitude is the detuned |G_ij|'s),
 * cbet_exchange_matrix, and cbet_cbet_solve with a caller's context; with ctx == NULL the solve runs without shifts.
 * cbet_context_detuning: *nbeams = the number of shifts in use, 0 for none, and out[0 .. *nbeams) = their values (out holds
 * CBET_MAX_CBET_BEAMS doubles, or is NULL to ask for the count alone).
 * cbet_exchange_matrix_host_shifted: cbet_exchange_matrix_host with shift[nbeams] HOST doubles or NULL: the ordered
 * statements with the beat frequency, compensated sums as there.  cbet_exchange_matrix_host calls it with NULL.
 */
int cbet_context_set_detuning(cbet_context *ctx, const double *domega, int nbeams, void *stream);
int cbet_context_detuning(cbet_context *ctx, double *out, int *nbeams);
int cbet_exchange_matrix_host_shifted(const double *fields, const double *ne3d, double *out, double *gross, int hx_lo, int hx_hi,
                                      const cbet_params *p, const cbet_gain_params *g, const double *flow, const double *state,
                                      double dn_max, const double *shift);

/* ---- polarization smoothing --------------------------------------------------------------- */
/*
 * How the beams are polarized in the gain stage.  CBET_POL_ALIGNED (0, a new context's default): every pair of beams is
 * polarized alike and the pair gain is G_ij = pref P(eta_ij), as in the sections above.  CBET_POL_SMOOTHED (1): every beam is
 * an equal, incoherent mix of two orthogonal polarizations -- a distributed polarization rotator on every beam, as on
 * OMEGA -- and two such beams crossing at the angle theta exchange (1 + cos^2 theta) / 4 of the aligned value.  In a cell a
 * present pair has |k_i| = |k_j| = kmag = k0 sqrt(eps), the value the normalisation wrote, and the ordered kernel runs
 *     cth = ((k_i.x*k_j.x + k_i.y*k_j.y) + k_i.z*k_j.z) / (kmag*kmag)
 *     f   = 0.25 * (1.0 + cth*cth)
 *     g   = (pref * P(eta_ij)) * f
 * -- every written operator ONE IEEE fp64 operation in the written order, no fused multiply-add -- while the pair-once
 * kernels form cth = 1 - |k_j - k_i|^2 / (2 kmag^2) from the |q|^2 they hold (measured: within 5.7 units of 2^-53 S of a
 * 200-bit model, the ordered statements within 3.9: DESIGN.md section 9, "Per-pair accuracy").
 * Identities: 1/4 <= f <= 1/2, exactly 1/4 for beams at right angles and 1/2 for parallel or opposed ones; f is the same bits
 * for (i, j) and (j, i), so G_ji = -G_ij stays exact and a cell's exchange sum_i I_i K_i still cancels, with or without a
 * saturation limit; eta is untouched, so detuning composes unchanged; which pairs are present is unchanged.
 * The model's choice: f multiplies the gain BEFORE the saturation clamp.  The clamp, cbet_pair_amplitude and the exchange
 * matrix see f G_ij, and the ion-acoustic amplitude reported is that of the pair's total exchange, not of the s-s and p-p
 * gratings separately.
 * Out of scope: linearly polarized beams with per-beam polarization vectors (the factor would be (e_i . e_j)^2), the spatial
 * offset between a rotator's two sub-beams, and the trace kernels, which only gather K.  The mode is an int so that a later
 * mode needs no new entry point.
 *
 * cbet_context_set_polarization: a SET-UP call like cbet_context_set_detuning, it applies to launches made after it (no
 * device work, no synchronisation).  CBET_EINVAL naming the offence: a mode that is neither of the two, a NULL context; a
 * refused call changes nothing.  Every entry that builds its gain arguments from that context honours the mode --
 * cbet_gain_field, cbet_gain_field_slab, cbet_gain_field_packed, cbet_pair_amplitude (the amplitude is the smoothed
 * |G_ij|'s), cbet_exchange_matrix, and cbet_cbet_solve with a caller's context; with ctx == NULL the solve runs aligned.
 * cbet_context_polarization: *mode = the mode in use.
 * cbet_exchange_matrix_host_polarized: cbet_exchange_matrix_host_shifted with a mode: the ordered statements above,
 * compensated sums as there; an unknown mode is CBET_EINVAL.  cbet_exchange_matrix_host_shifted calls it with
 * CBET_POL_ALIGNED.
 */
#define CBET_POL_ALIGNED 0
#define CBET_POL_SMOOTHED 1
int cbet_context_set_polarization(cbet_context *ctx, int mode);
int cbet_context_polarization(cbet_context *ctx, int *mode);
int cbet_exchange_matrix_host_polarized(const double *fields, const double *ne3d, double *out, double *gross, int hx_lo, int hx_hi,
                                        const cbet_params *p, const cbet_gain_params *g, const double *flow, const double *state,
                                        double dn_max, const double *shift, int pol);

/* ---- laser bandwidth ------------------------------------------------------------------------ */
/*
 * A line spectrum in the gain stage.  Every beam carries the SAME spectrum about its own centre frequency omega + w_b (w_b the
 * shift of cbet_context_set_detuning): L <= CBET_MAX_BAND_LINES lines with offsets o_a in rad/s and weights p_a > 0, which the
 * library normalises to sum p_a = 1.  The lines are mutually incoherent -- the line spacing is taken to be far above the
 * ion-acoustic damping rate -- so line a of beam i and line b of beam j drive their own grating at the beat
 * (w_j - w_i) + (o_b - o_a), and the pair gain is
 *     G_ij = pref sum_a sum_b p_a p_b P((N + (o_b - o_a)) / D),    N = (0.0 - q . u) + (w_j - w_i),    D = kiaw*cs + 1e-10.
 * The spectrum is shared, so the double sum collapses onto its autocorrelation: a difference table of M <= L (L - 1) / 2
 * entries d_m > 0 with weights c_m = sum_{a < b, |o_b - o_a| = d_m} p_a p_b, and the centre weight c_0 = sum p_a^2.  The
 * ordered kernel runs
 *     S = c_0 * P(N / D)
 *     for m = 0 .. M-1:   S = S + c_m * (P((N + d_m) / D) + P((N - d_m) / D))
 *     g = pref * S        then the polarization factor, then the saturation clamp, as without a spectrum
 * -- every written operator ONE IEEE fp64 operation in the written order -- and the pair-once kernels the same sum with their
 * quotient form of P (measured with shifts, smoothing and a 3-line spectrum: within 4.2 units of 2^-53 S of a 200-bit model,
 * the ordered statements within 2.5: DESIGN.md section 9, "Per-pair accuracy").  The table is built deterministically: weights normalised by their sum in line
 * order; c_0 summed in line order; the differences |o_b - o_a| in fp64 for a < b in ascending order (a, then b); a zero
 * difference adds 2 p_a p_b to c_0; bitwise-equal differences are merged; the entries are sorted by d.
 * Identities: G_ji = -G_ij bit for bit (N -> -N and (-N + d) = -(N - d) exactly, P is odd, the bracket is one commutative
 * add), so a cell's exchange still cancels, with or without a limit; still plasma without shifts gives exactly zero under any
 * spectrum (N = 0 makes every bracket zero): bandwidth alone transfers nothing, it smears a resonance that flow or detuning
 * creates; M = 0 (no lines, one line, or all offsets equal) selects no spectrum at all and the bits of the sections above; two
 * exactly parallel beams exchange exactly nothing; far off resonance (d_m >> |q| cs) only the centre term survives and
 * G -> c_0 G_mono, 1/L for L equal lines.
 * The model's choices: the field model keeps ONE intensity per beam -- the spectral shape is not changed by the exchange, no
 * per-line depletion.  The saturation limit clamps the SUMMED pair gain, and cbet_pair_amplitude reports the amplitude of the
 * pair's total exchange, not of one line pair's grating (the choice of polarization smoothing).
 * Out of scope: per-beam spectra; per-line fields or depletion; coherent or FM (SSD phase-modulated) spectra; any effect on
 * refraction, ncrit or k0.  The trace kernels only gather K and do not see the spectrum.
 *
 * cbet_context_set_bandwidth: line_domega[nlines] and line_weight[nlines] HOST doubles.  nlines = 0, NULL arrays, one line or
 * offsets that are all equal select none (a new context's default); otherwise the difference table goes to a device block the
 * context owns (the first such call allocates it).  A SET-UP call like cbet_context_set_detuning: it synchronises `stream`
 * before it overwrites the table, copies synchronously, is not capturable in a graph, and applies to launches made after it.
 * CBET_EINVAL naming the offence, judged before the context (no device needed): a NaN or infinite offset, a weight that is not
 * finite and > 0, nlines < 0 or above CBET_MAX_BAND_LINES, one array NULL and the other not; then a NULL context.  A refused
 * call changes nothing.  Every entry that builds its gain arguments from that context honours the spectrum -- cbet_gain_field,
 * cbet_gain_field_slab, cbet_gain_field_packed, cbet_pair_amplitude, cbet_exchange_matrix, and cbet_cbet_solve with a caller's
 * context; with ctx == NULL the solve runs without one.
 * cbet_context_bandwidth: *nlines = the lines in use, 0 for none, and their offsets and NORMALISED weights in
 * line_domega / line_weight[0 .. *nlines) (each holds CBET_MAX_BAND_LINES doubles, or is NULL).
 * cbet_exchange_matrix_host_banded: cbet_exchange_matrix_host_polarized with lines (HOST arrays, the same refusals): the
 * ordered statements above on the same table, compensated sums as there.  The earlier twins call it with no lines.
 */
#define CBET_MAX_BAND_LINES 8
int cbet_context_set_bandwidth(cbet_context *ctx, const double *line_domega, const double *line_weight, int nlines, void *stream);
int cbet_context_bandwidth(cbet_context *ctx, double *line_domega, double *line_weight, int *nlines);
int cbet_exchange_matrix_host_banded(const double *fields, const double *ne3d, double *out, double *gross, int hx_lo, int hx_hi,
                                     const cbet_params *p, const cbet_gain_params *g, const double *flow, const double *state,
                                     double dn_max, const double *shift, int pol, const double *line_domega,
                                     const double *line_weight, int nlines);

/* ---- quarter-critical LPI maps ------------------------------------------------------------- */
/*
 * What the light that CBET redistributes does at quarter-critical density: per cell of the haloed deposit grid inside a band
 * of ne / ncrit, the overlapped intensity, the density scale length and the two-plasmon-decay threshold parameter.  No
 * reference counterpart: parity UNPINNED, like the whole CBET stage.  The statements are csrc/cbet_lpi_model.h's, one IEEE
 * fp64 operation per written operator, for the kernel and the host twin alike, so the two agree bit for bit.
 *
 * A cell takes its plasma from its clamped node (i, j, k), as the gain kernels' cells do.  frac = ne3d[node] / ncrit; the cell
 * is IN BAND iff frac_lo <= frac <= frac_hi.  A cell out of band holds 0.0 in every quantity and adds nothing to the summary.
 *     gradient   per axis (ne[c + p] - ne[c + m]) / (2.0 d), (m, p) = -+1 inside, (0, 2) and (n-3, n-1) on the faces (the
 *                tracer's own face rule); 0 along an axis of fewer than 3 nodes
 *     gn         sqrt(gx gx + gy gy + gz gz);   L_n = ne / gn in cm, 0 where gn == 0
 *     beam b     PRESENT iff I_b > 0 and kn_b = sqrt(kx kx + ky ky + kz kz) > 0; beams in increasing order, sums in that order
 *     I_sum, I_max, n_present     the sum, the maximum and the number of the present beams' intensities (W/cm^2)
 *     mu_b       ((kx gx + ky gy) + kz gz) / (kn_b gn), clamped to [-1, 1]; 1 for every beam where gn == 0
 *     bin_b      min(NB - 1, (int)((1.0 - mu_b) * (0.5 * NB))), NB = cone_bins
 *     I_cw       max over the bins of the sum of I_b in the bin (beam order): the largest overlapped intensity of beams on
 *                one cone about the density gradient, which can share a common electron-plasma wave.  NB = 1: I_cw == I_sum
 *     te         te3d[node] in eV, or te_ev where te3d is NULL
 *     T          ((L_n * 1e4) * lambda_um) / (81.86 * (te * 1e-3)), 0 where te <= 0 or L_n == 0: Simon et al., Phys. Fluids 26,
 *                3107 (1983), eta = I_14 L_um lambda_um / (81.86 T_keV) (I_14 L_um / (233 T_keV) at 351 nm); lambda_um is the
 *                vacuum wavelength 2 pi c / omega of cbet_derive in micrometres
 *     eta_x      (I_x * 1e-14) * T for x in {sum, cw, max}
 * The absolute-SRS threshold at n_c / 4 needs a 4/3 power and is not evaluated here (cbet_raytracing_3d_amd/lpi.py).
 *
 * `lpi` is [CBET_LPI_NQ][hsize] doubles, whole-grid storage per quantity (CBET_LPI_BAND ... CBET_LPI_ETA_CW).  Every cell of
 * the planes [hx_lo, hx_hi) is written in all seven quantities, so the caller need not clear; other planes are not touched.
 * `fields` are NORMALISED whole-grid fields [4][nbeams][hsize] (I, kx, ky, kz) under cbet_pair_amplitude's contract, never
 * written; fields and lpi need only a double's alignment.
 *
 * cbet_lpi_summary is MERGED INTO: counts and sums add, maxima take the maximum, argmax_cw (a haloed cell index) follows
 * max_eta_cw, the lowest index among ties -- slab calls and ranks compose.  cbet_lpi_summary_init zeroes one and sets
 * argmax_cw = -1 (host memory; a device summary is initialised by copying one).  lit_cells counts band cells with
 * n_present >= 1; above_x those with eta_x >= 1; sum_I_sum / band_cells is the band mean of I_sum.
 *
 * cbet_lpi_map: device pointers; ne3d NULL = the context's table, te3d NULL = te_ev everywhere.  summary may be NULL (no
 * reduction runs and `work` is not read); otherwise `work` holds cbet_lpi_work_bytes(p) bytes (enough for any slab; 0 for bad
 * parameters).  Bricks whose cells are all out of band are written as zeros without reading `fields`.  The reduction uses
 * no atomics: per-workgroup partial summaries go to `work` and a second kernel merges them in workgroup order, and the
 * number of workgroups follows from the slab alone, so two calls give the same bits on any device.  Stream-ordered, no
 * synchronisation, no allocation: capturable.  CBET_EINVAL naming the offence: NULL fields or lpi, a band that is not
 * 0 <= frac_lo <= frac_hi < 1, cone_bins outside 1 .. CBET_LPI_MAX_BINS, nbeams > CBET_MAX_CBET_BEAMS, te3d NULL with
 * te_ev <= 0, a summary without work, a slab outside [0, nx + 2] or reversed.
 * cbet_lpi_map_host: the host twin on HOST pointers (ne3d required), cells in index order, no HIP call.
 */
#define CBET_LPI_NQ 7
#define CBET_LPI_BAND 0
#define CBET_LPI_I_SUM 1
#define CBET_LPI_I_CW 2
#define CBET_LPI_I_MAX 3
#define CBET_LPI_LN 4
#define CBET_LPI_ETA_SUM 5
#define CBET_LPI_ETA_CW 6
#define CBET_LPI_MAX_BINS 16
#define CBET_LPI_MAX_GROUPS 8192
typedef struct cbet_lpi_summary {
    long long band_cells, lit_cells;
    long long above_max, above_cw, above_sum;
    long long argmax_cw;
    double max_eta_max, max_eta_cw, max_eta_sum;
    double sum_I_sum, sum_I_cw;
    int max_present, reserved;
} cbet_lpi_summary;
size_t cbet_lpi_work_bytes(const cbet_params *p);
int cbet_lpi_summary_init(cbet_lpi_summary *s);
int cbet_lpi_map(const double *fields, const double *ne3d, const double *te3d, double te_ev, double frac_lo, double frac_hi,
                 int cone_bins, double *lpi, cbet_lpi_summary *summary, void *work, int hx_lo, int hx_hi, const cbet_params *p,
                 cbet_context *ctx, void *stream);
int cbet_lpi_map_host(const double *fields, const double *ne3d, const double *te3d, double te_ev, double frac_lo,
                      double frac_hi, int cone_bins, double *lpi, cbet_lpi_summary *summary, int hx_lo, int hx_hi,
                      const cbet_params *p);

/* ---- exit pass --------------------------------------------------------------- */
/*
 * Where the light that is not absorbed goes.  A trajectory-only pass traces the rays of a deposit pass, deposits
 * nothing, and writes ONE record per ray when the ray ends: in the step where the reference's stop test
 * (launch_ray_XZ.cu:351-356) first holds, or after nt steps.
 */
#define CBET_RAY_LAUNCHED 1   /* slot holds a traced ray (0: idle lane of the bundle)                */
#define CBET_RAY_CUTOFF   2   /* uray <= 0.05 uray0 at the end (launch_ray_XZ.cu:351)                 */
#define CBET_RAY_ESCAPED  4   /* outside xmin - dx/2 ... zmax + dz/2 at the end (:352-354)            */
#define CBET_RAY_TIMEOUT  8   /* still inside and above the cutoff after nt steps                      */
typedef struct cbet_ray_exit {
    double x, y, z;       /* position after the last step (cm)                                        */
    double vx, vy, vz;    /* velocity after the last kick (cm/s)                                       */
    double uray;          /* energy the ray still carries                                              */
    double uray0;         /* launch energy (:113)                                                      */
    double gained;        /* CBET: energy gained on the way (0 without a gain grid)                    */
    int steps;            /* steps taken: the ray's share of cbet_counters.ray_steps                   */
    int status;           /* CBET_RAY_* bits; CUTOFF and ESCAPED may both be set                       */
} cbet_ray_exit;          /* 80 bytes */
#ifdef __cplusplus
static_assert(sizeof(cbet_ray_exit) == 80, "cbet_ray_exit is 80 bytes");
#else
_Static_assert(sizeof(cbet_ray_exit) == 80, "cbet_ray_exit is 80 bytes");
#endif

/* Columns of a cbet_exit_tally row. */
#define CBET_TALLY_COLUMNS 8
#define CBET_TALLY_LAUNCHED 0     /* sum of uray0                                                  */
#define CBET_TALLY_GAINED 1       /* sum of gained                                                 */
#define CBET_TALLY_ABSORBED 2     /* sum of (uray0 + gained - uray)                                */
#define CBET_TALLY_ESCAPED 3      /* sum of uray over rays with CBET_RAY_ESCAPED                   */
#define CBET_TALLY_STRANDED 4     /* ... over rays with CUTOFF and not ESCAPED                     */
#define CBET_TALLY_UNFINISHED 5   /* ... over rays with neither: the trace's TIMEOUT rays          */
#define CBET_TALLY_N_RAYS 6       /* records with CBET_RAY_LAUNCHED                                */
#define CBET_TALLY_N_ESCAPED 7    /* ... of those, ESCAPED                                         */

/*
 * The exit pass: cbet_trace_nodes's rays (same arguments, same beam range, shard_index / shard_count split and
 * grid_beam0 / grid_beams), no deposit.  exits: device [grid beams][L] records, L = cbet_context_list_length; the
 * record of launch-list entry li of beam b is exits[(b - grid_beam0) * L + li].  Slots of bundles this launch does not
 * trace are not written, so shards fill one buffer between them; an idle lane's slot gets a zero record.
 * ne3d / kappa3d NULL = the context's own tables (fill them first: cbet_tabulate_plasma).  gain: device
 * [grid beams][(nx+2)(ny+2)(nz+2)] gain coefficient, or NULL: with it every step applies the CBET hook of
 * cbet_trace_cbet (and g supplies max_exponent); when gain is NULL, g may be NULL too.  Absorbing mode only
 * (p->absorption == 1, else CBET_EINVAL): in bookkeeping mode the reference's increment is not an energy loss.
 * p->kernel_variant, per_beam_grids, edep_zpitch and window_stats do not apply.  Counts ray_steps and rays_traced
 * into the context's counters.  Enqueued on `stream`, no synchronisation (graph-capturable).
 */
int cbet_trace_exits(const double *ne3d, const double *kappa3d, const double *gain, cbet_ray_exit *exits,
                     const double *bbeam_norm, const double *beam_norm, const double *pow_r, const double *phase_r,
                     double xconst, double yconst, double zconst, const cbet_params *p, const cbet_gain_params *g,
                     cbet_context *ctx, void *stream);
/*
 * Per-beam energy balance of exit records: exits = device [nbeams][L], tally = device double[nbeams][8] (columns
 * CBET_TALLY_*), OVERWRITTEN.  Only records with CBET_RAY_LAUNCHED count, and each of them is booked in exactly one of
 * escaped, stranded, unfinished -- escaped if ESCAPED is set, else stranded if CUTOFF is set, else unfinished -- so per beam
 *   launched + gained = absorbed + escaped + stranded + unfinished   (up to rounding)
 * for ANY records.  cbet_trace_exits sets TIMEOUT on exactly the rays with neither ESCAPED nor CUTOFF; in a record from
 * elsewhere the TIMEOUT bit itself is not looked at (LAUNCHED alone counts as unfinished, CUTOFF | TIMEOUT as stranded).
 * Fixed-order reduction (no atomics): bit-reproducible from run to run.  Enqueued on `stream`.
 */
int cbet_exit_tally(const cbet_ray_exit *exits, long L, int nbeams, double *tally, void *stream);
/*
 * Far field of the escaped light: the remaining uray of every record with CBET_RAY_LAUNCHED and CBET_RAY_ESCAPED among
 * the n records is ADDED into device double hist[ntheta][nphi], binned by the exit direction v / |v|:
 *   it = min(ntheta - 1, floor((1 - vz / |v|) / 2 * ntheta))        (equal solid angle per polar bin)
 *   ip = min(nphi - 1, floor((atan2(vy, vx) + pi) / (2 pi) * nphi))
 * A coordinate (the argument of floor) that is not > 0 goes to bin 0; that includes NaN: a record with v = 0 has no polar
 * coordinate (0 / 0) and lands in it = 0, with ip from atan2(+-0, +-0) as IEEE 754 defines it (+0 for v = +0).
 * A beam's own map: pass its contiguous slice exits + (b - grid_beam0) * L, n = L.  Enqueued on `stream`; the sum
 * order of a bin is not fixed (fp64 atomics).
 */
int cbet_farfield(const cbet_ray_exit *exits, long n, int ntheta, int nphi, double *hist, void *stream);

/* ---- ray path recorder -------------------------------------------------------- */
/*
 * Single rays made visible: sampled trajectories and one closest-approach record per ray, for an explicit list of rays.
 *
 * Items.  beams[nitems] and raynums[nitems] are int32 DEVICE arrays; item k is the ray with thread-ray id raynums[k]
 * (the ids of cbet_live_ray_list, launch_ray_XZ.cu:125,156) of beam beams[k].  An item is TRACED when
 *     0 <= beam < p->nbeams,   0 <= raynum < cbet_derived.nrays,   and the launch accepts the ray (:94,114: the launch
 *     point lies inside the beam radius).
 * Every other item is an idle lane: its turn record is all zeros (status 0) and it writes no sample.  The kernel makes
 * that test itself, so a list may hold anything.  Which ids are safe: the launch decodes an id into the ray's column and
 * row of the beam cross-section (:70-73), tile = id / rpz^2, within = id % rpz^2, row = tile / zones * rpz + within / rpz,
 * column = tile % zones * rpz + within % rpz, with nrays = nrays_x * nrays_y, nrays_x = rpz * zones and nrays_y =
 * rpz * zones_y.  For 0 <= id < nrays: tile < zones * zones_y, so row < nrays_y and column < nrays_x -- EVERY id in
 * [0, nrays) indexes the two launch axes (nrays_x and nrays_y entries) in range, whether or not the launch shape of
 * max_threads visits it; ids outside that interval are never decoded.  Ids the launch rule leaves out may be traced: the
 * list is the caller's.  One wavefront takes 64 consecutive items.
 *
 * Samples.  Sample 0 is the launch state: the launch point, uray0, absorbed = gained = 0, the launch node, step 0.
 * Sample m >= 1 is the state after step min(m * stride, steps); a ray of `steps` steps has nsamples = 1 +
 * ceil(steps / stride) samples and its last sample is always its end state.  Storage is SAMPLE-major:
 * samples[m * nitems + k] is sample m of item k, capacity * nitems records.  Samples with m >= capacity are not written,
 * and nothing is ever written outside [0, capacity); slots the call does not write (samples a ray does not have, idle
 * items) are left as they are.
 */
typedef struct cbet_path_sample {
    double x, y, z;       /* position (cm)                                                                       */
    double uray;          /* energy the ray carries (after the step's gain and absorption)                       */
    double absorbed;      /* energy absorbed in the steps since the previous sample, summed in step order        */
    double gained;        /* energy gained through CBET in those steps, summed in step order (0 without a gain)  */
    int ci, cj, ck;       /* the ray's node (the reference's cell, after the nearest-node update)                */
    int step;             /* 0 = launch point; t = state after step t                                            */
} cbet_path_sample;       /* 64 bytes */
/*
 * Turn records, one per item: the ray's closest approach to `center`, over the launch point and the position after every
 * step, with r2 evaluated exactly as
 *     r2 = ((x - cx) * (x - cx) + (y - cy) * (y - cy)) + (z - cz) * (z - cz)
 * (that parenthesisation, no fused multiply-add).  The FIRST minimum wins: a later position replaces the record only when
 * its r2 is strictly smaller.
 */
typedef struct cbet_ray_turn {
    double r2;            /* smallest squared distance to `center` (cm^2)                                        */
    double x, y, z;       /* position there                                                                      */
    double uray;          /* energy there (as in the sample of that step)                                        */
    double ne;            /* ne3d at the ray's node there: the node table's entry, cm^-3                         */
    int step;             /* where: 0 = launch point, t = after step t                                           */
    int steps, status;    /* as cbet_ray_exit.steps / .status (CBET_RAY_* bits); status 0 = idle item            */
    int nsamples;         /* 1 + ceil(steps / stride), whether or not `capacity` held them                       */
} cbet_ray_turn;          /* 64 bytes */
#ifdef __cplusplus
static_assert(sizeof(cbet_path_sample) == 64 && sizeof(cbet_ray_turn) == 64, "path records are 64 bytes");
#else
_Static_assert(sizeof(cbet_path_sample) == 64 && sizeof(cbet_ray_turn) == 64, "path records are 64 bytes");
#endif
/*
 * The recorder: the exit pass's integrator (a traced ray's positions, nodes, energies, step count and status are that
 * pass's, bit for bit) on the items of the list.  stride >= 1, capacity >= 0 (0: turn records only; samples may then be
 * NULL), center = three finite doubles (cm).  samples: device [capacity][nitems]; turns: device [nitems], every entry
 * written.  ne3d / kappa3d NULL = the context's own tables and step records, as in cbet_trace_exits.  gain: device
 * [nbeams][(nx+2)(ny+2)(nz+2)] indexed by the ITEM's beam, or NULL; with it every step applies the CBET hook (g supplies
 * max_exponent).  The hook's choice of series is a vote of the wavefront, so with a gain a ray's last bits may depend on
 * the 63 items beside it; without one, an item's records depend on neither its place in the list nor its neighbours.
 * Absorbing mode only.  The beam range, the shard split, grid_beam0 / grid_beams, kernel_variant and the per-beam-grid
 * options of *p do not apply.  The context's counters are not touched.  nitems == 0 succeeds and launches nothing.
 * CBET_EINVAL, naming the offence, judged before the context and before any device call: stride < 1; capacity < 0;
 * nitems < 0, or nitems * max(capacity, 1) records beyond what a 64-bit byte count holds (or more items than one launch
 * takes, 2^31 - 1 wavefronts); NULL turns, NULL beams / raynums with nitems > 0, NULL samples with capacity > 0; a
 * non-finite center; non-absorbing mode; a gain grid without gain params.  Enqueued on `stream`, no synchronisation.
 */
int cbet_trace_paths(const double *ne3d, const double *kappa3d, const double *gain, const int *beams, const int *raynums,
                     long nitems, int stride, int capacity, const double *center, cbet_path_sample *samples,
                     cbet_ray_turn *turns, const double *bbeam_norm, const double *beam_norm, const double *pow_r,
                     const double *phase_r, double xconst, double yconst, double zconst, const cbet_params *p,
                     const cbet_gain_params *g, cbet_context *ctx, void *stream);

/* ---- backscatter SBS gain spectra along rays --------------------------------------------- */
/*
 * Stimulated Brillouin backscatter as a ray-based LINEAR gain post-processor: for every ray of a list and every frequency
 * shift delta_m of the scattered light (rad/s relative to the ray's own beam, negative = red) the convective gain exponent
 *     Gamma_m = sum over the ray's steps of (g_m * I) * ds
 * No reference counterpart: parity UNPINNED, like the whole CBET stage.  The statements are csrc/cbet_sbs_model.h's, one IEEE
 * fp64 operation per written operator, for the kernel and the host twin alike, so the two agree bit for bit.
 *
 * A ray is traced exactly as cbet_trace_paths traces it (items, idle items, gain hook, absorbing mode: that contract).  With
 * p_t the position after step t (p_0 the launch point) and (ci, cj, ck)_t the ray's node after it, step t = 1 .. steps adds
 *     d       p_t - p_(t-1), per component;   ds = sqrt((d.x d.x + d.y d.y) + d.z d.z);   a step with ds == 0.0 adds nothing
 *     h       ((ci + 1) (ny + 2) + (cj + 1)) (nz + 2) + (ck + 1): the deposit-grid cell whose plasma is that node's
 *     c, pref the gain stage's cell state and prefactor of cell h, from the context's flow table / state table if it has them
 *             (the closed-form Mach ramp and cbet_gain_constants' scalars otherwise); pref = 0 at and above critical density
 *     q       the ion-acoustic wave of the pair (backscattered seed, the ray's own light): q = 2 k_ray = qs d,
 *             qs = ((2.0 * k0) / c) / dt computed once on the host;   kiaw = sqrt((q.x q.x + q.y q.y) + q.z q.z)
 *     g_m     pref P(((0.0 - q . u) + (0.0 - delta_m)) / (kiaw cs + 1e-10)), the gain stage's detuned pair gain;
 *             times 0.5 under CBET_POL_SMOOTHED (the smoothing factor at cos theta = -1)
 *     I       fields[0][beam][h], the beam's own normalised intensity in that cell
 * and Gamma_m starts from +0.0 and takes its terms in step order.  The context's saturation limit, per-beam detuning and
 * line spectrum are NOT applied: the seed's shift is the scan variable and the gain is linear.  Left out as well: pump
 * depletion, shared-wave (multi-beam) SBS, sidescatter, absorption of the scattered light, and where along the ray the gain
 * accrues (re-trace chosen rays with cbet_trace_paths).
 *
 * gamma is SHIFT-major: gamma[m * nitems + k] is Gamma_m of item k, nshift * nitems doubles; rays[k] is item k's record.
 * Every entry of both is written; an idle item gets zeros.
 */
#define CBET_SBS_MAX_SHIFTS 16
typedef struct cbet_ray_sbs {
    double gmax;          /* the largest Gamma_m of the ray                                                      */
    double uray0;         /* launch energy                                                                       */
    double uray_end;      /* energy the ray still carries when it ends                                           */
    int steps;            /* as cbet_ray_exit.steps                                                              */
    short imax;           /* the shift index of gmax, 0 .. nshift - 1: the FIRST maximum wins                    */
    short status;         /* as cbet_ray_exit.status (CBET_RAY_* bits); 0 = idle item                            */
} cbet_ray_sbs;           /* 32 bytes: a wavefront's 64 records are 2 KB of whole lines; three doubles and four ints
                             would be 40, so the two small members are 16-bit and there is no padding member */
#ifdef __cplusplus
static_assert(sizeof(cbet_ray_sbs) == 32, "cbet_ray_sbs is 32 bytes");
#else
_Static_assert(sizeof(cbet_ray_sbs) == 32, "cbet_ray_sbs is 32 bytes");
#endif
/* Columns of a cbet_backscatter_tally entry. */
#define CBET_SBS_TALLY_COLUMNS 4
#define CBET_SBS_TALLY_URAY0 0        /* sum of uray0 over the beam's launched items                   */
#define CBET_SBS_TALLY_WEIGHTED 1     /* sum of uray0 * Gamma_m                                        */
#define CBET_SBS_TALLY_MAX 2          /* max of Gamma_m (0 while the entry counts no ray)              */
#define CBET_SBS_TALLY_N_RAYS 3       /* launched items                                                */
/*
 * cbet_trace_backscatter: cbet_trace_paths' arguments without the recorder's own, plus fields (device, NORMALISED whole-grid
 * [4][nbeams][(nx+2)(ny+2)(nz+2)] as a gain update leaves them, never written; only the intensities are read), shifts
 * (nshift HOST doubles, captured at the call), gamma and rays (device).  g is REQUIRED: it carries the ion-acoustic damping,
 * the Mach ramp and the plasma state of the model (and max_exponent for a gain grid).  ne3d NULL = the context's table, for
 * the trace and the model alike.  The context's counters are not touched.  nitems == 0 succeeds and launches nothing.
 * CBET_EINVAL, naming the first offence, judged before the context and before any device call: nshift outside
 * 1 .. CBET_SBS_MAX_SHIFTS; NULL shifts or a shift that is not finite; NULL fields; NULL gain params; nitems < 0 or more
 * items than one launch takes or nshift * nitems beyond a 64-bit byte count; NULL rays or gamma; NULL beams / raynums with
 * nitems > 0; non-absorbing mode; nbeams > CBET_MAX_CBET_BEAMS.  Enqueued on `stream`, no synchronisation.
 *
 * cbet_backscatter_tally: per beam and shift, over the LAUNCHED items of that beam, {sum uray0, sum uray0 * Gamma_m,
 * max Gamma_m, number of rays} MERGED INTO tally (device double [nbeams][nshift][4]: sums and counts add, the maximum is
 * taken over entries that count a ray), so calls on parts of a list compose; zero it before the first.  beams: the item
 * list's device array.  No atomics: fixed-order partial entries go to `work` (cbet_backscatter_work_bytes(nitems, nshift,
 * nbeams) bytes; 0 for bad arguments) and a second kernel merges them in a fixed order that follows from nitems alone, so
 * two calls give the same bytes.  Items whose beam is outside [0, nbeams) or whose record is not LAUNCHED count nowhere.
 *
 * cbet_backscatter_host: the host twin, HOST pointers, no HIP call.  samples ([capacity][nitems], sample-major) and turns
 * ([nitems]) are STRIDE-1 records of the same items as cbet_trace_paths writes them (or built from the CPU oracle's ray
 * paths): positions, nodes, uray and nsamples are read, and steps / status are copied into the records.  An item whose turn
 * record has status 0 is idle.  flow ([3][nodes]) and state ([2][nodes]) are node tables or NULL, pol a CBET_POL_* mode.
 * CBET_EINVAL beside the refusals above: an item with nsamples > capacity or nsamples < 1, a launched item's beam outside
 * [0, nbeams) or a sample's node outside the grid.
 */
int cbet_trace_backscatter(const double *ne3d, const double *kappa3d, const double *gain, const int *beams, const int *raynums,
                           long nitems, const double *fields, const double *shifts, int nshift, double *gamma,
                           cbet_ray_sbs *rays, const double *bbeam_norm, const double *beam_norm, const double *pow_r,
                           const double *phase_r, double xconst, double yconst, double zconst, const cbet_params *p,
                           const cbet_gain_params *g, cbet_context *ctx, void *stream);
size_t cbet_backscatter_work_bytes(long nitems, int nshift, int nbeams);
int cbet_backscatter_tally(const double *gamma, const cbet_ray_sbs *rays, const int *beams, long nitems, int nshift, int nbeams,
                           double *tally, void *work, void *stream);
int cbet_backscatter_host(const cbet_path_sample *samples, const cbet_ray_turn *turns, const int *beams, long nitems,
                          int capacity, const double *fields, const double *ne3d, const double *flow, const double *state,
                          int pol, const double *shifts, int nshift, double *gamma, cbet_ray_sbs *rays, const cbet_params *p,
                          const cbet_gain_params *g);

/* ---- Anderson mixing of the gain iterate -------------------------------------------------- */
/*
 * The streaming work of Anderson mixing over plain arrays of n doubles (the gain stack of a CBET solve is one such array):
 * nothing here knows a grid, a beam or a context.  A fixed-point iteration x -> y(x) holds up to CBET_MIX_MAX_DEPTH + 1
 * entries (y_j, f_j = y_j - x_j), OLDEST FIRST in every list below, and its next iterate is sum_j alpha_j y_j with the alpha
 * that minimise || sum_j alpha_j f_j ||_2 under sum_j alpha_j = 1.  Every statement is ONE IEEE fp64 operation per written
 * operator in the written order (csrc/cbet_mix_model.h, no fused multiply-add), for the kernels and the host twins alike.
 *
 * cbet_mix_residual: f[e] = y[e] - x[e] for e < n, and the Gram row
 *     row[j] = sum_e f[e] * f_held[j][e]   (j < h, the h held residuals)        row[h] = sum_e f[e] * f[e]
 * into row (h + 1 doubles; DEVICE memory for cbet_mix_residual, OVERWRITTEN).  The order of every sum follows from n and
 * the ELEMENT INDEX alone: element e belongs to span e / CBET_MIX_SPAN, spans go round-robin to
 * G = min(ceil(n / CBET_MIX_SPAN), CBET_MIX_MAX_GROUPS) workgroups of 256 threads, thread t of a workgroup takes the elements
 * 2 (256 i + t) and 2 (256 i + t) + 1 of a span (i = 0 .. CBET_MIX_SPAN / 512 - 1) and adds its products in ascending element
 * order from +0.0; the 64 lanes of a wavefront are summed by six butterfly steps (s = s + s[lane ^ 32], ^ 16, ... ^ 1), the
 * four wavefronts in order, one partial row per workgroup goes to `work` (cbet_mix_work_bytes(n) bytes of device memory; 0
 * for n < 0; no atomics), and a second kernel of one workgroup sums the partial rows (thread t rows t, t + 256, ... in
 * order, then the same butterfly and wavefront order).  Nothing depends on the device or on an address: two calls give the
 * same bytes, a view that starts anywhere inside an allocation gives the bytes of an aligned copy, and the host twin,
 * which walks the same order, gives the same bytes as the device.  Arrays need the alignment of a double only (a thread's
 * pair of elements moves as one 16-byte access at any such address, which changes no sum).  f must not overlap any input.
 *
 * cbet_mix_apply: x[e] = alpha[0] * y_held[0][e], then x[e] = x[e] + alpha[j] * y_held[j][e] for j = 1 .. count - 1, stored
 * to x_out[e] and, when x_keep is not NULL, to x_keep[e].  alpha: count HOST doubles, captured at the call.  count = 1 with
 * alpha = {1.0} copies y_held[0]'s bytes.  x_out may BE one of the y_held arrays (the slot that retires): every element is
 * read from all of them before it is written; any other overlap is the caller's error.
 *
 * cbet_mix_coefficients: pure host arithmetic, the same bytes wherever it runs.  gram: count x count HOST doubles, row-major,
 * gram[a * count + b] = <f_a, f_b> (only a <= b is read).  With n = count - 1 the newest entry and d entries dropped, the
 * differences against the newest, H_ab = G_ab - G_an - G_bn + G_nn and c_a = G_nn - G_an over a, b = n - 1 down to d, are
 * factored by Cholesky from the newest difference to the oldest, gamma solves H gamma = c, alpha_a = gamma_a and
 * alpha_n = 1.0 - sum_a gamma_a (summed newest to oldest).  A pivot that is not > 1e-12 * its own diagonal entry H_aa is
 * lost (the Gram entries are known to that relative bound): the OLDEST held entry is dropped (d = d + 1) and the system is
 * solved again.  alpha[0 .. d) = 0.0; *dropped = d.  count = 1 gives alpha = {1.0}.
 *
 * CBET_EINVAL with cbet_last_error, before any device work: h outside 0 .. CBET_MIX_MAX_DEPTH, count outside
 * 1 .. CBET_MIX_MAX_DEPTH + 1, n < 0, a NULL array (f_held may be NULL when h == 0; x_keep may be NULL; work may be NULL
 * when n == 0).  The device entries run on the calling thread's current device, enqueue on `stream` and do not synchronise.
 */
#define CBET_MIX_MAX_DEPTH 4
#define CBET_MIX_SPAN 2048
#define CBET_MIX_MAX_GROUPS 2048
size_t cbet_mix_work_bytes(long n);
int cbet_mix_residual(const double *y, const double *x, double *f, const double *const *f_held, int h, long n, double *row,
                      void *work, void *stream);
int cbet_mix_apply(const double *const *y_held, const double *alpha, int count, long n, double *x_out, double *x_keep,
                   void *stream);
int cbet_mix_coefficients(const double *gram, int count, double *alpha, int *dropped);
int cbet_mix_residual_host(const double *y, const double *x, double *f, const double *const *f_held, int h, long n,
                           double *row);
int cbet_mix_apply_host(const double *const *y_held, const double *alpha, int count, long n, double *x_out, double *x_keep);

/* ---- mode spectra of the deposit ---------------------------------------------------------- */
/*
 * How uniformly the energy is deposited around a centre: the real spherical-harmonic coefficients of each grid on
 * spherical shells.
 *
 * Nodes.  The input is the haloed deposit grid edep[I][J][K], I in [0, nx+1] etc., halo nodes included (they hold real
 * deposits); rows are nz + 2 doubles, or p->edep_zpitch when that is set; ngrids grids lie grid_stride doubles apart.
 * The coordinates of node (I, J, K) relative to the centre c are evaluated exactly in this order, with no fused
 * operations (dx, dy, dz from cbet_derive; the node coordinates of cbet_node_coordinates with i = I - 1):
 *     x = ((I - 1) * dx + xmin) - cx,  y and z alike,  r = sqrt(x*x + y*y + z*z)
 * Shell s holds the nodes with r_edges[s] <= r < r_edges[s+1]; nodes in no shell are ignored.  r_edges: strictly
 * increasing, finite, r_edges[0] >= 0.  Angles: cos(theta) = z / r, phi = atan2(y, x).  A node at r == 0 contributes to
 * its shell's energy and to Y_00 only.
 *
 * Harmonics: real, orthonormal, WITHOUT the Condon-Shortley phase (scipy's sph_harm_y includes (-1)^m):
 *     Y_l0 = N_l0 P_l^0(cos theta),  Y_l,m = sqrt(2) N_lm P_l^m(cos theta) cos(m phi),
 *     Y_l,-m = sqrt(2) N_lm P_l^m(cos theta) sin(m phi)   (m > 0),
 *     N_lm = sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!),  P_l^m(x) = (1-x^2)^(m/2) d^m P_l / dx^m  (>= 0 near x = 1).
 * Coefficient index c = l*l + l + m.
 *
 * Outputs, OVERWRITTEN:
 *     coeffs       double [ngrids][nshell][(lmax+1)^2]  a_gsc = sum over the nodes of shell s of E_g(node) Y_c(node)
 *     shell_energy double [ngrids][nshell]              sum of E_g over the shell's nodes
 *     shell_nodes  int64  [nshell]                      nodes in the shell
 * Geometry mode: edep == NULL with ngrids == 1 projects E = 1: the lattice's own spectrum, the floor a perfectly uniform
 * deposit shows (about a cubic grid's centre, odd l and l = 2 vanish and l = 4, 6, 8, ... do not).
 *
 * Limits: 0 <= lmax <= CBET_SPH_LMAX, 1 <= nshell <= CBET_SPH_MAX_SHELLS, 1 <= ngrids <= CBET_SPH_MAX_GRIDS; with
 * ngrids > 1, grid_stride >= one grid's (nx+2)(ny+2)(row length) doubles.  Anything else is CBET_EINVAL before any
 * device work.
 *
 * Determinism: fixed-order sums, no floating-point atomics -- the same bits from run to run -- and the order follows the
 * logical node index, so a padded grid gives the bits of the dense grid with the same values.
 */
#define CBET_SPH_LMAX 32
#define CBET_SPH_MAX_SHELLS 256
#define CBET_SPH_MAX_GRIDS 64
/* Device grids and outputs; center (3 doubles) and r_edges (nshell + 1 doubles) are HOST arrays, captured at the call.
 * Enqueued on `stream`, no synchronisation (graph-capturable). */
int cbet_sph_modes_device(const double *edep, int ngrids, long grid_stride, const cbet_params *p, const double center[3],
                          const double *r_edges, int nshell, int lmax, double *coeffs, double *shell_energy,
                          long long *shell_nodes, void *stream);
/* The same on HOST arrays, as plain loops (the reference the device result is checked against); stream is unused. */
int cbet_sph_modes(const double *edep, int ngrids, long grid_stride, const cbet_params *p, const double center[3],
                   const double *r_edges, int nshell, int lmax, double *coeffs, double *shell_energy,
                   long long *shell_nodes, void *stream);

/* ---- deposit on the hydro mesh: conservative remap to spherical-polar cells --------------- */
/*
 * The way back to a hydrodynamics code: the energy of one deposit grid, or of a stack of per-beam grids, binned into the
 * CELLS of a spherical-polar mesh about a centre o.  Every sample of the grid lands in exactly one cell or in `outside`,
 * so sum(cell_energy) + outside = sum(grid) up to rounding.
 *
 * Cells (cbet_mesh_cells, HOST arrays, captured by cbet_mesh_cells_create): nr >= 1 shells, ntheta >= 1 rows, nphi >= 1
 * columns between the edges
 *     r_edges[nr+1]          strictly ascending, finite, r_edges[0] >= 0
 *     theta_edges[ntheta+1]  strictly ascending, |theta_edges[0]| <= 1e-12, |theta_edges[ntheta] - pi| <= 1e-12;
 *                            may be NULL when ntheta == 1
 *     phi_edges[nphi+1]      strictly ascending, -pi <= phi_edges[0] < pi,
 *                            |phi_edges[nphi] - phi_edges[0] - TWO_PI| <= 1e-12; may be NULL when nphi == 1
 * Only the interior theta edges and the first nphi phi edges enter the lookup, so every direction belongs to exactly one
 * (row, column).  nr + ntheta + nphi + 3 <= CBET_MESH_MAX_COORDS and nr * ntheta * nphi < 2^31.
 *
 * Samples.  The input is cbet_sph_modes's: the haloed grid edep[I][J][K], halo nodes included, rows of nz + 2 doubles or
 * p->edep_zpitch, ngrids grids grid_stride doubles apart.  The energy E of node (I, J, K) is spread evenly over the box
 * dx dy dz centred on the node, as S^3 sub-samples, S = subsamples in {1, 2, 3, 4}.  Every statement below is ONE IEEE
 * fp64 operation per written operator, in the written order, no fused multiply-add:
 *     off[a] = (2a + 1 - S) / (2.0 * S)   a = 0 .. S-1     (a table the host makes)
 *     xs = ((I - 1) * dx + xmin) + off[a] * dx,  sx = xs - ox;      y with (J, b) and z with (K, c) alike
 *     rho = sqrt(sx*sx + sy*sy + sz*sz)                             squares summed x, y, z
 * and each sample carries E * inv, inv = 1.0 / (S*S*S) (host-made).  With S = 1, off = 0 and the sample is the node with
 * cbet_sph_modes's coordinates, bit for bit.
 *
 * Cell of a sample.  No trigonometric function is evaluated per sample on either side, so the device and the host twin
 * put every sample into the same cell, bit for bit (the atan2 caveat of the hydro-mesh plasma does not apply here, where it
 * would move a whole node's energy):
 *     shell m:  r_edges[m] <= rho < r_edges[m+1]; a sample in no shell (a NaN rho included) goes to `outside`
 *     row:      c = sz / rho;  row = the number of interior theta edges e with c <= ct[e],
 *               ct[e] = cos(theta_edges[e]), a table the host makes (descending)
 *     column:   the "diamond angle" of (sx, sy):  a = |sx| + |sy|;  d = 0 if a == 0, else t = sx / a and
 *               d = (sy >= 0) ? 1.0 - t : 3.0 + t, in [0, 4), ascending with phi.  The host makes
 *               pe[k] = d(cos(phi_edges[k]), sin(phi_edges[k])) for k < nphi, + 4.0 wherever pe[k] < pe[0], and refuses
 *               cells whose pe is not strictly ascending (columns thinner than the rounding of cos and sin).
 *               d = d + 4.0 if d < pe[0];  column = the last k with pe[k] <= d
 * Degenerate samples: rho == 0 (the sample is the centre) is counted in row 0 and column 0 of its shell.  A sample on the
 * polar axis (a == 0, rho > 0) has d = 0: the column that holds phi = 0; its row is 0 above the centre (c = 1) and
 * ntheta - 1 below (c = -1).  sy == -0.0 counts as sy >= 0.
 * Every index lies inside its table whatever the grid and the cells hold, NaN included.
 *
 * Outputs, OVERWRITTEN:
 *     cell_energy  double [ngrids][nr][ntheta][nphi]   sum of E * inv over the cell's samples
 *     outside      double [ngrids]                     the same over the samples in no shell
 *     cell_samples int64  [nr][ntheta][nphi]           samples in the cell; times dx dy dz / S^3: the sampled volume, which
 *                                                      turns an energy into a power density
 * edep == NULL with ngrids == 1 writes cell_samples only (cell_energy and outside may then be NULL).
 * Limits: 1 <= ngrids <= CBET_SPH_MAX_GRIDS, 1 <= subsamples <= the handle's subsamples_max <= CBET_MESH_MAX_SUBSAMPLES;
 * with ngrids > 1, grid_stride >= one grid's doubles.  Anything else is CBET_EINVAL before any device work.
 *
 * Sums.  The counts are integers and exact.  The device adds the energies with floating-point atomics, in any order, and
 * books a run of consecutive samples of one node that share a cell as ONE contribution (E * inv) * n: like the deposit it
 * remaps, and like cbet_farfield, the energies are NOT bit-reproducible from run to run; they agree with the host twin
 * within the rounding of sums taken in another order.  A sample with E == 0 issues no energy atomic.
 *
 * cbet_mesh_cells_create validates the cells (CBET_EINVAL names the first offence), builds ct, pe and off, keeps host
 * copies and, with gpu >= 0, uploads them once to that device (allocates and synchronises here); gpu == -1 makes a
 * host-only handle, which cbet_mesh_deposit accepts and cbet_mesh_deposit_device refuses.
 * cbet_mesh_deposit_device: DEVICE grids and outputs; enqueues the zero-fill of the outputs and one kernel on `stream`:
 * no allocation, no synchronisation, graph-capturable.  method: CBET_MESH_DEPOSIT_AUTO, _GLOBAL (every contribution a
 * global atomic: meshes with many cells, where few contributions meet) or _LDS (workgroup-private accumulators in LDS,
 * flushed once: the 1-D and coarse 2-D meshes, where millions of nodes would meet at a few hundred addresses).  The LDS
 * arm handles ceil(ngrids / 8) grids per workgroup and needs
 *     8 (nr + ntheta + nphi + subsamples + ngrids') + nr ntheta nphi (8 ceil(ngrids / 8) + 4) <= 40960 bytes
 * (ngrids' = ceil(ngrids / 8)); where that does not hold _LDS is CBET_EINVAL and _AUTO takes _GLOBAL.
 * cbet_mesh_deposit: the host twin on HOST arrays: plain loops in logical node order, a node's samples in (a, b, c)
 * order, c fastest, one addition per sample; its sums are the same bits from call to call.  method and stream are ignored.
 */
#define CBET_MESH_MAX_SUBSAMPLES 4
#define CBET_MESH_DEPOSIT_AUTO 0
#define CBET_MESH_DEPOSIT_GLOBAL 1
#define CBET_MESH_DEPOSIT_LDS 2
typedef struct cbet_mesh_cells {
    double center[3];                       /* o (cm)                                                             */
    int nr, ntheta, nphi;                   /* cells                                                              */
    const double *r_edges, *theta_edges, *phi_edges;   /* HOST, nr + 1, ntheta + 1 (or NULL), nphi + 1 (or NULL) */
} cbet_mesh_cells;
typedef struct cbet_mesh_cells_handle cbet_mesh_cells_handle;
int cbet_mesh_cells_create(cbet_mesh_cells_handle **out, const cbet_mesh_cells *cells, int subsamples_max, int gpu);
void cbet_mesh_cells_destroy(cbet_mesh_cells_handle *handle);
int cbet_mesh_deposit_device(const cbet_mesh_cells_handle *handle, const double *edep, int ngrids, long grid_stride,
                             const cbet_params *p, int subsamples, int method, double *cell_energy, double *outside,
                             long long *cell_samples, void *stream);
int cbet_mesh_deposit(const cbet_mesh_cells_handle *handle, const double *edep, int ngrids, long grid_stride,
                      const cbet_params *p, int subsamples, int method, double *cell_energy, double *outside,
                      long long *cell_samples, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CBET_MI355X_H_ */
