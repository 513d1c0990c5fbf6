// cbet_device.h -- argument blocks shared by the host ABI (cbet_*_abi.cpp, cbet_host_internal.h) and the gfx950 kernels
// (cbet_kernels.hip).  Internal; the public boundary is include/cbet_mi355x.h.
#ifndef CBET_DEVICE_H_
#define CBET_DEVICE_H_

#include <hip/hip_runtime_api.h>

#include "cbet_mi355x.h"

namespace cbet {

// Physical constants, /root/reference/def.cuh:61-69, 78, 91, 119, 55-56.
constexpr double kC = 29979245800.0;
constexpr double kE0 = 8.85418782e-12;
constexpr double kMe = 9.10938356e-31;
constexpr double kEc = 1.60217662e-19;
constexpr double kLambda = 1.053e-4 / 3.0;
constexpr double kSigma = 0.0375;
constexpr double kIntensity = 1.0e14;
constexpr double kFocal = 0.1;
constexpr double kBeamMin = -450.0e-4;
constexpr double kBeamMax = 450.0e-4;

constexpr unsigned kEmptyTag = 0xFFFFFFFFu;
constexpr int kWave = 64;

// Device counter slots (unsigned long long each); mirrors cbet_counters.
enum CounterSlot { kCntSteps = 0, kCntRays = 1, kCntGlobalAtomics = 2, kCntEvictions = 3, kCntWaveSteps = 4,
                   kCntWaveStepsMiss = 5, kCntWaveStepsWide = 6, kCntSlabsRetired = 7, kCntSlots = 8 };

// Everything the tabulation kernel needs.
struct TabulateArgs {
    int nx, ny, nz, nprofile;
    double xmin, ymin, zmin;
    double dx, dy, dz, dt;
    double ncrit;
    const double *r, *ne, *te;  // device, nprofile each
    double *ne3d, *kap3d;       // device, nx*ny*nz each
};

// What a ray-step of the shipped integrator reads at its (new) node, as ONE 32-byte record: the three velocity
// kicks of launch_ray_XZ.cu:268-270 -- xconst * (ne(x+1) - ne(x-1)) with the one-sided face rule of :212-238,
// the very products the reference forms, tabulated once per node -- and the absorption coefficient of :296-305
// (kappa3d).  One aligned 32-byte gather per lane and step instead of seven 8-byte gathers from five lines.
struct StepRecord {
    double kx, ky, kz, kap;
};

struct StepTableArgs {
    int nx, ny, nz;
    double xconst, yconst, zconst;          // main.cu:156-159
    const double *ne3d, *kap3d;             // node tables, nx*ny*nz each
    StepRecord *rec;                        // out, nx*ny*nz
};

// The fused table kernel (k_plasma_records): both of the above in one pass.
struct PlasmaRecordsArgs {
    TabulateArgs t;
    double xconst, yconst, zconst;
    StepRecord *rec;
};

// Everything the trace kernel needs, passed by value as the kernel argument.
struct TraceArgs {
    // grid (def.cuh:35-53)
    int nx, ny, nz;
    double xmin, ymin, zmin;
    double dx, dy, dz, dt;
    double inv_dx, inv_dy, inv_dz;          // (1/dx) of launch_ray_XZ.cu:276-278
    double fx_hi, fy_hi, fz_hi;             // n - 3: cell-unit positions beyond it are "near a face"
    const double *bounds;                   // device: {xlo,xhi,ylo,yhi,zlo,zhi} = xmin-(dx/2.0) ... launch_ray_XZ.cu:352-354
    double exit_planes[6];                  // ... the same six values in the argument segment (host_exit_planes): the shipped kernel compares with scalar operands
    double tol_x, tol_y, tol_z;             // 0.5001*dx of launch_ray_XZ.cu:164-176
    double xconst, yconst, zconst;          // main.cu:156-159
    int nt, absorption;
    // launch geometry (launch_ray_XZ.cu:65-115)
    int rpz, zones, nrays_x;
    double z_launch;                        // focal_length - dz/2
    double uray_mult, omega, ncrit;
    const double *xlaunch, *ylaunch;        // running-sum launch coordinates, dx/2 already added
    const int *live;                        // compacted thread-ray ids (beam independent)
    int nlive;
    // work split
    int beam_lo, nbeams_local, bundles_per_beam;
    long total_bundles;
    long first_item, item_count;            // this launch's contiguous share of the (beam, patch) list
    // tables
    const double *ne3d, *kap3d;
    const StepRecord *steprec;              // LDS_WINDOW kernel: per-node step records built from the two tables
    const double *beam_norm, *bbeam_norm, *pow_r, *phase_r;
    double *edep;
    int sYh, sXh;                           // strides of the haloed deposit grid in doubles: a row (nz+2, or cbet_params.edep_zpitch), a plane
    long grid_stride;                       // 0: one grid for all beams; else doubles between per-beam grids
    unsigned long long *counters;
    int stats;                              // cbet_params.window_stats: count the window diagnostics too (LDS_WINDOW kernel)
    // bounds-audit builds (-DCBET_DEBUG_BOUNDS) only; unused otherwise
    unsigned long long *audit_count;        // violations counter
    const double *audit_lo, *audit_hi;      // the grid range a launch may add into
    unsigned long long audit_nodes, audit_hsize;  // entries of a node table / of a beam's haloed gain grid
    // CBET extension (no reference counterpart).  All zero / NULL = the reference path.
    int grid_beam0;                         // beam whose grid comes first in a beam-resolved `edep` / in `gain` (cbet_params.grid_beam0)
    const double *gain;                     // [grid beams][(n+2)^3] gain coefficient on the deposit grid, 1/cm
    long hsize;                             // (nx+2)(ny+2)(nz+2)
    int quantity;                           // 0: deposit the absorbed energy; 1: the four field components (fused field pass); 2: the energy field alone
    long comp_stride;                       // field pass: doubles between the component arrays (nbeams * hsize)
    double max_exponent;                    // clamp on |K ds| per step (<= 1)
    double *beam_gain;                      // [nbeams] energy gained through CBET, or NULL
};

// Field normalisation + gain coefficient kernel (CBET extension).
struct GainArgs {
    int nx, ny, nz, nbeams;
    double xmin, ymin, zmin, dx, dy, dz, dt;
    double ncrit, k0;                       // k0 = omega / c
    double cs, gain_const, iaw;
    double mach_r0, mach_0, mach_r1, mach_1;
    double relax;
    double *fields;                         // [4][nbeams][hsize]: (E, Dx, Dy, Dz) in; (I, kx, ky, kz) out where the beam is present
    const double *ne3d;                     // [nx*ny*nz]
    double *gain;                           // [nbeams][hsize]
    double *scratch;                        // [nbeams][hsize] work array of the symmetric kernel, or NULL (ordered kernel)
    double *change;                         // device {sum |new-old|, sum |new|} accumulators, or NULL
    int hx_lo, hx_hi;                       // planes [hx_lo, hx_hi) of the haloed grid to update (a rank's slab; 0 .. nx+2 = all)
    // storage of fields / gain / scratch: entry of cell h of beam b at [b * bstride + h - store0] (+ component * nbeams * bstride)
    int consume;                            // symmetric kernel: leave the energy entries zeroed instead of normalised (the solve loop's next pass accumulates into them)
    int frozen;                             // the direction entries already hold k (cbet_gain_params.directions_frozen)
    long store0, bstride;                   // whole-grid arrays: 0, hsize; slab-packed arrays: hx_lo * (ny+2)(nz+2), slab entries
    const double *flow;                     // [3][nx*ny*nz] node flow table (ux, uy, uz; cbet_tabulate_flow), or NULL: the closed-form ramp about the origin
    const double *state;                    // [2][nx*ny*nz] node state table (cs, gain_const; cbet_tabulate_mesh_state), or NULL: the scalars cs / gain_const above
    double sat;                             // limit dn_max of the ion-acoustic amplitude a pair's gain corresponds to (cbet_context_set_saturation), 0 = none
    const double *shift;                    // [CBET_MAX_CBET_BEAMS] per-beam angular-frequency shifts, rad/s (cbet_context_set_detuning; entries past nbeams are 0), or NULL: one colour
    int pol;                                // CBET_POL_*: 0 = every pair polarized alike; 1 = polarization smoothing, every pair gain times (1 + cos^2 theta) / 4 (cbet_context_set_polarization)
    // laser bandwidth (cbet_context_set_bandwidth): the difference table of the line spectrum every beam
    // carries, [1 + 2 nband] doubles {c_0, d_0, c_0', d_1, c_1', ...} -- the centre weight, then per entry the difference d_m > 0
    // (rad/s, ascending) and its weight c_m' (band_table, cbet_exchange_host.cpp) -- or NULL: monochromatic beams.  A block with
    // a table always carries `shift` too (zeros where the context has no shifts).
    const double *band;
    int nband;                              // M, the entries behind c_0: 1 .. CBET_MAX_BAND_LINES (CBET_MAX_BAND_LINES - 1) / 2; 0 with band == NULL
};

// What the path recorder (cbet_trace_path.hip) takes BESIDE TraceArgs, as a second by-value kernel
// argument: TraceArgs keeps its members and their offsets, so no other kernel's code moves.
struct PathArgs {
    const int *beams, *raynums;             // device, nitems each: the rays to trace (cbet_trace_paths)
    long nitems;
    int nbeams, nrays;                      // an item is decoded only when 0 <= beam < nbeams and 0 <= raynum < nrays
    int stride, capacity;                   // a sample every `stride` steps; samples m >= capacity are not written
    double cx, cy, cz;                      // the centre of the closest approach
    cbet_path_sample *samples;              // [capacity][nitems], sample-major
    cbet_ray_turn *turns;                   // [nitems]
    // bounds-audit builds (-DCBET_DEBUG_BOUNDS) only; unused otherwise: the ranges the two arrays' stores are checked against
    const cbet_path_sample *audit_samples_lo, *audit_samples_hi;
    const cbet_ray_turn *audit_turns_lo, *audit_turns_hi;
};

// What the backscatter kernel (cbet_backscatter.hip) takes BESIDE TraceArgs and a GainArgs (the gain
// stage's own block, built by gain_args: grid, plasma constants, fields, ne3d, flow and state tables, pol), as a third by-value
// kernel argument: the other two keep their members and their offsets.
struct SbsArgs {
    const int *beams, *raynums;             // device, nitems each: the rays to trace, as PathArgs'
    long nitems;
    int nbeams, nrays;                      // an item is decoded only when 0 <= beam < nbeams and 0 <= raynum < nrays
    int nshift;                             // 1 .. CBET_SBS_MAX_SHIFTS
    double qs;                              // sbs_qs (cbet_sbs_model.h): q = qs * displacement
    double iaw2;                            // GainArgs.iaw squared, once on the host
    double shifts[CBET_SBS_MAX_SHIFTS];     // delta_m, rad/s; entries past nshift are 0 and never read
    double *gamma;                          // [nshift][nitems], shift-major
    cbet_ray_sbs *rays;                     // [nitems]
    // bounds-audit builds (-DCBET_DEBUG_BOUNDS) only; unused otherwise: the ranges the two arrays' stores are checked against
    const double *audit_gamma_lo, *audit_gamma_hi;
    const cbet_ray_sbs *audit_rays_lo, *audit_rays_hi;
};
// k_backscatter_tally + k_backscatter_reduce (cbet_backscatter.hip): chunk c of the list is the items [c * sbs_chunk_items,
// (c + 1) * sbs_chunk_items); both follow from nitems alone.
constexpr long kSbsChunkMin = 4096, kSbsMaxChunks = 1024;
inline long sbs_chunk_items(long nitems)
{
    const long per = ((nitems + kSbsMaxChunks - 1) / kSbsMaxChunks + kWave - 1) / kWave * kWave;
    return per > kSbsChunkMin ? per : kSbsChunkMin;
}
inline long sbs_chunks(long nitems) { return nitems > 0 ? (nitems + sbs_chunk_items(nitems) - 1) / sbs_chunk_items(nitems) : 0; }
hipError_t launch_backscatter_tally(const double *gamma, const cbet_ray_sbs *rays, const int *beams, long nitems, int nshift,
                                    int nbeams, double *tally, double *work, hipStream_t stream);

hipError_t launch_tabulate(const TabulateArgs &a, hipStream_t stream);
hipError_t launch_step_table(const StepTableArgs &a, hipStream_t stream);
hipError_t launch_plasma_records(const PlasmaRecordsArgs &a, hipStream_t stream);
size_t plasma_records_lds(int nprofile);       // dynamic LDS of that launch, bytes
hipError_t audit_violations(unsigned long long *out, bool reset, hipStream_t stream);
// variant: CBET_KERNEL_GLOBAL_ATOMICS, _LDS_COMBINE (cbet_kernels.hip) or _LDS_WINDOW (cbet_trace_window.hip)
// (path: the recorder's second block, variant kTracePaths only)
// (sbs, sbs_gain: the backscatter kernel's second and third block, variant kTraceBackscatter only)
hipError_t launch_trace(const TraceArgs &a, int variant, bool force_idx64, hipStream_t stream, const PathArgs *path = nullptr,
                        const SbsArgs *sbs = nullptr, const GainArgs *sbs_gain = nullptr);
hipError_t launch_trace_window(const TraceArgs &a, bool force_idx64, hipStream_t stream);
// Exit pass (cbet_trace_exit.hip): launch_trace with variant kTraceExits runs it -- TraceArgs.edep is then the record array
// as doubles and grid_stride = kExitDoubles * L -- after the bounds-audit set-up every trace gets.
constexpr int kTraceExits = 100;
constexpr int kExitDoubles = 10;                // sizeof(cbet_ray_exit) / sizeof(double)
hipError_t launch_trace_exit(const TraceArgs &a, bool force_idx64, hipStream_t stream);
// Path recorder (cbet_trace_path.hip): launch_trace with variant kTracePaths and the second block runs it, one wavefront
// per 64 items of q, after the same bounds-audit set-up.
constexpr int kTracePaths = 101;
hipError_t launch_trace_path(const TraceArgs &a, const PathArgs &q, bool force_idx64, hipStream_t stream);
// Backscatter gain spectra (cbet_backscatter.hip): launch_trace with variant kTraceBackscatter and both blocks runs it, one
// wavefront per 64 items of q, after the same bounds-audit set-up.
constexpr int kTraceBackscatter = 102;
hipError_t launch_trace_backscatter(const TraceArgs &a, const GainArgs &g, const SbsArgs &q, bool force_idx64, hipStream_t stream);
hipError_t launch_exit_tally(const cbet_ray_exit *exits, long L, int nbeams, double *tally, hipStream_t stream);
hipError_t launch_farfield(const cbet_ray_exit *exits, long n, int ntheta, int nphi, double *hist, hipStream_t stream);
hipError_t launch_gain_field(const GainArgs &a, hipStream_t stream);
// k_pair_amplitude: the unclamped amplitude map of normalised fields over the planes [a.hx_lo, a.hx_hi) into amp[hsize]; a.sat is not read
hipError_t launch_pair_amplitude(const GainArgs &a, double *amp, hipStream_t stream);
// k_exchange_matrix + k_exchange_reduce: the pairwise exchange of normalised fields over the planes
// [a.hx_lo, a.hx_hi), added into out / gross ([nbeams][nbeams], gross may be NULL); a.sat is honoured.  work holds
// exchange_groups(rows) x 2 x nbeams (nbeams - 1) / 2 doubles, rows = planes x (ny + 2).
inline long exchange_groups(long rows) { return rows < CBET_EXCHANGE_MAX_GROUPS ? rows : CBET_EXCHANGE_MAX_GROUPS; }
hipError_t launch_exchange_matrix(const GainArgs &a, double *work, double *out, double *gross, hipStream_t stream);
hipError_t launch_pack_segments(const double *src, long beam_stride, int hy, int hz, const int *seg, long nseg, double *out,
                                hipStream_t stream);
hipError_t launch_unpack_segments(double *dst, long beam_stride, int hy, int hz, const int *seg, long nseg, const double *in,
                                  hipStream_t stream);
hipError_t launch_edep_average(const double *edep, double *out, int nx, int ny, int nz, hipStream_t stream);

// Spherical-harmonic mode spectra (cbet_sph_modes.hip).  Passed by value: the shell edges are
// captured at the call.
struct SphArgs {
    const double *edep;                     // [ngrids] grids grid_stride doubles apart, or NULL (geometry mode: E = 1)
    long grid_stride;                       // doubles between grids
    long row_pitch;                         // doubles per (I, J) row: nz + 2 or cbet_params.edep_zpitch
    int ngrids, nx, ny, nz;
    int nshell, lmax;
    double xmin, ymin, zmin, dx, dy, dz;
    double cx, cy, cz;                      // centre
    double *coeffs;                         // [ngrids][nshell][(lmax+1)^2], overwritten
    double *shell_energy;                   // [ngrids][nshell], overwritten
    long long *shell_nodes;                 // [nshell], overwritten
    double r_edges[CBET_SPH_MAX_SHELLS + 1];
};
hipError_t launch_sph_modes(const SphArgs &a, hipStream_t stream);

// Perturbed targets (cbet_target.hip, cbet_target_host.cpp, cbet_target_model.h).
// The factor table F of the header's contract, computed once on the host (target_factors) and read by the two kernels (from
// constant memory, target_upload_factors) and by the host twins alike:
//   [kTfY00] 1/sqrt(4 pi), [kTfSqrt2] sqrt(2), [kTfD + k] d_k, [kTfA + l * kTargetS + m] a_lm, [kTfB + ...] b_lm
constexpr int kTargetS = CBET_TARGET_LMAX + 1;
constexpr int kTargetCoeffs = kTargetS * kTargetS;
constexpr int kTfY00 = 0, kTfSqrt2 = 1, kTfD = 2, kTfA = kTfD + kTargetS, kTfB = kTfA + kTargetCoeffs,
              kTargetFactors = kTfB + kTargetCoeffs;
const double *target_factors();                      // host table, filled on first use
hipError_t target_upload_factors();                  // host table -> the current device's constant memory (synchronous)
// Passed by value: offset and coefficients are captured at the call (zero beyond the call's lmax).
struct TargetArgs {
    TabulateArgs t;
    double ox, oy, oz;
    double c[kTargetCoeffs];
};
// Argument checks of both entry points; *inst = the instantiation (0, 2, 8 or 16) that covers the non-zero coefficients.
int target_check(const cbet_target *target, int *inst);
void target_fill(const cbet_target *target, TargetArgs *a);   // offset and coefficients into *a
hipError_t launch_tabulate_target(const TargetArgs &a, int inst, hipStream_t stream);

// Flow table of the gain kernels on a target (cbet_target.hip, cbet_target_host.cpp, cbet_target_model.h target_flow;
// DESIGN.md section 13).  Passed by value like TargetArgs; c sits last, as the kernel reads it from the argument segment.
struct FlowArgs {
    int nx, ny, nz;
    double xmin, ymin, zmin, dx, dy, dz;
    double cs, mach_r0, mach_0, mach_r1, mach_1;
    double *flow;                           // out, [3][nx*ny*nz]: ux, uy, uz
    double ox, oy, oz;
    double c[kTargetCoeffs];
};
hipError_t launch_tabulate_flow(const FlowArgs &a, int inst, hipStream_t stream);

// Plasma on a spherical-polar mesh (cbet_mesh.hip, cbet_mesh_host.cpp, cbet_mesh_model.h).
// The kernels stage r, theta and phi in LDS; CBET_MESH_MAX_COORDS doubles (20 KiB) let eight 256-thread workgroups share
// a CU's 160 KiB, which is the 32 waves a CU holds at most: the staging never costs occupancy.
// The node-independent factors of the state model (cbet_state_model.h), cbet_gain_constants' own: E2 = pow(estat, 2),
// A = 4 (1.0e3 me) c omega kb, F = 8 pi 1.0e7 / c and the ion mass in kg.
struct StateConsts {
    double e2, a, f, mi_kg;
};
struct MeshArgs {
    int nx, ny, nz;
    double xmin, ymin, zmin, dx, dy, dz, dt;
    double ncrit;
    double ox, oy, oz;                      // the mesh's centre
    int nr, nth, nph;
    const double *r, *theta, *phi;          // nr, nth, nph node coordinates
    const double *ne, *te;                  // [nr][nth][nph], phi fastest
    const double *ur, *uth, *uph;           // the same shape, each may be NULL (zero)
    double *ne3d, *kap3d;                   // out of the table kernel, nx*ny*nz each
    double *flow;                           // out of the flow kernel, [3][nx*ny*nz]: ux, uy, uz
    // the state kernel's (appended: the members above keep their places)
    const double *ti, *zbar;                // the fields' shape, each may be NULL (ti0 / z0 everywhere)
    double ti0, z0;                         // cbet_gain_params.ti_ev / z_ion
    StateConsts sc;
    double *state;                          // out of the state kernel, [2][nx*ny*nz]: cs, gain_const
};
hipError_t launch_tabulate_mesh(const MeshArgs &a, hipStream_t stream);   // k_tabulate_mesh: a.ne3d / a.kap3d
hipError_t launch_mesh_flow(const MeshArgs &a, hipStream_t stream);       // k_mesh_flow: a.flow
hipError_t launch_mesh_state(const MeshArgs &a, hipStream_t stream);      // k_mesh_state: a.state

// Deposit on the hydro mesh (cbet_mesh_deposit.hip, cbet_mesh_deposit_host.cpp, cbet_mesh_deposit_model.h; DESIGN.md
// section 15).  The four lookup tables are the handle's: device copies for the kernel, host copies for the twin.
struct MeshDepositArgs {
    const double *edep;                     // [ngrids] haloed grids grid_stride doubles apart, or NULL (counts only)
    long grid_stride, row_pitch;            // doubles between grids / per (I, J) row
    int ngrids, nx, ny, nz;
    double xmin, ymin, zmin, dx, dy, dz;
    double ox, oy, oz;                      // the cells' centre
    int nr, nth, nph;                       // cells
    int S;                                  // sub-samples per axis
    double inv;                             // 1.0 / (S*S*S)
    const double *re, *ct, *pe, *off;       // r_edges [nr+1], cos of the interior theta edges [nth-1], diamond angles of the first nph phi edges, offsets [S]
    double *cell_energy, *outside;          // [ngrids][nr][nth][nph], [ngrids]; launch_mesh_deposit zeroes them first
    long long *cell_samples;                // [nr][nth][nph]; likewise
    int chunk;                              // grids per workgroup: blockIdx.y takes the chunk-th part of the stack
};
constexpr int kMeshDepositChunks = 8;               // the LDS arm splits a stack into at most this many parts
constexpr size_t kMeshDepositLds = 40960;           // ... and takes at most this much LDS: four workgroups per CU
size_t mesh_deposit_lds(const MeshDepositArgs &a, bool lds_arm);   // dynamic LDS of a launch with a.chunk, bytes
hipError_t launch_mesh_deposit(const MeshDepositArgs &a, bool lds_arm, hipStream_t stream);

}  // namespace cbet
#endif
