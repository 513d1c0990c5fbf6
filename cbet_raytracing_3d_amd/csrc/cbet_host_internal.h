// cbet_host_internal.h -- what the host .cpp files share and nothing outside them sees: the error helpers, the device
// guard, the per-device context, the checks every entry point starts with and ONE builder per kernel argument block
// (a device kernel and its host twin run the same statements on arguments filled by the same function).
#ifndef CBET_HOST_INTERNAL_H_
#define CBET_HOST_INTERNAL_H_

#include <hip/hip_runtime_api.h>

#include <vector>

#include "cbet_device.h"
#include "cbet_mi355x.h"

struct cbet_context {
    int gpu = -1;
    cbet_params p{};
    cbet_derived d{};
    double *ne3d = nullptr, *kap3d = nullptr;
    cbet::StepRecord *steprec = nullptr;  // per-node step records of the LDS_WINDOW kernel (cbet_device.h)
    // what the records were built from: valid while the context's own tables are unchanged (tables_version)
    unsigned long long tables_version = 0, rec_version = ~0ull;
    unsigned long long rec_builds = 0;  // launches that wrote the records (cbet_context_step_records)
    const double *rec_ne3d = nullptr, *rec_kap3d = nullptr;
    double rec_const[3] = {0, 0, 0};
    double *xlaunch = nullptr, *ylaunch = nullptr;
    double *bounds = nullptr;  // {xlo,xhi,ylo,yhi,zlo,zhi}
    int *live = nullptr;
    int nlive = 0;  // launch-list slots (64 per bundle, holes included)
    unsigned long long *counters = nullptr;
    // flow table of the gain kernels (cbet_tabulate_flow / cbet_context_set_flow): NULL = the closed-form ramp
    double *flow_own = nullptr;         // the context's own [3][nx*ny*nz] table, allocated by the first cbet_tabulate_flow
    const double *flow = nullptr;       // the table in use: flow_own, a caller's, or NULL
    // state table of the gain kernels (cbet_tabulate_mesh_state / cbet_context_set_state): NULL = the scalars cs, gain_const
    double *state_own = nullptr;        // the context's own [2][nx*ny*nz] table, allocated by the first cbet_tabulate_mesh_state
    const double *state = nullptr;      // the table in use: state_own, a caller's, or NULL
    // limit of the ion-acoustic amplitude in the gain kernels (cbet_context_set_saturation): 0 = none
    double dn_max = 0.0;
    // per-beam frequency shifts of the gain kernels (cbet_context_set_detuning): NULL = one colour
    double *shift_own = nullptr;        // the context's own [CBET_MAX_CBET_BEAMS] table, allocated by the first cbet_context_set_detuning that selects shifts
    const double *shift = nullptr;      // the table in use: shift_own, or NULL
    double shift_host[CBET_MAX_CBET_BEAMS] = {};   // what shift_own holds (cbet_context_detuning)
    // polarization mode of the gain kernels (cbet_context_set_polarization): CBET_POL_ALIGNED = every pair polarized alike
    int pol = CBET_POL_ALIGNED;
    // line spectrum of the gain kernels (cbet_context_set_bandwidth): NULL = monochromatic beams
    double *band_own = nullptr;         // the context's own device block, allocated by the first cbet_context_set_bandwidth that selects lines:
                                        // the difference table [1 + 2 M_max] and behind it CBET_MAX_CBET_BEAMS zeros, the shifts of a context without detuning
    const double *band = nullptr;       // the table in use: band_own, or NULL
    int nband = 0;                      // its entries M
    int nlines = 0;                     // the lines in use and their offsets and normalised weights (cbet_context_bandwidth)
    double line_domega[CBET_MAX_BAND_LINES] = {}, line_weight[CBET_MAX_BAND_LINES] = {};
};

namespace cbet {
#pragma GCC visibility push(hidden)   // internal: none of these is an exported symbol

// fail (cbet_params.cpp) only records the text, so that file links without the HIP runtime.  HIP keeps its last error
// sticky until read, and a reported failure must not leak into the caller's (or torch's) next hipGetLastError() check:
// every return of CBET_EHIP, CBET_ENODEVICE or CBET_ENOMEM goes through fail_hip, which reads it away.
int fail(int code, const char *fmt, ...);
template <class... Values>
int fail_hip(int code, const char *fmt, Values... values)
{
    (void)hipGetLastError();
    return fail(code, fmt, values...);
}

#define CBET_HIP(call)                                                                          \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return ::cbet::fail_hip(CBET_EHIP, "%s failed: %s", #call, hipGetErrorString(e_));  \
    } while (0)

// Restores the caller's current device on scope exit (moveToAndFromGPU's save/restore, multi_gpu.cpp:50-57);
// clear_sticky: and leaves no sticky HIP error behind, whatever happened in the scope (cbet_ray_tracing).
struct DeviceGuard {
    int saved = -1;
    bool clear_sticky;
    explicit DeviceGuard(bool clear = false) : clear_sticky(clear) { if (hipGetDevice(&saved) != hipSuccess) saved = -1; }
    ~DeviceGuard()
    {
        if (saved >= 0) (void)hipSetDevice(saved);
        if (clear_sticky) (void)hipGetLastError();
    }
};

// For the rest of the scope the context's device is current; the caller's comes back on scope exit.
#define CBET_ENTER_DEVICE(context)                                                                                        \
    ::cbet::DeviceGuard device_guard_;                                                                                    \
    if (hipError_t e_ = hipSetDevice((context)->gpu))                                                                     \
        return ::cbet::fail_hip(CBET_EHIP, "hipSetDevice(ctx->gpu) failed: %s", hipGetErrorString(e_))

// ---- cbet_params.cpp (no HIP call) ----------------------------------------------------------------------
int validate(const cbet_params *p);
int validate_gain(const cbet_params *p, const cbet_gain_params *g);
// validate, the derived constants and the "no threads per beam" refusal, without the launch list that cbet_derive builds
// and sorts (ntraced_ids and nlive_rays stay 0); derive_launch: with both launch axes and the list.
int derive_grid(const cbet_params *p, cbet_derived *d);
int derive_launch(const cbet_params *p, cbet_derived *d, std::vector<double> &xl, std::vector<double> &yl,
                  std::vector<int> &live);
// The state model's four host factors (cbet_state_model.h), beside cbet_gain_constants; validates p and g.
int state_consts(const cbet_params *p, const cbet_gain_params *g, StateConsts *out);

// ---- cbet_context.cpp -------------------------------------------------------------------------------------
int check_geometry(const cbet_context *ctx, const cbet_params *p);  // the launch describes the geometry ctx was sized for
int entry_checks(const cbet_context *ctx, const cbet_params *p);    // ctx != NULL, validate(p), check_geometry: in that order
int default_context(const cbet_params *p, cbet_context **out);      // the calling thread's device's own, for ctx == NULL

// ---- one builder per argument block -------------------------------------------------------------------------
// The nine grid scalars of TabulateArgs, TraceArgs, GainArgs, FlowArgs and SphArgs (grid_dims: StepTableArgs' three).
template <class Args>
void grid_dims(Args &a, const cbet_params *p)
{
    a.nx = p->nx; a.ny = p->ny; a.nz = p->nz;
}
template <class Args>
void grid_args(Args &a, const cbet_params *p, const cbet_derived &d)
{
    grid_dims(a, p);
    a.xmin = p->xmin; a.ymin = p->ymin; a.zmin = p->zmin;
    a.dx = d.dx; a.dy = d.dy; a.dz = d.dz;
}
// The Mach ramp of radial_flow (cbet_node_model.h) and the sound speed it scales: GainArgs' and FlowArgs'.
template <class Args>
void ramp_args(Args &a, const cbet_gain_params *g, double cs)
{
    a.cs = cs;
    a.mach_r0 = g->mach_r0; a.mach_0 = g->mach_0; a.mach_r1 = g->mach_r1; a.mach_1 = g->mach_1;
}
// The six exit planes {xlo, xhi, ylo, yhi, zlo, zhi} of launch_ray_XZ.cu:352-354, xmin - (dx / 2.0), xmax + (dx / 2.0), ...:
// ONE statement for the array context_create uploads (cbet_context::bounds) and for TraceArgs::exit_planes.
inline void host_exit_planes(const cbet_params *p, const cbet_derived &d, double out[6])
{
    out[0] = p->xmin - (d.dx / 2.0); out[1] = p->xmax + (d.dx / 2.0);
    out[2] = p->ymin - (d.dy / 2.0); out[3] = p->ymax + (d.dy / 2.0);
    out[4] = p->zmin - (d.dz / 2.0); out[5] = p->zmax + (d.dz / 2.0);
}
// The host twins' walk over the nodes, in node order: body(i, j, k, idx) with idx = (i * ny + j) * nz + k.
template <class Body>
void for_each_node_host(int nx, int ny, int nz, Body body)
{
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < ny; ++j)
            for (int k = 0; k < nz; ++k) body(i, j, k, ((long)i * ny + j) * nz + k);
}
// k_tabulate's and its host twin's (cbet_tables_abi.cpp); the twin passes the profiles beside the block.
TabulateArgs tabulate_args(const cbet_params *p, const cbet_derived &d, double *ne3d, double *kap3d, const double *te,
                           const double *r, const double *ne);
// k_tabulate_flow's and its host twin's (cbet_target_host.cpp); target NULL = the sphere about the origin.
FlowArgs flow_args(const cbet_params *p, const cbet_derived &d, const cbet_gain_params *g, double cs,
                   const cbet_target *target, double *out);
// k_tabulate_mesh's, k_mesh_flow's, k_mesh_state's and their host twins' (cbet_mesh_host.cpp): the outputs a launch does
// not write stay NULL.  mesh_state_args: the state kernel's members on top (ions may be NULL).
MeshArgs mesh_args(const cbet_params *p, const cbet_derived &d, const cbet_mesh *mesh, double *ne3d, double *kap3d,
                   double *flow);
MeshArgs mesh_state_args(const cbet_params *p, const cbet_derived &d, const cbet_gain_params *g, const StateConsts &sc,
                         const cbet_mesh *mesh, const cbet_mesh_ions *ions, double *state);
// The mesh's sizes and NULL pointers (all a device entry can check); whole: the values too (HOST arrays).
int mesh_check(const cbet_mesh *mesh, bool whole);
// The gain kernels', k_pair_amplitude's, k_exchange_matrix's and its host twin's (cbet_exchange_host.cpp).  cs, gc: cbet_gain_constants';
// packed: the arrays hold the slab's planes only.  gain, scratch, change, consume and frozen stay zero: the gain update sets them.
// The options reach the block in ONE record, from a context (context_gain_options) or from the twin's arguments.
constexpr int kBandMax = CBET_MAX_BAND_LINES * (CBET_MAX_BAND_LINES - 1) / 2;
// What a gain-stage launch (or the host twin) reads beside fields and ne3d: GainArgs' members of the same names.  shift: a table
// of CBET_MAX_CBET_BEAMS doubles, band: band_table's of nband entries (device memory for a kernel, the host's for the twin), or NULL.
struct GainOptions {
    const double *flow = nullptr, *state = nullptr;
    double sat = 0.0;
    const double *shift = nullptr;
    int pol = CBET_POL_ALIGNED;
    const double *band = nullptr;
    int nband = 0;
};
GainArgs gain_args(const cbet_params *p, const cbet_derived &d, const cbet_gain_params *g, double cs, double gc,
                   const double *fields, const double *ne3d, const GainOptions &o, int hx_lo, int hx_hi, bool packed);
// The ONE rule of the zero shifts, for whoever fills a GainOptions: a block with a spectrum always carries shifts too (the BAND
// arms of the kernels run the DETUNE statements with dw = 0), the given ones or `zeros`.
inline void carry_shifts(GainOptions &o, const double *zeros) { if (o.band && !o.shift) o.shift = zeros; }
// A context's options, as every device entry of the gain stage launches with them (zeros: behind band_own's table).
inline GainOptions context_gain_options(const cbet_context *ctx)
{
    GainOptions o;
    o.flow = ctx->flow; o.state = ctx->state; o.sat = ctx->dn_max; o.shift = ctx->shift; o.pol = ctx->pol; o.band = ctx->band; o.nband = ctx->nband;
    carry_shifts(o, ctx->band_own ? ctx->band_own + (1 + 2 * kBandMax) : nullptr);
    return o;
}
// The line spectrum of the gain stage (cbet_exchange_host.cpp, no HIP call).  band_check: the refusals of
// cbet_context_set_bandwidth and of the banded twin, `who` in front.  band_table: the difference table of nlines valid lines
// into table[1 + 2 kBandMax] = {c_0, d_0, c_0', ...} and the normalised weights into norm[nlines] (or NULL); returns M.
int band_check(const char *who, const double *line_domega, const double *line_weight, int nlines);
int band_table(const double *line_domega, const double *line_weight, int nlines, double *table, double *norm);
// The slab [hx_lo, hx_hi) lies in the haloed grid; who: the entry point's name and ": " in front of the message, or "".
int slab_check(const char *who, int hx_lo, int hx_hi, const cbet_params *p);
// k_lpi_map's and its host twin's (cbet_lpi_host.cpp, no HIP call).  lpi_check: the refusals both
// entries share, `who` in front, and the derived constants into *d; lpi_args: the block (ne3d: the table in use).
struct LpiArgs;
int lpi_check(const char *who, const double *fields, const double *te3d, double te_ev, double frac_lo, double frac_hi,
              int cone_bins, const double *lpi, int hx_lo, int hx_hi, const cbet_params *p, cbet_derived *d);
LpiArgs lpi_args(const cbet_params *p, const cbet_derived &d, const double *fields, const double *ne3d, const double *te3d,
                 double te_ev, double frac_lo, double frac_hi, int cone_bins, double *lpi, int hx_lo, int hx_hi);
// the grid of k_lpi_map for a slab: four bricks per workgroup up to CBET_LPI_MAX_GROUPS, from the slab alone
long lpi_groups(const cbet_params *p, int hx_lo, int hx_hi);
// k_lpi_map over the block's planes with `groups` workgroups; summary != NULL: the workgroups' partial summaries into
// work[groups], then k_lpi_reduce merges them into *summary in workgroup order (cbet_lpi.hip)
hipError_t launch_lpi_map(const LpiArgs &a, cbet_lpi_summary *summary, cbet_lpi_summary *work, long groups, hipStream_t stream);
// k_trace_backscatter's third block and its host twin's (cbet_backscatter_host.cpp, no HIP call).
// sbs_check: the refusals both entries share, `who` in front, each naming the first offence; sbs_args: the block, beside a
// GainArgs of gain_args (whole grid) whose k0, dt, iaw and nbeams it reads.  The twin passes no raynums (nrays 0).
int sbs_check(const char *who, long nitems, const int *beams, const double *fields, const double *shifts, int nshift,
              const double *gamma, const cbet_ray_sbs *rays, const cbet_params *p, const cbet_gain_params *g);
SbsArgs sbs_args(const GainArgs &g, const int *beams, const int *raynums, long nitems, int nrays, const double *shifts, int nshift,
                 double *gamma, cbet_ray_sbs *rays);
// The refusals the Anderson-mixing entries share with their host twins (cbet_mix_host.cpp, no HIP call),
// `who` in front, each naming the first offence.
int mix_residual_check(const char *who, const double *y, const double *x, const double *f, const double *const *f_held, int h,
                       long n, const double *row);
int mix_apply_check(const char *who, const double *const *y_held, const double *alpha, int count, long n, const double *x_out);

// ---- launches that cross files (cbet_tables_abi.cpp, cbet_trace_abi.cpp, cbet_gain_abi.cpp) ---------------------
// The context's own device table of `doubles` doubles (own_node_table: `components` per node) in *slot, allocated on the first call (not capturable).
int own_table(double **slot, size_t doubles, const char *what);
inline int own_node_table(double **slot, const cbet_params *p, int components, const char *what) { return own_table(slot, (size_t)components * p->nx * p->ny * p->nz, what); }
inline int flow_own_table(cbet_context *ctx, const cbet_params *p) { return own_node_table(&ctx->flow_own, p, 3, "flow table"); }     // cbet_tabulate_flow, cbet_tabulate_mesh_flow
inline int state_own_table(cbet_context *ctx, const cbet_params *p) { return own_node_table(&ctx->state_own, p, 2, "state table"); }  // cbet_tabulate_mesh_state
int step_records(cbet_context *ctx, const cbet_params *p, const double *ne3d, const double *kappa3d, double xconst,
                 double yconst, double zconst, void *stream, bool force);
// CBET hooks of a trace launch (all zero: the reference path).
struct CbetHooks {
    const double *gain = nullptr;
    int quantity = 0;
    double *beam_gain = nullptr;
    double max_exponent = 0.0;
    bool exits = false;     // the exit pass (cbet_trace_exits): `edep` is the record array, no deposit
    const PathArgs *paths = nullptr;   // the path recorder (cbet_trace_paths): its second block; `edep` is the turn records, no deposit
    const SbsArgs *sbs = nullptr;      // the backscatter spectra (cbet_trace_backscatter): its third block and, in sbs_gain, its second;
    const GainArgs *sbs_gain = nullptr;   // `edep` is the ray records, no deposit
};
int trace_impl(int b, unsigned nindices, const double *ne3d, const double *kappa3d, double *edep, const double *bbeam_norm,
               const double *beam_norm, const double *pow_r, const double *phase_r, double xconst, double yconst,
               double zconst, const cbet_params *p, cbet_context *ctx, void *stream, const CbetHooks &hooks);
int gain_field_impl(double *fields, const double *ne3d, double *gain, double *scratch, double *change, int hx_lo, int hx_hi,
                    bool packed, const cbet_params *p, const cbet_gain_params *g, cbet_context *ctx, void *stream,
                    bool consume = false);

#pragma GCC visibility pop
}  // namespace cbet
#endif
