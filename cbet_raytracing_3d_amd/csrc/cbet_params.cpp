// cbet_params.cpp -- the part of the C ABI (include/cbet_mi355x.h) that is pure arithmetic: the error text, parameter
// validation and derivation, the launch-list builder, the host tables and the workspace sizes.  It makes no HIP runtime
// call (the HIP headers are included for their types only) and links without the HIP runtime, so it can be compiled and
// run on its own -- under sanitizers, tests/test_params_sanitizers.py.  Citations are into /root/reference/.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cbet_host_internal.h"
#include "cbet_omega_beams.h"

namespace cbet {

static thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int validate(const cbet_params *p)
{
    if (!p) return fail(CBET_EINVAL, "params is NULL");
    if (p->nx < 3 || p->ny < 3 || p->nz < 3) return fail(CBET_EINVAL, "grid needs >= 3 nodes per axis");
    if ((long)(p->nx + 2) * (p->ny + 2) * (p->nz + 2) >= 0x7FFFFFFFL)
        return fail(CBET_EINVAL, "grid too large for 32-bit node tags ((n+2)^3 must be < 2^31)");
    // the kernels build cell and haloed-node indices with 24-bit multiplies (v_mul_i32_i24): both operands of
    // (ci*ny + cj)*nz + ck and of X*(ny+2)(nz+2) + Y*(nz+2) + Z must stay below 2^23 (thin anisotropic grids)
    if ((long)p->nx * p->ny >= (1L << 23) || (long)(p->ny + 2) * (p->nz + 2) >= (1L << 23) || p->nx + 2 >= (1 << 23) ||
        p->nz + 2 >= (1 << 23))
        return fail(CBET_EINVAL, "grid too anisotropic for 24-bit index products (need nx*ny < 2^23 and (ny+2)(nz+2) < 2^23)");
    if (!(p->xmax > p->xmin) || !(p->ymax > p->ymin) || !(p->zmax > p->zmin))
        return fail(CBET_EINVAL, "empty extent");
    if (p->nbeams < 1) return fail(CBET_EINVAL, "nbeams < 1");
    if (p->rays_per_zone < 1 || p->rays_per_zone > 64) return fail(CBET_EINVAL, "rays_per_zone out of range");
    if (!(p->courant_mult > 0)) return fail(CBET_EINVAL, "courant_mult <= 0");
    // k_tabulate stages 3 * nprofile doubles in dynamic LDS; 2048 rows = 48 KB, inside the default limit
    if (p->nprofile < 2 || p->nprofile > 2048) return fail(CBET_EINVAL, "nprofile out of range [2,2048]");
    if (p->max_threads < 1 || p->threads_per_block < 1) return fail(CBET_EINVAL, "bad launch-shape rule");
    if (p->shard_count > 1 && (p->shard_index < 0 || p->shard_index >= p->shard_count))
        return fail(CBET_EINVAL, "shard_index outside [0, shard_count)");
    if (p->rim_merge != 0 && (p->rim_merge < 2 || p->rim_merge > 16))
        return fail(CBET_EINVAL, "rim_merge must be 0 (off) or a footprint of 2 .. 16 launch zones");
    if (p->edep_zpitch != 0 && (p->edep_zpitch < p->nz + 2 || (long)(p->ny + 2) * p->edep_zpitch >= (1L << 23) ||
                                (long)(p->nx + 2) * (p->ny + 2) * p->edep_zpitch >= 0x7FFFFFFFL))
        return fail(CBET_EINVAL, "edep_zpitch must be 0 (dense rows) or a row length >= nz + 2 that keeps the grid below 2^31 entries");
    return CBET_OK;
}

// def.cuh:33-131 and main.cu:156-161, evaluated operation by operation as written there.
static void derive_core(const cbet_params *p, cbet_derived *d)
{
    d->dx = (p->xmax - p->xmin) / (p->nx - 1);
    d->dy = (p->ymax - p->ymin) / (p->ny - 1);
    d->dz = (p->zmax - p->zmin) / (p->nz - 1);
    d->dt = p->courant_mult * std::min(d->dx, d->dz) / kC;           // def.cuh:81
    d->nt = (int)((1 / p->courant_mult) * p->nx * 2.0);               // def.cuh:83-84
    d->zones_spanned = (int)std::ceil((kBeamMax - kBeamMin) / d->dx); // launch_ray_XZ.cu:69
    d->nrays_x = (int)(p->rays_per_zone * std::ceil((kBeamMax - kBeamMin) / d->dx));
    d->nrays_y = (int)(p->rays_per_zone * std::ceil((kBeamMax - kBeamMin) / d->dy));
    d->nrays = d->nrays_x * d->nrays_y;
    const double freq = kC / kLambda;                                 // def.cuh:67
    d->omega = 2 * M_PI * freq;                                       // def.cuh:68
    d->ncrit = 1e-6 * (d->omega * d->omega) * kMe * kE0 / (kEc * kEc);// def.cuh:69
    d->uray_mult = kIntensity * (p->courant_mult) / (double(p->rays_per_zone * p->rays_per_zone));
    const double grad_const = std::pow(kC, 2) / (2.0 * d->ncrit) * d->dt * 0.5;  // main.cu:156
    d->xconst = grad_const / d->dx;
    d->yconst = grad_const / d->dy;
    d->zconst = grad_const / d->dz;
    const long total = (long)d->nrays * p->nbeams;                    // def.cuh:125-129
    const long nthreads = std::min<long>(p->max_threads, total);
    d->threads_per_beam = nthreads / p->nbeams;
    d->nindices = (int)std::ceil(d->nrays / (float)(d->threads_per_beam));
    d->grid_y = (int)(d->threads_per_beam / p->threads_per_block);    // main.cu:161
    d->edep_size = ((long)p->nx + 2) * ((long)p->ny + 2) * ((long)p->nz + 2);
    d->ntraced_ids = 0;
    d->nlive_rays = 0;
}

// launch_ray_XZ.cu:125,155-158 with main.cu:161's truncated grid.y: is thread-ray id visited?
static bool id_is_traced(const cbet_params *p, const cbet_derived *d, int nindices, long id)
{
    const long start = id % d->threads_per_beam, pass = id / d->threads_per_beam;
    return start < (long)d->grid_y * p->threads_per_block && pass < nindices;
}

// launch_ray_XZ.cu:76-92 : launch coordinate by repeated addition, then + d/2.
static std::vector<double> launch_axis(int count, int denom_count, double half_cell)
{
    std::vector<double> t(count);
    double acc = kBeamMin;
    for (int i = 0; i < count; ++i) {
        t[i] = acc + half_cell;
        acc += (kBeamMax - kBeamMin) / (denom_count - 1);
    }
    return t;
}

static unsigned morton2(unsigned x, unsigned y)
{
    auto spread = [](unsigned v) {
        v &= 0xFFFF;
        v = (v | (v << 8)) & 0x00FF00FF;
        v = (v | (v << 4)) & 0x0F0F0F0F;
        v = (v | (v << 2)) & 0x33333333;
        v = (v | (v << 1)) & 0x55555555;
        return v;
    };
    return spread(x) | (spread(y) << 1);
}

// The beam-independent launch list.  The beam cross-section (nrays_x x nrays_y rays,
// launch_ray_XZ.cu:69-74) is cut into 8x8-ray patches visited along a Morton curve; each patch is
// one ray bundle = one wavefront, lane = 8*row + column.  An entry is the thread-ray id the
// reference would give that ray (the inverse of :70-74's permutation), or -1 for a hole: a ray
// outside the ray grid, one the reference launch shape never visits (:155-158, main.cu:161), or one
// that fails init()'s beam-radius test (:94,114).  Patches with no live ray are dropped.
static void build_live_list(const cbet_params *p, const cbet_derived *d, int nindices,
                            const std::vector<double> &xl, const std::vector<double> &yl,
                            std::vector<int> &slots, long &ntraced, long &nlive)
{
    const int rpz = p->rays_per_zone, rpz2 = rpz * rpz;
    const int zx = d->zones_spanned;
    const int px = (d->nrays_x + 7) / 8, py = (d->nrays_y + 7) / 8;
    // Visit order of the patches.  patch_order 0: Morton curve (neighbouring patches consecutive).
    // patch_order 1 (default): longest rays first -- rays launched far from the beam axis cross the
    // whole box (~4x the steps of the central rays, which are absorbed early), and a launch is only
    // a few rounds of the chip once the work is sharded 8 ways, so dispatching the long bundles
    // first and the short ones last trims the tail.  Ties (and order 0) fall back to Morton.
    std::vector<std::pair<unsigned long long, int>> order;
    order.reserve((size_t)px * py);
    for (int y = 0; y < py; ++y)
        for (int x = 0; x < px; ++x) {
            unsigned long long key = morton2(x, y);
            if (p->patch_order != 0) {
                const int cx = std::min(d->nrays_x - 1, x * 8 + 4), cy = std::min(d->nrays_y - 1, y * 8 + 4);
                const double r2 = xl[cx] * xl[cx] + yl[cy] * yl[cy];
                const double rmax2 = 2.0 * kBeamMax * kBeamMax * 1.1;
                const double levels = p->patch_order == 1 ? 4095.0 : (double)(p->patch_order - 1);   // >= 2: that many radial rings, Morton inside each
                const unsigned long long ring = (unsigned long long)((1.0 - std::min(1.0, r2 / rmax2)) * levels);  // 0 = outermost
                key |= ring << 32;
            }
            order.emplace_back(key, y * px + x);
        }
    std::sort(order.begin(), order.end());
    slots.clear();
    ntraced = 0;
    nlive = 0;
    // ids the launch shape visits, counted once over the whole ray grid
    for (long id = 0; id < d->nrays; ++id)
        if (id_is_traced(p, d, nindices, id)) ++ntraced;
    struct RimRay {
        double angle;
        int id, rx, ry;
    };
    // cbet_params.rim_merge: patches on the rim of the beam hold fewer than 64 live rays, and those rays cross the whole
    // box -- the longest bundles would run with idle lanes (256^3: 144 of 1620 bundles, lane utilisation 0.907).  The rays
    // of all partial patches are pooled, walked by their angle around the beam axis and cut into bundles of up to 64 rays
    // whose footprint stays within rim_merge launch zones per axis (4 = 16 rays: 76 bundles instead of 144, 0.957).  A
    // ray keeps the lane of its patch position where that lane is free, so rays that share a zone still differ in the
    // lane bits that pick the corner order.  The rim bundles -- the longest rays -- head the list.
    const int merge_w = p->rim_merge > 0 ? std::max(8, p->rim_merge * rpz) : 0;   // in rays, never narrower than a patch
    std::vector<RimRay> pool;
    std::vector<int> full;                // the whole patches, in visit order
    std::vector<int> partial;             // the rim patches as they are (kept if packing them gains nothing)
    std::vector<int> packed;
    for (auto &o : order) {
        const int bx = (o.second % px) * 8, by = (o.second / px) * 8;
        int patch[kWave];
        int alive = 0;
        for (int l = 0; l < kWave; ++l) {
            const int rx = bx + (l & 7), ry = by + (l >> 3);
            patch[l] = -1;
            if (rx >= d->nrays_x || ry >= d->nrays_y) continue;
            const long tile = (long)(ry / rpz) * zx + rx / rpz;           // inverse of :72-73
            const long id = tile * rpz2 + (ry % rpz) * rpz + rx % rpz;    // inverse of :70-71
            if (id >= d->nrays || !id_is_traced(p, d, nindices, id)) continue;
            const double ref = std::sqrt(xl[rx] * xl[rx] + yl[ry] * yl[ry]);
            if (!(ref <= kBeamMax)) continue;
            patch[l] = (int)id;
            ++alive;
        }
        if (!alive) continue;
        nlive += alive;
        if (merge_w > 0 && alive < kWave) {
            partial.insert(partial.end(), patch, patch + kWave);
            for (int l = 0; l < kWave; ++l)
                if (patch[l] >= 0) {
                    const int rx = bx + (l & 7), ry = by + (l >> 3);
                    pool.push_back({std::atan2(ry - 0.5 * (d->nrays_y - 1), rx - 0.5 * (d->nrays_x - 1)), patch[l], rx, ry});
                }
        } else {
            full.insert(full.end(), patch, patch + kWave);
        }
    }
    std::sort(pool.begin(), pool.end(), [](const RimRay &u, const RimRay &v) { return u.angle != v.angle ? u.angle < v.angle : u.id < v.id; });
    for (size_t s0 = 0; s0 < pool.size();) {
        size_t e = s0;
        int x0 = pool[s0].rx, x1 = x0, y0 = pool[s0].ry, y1 = y0;
        while (e < pool.size() && e - s0 < (size_t)kWave) {
            const int nx0 = std::min(x0, pool[e].rx), nx1 = std::max(x1, pool[e].rx), ny0 = std::min(y0, pool[e].ry), ny1 = std::max(y1, pool[e].ry);
            if (nx1 - nx0 + 1 > merge_w || ny1 - ny0 + 1 > merge_w) break;
            x0 = nx0; x1 = nx1; y0 = ny0; y1 = ny1;
            ++e;
        }
        int bundle[kWave];
        for (int l = 0; l < kWave; ++l) bundle[l] = -1;
        std::vector<int> extra;           // rays whose own lane is taken
        for (size_t k = s0; k < e; ++k) {
            const int l = (pool[k].rx & 7) + 8 * (pool[k].ry & 7);
            if (bundle[l] < 0) bundle[l] = pool[k].id;
            else extra.push_back(pool[k].id);
        }
        for (int l = 0, q = 0; l < kWave && q < (int)extra.size(); ++l)
            if (bundle[l] < 0) bundle[l] = extra[q++];
        packed.insert(packed.end(), bundle, bundle + kWave);
        s0 = e;
    }
    const std::vector<int> &rim = packed.size() < partial.size() ? packed : partial;
    slots.insert(slots.end(), rim.begin(), rim.end());
    slots.insert(slots.end(), full.begin(), full.end());
}

int derive_grid(const cbet_params *p, cbet_derived *d)
{
    if (int rc = validate(p)) return rc;
    derive_core(p, d);
    if (d->threads_per_beam < 1) return fail(CBET_EINVAL, "no threads per beam");
    return CBET_OK;
}

// Everything a launch shape implies, in one place: the derived constants, both launch axes and the launch list
// (with cbet_derived.ntraced_ids / nlive_rays filled from it).  Callers that owe their caller another check between
// validate's and these validate first themselves; a second pass over valid parameters changes nothing.
int derive_launch(const cbet_params *p, cbet_derived *d, std::vector<double> &xl, std::vector<double> &yl,
                  std::vector<int> &live)
{
    if (int rc = derive_grid(p, d)) return rc;
    xl = launch_axis(d->nrays_x, d->nrays_x, d->dx / 2);
    yl = launch_axis(d->nrays_y, d->nrays_y, d->dy / 2);
    long ntraced = 0, nlive = 0;
    build_live_list(p, d, d->nindices, xl, yl, live, ntraced, nlive);
    d->ntraced_ids = ntraced;
    d->nlive_rays = nlive;
    return CBET_OK;
}

// The CBET stage's parameters (parity unpinned -- see the header); p has passed validate.
int validate_gain(const cbet_params *p, const cbet_gain_params *g)
{
    if (!g) return fail(CBET_EINVAL, "gain params is NULL");
    if (p->nbeams > CBET_MAX_CBET_BEAMS) return fail(CBET_EINVAL, "the CBET stage supports at most %d beams", CBET_MAX_CBET_BEAMS);
    if (!(g->max_exponent > 0.0 && g->max_exponent <= 1.0)) return fail(CBET_EINVAL, "max_exponent must be in (0, 1]");
    if (!(g->relax > 0.0 && g->relax <= 1.0)) return fail(CBET_EINVAL, "relax must be in (0, 1]");
    if (!(g->iaw > 0.0) || !(g->z_ion > 0.0) || !(g->te_ev > 0.0) || !(g->ti_ev >= 0.0) || !(g->mi_over_me > 0.0))
        return fail(CBET_EINVAL, "bad plasma constants in gain params");
    if (!(g->mach_r1 > g->mach_r0)) return fail(CBET_EINVAL, "mach_r1 must exceed mach_r0");
    if (g->direction_passes < 1) return fail(CBET_EINVAL, "direction_passes must be >= 1");
    return CBET_OK;
}

}  // namespace cbet

using namespace cbet;

extern "C" {

const char *cbet_last_error(void) { return g_err; }
const char *cbet_version(void) { return "cbet-mi355x 0.1 (gfx950, hip)"; }

int cbet_params_default(cbet_params *p, int n)
{
    if (!p) return fail(CBET_EINVAL, "params is NULL");
    std::memset(p, 0, sizeof *p);
    p->nx = p->ny = p->nz = n;
    p->xmin = p->ymin = p->zmin = -0.13;
    p->xmax = p->ymax = p->zmax = 0.13;
    p->nbeams = 60;
    p->rays_per_zone = 4;
    p->courant_mult = 0.5;
    p->absorption = 1;
    p->nprofile = 443;
    p->max_threads = 120000000;
    p->threads_per_block = 256;
    p->ngpus = 1;
    p->beam_lo = 0;
    p->beam_hi = CBET_BEAMS_BY_GPU;
    p->shard_index = 0;
    p->shard_count = 1;
    p->kernel_variant = CBET_KERNEL_DEFAULT;
    p->patch_order = 1;
    p->rim_merge = 4;
    return CBET_OK;
}

int cbet_derive(const cbet_params *p, cbet_derived *d)
{
    if (int rc = validate(p)) return rc;
    if (!d) return fail(CBET_EINVAL, "derived is NULL");
    std::vector<double> xl, yl;
    std::vector<int> live;
    return derive_launch(p, d, xl, yl, live);
}

int cbet_live_ray_list(const cbet_params *p, int *out, long cap, long *count)
{
    if (int rc = validate(p)) return rc;
    if (!count) return fail(CBET_EINVAL, "count is NULL");
    cbet_derived d;
    std::vector<double> xl, yl;
    std::vector<int> live;
    if (int rc = derive_launch(p, &d, xl, yl, live)) return rc;
    *count = (long)live.size();
    if (out)
        for (long i = 0; i < std::min<long>(cap, (long)live.size()); ++i) out[i] = live[i];
    return CBET_OK;
}

const double *cbet_omega60_beam_norm(void) { return &cbet_omega60_ports[0][0]; }

int cbet_host_power_table(double *phase_r, double *pow_r)
{
    if (!phase_r || !pow_r) return fail(CBET_EINVAL, "NULL table");
    // main.cu:24-32 span(0.0, 0.1, 2001): running sum
    const double step = (0.1 - 0.0) / (CBET_NPHASE - 1);
    double acc = 0.0;
    for (unsigned i = 0; i < CBET_NPHASE; ++i) {
        phase_r[i] = acc;
        acc += step;
    }
    for (unsigned i = 0; i < CBET_NPHASE; ++i)  // main.cu:108-110
        pow_r[i] = std::exp(-1 * std::pow(std::pow((phase_r[i] / kSigma), 2), (5.0 / 2.0)));
    return CBET_OK;
}

int cbet_host_beam_trig(const double *beam_norm, int nbeams, double *bbeam_norm)
{
    if (!beam_norm || !bbeam_norm || nbeams < 1) return fail(CBET_EINVAL, "bad beam table");
    for (int b = 0; b < nbeams; ++b) {  // main.cu:122-129
        const double theta1 = std::acos(beam_norm[3 * b + 2]);
        const double theta2 = std::atan2(beam_norm[3 * b + 1] * kFocal, beam_norm[3 * b + 0] * kFocal);
        bbeam_norm[4 * b] = std::cos(theta1);
        bbeam_norm[4 * b + 1] = std::sin(theta1);
        bbeam_norm[4 * b + 2] = std::cos(theta2);
        bbeam_norm[4 * b + 3] = std::sin(theta2);
    }
    return CBET_OK;
}

int cbet_read_profile(const char *path, int nprofile, double *r, double *v)
{
    if (!path || !r || !v || nprofile < 1) return fail(CBET_EINVAL, "bad profile arguments");
    FILE *f = std::fopen(path, "r");
    if (!f) return fail(CBET_EINVAL, "cannot open profile file %s", path);
    for (int i = 0; i < nprofile; ++i) {  // main.cu:251-252: exactly nr rows
        if (std::fscanf(f, "%lf %lf", &r[i], &v[i]) != 2) {
            std::fclose(f);
            return fail(CBET_EINVAL, "profile file %s has fewer than %d rows", path, nprofile);
        }
    }
    std::fclose(f);
    return CBET_OK;
}

int cbet_gain_params_default(cbet_gain_params *g)
{
    if (!g) return fail(CBET_EINVAL, "gain params is NULL");
    std::memset(g, 0, sizeof *g);
    g->z_ion = 3.1;           // def.cuh:100
    g->te_ev = 2.0e3;         // def.cuh:104
    g->ti_ev = 1.0e3;         // def.cuh:106
    g->mi_over_me = 10230.0;  // def.cuh:101-102
    g->iaw = 0.2;             // def.cuh:107
    g->mach_r0 = 0.04; g->mach_0 = 0.4;   // def.cuh:114 names an undefined `machnum`; a radial ramp stands in
    g->mach_r1 = 0.13; g->mach_1 = 2.4;
    g->max_exponent = 1.0;
    g->relax = 0.5;           // plain fixed-point iteration (1.0) oscillates with 60 overlapping beams (scripts/cbet_converge.py)
    g->tolerance = 1e-4;
    g->max_passes = 40;
    g->direction_passes = 1;  // ray paths do not depend on the gain: the direction field of the gain-free first pass is kept
    return CBET_OK;
}

int cbet_gain_constants(const cbet_params *p, const cbet_gain_params *g, double *constant1, double *cs,
                        double *gain_const)
{
    if (int rc = validate(p)) return rc;
    if (int rc = validate_gain(p, g)) return rc;
    cbet_derived d;
    derive_core(p, &d);
    const double estat = 4.80320427e-10;            // def.cuh:98
    const double kb = 1.3806485279e-16;             // def.cuh:108
    const double te_k = g->te_ev * 11604.5052;      // def.cuh:103
    const double ti_k = g->ti_ev * 11604.5052;      // def.cuh:105
    const double mi_kg = g->mi_over_me * kMe;       // def.cuh:102
    const double c1 = (std::pow(estat, 2)) / (4 * (1.0e3 * kMe) * kC * d.omega * kb * te_k * (1 + 3 * ti_k / (g->z_ion * te_k)));  // def.cuh:111
    const double sound = 1e2 * std::sqrt(kEc * (g->z_ion * g->te_ev + 3.0 * g->ti_ev) / mi_kg);                                   // def.cuh:113
    if (constant1) *constant1 = c1;
    if (cs) *cs = sound;
    if (gain_const) *gain_const = c1 * (8.0 * M_PI * 1.0e7 / kC);  // |E|^2 = 8 pi 1e7 I / c
    return CBET_OK;
}

}  // extern "C"

// The node-independent factors of the state model (cbet_state_model.h), each computed as cbet_gain_constants above computes it.
int cbet::state_consts(const cbet_params *p, const cbet_gain_params *g, StateConsts *out)
{
    if (int rc = validate(p)) return rc;
    if (int rc = validate_gain(p, g)) return rc;
    cbet_derived d;
    derive_core(p, &d);
    const double estat = 4.80320427e-10;            // def.cuh:98
    const double kb = 1.3806485279e-16;             // def.cuh:108
    out->e2 = std::pow(estat, 2);
    out->a = 4 * (1.0e3 * kMe) * kC * d.omega * kb;
    out->f = 8.0 * M_PI * 1.0e7 / kC;
    out->mi_kg = g->mi_over_me * kMe;               // def.cuh:102
    return CBET_OK;
}

extern "C" {

size_t cbet_cbet_slab_workspace_bytes_parts(const cbet_params *p, int own_beams, int own_planes, size_t staging_doubles)
{
    if (!p || validate(p) != CBET_OK || own_beams < 0 || own_beams > p->nbeams || own_planes < 0 || own_planes > p->nx + 2) return 0;
    const size_t plane = (size_t)(p->ny + 2) * (p->nz + 2), hsize = (size_t)(p->nx + 2) * plane, nb = (size_t)p->nbeams;
    // own beams over the whole grid: 4 field components + gain; all beams over the own slab: 4 components + gain
    // (the pair-once gain kernel keeps its sums in LDS: no scratch array since round 3; the dense exchange sends from and
    // receives into these arrays: no staging since round 4)
    return (5 * (size_t)own_beams * hsize + 5 * nb * (size_t)own_planes * plane + staging_doubles + 2 + CBET_MAX_CBET_BEAMS) * sizeof(double);
}

size_t cbet_cbet_slab_workspace_bytes(const cbet_params *p, int world_size, int rank)
{
    if (!p || validate(p) != CBET_OK || world_size < 1 || rank < 0 || rank >= world_size) return 0;
    // contiguous near-equal parts, as tracer._parts
    const size_t nb = (size_t)p->nbeams;
    const size_t own_beams = ((size_t)(rank + 1) * nb) / world_size - ((size_t)rank * nb) / world_size;
    const size_t own_planes = ((size_t)(rank + 1) * (p->nx + 2)) / world_size - ((size_t)rank * (p->nx + 2)) / world_size;
    return cbet_cbet_slab_workspace_bytes_parts(p, (int)own_beams, (int)own_planes, 0);
}

size_t cbet_cbet_workspace_bytes(const cbet_params *p)
{
    if (!p || validate(p) != CBET_OK) return 0;
    const size_t hsize = (size_t)(p->nx + 2) * (p->ny + 2) * (p->nz + 2);
    return (5 * (size_t)p->nbeams * hsize + 2 + CBET_MAX_CBET_BEAMS) * sizeof(double);   // 4 field components + gain
}

}  // extern "C"
