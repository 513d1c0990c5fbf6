// cbet_grid_kernels.hip -- the cell-parallel kernels beside the ray integrator (cbet_kernels.hip):
//   * k_gain_field (ordered), k_gain_field_sym (pairs once, LDS-staged) : per-beam fields -> CBET gain coefficient (no
//     reference counterpart, parity unpinned -- model and layout in DESIGN.md section 9)
//   * k_pair_amplitude               : normalised fields -> the largest ion-acoustic amplitude a cell's pair gains correspond to
//     (the map the saturation limit of both gain kernels is chosen by)
//   * k_exchange_matrix, k_exchange_reduce : normalised fields -> the N x N table of energy beam j hands to beam i per pass, and
//     its gross counterpart (lanes are beam pairs, per-workgroup tables in LDS, no atomics)
//   * k_edep_average                 : the 27-point node average of main.cu:334-349
// The gain model -- a cell's plasma state (cell_state), its prefactor and saturation limit, the ordered pair gain and its clamp
// -- is cbet_gain_model.h's, written once for these kernels and the exchange matrix's host twin (cbet_exchange_host.cpp).  Shared
// inside this file: brick_cell (k_gain_field, k_pair_amplitude), row_runs (k_gain_field_sym, k_exchange_matrix), pair_gain_fast
// and saturate_fast (the two pair-once kernels), one dispatch of run-time switches onto template arguments (all four).
// DETUNE (GainArgs.shift != NULL): per-beam frequency shifts, DESIGN.md section 19.  POL, the last switch of all four
// (GainArgs.pol != 0): polarization smoothing, every pair gain times (1 + cos^2 theta) / 4 before the clamp, DESIGN.md section 20.
// BAND (GainArgs.band != NULL): a line spectrum shared by all beams, the pair gain summed over its difference table, DESIGN.md
// section 21 -- the third value of the DETUNE switch (Tune), never instantiated without the DETUNE statements.
// Built with -ffp-contract=off like the rest of the library: every statement of the ordered kernel and of the
// normalisation is one IEEE operation in the order written, which is the order the CPU checker of the CBET stage
// uses; the pair-once kernel's pair function (pair_gain_fast) is the exception and says so.
#include <hip/hip_runtime.h>
#include <type_traits>

#include "cbet_device.h"
#include "cbet_gain_model.h"

namespace cbet {
namespace {

// The colour switch of all four kernels: one colour; per-beam shifts (DETUNE, section 19); shifts and a line spectrum (BAND,
// section 21: a block with a table always carries shifts, zeros if need be, so BAND is only built on top of DETUNE).
enum Tune { kMono = 0, kDetune = 1, kBand = 2 };

// The difference table as the kernels read it: by SCALAR loads.  The table is wave-uniform, written by a set-up call before
// the launch and never by a kernel; through the constant address space every read is a scalar load into scalar registers,
// whatever stores the kernel itself makes -- no vector register holds a table entry.
typedef const __attribute__((address_space(4))) double *BandTable;
__device__ __forceinline__ BandTable band_table_of(const GainArgs &a) { return (BandTable)a.band; }

// The epilogue of both gain kernels: the wave's sums of |new - old| and |new| into GainArgs.change, two atomics per wave.
__device__ __forceinline__ void report_change(const GainArgs &a, int lane, double sum_change, double sum_abs)
{
    if (!a.change) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum_change += __shfl_xor(sum_change, off, kWave);
        sum_abs += __shfl_xor(sum_abs, off, kWave);
    }
    if (lane == 0) {
        atomicAdd(&a.change[0], sum_change);
        atomicAdd(&a.change[1], sum_abs);
    }
}

// Phase 1 of both gain kernels for one beam's entry of a cell that the beam's rays touched (E != 0): the deposited
// (E, Dx, Dy, Dz) become (I, kx, ky, kz) in place.  I = E / (group speed x dt) where the beam is present (E > 0,
// sub-critical plasma, a direction known), else 0; k = |k| D / |D|.  With GainArgs.frozen the three direction
// entries already hold k -- written by an earlier call on the fields of the gain-free first pass -- and only the
// energy entry is read and replaced.
__device__ __forceinline__ void normalise_entry(const GainArgs &a, const CellState &c, double kmag, double ds_node,
                                                double E, double *fI, double *fx, double *fy, double *fz, long o)
{
    double I = 0.0;
    if (a.frozen) {
        const double kx = fx[o], ky = fy[o], kz = fz[o];
        if (E > 0.0 && c.eps > 0.0 && (kx != 0.0 || ky != 0.0 || kz != 0.0)) I = E / ds_node;
        fI[o] = I;
        return;
    }
    const double ax = fx[o], ay = fy[o], az = fz[o];
    const double dn = sqrt(ax * ax + ay * ay + az * az);
    double kx = 0.0, ky = 0.0, kz = 0.0;
    if (c.eps > 0.0 && dn > 0.0) {
        if (E > 0.0) I = E / ds_node;
        kx = kmag * (ax / dn);
        ky = kmag * (ay / dn);
        kz = kmag * (az / dn);
    }
    fI[o] = I; fx[o] = kx; fy[o] = ky; fz[o] = kz;
}

// The walk of k_gain_field and k_pair_amplitude: one wavefront per 2 x 4 x 8 brick of deposit-grid cells (z fastest: every
// load is eight 64-B runs), the bricks that touch the slab [hx_lo, hx_hi) in z, y, x order.  A compact brick keeps the set of
// beams present ANYWHERE in the wave small -- the beam loops of both kernels run over that set (a ballot-built bit mask),
// and a 64-cell z-row crosses several times more beams than a brick does.
// h, hs: the lane's cell of the haloed grid and its index into the (possibly slab-packed) arrays; cell store0 where not valid
struct BrickCell { bool valid; long h, hs; };
__host__ __device__ inline long brick_count(const GainArgs &a) { return (long)(((a.hx_hi + 1) >> 1) - (a.hx_lo >> 1)) * ((a.ny + 5) / 4) * ((a.nz + 9) / 8); }
__device__ __forceinline__ BrickCell brick_cell(const GainArgs &a, long brick, int lane)
{
    const int HY = a.ny + 2, HZ = a.nz + 2;
    const int bx0 = a.hx_lo >> 1, by = (HY + 3) / 4, bz = (HZ + 7) / 8;
    const int ibz = (int)(brick % bz);
    const long t = brick / bz;
    const int iby = (int)(t % by), ibx = bx0 + (int)(t / by);
    const int hi = 2 * ibx + (lane >> 5), hj = 4 * iby + ((lane >> 3) & 3), hk = 8 * ibz + (lane & 7);
    const bool valid = hi >= a.hx_lo && hi < a.hx_hi && hj < HY && hk < HZ;
    const long h = valid ? ((long)hi * HY + hj) * HZ + hk : a.store0;
    return {valid, h, h - a.store0};
}

// fields (E, Dx, Dy, Dz) -> gain coefficient, brick by brick (brick_cell).
//   phase 1: every entry a beam's rays touched (E != 0) is normalised in place to (I, kx, ky, kz), I = 0 where the
//            beam is not present (E <= 0); with GainArgs.frozen only the energy entry (normalise_entry).
//   phase 2: K_i = sum_{j != i} G_ij I_j, beams in increasing order; gain <- gain + relax (K - gain), stored only where it changes.
// SAT (GainArgs.sat > 0): every pair gain goes through pair_clamp -- one factor for (i, j) and (j, i), so the cell's
// exchange still cancels; a pair below the limit keeps its bits ((pref * P) * Ij either way).
// DETUNE (GainArgs.shift != NULL): the pair's resonance gains the beat frequency shift[bj] - shift[bi]
// (pair_gain's second form) -- both beams are wave-uniform, the two entries come by scalar loads.
// POL (GainArgs.pol != 0): the pair gain times pair_smoothing's (1 + cos^2 theta) / 4, before the clamp.
// BAND (TUNE == kBand, GainArgs.band != NULL): pair_gain_band's sum over the difference table instead.
template <bool FLOW, bool STATE, bool SAT, int TUNE, bool POL>
__global__ void __launch_bounds__(256) k_gain_field(const GainArgs a)
{
    constexpr bool DETUNE = TUNE != kMono, BAND = TUNE == kBand;
    const long hsize = a.bstride;                 // entries stored per beam (the whole haloed grid, or one x-slab of it)
    const long total = hsize * a.nbeams;
    const long bricks = brick_count(a);
    const int lane = threadIdx.x & (kWave - 1);
    const long wave0 = (long)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
    const long nwaves = (long)gridDim.x * (blockDim.x / kWave);
    const double iaw2 = a.iaw * a.iaw;
    double sum_change = 0.0, sum_abs = 0.0;
    for (long brick = wave0; brick < bricks; brick += nwaves) {
        const BrickCell cell = brick_cell(a, brick, lane);
        const bool valid = cell.valid;
        double *fI = a.fields + cell.hs, *fx = fI + total, *fy = fx + total, *fz = fy + total;
        const CellState c = cell_state<FLOW, STATE>(a, cell.h);
        const double kmag = a.k0 * c.rt;
        const double ds_node = (kC * c.rt) * a.dt;  // group speed x dt: energy x length -> intensity
        unsigned long long mask = 0ull;             // beams present in some cell of this brick
        for (int b = 0; b < a.nbeams; ++b) {
            const long o = (long)b * hsize;
            const double E = valid ? fI[o] : 0.0;
            if (__builtin_amdgcn_ballot_w64(E != 0.0) == 0ull) continue;   // no ray of this beam came near the brick
            if (__builtin_amdgcn_ballot_w64(E > 0.0) != 0ull) mask |= 1ull << b;
            if (E != 0.0) normalise_entry(a, c, kmag, ds_node, E, fI, fx, fy, fz, o);
        }
        const double pref = cell_pref(a, c);
        const double lim = SAT ? cell_sat_limit(a, c) : 0.0;
        for (int bi = 0; bi < a.nbeams; ++bi) {
            const long oi = (long)bi * hsize;
            double raw = 0.0;
            if ((mask >> bi) & 1ull) {
                const BeamAtCell Bi = beam_at(fI, fx, fy, fz, oi);
                double acc = 0.0;
                unsigned long long m = mask & ~(1ull << bi);
                while (m != 0ull) {
                    const int bj = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const BeamAtCell Bj = beam_at(fI, fx, fy, fz, (long)bj * hsize);
                    const PairWave w = pair_wave(Bi, Bj);
                    if (valid && pair_present(Bi, Bj, w)) {
                        double g;
                        if constexpr (BAND) g = pair_gain_band(c, pref, iaw2, w, a.shift[bj] - a.shift[bi], a.band, a.nband);
                        else if constexpr (DETUNE) g = pair_gain(c, pref, iaw2, w, a.shift[bj] - a.shift[bi]);
                        else g = pair_gain(c, pref, iaw2, w);
                        if constexpr (POL) g = g * pair_smoothing(Bi, Bj, kmag);
                        if (SAT) g = pair_clamp(g, Bi.I, Bj.I, lim);
                        acc += g * Bj.I;
                    }
                }
                raw = acc;
            }
            if (valid) {
                double *gp = a.gain + oi + cell.hs;
                const double old = *gp;
                const double nw = old + a.relax * (raw - old);
                if (nw != old) *gp = nw;
                sum_change += fabs(nw - old);
                sum_abs += fabs(nw);
            }
        }
    }
    report_change(a, lane, sum_change, sum_abs);
}

// The amplitude map: for NORMALISED fields (I, kx, ky, kz) the largest, over the cell's beam pairs i < j,
// of the ion-acoustic amplitude the pair's unclamped gain corresponds to, A_ij = |G_ij| sqrt(Ii Ij) / kap -- the ordered
// kernel's statements, its bricks and its presence mask; one store per valid cell, 0 where no pair exchanges anything or the
// plasma is not sub-critical.  w / kap grows with w, so the largest w is divided once.  Reads a.fields only; a.sat is not read.
// DETUNE: the amplitude is that of the detuned |G_ij|.  POL: ... of the smoothed one, f |G_ij| (section 20).
// BAND: ... of the pair's gain summed over the line spectrum, its total exchange, not of one line pair's grating (section 21).
template <bool FLOW, bool STATE, int TUNE, bool POL>
__global__ void __launch_bounds__(256) k_pair_amplitude(const GainArgs a, double *__restrict__ amp)
{
    constexpr bool DETUNE = TUNE != kMono, BAND = TUNE == kBand;
    const long hsize = a.bstride;
    const long total = hsize * a.nbeams;
    const long bricks = brick_count(a);
    const int lane = threadIdx.x & (kWave - 1);
    const long wave0 = (long)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
    const long nwaves = (long)gridDim.x * (blockDim.x / kWave);
    const double iaw2 = a.iaw * a.iaw;
    for (long brick = wave0; brick < bricks; brick += nwaves) {
        const BrickCell cell = brick_cell(a, brick, lane);
        const bool valid = cell.valid;
        const double *fI = a.fields + cell.hs, *fx = fI + total, *fy = fx + total, *fz = fy + total;
        const CellState c = cell_state<FLOW, STATE>(a, cell.h);
        unsigned long long mask = 0ull;             // beams present in some cell of this brick
        for (int b = 0; b < a.nbeams; ++b) {
            const double I = valid ? fI[(long)b * hsize] : 0.0;
            if (__builtin_amdgcn_ballot_w64(I > 0.0) != 0ull) mask |= 1ull << b;
        }
        const double pref = cell_pref(a, c);
        const double kap = cell_kap(a, c);
        const double kmag = a.k0 * c.rt;            // POL: |k| of every beam present in the cell, as normalise_entry wrote it
        double top = 0.0;
        unsigned long long mi = mask;
        while (mi != 0ull) {
            const int bi = __ffsll((long long)mi) - 1;
            mi &= mi - 1;
            const BeamAtCell Bi = beam_at(fI, fx, fy, fz, (long)bi * hsize);
            unsigned long long m = mi;              // the beams after bi
            while (m != 0ull) {
                const int bj = __ffsll((long long)m) - 1;
                m &= m - 1;
                const BeamAtCell Bj = beam_at(fI, fx, fy, fz, (long)bj * hsize);
                const PairWave w = pair_wave(Bi, Bj);
                if (valid && pair_present(Bi, Bj, w)) {
                    double gn;
                    if constexpr (BAND) gn = pair_gain_band(c, pref, iaw2, w, a.shift[bj] - a.shift[bi], a.band, a.nband);
                    else if constexpr (DETUNE) gn = pair_gain(c, pref, iaw2, w, a.shift[bj] - a.shift[bi]);
                    else gn = pair_gain(c, pref, iaw2, w);
                    if constexpr (POL) gn = gn * pair_smoothing(Bi, Bj, kmag);
                    const double sw = pair_swing(gn, Bi.I, Bj.I);
                    if (sw > top) top = sw;
                }
            }
        }
        if (valid) amp[cell.h] = kap > 0.0 ? top / kap : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------
// The same update with every unordered beam pair evaluated ONCE (G_ji = -G_ij exactly: eta changes sign, P is odd) and
// every entry read from memory ONCE: one wavefront (= one workgroup) per run of LC = 16 cells along z, LG = 4 lanes per
// cell, the run's present beams staged in LDS.
//   masks  : lane (cell, g) loads beam 4 r + g in round r, all rounds in flight; the values are transposed through LDS
//            so that lane b holds beam b's sixteen entries and one compare per cell accumulates the masks of the beams
//            that touched the run (E != 0 somewhere) and that are present in it (E > 0 somewhere) in scalar registers.
//   phase 1: the touched beams, four per round: normalise the entry as k_gain_field does, write it back, and stage
//            (I, kx, ky, kz) of the present beams in LDS, compacted to slots, with a zeroed sum beside them.
//   phase 2: the slots in tiles of four.  Inside a tile lane group g pairs its own beam with the next and (g < 2) the
//            next but one, cyclically -- six pairs in two evaluations; against the later tiles the A tile sits in the
//            registers of all four lanes of the cell and lane group g takes slot g of every B tile, so its sum for that
//            B beam is complete (no atomics) and the four partial sums of the A beams are folded across the lane groups
//            once per A tile.
//   phase 3: every beam's gain relaxes towards its sum (zero where the beam is absent from the cell).
// A run crossed by more beams than LDS has slots for (LCAP = 20) is taken in halves or quarters: fewer cells, more slots.
// LDS 5 arrays x LCAP x LC doubles = 12.8 KB and 168 registers: twelve wavefronts per CU.  The plasma state of a cell
// (cell_state: two square roots, five divisions) is computed for 64 cells at a time and handed out by lane shuffles.
// The sums live in LDS: GainArgs.scratch only selects this kernel, it is never dereferenced.
//
// Measured (round 3, 256^3, 60 beams, frozen directions; profiles/r3/cbet/): 10.9-11.4 ms against 19.2 ms for the kernel
// it replaces (one wavefront per 2x4x8 brick, B tiles re-streamed from memory, sums in a scratch array: 108 GB fetched +
// 14 GB written per call, 70 % of its 1.3e9 line requests missing L2); now ~49 GB fetched + 5.2 GB written,
// SQ_INSTS_VALU 3.7e9 = 0.55 of the vector issue rate.  The steps in between (profiles/r3/experiments/gain_kernel.log):
// 64 slots and 4 waves per CU 27.9 ms; 32 slots / 8 waves with the exact IEEE pair function 22.8; the pair function as
// one quotient, in-tile pairs in two evaluations, phase 1 over touched beams only 14.4 (20 slots: 12.5); masks by
// transposition instead of ballots + 530 scalar bit tests per run, plasma state per 64 cells 11.8; all of phase 1's
// loads in flight 11.4.  LCAP 16 / 24 / 28 / 32: 13.0 / 12.0 / 13.2 / 13.4 ms; LDS-DMA prefetch of the next run's
// lines 13.4 ms; FROZEN as a template parameter 11.5 -> 11.1; skipping phase-3 rounds whose four beams are absent and
// carry no gain: nothing.  Where the 11.2 ms go (timing builds that skip phases): masks 2.3, phase 1 2.5, phase 2 4.0,
// phase 3 2.6 -- additive: a wavefront's phases do not overlap with each other, only with other wavefronts'.  Whole-line
// z-rows (grids with nz + 2 a multiple of 16: 270^3) are ~8 % faster per cell, not more: the memory phases wait on
// latency at 12 waves per CU, not on bytes.
// ---------------------------------------------------------------------------------------------
constexpr int LC = 16, LG = 4, LCAP = 20, LROUNDS = 64 / LG;
constexpr int LCH = 4, LCH3 = 8;   // rounds whose loads are in flight together in phase 1 / phase 3

// The cut of z-row (hi, hj) of the haloed grid into runs of LC cells, k_gain_field_sym's and k_exchange_matrix's.  Runs start
// on 128-byte lines of the arrays, not at z = 16 k of the row: the row's first entry sits `sft` doubles into a line (rows are
// nz + 2 doubles long), so the first run holds the 16 - sft cells up to the next line and every later one is exactly one line
// per beam and array (beams whose stride from beam 0 is an odd multiple of 8 doubles -- every second one at 256^3 -- stay
// half a line off: the arrays' beam stride is the caller's).  Plain members and a function of scalars on purpose: the validity
// test and the clamp of the 64-cell state index stay written out in both kernels, since either of them behind a call -- or
// any member function here -- changes the code the compiler emits for kernels whose register budget is spent.
struct RowRuns { long base; int sft, count; };   // the row's first cell, the shift, the number of runs
__device__ __forceinline__ RowRuns row_runs(const GainArgs &a, int hi, int hj)
{
    const int hz = a.nz + 2;
    const long base = ((long)hi * (a.ny + 2) + hj) * hz;
    const int sft = (int)((base - a.store0) & (LC - 1));
    return {base, sft, (hz + sft + LC - 1) / LC};
}
// z of lane c's cell of run `run`: outside [0, nz + 2) for the lanes in front of the first run's cells and behind the last's
__device__ __forceinline__ int run_hk(int run, int c, int sft) { return LC * run + c - sft; }

// pref * P(eta_ij) as ONE quotient: with N = -(q . u) and D = |q| cs + 1e-10 (eta = N / D),
//   P = iaw^2 eta / ((eta^2 - 1)^2 + iaw^2 eta^2) = iaw^2 N D^3 / ((N^2 - D^2)^2 + iaw^2 N^2 D^2),
// square root and reciprocal by the hardware estimates and Newton steps (measured: K within 5.7 units of 2^-53 S of a 200-bit
// model where the ordered statements reach 4.7, DESIGN.md section 9, "Per-pair accuracy"; the sums of the symmetric kernels
// are grouped differently from the ordered kernel's anyway).  q = 0 (a beam against itself, or two parallel beams) gives
// N = 0 over D^4 = 1e-40: zero, as in the ordered kernel.
// DETUNE: N = -(q . u) + dw with dw = w_j - w_i, the pair's beat frequency.  Two parallel beams of
// different colour would give N = dw over D = 1e-10; the ordered kernel does not evaluate them (pair_present), so here dw
// counts only where q != 0: one compare and one select, and q = 0 keeps N = 0 and the exact zero.
// POL: the quotient times f = (1 + cth^2) / 4.  With |k_i| = |k_j| = kmag, |q|^2 = 2 kmag^2 (1 - cth), so
// cth = 1 - q2raw * rk with rk = 1 / (2 kmag^2), the cell's (cell_rk: 0 where the plasma is not sub-critical -- nothing is
// present there and f = 1/2 multiplies zeros): one fma on q2raw, which is held anyway, one for f, one multiply.  An absolute
// error of an ulp of 1 in cth is a relative one of at most two ulp in f >= 1/4.  A slot whose beam is absent from the cell holds
// k = 0: cth = 1/2 there, a finite f on a gain that only ever multiplies that beam's I = 0.
// BAND: the quotient is Q(x) = x D^3 / ((x^2 - D^2)^2 + iaw^2 x^2 D^2) = P(x / D) / iaw^2, and the gain
// pref iaw^2 (c_0 Q(N) + sum_m c_m (Q(N + d_m) + Q(N - d_m))).  The square-root chain, D, D^2 and D^3 are formed once per pair;
// every table entry costs two more quotients of the same shape (estimate, Newton step, correction) and comes by one scalar
// load of {d_m, c_m} (BandTable): the loop holds N, D^2, D^3 and S in vector registers beside the caller's, nothing per
// entry.  Q is odd to the bit -- x enters the denominator squared, the numerator and both corrections change sign with it --
// so where N = 0 (still plasma without shifts; q = 0, where dw does not count) every bracket is an exact zero whatever
// d_m is: the guard of the DETUNE arm covers the table entries too, and parallel beams still exchange exactly nothing.
template <bool DETUNE = false, bool POL = false, bool BAND = false>
__device__ __forceinline__ double pair_gain_fast(const BeamAtCell &bi, const BeamAtCell &bj, double ux, double uy, double uz,
                                                 double cs, double iaw2, double pref_iaw2, double dw = 0.0, double rk = 0.0,
                                                 BandTable band = nullptr, int nband = 0)
{
    static_assert(DETUNE || !BAND, "the BAND statements are built on the DETUNE ones");
    const double qx = bj.kx - bi.kx, qy = bj.ky - bi.ky, qz = bj.kz - bi.kz;
    const double q2raw = __builtin_fma(qz, qz, __builtin_fma(qy, qy, qx * qx));
    const double q2 = fmax(q2raw, 1e-280);
    double N;
    // DETUNE forms the numerator first: dw is dead before the square-root chain starts (k_gain_field_sym's registers are spent)
    if constexpr (DETUNE) N = (q2raw > 0.0 ? dw : 0.0) - __builtin_fma(qz, uz, __builtin_fma(qy, uy, qx * ux));
    // |q| = sqrt(q2): one Goldschmidt step from the reciprocal-square-root estimate, one correction
    const double r0 = __builtin_amdgcn_rsq(q2);
    double gq = q2 * r0, hq = 0.5 * r0;
    const double e = __builtin_fma(-hq, gq, 0.5);
    gq = __builtin_fma(gq, e, gq); hq = __builtin_fma(hq, e, hq);
    gq = __builtin_fma(__builtin_fma(-gq, gq, q2), hq, gq);
    if constexpr (!DETUNE) N = -__builtin_fma(qz, uz, __builtin_fma(qy, uy, qx * ux));
    const double D = __builtin_fma(gq, cs, 1e-10);
    double gn;
    if constexpr (BAND) {
        const double D2 = D * D, D3 = D * D2;
        auto Q = [&](double x) {
            const double x2 = x * x, t = x2 - D2;
            const double den = __builtin_fma(t, t, (iaw2 * x2) * D2);
            const double num = x * D3;
            double y = __builtin_amdgcn_rcp(den);
            y = __builtin_fma(__builtin_fma(-den, y, 1.0), y, y);
            const double qt = num * y;
            return __builtin_fma(__builtin_fma(-den, qt, num), y, qt);
        };
        double S = band[0] * Q(N);
        for (int m = 0; m < nband; ++m) {
            const double d = band[1 + 2 * m], cm = band[2 + 2 * m];
            S = __builtin_fma(cm, Q(N + d) + Q(N - d), S);
        }
        gn = pref_iaw2 * S;
    } else {
        const double N2 = N * N, D2 = D * D, t = N2 - D2;
        const double den = __builtin_fma(t, t, (iaw2 * N2) * D2);
        const double num = ((pref_iaw2 * N) * D) * D2;
        // num / den: reciprocal estimate, one Newton step, one correction of the quotient
        double y = __builtin_amdgcn_rcp(den);
        y = __builtin_fma(__builtin_fma(-den, y, 1.0), y, y);
        const double qt = num * y;
        gn = __builtin_fma(__builtin_fma(-den, qt, num), y, qt);
    }
    if constexpr (POL) {
        const double cth = __builtin_fma(-q2raw, rk, 1.0);
        return gn * __builtin_fma(0.25 * cth, cth, 0.25);
    } else return gn;
}
// rk of pair_gain_fast's POL form for a cell with rt = sqrt(eps): 1 / (2 kmag^2), kmag = k0 rt; 0 at and above critical density
__device__ __forceinline__ double cell_rk(double k0, double rt)
{
    const double kmag = k0 * rt;
    return rt > 0.0 ? 1.0 / ((kmag + kmag) * kmag) : 0.0;
}

// The clamp of the pair-once kernel on the value pair_gain_fast returned: with w^2 = (gn Ii) (gn Ij)
// beyond lim^2 the gain is scaled by lim / w = lim rsqrt(w^2) -- the estimate and two Goldschmidt steps, the clamped K
// within 4.9 such units like the pair function itself; squares are compared, and gn comes back untouched where the limit is not reached.
__device__ __forceinline__ double saturate_fast(double gn, double Ii, double Ij, double lim)
{
    const double w2 = (gn * Ii) * (gn * Ij);
    if (w2 > lim * lim) {
        const double r0 = __builtin_amdgcn_rsq(w2);
        double gq = w2 * r0, hq = 0.5 * r0;      // gq -> w, hq -> 1 / (2 w)
        double e = __builtin_fma(-hq, gq, 0.5);
        gq = __builtin_fma(gq, e, gq); hq = __builtin_fma(hq, e, hq);
        e = __builtin_fma(-hq, gq, 0.5);
        hq = __builtin_fma(hq, e, hq);
        gn = gn * ((lim + lim) * hq);
    }
    return gn;
}

// LDS traffic between lanes of ONE wavefront: the hardware keeps a wavefront's LDS instructions in order, the compiler
// has to be told that they may not be reordered across this point
__device__ __forceinline__ void lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// a double that is the same in every active lane, moved to scalar registers
__device__ __forceinline__ double uniform_f64(double v)
{
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// STATE (the cell's own sound speed, cell_state): cs is one more per-lane value of the 64-cell state block and of the pair
// loop, where the uniform one sits in scalar registers.  The 168 registers have no room for it -- the instantiations without
// STATE already keep some loop invariants in scratch -- so the STATE arm gives registers back where they are cheapest: the
// sixteen per-lane beam offsets of the mask loads are formed per run instead of once per kernel (hs0, the trick of hs1 and
// hs3), and the first call's arm (not FROZEN: once per solve) keeps three rounds of phase 1 and four of phase 3 in flight
// instead of four and eight.  None of this reorders a sum: no scratch in any STATE instantiation.
// SAT (GainArgs.sat > 0): the cell's limit is one more per-lane value of the state block and of the pair
// loop, and every pair's gain goes through saturate_fast once, before both of its addends.  The SAT arm takes the same
// registers back as the STATE arm does; the instantiations without SAT keep their statements.
// DETUNE (GainArgs.shift != NULL): the pair loop knows a beam by its compacted SLOT, not its number, and
// the slot -> beam map is the run's (the rank of the beam's bit in the presence mask), uniform over its cells: the shifts are
// staged once per run as 64 doubles of LDS indexed by slot (sW; 13.3 KB in all, still twelve workgroups per CU), zero in the
// padding slots of the last tile.  In phase 2 the A tile's four shifts are the same in every lane and are moved to scalar
// registers; the B beam's slot differs between the four lane groups, so its shift is one more LDS read beside its entry.
// The pair function takes dw = w_B - w_A once per pair, before both of its addends: the exchange still cancels.
// POL (GainArgs.pol != 0): the pair function's POL form scales the quotient by f before saturate_fast and
// before both addends; it needs rk = 1 / (2 kmag^2), one more per-lane value of the pair loop.  rk is formed per RUN from the
// cell's rt (cell_rk: one division per sixteen cells and lane, nothing per pair), not kept as an eighth value of the 64-cell
// state block: the state block's values live in registers across the whole kernel, and the listing has 5 more of the 32 POL
// instantiations in scratch that way (DESIGN.md section 20 has both sets of figures, and those of re-deriving kmag^2 from
// the A entry per pair).  The POL arm takes the registers back that the STATE, SAT and DETUNE arms do (LEAN, and the
// DETUNE arm's kernel-wide invariants); the instantiations without POL keep their statements.
// BAND (TUNE == kBand, GainArgs.band != NULL): the DETUNE arm's statements with the pair function's BAND
// form -- the table by scalar loads inside it, the wave-uniform table pointer and count in scalar registers.
template <bool FROZEN, bool FLOW, bool STATE, bool SAT, int TUNE, bool POL>
__global__ void __launch_bounds__(64, 3) k_gain_field_sym(const GainArgs a)
{
    constexpr bool DETUNE = TUNE != kMono, BAND = TUNE == kBand;
    constexpr bool LEAN = STATE || SAT || DETUNE || POL;
    constexpr int PCH = (LEAN && !FROZEN) ? 3 : LCH, QCH = (LEAN && !FROZEN) ? 4 : LCH3;
    static_assert(5 * LCAP * LC >= 64 * (LC + 1), "the slot arrays double as the staging area of the presence masks");
    __shared__ double lds[5 * LCAP * LC];
    double *const sI = lds, *const sX = sI + LCAP * LC, *const sY = sX + LCAP * LC, *const sZ = sY + LCAP * LC,
                 *const sR = sZ + LCAP * LC;
    double *sW = nullptr;                        // [slot] the run's shifts (DETUNE only: no LDS in the other instantiations)
    if constexpr (DETUNE) {
        __shared__ double shifts_by_slot[64];
        sW = shifts_by_slot;
    }
    const int HY = a.ny + 2, HZ = a.nz + 2;
    const long hsize = a.bstride;
    const long total = hsize * a.nbeams;
    const long rows = (long)(a.hx_hi - a.hx_lo) * HY;
    const int lane = threadIdx.x, c = lane & (LC - 1), g = lane >> 4;
    const double iaw2 = a.iaw * a.iaw;
    const int rounds = (a.nbeams + LG - 1) / LG;
    double sum_change = 0.0, sum_abs = 0.0;
    double st_rt = 0.0, st_ux = 0.0, st_uy = 0.0, st_uz = 0.0, st_pref = 0.0, st_cs = 0.0, st_lim = 0.0;
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        const RowRuns runs = row_runs(a, a.hx_lo + (int)(row / HY), (int)(row % HY));
        for (int ibz = 0; ibz < runs.count; ++ibz) {
            const int hk = run_hk(ibz, c, runs.sft);
            const bool valid = hk >= 0 && hk < HZ;
            const long h = runs.base + (valid ? hk : 0);
            const long hs = h - a.store0;
            double *fI = a.fields + hs, *fx = fI + total, *fy = fx + total, *fz = fy + total;
            // ---- which beams touched the run (E != 0 somewhere), which are present (E > 0 somewhere): every round's
            //      load in flight together, transposed through LDS so that lane b sees beam b's sixteen entries and one
            //      compare per cell accumulates the masks (bit b = lane b) in scalar registers
            unsigned long long mask = 0ull, touched = 0ull;
            {
                double E[LROUNDS];
                long hs0 = hsize;
                if (LEAN) asm volatile("" : "+s"(hs0));   // opaque: the sixteen offsets below are formed here, not kept across the kernel
#pragma unroll
                for (int r = 0; r < LROUNDS; ++r) {
                    const int b = LG * r + g;
                    E[r] = (r < rounds && b < a.nbeams && valid) ? fI[(long)b * hs0] : 0.0;
                }
                __syncthreads();                 // the previous run's LDS reads are done
#pragma unroll
                for (int r = 0; r < LROUNDS; ++r) lds[(LG * r + g) * (LC + 1) + c] = E[r];
                __syncthreads();
#pragma unroll
                for (int k = 0; k < LC; ++k) {
                    const double e = lds[lane * (LC + 1) + k];
                    mask |= __builtin_amdgcn_ballot_w64(e > 0.0);
                    touched |= __builtin_amdgcn_ballot_w64(e != 0.0);
                }
            }
            const int n = __popcll(mask), tiles = (n + LG - 1) / LG;
            if constexpr (DETUNE) {
                // the run's shifts by slot: lane b holds beam b's (the table has an entry per lane: CBET_MAX_CBET_BEAMS = 64);
                // zeros first, for the padding slots.  The barriers in front of phase 2 order these stores before its reads,
                // the one behind it orders the reads before the next run's stores.
                static_assert(CBET_MAX_CBET_BEAMS == 64, "one lane per entry of GainArgs.shift");
                int ln = lane;
                asm volatile("" : "+v"(ln));     // opaque: the entry's address and the lane's bit mask are formed here, not kept across the kernel
                sW[ln] = 0.0;
                lds_order();
                if ((mask >> ln) & 1ull) sW[__popcll(mask & ((1ull << ln) - 1ull))] = a.shift[ln];
            }
            // the plasma state of 64 cells at a time (lane = cell), handed to the four runs they make up
            if ((ibz & 3) == 0) {
                const int hk64 = run_hk(ibz, lane, runs.sft);
                if constexpr (DETUNE || POL) {
                    // The DETUNE and POL arms give back the registers their pair loops take: the kernel-wide invariants of cell_state,
                    // cell_pref and cell_kap -- (mach_r1 - mach_r0), (mach_1 - mach_0), 1.0 / iaw, 0.5 * k0, hoisted into vector
                    // registers or scratch in the other instantiations -- are formed here, once per 64 cells, from operands the
                    // compiler cannot see through.  The same operations on the same values: no bit changes.
                    GainArgs b = a;
                    asm volatile("" : "+s"(b.mach_r0), "+s"(b.mach_0), "+s"(b.iaw), "+s"(b.k0));
                    const CellState c64 = cell_state<FLOW, STATE>(b, runs.base + (hk64 < 0 ? 0 : (hk64 < HZ ? hk64 : HZ - 1)));
                    st_rt = c64.rt; st_ux = c64.ux; st_uy = c64.uy; st_uz = c64.uz;
                    st_pref = cell_pref(b, c64);
                    if (STATE) st_cs = c64.cs;
                    if (SAT) st_lim = cell_sat_limit(b, c64);
                } else {
                    const CellState c64 = cell_state<FLOW, STATE>(a, runs.base + (hk64 < 0 ? 0 : (hk64 < HZ ? hk64 : HZ - 1)));
                    st_rt = c64.rt; st_ux = c64.ux; st_uy = c64.uy; st_uz = c64.uz;
                    st_pref = cell_pref(a, c64);
                    if (STATE) st_cs = c64.cs;
                    if (SAT) st_lim = cell_sat_limit(a, c64);
                }
            }
            const int from = LC * (ibz & 3) + c;
            const double rt = __shfl(st_rt, from, kWave), ux = __shfl(st_ux, from, kWave), uy = __shfl(st_uy, from, kWave),
                         uz = __shfl(st_uz, from, kWave);
            const double pref = valid ? __shfl(st_pref, from, kWave) : 0.0;
            const double cs = STATE ? __shfl(st_cs, from, kWave) : a.cs;   // the cell's own, or the uniform one (scalar registers)
            const double lim = SAT ? __shfl(st_lim, from, kWave) : 0.0;
            const double rk = POL ? cell_rk(a.k0, rt) : 0.0;
            const bool subcritical = rt > 0.0;   // eps > 0
            const double kmag = a.k0 * rt;
            const double ds_node = (kC * rt) * a.dt;
            const double pref_iaw2 = pref * iaw2;
            // a run crossed by more beams than LDS has slots for is taken in halves or quarters (fewer cells, more slots)
            const int sh = n <= LCAP ? 4 : (n <= 2 * LCAP ? 3 : 2), lc = 1 << sh, cl = c & (lc - 1);
            for (int part = 0; part < (LC >> sh); ++part) {
                const bool mine_ = (c >> sh) == part;
                __syncthreads();                 // the previous part's LDS reads are done
                // ---- phase 1: the touched beams, four per round (lane group g takes the g-th of them): normalise the
                //      entry (the energy is in L1 / L2 from the loads above), write it back, stage it if the beam is present
                if (mine_) {
                    long hs1 = hsize;            // opaque: keeps the address arithmetic of this phase out of the pair loop's registers
                    asm volatile("" : "+s"(hs1));
                    unsigned long long tm = touched;
                    while (tm != 0ull) {
                        int bb[PCH];
                        double E[PCH], X[PCH], Y[PCH], Z[PCH];
#pragma unroll
                        for (int u = 0; u < PCH; ++u) {
                            int bq[LG];
#pragma unroll
                            for (int q = 0; q < LG; ++q) {
                                bq[q] = tm != 0ull ? __ffsll((long long)tm) - 1 : -1;
                                tm &= tm - 1ull;
                            }
                            bb[u] = g == 0 ? bq[0] : (g == 1 ? bq[1] : (g == 2 ? bq[2] : bq[3]));
                            // the three direction entries are fetched whether this cell's energy entry turns out to be
                            // zero or not (few are): all four loads of all rounds of the chunk are in flight together
                            const bool in = bb[u] >= 0 && valid;
                            const long o = (long)bb[u] * hs1;
                            E[u] = in ? fI[o] : 0.0;
                            X[u] = in ? fx[o] : 0.0;
                            Y[u] = in ? fy[o] : 0.0;
                            Z[u] = in ? fz[o] : 0.0;
                        }
#pragma unroll
                        for (int u = 0; u < PCH; ++u) {
                            const int b = bb[u];
                            const long o = (long)b * hs1;
                            double I = 0.0;
                            if (E[u] != 0.0) {
                                if (FROZEN) {
                                    if (E[u] > 0.0 && subcritical && (X[u] != 0.0 || Y[u] != 0.0 || Z[u] != 0.0)) I = E[u] / ds_node;
                                } else {
                                    const double ax = X[u], ay = Y[u], az = Z[u];
                                    const double dn = sqrt(ax * ax + ay * ay + az * az);
                                    X[u] = Y[u] = Z[u] = 0.0;
                                    if (subcritical && dn > 0.0) {
                                        if (E[u] > 0.0) I = E[u] / ds_node;
                                        X[u] = kmag * (ax / dn);
                                        Y[u] = kmag * (ay / dn);
                                        Z[u] = kmag * (az / dn);
                                    }
                                    fx[o] = X[u]; fy[o] = Y[u]; fz[o] = Z[u];
                                }
                                fI[o] = a.consume ? 0.0 : I;
                            }
                            if (b >= 0 && ((mask >> b) & 1ull)) {
                                const int at = (__popcll(mask & ((1ull << b) - 1ull)) << sh) + cl;
                                const bool here = I > 0.0;   // a beam absent from THIS cell gives and takes nothing
                                sI[at] = here ? I : 0.0;
                                sX[at] = here ? X[u] : 0.0;
                                sY[at] = here ? Y[u] : 0.0;
                                sZ[at] = here ? Z[u] : 0.0;
                                sR[at] = 0.0;
                            }
                        }
                    }
                    if (n + g < LG * tiles) {    // the padding slots of the last tile
                        const int at = ((n + g) << sh) + cl;
                        sI[at] = 0.0; sX[at] = 0.0; sY[at] = 0.0; sZ[at] = 0.0; sR[at] = 0.0;
                    }
                }
                __syncthreads();
                // ---- phase 2: every unordered pair once
                if (mine_) {
                    for (int ta = 0; ta < tiles; ++ta) {
                        // inside the tile: lane group g pairs its own beam g with beams g+1 and (g < 2) g+2, cyclically --
                        // the six pairs in two evaluations; each lane adds to its own beam's sum and to the partner's,
                        // and the partners of one instruction are four different beams
                        {
                            const int self = ((LG * ta + g) << sh) + cl;
                            const int p1 = ((LG * ta + ((g + 1) & 3)) << sh) + cl, p2 = ((LG * ta + ((g + 2) & 3)) << sh) + cl;
                            BeamAtCell S, P1, P2;
                            S.I = sI[self]; S.kx = sX[self]; S.ky = sY[self]; S.kz = sZ[self];
                            P1.I = sI[p1]; P1.kx = sX[p1]; P1.ky = sY[p1]; P1.kz = sZ[p1];
                            P2.I = sI[p2]; P2.kx = sX[p2]; P2.ky = sY[p2]; P2.kz = sZ[p2];
                            double g1, g2;
                            if constexpr (BAND) {
                                const double wS = sW[LG * ta + g];
                                g1 = pair_gain_fast<true, POL, true>(S, P1, ux, uy, uz, cs, iaw2, pref_iaw2, sW[LG * ta + ((g + 1) & 3)] - wS, rk, band_table_of(a), a.nband);
                                g2 = g < 2 ? pair_gain_fast<true, POL, true>(S, P2, ux, uy, uz, cs, iaw2, pref_iaw2, sW[LG * ta + ((g + 2) & 3)] - wS, rk, band_table_of(a), a.nband) : 0.0;
                            } else if constexpr (POL) {
                                double d1 = 0.0, d2 = 0.0;
                                if constexpr (DETUNE) {
                                    const double wS = sW[LG * ta + g];
                                    d1 = sW[LG * ta + ((g + 1) & 3)] - wS;
                                    d2 = sW[LG * ta + ((g + 2) & 3)] - wS;
                                }
                                g1 = pair_gain_fast<DETUNE, true>(S, P1, ux, uy, uz, cs, iaw2, pref_iaw2, d1, rk);
                                g2 = g < 2 ? pair_gain_fast<DETUNE, true>(S, P2, ux, uy, uz, cs, iaw2, pref_iaw2, d2, rk) : 0.0;
                            } else if constexpr (DETUNE) {
                                const double wS = sW[LG * ta + g];
                                g1 = pair_gain_fast<true>(S, P1, ux, uy, uz, cs, iaw2, pref_iaw2, sW[LG * ta + ((g + 1) & 3)] - wS);
                                g2 = g < 2 ? pair_gain_fast<true>(S, P2, ux, uy, uz, cs, iaw2, pref_iaw2, sW[LG * ta + ((g + 2) & 3)] - wS) : 0.0;
                            } else {
                                g1 = pair_gain_fast(S, P1, ux, uy, uz, cs, iaw2, pref_iaw2);
                                g2 = g < 2 ? pair_gain_fast(S, P2, ux, uy, uz, cs, iaw2, pref_iaw2) : 0.0;
                            }
                            if (SAT) {
                                g1 = saturate_fast(g1, S.I, P1.I, lim);
                                g2 = saturate_fast(g2, S.I, P2.I, lim);
                            }
                            sR[self] += g1 * P1.I + g2 * P2.I;
                            lds_order();             // the next statement's entries are other lanes' `self`
                            sR[p1] -= g1 * S.I;
                            lds_order();
                            sR[p2] -= g2 * S.I;
                            lds_order();
                        }
                        if (ta + 1 == tiles) break;
                        BeamAtCell A[LG];
                        double KA[LG];
#pragma unroll
                        for (int s_ = 0; s_ < LG; ++s_) {
                            const int at = ((LG * ta + s_) << sh) + cl;
                            A[s_].I = sI[at]; A[s_].kx = sX[at]; A[s_].ky = sY[at]; A[s_].kz = sZ[at];
                            KA[s_] = 0.0;
                        }
                        double WA[LG] = {};      // the A tile's shifts: the same in every lane, kept in scalar registers
                        if constexpr (DETUNE) {
#pragma unroll
                            for (int s_ = 0; s_ < LG; ++s_) WA[s_] = uniform_f64(sW[LG * ta + s_]);
                        }
                        for (int tb = ta + 1; tb < tiles; ++tb) {
                            const int bt = ((LG * tb + g) << sh) + cl;
                            BeamAtCell B;
                            B.I = sI[bt]; B.kx = sX[bt]; B.ky = sY[bt]; B.kz = sZ[bt];
                            double WB = 0.0;
                            if constexpr (DETUNE) WB = sW[LG * tb + g];
                            double KB = 0.0;
#pragma unroll
                            for (int s_ = 0; s_ < LG; ++s_) {
                                double gn;
                                if constexpr (BAND) gn = pair_gain_fast<true, POL, true>(A[s_], B, ux, uy, uz, cs, iaw2, pref_iaw2, WB - WA[s_], rk, band_table_of(a), a.nband);
                                else if constexpr (POL) gn = pair_gain_fast<DETUNE, true>(A[s_], B, ux, uy, uz, cs, iaw2, pref_iaw2, DETUNE ? WB - WA[s_] : 0.0, rk);
                                else if constexpr (DETUNE) gn = pair_gain_fast<true>(A[s_], B, ux, uy, uz, cs, iaw2, pref_iaw2, WB - WA[s_]);
                                else gn = pair_gain_fast(A[s_], B, ux, uy, uz, cs, iaw2, pref_iaw2);
                                if (SAT) gn = saturate_fast(gn, A[s_].I, B.I, lim);
                                KA[s_] += gn * B.I;
                                KB -= gn * A[s_].I;
                            }
                            sR[bt] += KB;
                        }
                        // fold the four lane groups' partial sums of the A beams; group g keeps beam g's
                        double fold = 0.0;
#pragma unroll
                        for (int s_ = 0; s_ < LG; ++s_) {
                            double t = KA[s_];
                            t += __shfl_xor(t, 16, kWave);
                            t += __shfl_xor(t, 32, kWave);
                            if (s_ == g) fold = t;
                        }
                        sR[((LG * ta + g) << sh) + cl] += fold;
                    }
                }
                __syncthreads();
                // ---- phase 3: relax the gain of every beam towards its sum (zero where the beam is not in the cell)
                if (mine_ && valid) {
                    long hs3 = hsize;
                    asm volatile("" : "+s"(hs3));
                    for (int r0 = 0; r0 < rounds; r0 += QCH) {
                        double old[QCH];
#pragma unroll
                        for (int u = 0; u < QCH; ++u) {
                            const int b = LG * (r0 + u) + g;
                            old[u] = b < a.nbeams ? a.gain[(long)b * hs3 + hs] : 0.0;
                        }
#pragma unroll
                        for (int u = 0; u < QCH; ++u) {
                            const int b = LG * (r0 + u) + g;
                            if (b >= a.nbeams) continue;
                            double raw = 0.0;
                            if ((mask >> b) & 1ull) {
                                const int at = (__popcll(mask & ((1ull << b) - 1ull)) << sh) + cl;
                                raw = sI[at] > 0.0 ? sR[at] : 0.0;
                            }
                            const double nw = old[u] + a.relax * (raw - old[u]);
                            if (nw != old[u]) a.gain[(long)b * hs3 + hs] = nw;
                            sum_change += fabs(nw - old[u]);
                            sum_abs += fabs(nw);
                        }
                    }
                }
            }
        }
    }
    report_change(a, lane, sum_change, sum_abs);
}

// ---------------------------------------------------------------------------------------------
// The pairwise exchange matrix: for NORMALISED fields, T[i][j] = sum over cells of
// ((ds_node g_ij) I_i) I_j and Gross[i][j] = the sum of its magnitudes, every unordered pair once per cell with
// pair_gain_fast (+ saturate_fast under SAT), the arithmetic of k_gain_field_sym.  Reads a.fields only; a.sat is honoured.
// One workgroup of four wavefronts per z-row (grid-stride), the row cut into runs of XC = 16 cells by element index with
// k_gain_field_sym's `sft`, so a view of the fields that starts off a 128-byte line is grouped as the aligned one.  Per run:
//   masks : thread (cell c, group g) loads the intensity of beam 16 r + g in round r; one ballot per round gives the
//           wavefront's share of the presence mask (I > 0 somewhere in the run), four shares are OR-ed through LDS.
//   stage : the same thread stages its entry (I, kx, ky, kz) at [cell][slot] -- slot = the beam's rank in the mask -- with
//           zeros where the beam is absent from the cell, so the pair adds an exact zero there; the direction entries are
//           loaded only where I > 0.  Up to 32 present beams: 16 cells x 33; more: two halves of 8 cells x 65.
//   pairs : LANES ARE PAIRS of the compacted slots, not cells: thread t takes pairs t, t + 256, ... of the n (n - 1) / 2,
//           walks the cells (both beams from LDS, slot-fastest: neighbouring lanes read neighbouring words; the cell's
//           state from the registers of the lane that holds it, by readlane) and sums x and |x| in registers, then adds once
//           into the workgroup's table at the pair's triangular index.  Inside a round every lane owns a different pair and
//           rounds, halves and runs are separated by barriers: no LDS atomics, and every entry's adds come in run order.
// The table (T then Gross, 2 x npairs doubles, zeroed first) leaves by plain vector stores to work[group][2][npairs];
// k_exchange_reduce sums the groups in order.  LDS 2 x 2016 + 4 x 528 + 7 x 64 doubles + masks = 53 KB: three workgroups,
// twelve wavefronts per CU.  The plasma state is computed for 64 cells at a time, as in k_gain_field_sym.
// ---------------------------------------------------------------------------------------------
constexpr int XT = 256, XC = 16, XG = XT / XC, XROUNDS = CBET_MAX_CBET_BEAMS / XG;
constexpr int XSTAGE = 528;                                                        // 16 x 33 >= 8 x 65
constexpr int XPAIRS = CBET_MAX_CBET_BEAMS * (CBET_MAX_CBET_BEAMS - 1) / 2;        // 2016
static_assert(XG * XROUNDS == 64 && XT / kWave == 4, "the mask shares below are written for four wavefronts of 4 x 16 lanes");
static_assert(XC == LC, "RowRuns cuts both kernels' rows");

// a double of lane `l` of the wavefront (l wave-uniform), whatever lanes are active
__device__ __forceinline__ double readlane_f64(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// first pair index of row i of the upper triangle of an n x n matrix, rows in order: (i, i + 1), (i, i + 2), ...
__device__ __forceinline__ int tri_start(int i, int n) { return i * (2 * n - i - 1) / 2; }

// DETUNE (GainArgs.shift != NULL): a lane's pair is (sBeam[sa], sBeam[sb]); it forms w_j - w_i once, in
// front of its walk over the cells.
// POL (GainArgs.pol != 0): rk = 1 / (2 kmag^2) is an eighth row of the state block (cell_rk; 512 bytes of
// LDS more in the POL instantiations only, 53.5 KB: still three workgroups per CU) and the pair function's POL form scales the
// quotient before saturate_fast.
// BAND (TUNE == kBand, GainArgs.band != NULL): the pair function's BAND form, the table by scalar loads.
template <bool FLOW, bool STATE, bool SAT, int TUNE, bool POL>
__global__ void __launch_bounds__(XT, 3) k_exchange_matrix(const GainArgs a, double *__restrict__ work)
{
    constexpr bool DETUNE = TUNE != kMono, BAND = TUNE == kBand;
    __shared__ double tab[2 * XPAIRS];
    __shared__ double sI[XSTAGE], sX[XSTAGE], sY[XSTAGE], sZ[XSTAGE];
    __shared__ double sSt[POL ? 8 : 7][64];
    __shared__ unsigned long long sMask[XT / kWave];
    __shared__ int sBeam[CBET_MAX_CBET_BEAMS];
    const int nb = a.nbeams, npairs = nb * (nb - 1) / 2;
    const int tid = threadIdx.x, c = tid & (XC - 1), g = tid >> 4, lane = tid & (kWave - 1), wv = tid >> 6;
    const int HY = a.ny + 2, HZ = a.nz + 2;
    const long hsize = a.bstride;
    const long total = hsize * nb;
    const long rows = (long)(a.hx_hi - a.hx_lo) * HY;
    const double iaw2 = a.iaw * a.iaw;
    for (int t = tid; t < 2 * npairs; t += XT) tab[t] = 0.0;   // pairs this workgroup never meets leave as zeros
    __syncthreads();
    double st_ux = 0.0, st_uy = 0.0, st_uz = 0.0, st_cs = 0.0, st_pi = 0.0, st_lim = 0.0, st_ds = 0.0, st_rk = 0.0;
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        const RowRuns runs = row_runs(a, a.hx_lo + (int)(row / HY), (int)(row % HY));   // k_gain_field_sym's: cut by element index
        for (int ibz = 0; ibz < runs.count; ++ibz) {
            const int hk = run_hk(ibz, c, runs.sft);
            const bool valid = hk >= 0 && hk < HZ;
            const long hs = runs.base + (valid ? hk : 0) - a.store0;
            const double *fI = a.fields + hs, *fx = fI + total, *fy = fx + total, *fz = fy + total;
            double E[XROUNDS];
#pragma unroll
            for (int r = 0; r < XROUNDS; ++r) {
                const int b = XG * r + g;
                E[r] = (b < nb && valid) ? fI[(long)b * hsize] : 0.0;
            }
            // this wavefront's lanes are groups 4 wv .. 4 wv + 3, sixteen cells each: bits [16 q, 16 q + 16) of a ballot
            unsigned long long share = 0ull;
#pragma unroll
            for (int r = 0; r < XROUNDS; ++r) {
                const unsigned long long bal = __builtin_amdgcn_ballot_w64(E[r] > 0.0);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if ((bal >> (16 * q)) & 0xffffull) share |= 1ull << (XG * r + 4 * wv + q);
            }
            if (lane == 0) sMask[wv] = share;
            // the plasma state of 64 cells at a time (thread = cell), for the four runs they make up
            if ((ibz & 3) == 0 && tid < 64) {
                const int hk64 = run_hk(ibz, tid, runs.sft);
                const CellState c64 = cell_state<FLOW, STATE>(a, runs.base + (hk64 < 0 ? 0 : (hk64 < HZ ? hk64 : HZ - 1)));
                sSt[0][tid] = c64.ux; sSt[1][tid] = c64.uy; sSt[2][tid] = c64.uz; sSt[3][tid] = c64.cs;
                sSt[4][tid] = cell_pref(a, c64) * iaw2;
                sSt[5][tid] = SAT ? cell_sat_limit(a, c64) : 0.0;
                sSt[6][tid] = (kC * c64.rt) * a.dt;
                if constexpr (POL) sSt[7][tid] = cell_rk(a.k0, c64.rt);
            }
            __syncthreads();                     // masks and state are in LDS; the previous run's pair loops are done
            const unsigned long long mask = sMask[0] | sMask[1] | sMask[2] | sMask[3];
            const int n = __popcll(mask);
            if (n < 2) {                         // nothing to exchange (uniform over the workgroup)
                __syncthreads();                 // sMask is read before it is written again
                continue;
            }
            {
                const int from = XC * (ibz & 3) + c;   // lane l of every wavefront holds the state of cell l & 15 of the run
                st_ux = sSt[0][from]; st_uy = sSt[1][from]; st_uz = sSt[2][from]; st_cs = sSt[3][from];
                st_pi = sSt[4][from]; st_lim = sSt[5][from]; st_ds = sSt[6][from];
                if constexpr (POL) st_rk = sSt[7][from];
            }
            // up to 32 present beams: all sixteen cells at once; more: two halves of eight cells (fewer cells, more slots)
            const int sh = n <= 32 ? 4 : 3, lc = 1 << sh, cl = c & (lc - 1), sp = n <= 32 ? 33 : 65;
            const int np = n * (n - 1) / 2;
            for (int part = 0; part < (XC >> sh); ++part) {
                if (part) __syncthreads();       // the previous half's pair loops are done
                if ((c >> sh) == part) {
                    int at[XROUNDS];
                    double X[XROUNDS], Y[XROUNDS], Z[XROUNDS];
#pragma unroll
                    for (int r = 0; r < XROUNDS; ++r) {   // every direction load in flight before the first LDS store
                        const int b = XG * r + g;
                        const bool staged = b < nb && ((mask >> b) & 1ull);
                        at[r] = staged ? cl * sp + __popcll(mask & ((1ull << b) - 1ull)) : -1;
                        const bool here = staged && E[r] > 0.0;   // a beam absent from THIS cell gives and takes nothing
                        const long o = (long)b * hsize;
                        X[r] = here ? fx[o] : 0.0;
                        Y[r] = here ? fy[o] : 0.0;
                        Z[r] = here ? fz[o] : 0.0;
                    }
#pragma unroll
                    for (int r = 0; r < XROUNDS; ++r) {
                        if (at[r] < 0) continue;
                        sI[at[r]] = E[r] > 0.0 ? E[r] : 0.0;
                        sX[at[r]] = X[r]; sY[at[r]] = Y[r]; sZ[at[r]] = Z[r];
                        if (cl == 0) sBeam[at[r]] = XG * r + g;   // (cl == 0: at[r] is the slot)
                    }
                }
                __syncthreads();
                for (int q = tid; q < np; q += XT) {
                    // pair q of the slots' upper triangle -> (sa, sb), sa < sb
                    const float fn = (float)(2 * n - 1);
                    int sa = (int)((fn - sqrtf(fn * fn - 8.0f * (float)q)) * 0.5f);
                    sa = sa < 0 ? 0 : (sa > n - 2 ? n - 2 : sa);
                    while (tri_start(sa, n) > q) --sa;
                    while (tri_start(sa + 1, n) <= q) ++sa;
                    const int sb = sa + 1 + q - tri_start(sa, n);
                    double dw = 0.0;             // DETUNE: the lane's pair's beat frequency, formed once
                    if constexpr (DETUNE) dw = a.shift[sBeam[sb]] - a.shift[sBeam[sa]];
                    double sum_t = 0.0, sum_g = 0.0;
                    for (int k = 0; k < lc; ++k) {
                        const int cell = (part << sh) + k;
                        const double ux = readlane_f64(st_ux, cell), uy = readlane_f64(st_uy, cell), uz = readlane_f64(st_uz, cell);
                        const double cs = STATE ? readlane_f64(st_cs, cell) : a.cs;
                        const double pref_iaw2 = readlane_f64(st_pi, cell), ds_node = readlane_f64(st_ds, cell);
                        BeamAtCell A, B;
                        A.I = sI[k * sp + sa]; A.kx = sX[k * sp + sa]; A.ky = sY[k * sp + sa]; A.kz = sZ[k * sp + sa];
                        B.I = sI[k * sp + sb]; B.kx = sX[k * sp + sb]; B.ky = sY[k * sp + sb]; B.kz = sZ[k * sp + sb];
                        double gn;
                        if constexpr (BAND) gn = pair_gain_fast<true, POL, true>(A, B, ux, uy, uz, cs, iaw2, pref_iaw2, dw, POL ? readlane_f64(st_rk, cell) : 0.0, band_table_of(a), a.nband);
                        else if constexpr (POL) gn = pair_gain_fast<DETUNE, true>(A, B, ux, uy, uz, cs, iaw2, pref_iaw2, dw, readlane_f64(st_rk, cell));
                        else if constexpr (DETUNE) gn = pair_gain_fast<true>(A, B, ux, uy, uz, cs, iaw2, pref_iaw2, dw);
                        else gn = pair_gain_fast(A, B, ux, uy, uz, cs, iaw2, pref_iaw2);
                        if (SAT) gn = saturate_fast(gn, A.I, B.I, readlane_f64(st_lim, cell));
                        const double x = ((ds_node * gn) * A.I) * B.I;
                        sum_t += x;
                        sum_g += fabs(x);
                    }
                    const int bi = sBeam[sa], bj = sBeam[sb];
                    const int at = tri_start(bi, nb) + (bj - bi - 1);
                    tab[at] += sum_t;
                    tab[npairs + at] += sum_g;
                }
            }
        }
    }
    __syncthreads();
    double *mine = work + (long)blockIdx.x * (2 * npairs);
    for (int t = tid; t < 2 * npairs; t += XT) mine[t] = tab[t];
}

// One lane per unordered pair: the groups' partial sums in group order, added into the upper triangle of out (and gross);
// the lower triangle is rewritten from the upper one, the diagonal as zero.
__global__ void __launch_bounds__(256) k_exchange_reduce(const double *__restrict__ work, int groups, int nb,
                                                         double *__restrict__ out, double *__restrict__ gross)
{
    const int npairs = nb * (nb - 1) / 2;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < nb) {
        out[p * nb + p] = 0.0;
        if (gross) gross[p * nb + p] = 0.0;
    }
    if (p >= npairs) return;
    int i = 0;
    while (tri_start(i + 1, nb) <= p) ++i;
    const int j = i + 1 + p - tri_start(i, nb);
    double t = 0.0, s = 0.0;
    for (int grp = 0; grp < groups; ++grp) {
        t += work[(long)grp * (2 * npairs) + p];
        s += work[(long)grp * (2 * npairs) + npairs + p];
    }
    const double nt = out[i * nb + j] + t;
    out[i * nb + j] = nt;
    out[j * nb + i] = -nt;
    if (gross) {
        const double ng = gross[i * nb + j] + s;
        gross[i * nb + j] = ng;
        gross[j * nb + i] = ng;
    }
}

// ---------------------------------------------------------------------------------------------
// main.cu:334-349 (commented out there): edepavg[i][j][k] = (27 haloed cells around node (i,j,k)) / 27,
// terms added in the order the reference writes them (i offset fastest, then j, then k).  A 4 x 4 x 64
// output tile per workgroup, its 6 x 6 x 66 input block staged through LDS: HBM sees every input once.
// ---------------------------------------------------------------------------------------------
constexpr int kAvgTI = 4, kAvgTJ = 4, kAvgTK = 64, kAvgPad = kAvgTK + 3;

__global__ void __launch_bounds__(256) k_edep_average(const double *__restrict__ edep, double *__restrict__ out,
                                                      int nx, int ny, int nz)
{
    __shared__ double t[kAvgTI + 2][kAvgTJ + 2][kAvgPad];
    const int tk = (nz + kAvgTK - 1) / kAvgTK, tj = (ny + kAvgTJ - 1) / kAvgTJ;
    const int bk = blockIdx.x % tk, bj = (blockIdx.x / tk) % tj, bi = blockIdx.x / (tk * tj);
    const int i0 = bi * kAvgTI, j0 = bj * kAvgTJ, k0 = bk * kAvgTK;
    const long sY = nz + 2, sX = (long)(ny + 2) * (nz + 2);
    for (int idx = threadIdx.x; idx < (kAvgTI + 2) * (kAvgTJ + 2) * (kAvgTK + 2); idx += blockDim.x) {
        const int c = idx % (kAvgTK + 2), b = (idx / (kAvgTK + 2)) % (kAvgTJ + 2), a = idx / ((kAvgTK + 2) * (kAvgTJ + 2));
        const int gi = i0 + a, gj = j0 + b, gk = k0 + c;
        t[a][b][c] = (gi < nx + 2 && gj < ny + 2 && gk < nz + 2) ? edep[gi * sX + gj * sY + gk] : 0.0;
    }
    __syncthreads();
    const int lk = threadIdx.x & (kAvgTK - 1), lj = threadIdx.x / kAvgTK;
    const int j = j0 + lj, k = k0 + lk;
    if (j >= ny || k >= nz) return;
#pragma unroll
    for (int li = 0; li < kAvgTI; ++li) {
        const int i = i0 + li;
        if (i >= nx) break;
        double acc = t[li][lj][lk];
#pragma unroll
        for (int dk = 0; dk < 3; ++dk)
#pragma unroll
            for (int dj = 0; dj < 3; ++dj)
#pragma unroll
                for (int di = 0; di < 3; ++di)
                    if (dk + dj + di != 0) acc = acc + t[li + di][lj + dj][lk + dk];
        out[((long)i * ny + j) * nz + k] = acc / 27;
    }
}

// ---------------------------------------------------------------------------------------------
// Sparse exchange of the slab-owned CBET loop (tracer._Exchanger): a beam's rays touch ~10 % of a slab, so what a rank
// sends a slab owner is the list of 64-byte z-runs ("segments": 8 doubles, aligned to 8 along z) its beams can ever
// deposit into, not the dense sub-array.  A segment is {beam (row of the array), index of the run inside one beam's
// [planes][ny+2][ceil((nz+2)/8)] run grid}; the lists are fixed for the life of a solve (ray paths do not depend on
// the gain) and live in device memory.  pack gathers the runs of one message into a contiguous buffer (64-B stores),
// unpack scatters a received buffer; the run that straddles the end of a z-row is zero-filled / clipped.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pack_segments(const double *__restrict__ src, long beam_stride, int hz, int zsegs,
                                                        const int2 *__restrict__ seg, long nseg, double *__restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;   // one double per thread: 8 threads = one 64-B run
    if (i >= nseg * 8) return;
    const int2 sg = seg[i >> 3];
    const int k = (int)(i & 7), zs = sg.y % zsegs, row = sg.y / zsegs;   // row = plane * (ny + 2) + y
    const int z = 8 * zs + k;
    out[i] = z < hz ? src[(long)sg.x * beam_stride + (long)row * hz + z] : 0.0;
}

__global__ void __launch_bounds__(256) k_unpack_segments(double *__restrict__ dst, long beam_stride, int hz, int zsegs,
                                                          const int2 *__restrict__ seg, long nseg, const double *__restrict__ in)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nseg * 8) return;
    const int2 sg = seg[i >> 3];
    const int k = (int)(i & 7), zs = sg.y % zsegs, row = sg.y / zsegs;
    const int z = 8 * zs + k;
    if (z < hz) dst[(long)sg.x * beam_stride + (long)row * hz + z] = in[i];
}

}  // namespace

hipError_t launch_pack_segments(const double *src, long beam_stride, int hy, int hz, const int *seg, long nseg, double *out,
                                hipStream_t stream)
{
    if (nseg <= 0) return hipSuccess;
    const long blocks = (nseg * 8 + 255) / 256;
    (void)hy;
    hipLaunchKernelGGL(k_pack_segments, dim3((unsigned)blocks), dim3(256), 0, stream, src, beam_stride, hz, (hz + 7) / 8,
                       reinterpret_cast<const int2 *>(seg), nseg, out);
    return hipGetLastError();
}

hipError_t launch_unpack_segments(double *dst, long beam_stride, int hy, int hz, const int *seg, long nseg, const double *in,
                                  hipStream_t stream)
{
    if (nseg <= 0) return hipSuccess;
    const long blocks = (nseg * 8 + 255) / 256;
    (void)hy;
    hipLaunchKernelGGL(k_unpack_segments, dim3((unsigned)blocks), dim3(256), 0, stream, dst, beam_stride, hz, (hz + 7) / 8,
                       reinterpret_cast<const int2 *>(seg), nseg, in);
    return hipGetLastError();
}

hipError_t launch_edep_average(const double *edep, double *out, int nx, int ny, int nz, hipStream_t stream)
{
    const long blocks = (long)((nx + kAvgTI - 1) / kAvgTI) * ((ny + kAvgTJ - 1) / kAvgTJ) * ((nz + kAvgTK - 1) / kAvgTK);
    hipLaunchKernelGGL(k_edep_average, dim3((unsigned)blocks), dim3(256), 0, stream, edep, out, nx, ny, nz);
    return hipGetLastError();
}

// One dispatch of run-time switches onto template arguments, for the four templated kernels: dispatch({s0, s1, ...}, launch)
// calls launch(c0, c1, ...) with ck a std::integral_constant<int, v> -- the launch names <decltype(ck)::value...>.  A switch is
// 0 or 1, but for the colour switch (tune_of), which alone may be 2 (kBand): three values, not two switches, so the kernels
// grow by half with BAND and no BAND kernel is built without the DETUNE statements.
template <int N, class Launch, class... Cs>
void dispatch(const int (&on)[N], Launch launch, Cs... cs)
{
    if constexpr (sizeof...(Cs) == N) launch(cs...);
    else if (on[sizeof...(Cs)] == 0) dispatch(on, launch, cs..., std::integral_constant<int, 0>{});
    else if (on[sizeof...(Cs)] == 1) dispatch(on, launch, cs..., std::integral_constant<int, 1>{});
    else if constexpr (sizeof...(Cs) == N - 2) dispatch(on, launch, cs..., std::integral_constant<int, kBand>{});   // the colour switch is the last but one of all four
}
static int tune_of(const GainArgs &a) { return a.band && a.shift ? kBand : (a.shift ? kDetune : kMono); }

// k_gain_field's and k_pair_amplitude's grid: four wavefronts per workgroup, one brick per wavefront up to the cap
static dim3 brick_grid(const GainArgs &a)
{
    long blocks = (brick_count(a) + 3) / 4;
    if (blocks > 256 * 64) blocks = 256 * 64;
    return dim3((unsigned)blocks);
}

hipError_t launch_gain_field(const GainArgs &a, hipStream_t stream)
{
    if (a.hx_hi <= a.hx_lo) return hipSuccess;
    if (a.scratch) {                       // one single-wavefront workgroup per z-row of the slab
        const long rows = (long)(a.hx_hi - a.hx_lo) * (a.ny + 2);
        dispatch({a.frozen != 0, a.flow != nullptr, a.state != nullptr, a.sat > 0.0, tune_of(a), a.pol != 0}, [&](auto... s) {
            hipLaunchKernelGGL((k_gain_field_sym<decltype(s)::value...>), dim3((unsigned)rows), dim3(64), 0, stream, a);
        });
    } else {
        dispatch({a.flow != nullptr, a.state != nullptr, a.sat > 0.0, tune_of(a), a.pol != 0}, [&](auto... s) {
            hipLaunchKernelGGL((k_gain_field<decltype(s)::value...>), brick_grid(a), dim3(256), 0, stream, a);
        });
    }
    return hipGetLastError();
}

hipError_t launch_pair_amplitude(const GainArgs &a, double *amp, hipStream_t stream)
{
    if (a.hx_hi <= a.hx_lo) return hipSuccess;
    dispatch({a.flow != nullptr, a.state != nullptr, tune_of(a), a.pol != 0}, [&](auto... s) {
        hipLaunchKernelGGL((k_pair_amplitude<decltype(s)::value...>), brick_grid(a), dim3(256), 0, stream, a, amp);
    });
    return hipGetLastError();
}

hipError_t launch_exchange_matrix(const GainArgs &a, double *work, double *out, double *gross, hipStream_t stream)
{
    if (a.hx_hi <= a.hx_lo || a.nbeams < 2) return hipSuccess;
    // the number of workgroups follows from the slab alone, never from the device: the same partial sums everywhere
    const long groups = exchange_groups((long)(a.hx_hi - a.hx_lo) * (a.ny + 2));
    dispatch({a.flow != nullptr, a.state != nullptr, a.sat > 0.0, tune_of(a), a.pol != 0}, [&](auto... s) {
        hipLaunchKernelGGL((k_exchange_matrix<decltype(s)::value...>), dim3((unsigned)groups), dim3(XT), 0, stream, a, work);
    });
    if (hipError_t e = hipGetLastError()) return e;
    const int npairs = a.nbeams * (a.nbeams - 1) / 2, lanes = npairs > a.nbeams ? npairs : a.nbeams;
    hipLaunchKernelGGL(k_exchange_reduce, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, work, (int)groups, a.nbeams, out, gross);
    return hipGetLastError();
}

}  // namespace cbet
