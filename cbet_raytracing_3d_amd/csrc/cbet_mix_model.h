// cbet_mix_model.h -- the statements of the Anderson mixing of the gain iterate (include/cbet_mi355x.h
// cbet_mix_residual, cbet_mix_apply), each written once for the gfx950 kernels (cbet_mix.hip) and the host twins
// (cbet_mix_host.cpp).  Built with -ffp-contract=off on both sides: every operator below is one IEEE fp64 operation, in the
// order written.  The ORDER of the sums is part of the model too: which elements a thread takes (mix_element) and how 256
// thread sums become one (the butterfly of a wavefront, then the wavefronts in order) are stated here, and the twin walks
// them as the kernels do, so a Gram row has the same bytes on both sides.
#ifndef CBET_MIX_MODEL_H_
#define CBET_MIX_MODEL_H_

#include "cbet_hd.h"
#include "cbet_mi355x.h"

namespace cbet {

constexpr int kMixThreads = 256;                                   // threads of a workgroup: four wavefronts
constexpr int kMixWave = 64;
constexpr int kMixIters = CBET_MIX_SPAN / (2 * kMixThreads);       // pairs of elements a thread takes from one span
constexpr int kMixRow = CBET_MIX_MAX_DEPTH + 1;                    // doubles of a partial row in `work`, whatever h
static_assert(kMixIters * 2 * kMixThreads == CBET_MIX_SPAN && kMixIters >= 1, "a span is whole pairs for every thread");

// Spans of n elements, and the workgroups they go round-robin to: from n alone.
CBET_HD long mix_spans(long n) { return (n + (CBET_MIX_SPAN - 1)) / CBET_MIX_SPAN; }
CBET_HD long mix_groups(long n) { const long s = mix_spans(n); return s < CBET_MIX_MAX_GROUPS ? s : CBET_MIX_MAX_GROUPS; }
// The first element of thread t's pair i of span s; the pair's second element is the next one.
CBET_HD long mix_element(long s, int i, int t) { return s * CBET_MIX_SPAN + 2L * (i * kMixThreads + t); }

// One element of the residual pass: f = y - x, and its products added to the thread's H + 1 running sums.
template <int H>
CBET_HD double mix_residual_element(double y, double x, const double *fh, double *dot)
{
    const double f = y - x;
    for (int j = 0; j < H; ++j) dot[j] = dot[j] + f * fh[j];
    dot[H] = dot[H] + f * f;
    return f;
}

// One element of the combination, oldest entry first.
template <int C>
CBET_HD double mix_combine(const double *y, const double *alpha)
{
    double acc = alpha[0] * y[0];
    for (int j = 1; j < C; ++j) acc = acc + alpha[j] * y[j];
    return acc;
}

}  // namespace cbet
#endif
