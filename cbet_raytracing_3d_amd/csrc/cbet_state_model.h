// cbet_state_model.h -- the local plasma state of the gain kernels at one node (include/cbet_mi355x.h, "local plasma state
// of the gain kernels"): the sound speed cs and the prefactor gain_const from the node's Te, Ti (eV)
// and Z, written once for the gfx950 producer (cbet_mesh.hip) and its host twin (cbet_mesh_host.cpp).  Built with
// -ffp-contract=off on both sides: every operator below is one IEEE fp64 operation, in the order the header fixes, which
// is cbet_gain_constants' own (cbet_params.cpp) -- with the gain parameters' te_ev, ti_ev and z_ion the two results are
// cbet_gain_constants' cs and gain_const bit for bit.  The includer provides sqrt(double).
#ifndef CBET_STATE_MODEL_H_
#define CBET_STATE_MODEL_H_

#include "cbet_device.h"
#include "cbet_hd.h"

namespace cbet {

// k: the four node-independent factors, computed once on the host (state_consts, cbet_params.cpp).
CBET_HD void state_model(const StateConsts &k, double te, double ti, double z, double &cs, double &gc)
{
    const double te_k = te * 11604.5052;
    const double ti_k = ti * 11604.5052;
    const double c1 = k.e2 / ((k.a * te_k) * (1 + 3 * ti_k / (z * te_k)));
    gc = c1 * k.f;
    cs = 1e2 * sqrt(kEc * (z * te + 3.0 * ti) / k.mi_kg);
}

}  // namespace cbet
#endif
