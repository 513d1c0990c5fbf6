"""Spherical-harmonic mode spectra of the deposited energy (include/cbet_mi355x.h cbet_sph_modes).

The library projects a grid onto real orthonormal harmonics on spherical shells (RayTracer.sph_modes, api.sph_modes);
this module holds the conventions and the quantities derived from the coefficients.  Works on numpy arrays and torch
tensors alike.
"""
import numpy as np


def sph_index(l, m):
    """Coefficient index of (l, m), -l <= m <= l: l*l + l + m."""
    if not (0 <= abs(m) <= l):
        raise ValueError("need |m| <= l, got l=%d m=%d" % (l, m))
    return l * l + l + m


def lmax_of(ncoef):
    """lmax of a coefficient axis of length (lmax + 1)^2."""
    l = int(round(ncoef ** 0.5)) - 1
    if (l + 1) ** 2 != ncoef:
        raise ValueError("%d is not a square number of coefficients" % ncoef)
    return l


def default_shells(params, nshell=32):
    """nshell + 1 edges of equal width from 0 out to the sphere inscribed in the grid, min(|xmin|, xmax, |ymin|, ymax,
    |zmin|, zmax) (the box around the origin).  Shells further out would be cut by the cube's faces: a shell that the
    faces cut is not a sphere, and its spectrum shows the cut.  float64 numpy array."""
    R = min(abs(params.xmin), params.xmax, abs(params.ymin), params.ymax, abs(params.zmin), params.zmax)
    if not R > 0:
        raise ValueError("the grid does not contain the origin")
    return np.linspace(0.0, R, nshell + 1)


def mode_power(coeffs):
    """P_l = sum over m of a_lm^2: [..., (lmax+1)^2] -> [..., lmax+1]."""
    L = lmax_of(coeffs.shape[-1])
    sq = coeffs * coeffs
    return _stack([sq[..., l * l:(l + 1) * (l + 1)].sum(-1) for l in range(L + 1)], sq)


def nonuniformity(coeffs):
    """(sigma_l [..., lmax+1], sigma_rms [...]): sigma_l = sqrt(P_l) / a_00 and sigma_rms = sqrt(sum_{l=1..lmax} P_l) / a_00,
    the rms over the mean of the angular distribution.  A shell with a_00 = 0 gives inf or nan."""
    P = mode_power(coeffs)
    a00 = coeffs[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        sigma_l = P ** 0.5 / a00[..., None]
        sigma_rms = P[..., 1:].sum(-1) ** 0.5 / a00
    return sigma_l, sigma_rms


def balance(per_beam_coeffs, weights):
    """sum_b w_b a_b over the leading (beam) axis: the coefficients of the deposit with beam b's launch energy scaled by
    w_b, without re-tracing.  Exact for the plain pass only -- its absorption is multiplicative and its cutoff relative to
    a ray's launch energy, so a beam's deposit is linear in that beam's power.  NOT for a CBET solve: the gain couples the
    beams, and the deposit is not linear in any beam's power."""
    w = weights
    if hasattr(per_beam_coeffs, "new_tensor"):
        w = per_beam_coeffs.new_tensor(np.asarray(weights, dtype=np.float64))
        return (w.reshape((-1,) + (1,) * (per_beam_coeffs.dim() - 1)) * per_beam_coeffs).sum(0)
    w = np.asarray(weights, dtype=np.float64)
    return (w.reshape((-1,) + (1,) * (per_beam_coeffs.ndim - 1)) * per_beam_coeffs).sum(0)


def target_coeffs(lmax, amplitudes):
    """The coefficient vector ((lmax + 1)^2 float64) of a distorted target (api.Target, RayTracer.set_target): amplitudes
    maps (l, m) to c_lm, the relative radial displacement dR/R carried by the real orthonormal harmonic Y_lm of this
    module's convention -- target_coeffs(2, {(2, 0): 0.01}).  A uniform relative expansion a is {(0, 0): a * sqrt(4 pi)}."""
    c = np.zeros((lmax + 1) ** 2)
    for (l, m), v in amplitudes.items():
        if l > lmax:
            raise ValueError("l = %d exceeds lmax = %d" % (l, lmax))
        c[sph_index(l, m)] = float(v)
    return c


def offset_response(tracer, deltas, axis=2, lmax=8, r_edges=None, coeffs=None, cbet=None):
    """How the deposit's mode spectrum answers a displaced target: for every delta (cm) the target is set delta along
    `axis` (0, 1, 2 = x, y, z; `coeffs` adds a fixed distortion), one plain pass is traced, and its grid is projected about
    the ORIGIN -- where the beams point -- on the shells r_edges (default modes.default_shells).  Returns (sigma_l
    [len(deltas), lmax + 1], sigma_rms [len(deltas)]) of the shell-summed coefficients as numpy arrays.  cbet: gain
    parameters (api.default_gain_params()) -- instead of the plain pass every offset runs the CBET iteration on the
    displaced target with the flow centred on it (set_flow("target"), cbet_solve) and the CBET deposit is projected.
    The tracer's own target and flow are restored afterwards."""
    saved = tracer.target
    saved_flow = (tracer.flow, tracer._flow_gp)
    grid = tracer.new_grid()
    rows, rms = [], []
    try:
        for delta in deltas:
            offset = [0.0, 0.0, 0.0]
            offset[axis] = float(delta)
            tracer.set_target(offset, coeffs)
            grid.zero_()
            if cbet is None:
                tracer.launch(grid)
            else:
                tracer.set_flow("target", cbet)
                tracer.cbet_solve(grid, cbet)
            c = tracer.sph_modes(grid, r_edges, lmax)[0].sum(0).cpu().numpy()
            sl, sr = nonuniformity(c)
            rows.append(sl)
            rms.append(float(sr))
    finally:
        tracer.target = saved
        if cbet is not None:
            tracer.set_flow(saved_flow[0], saved_flow[1])
    return np.stack(rows), np.asarray(rms)


def _stack(parts, like):
    if hasattr(like, "new_tensor"):
        import torch
        return torch.stack(parts, -1)
    return np.stack(parts, -1)
