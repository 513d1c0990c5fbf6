"""Quarter-critical LPI maps (include/cbet_mi355x.h cbet_lpi_map): what is derived from the map.

The library writes, per deposit-grid cell inside a band of ne / ncrit, the overlapped intensity, the density scale length and
the two-plasmon-decay threshold parameter (RayTracer.lpi_map, api.lpi_map_host) and a summary of them.  This module holds the
quantities derived from those: the absolute-SRS threshold, which needs a 4/3 power the kernel does not evaluate, the band
means over the angular bins of the quarter-critical surface, and fractions and means from the summary's counts and sums.
Unpinned, like the map: the reference has no such diagnostics.  Works on numpy arrays and torch tensors alike.
Behind them, what is derived from the backscatter SBS gain spectra of section 24: per-beam spectra and a linear-gain proxy of
the reflectivity.
"""
import numpy as np

from . import api


def wavelength_um(params):
    """The vacuum wavelength 2 pi c / omega of `params` in micrometres: the lambda_um of the map's threshold parameter."""
    return 2.0 * np.pi * 29979245800.0 / api.derive(params).omega * 1e4


def srs_parameter(I, L_n, lambda_um):
    """The absolute-SRS threshold parameter at n_c / 4 (Liu, Rosenbluth and White: I_14 > 2377 / (L_um^(4/3) lambda_um^(2/3))):
    I_14 L_um^(4/3) lambda_um^(2/3) / 2377 for I in W/cm^2 and L_n in cm, the map's units (its LPI_I_* and LPI_LN planes);
    >= 1 is above threshold.  0 where L_n is 0."""
    return (I * 1e-14) * (L_n * 1e4) ** (4.0 / 3.0) * lambda_um ** (2.0 / 3.0) / 2377.0


def surface_means(tracer, stack, cells):
    """The band means of a map over the angular bins of the quarter-critical surface.  `stack`: RayTracer.lpi_map's
    [LPI_NQ, *grid_shape]; `cells`: an api.MeshCells of ONE radial shell that holds the band (r_edges of two entries; made
    for the tracer's device).  Every cell of the stack is binned at its own position (deposit_on_mesh, subsamples = 1) and
    each quantity's per-(theta, phi) sum is divided by the band quantity's sum -- the number of band cells in the bin, since
    every quantity is 0 out of band.  Returns a dict: "cells" the band cells per bin [ntheta, nphi], and per quantity name
    of api.LPI_QUANTITIES but "band" the mean over the bin's band cells, NaN where the bin holds none."""
    if cells.shape[0] != 1:
        raise ValueError("surface_means: cells must hold one radial shell, got %d" % cells.shape[0])
    sums, _, _ = tracer.deposit_on_mesh(stack, cells, subsamples=1)
    sums = sums[:, 0]
    count = sums[api.LPI_BAND]
    out = {"cells": count}
    for q, name in enumerate(api.LPI_QUANTITIES):
        if q != api.LPI_BAND:
            out[name] = sums[q] / count            # 0 / 0: NaN, a bin without a band cell
    return out


def summarize(summary):
    """Fractions and means from a summary dict (RayTracer.lpi_map's, api.lpi_summary_from's): the lit fraction of the band,
    the fraction of band cells at or above the threshold per intensity measure, and the band means of I_sum and I_cw (W/cm^2);
    NaN for an empty band.  The maxima and argmax_cw are passed through."""
    n = summary["band_cells"]
    part = (lambda x: x / n) if n else (lambda x: float("nan"))
    out = {"band_cells": n, "lit_fraction": part(summary["lit_cells"]),
           "mean_I_sum": part(summary["sum_I_sum"]), "mean_I_cw": part(summary["sum_I_cw"])}
    for x in ("max", "cw", "sum"):
        out["above_%s_fraction" % x] = part(summary["above_%s" % x])
        out["max_eta_%s" % x] = summary["max_eta_%s" % x]
    out["argmax_cw"], out["max_present"] = summary["argmax_cw"], summary["max_present"]
    return out


# ---- backscatter SBS gain spectra (include/cbet_mi355x.h cbet_trace_backscatter) ----------------
def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def backscatter_spectrum(tally):
    """Per-beam spectra from RayTracer.backscatter_tally's table [nbeams, nshift, 4] (columns api.SBS_TALLY_COLUMNS): a dict of
    numpy arrays -- "mean" [nbeams, nshift], the launch-energy-weighted mean of the gain exponent, sum uray0 Gamma / sum uray0;
    "max" [nbeams, nshift], the largest exponent of any of the beam's rays; "rays" [nbeams], the rays counted; "peak"
    [nbeams], the shift index of the largest mean.  A beam without rays has zeros (no 0 / 0).  Against the scan's shifts
    (the result's "shifts") the rows are the beams' backscatter gain spectra."""
    t = _host(tally).astype(np.float64)
    if t.ndim != 3 or t.shape[2] != len(api.SBS_TALLY_COLUMNS):
        raise ValueError("tally must be [nbeams, nshift, %d], got shape %s" % (len(api.SBS_TALLY_COLUMNS), t.shape))
    has = t[:, :, 3] > 0
    mean = np.where(has, t[:, :, 1] / np.where(has, t[:, :, 0], 1.0), 0.0)
    return {"mean": mean, "max": np.where(has, t[:, :, 2], 0.0), "rays": t[:, 0, 3].astype(np.int64), "peak": np.argmax(mean, axis=1)}


def linear_reflectivity(gamma, rays, seed):
    """A LINEAR-GAIN PROXY of the backscattered fraction: sum uray0 min(1, seed exp(max_m Gamma)) / sum uray0 over the launched
    rays of a RayTracer.backscatter_gain result (gamma [nshift, nitems]; rays [nitems, 4] float64 or [nitems] of
    api.SBS_DTYPE), for a seed level `seed` (the noise source relative to the pump, e.g. 1e-9).  Every ray amplifies the seed
    by its own largest exponent of the scan, capped at the pump's launch energy; no pump depletion, no absorption of the
    scattered light, no competition between rays or shifts -- a ranking of designs, not a prediction.  0.0 without rays."""
    g = _host(gamma).astype(np.float64)
    r = np.ascontiguousarray(_host(rays))
    if r.dtype != api.SBS_DTYPE:
        r = r.astype(np.float64, copy=False).reshape(-1, 4).view(api.SBS_DTYPE)[:, 0]
    r = r.reshape(-1)
    if g.ndim != 2 or g.shape[1] != r.size:
        raise ValueError("gamma must be [nshift, %d], got shape %s" % (r.size, g.shape))
    live = (r["status"] & api.RAY_LAUNCHED) != 0
    total = float(r["uray0"][live].sum())
    if not live.any() or total == 0.0:
        return 0.0
    with np.errstate(over="ignore"):
        amp = np.minimum(1.0, seed * np.exp(g[:, live].max(axis=0)))
    return float((r["uray0"][live] * amp).sum() / total)
