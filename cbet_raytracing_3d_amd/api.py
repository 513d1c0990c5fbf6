"""ctypes binding of the C ABI in include/cbet_mi355x.h.

This is plumbing over libcbet_mi355x.so (hand-written HIP for gfx950): every function here calls
straight into the library and raises CbetError when the library reports a failure.  There is no
CPU fallback -- if the shared library is missing, importing this module raises.

Names mirror the reference's interface for the path (file:line into /root/reference):
    safeGPUAlloc / moveToAndFromGPU   multi_gpu.cuh:6-7
    launch_ray_XYZ                    launch_ray_XZ.cu:117-121 (launch site main.cu:171-174)
    ray_tracing                       rayTracing(), main.cu:96-232
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# CBET_LIB_PATH: point at an alternative build of the same library (profiling experiments only)
LIB_PATH = os.environ.get("CBET_LIB_PATH") or os.path.join(_PKG, "lib", "libcbet_mi355x.so")
DATA_DIR = os.path.join(_PKG, "data")

OK, EINVAL, EHIP, ENOMEM, ENODEVICE, ECOMM = 0, -1, -2, -3, -4, -5
NPHASE = 2001
KERNEL_DEFAULT, KERNEL_GLOBAL_ATOMICS, KERNEL_LDS_COMBINE, KERNEL_LDS_WINDOW = 0, 1, 2, 3


class CbetError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("cbet error %d: %s" % (code, msg))
        self.code = code


class Params(C.Structure):
    """cbet_params (def.cuh:33-131 as run-time fields)."""
    _fields_ = [
        ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
        ("xmin", C.c_double), ("xmax", C.c_double),
        ("ymin", C.c_double), ("ymax", C.c_double),
        ("zmin", C.c_double), ("zmax", C.c_double),
        ("nbeams", C.c_int), ("rays_per_zone", C.c_int),
        ("courant_mult", C.c_double),
        ("absorption", C.c_int), ("nprofile", C.c_int),
        ("max_threads", C.c_int), ("threads_per_block", C.c_int),
        ("ngpus", C.c_int),
        ("beam_lo", C.c_int), ("beam_hi", C.c_int),
        ("shard_index", C.c_int), ("shard_count", C.c_int),
        ("kernel_variant", C.c_int), ("force_wide_index", C.c_int),
        ("per_beam_grids", C.c_int), ("patch_order", C.c_int),
        ("grid_beam0", C.c_int), ("grid_beams", C.c_int),
        ("rim_merge", C.c_int), ("edep_zpitch", C.c_int),
        ("window_stats", C.c_int),
    ]

    def copy(self, **overrides):
        q = Params()
        C.memmove(C.byref(q), C.byref(self), C.sizeof(Params))
        for k, v in overrides.items():
            setattr(q, k, v)
        return q


class Derived(C.Structure):
    """cbet_derived (def.cuh / main.cu:156-161 derived constants)."""
    _fields_ = [
        ("dx", C.c_double), ("dy", C.c_double), ("dz", C.c_double), ("dt", C.c_double),
        ("nt", C.c_int), ("zones_spanned", C.c_int),
        ("nrays_x", C.c_int), ("nrays_y", C.c_int), ("nrays", C.c_int),
        ("omega", C.c_double), ("ncrit", C.c_double), ("uray_mult", C.c_double),
        ("xconst", C.c_double), ("yconst", C.c_double), ("zconst", C.c_double),
        ("threads_per_beam", C.c_long), ("nindices", C.c_int), ("grid_y", C.c_int),
        ("edep_size", C.c_long), ("ntraced_ids", C.c_long), ("nlive_rays", C.c_long),
    ]


class Counters(C.Structure):
    _fields_ = [
        ("ray_steps", C.c_ulonglong), ("rays_traced", C.c_ulonglong),
        ("global_atomics", C.c_ulonglong), ("lds_evictions", C.c_ulonglong),
        ("wave_steps", C.c_ulonglong), ("wave_steps_miss", C.c_ulonglong),
        ("wave_steps_wide", C.c_ulonglong), ("slabs_retired", C.c_ulonglong),
    ]


MAX_CBET_BEAMS = 64
DEPOSIT_ENERGY, DEPOSIT_FIELDS, DEPOSIT_FIELD_ENERGY = 0, 1, 2   # cbet_trace_cbet's `quantity`


class GainParams(C.Structure):
    """cbet_gain_params -- the CBET stage (parity unpinned: no reference counterpart)."""
    _fields_ = [
        ("z_ion", C.c_double), ("te_ev", C.c_double), ("ti_ev", C.c_double), ("mi_over_me", C.c_double),
        ("iaw", C.c_double),
        ("mach_r0", C.c_double), ("mach_0", C.c_double), ("mach_r1", C.c_double), ("mach_1", C.c_double),
        ("max_exponent", C.c_double), ("relax", C.c_double), ("tolerance", C.c_double),
        ("max_passes", C.c_int), ("direction_passes", C.c_int), ("directions_frozen", C.c_int), ("reserved_", C.c_int),
    ]


class CbetReport(C.Structure):
    _fields_ = [
        ("passes", C.c_int), ("converged", C.c_int), ("change", C.c_double), ("imbalance", C.c_double),
        ("beam_gain", C.c_double * MAX_CBET_BEAMS),
        ("ray_steps", C.c_ulonglong), ("ray_steps_final", C.c_ulonglong),
    ]


# ---- exit pass (cbet_trace_exits) ----------------------------------------------------------------
RAY_LAUNCHED, RAY_CUTOFF, RAY_ESCAPED, RAY_TIMEOUT = 1, 2, 4, 8   # cbet_ray_exit.status bits
TALLY_COLUMNS = ("launched", "gained", "absorbed", "escaped", "stranded", "unfinished", "n_rays", "n_escaped")


class RayExit(C.Structure):
    """cbet_ray_exit: one ray's state when it ended (80 bytes)."""
    _fields_ = [
        ("x", C.c_double), ("y", C.c_double), ("z", C.c_double),
        ("vx", C.c_double), ("vy", C.c_double), ("vz", C.c_double),
        ("uray", C.c_double), ("uray0", C.c_double), ("gained", C.c_double),
        ("steps", C.c_int), ("status", C.c_int),
    ]


def record_dtype(cls):
    """The numpy structured dtype of a ctypes record of doubles, ints and shorts: the same names in the same order."""
    kinds = {C.c_double: "<f8", C.c_int: "<i4", C.c_short: "<i2"}
    return np.dtype([(name, kinds[ct]) for name, ct in cls._fields_])


# the same record as a numpy structured dtype: view a downloaded [..., 10] float64 array with .view(EXIT_DTYPE)
EXIT_DTYPE = record_dtype(RayExit)
assert EXIT_DTYPE.itemsize == C.sizeof(RayExit) == 80


def farfield_bins(vx, vy, vz, ntheta, nphi):
    """The bin coordinates cbet_farfield uses, (1 - vz/|v|)/2 * ntheta and (atan2(vy, vx) + pi)/(2 pi) * nphi, before the floor."""
    vx, vy, vz = (np.asarray(v, dtype=np.float64) for v in (vx, vy, vz))
    vn = np.sqrt(vx * vx + vy * vy + vz * vz)
    return (1.0 - vz / vn) / 2.0 * ntheta, (np.arctan2(vy, vx) + np.pi) / (2.0 * np.pi) * nphi


def farfield_numpy(records, ntheta, nphi):
    """Host restatement of cbet_farfield on a structured array of records (EXIT_DTYPE): hist[ntheta][nphi]."""
    r = np.asarray(records).reshape(-1)
    want = RAY_LAUNCHED | RAY_ESCAPED
    r = r[(r["status"] & want) == want]
    ct, cp = farfield_bins(r["vx"], r["vy"], r["vz"], ntheta, nphi)

    def idx(c, n):
        c = np.where(c > 0.0, c, 0.0)
        return np.minimum(np.floor(c), n - 1).astype(np.int64)

    hist = np.zeros((ntheta, nphi))
    np.add.at(hist, (idx(ct, ntheta), idx(cp, nphi)), r["uray"])
    return hist


# ---- ray path recorder (cbet_trace_paths) --------------------------------------------------------
class PathSample(C.Structure):
    """cbet_path_sample: a ray's state at the launch point (step 0) or after a step (64 bytes)."""
    _fields_ = [
        ("x", C.c_double), ("y", C.c_double), ("z", C.c_double),
        ("uray", C.c_double), ("absorbed", C.c_double), ("gained", C.c_double),
        ("ci", C.c_int), ("cj", C.c_int), ("ck", C.c_int), ("step", C.c_int),
    ]


class RayTurn(C.Structure):
    """cbet_ray_turn: a ray's closest approach to the centre, and how it ended (64 bytes)."""
    _fields_ = [
        ("r2", C.c_double), ("x", C.c_double), ("y", C.c_double), ("z", C.c_double),
        ("uray", C.c_double), ("ne", C.c_double),
        ("step", C.c_int), ("steps", C.c_int), ("status", C.c_int), ("nsamples", C.c_int),
    ]


# the same records as numpy structured dtypes: view a downloaded [..., 8] float64 array with .view(PATH_DTYPE) / .view(TURN_DTYPE)
PATH_DTYPE = record_dtype(PathSample)
TURN_DTYPE = record_dtype(RayTurn)
assert PATH_DTYPE.itemsize == C.sizeof(PathSample) == 64
assert TURN_DTYPE.itemsize == C.sizeof(RayTurn) == 64


# ---- backscatter SBS gain spectra (cbet_trace_backscatter) ------------------------
SBS_MAX_SHIFTS = 16                               # CBET_SBS_MAX_SHIFTS
SBS_TALLY_COLUMNS = ("uray0", "weighted", "max", "n_rays")   # CBET_SBS_TALLY_*


class RaySbs(C.Structure):
    """cbet_ray_sbs: a ray's largest gain exponent, where in the spectrum it is, and how the ray ended (32 bytes)."""
    _fields_ = [
        ("gmax", C.c_double), ("uray0", C.c_double), ("uray_end", C.c_double),
        ("steps", C.c_int), ("imax", C.c_short), ("status", C.c_short),
    ]


# the same record as a numpy structured dtype: view a downloaded [..., 4] float64 array with .view(SBS_DTYPE)
SBS_DTYPE = record_dtype(RaySbs)
assert SBS_DTYPE.itemsize == C.sizeof(RaySbs) == 32


# ---- perturbed targets (cbet_tabulate_target) ----------------------------------------------------
TARGET_LMAX = 16


class LpiSummary(C.Structure):
    """cbet_lpi_summary: counts, maxima and sums over the band cells of an LPI map; merged into."""
    _fields_ = [("band_cells", C.c_longlong), ("lit_cells", C.c_longlong),
                ("above_max", C.c_longlong), ("above_cw", C.c_longlong), ("above_sum", C.c_longlong),
                ("argmax_cw", C.c_longlong),
                ("max_eta_max", C.c_double), ("max_eta_cw", C.c_double), ("max_eta_sum", C.c_double),
                ("sum_I_sum", C.c_double), ("sum_I_cw", C.c_double),
                ("max_present", C.c_int), ("reserved", C.c_int)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


# the quantities of an LPI map, CBET_LPI_* of the header
LPI_NQ = 7
LPI_BAND, LPI_I_SUM, LPI_I_CW, LPI_I_MAX, LPI_LN, LPI_ETA_SUM, LPI_ETA_CW = range(LPI_NQ)
LPI_QUANTITIES = ("band", "I_sum", "I_cw", "I_max", "L_n", "eta_sum", "eta_cw")
LPI_MAX_BINS = 16                               # CBET_LPI_MAX_BINS
LPI_SUMMARY_BYTES = 96                          # sizeof(cbet_lpi_summary)
EC, ME = 1.60217662e-19, 9.10938356e-31         # the library's electron charge and mass (csrc/cbet_device.h kEc, kMe)


class Target(C.Structure):
    """cbet_target: a target whose centre sits at `offset` (cm) and whose iso-surfaces are displaced by
    delta(theta, phi) = sum_c coeffs[c] Y_c (relative, dR/R; modes.target_coeffs builds the vector, index l*l + l + m).
    lmax defaults to what the coefficient vector's length says (0 without one).  The library checks the values."""
    _fields_ = [("offset", C.c_double * 3), ("lmax", C.c_int), ("coeffs", C.POINTER(C.c_double))]

    def __init__(self, offset=(0.0, 0.0, 0.0), coeffs=None, lmax=None):
        super().__init__()
        self.offset = (C.c_double * 3)(*[float(v) for v in offset])
        self._keep = None
        if coeffs is not None:
            self._keep = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(-1).copy()
            n = int(round(self._keep.size ** 0.5)) - 1
            if (n + 1) ** 2 != self._keep.size or (lmax is not None and lmax != n):
                raise ValueError("coeffs must hold (lmax + 1)^2 values, got %d%s" % (
                    self._keep.size, "" if lmax is None else " with lmax = %d" % lmax))
            lmax = n
            self.coeffs = _dptr(self._keep)
        self.lmax = 0 if lmax is None else int(lmax)

    def coeff_array(self):
        """A copy of the coefficient vector ((lmax + 1)^2 zeros without one)."""
        return np.zeros((self.lmax + 1) ** 2) if self._keep is None else self._keep.copy()


# ---- hydro-mesh plasma (cbet_tabulate_mesh) -----------------------------------
MESH_MAX_COORDS = 2560


class MeshIons(C.Structure):
    """cbet_mesh_ions: ion temperature (eV) and mean charge on a mesh's nodes, each an address or None (the gain
    parameters' ti_ev / z_ion everywhere).  api.Mesh(..., ti=, zbar=) builds it (Mesh.ions) and keeps the arrays alive."""
    _fields_ = [("ti", C.c_void_p), ("zbar", C.c_void_p)]


class Mesh(C.Structure):
    """cbet_mesh: ne, te and optionally the velocity of a plasma on a spherical-polar mesh about `center` (cm).
    r [nr], theta [ntheta], phi [nphi]: node coordinates (theta / phi None: the state does not depend on that angle);
    ne, te: [nr, ntheta, nphi] (a 1-D or 2-D array is taken as [nr] / [nr, ntheta]); velocity: None, three arrays
    (ur, uth, uph), each of the fields' shape or None (zero), or one array [3, nr, ntheta, nphi].  ti (eV), zbar: the ion
    temperature and the mean charge for the gain kernels' state table, each of the fields' shape or None (the gain
    parameters' value everywhere); they travel beside the struct (Mesh.ions, a MeshIons), which keeps cbet_mesh's layout.
    Numpy arrays make a HOST mesh (mesh_check, mesh_tables, mesh_flow_table, mesh_state_table); to(device) uploads it once
    and returns the DEVICE mesh (tabulate_mesh, tabulate_mesh_flow, tabulate_mesh_state).  The struct keeps its arrays
    alive.  The library checks the values."""
    _fields_ = [("center", C.c_double * 3), ("nr", C.c_int), ("ntheta", C.c_int), ("nphi", C.c_int)] + \
               [(name, C.c_void_p) for name in ("r", "theta", "phi", "ne", "te", "ur", "uth", "uph")]

    def __init__(self, r, theta, phi, ne, te, velocity=None, center=(0.0, 0.0, 0.0), ti=None, zbar=None):
        super().__init__()

        def axis(a, alone):
            return _host([alone] if a is None else a).reshape(-1).copy()

        r, theta, phi = axis(r, 0.0), axis(theta, 0.5 * np.pi), axis(phi, 0.0)
        shape = (r.size, theta.size, phi.size)

        def field(a, what):
            a = _host(a)
            if a.ndim < 3 and a.shape == shape[:a.ndim] and a.size == int(np.prod(shape)):
                a = a.reshape(shape)
            if a.shape != shape:
                raise ValueError("mesh: %s has shape %s, the coordinates say %s" % (what, a.shape, shape))
            return a.copy()

        if velocity is None:
            velocity = (None, None, None)
        if len(velocity) != 3:
            raise ValueError("mesh: velocity is (ur, uth, uph)")
        u = [None if c is None else field(c, name) for c, name in zip(velocity, ("ur", "uth", "uph"))]
        self._set(center, shape, [r, theta, phi, field(ne, "ne"), field(te, "te")] + u,
                  [None if a is None else field(a, name) for a, name in ((ti, "ti"), (zbar, "zbar"))])

    def _set(self, center, shape, arrays, ions=(None, None)):
        self.center = (C.c_double * 3)(*[float(v) for v in center])
        self.nr, self.ntheta, self.nphi = shape
        self._keep = arrays
        for name, a in zip(("r", "theta", "phi", "ne", "te", "ur", "uth", "uph"), arrays):
            setattr(self, name, _addr(a))
        self._ions = list(ions)         # (ti, zbar) beside the struct
        self.ions = MeshIons(_addr(self._ions[0]), _addr(self._ions[1]))

    @property
    def shape(self):
        return (self.nr, self.ntheta, self.nphi)

    @property
    def has_velocity(self):
        return any(a is not None for a in self._keep[5:])

    def to(self, device):
        """The same mesh with its arrays on `device` (a torch device), uploaded once."""
        import torch
        m = Mesh.__new__(Mesh)
        C.Structure.__init__(m)
        up = lambda arrays: [None if a is None else torch.as_tensor(a).to(device) for a in arrays]      # noqa: E731
        m._set(self.center, self.shape, up(self._keep), up(self._ions))
        return m


# ---- deposit on the hydro mesh (cbet_mesh_deposit) ----------------------------
MESH_MAX_SUBSAMPLES = 4
MESH_DEPOSIT_AUTO, MESH_DEPOSIT_GLOBAL, MESH_DEPOSIT_LDS = 0, 1, 2


class MeshCellsStruct(C.Structure):
    """cbet_mesh_cells: the argument of cbet_mesh_cells_create (HOST edge arrays)."""
    _fields_ = [("center", C.c_double * 3), ("nr", C.c_int), ("ntheta", C.c_int), ("nphi", C.c_int),
                ("r_edges", C.c_void_p), ("theta_edges", C.c_void_p), ("phi_edges", C.c_void_p)]


class MeshCells:
    """The cells of a spherical-polar mesh about `center` (cm) that deposit grids are binned into: r_edges [nr+1],
    theta_edges [ntheta+1] from 0 to pi (None: one row), phi_edges [nphi+1] over one period (None: one column).  Wraps a
    cbet_mesh_cells_handle: the library validates the edges (CbetError names the first offence), builds the lookup tables
    and, with gpu a device index, uploads them once; gpu None makes a host-only handle (mesh_deposit_host).  close(), or
    the object's end, frees it."""

    def __init__(self, r_edges, theta_edges=None, phi_edges=None, center=(0.0, 0.0, 0.0), subsamples_max=4, gpu=None):
        self._h = C.c_void_p()

        def edges(a):
            return None if a is None else _host(a).reshape(-1).copy()

        self.r_edges, self.theta_edges, self.phi_edges = edges(r_edges), edges(theta_edges), edges(phi_edges)
        self.center = tuple(float(v) for v in center)
        self.subsamples_max = int(subsamples_max)
        self.gpu = -1 if gpu is None else int(gpu)
        self.shape = tuple(1 if e is None else e.size - 1 for e in (self.r_edges, self.theta_edges, self.phi_edges))
        self.column_shift = 0           # from_nodes: column k is node (k + column_shift) % nphi's cell
        c = MeshCellsStruct()
        c.center = (C.c_double * 3)(*self.center)
        c.nr, c.ntheta, c.nphi = self.shape
        c.r_edges, c.theta_edges, c.phi_edges = _addr(self.r_edges), _addr(self.theta_edges), _addr(self.phi_edges)
        _check(lib().cbet_mesh_cells_create(C.byref(self._h), C.byref(c), self.subsamples_max, self.gpu))

    @classmethod
    def from_nodes(cls, r, theta=None, phi=None, center=(0.0, 0.0, 0.0), **kw):
        """The dual cells of a node mesh (api.Mesh's coordinates): edges at the midpoints between nodes; the first r edge
        max(0, r[0] - (r[1] - r[0]) / 2), the last r[-1] + (r[-1] - r[-2]) / 2; the theta edges closed with 0 and pi;
        the phi edges periodic (the first lies half-way between the last node, one period back, and the first).  theta /
        phi None or of one node: one row / one column.  Column k is node k's cell, except where the first phi edge would fall
        below -pi (the library wants it in [-pi, pi)): the edges then start one column later and column k is node
        (k + column_shift) % nphi's cell, column_shift = 1; RayTracer.deposit_on_mesh rolls its outputs back."""
        r = np.asarray(r, dtype=np.float64).reshape(-1)
        if r.size < 2:
            raise ValueError("from_nodes: r needs two nodes or more")
        mid = 0.5 * (r[1:] + r[:-1])
        r_edges = np.concatenate(([max(0.0, r[0] - (r[1] - r[0]) / 2)], mid, [r[-1] + (r[-1] - r[-2]) / 2]))
        theta_edges = phi_edges = None
        shift = 0
        if theta is not None and np.size(theta) > 1:
            t = np.asarray(theta, dtype=np.float64).reshape(-1)
            theta_edges = np.concatenate(([0.0], 0.5 * (t[1:] + t[:-1]), [np.pi]))
        if phi is not None and np.size(phi) > 1:
            f = np.asarray(phi, dtype=np.float64).reshape(-1)
            first = 0.5 * ((f[-1] - 6.283185307179586) + f[0])
            phi_edges = np.concatenate(([first], 0.5 * (f[1:] + f[:-1]), [first + 6.283185307179586]))
            if phi_edges[0] < -np.pi:        # the same columns, named one period later
                shift = 1
                phi_edges = np.concatenate((phi_edges[1:], [phi_edges[1] + 6.283185307179586]))
        cells = cls(r_edges, theta_edges, phi_edges, center, **kw)
        cells.column_shift = shift
        return cells

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().cbet_mesh_cells_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the C ABI, stated once ----------------------------------------------------------------------
# The ctypes mirror of every struct of include/cbet_mi355x.h, by its C name; tests/test_abi_host.py asks gcc for sizeof and
# every offsetof of each.
STRUCTS = {
    "cbet_params": Params, "cbet_derived": Derived, "cbet_counters": Counters, "cbet_gain_params": GainParams,
    "cbet_cbet_report": CbetReport, "cbet_ray_exit": RayExit, "cbet_path_sample": PathSample, "cbet_ray_turn": RayTurn,
    "cbet_ray_sbs": RaySbs, "cbet_lpi_summary": LpiSummary, "cbet_target": Target, "cbet_mesh": Mesh,
    "cbet_mesh_ions": MeshIons, "cbet_mesh_cells": MeshCellsStruct,
}


def _signatures():
    """name -> (return type, argument types) of every function the header declares, in the header's words: the one place
    that says how Python calls the library.  lib() binds restype and argtypes from it; tests/test_abi_host.py compares it
    with the header prototype by prototype.  A pointer the callers hand over as an address (_addr: a tensor's, an array's,
    an int) is a c_void_p whatever it points to in the header; a struct passed with byref() is a POINTER to its mirror."""
    i32, u32, i64, i64l, usz, f64, cstr = C.c_int, C.c_uint, C.c_long, C.c_longlong, C.c_size_t, C.c_double, C.c_char_p
    vp, dp, ip, lp, vpp, ullp = (C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_long),
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_ulonglong))
    P, G, T, M, MI = (C.POINTER(S) for S in (Params, GainParams, Target, Mesh, MeshIons))
    consts = [f64, f64, f64]                                        # xconst, yconst, zconst
    sph = [vp, i32, i64, P, dp, dp, i32, i32, vp, vp, vp, vp]       # cbet_sph_modes and its device flavour
    deposit = [vp, vp, i32, i64, P, i32, i32, vp, vp, vp, vp]       # cbet_mesh_deposit and its device flavour
    slab = [vp] * 5 + [i32, i32, P, G, vp, vp]                      # the gain update and the exchange matrix over planes
    segments = [vp, i64, i32, i32, vp, i64, vp, vp]
    xhost = [vp] * 4 + [i32, i32, P, G, vp, vp, f64]                # cbet_exchange_matrix_host; its successors append
    return {
        "cbet_last_error": (cstr, []),
        "cbet_version": (cstr, []),
        "cbet_params_default": (i32, [P, i32]),
        "cbet_derive": (i32, [P, C.POINTER(Derived)]),
        "cbet_live_ray_list": (i32, [P, ip, i64, lp]),
        "cbet_omega60_beam_norm": (dp, []),
        "cbet_host_power_table": (i32, [dp, dp]),
        "cbet_host_beam_trig": (i32, [dp, i32, dp]),
        "cbet_read_profile": (i32, [cstr, i32, dp, dp]),
        "cbet_safeGPUAlloc": (i32, [vpp, usz, i32]),
        "cbet_moveToAndFromGPU": (i32, [vp, vp, usz, i32]),
        "cbet_gpuFree": (i32, [vp, i32]),
        "cbet_context_create": (i32, [vpp, P, i32]),
        "cbet_context_destroy": (i32, [vp]),
        "cbet_context_counters": (i32, [vp, vp, C.POINTER(Counters), i32]),
        "cbet_context_tables": (i32, [vp, vpp, vpp]),
        "cbet_context_set_launch_list": (i32, [vp, ip, i64]),
        "cbet_launch_ray_XYZ": (i32, [i32, u32] + [vp] * 8 + consts + [P, vp, vp]),
        "cbet_tabulate_plasma": (i32, [vp, P, vp, vp, vp, vp]),
        "cbet_trace_nodes": (i32, [i32, u32] + [vp] * 7 + consts + [P, vp, vp]),
        "cbet_prepare_step_records": (i32, [vp, P, vp, vp] + consts + [vp]),
        "cbet_ray_tracing": (i32, [dp, dp, dp, dp, P, dp, ip, i32, dp, C.POINTER(Counters)]),
        "cbet_write_text": (i64l, [dp, i32, i32, i32, cstr]),
        "cbet_edep_average": (i32, [dp, dp, i32, i32, i32]),
        "cbet_edep_average_device": (i32, [vp, vp, i32, i32, i32, vp]),
        "cbet_node_coordinates": (i32, [P, dp, dp, dp]),
        "cbet_write_npy": (i64l, [dp, i32, lp, cstr]),
        "cbet_debug_bounds_violations": (i32, [ullp, i32, vp]),
        "cbet_gain_params_default": (i32, [G]),
        "cbet_gain_constants": (i32, [P, G, dp, dp, dp]),
        "cbet_trace_cbet": (i32, [i32, u32, vp, vp, vp, i32] + [vp] * 6 + consts + [P, G, vp, vp]),
        "cbet_gain_field": (i32, [vp] * 5 + [P, G, vp, vp]),
        "cbet_cbet_workspace_bytes": (usz, [P]),
        "cbet_cbet_solve": (i32, [vp] * 8 + [P, G, vp, vp, vp, C.POINTER(CbetReport)]),
        "cbet_gain_field_slab": (i32, slab),
        "cbet_gain_field_packed": (i32, slab),
        "cbet_cbet_slab_workspace_bytes": (usz, [P, i32, i32]),
        "cbet_cbet_slab_workspace_bytes_parts": (usz, [P, i32, i32, usz]),
        "cbet_pack_segments": (i32, segments),
        "cbet_unpack_segments": (i32, segments),
        "cbet_context_list_length": (i32, [vp, lp]),
        "cbet_cbet_workspace_gain": (vp, [P, vp]),
        "cbet_trace_exits": (i32, [vp] * 8 + consts + [P, G, vp, vp]),
        "cbet_exit_tally": (i32, [vp, i64, i32, vp, vp]),
        "cbet_farfield": (i32, [vp, i64, i32, i32, vp, vp]),
        "cbet_sph_modes_device": (i32, sph),
        "cbet_sph_modes": (i32, sph),
        "cbet_prepare_plasma": (i32, [vp, P, vp, vp, vp] + consts + [vp]),
        "cbet_context_step_records": (i32, [vp, vpp, ullp]),
        "cbet_tabulate_target": (i32, [vp, P, vp, vp, vp, T, vp]),
        "cbet_target_tables": (i32, [P, dp, dp, dp, T, dp, dp]),
        "cbet_tabulate_flow": (i32, [vp, P, G, T, vp]),
        "cbet_context_set_flow": (i32, [vp, vp]),
        "cbet_context_flow": (i32, [vp, vpp]),
        "cbet_flow_table": (i32, [P, G, T, dp]),
        "cbet_tabulate_mesh": (i32, [vp, P, M, vp]),
        "cbet_tabulate_mesh_flow": (i32, [vp, P, M, vp]),
        "cbet_mesh_check": (i32, [M]),
        "cbet_mesh_tables": (i32, [P, M, dp, dp]),
        "cbet_mesh_flow_table": (i32, [P, M, dp]),
        "cbet_tabulate_mesh_state": (i32, [vp, P, G, M, MI, vp]),
        "cbet_context_set_state": (i32, [vp, vp]),
        "cbet_context_state": (i32, [vp, vpp]),
        "cbet_mesh_state_table": (i32, [P, G, M, MI, dp]),
        "cbet_mesh_cells_create": (i32, [vpp, C.POINTER(MeshCellsStruct), i32, i32]),
        "cbet_mesh_cells_destroy": (None, [vp]),
        "cbet_mesh_deposit_device": (i32, deposit),
        "cbet_mesh_deposit": (i32, deposit),
        "cbet_context_set_saturation": (i32, [vp, f64]),
        "cbet_context_saturation": (i32, [vp, dp]),
        "cbet_pair_amplitude": (i32, [vp, vp, vp, i32, i32, P, G, vp, vp]),
        "cbet_exchange_matrix_work_bytes": (usz, [P]),
        "cbet_exchange_matrix": (i32, slab),
        "cbet_exchange_matrix_host": (i32, xhost),
        "cbet_context_set_detuning": (i32, [vp, vp, i32, vp]),
        "cbet_context_detuning": (i32, [vp, dp, ip]),
        "cbet_exchange_matrix_host_shifted": (i32, xhost + [vp]),
        "cbet_context_set_polarization": (i32, [vp, i32]),
        "cbet_context_polarization": (i32, [vp, ip]),
        "cbet_exchange_matrix_host_polarized": (i32, xhost + [vp, i32]),
        "cbet_context_set_bandwidth": (i32, [vp, vp, vp, i32, vp]),
        "cbet_context_bandwidth": (i32, [vp, dp, dp, ip]),
        "cbet_exchange_matrix_host_banded": (i32, xhost + [vp, i32, vp, vp, i32]),
        "cbet_trace_paths": (i32, [vp] * 5 + [i64, i32, i32, dp] + [vp] * 6 + consts + [P, G, vp, vp]),
        "cbet_lpi_work_bytes": (usz, [P]),
        "cbet_lpi_summary_init": (i32, [C.POINTER(LpiSummary)]),
        "cbet_lpi_map": (i32, [vp, vp, vp, f64, f64, f64, i32, vp, vp, vp, i32, i32, P, vp, vp]),
        "cbet_lpi_map_host": (i32, [vp, vp, vp, f64, f64, f64, i32, vp, C.POINTER(LpiSummary), i32, i32, P]),
        "cbet_trace_backscatter": (i32, [vp] * 5 + [i64, vp, dp, i32] + [vp] * 6 + consts + [P, G, vp, vp]),
        "cbet_backscatter_work_bytes": (usz, [i64, i32, i32]),
        "cbet_backscatter_tally": (i32, [vp, vp, vp, i64, i32, i32, vp, vp, vp]),
        "cbet_backscatter_host": (i32, [vp, vp, vp, i64, i32, vp, vp, vp, vp, i32, dp, i32, vp, vp, P, G]),
        "cbet_mix_work_bytes": (usz, [i64]),
        "cbet_mix_residual": (i32, [vp, vp, vp, vp, i32, i64, vp, vp, vp]),
        "cbet_mix_apply": (i32, [vp, dp, i32, i64, vp, vp, vp]),
        "cbet_mix_coefficients": (i32, [dp, i32, dp, ip]),
        "cbet_mix_residual_host": (i32, [vp, vp, vp, vp, i32, i64, dp]),
        "cbet_mix_apply_host": (i32, [vp, dp, i32, i64, vp, vp]),
    }


SIGNATURES = _signatures()
EXPORTS = list(SIGNATURES)      # every symbol include/cbet_mi355x.h declares
# lib(tolerate=...): the detuning, polarization, bandwidth, backscatter and mixing entries, which an older build may lack
OPTIONAL = frozenset((
    "cbet_mix_work_bytes", "cbet_mix_residual", "cbet_mix_apply", "cbet_mix_coefficients", "cbet_mix_residual_host",
    "cbet_mix_apply_host",
    "cbet_context_set_detuning", "cbet_context_detuning", "cbet_exchange_matrix_host_shifted",
    "cbet_context_set_polarization", "cbet_context_polarization", "cbet_exchange_matrix_host_polarized",
    "cbet_context_set_bandwidth", "cbet_context_bandwidth", "cbet_exchange_matrix_host_banded",
    "cbet_trace_backscatter", "cbet_backscatter_work_bytes", "cbet_backscatter_tally", "cbet_backscatter_host"))


_lib = None


def lib(tolerate=()):
    """Loads libcbet_mi355x.so; raises (loudly) if it has not been built.  tolerate: names of the detuning, polarization,
    bandwidth and backscatter entries that an OLDER build of the library (CBET_LIB_PATH, timing experiments against a parent commit) may lack;
    such a build must then not be asked for shifts, for a polarization mode or for a line spectrum."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process.  torch ships its own libamdhip64 / libhsa-runtime64 / librccl;
    # if libcbet_mi355x.so were loaded first it would pull in /opt/rocm's copies and the process would
    # hold two runtimes (the second to touch the device then fails, and streams / events of one mean
    # nothing to the other).  Importing torch first makes the loader resolve this library's HIP and
    # RCCL dependencies to the copies torch has already mapped (checked with scripts/which_hip.py),
    # so torch.cuda streams, events and tensors are valid arguments to every call below.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -m cbet_raytracing_3d_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        if name in OPTIONAL and name in tolerate and not hasattr(L, name):
            continue
        fn = getattr(L, name)       # AttributeError here = the library is older than the header
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _check(rc):
    if rc != OK:
        raise CbetError(rc, lib().cbet_last_error().decode("utf-8", "replace"))


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _host(x):
    """`x` -- a numpy array, a sequence or a torch tensor -- as a contiguous float64 numpy array; None stays None."""
    if x is None:
        return None
    return np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)


def _handle(ctx):
    """A Context's handle for an entry whose context is optional (None -> NULL)."""
    return None if ctx is None else ctx.handle


def _byref(struct):
    """byref() for an entry whose struct is optional (None -> NULL)."""
    return None if struct is None else C.byref(struct)


def _addr(x):
    """Device/host address of a torch tensor, numpy array, ctypes pointer or int (None -> NULL)."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if isinstance(x, C.c_void_p):
        return x.value
    raise TypeError("cannot take the address of %r" % type(x))


# ---- configuration -----------------------------------------------------------------------------
def version():
    return lib().cbet_version().decode()


def default_params(n=100, **overrides):
    p = Params()
    _check(lib().cbet_params_default(C.byref(p), n))
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def derive(p):
    d = Derived()
    _check(lib().cbet_derive(C.byref(p), C.byref(d)))
    return d


def live_ray_list(p):
    """Launch list in kernel order: 64 consecutive entries form one bundle, -1 marks a hole
    (see cbet_live_ray_list in the header)."""
    n = C.c_long()
    _check(lib().cbet_live_ray_list(C.byref(p), None, 0, C.byref(n)))
    out = np.zeros(n.value, dtype=np.int32)
    _check(lib().cbet_live_ray_list(C.byref(p), out.ctypes.data_as(C.POINTER(C.c_int)), n.value,
                                    C.byref(n)))
    return out


def shard_items(p, nbeams_local, shard_index, shard_count):
    """Host-side statement of the kernel's work split: the (beam_local, thread-ray id) pairs that
    shard `shard_index` of `shard_count` traces (a contiguous near-equal part of the beam-major bundle list)."""
    live = live_ray_list(p)
    bpb = (len(live) + 63) // 64
    beams, ids = [], []
    total = nbeams_local * bpb
    K, r = max(1, shard_count), (shard_index if shard_count > 1 else 0)
    for g in range((r * total) // K, ((r + 1) * total) // K):
        b, k = g // bpb, g % bpb
        chunk = live[64 * k: 64 * k + 64]
        chunk = chunk[chunk >= 0]
        beams.append(np.full(len(chunk), b, dtype=np.int32))
        ids.append(chunk)
    if not ids:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    return np.concatenate(beams), np.concatenate(ids)


def omega60_beam_norm():
    ptr = lib().cbet_omega60_beam_norm()
    return np.ctypeslib.as_array(ptr, shape=(60, 3)).copy()


def host_power_table():
    phase, powr = np.zeros(NPHASE), np.zeros(NPHASE)
    _check(lib().cbet_host_power_table(_dptr(phase), _dptr(powr)))
    return phase, powr


def host_beam_trig(beam_norm):
    bn = np.ascontiguousarray(beam_norm, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((bn.shape[0], 4))
    _check(lib().cbet_host_beam_trig(_dptr(bn), bn.shape[0], _dptr(out)))
    return out


def read_profile(path, nprofile=443):
    r, v = np.zeros(nprofile), np.zeros(nprofile)
    _check(lib().cbet_read_profile(os.fsencode(path), nprofile, _dptr(r), _dptr(v)))
    return r, v


def load_s83177(nprofile=443):
    """(r, ne, te) of the s83177 shot at 1.5 ns, first `nprofile` rows (main.cu:249-260:
    the Te file is read first, then the ne file, whose radii overwrite the first's)."""
    _, te = read_profile(os.path.join(DATA_DIR, "s83177_te.txt"), nprofile)
    r, ne = read_profile(os.path.join(DATA_DIR, "s83177_ne.txt"), nprofile)
    return r, ne, te


# ---- multi_gpu.cuh helpers ---------------------------------------------------------------------
def safeGPUAlloc(size, gpu):
    """multi_gpu.cpp:3-28.  Returns the device address (int)."""
    out = C.c_void_p()
    _check(lib().cbet_safeGPUAlloc(C.byref(out), size, gpu))
    return out.value


def moveToAndFromGPU(dst, src, size, gpu):
    """multi_gpu.cpp:44-59.  dst/src: addresses, numpy arrays or torch tensors."""
    _check(lib().cbet_moveToAndFromGPU(_addr(dst), _addr(src), size, gpu))


def gpuFree(ptr, gpu):
    _check(lib().cbet_gpuFree(_addr(ptr), gpu))


# ---- workspace ---------------------------------------------------------------------------------
class Context:
    """cbet_context: per-device workspace (node tables, live-ray list, counters)."""

    def __init__(self, params, gpu=0):
        self._h = C.c_void_p()
        self.gpu = gpu
        self._flow_ref = None           # set_flow(): the caller's table, kept alive
        self._state_ref = None          # set_state(): likewise
        self._given = (None, None)      # given_beam_options(): what set_detuning() and set_bandwidth() were last given
        _check(lib().cbet_context_create(C.byref(self._h), C.byref(params), gpu))

    @property
    def handle(self):
        return self._h

    def counters(self, stream=None, reset=False):
        c = Counters()
        _check(lib().cbet_context_counters(self._h, _addr(stream), C.byref(c), 1 if reset else 0))
        return c

    def set_launch_list(self, slots):
        """Regroup the bundles: `slots` holds the context's live rays, each once, 64 entries per bundle, -1 = idle lane."""
        arr = np.ascontiguousarray(slots, dtype=np.int32)
        _check(lib().cbet_context_set_launch_list(self._h, arr.ctypes.data_as(C.POINTER(C.c_int)), arr.size))

    def list_length(self):
        """L: entries of the current launch list (64 per bundle, holes included) -- the exit records' per-beam stride."""
        n = C.c_long()
        _check(lib().cbet_context_list_length(self._h, C.byref(n)))
        return n.value

    def tables(self):
        a, b = C.c_void_p(), C.c_void_p()
        _check(lib().cbet_context_tables(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def step_records(self):
        """(device address of the per-node step records, number of launches that have written them) -- for tests."""
        a, n = C.c_void_p(), C.c_ulonglong()
        _check(lib().cbet_context_step_records(self._h, C.byref(a), C.byref(n)))
        return a.value, n.value

    def set_flow(self, flow):
        """cbet_context_set_flow: the gain updates of this context read the flow from `flow`, a device table
        [3][nx][ny][nz] of doubles (a torch tensor, kept referenced here, or an address the caller keeps alive); None =
        back to the closed-form ramp about the origin."""
        _check(lib().cbet_context_set_flow(self._h, _addr(flow)))
        self._flow_ref = flow

    def flow(self):
        """Device address of the flow table in use (tabulate_flow's or set_flow's), None if none -- for tests."""
        a = C.c_void_p()
        _check(lib().cbet_context_flow(self._h, C.byref(a)))
        return a.value

    def set_state(self, state):
        """cbet_context_set_state: the gain updates of this context read the sound speed and gain_const from `state`, a
        device table [2][nx][ny][nz] of doubles (a torch tensor, kept referenced here, or an address the caller keeps
        alive); None = back to the scalars of the gain parameters."""
        _check(lib().cbet_context_set_state(self._h, _addr(state)))
        self._state_ref = state

    def state(self):
        """Device address of the state table in use (tabulate_mesh_state's or set_state's), None if none -- for tests."""
        a = C.c_void_p()
        _check(lib().cbet_context_state(self._h, C.byref(a)))
        return a.value

    def set_saturation(self, dn_max):
        """cbet_context_set_saturation: the gain updates of this context limit the ion-acoustic amplitude every beam pair's
        gain corresponds to at `dn_max` (> 0); 0 = no limit, the default.  A negative, NaN or infinite value raises."""
        _check(lib().cbet_context_set_saturation(self._h, float(dn_max)))

    def saturation(self):
        """The limit in use (cbet_context_saturation), 0.0 if none."""
        v = C.c_double()
        _check(lib().cbet_context_saturation(self._h, C.byref(v)))
        return v.value

    def set_detuning(self, domega, stream=None):
        """cbet_context_set_detuning: the gain updates of this context give beam b the angular-frequency shift domega[b]
        (rad/s, one per beam of the context's parameters); None, or shifts that are all equal, = none, the default.  A set-up
        call: it synchronises `stream` and copies synchronously.  A NaN or infinite shift or a wrong count raises.
        A RayTracer's own context is where the tracer's shifts live: RayTracer.set_detuning calls this, RayTracer.detuning reads
        the context back, and the contexts the tracer prepares later are given what this context was last given."""
        arr = None if domega is None else np.array(domega, dtype=np.float64).reshape(-1)
        _check(lib().cbet_context_set_detuning(self._h, _addr(arr), 0 if arr is None else arr.size, _addr(stream)))
        self._given = (arr, self._given[1])

    def detuning(self):
        """The shifts in use (cbet_context_detuning): a numpy array of one double per beam, or None if none."""
        out, n = np.zeros(MAX_CBET_BEAMS), C.c_int()
        _check(lib().cbet_context_detuning(self._h, _dptr(out), C.byref(n)))
        return out[:n.value].copy() if n.value else None

    def set_bandwidth(self, domega, weights=None, stream=None):
        """cbet_context_set_bandwidth: the gain updates of this context give EVERY beam the same line spectrum about its own
        centre frequency: lines at the offsets domega[a] (rad/s) with the weights weights[a] > 0 (None: equal weights), at most
        MAX_BAND_LINES of them; the library normalises the weights to sum 1.  None, one line, or offsets that are all equal =
        none, the default.  A set-up call: it synchronises `stream` and copies synchronously.  A NaN or infinite offset, a weight
        that is not finite and > 0 or too many lines raise and change nothing.  A RayTracer's own context is where the tracer's
        spectrum lives, as its shifts do (set_detuning)."""
        lines = None if domega is None else line_arrays(domega, weights)
        off, wts = lines or (None, None)
        _check(lib().cbet_context_set_bandwidth(self._h, _addr(off), _addr(wts), 0 if off is None else off.size, _addr(stream)))
        self._given = (self._given[0], lines)

    def bandwidth(self):
        """The spectrum in use (cbet_context_bandwidth): (offsets in rad/s, normalised weights), two numpy arrays of one double
        per line, or None if none."""
        off, wts, n = np.zeros(MAX_BAND_LINES), np.zeros(MAX_BAND_LINES), C.c_int()
        _check(lib().cbet_context_bandwidth(self._h, _dptr(off), _dptr(wts), C.byref(n)))
        return (off[:n.value].copy(), wts[:n.value].copy()) if n.value else None

    def set_polarization(self, mode):
        """cbet_context_set_polarization: "aligned" (every beam pair polarized alike, the default) or "smoothed" (every beam
        an equal incoherent mix of two orthogonal polarizations: each pair's gain times (1 + cos^2 theta) / 4, theta the
        pair's crossing angle in the cell), or the CBET_POL_* integer.  An unknown mode raises and changes nothing."""
        _check(lib().cbet_context_set_polarization(self._h, polarization_mode(mode)))

    def polarization(self):
        """The mode in use (cbet_context_polarization): "aligned" or "smoothed"."""
        mode = C.c_int()
        _check(lib().cbet_context_polarization(self._h, C.byref(mode)))
        return POLARIZATIONS[mode.value]

    def given_beam_options(self):
        """(shifts, (offsets, weights)): the arrays set_detuning and set_bandwidth were last given (own copies), None for none."""
        return self._given

    def adopt_beam_options(self, source, stream=None):
        """Gives this context `source`'s limit and polarization mode (host-only calls, made every time) and the shifts and lines `source`
        was last given: set-up calls that synchronise `stream`, made only if those arrays are not the very ones this context has recorded."""
        self.set_saturation(source.saturation())
        self.set_polarization(source.polarization())
        shifts, lines = source.given_beam_options()
        if self._given[0] is not shifts:
            self.set_detuning(shifts, stream)
        if self._given[1] is not lines:
            self.set_bandwidth(*(lines or (None, None)), stream=stream)
        self._given = (shifts, lines)

    def close(self):
        if self._h:
            lib().cbet_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the hot path ------------------------------------------------------------------------------
def launch_ray_XYZ(b, nindices, te_data_g, r_data_g, ne_data_g, edep, bbeam_norm, beam_norm, pow_r,
                   phase_r, xconst, yconst, zconst, params, ctx=None, stream=None):
    """launch_ray_XZ.cu:117-121 argument for argument, plus params / workspace / stream.
    Pointer arguments are device addresses (ints) or torch tensors."""
    _check(lib().cbet_launch_ray_XYZ(
        b, nindices, _addr(te_data_g), _addr(r_data_g), _addr(ne_data_g), _addr(edep),
        _addr(bbeam_norm), _addr(beam_norm), _addr(pow_r), _addr(phase_r), xconst, yconst, zconst,
        C.byref(params), _handle(ctx), _addr(stream)))


def tabulate_plasma(ctx, params, te_data_g, r_data_g, ne_data_g, stream=None):
    _check(lib().cbet_tabulate_plasma(ctx.handle, C.byref(params), _addr(te_data_g),
                                      _addr(r_data_g), _addr(ne_data_g), _addr(stream)))


def prepare_step_records(ctx, params, ne3d, kappa3d, xconst, yconst, zconst, stream=None):
    """Build the default kernel's per-node step records now instead of inside the next launch (see the header)."""
    _check(lib().cbet_prepare_step_records(ctx.handle, C.byref(params), _addr(ne3d), _addr(kappa3d), xconst, yconst,
                                           zconst, _addr(stream)))


def prepare_plasma(ctx, params, te_data_g, r_data_g, ne_data_g, xconst, yconst, zconst, stream=None):
    """tabulate_plasma + prepare_step_records of the context's own tables as one kernel (see the header)."""
    _check(lib().cbet_prepare_plasma(ctx.handle, C.byref(params), _addr(te_data_g), _addr(r_data_g), _addr(ne_data_g),
                                     xconst, yconst, zconst, _addr(stream)))


def tabulate_target(ctx, params, te_data_g, r_data_g, ne_data_g, target, stream=None):
    """cbet_tabulate_target: tabulate_plasma on a displaced / distorted target (api.Target), captured at the call."""
    _check(lib().cbet_tabulate_target(ctx.handle, C.byref(params), _addr(te_data_g), _addr(r_data_g), _addr(ne_data_g),
                                      C.byref(target), _addr(stream)))


def target_tables(params, r_profile, ne_profile, te_profile, target):
    """cbet_target_tables, the host twin: numpy (ne3d, kappa3d), each (nx, ny, nz), from host profiles."""
    r, ne, te = (np.ascontiguousarray(a, dtype=np.float64) for a in (r_profile, ne_profile, te_profile))
    if not (r.size == ne.size == te.size == params.nprofile):
        raise ValueError("profile length != params.nprofile")
    shape = (params.nx, params.ny, params.nz)
    ne3d, kap = np.empty(shape), np.empty(shape)
    _check(lib().cbet_target_tables(C.byref(params), _dptr(te), _dptr(r), _dptr(ne), C.byref(target), _dptr(ne3d), _dptr(kap)))
    return ne3d, kap


def tabulate_flow(ctx, params, gain_params, target=None, stream=None):
    """cbet_tabulate_flow: the gain kernels' flow on `target` (api.Target; None = the sphere about the origin) into the
    context's own flow table, which the context's gain updates then read.  The first call on a context allocates."""
    _check(lib().cbet_tabulate_flow(ctx.handle, C.byref(params), C.byref(gain_params),
                                    _byref(target), _addr(stream)))
    ctx._flow_ref = None


def flow_table(params, gain_params, target=None):
    """cbet_flow_table, the host twin: numpy (3, nx, ny, nz) -- ux, uy, uz at the nodes."""
    out = np.empty((3, params.nx, params.ny, params.nz))
    _check(lib().cbet_flow_table(C.byref(params), C.byref(gain_params), _byref(target),
                                 _dptr(out)))
    return out


def tabulate_mesh(ctx, params, mesh, stream=None):
    """cbet_tabulate_mesh: the context's node tables from a DEVICE mesh (api.Mesh(...).to(device))."""
    _check(lib().cbet_tabulate_mesh(ctx.handle, C.byref(params), C.byref(mesh), _addr(stream)))


def tabulate_mesh_flow(ctx, params, mesh, stream=None):
    """cbet_tabulate_mesh_flow: a DEVICE mesh's velocity into the context's own flow table, which the context's gain
    updates then read.  The first call on a context allocates."""
    _check(lib().cbet_tabulate_mesh_flow(ctx.handle, C.byref(params), C.byref(mesh), _addr(stream)))
    ctx._flow_ref = None


def tabulate_mesh_state(ctx, params, gain_params, mesh, stream=None, ions=True):
    """cbet_tabulate_mesh_state: a DEVICE mesh's Te -- and its ti / zbar (Mesh.ions), where it has them; ions=False: the
    gain parameters' ti_ev / z_ion whatever the mesh carries -- into the context's own state table (cs, gain_const), which
    the context's gain updates then read.  The first call on a context allocates."""
    _check(lib().cbet_tabulate_mesh_state(ctx.handle, C.byref(params), C.byref(gain_params), C.byref(mesh),
                                          C.byref(mesh.ions) if ions else None, _addr(stream)))
    ctx._state_ref = None


def mesh_state_table(params, gain_params, mesh, ions=True):
    """cbet_mesh_state_table, the host twin: numpy (2, nx, ny, nz) -- cs, gain_const at the nodes -- from a HOST mesh."""
    out = np.empty((2, params.nx, params.ny, params.nz))
    _check(lib().cbet_mesh_state_table(C.byref(params), C.byref(gain_params), C.byref(mesh),
                                       C.byref(mesh.ions) if ions else None, _dptr(out)))
    return out


def mesh_check(mesh):
    """cbet_mesh_check: the host twins' validation of a HOST mesh alone (raises CbetError naming the first offence)."""
    _check(lib().cbet_mesh_check(C.byref(mesh)))


def mesh_tables(params, mesh):
    """cbet_mesh_tables, the host twin: numpy (ne3d, kappa3d), each (nx, ny, nz), from a HOST mesh."""
    shape = (params.nx, params.ny, params.nz)
    ne3d, kap = np.empty(shape), np.empty(shape)
    _check(lib().cbet_mesh_tables(C.byref(params), C.byref(mesh), _dptr(ne3d), _dptr(kap)))
    return ne3d, kap


def mesh_flow_table(params, mesh):
    """cbet_mesh_flow_table, the host twin: numpy (3, nx, ny, nz) -- ux, uy, uz at the nodes -- from a HOST mesh."""
    out = np.empty((3, params.nx, params.ny, params.nz))
    _check(lib().cbet_mesh_flow_table(C.byref(params), C.byref(mesh), _dptr(out)))
    return out


def trace_nodes(b, nindices, ne3d, kappa3d, edep, bbeam_norm, beam_norm, pow_r, phase_r, xconst,
                yconst, zconst, params, ctx, stream=None):
    _check(lib().cbet_trace_nodes(
        b, nindices, _addr(ne3d), _addr(kappa3d), _addr(edep), _addr(bbeam_norm), _addr(beam_norm),
        _addr(pow_r), _addr(phase_r), xconst, yconst, zconst, C.byref(params), ctx.handle,
        _addr(stream)))


# ---- CBET stage (parity unpinned) -----------------------------------------------
def default_gain_params(**overrides):
    g = GainParams()
    _check(lib().cbet_gain_params_default(C.byref(g)))
    for k, v in overrides.items():
        setattr(g, k, v)
    return g


def gain_constants(params, gain_params):
    """(constant1, cs, gain_const) of def.cuh:111, 113."""
    out = [C.c_double() for _ in range(3)]
    _check(lib().cbet_gain_constants(C.byref(params), C.byref(gain_params), *[C.byref(o) for o in out]))
    return tuple(o.value for o in out)


def trace_cbet(b, nindices, ne3d, kappa3d, gain, quantity, out, beam_gain, bbeam_norm, beam_norm, pow_r,
               phase_r, xconst, yconst, zconst, params, gain_params, ctx, stream=None):
    _check(lib().cbet_trace_cbet(
        b, nindices, _addr(ne3d), _addr(kappa3d), _addr(gain), quantity, _addr(out), _addr(beam_gain),
        _addr(bbeam_norm), _addr(beam_norm), _addr(pow_r), _addr(phase_r), xconst, yconst, zconst,
        C.byref(params), C.byref(gain_params), ctx.handle, _addr(stream)))


def gain_field(fields, ne3d, gain, scratch, change, params, gain_params, ctx, stream=None):
    _check(lib().cbet_gain_field(_addr(fields), _addr(ne3d), _addr(gain), _addr(scratch), _addr(change),
                                 C.byref(params), C.byref(gain_params), ctx.handle, _addr(stream)))


def gain_field_packed(fields, ne3d, gain, scratch, change, hx_lo, hx_hi, params, gain_params, ctx, stream=None):
    """cbet_gain_field_slab on slab-packed arrays (planes [hx_lo, hx_hi) of every beam only)."""
    _check(lib().cbet_gain_field_packed(_addr(fields), _addr(ne3d), _addr(gain), _addr(scratch), _addr(change), hx_lo, hx_hi,
                                        C.byref(params), C.byref(gain_params), ctx.handle, _addr(stream)))


def pack_segments(src, beam_stride, hy, hz, segments, nseg, out, stream=None):
    """cbet_pack_segments: gather the 64-byte z-runs listed in `segments` (device int32 [nseg][2]) of `src` into `out`."""
    _check(lib().cbet_pack_segments(_addr(src), beam_stride, hy, hz, _addr(segments), nseg, _addr(out), _addr(stream)))


def unpack_segments(dst, beam_stride, hy, hz, segments, nseg, buf, stream=None):
    """cbet_unpack_segments: scatter `buf` (nseg runs of 8 doubles) into the listed runs of `dst`."""
    _check(lib().cbet_unpack_segments(_addr(dst), beam_stride, hy, hz, _addr(segments), nseg, _addr(buf), _addr(stream)))


def cbet_slab_workspace_bytes(params, world_size, rank):
    return int(lib().cbet_cbet_slab_workspace_bytes(C.byref(params), world_size, rank))


def cbet_slab_workspace_bytes_parts(params, own_beams, own_planes, staging_doubles=0):
    return int(lib().cbet_cbet_slab_workspace_bytes_parts(C.byref(params), own_beams, own_planes, staging_doubles))


def gain_field_slab(fields, ne3d, gain, scratch, change, hx_lo, hx_hi, params, gain_params, ctx, stream=None):
    _check(lib().cbet_gain_field_slab(_addr(fields), _addr(ne3d), _addr(gain), _addr(scratch), _addr(change), hx_lo, hx_hi,
                                      C.byref(params), C.byref(gain_params), ctx.handle, _addr(stream)))


def pair_amplitude(fields, ne3d, amp, hx_lo, hx_hi, params, gain_params, ctx, stream=None):
    """cbet_pair_amplitude: into `amp` (whole-grid [hsize] doubles), for the planes [hx_lo, hx_hi), the largest ion-acoustic
    amplitude any beam pair's unclamped gain corresponds to, from the NORMALISED `fields` a gain update leaves."""
    _check(lib().cbet_pair_amplitude(_addr(fields), _addr(ne3d), _addr(amp), hx_lo, hx_hi, C.byref(params), C.byref(gain_params),
                                     _handle(ctx), _addr(stream)))


def exchange_matrix_work_bytes(params):
    """cbet_exchange_matrix_work_bytes: device bytes of the `work` array of exchange_matrix, for any slab of the grid."""
    return int(lib().cbet_exchange_matrix_work_bytes(C.byref(params)))


def exchange_matrix(fields, ne3d, out, gross, work, hx_lo, hx_hi, params, gain_params, ctx, stream=None):
    """cbet_exchange_matrix: the pairwise exchange of the NORMALISED device `fields` over the planes [hx_lo, hx_hi), ADDED into
    the upper triangle of `out` (device [nbeams, nbeams]: out[i, j] = the energy beam i gains from beam j per field pass; lower
    triangle negated, diagonal zero) and of `gross` (the sum of magnitudes, symmetric; may be None).  The context's flow and
    state tables and its saturation limit are honoured."""
    _check(lib().cbet_exchange_matrix(_addr(fields), _addr(ne3d), _addr(out), _addr(gross), _addr(work), hx_lo, hx_hi,
                                      C.byref(params), C.byref(gain_params), _handle(ctx), _addr(stream)))


def lpi_work_bytes(params):
    """cbet_lpi_work_bytes: device bytes of the `work` array of lpi_map, for any slab of the grid."""
    return int(lib().cbet_lpi_work_bytes(C.byref(params)))


def lpi_summary_new():
    """A cbet_lpi_summary as cbet_lpi_summary_init leaves it: zeros, argmax_cw = -1."""
    s = LpiSummary()
    _check(lib().cbet_lpi_summary_init(C.byref(s)))
    return s


def lpi_summary_from(buffer):
    """The summary a device call merged into `buffer` (a uint8 tensor or array of LPI_SUMMARY_BYTES bytes), as a dict."""
    raw = buffer.cpu().numpy() if hasattr(buffer, "cpu") else np.asarray(buffer)
    return LpiSummary.from_buffer_copy(np.ascontiguousarray(raw).tobytes()).as_dict()


def lpi_map(fields, ne3d, te3d, te_ev, frac_lo, frac_hi, cone_bins, lpi, summary, work, hx_lo, hx_hi, params, ctx, stream=None):
    """cbet_lpi_map: into `lpi` (device [LPI_NQ][hsize] doubles), for the planes [hx_lo, hx_hi), the quarter-critical LPI maps
    of the NORMALISED device `fields`; summary: a device cbet_lpi_summary to merge into (with `work`), or None."""
    _check(lib().cbet_lpi_map(_addr(fields), _addr(ne3d), _addr(te3d), te_ev, frac_lo, frac_hi, cone_bins, _addr(lpi),
                              _addr(summary), _addr(work), hx_lo, hx_hi, C.byref(params),
                              _handle(ctx), _addr(stream)))


def lpi_map_host(fields, ne3d, params, te=1000.0, band=(0.20, 0.25), cone_bins=8, hx_lo=0, hx_hi=None, out=None, summary=None):
    """cbet_lpi_map_host, the host twin: (stack [LPI_NQ, nx + 2, ny + 2, nz + 2], summary dict) of normalised HOST fields
    [4, nbeams, nx + 2, ny + 2, nz + 2] over the planes [hx_lo, hx_hi).  ne3d (nx, ny, nz); te: a float (eV, uniform) or an
    (nx, ny, nz) array; out: a stack to write the planes of (default: a zeroed new one); summary: an LpiSummary to merge
    into (default: a new one)."""
    fields, ne3d = _host(fields), _host(ne3d)
    te3d, te_ev = (None, float(te)) if np.isscalar(te) else (_host(te), 0.0)
    grid = (params.nx + 2, params.ny + 2, params.nz + 2)
    out = np.zeros((LPI_NQ,) + grid) if out is None else out
    summary = lpi_summary_new() if summary is None else summary
    _check(lib().cbet_lpi_map_host(_addr(fields), _addr(ne3d), _addr(te3d), te_ev, float(band[0]), float(band[1]), int(cone_bins),
                                   _addr(out), C.byref(summary), hx_lo, grid[0] if hx_hi is None else hx_hi, C.byref(params)))
    return out, summary.as_dict()


POL_ALIGNED, POL_SMOOTHED = 0, 1                # CBET_POL_* of the header
POLARIZATIONS = ("aligned", "smoothed")


def polarization_mode(mode):
    """A polarization mode by name ("aligned", "smoothed") as the header's CBET_POL_* integer; an integer passes as it is (the
    library judges it)."""
    if isinstance(mode, str):
        if mode not in POLARIZATIONS:
            raise ValueError("polarization is one of %s, got %r" % (", ".join(repr(m) for m in POLARIZATIONS), mode))
        return POLARIZATIONS.index(mode)
    return int(mode)


def wavelength_shift_to_domega(params, dlambda_angstrom):
    """Wavelength shifts (Angstrom, scalar or array; > 0 = red) of the nominal wavelength l0 = 2 pi c / omega of `params` as
    angular-frequency shifts in rad/s: omega l0 / (l0 + dl) - omega, not its first-order form."""
    omega = derive(params).omega
    lam0 = 2.0 * np.pi * 29979245800.0 / omega          # cm; the library's c (cbet_device.h kC)
    dl = np.asarray(dlambda_angstrom, dtype=np.float64) * 1e-8
    return omega * lam0 / (lam0 + dl) - omega


MAX_BAND_LINES = 8                              # CBET_MAX_BAND_LINES of the header
LINE_SHAPES = ("flat", "gaussian")


def line_arrays(domega, weights=None):
    """A line spectrum as two contiguous float64 arrays of equal length (offsets, weights); weights None = equal weights.  The
    library judges the values."""
    off = np.array(domega, dtype=np.float64).reshape(-1)
    wts = np.ones(off.size) if weights is None else np.array(weights, dtype=np.float64).reshape(-1)
    if wts.size != off.size:
        raise ValueError("a line spectrum holds one weight per offset: %d offsets, %d weights" % (off.size, wts.size))
    return off, wts


def line_spectrum(params, width_angstrom, nlines, shape="flat"):
    """A line spectrum of `nlines` lines equally spaced in wavelength across `width_angstrom` (the distance between the outermost
    lines, centred on the nominal wavelength of `params`) as (domega, weights): offsets in rad/s through the exact
    wavelength_shift_to_domega, red lines first; weights that sum to 1 -- "flat": equal; "gaussian": exp(-4 ln 2 (dl / width)^2),
    the width taken as the full width at half maximum, so the outermost lines carry half the centre's weight.  One line is
    (0, 1): no spectrum."""
    if shape not in LINE_SHAPES:
        raise ValueError("shape is one of %s, got %r" % (", ".join(repr(s) for s in LINE_SHAPES), shape))
    if not 1 <= int(nlines) <= MAX_BAND_LINES:
        raise ValueError("nlines = %r: 1 .. %d lines" % (nlines, MAX_BAND_LINES))
    if not np.isfinite(width_angstrom) or width_angstrom < 0:
        raise ValueError("width_angstrom = %r: a finite width >= 0" % (width_angstrom,))
    nlines = int(nlines)
    dl = np.linspace(0.5 * width_angstrom, -0.5 * width_angstrom, nlines) if nlines > 1 else np.zeros(1)
    weights = np.ones(nlines) if shape == "flat" or width_angstrom == 0 else np.exp(-4.0 * np.log(2.0) * (dl / width_angstrom) ** 2)
    return wavelength_shift_to_domega(params, dl), weights / weights.sum()


def exchange_matrix_host(fields, ne3d, params, gain_params, flow=None, state=None, dn_max=0.0, hx_lo=0, hx_hi=None, out=None,
                         gross=None, shift=None, polarization="aligned", lines=None):
    """cbet_exchange_matrix_host, the host twin: numpy (T, Gross), each (nbeams, nbeams), of normalised HOST fields
    [4, nbeams, nx + 2, ny + 2, nz + 2] over the planes [hx_lo, hx_hi).  ne3d (nx, ny, nz); flow (3, nx, ny, nz) or None = the
    closed-form ramp; state (2, nx, ny, nz) or None = the scalars; dn_max 0 = no limit; shift (nbeams,) per-beam frequency
    shifts in rad/s or None; polarization "aligned" or "smoothed"; lines (offsets in rad/s, weights) of the spectrum every beam
    carries, or None (cbet_exchange_matrix_host_banded).  out / gross: arrays to ADD into (default: new zeroed ones)."""
    nb = params.nbeams
    fields, ne3d, flow, state, shift = (_host(a) for a in (fields, ne3d, flow, state, shift))
    if shift is not None and shift.shape != (nb,):
        raise ValueError("shift holds one value per beam: shape (%d,), got %r" % (nb, shift.shape))
    out = np.zeros((nb, nb)) if out is None else out
    gross = np.zeros((nb, nb)) if gross is None else gross
    pol = polarization_mode(polarization)
    off, wts = (None, None) if lines is None else line_arrays(*lines)
    _check(lib().cbet_exchange_matrix_host_banded(_addr(fields), _addr(ne3d), _addr(out), _addr(gross), hx_lo,
                                                  params.nx + 2 if hx_hi is None else hx_hi, C.byref(params),
                                                  C.byref(gain_params), _addr(flow), _addr(state), dn_max, _addr(shift), pol,
                                                  _addr(off), _addr(wts), 0 if off is None else off.size))
    return out, gross


def cbet_workspace_bytes(params):
    return int(lib().cbet_cbet_workspace_bytes(C.byref(params)))


def cbet_solve(te_data_g, r_data_g, ne_data_g, edep, bbeam_norm, beam_norm, pow_r, phase_r, params,
               gain_params, workspace=None, ctx=None, stream=None):
    rep = CbetReport()
    _check(lib().cbet_cbet_solve(_addr(te_data_g), _addr(r_data_g), _addr(ne_data_g), _addr(edep),
                                 _addr(bbeam_norm), _addr(beam_norm), _addr(pow_r), _addr(phase_r),
                                 C.byref(params), C.byref(gain_params), _addr(workspace),
                                 _handle(ctx), _addr(stream), C.byref(rep)))
    return rep


def cbet_workspace_gain(params, workspace):
    """Device address of the converged gain inside a workspace cbet_solve has run in ([nbeams][(n+2)^3] doubles)."""
    addr = lib().cbet_cbet_workspace_gain(C.byref(params), _addr(workspace))
    if not addr:
        raise CbetError(EINVAL, lib().cbet_last_error().decode("utf-8", "replace"))
    return addr


# ---- exit pass ---------------------------------------------------------------------------------------
def trace_exits(ne3d, kappa3d, gain, exits, bbeam_norm, beam_norm, pow_r, phase_r, xconst, yconst, zconst, params,
                gain_params, ctx, stream=None):
    """cbet_trace_exits: one cbet_ray_exit record per ray into `exits` ([grid beams][L] records, device)."""
    _check(lib().cbet_trace_exits(
        _addr(ne3d), _addr(kappa3d), _addr(gain), _addr(exits), _addr(bbeam_norm), _addr(beam_norm), _addr(pow_r),
        _addr(phase_r), xconst, yconst, zconst, C.byref(params), _byref(gain_params),
        ctx.handle, _addr(stream)))


def exit_tally(exits, L, nbeams, tally, stream=None):
    """cbet_exit_tally: tally[nbeams][8] (TALLY_COLUMNS) overwritten with the per-beam energy balance."""
    _check(lib().cbet_exit_tally(_addr(exits), L, nbeams, _addr(tally), _addr(stream)))


def farfield(exits, n, ntheta, nphi, hist, stream=None):
    """cbet_farfield: the escaped rays' energy among n records ADDED into hist[ntheta][nphi]."""
    _check(lib().cbet_farfield(_addr(exits), n, ntheta, nphi, _addr(hist), _addr(stream)))


# ---- ray path recorder --------------------------------------------------------------------------
def path_items(beams, raynums):
    """The item list of cbet_trace_paths as two contiguous int32 numpy arrays of one length, or ValueError: the arrays must
    be one-dimensional, equally long, of an integer dtype, and hold values an int32 holds.  (Which VALUES name a ray is the
    kernel's test: anything else is an idle item.)  No library call."""
    out = []
    for what, a in (("beams", beams), ("raynums", raynums)):
        a = np.asarray(a)
        if a.ndim != 1:
            raise ValueError("%s must be one-dimensional, got shape %s" % (what, a.shape))
        if a.size and a.dtype.kind not in "iu":        # (an empty list has no dtype to speak of)
            raise ValueError("%s must hold integers, got dtype %s" % (what, a.dtype))
        lim = np.iinfo(np.int32)
        if a.size and (int(a.min()) < lim.min or int(a.max()) > lim.max):
            raise ValueError("%s holds values outside the int32 range" % what)
        out.append(np.ascontiguousarray(a, dtype=np.int32))
    if out[0].size != out[1].size:
        raise ValueError("beams and raynums differ in length: %d and %d" % (out[0].size, out[1].size))
    return out[0], out[1]


def trace_paths(ne3d, kappa3d, gain, beams, raynums, nitems, stride, capacity, center, samples, turns, bbeam_norm, beam_norm,
                pow_r, phase_r, xconst, yconst, zconst, params, gain_params, ctx, stream=None):
    """cbet_trace_paths: the rays (beams[k], raynums[k]) (device int32) traced with a sample every `stride` steps into
    samples ([capacity][nitems] cbet_path_sample, device) and one closest-approach record each into turns ([nitems])."""
    c = np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    _check(lib().cbet_trace_paths(
        _addr(ne3d), _addr(kappa3d), _addr(gain), _addr(beams), _addr(raynums), nitems, stride, capacity,
        c.ctypes.data_as(C.POINTER(C.c_double)), _addr(samples), _addr(turns), _addr(bbeam_norm), _addr(beam_norm),
        _addr(pow_r), _addr(phase_r), xconst, yconst, zconst, C.byref(params),
        _byref(gain_params), ctx.handle, _addr(stream)))


# ---- backscatter SBS gain spectra ---------------------------------------------------------------
def sbs_shifts(domega):
    """The scan of cbet_trace_backscatter as a contiguous float64 array: 1 .. SBS_MAX_SHIFTS finite angular-frequency shifts of
    the scattered light relative to its beam (rad/s, negative = red), or ValueError.  No library call."""
    s = np.ascontiguousarray(domega, dtype=np.float64).reshape(-1)
    if not 1 <= s.size <= SBS_MAX_SHIFTS:
        raise ValueError("a backscatter scan holds 1 .. %d shifts, got %d" % (SBS_MAX_SHIFTS, s.size))
    if not np.isfinite(s).all():
        raise ValueError("a backscatter scan's shifts must be finite")
    return s


def trace_backscatter(ne3d, kappa3d, gain, beams, raynums, nitems, fields, shifts, gamma, rays, bbeam_norm, beam_norm, pow_r,
                      phase_r, xconst, yconst, zconst, params, gain_params, ctx, stream=None):
    """cbet_trace_backscatter: the rays (beams[k], raynums[k]) (device int32) traced as cbet_trace_paths traces them, the SBS
    backscatter gain exponent of every shift (host float64 array) into gamma ([nshift][nitems], device) and one cbet_ray_sbs
    each into rays ([nitems], device); fields: normalised device fields [4][nbeams][grid]."""
    s = np.ascontiguousarray(shifts, dtype=np.float64).reshape(-1)
    _check(lib().cbet_trace_backscatter(
        _addr(ne3d), _addr(kappa3d), _addr(gain), _addr(beams), _addr(raynums), nitems, _addr(fields), _dptr(s), int(s.size),
        _addr(gamma), _addr(rays), _addr(bbeam_norm), _addr(beam_norm), _addr(pow_r), _addr(phase_r), xconst, yconst, zconst,
        C.byref(params), _byref(gain_params), ctx.handle, _addr(stream)))


def backscatter_work_bytes(nitems, nshift, nbeams):
    """cbet_backscatter_work_bytes: device bytes of the `work` array of backscatter_tally (0 for bad arguments)."""
    return int(lib().cbet_backscatter_work_bytes(nitems, nshift, nbeams))


def backscatter_tally(gamma, rays, beams, nitems, nshift, nbeams, tally, work, stream=None):
    """cbet_backscatter_tally: per beam and shift {sum uray0, sum uray0 Gamma, max Gamma, rays} over the launched items,
    MERGED INTO tally (device float64 [nbeams][nshift][4]); deterministic."""
    _check(lib().cbet_backscatter_tally(_addr(gamma), _addr(rays), _addr(beams), nitems, nshift, nbeams, _addr(tally), _addr(work),
                                        _addr(stream)))


def backscatter_host(samples, turns, beams, fields, ne3d, shifts, params, gain_params, flow=None, state=None,
                     polarization="aligned"):
    """cbet_backscatter_host, the host twin: (gamma float64 [nshift, nitems], rays [nitems] of SBS_DTYPE) from STRIDE-1 path
    records of the items -- samples [capacity, nitems] of PATH_DTYPE (or float64 [capacity, nitems, 8]), turns [nitems] of
    TURN_DTYPE (or float64 [nitems, 8]), as trace_paths writes them -- their beams, normalised HOST fields
    [4, nbeams, nx + 2, ny + 2, nz + 2], ne3d (nx, ny, nz), flow (3, nx, ny, nz) or None = the closed-form ramp, state
    (2, nx, ny, nz) or None = the scalars, and a polarization mode."""
    fields, ne3d, flow, state = (_host(a) for a in (fields, ne3d, flow, state))
    samples, turns = np.ascontiguousarray(samples), np.ascontiguousarray(turns)
    b = np.ascontiguousarray(beams, dtype=np.int32).reshape(-1)
    nitems = int(b.size)
    if turns.nbytes != nitems * 64:
        raise ValueError("turns holds one 64-byte record per item: %d items, %d bytes" % (nitems, turns.nbytes))
    capacity = samples.nbytes // (64 * nitems) if nitems else 0
    if samples.nbytes != capacity * nitems * 64:
        raise ValueError("samples holds capacity x nitems 64-byte records, got %d bytes for %d items" % (samples.nbytes, nitems))
    s = np.ascontiguousarray(shifts, dtype=np.float64).reshape(-1)
    gamma = np.zeros((s.size, nitems))
    rays = np.zeros(nitems, dtype=SBS_DTYPE)
    one = np.zeros(1)                          # (empty arrays have no address to speak of)
    _check(lib().cbet_backscatter_host(_addr(samples) if samples.size else None, _addr(turns) if nitems else _addr(one),
                                       _addr(b) if nitems else None, nitems, capacity, _addr(fields), _addr(ne3d), _addr(flow),
                                       _addr(state), polarization_mode(polarization), _dptr(s), int(s.size),
                                       _addr(gamma) if gamma.size else _addr(one), _addr(rays) if nitems else _addr(one),
                                       C.byref(params), _byref(gain_params)))
    return gamma, rays


# ---- Anderson mixing of the gain iterate --------------------------------------------------------
MIX_MAX_DEPTH, MIX_SPAN, MIX_MAX_GROUPS = 4, 2048, 2048        # CBET_MIX_* of the header


def _pointers(arrays):
    """The addresses of `arrays` as a C array of pointers (None for an empty list); keep it alive across the call."""
    return (C.c_void_p * len(arrays))(*[_addr(a) for a in arrays]) if len(arrays) else None


def _numel(a):
    return int(a.numel()) if hasattr(a, "numel") else int(a.size)


def mix_work_bytes(n):
    """cbet_mix_work_bytes: device bytes of the `work` array of mix_residual for arrays of n doubles (0 for n < 0)."""
    return int(lib().cbet_mix_work_bytes(n))


def mix_residual(y, x, f, f_held, row, work, n=None, stream=None):
    """cbet_mix_residual on device arrays of n doubles (default: y's size): f = y - x, and into `row` (device, len(f_held) + 1
    doubles) the dot products of f with every held residual of the list f_held (oldest first) and with itself."""
    held = _pointers(f_held)
    _check(lib().cbet_mix_residual(_addr(y), _addr(x), _addr(f), held, len(f_held), _numel(y) if n is None else n, _addr(row),
                                   _addr(work), _addr(stream)))


def mix_apply(y_held, alpha, x_out, x_keep=None, n=None, stream=None):
    """cbet_mix_apply on device arrays of n doubles (default: x_out's size): sum_j alpha[j] y_held[j], oldest first, into x_out
    (which may be one of y_held) and x_keep (or None).  alpha: len(y_held) host floats."""
    al = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
    if al.size != len(y_held):
        raise ValueError("mix_apply takes one coefficient per held iterate, got %d for %d" % (al.size, len(y_held)))
    held = _pointers(y_held)
    _check(lib().cbet_mix_apply(held, _dptr(al) if al.size else None, len(y_held), _numel(x_out) if n is None else n, _addr(x_out),
                                _addr(x_keep), _addr(stream)))


def mix_coefficients(gram):
    """cbet_mix_coefficients: (alpha float64 [count], dropped) from the count x count Gram matrix of the held residuals, oldest
    first.  Pure host arithmetic: the same bytes on every rank that passes the same numbers."""
    g = np.ascontiguousarray(gram, dtype=np.float64)
    count = g.shape[0] if g.ndim == 2 and g.shape[0] == g.shape[1] else 0
    alpha, dropped = np.zeros(max(count, 1)), C.c_int(0)
    _check(lib().cbet_mix_coefficients(_dptr(g) if g.size else None, count, _dptr(alpha), C.byref(dropped)))
    return alpha, int(dropped.value)


def mix_residual_host(y, x, f, f_held, n=None):
    """cbet_mix_residual_host, the host twin on contiguous float64 numpy arrays: writes f, returns the row [len(f_held) + 1]."""
    row = np.zeros(len(f_held) + 1)
    held = _pointers(f_held)
    _check(lib().cbet_mix_residual_host(_addr(y), _addr(x), _addr(f), held, len(f_held), _numel(y) if n is None else n, _dptr(row)))
    return row


def mix_apply_host(y_held, alpha, x_out, x_keep=None, n=None):
    """cbet_mix_apply_host, the host twin on contiguous float64 numpy arrays (x_out may be one of y_held)."""
    al = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
    if al.size != len(y_held):
        raise ValueError("mix_apply_host takes one coefficient per held iterate, got %d for %d" % (al.size, len(y_held)))
    held = _pointers(y_held)
    _check(lib().cbet_mix_apply_host(held, _dptr(al) if al.size else None, len(y_held), _numel(x_out) if n is None else n,
                                     _addr(x_out), _addr(x_keep)))


# ---- deposit grids as cbet_sph_modes and cbet_mesh_deposit take them ------------------------------------------------
def grid_layout(shape, params):
    """One grid, a padded grid or a stack: what the shape of a deposit array says, as (ngrids, grid_stride, params with
    edep_zpitch set, stacked).  shape: (nx+2, ny+2, row) -- one grid -- or (G, nx+2, ny+2, row) -- a stack of G, `stacked`
    then True -- with row = nz + 2, or longer: padded rows, edep_zpitch = row (0 for dense rows); None: no array (geometry
    mode, counts alone), one grid.  grid_stride is one grid's doubles, (nx+2)(ny+2) row; the library reads it only with
    ngrids > 1.  Any other shape is a ValueError."""
    p = params.copy(edep_zpitch=0)
    if shape is None:
        return 1, 0, p, False
    shape = tuple(int(n) for n in shape)
    if len(shape) not in (3, 4) or shape[-3:-1] != (p.nx + 2, p.ny + 2) or shape[-1] < p.nz + 2:
        raise ValueError("a deposit grid is (nx+2, ny+2, >= nz+2) = (%d, %d, >= %d), or a [G, ...] stack of them, got %s"
                         % (p.nx + 2, p.ny + 2, p.nz + 2, shape))
    if shape[-1] > p.nz + 2:
        p.edep_zpitch = shape[-1]
    return (shape[0] if len(shape) == 4 else 1), shape[-3] * shape[-2] * shape[-1], p, len(shape) == 4


# ---- mode spectra (cbet_sph_modes) ------------------------------------------------------------
def _sph_geometry(center, r_edges):
    c = np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    e = np.ascontiguousarray(r_edges, dtype=np.float64).reshape(-1)
    return c, e


def sph_modes(edep, ngrids, grid_stride, params, center, r_edges, lmax, coeffs, shell_energy, shell_nodes, stream=None):
    """cbet_sph_modes_device: device grids (edep None = geometry mode) and outputs, OVERWRITTEN -- coeffs
    [ngrids][nshell][(lmax+1)^2], shell_energy [ngrids][nshell], shell_nodes int64 [nshell].  center and r_edges are
    host values (nshell = len(r_edges) - 1).  Enqueued on `stream`."""
    c, e = _sph_geometry(center, r_edges)
    _check(lib().cbet_sph_modes_device(_addr(edep), ngrids, grid_stride, C.byref(params), _dptr(c), _dptr(e), e.size - 1,
                                       lmax, _addr(coeffs), _addr(shell_energy), _addr(shell_nodes), _addr(stream)))


def sph_modes_host(edep, params, center, r_edges, lmax):
    """cbet_sph_modes on host arrays: edep a float64 numpy grid (nx+2, ny+2, row), a stack (G, nx+2, ny+2, row) of them,
    or None (geometry mode); a row longer than nz + 2 is a padded row (cbet_params.edep_zpitch).
    Returns numpy (coeffs [G][nshell][(lmax+1)^2], shell_energy [G][nshell], shell_nodes int64 [nshell])."""
    c, e = _sph_geometry(center, r_edges)
    a = _host(edep)
    ngrids, stride, p, _ = grid_layout(None if a is None else a.shape, params)
    nshell, ncoef = e.size - 1, (lmax + 1) ** 2
    coeffs = np.zeros((ngrids, max(nshell, 0), ncoef))
    energy = np.zeros((ngrids, max(nshell, 0)))
    nodes = np.zeros(max(nshell, 0), dtype=np.int64)
    _check(lib().cbet_sph_modes(_addr(a), ngrids, stride, C.byref(p), _dptr(c), _dptr(e), nshell, lmax, _addr(coeffs),
                                _addr(energy), _addr(nodes), None))
    return coeffs, energy, nodes


# ---- deposit on the hydro mesh (cbet_mesh_deposit) --------------------------------------------
def mesh_deposit(cells, edep, ngrids, grid_stride, params, subsamples, method, cell_energy, outside, cell_samples, stream=None):
    """cbet_mesh_deposit_device: device grids (edep None: counts alone) binned into `cells` (a MeshCells made with a gpu);
    outputs OVERWRITTEN -- cell_energy [ngrids][nr][ntheta][nphi], outside [ngrids], cell_samples int64 [nr][ntheta][nphi].
    method: MESH_DEPOSIT_AUTO, _GLOBAL or _LDS.  Enqueued on `stream`."""
    _check(lib().cbet_mesh_deposit_device(cells.handle, _addr(edep), ngrids, grid_stride, C.byref(params), subsamples, method,
                                          _addr(cell_energy), _addr(outside), _addr(cell_samples), _addr(stream)))


def mesh_deposit_host(cells, edep, params, subsamples=2):
    """cbet_mesh_deposit, the host twin, on host arrays: edep as sph_modes_host takes it -- a float64 numpy grid
    (nx+2, ny+2, row), a stack (G, nx+2, ny+2, row), or None (counts alone).  Returns numpy (cell_energy [G][nr][ntheta][nphi],
    outside [G], cell_samples int64 [nr][ntheta][nphi])."""
    a = _host(edep)
    ngrids, stride, p, _ = grid_layout(None if a is None else a.shape, params)
    energy = np.zeros((ngrids,) + cells.shape)
    outside = np.zeros(ngrids)
    samples = np.zeros(cells.shape, dtype=np.int64)
    _check(lib().cbet_mesh_deposit(cells.handle, _addr(a), ngrids, stride, C.byref(p), subsamples, 0, _addr(energy),
                                   _addr(outside), _addr(samples), None))
    return energy, outside, samples


def ray_tracing(te_profile, r_profile, ne_profile, edep, params, beam_norm=None, gpus=None, ngpu=1):
    """rayTracing() (main.cu:96-232): host profiles in, host `edep` (numpy, (nx+2,ny+2,nz+2))
    ADDED into.  Returns (timers{init,tracing,combining,total}, Counters)."""
    te = np.ascontiguousarray(te_profile, dtype=np.float64)
    r = np.ascontiguousarray(r_profile, dtype=np.float64)
    ne = np.ascontiguousarray(ne_profile, dtype=np.float64)
    if not (isinstance(edep, np.ndarray) and edep.dtype == np.float64 and edep.flags.c_contiguous):
        raise TypeError("edep must be a C-contiguous float64 numpy array")
    bn = None
    if beam_norm is not None:
        bn = np.ascontiguousarray(beam_norm, dtype=np.float64)
    garr = None
    if gpus is not None:
        garr = (C.c_int * len(gpus))(*gpus)
        ngpu = len(gpus)
    timers = np.zeros(4)
    cnt = Counters()
    _check(lib().cbet_ray_tracing(_dptr(te), _dptr(r), _dptr(ne), _dptr(edep), C.byref(params),
                                  _dptr(bn) if bn is not None else None, garr, ngpu, _dptr(timers),
                                  C.byref(cnt)))
    return dict(zip(("init", "tracing", "combining", "total"), timers.tolist())), cnt


# ---- output stage ------------------------------------------------------------------------------
def write_text(edep, path):
    """main.cu:6-22 `-D PRINT` rendering (truth_100's format) of a host (d0,d1,d2) array."""
    e = np.ascontiguousarray(edep, dtype=np.float64)
    n = lib().cbet_write_text(_dptr(e), e.shape[0], e.shape[1], e.shape[2],
                              os.fsencode(path) if path is not None else None)
    if n < 0:
        _check(int(n))
    return int(n)


def edep_average(edep):
    """main.cu:334-349: 27-point average of the haloed grid -> (nx, ny, nz)."""
    e = np.ascontiguousarray(edep, dtype=np.float64)
    nx, ny, nz = (d - 2 for d in e.shape)
    out = np.zeros((nx, ny, nz))
    _check(lib().cbet_edep_average(_dptr(e), _dptr(out), nx, ny, nz))
    return out


def node_coordinates(params):
    """main.cu:321-332: (x, y, z), each [nx][ny][nz]."""
    shape = (params.nx, params.ny, params.nz)
    x, y, z = np.empty(shape), np.empty(shape), np.empty(shape)
    _check(lib().cbet_node_coordinates(C.byref(params), _dptr(x), _dptr(y), _dptr(z)))
    return x, y, z


def write_npy(array, path):
    """The library's .npy writer (stand-in for the reference's dead HDF5 output); returns bytes written."""
    a = np.ascontiguousarray(array, dtype=np.float64)
    shape = (C.c_long * a.ndim)(*a.shape)
    n = lib().cbet_write_npy(_dptr(a), a.ndim, shape, os.fsencode(path))
    if n < 0:
        _check(int(n))
    return int(n)


def edep_average_device(edep, out, nx, ny, nz, stream=None):
    """main.cu:334-349 on the device: edep (n+2)^3 and out n^3 are device tensors / addresses."""
    _check(lib().cbet_edep_average_device(_addr(edep), _addr(out), nx, ny, nz, _addr(stream)))


def debug_bounds_violations(reset=True, stream=None):
    """Bounds-audit builds only: out-of-range accesses the kernels attempted since the last reset."""
    n = C.c_ulonglong()
    _check(lib().cbet_debug_bounds_violations(C.byref(n), 1 if reset else 0, _addr(stream)))
    return int(n.value)
