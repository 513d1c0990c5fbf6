"""RayTracer: torch-held device buffers around the C-ABI launch, and the multi-GPU step.

torch is plumbing here -- device memory, streams and torch.distributed (backend "nccl" = RCCL over
xGMI).  All computation happens in libcbet_mi355x.so through cbet_raytracing_3d_amd.api.

The multi-GPU scheme replaces main.cu:166-210 of the reference: instead of blocks of nbeams/nGPUs
whole beams per device (60/8 truncates to 7 and drops four beams) and a host-side sum of whole grids,
rank r traces the CONTIGUOUS part [T r / W, T (r+1) / W) of the beam-major list of T ray bundles into
its private (nx+2)(ny+2)(nz+2) grid, and the grids are combined by one reduce-scatter into x-slabs
(rank r ends up owning slab r of the sum: pipeline.SweepPipeline, reduce_scatter_grid); allreduce_grid
is kept for callers that need the whole sum on every rank.

This module is also the package's facade: the plain path's combine and pipeline live in pipeline.py, the
CBET fixed-point loops in cbet_loop.py and their slab exchange in exchange.py, and every name of theirs
that callers use is importable from here.
"""
import numpy as np
import torch

from . import api
from .cbet_loop import (HostMixing, _check_mixing, _DeviceCbetEngine, _agree, _frozen, _parts, balanced_slabs,  # noqa: F401
                        cbet_fixed_point, cbet_fixed_point_slabs, gain_update_weights, slab_pieces)
from .exchange import SegmentPlan, _pack_rows_cpu, _segment_rows, _SlabExchanger  # noqa: F401
from .pipeline import SweepPipeline, allreduce_grid, reduce_scatter_grid, row_pitch  # noqa: F401


def _require(t, shape, what):
    """`t` is a contiguous float64 tensor of that shape, or ValueError."""
    if t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be a contiguous float64 tensor of shape %s" % (what, tuple(shape)))


def shifts_to_domega(params, what, dlambda_angstrom, domega, required):
    """Wavelength shifts or frequency shifts, as frequency shifts: ONE of dlambda_angstrom (shifts of the nominal wavelength
    of `params` in Angstrom, > 0 = red; converted by api.wavelength_shift_to_domega) or domega (rad/s, handed back as it is).
    Both given is a ValueError in the name of `what`, and so is a NaN or infinite wavelength shift; neither given is one if
    `required`, and None (= off) otherwise.  No device call."""
    if dlambda_angstrom is not None and domega is not None:
        raise ValueError("%s takes dlambda_angstrom or domega, not both" % what)
    if dlambda_angstrom is None:
        if domega is None and required:
            raise ValueError("%s takes ONE of dlambda_angstrom or domega" % what)
        return domega
    dl = np.asarray(dlambda_angstrom, dtype=np.float64)
    if not np.isfinite(dl).all():
        raise ValueError("%s: dlambda_angstrom holds a NaN or infinite value" % what)
    return api.wavelength_shift_to_domega(params, dl)


def _ramp(g):
    """What a "target" flow table is tabulated from: the Mach ramp and the sound speed's inputs of gain parameters."""
    return (g.mach_r0, g.mach_0, g.mach_r1, g.mach_1, g.z_ion, g.te_ev, g.ti_ev, g.mi_over_me)


class RayTracer:
    """One device's share of a ray-tracing pass.

    Mirrors the device-side state rayTracing() sets up per GPU (main.cu:133-152): the seven small
    read-only arrays uploaded once, a deposition grid, and the launch constants of main.cu:156-159.
    """

    def __init__(self, params, r_profile, ne_profile, te_profile, beam_norm=None, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("RayTracer needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None \
            else torch.device(device)
        self.gpu = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.params = params.copy()
        self.derived = api.derive(self.params)
        if beam_norm is None:
            beam_norm = api.omega60_beam_norm()[: self.params.nbeams]
        beam_norm = np.ascontiguousarray(beam_norm, dtype=np.float64).reshape(-1, 3)
        if beam_norm.shape[0] != self.params.nbeams:
            raise ValueError("beam_norm has %d rows, params.nbeams=%d" % (beam_norm.shape[0], self.params.nbeams))
        phase_r, pow_r = api.host_power_table()
        bbeam = api.host_beam_trig(beam_norm)

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)

        self.d_beam_norm, self.d_bbeam_norm = up(beam_norm), up(bbeam)
        self.d_pow_r, self.d_phase_r = up(pow_r), up(phase_r)
        self.d_r, self.d_ne, self.d_te = up(r_profile), up(ne_profile), up(te_profile)
        for t in (self.d_r, self.d_ne, self.d_te):
            if t.numel() != self.params.nprofile:
                raise ValueError("profile length != params.nprofile")
        self.ctx = api.Context(self.params, self.gpu)
        self._launch_list = None        # set_launch_list(): the regrouped list (ray_ids())
        self.target = None              # set_target(): api.Target, or None = the spherical target about the origin
        self.mesh = None                # set_plasma_mesh(): the DEVICE api.Mesh the tables come from, or None = the profiles
        self._mesh_nodes = None         # ... its host (r, theta, phi, center), and the dual cells deposit_on_mesh builds from them
        self._mesh_cells = None
        self.flow = None                # set_flow(): None, "target", "mesh" or the caller's [3, nx, ny, nz] table
        self._flow_gp = None            # the gain parameters a "target" flow is tabulated from
        self.gain_state = None          # set_gain_state(): None, "mesh" or the caller's [2, nx, ny, nz] table
        self._state_gp = None           # the gain parameters a "mesh" state takes ti_ev, z_ion and mi_over_me from
        self.saturation = 0.0           # set_saturation(): the limit of the ion-acoustic amplitude, 0.0 = none
        self._exchange_work = None      # exchange_matrix(): the per-workgroup partial tables, allocated by the first call
        self._lpi_work = None           # lpi_map(): the per-workgroup partial summaries, allocated by the first call
        self._tables_filled = False     # tabulate() or the pipeline's preparation has filled this context's node tables
        self._table_addrs = None        # table_te(): the context's (ne3d, kappa3d) addresses, asked for once
        self.grid_shape = (self.params.nx + 2, self.params.ny + 2, self.params.nz + 2)

    # ---- the one spelling of what every launch repeats -------------------------------------------------------------
    def _stream(self):
        """The raw handle of torch's current stream on this tracer's device."""
        return torch.cuda.current_stream(self.device).cuda_stream

    def _grad_consts(self):
        d = self.derived
        return d.xconst, d.yconst, d.zconst

    def _tail(self, host_trig=True):
        """The arguments every trace entry point of the C ABI takes between its output array and its params, in the
        header's order: bbeam_norm, beam_norm, pow_r, phase_r, xconst, yconst, zconst."""
        return (self.d_bbeam_norm if host_trig else None, self.d_beam_norm, self.d_pow_r, self.d_phase_r) + self._grad_consts()

    def _launch_params(self, beam_lo, beam_hi, shard_index, shard_count, **more):
        """A launch's copy of the parameters: its beams [beam_lo, beam_hi) (beam_hi None = all that follow) and its shard."""
        return self.params.copy(beam_lo=beam_lo, beam_hi=self.params.nbeams if beam_hi is None else beam_hi,
                                shard_index=shard_index, shard_count=shard_count, **more)

    def _x_hi(self, x_hi):
        """The end of a slab of planes [x_lo, x_hi): None = the grid's last plane."""
        return self.grid_shape[0] if x_hi is None else x_hi

    def _out(self, out, shape, what="out"):
        """`out` if it is a contiguous float64 tensor of `shape` (ValueError otherwise); None: a zeroed new one."""
        if out is None:
            return torch.zeros(shape, dtype=torch.float64, device=self.device)
        _require(out, shape, what)
        return out

    def _require_fields(self, fields):
        _require(fields, (4, self.params.nbeams) + self.grid_shape, "fields (new_fields(), normalised by gain_field)")

    def _require_gain(self, gain):
        _require(gain, (self.params.nbeams,) + self.grid_shape, "gain")

    def _upload_items(self, *lists):
        """The int32 item lists of api.path_items on this device."""
        return [torch.from_numpy(a).to(self.device) for a in lists]

    def _require_tabulated(self, who, gain_params=None):
        """What the gain model reads is tabulated, or ValueError in the name of `who`: a "mesh" state needs the context's
        state table and a "target" or "mesh" flow its flow table (tabulate() fills both).  gain_params: the caller's, for
        the callers that hand them to the model with a "target" flow -- they must carry the ramp the table was tabulated
        from."""
        if self._state_is_mesh() and self.ctx.state() is None:
            raise ValueError('%s: set_gain_state("mesh") needs tabulate() first' % who)
        if isinstance(self.flow, str):
            if gain_params is not None and self._flow_is("target") and _ramp(gain_params) != _ramp(self._flow_gp):
                raise ValueError("%s: the flow table was tabulated from another Mach ramp or sound speed than gain_params "
                                 "carries (set_flow(\"target\", gain_params), then tabulate())" % who)
            if self.ctx.flow() is None:
                raise ValueError('%s: set_flow("%s") needs tabulate() first' % (who, self.flow))

    def _grid_layout(self, grid):
        """api.grid_layout of a deposit tensor on this device: one grid, a padded one or a [G, ...] stack of dense ones."""
        _require(grid, grid.shape, "grid")          # (which shapes: api.grid_layout)
        if grid.device != self.device:
            raise ValueError("grid must be on %s" % self.device)
        layout = api.grid_layout(grid.shape, self.params)
        if layout[3] and layout[2].edep_zpitch:
            raise ValueError("grid: a stack holds dense grids %s, got %s" % (self.grid_shape, tuple(grid.shape)))
        return layout

    def _trace(self, out, params, ctx=None):
        """cbet_trace_nodes into `out` with `params` on torch's current stream, from the tables of `ctx` (default: this
        tracer's context)."""
        api.trace_nodes(0, self.derived.nindices, None, None, out, *self._tail(), params, self.ctx if ctx is None else ctx,
                        self._stream())

    def _prepare_plasma(self, params, ctx):
        """Node tables and step records of `ctx` from the radial profiles, one kernel (cbet_prepare_plasma), on torch's
        current stream.  With a target or a mesh set: cbet_tabulate_target / cbet_tabulate_mesh, then the records of those
        tables."""
        if self._tabulate_other(ctx, params):
            api.prepare_step_records(ctx, params, None, None, *self._grad_consts(), self._stream())
        else:
            api.prepare_plasma(ctx, params, self.d_te, self.d_r, self.d_ne, *self._grad_consts(), self._stream())
        if ctx is self.ctx:
            self._tables_filled = True
        self._tabulate_flow(ctx, params)
        self._tabulate_state(ctx, params)
        if ctx is not self.ctx:     # a prepared context carries what the tracer's own was last given, by the tracer or by a caller
            ctx.adopt_beam_options(self.ctx, self._stream())
        ctx.set_saturation(self.saturation)         # ... but the TRACER's limit, like the tracer's own

    def _tabulate_other(self, ctx, params):
        """The node tables of `ctx` from the mesh or on the target, if one is set, on torch's current stream: True.  False
        and nothing done otherwise (the caller then takes the path of the radial profiles)."""
        if self.mesh is not None:
            api.tabulate_mesh(ctx, params, self.mesh, self._stream())
        elif self.target is not None:
            api.tabulate_target(ctx, params, self.d_te, self.d_r, self.d_ne, self.target, self._stream())
        else:
            return False
        return True

    # ---- hydro-mesh plasma (include/cbet_mi355x.h cbet_tabulate_mesh) -------------------------
    def set_plasma_mesh(self, r, theta=None, phi=None, ne=None, te=None, velocity=None, center=(0.0, 0.0, 0.0), ti=None,
                        zbar=None):
        """Take the plasma from a hydrodynamics state on a spherical-polar mesh about `center` (cm) instead of the radial
        profiles: r [nr], theta [ntheta], phi [nphi] node coordinates (None: no dependence on that angle), ne (cm^-3) and
        te (the profiles' units) [nr, ntheta, nphi], velocity None or (ur, uth, uph) in cm/s (api.Mesh: numpy arrays or
        tensors).  The mesh is validated on the host by the host twins' rules (api.mesh_check) and uploaded once;
        tabulate(), launch(), trace_exits() and the pipeline's passes then fill the context's node tables with
        cbet_tabulate_mesh and trace those.  set_plasma_mesh(None) goes back to the profiles.  A mesh and a target exclude
        each other.  The CBET stage refuses a mesh while no flow is set, as it refuses a target: set_flow("mesh") gives it
        the mesh's own velocity.  ti (eV), zbar: the ion temperature and the mean charge on the mesh's nodes, each None or
        of the fields' shape, for set_gain_state("mesh"), which gives the gain kernels the local sound speed and gain
        constant; te must then be in eV (as the s83177 profile is) for that state to mean anything."""
        if r is None:
            self._drop_mesh_cells()
            self.mesh = None
            if self._flow_is("mesh"):
                self.set_flow(None)
            if self._state_is_mesh():
                self.set_gain_state(None)
            return
        if self.target is not None:
            raise ValueError("set_plasma_mesh: a target is set (set_target(None) first): a mesh and a target exclude each other")
        if ne is None or te is None:
            raise ValueError("set_plasma_mesh: ne and te are required")
        host = api.Mesh(r, theta, phi, ne, te, velocity, center, ti=ti, zbar=zbar)
        try:
            api.mesh_check(host)
            if ti is not None or zbar is not None:      # the host twin's checks of the two arrays, on a grid of a few nodes
                api.mesh_state_table(api.default_params(8, nbeams=1), api.default_gain_params(), host)
        except api.CbetError as e:
            raise ValueError(str(e)) from None
        if self._flow_is("mesh") and not host.has_velocity:
            raise ValueError('set_plasma_mesh: set_flow("mesh") is in force and this mesh has no velocity')
        self._drop_mesh_cells()
        self.mesh = host.to(self.device)
        self._mesh_nodes = tuple(a.copy() for a in host._keep[:3]) + (tuple(host.center),)

    def _drop_mesh_cells(self):
        if self._mesh_cells is not None:
            self._mesh_cells.close()
        self._mesh_nodes = self._mesh_cells = None

    # ---- perturbed targets (include/cbet_mi355x.h cbet_tabulate_target) ------------------------
    def set_target(self, offset=(0.0, 0.0, 0.0), coeffs=None, lmax=None):
        """Trace a target whose centre sits at `offset` (cm) and whose iso-surfaces are displaced by sum_c coeffs[c] Y_c
        (modes.target_coeffs) instead of the spherical one about the origin: tabulate(), launch(), trace_exits() and the
        pipeline's passes then fill the context's node tables with cbet_tabulate_target and trace those.  set_target(None)
        goes back to the spherical target and to the calls made without one.  The CBET stage -- launch_cbet, gain_field,
        cbet_solve -- refuses a target while no flow is set: its closed-form flow is centred on the origin.  With
        set_flow("target"), or a flow table of the caller's, it runs on the target's tables and that flow."""
        if offset is not None and self.mesh is not None:
            raise ValueError("set_target: a plasma mesh is set (set_plasma_mesh(None) first): a mesh and a target exclude each other")
        self.target = None if offset is None else api.Target(offset, coeffs, lmax)

    # ---- flow of the CBET stage (include/cbet_mi355x.h cbet_tabulate_flow) --------------------
    def set_flow(self, mode=None, gain_params=None):
        """Where the gain kernels take the plasma flow from.
        None (the default): the closed-form radial ramp about the origin; the CBET stage then refuses a target.
        "target": the ramp's flow on the current target (cbet_tabulate_flow; the sphere about the origin if no target is
        set), tabulated whenever the node tables are -- tabulate(), the pipeline's preparation, cbet_solve's start -- from
        the ramp of `gain_params` (default api.default_gain_params(); cbet_solve puts its own in their place).
        "mesh": the velocity of the current plasma mesh (set_plasma_mesh; cbet_tabulate_mesh_flow), tabulated at the same
        moments; an error without a mesh or if the mesh has no velocity.
        A float64 tensor [3, nx, ny, nz] on this device: the caller's own flow field (ux, uy, uz at the nodes, cm/s), kept
        referenced here and read as it is at every gain update.
        With a flow set launch_cbet, gain_field and cbet_solve (slabs=True too) run on a target."""
        if mode is None:
            self.flow, self._flow_gp = None, None
            self.ctx.set_flow(None)
            return
        if isinstance(mode, str):
            if mode == "mesh":
                if self.mesh is None or not self.mesh.has_velocity:
                    raise ValueError('set_flow("mesh"): no plasma mesh is set, or it has no velocity (set_plasma_mesh)')
                self.ctx.set_flow(None)                 # until the next tabulate() fills and selects the context's table
                self.flow, self._flow_gp = "mesh", None
                return
            if mode != "target":
                raise ValueError('set_flow: None, "target", "mesh" or a [3, nx, ny, nz] tensor, got %r' % (mode,))
            self.ctx.set_flow(None)                     # until the next tabulate() fills and selects the context's table
            self.flow = "target"
            self._flow_gp = self._copy_gp(api.default_gain_params() if gain_params is None else gain_params)
            return
        _require(mode, (3, self.params.nx, self.params.ny, self.params.nz), "flow")
        if mode.device != self.device:
            raise ValueError("flow must be on %s" % self.device)
        self.flow, self._flow_gp = mode, None
        self.ctx.set_flow(mode)

    def _flow_is(self, mode):
        return isinstance(self.flow, str) and self.flow == mode

    @staticmethod
    def _copy_gp(gain_params):
        return type(gain_params).from_buffer_copy(gain_params)

    def _tabulate_flow(self, ctx=None, params=None):
        """A "target" or "mesh" flow into `ctx` (default: this tracer's context) on torch's current stream; nothing otherwise."""
        ctx, params = self.ctx if ctx is None else ctx, self.params if params is None else params
        if self._flow_is("mesh"):
            api.tabulate_mesh_flow(ctx, params, self.mesh, self._stream())
        elif isinstance(self.flow, str):
            api.tabulate_flow(ctx, params, self._flow_gp, self.target, self._stream())

    # ---- local plasma state of the CBET stage (include/cbet_mi355x.h cbet_tabulate_mesh_state) --
    def set_gain_state(self, mode=None, gain_params=None):
        """Where the gain kernels take the sound speed and the gain constant from.
        None (the default): the scalars of the gain parameters (te_ev, ti_ev, z_ion: one state for the whole plasma).
        "mesh": the local state of the current plasma mesh (set_plasma_mesh: its te in eV, its ti and zbar where it has
        them; cbet_tabulate_mesh_state), tabulated whenever the node tables are -- tabulate(), the pipeline's preparation,
        cbet_solve's start; ti_ev and z_ion for the arrays the mesh lacks, and mi_over_me, come from `gain_params` (default
        api.default_gain_params(); cbet_solve puts its own in their place).  An error without a mesh.
        A float64 tensor [2, nx, ny, nz] on this device: the caller's own table (cs in cm/s, gain_const), kept referenced
        here and read as it is at every gain update.
        The flow is a separate choice (set_flow): the closed-form ramp and a "target" flow keep the scalar sound speed."""
        if mode is None:
            self.gain_state, self._state_gp = None, None
            self.ctx.set_state(None)
            return
        if isinstance(mode, str):
            if mode != "mesh":
                raise ValueError('set_gain_state: None, "mesh" or a [2, nx, ny, nz] tensor, got %r' % (mode,))
            if self.mesh is None:
                raise ValueError('set_gain_state("mesh"): no plasma mesh is set (set_plasma_mesh)')
            self.ctx.set_state(None)                    # until the next tabulate() fills and selects the context's table
            self.gain_state = "mesh"
            self._state_gp = self._copy_gp(api.default_gain_params() if gain_params is None else gain_params)
            return
        _require(mode, (2, self.params.nx, self.params.ny, self.params.nz), "gain state")
        if mode.device != self.device:
            raise ValueError("gain state must be on %s" % self.device)
        self.gain_state, self._state_gp = mode, None
        self.ctx.set_state(mode)

    def _state_is_mesh(self):
        return isinstance(self.gain_state, str)

    def _tabulate_state(self, ctx=None, params=None):
        """A "mesh" state into `ctx` (default: this tracer's context) on torch's current stream; nothing otherwise."""
        if self._state_is_mesh():
            api.tabulate_mesh_state(self.ctx if ctx is None else ctx, self.params if params is None else params,
                                    self._state_gp, self.mesh, self._stream())

    # ---- saturation of the ion-acoustic wave (include/cbet_mi355x.h cbet_context_set_saturation) --
    def set_saturation(self, dn_max=0.0):
        """The limit of the ion-acoustic amplitude in the gain kernels.
        0.0 (the default): none -- every pair gain is the linear one.
        dn_max > 0: the gain of every beam pair is scaled down where the amplitude it corresponds to, |G_ij| sqrt(Ii Ij) / kap
        with kap = (k0 / 2) (ne / ncrit) / sqrt(1 - ne / ncrit), exceeds dn_max; the same factor for both beams of the pair, so
        a cell's exchange still cancels.  pair_amplitude() maps that amplitude, to choose a value by.
        The limit is the context's: gain_field, both loops of cbet_solve and api.cbet_solve(ctx=tracer.ctx) honour it from
        the next gain update on, and so does every context prepared for this tracer later (the pipeline's).  A negative, NaN
        or infinite value raises and changes nothing."""
        self.ctx.set_saturation(dn_max)
        self.saturation = float(dn_max)

    # ---- wavelength detuning (include/cbet_mi355x.h cbet_context_set_detuning) --------------------
    def set_detuning(self, dlambda_angstrom=None, domega=None):
        """Per-beam colours in the gain kernels: ONE of dlambda_angstrom (wavelength shifts of the nominal wavelength in
        Angstrom, > 0 = red; api.wavelength_shift_to_domega) or domega (angular-frequency shifts in rad/s), one value per
        beam.  Neither given: off, the default.  The ion-acoustic resonance of the ordered pair (i, j) gains the beat frequency
        w_j - w_i: in still plasma the red-shifted beam gains.  Only differences enter, so equal shifts are the same as none.
        The shifts are the context's: gain_field, pair_amplitude, exchange_matrix, both loops of cbet_solve and
        api.cbet_solve(ctx=tracer.ctx) honour them from the next launch on, and so does every context prepared for this
        tracer later (the pipeline's).  A set-up call: it waits for torch's current stream.  A NaN or infinite shift or a
        wrong count raises and changes nothing."""
        self.ctx.set_detuning(shifts_to_domega(self.params, "set_detuning", dlambda_angstrom, domega, False), self._stream())

    def detuning(self):
        """The frequency shifts in use (rad/s, one per beam; the context's own record), or None if none."""
        return self.ctx.detuning()

    # ---- laser bandwidth (include/cbet_mi355x.h cbet_context_set_bandwidth) -----------------------
    def set_bandwidth(self, domega=None, weights=None, dlambda_angstrom=None):
        """A line spectrum in the gain kernels, the SAME for every beam about its own centre frequency (its colour of
        set_detuning): ONE of domega (line offsets in rad/s) or dlambda_angstrom (wavelength offsets of the nominal wavelength
        in Angstrom, > 0 = red; api.wavelength_shift_to_domega), with `weights` > 0 (None: equal; normalised to sum 1 by the
        library), at most api.MAX_BAND_LINES lines -- api.line_spectrum makes equally spaced ones.  No argument, one line or
        equal offsets select no spectrum, the default.  The lines are incoherent: every line pair of two beams drives its own
        grating, and the pair gain is the weighted sum of their resonances; bandwidth alone transfers nothing, it smears a
        resonance that flow or detuning creates.  The spectrum is the context's, like the shifts: gain_field, pair_amplitude,
        exchange_matrix, both loops of cbet_solve and the contexts this tracer prepares later honour it; the tracer keeps no
        copy.  A set-up call: it waits for torch's current stream.  A NaN or infinite offset or a weight that is not finite and
        > 0 raises and changes nothing."""
        domega = shifts_to_domega(self.params, "set_bandwidth", dlambda_angstrom, domega, False)
        self.ctx.set_bandwidth(domega, weights, self._stream())

    def bandwidth(self):
        """The line spectrum in use ((offsets in rad/s, normalised weights); the context's own record), or None if none."""
        return self.ctx.bandwidth()

    # ---- polarization smoothing (include/cbet_mi355x.h cbet_context_set_polarization) -------------
    def set_polarization(self, mode="aligned"):
        """How the beams are polarized in the gain kernels.
        "aligned" (the default): every pair of beams is polarized alike -- the pair gain is pref P(eta).
        "smoothed": every beam is an equal, incoherent mix of two orthogonal polarizations (a distributed polarization
        rotator on every beam, OMEGA's); the gain of every pair is scaled by (1 + cos^2 theta) / 4, theta the angle between
        the two beams in the cell -- between 1/4 and 1/2 -- BEFORE the saturation clamp, so pair_amplitude() maps the
        amplitude of the pair's total exchange.
        The mode is the context's: gain_field, pair_amplitude, exchange_matrix, both loops of cbet_solve and
        api.cbet_solve(ctx=tracer.ctx) honour it from the next launch on, and so does every context prepared for this tracer
        later (the pipeline's).  An unknown mode raises and changes nothing."""
        self.ctx.set_polarization(mode)

    def polarization(self):
        """The polarization mode in use ("aligned" or "smoothed"; the context's own record)."""
        return self.ctx.polarization()

    def pair_amplitude(self, fields, gain_params, x_lo=0, x_hi=None, ne3d=None, out=None):
        """The largest ion-acoustic amplitude any beam pair's UNCLAMPED gain corresponds to, per cell of the planes
        [x_lo, x_hi): a grid-shaped tensor (`out`, or a zeroed new one; cells of other planes are left as they are).
        `fields` are normalised fields [4, nbeams, ...] as gain_field leaves them; they are not changed.  The flow and the
        gain state are read as gain_field reads them; the limit of set_saturation is not."""
        self._require_fields(fields)
        self._require_tabulated("pair_amplitude")
        out = self._out(out, self.grid_shape)
        api.pair_amplitude(fields, ne3d, out, x_lo, self._x_hi(x_hi), self.params, gain_params, self.ctx, self._stream())
        return out

    def exchange_matrix(self, fields, gain_params, x_lo=0, x_hi=None, ne3d=None, out=None, gross=False):
        """Which beam feeds which: the [nbeams, nbeams] tensor T with T[i, j] = the energy beam i gains from beam j per field
        pass over the planes [x_lo, x_hi) (beam_gain's units; T[j, i] = -T[i, j]), ADDED into `out` if given (its upper
        triangle; slabs and ranks sum) or into a zeroed new one.  gross=True: (T, Gross) with Gross[i, j] the sum of the
        magnitudes of the cells' exchanges, symmetric; gross may also be a tensor to add into.
        `fields` are normalised fields [4, nbeams, ...] as gain_field leaves them; they are not changed.  The flow and the
        gain state are read as gain_field reads them, and the limit of set_saturation is honoured."""
        nb = self.params.nbeams
        self._require_fields(fields)
        self._require_tabulated("exchange_matrix")
        out = self._out(out, (nb, nb))
        if gross is False or gross is None:                # True: a zeroed new one; a tensor: that one
            gross = None
        else:
            gross = self._out(None if gross is True else gross, (nb, nb), "gross")
        if self._exchange_work is None:      # one double at the least: a single beam needs none, the entry wants a pointer
            self._exchange_work = torch.empty(max(api.exchange_matrix_work_bytes(self.params) // 8, 1), dtype=torch.float64,
                                              device=self.device)
        api.exchange_matrix(fields, ne3d, out, gross, self._exchange_work, x_lo, self._x_hi(x_hi), self.params, gain_params,
                            self.ctx, self._stream())
        return out if gross is None else (out, gross)

    # ---- quarter-critical LPI maps (include/cbet_mi355x.h cbet_lpi_map) -----------------------
    def table_te(self):
        """The electron temperature (eV) at the nodes, [nx, ny, nz] on this device, recovered from the context's own node
        tables by inverting the absorption coefficient's formula (csrc/cbet_node_model.h kappa()):
            Te = (5.2e-4 * 1e6 * ne^2 * e^2 / me * dt / (ncrit * kappa))^(2/3)
        whatever the tables were filled from (profiles, a target, a plasma mesh); 0 where ne or kappa is 0.  Needs
        tabulate() first.  A set-up step: it waits for torch's current stream and copies the two tables."""
        if not self._tables_filled:
            raise ValueError("table_te: the context's node tables are not filled: tabulate() first")
        if self._table_addrs is None:        # once: asking for the (writable) pointers makes the next launch rebuild its records
            self._table_addrs = self.ctx.tables()
        shape = (self.params.nx, self.params.ny, self.params.nz)
        torch.cuda.current_stream(self.device).synchronize()
        ne, kap = (torch.empty(shape, dtype=torch.float64, device=self.device) for _ in range(2))
        for t, addr in zip((ne, kap), self._table_addrs):
            api.moveToAndFromGPU(t, addr, 8 * t.numel(), self.gpu)
        d = self.derived
        live = (ne > 0) & (kap > 0)
        x = (5.2e-4 * 1e6) * ne * ne * (api.EC * api.EC / api.ME) * d.dt / (d.ncrit * torch.where(live, kap, torch.ones_like(kap)))
        return torch.where(live, x ** (2.0 / 3.0), torch.zeros_like(x))

    def new_lpi_summary(self):
        """A device cbet_lpi_summary as cbet_lpi_summary_init leaves it (a uint8 tensor of api.LPI_SUMMARY_BYTES bytes), for
        lpi_map(summary=...) calls that merge into one; api.lpi_summary_from() reads it."""
        return torch.frombuffer(bytearray(bytes(api.lpi_summary_new())), dtype=torch.uint8).to(self.device)

    def lpi_map(self, fields, te="tables", band=(0.20, 0.25), cone_bins=8, x_lo=0, x_hi=None, ne3d=None, out=None,
                summary=None):
        """The laser-plasma-instability maps of the cells whose ne / ncrit lies in `band` (both ends included), over the
        planes [x_lo, x_hi): (stack, summary).  stack [api.LPI_NQ, *grid_shape] (`out`, or a zeroed new one; cells of other
        planes are left as they are): api.LPI_BAND 1 in band / 0 out of it, LPI_I_SUM the overlapped intensity of the
        beams present (W/cm^2), LPI_I_CW the largest sum over beams on one of `cone_bins` cones about the density
        gradient (the beams that can share an electron-plasma wave), LPI_I_MAX the strongest beam, LPI_LN the density
        scale length (cm), LPI_ETA_SUM and LPI_ETA_CW the two-plasmon-decay threshold parameter I_14 L_um lambda_um /
        (81.86 T_keV) of the two intensities; every quantity is 0 out of band.  Unpinned: no reference counterpart.
        `fields` are normalised fields [4, nbeams, ...] as gain_field leaves them (the ones handed to
        cbet_solve(fields=...), for example); they are not changed.
        te: a float (eV, uniform), a device tensor [nx, ny, nz] in eV, or "tables" (the default): table_te(), which needs
        tabulate() first and is a set-up step (a float or a tensor keeps the call free of synchronisation).
        summary: None -- the counts, maxima and sums over the band cells come back as a dict (read from the device: the
        call then waits for the stream); a tensor of new_lpi_summary() -- the call MERGES into it (slab calls and ranks
        compose) and returns it, without waiting; False -- no summary, None comes back.
        Runs on torch's current stream; ne3d: a caller's node table instead of the context's."""
        self._require_fields(fields)
        nodes = (self.params.nx, self.params.ny, self.params.nz)
        if ne3d is not None:
            _require(ne3d, nodes, "ne3d")
        te3d, te_ev = None, 0.0
        if isinstance(te, str):
            if te != "tables":
                raise ValueError('lpi_map: te is a float (eV), a [nx, ny, nz] tensor or "tables", got %r' % (te,))
            if not self._tables_filled:
                raise ValueError('lpi_map: te="tables" needs tabulate() first')
            te3d = self.table_te()
        elif torch.is_tensor(te):
            _require(te, nodes, "te")
            if te.device != self.device:
                raise ValueError("te must be on %s" % self.device)
            te3d = te
        else:
            te_ev = float(te)
        out = self._out(out, (api.LPI_NQ,) + self.grid_shape)
        read_back = summary is None
        if summary is False:
            summary = None
        elif summary is None:
            summary = self.new_lpi_summary()
        elif summary.dtype != torch.uint8 or summary.numel() != api.LPI_SUMMARY_BYTES or not summary.is_contiguous() \
                or summary.device != self.device:
            raise ValueError("summary must be a tensor of new_lpi_summary()")
        if summary is not None and self._lpi_work is None:
            self._lpi_work = torch.empty(max(api.lpi_work_bytes(self.params), 8), dtype=torch.uint8, device=self.device)
        api.lpi_map(fields, ne3d, te3d, te_ev, float(band[0]), float(band[1]), int(cone_bins), out, summary,
                    self._lpi_work if summary is not None else None, x_lo, self._x_hi(x_hi), self.params, self.ctx,
                    self._stream())
        if read_back:
            return out, api.lpi_summary_from(summary)
        return out, summary

    def _no_target(self, what):
        if self.flow is not None:
            return
        if self.target is not None or self.mesh is not None:
            raise ValueError("%s models the flow of a spherical target about the origin: clear the target or the mesh first "
                             "(set_target(None), set_plasma_mesh(None)), or set a flow (set_flow)" % what)

    def _prepare_step_records(self):
        """The step records of the context's own tables, now and on torch's current stream (cbet_prepare_step_records)."""
        api.prepare_step_records(self.ctx, self.params, None, None, *self._grad_consts(), self._stream())

    def new_grid(self, per_beam=False, zpitch=None):
        """A zeroed deposition grid; per_beam=True: one grid per beam (cbet_params.per_beam_grids).  zpitch: rows of that
        many doubles (>= nz + 2; True = the next multiple of 8: whole 64-byte lines) instead of the reference's dense
        rows -- launch() recognises such a grid by its shape (cbet_params.edep_zpitch); [..., :nz + 2] is the reference's
        view of it.  Plain path only."""
        if zpitch:
            if per_beam:
                raise ValueError("a padded row pitch applies to the plain path's single grid")
            zp = row_pitch(self.params.nz, 1) if zpitch is True else int(zpitch)
            return torch.zeros(self.grid_shape[:2] + (zp,), dtype=torch.float64, device=self.device)
        shape = ((self.params.nbeams,) + self.grid_shape) if per_beam else self.grid_shape
        return torch.zeros(shape, dtype=torch.float64, device=self.device)

    def launch(self, edep, shard_index=0, shard_count=1, beam_lo=0, beam_hi=None,
               kernel_variant=None, force_wide_index=None, use_host_trig=True, stats=None):
        """Enqueue one launch_ray_XYZ on torch's current stream, accumulating into `edep`.  stats=True: the launch also
        counts the deposit windows' diagnostics (cbet_params.window_stats; a timed launch does not)."""
        per_beam = edep.dim() == 4
        want = ((self.params.nbeams,) + self.grid_shape) if per_beam else self.grid_shape
        # a single grid whose rows are longer than nz + 2 is a padded grid (new_grid(zpitch=...))
        padded = (not per_beam) and edep.dim() == 3 and tuple(edep.shape[:2]) == want[:2] and edep.shape[2] > want[2]
        _require(edep, edep.shape if padded else want, "edep (one grid, one per beam, or one with padded rows)")
        p = self._launch_params(beam_lo, beam_hi, shard_index, shard_count, per_beam_grids=1 if per_beam else 0,
                                edep_zpitch=int(edep.shape[2]) if padded else 0)
        if kernel_variant is not None:
            p.kernel_variant = kernel_variant
        if force_wide_index is not None:
            p.force_wide_index = force_wide_index
        if stats is not None:
            p.window_stats = 1 if stats else 0
        self._tables_filled = True              # either half below fills the context's node tables first
        if self._tabulate_other(self.ctx, p):   # the halves of the launch: the target's or the mesh's tables, then a trace of them
            api.trace_nodes(0, self.derived.nindices, None, None, edep, *self._tail(use_host_trig), p, self.ctx, self._stream())
            return edep
        api.launch_ray_XYZ(0, self.derived.nindices, self.d_te, self.d_r, self.d_ne, edep, *self._tail(use_host_trig), p,
                           ctx=self.ctx, stream=self._stream())
        return edep

    def counters(self, reset=False):
        return self.ctx.counters(self._stream(), reset)

    # ---- CBET stage (parity unpinned, see include/cbet_mi355x.h) --------------
    def tabulate(self):
        """Fill the context's node tables from the radial profiles (what launch() does first); on the target or from the
        mesh, if one is set."""
        if not self._tabulate_other(self.ctx, self.params):
            api.tabulate_plasma(self.ctx, self.params, self.d_te, self.d_r, self.d_ne, self._stream())
        self._tables_filled = True
        self._tabulate_flow()
        self._tabulate_state()

    def launch_cbet(self, out, gain_params, fields=False, gain=None, beam_gain=None, shard_index=0,
                    shard_count=1, ne3d=None, kappa3d=None, beam_lo=0, beam_hi=None, grid_beam0=0, grid_beams=0):
        """One trace with the CBET hooks on torch's current stream (node tables must be filled:
        tabulate(), or pass ne3d / kappa3d).  fields=False: deposit the absorbed energy into `out`
        ((n+2)^3 grid or a grid per beam); fields=True: the fused field pass, `out` = new_fields();
        fields="energy": the energy field alone, `out` = new_fields()[0] (a grid per beam).
        grid_beams > 0: the beam-resolved arrays (`out` when it is per beam, `gain`) hold only the grids of
        beams [grid_beam0, grid_beam0 + grid_beams) (cbet_params.grid_beam0 / grid_beams)."""
        self._no_target("launch_cbet")
        ngrids = grid_beams if grid_beams > 0 else self.params.nbeams
        if fields == "energy":
            want = (ngrids,) + self.grid_shape
            per_beam = True
        elif fields:
            want = (4, ngrids) + self.grid_shape
            per_beam = True
        else:
            per_beam = out.dim() == 4
            want = ((ngrids,) + self.grid_shape) if per_beam else self.grid_shape
        _require(out, want, "out")
        if gain is not None:
            _require(gain, (ngrids,) + self.grid_shape, "gain")
        p = self._launch_params(beam_lo, beam_hi, shard_index, shard_count, per_beam_grids=1 if per_beam else 0,
                                grid_beam0=grid_beam0, grid_beams=grid_beams)
        quantity = api.DEPOSIT_FIELD_ENERGY if fields == "energy" else (api.DEPOSIT_FIELDS if fields else api.DEPOSIT_ENERGY)
        api.trace_cbet(0, self.derived.nindices, ne3d, kappa3d, gain, quantity, out, beam_gain, *self._tail(), p, gain_params,
                       self.ctx, self._stream())
        return out

    def new_fields(self):
        """Zeroed [4][nbeams][(n+2)^3] field array (energy x path length, energy x displacement x/y/z)."""
        return torch.zeros((4, self.params.nbeams) + self.grid_shape, dtype=torch.float64, device=self.device)

    def gain_field(self, fields, gain, gain_params, change=None, ne3d=None, scratch=None, x_lo=0, x_hi=None, frozen=False,
                   pair_once=None):
        """Normalise `fields` in place and relax `gain` towards the gain coefficient they imply.
        pair_once: the kernel that evaluates each beam pair once, the cell's beams staged in LDS (True), or the ordered
        kernel in the CPU checker's sum order (False).  `scratch` is the C ABI's selector for the same choice (any
        tensor = pair-once; it is not touched) and is kept for callers of the earlier signature.
        x_lo, x_hi: only the planes [x_lo, x_hi) of the deposit grid (one rank's slab).
        frozen: fields[1:4] already hold k from an earlier call; only fields[0] is read and normalised.
        With a flow set (set_flow) the update reads it; a "target" flow is the one the last tabulate() wrote, from the
        ramp of set_flow's gain parameters -- `gain_params` must carry the same ramp; a "mesh" flow is the mesh's velocity
        as the last tabulate() wrote it.  With a gain state set (set_gain_state) the update reads the sound speed and the gain
        constant from it; a "mesh" state is the one the last tabulate() wrote."""
        self._require_tabulated("gain_field", gain_params)
        if pair_once is None:
            pair_once = scratch is not None
        scratch = gain if pair_once else None
        api.gain_field_slab(fields, ne3d, gain, scratch, change, x_lo, self._x_hi(x_hi), self.params,
                            _frozen(gain_params, frozen), self.ctx, self._stream())
        return gain

    def cbet_solve(self, edep, gain_params, rank=0, world_size=1, group=None, fields=None, gain=None, slabs=False,
                   force_collectives=False, sparse=False, mixing=0, **slab_options):
        """The CBET iteration, one rank's share (cbet_fixed_point -- or, with slabs=True, cbet_fixed_point_slabs,
        the exchange sized for xGMI -- with this device as the engine): the deposition pass is ADDED into
        `edep` (not reduced here: use allreduce_grid).  Single-rank callers can use the native loop instead:
        api.cbet_solve.
        mixing = 1 .. 4: Anderson mixing of that depth on the all-reduce loop's gain (cbet_fixed_point; rep["mixing"]).  The
        device then holds 2 mixing + 3 gain stacks instead of one -- 91 GB at depth 4 for 256^3 / 60 beams, beside the
        41.2 GB workspace -- and a caller's gain= tensor receives the result with one copy at the end.  Not with slabs=True."""
        mixing = _check_mixing(mixing)
        if mixing and slabs:
            raise ValueError("mixing is the all-reduce loop's: slabs=True with mixing = %d is not supported" % mixing)
        self._no_target("cbet_solve")
        if self._flow_is("target"):
            self._flow_gp = self._copy_gp(gain_params)      # the engine's tabulate() fills the flow table from this ramp
        if self._state_is_mesh():
            self._state_gp = self._copy_gp(gain_params)     # ... and the state table with these ti_ev, z_ion and mi_over_me
        engine = _DeviceCbetEngine(self, edep, gain_params, fields, gain)
        engine.force_collectives = force_collectives
        if slabs:
            rep = cbet_fixed_point_slabs(engine, gain_params, self.params.nbeams, self.grid_shape[0], rank, world_size, group,
                                         sparse=sparse, **slab_options)      # trace_groups=, slab_layout=
            rep["workspace_bytes"] = engine.slab_bytes()
            plan = engine.exchanger.plan
            rep["exchange"] = {"chunks": engine.exchanger.chunks, "messages": engine.exchanger.messages, "bytes_sent": engine.exchanger.bytes_sent,
                               "staging_bytes": engine.exchanger.staging_bytes(),
                               "sparse": plan is not None, "two_channels": engine.exchanger.two_channels,
                               "runs_per_exchange": plan.runs_out if plan is not None else None,
                               "dense_fraction": (8.0 * plan.runs_out / max(1, plan.dense_out)) if plan is not None else 1.0}
        else:
            rep = cbet_fixed_point(engine, gain_params, rank, world_size, group, mixing=mixing)
        rep["gain"] = engine.gain     # all beams (all-reduce loop) / this rank's beams (slab loop), whole grid
        return rep

    # ---- exit pass (include/cbet_mi355x.h cbet_trace_exits) -----------------
    def ray_ids(self):
        """The context's current launch list (int32 [L]): slot li of every beam holds thread-ray id ray_ids()[li], -1 = idle."""
        return api.live_ray_list(self.params) if self._launch_list is None else self._launch_list.copy()

    def set_launch_list(self, slots):
        """Regroup the bundles (cbet_context_set_launch_list); ray_ids() follows."""
        self.ctx.set_launch_list(slots)
        self._launch_list = np.ascontiguousarray(slots, dtype=np.int32).copy()

    def new_exits(self):
        """Zeroed exit records, float64 [nbeams, L, 10] (cbet_ray_exit: x, y, z, vx, vy, vz, uray, uray0, gained, then
        steps / status in column 9 -- read them with .view(torch.int32)[..., 18:20])."""
        return torch.zeros((self.params.nbeams, self.ctx.list_length(), 10), dtype=torch.float64, device=self.device)

    def _check_exits(self, exits):
        _require(exits, (self.params.nbeams, self.ctx.list_length(), 10), "exits (new_exits())")

    def _gain_args(self, gain, gain_params):
        """The gain_params a no-deposit pass (trace_exits, trace_paths) hands on: with a gain grid, its shape checked and
        api.default_gain_params() in place of None."""
        if gain is not None:
            self._require_gain(gain)
            if gain_params is None:
                gain_params = api.default_gain_params()
        return gain_params

    def trace_exits(self, exits, gain=None, gain_params=None, shard_index=0, shard_count=1, beam_lo=0, beam_hi=None,
                    tabulate=True):
        """The exit pass on torch's current stream: every traced ray's final state into `exits` (new_exits()); slots of
        rays this launch does not trace are left as they are.  gain: [nbeams][(n+2)^3] gain coefficient (e.g. a CBET
        solve's) -- the rays then gain energy as in the CBET deposition pass; gain_params defaults to
        api.default_gain_params().  tabulate: fill the node tables from the profiles first, as launch() does."""
        self._check_exits(exits)
        gain_params = self._gain_args(gain, gain_params)
        if tabulate:
            self.tabulate()
        p = self._launch_params(beam_lo, beam_hi, shard_index, shard_count)
        api.trace_exits(None, None, gain, exits, *self._tail(), p, gain_params, self.ctx, self._stream())
        return exits

    def energy_balance(self, exits):
        """Per-beam energy balance of exit records: float64 [nbeams, 8], columns api.TALLY_COLUMNS (launched, gained,
        absorbed, escaped, stranded, unfinished, n_rays, n_escaped); launched + gained = absorbed + escaped + stranded +
        unfinished per beam.  Deterministic."""
        self._check_exits(exits)
        tally = torch.empty((self.params.nbeams, 8), dtype=torch.float64, device=self.device)
        api.exit_tally(exits, exits.shape[1], self.params.nbeams, tally, self._stream())
        return tally

    def farfield(self, exits, ntheta, nphi, beams=None):
        """The escaped light's far field: float64 [ntheta, nphi] of remaining energy by exit direction (equal solid angle
        per polar bin, include/cbet_mi355x.h cbet_farfield), from all beams or the beams listed."""
        self._check_exits(exits)
        hist = torch.zeros((ntheta, nphi), dtype=torch.float64, device=self.device)
        stream, L = self._stream(), exits.shape[1]
        for b in (range(self.params.nbeams) if beams is None else beams):
            api.farfield(exits[b], L, ntheta, nphi, hist, stream)
        return hist

    # ---- ray path recorder (include/cbet_mi355x.h cbet_trace_paths) ---------------------------
    def ray_items(self, beams=None, bundles=False):
        """(beams, raynums), int32 numpy arrays: every live ray (ray_ids() >= 0) of the beams listed (default: all),
        beam by beam -- the item list of trace_paths for a whole fan.  bundles=True keeps the launch list's idle entries
        (raynum -1, an idle item with a zero turn record), so that every 64 items are one ray bundle of the deposit pass
        -- neighbouring rays that end together -- and a wavefront of the recorder is a wavefront of the exit pass."""
        ids = self.ray_ids()
        live = np.ascontiguousarray(ids if bundles else ids[ids >= 0], dtype=np.int32)
        which = np.arange(self.params.nbeams) if beams is None else np.asarray(list(beams), dtype=np.int64).reshape(-1)
        if which.size and (which.min() < 0 or which.max() >= self.params.nbeams):
            raise ValueError("beams outside [0, %d)" % self.params.nbeams)
        return np.repeat(which.astype(np.int32), live.size), np.tile(live, which.size)

    def new_paths(self, nitems, capacity):
        """Zeroed records for trace_paths: samples float64 [capacity, nitems, 8] (cbet_path_sample: x, y, z, uray, absorbed,
        gained, then ci, cj / ck, step as int32 pairs in columns 6, 7) and turns float64 [nitems, 8] (cbet_ray_turn: r2, x,
        y, z, uray, ne, then step, steps / status, nsamples).  Downloaded, .view(api.PATH_DTYPE)[..., 0] and
        .view(api.TURN_DTYPE)[..., 0] name the fields."""
        f64 = dict(dtype=torch.float64, device=self.device)
        return torch.zeros((capacity, nitems, 8), **f64), torch.zeros((nitems, 8), **f64)

    def trace_paths(self, beams, raynums, stride=1, capacity=None, center=(0.0, 0.0, 0.0), gain=None, gain_params=None,
                    tabulate=True, out=None):
        """The path recorder on torch's current stream: the rays (beams[k], raynums[k]) -- raynums as in ray_ids() --
        traced as the exit pass traces them, a sample every `stride` steps and one closest-approach record (to `center`,
        cm) per ray.  Ids that name no live ray are idle items: an all-zero turn record, no samples.  capacity: samples
        kept per ray; the default 1 + ceil(nt / stride) never truncates, 0 means turn records only.  gain, gain_params,
        tabulate: as trace_exits takes them.  out: (samples, turns) from new_paths to write into (samples may be None with
        capacity 0); slots the call does not write keep what they hold.  Returns (samples, turns); samples is
        sample-major, samples.permute(1, 0, 2) is the ray-major view, and turns' `ne` over derived.ncrit is the density
        at the closest approach in critical densities."""
        beams, raynums = api.path_items(beams, raynums)
        nitems = int(beams.size)
        if stride < 1:
            raise ValueError("stride must be >= 1")
        if capacity is None:
            capacity = 1 + -(-self.derived.nt // stride)
        if capacity < 0:
            raise ValueError("capacity must be >= 0")
        samples, turns = self.new_paths(nitems, capacity) if out is None else out
        _require(turns, (nitems, 8), "turns (new_paths())")
        if samples is not None or capacity > 0:
            _require(samples, (capacity, nitems, 8), "samples (new_paths())")
        gain_params = self._gain_args(gain, gain_params)
        if nitems == 0:                # (empty tensors have no address to hand over)
            return samples, turns
        if tabulate:
            self.tabulate()
        d_beams, d_raynums = self._upload_items(beams, raynums)
        api.trace_paths(None, None, gain, d_beams, d_raynums, nitems, stride, capacity, center,
                        samples if capacity > 0 else None, turns, *self._tail(), self.params, gain_params, self.ctx,
                        self._stream())
        return samples, turns

    # ---- backscatter SBS gain spectra (include/cbet_mi355x.h cbet_trace_backscatter) ----------
    def backscatter_gain(self, fields, gain_params, dlambda_angstrom=None, domega=None, beams=None, raynums=None, gain=None,
                         ne3d=None, out=None):
        """Stimulated Brillouin BACKSCATTER as a linear gain post-processor, on torch's current stream: for every ray of the
        list and every frequency shift of the scattered light the convective gain exponent Gamma = sum over the ray's steps
        of g(shift; ne, cs, u, k) I ds, with g the gain stage's own detuned pair gain for the pair (backscattered seed, the
        ray's light), q = 2 k_ray.  Unpinned: no reference counterpart.
        fields: normalised fields [4, nbeams, ...] as gain_field leaves them (only the intensities are read; not changed).
        gain_params: the damping, Mach ramp and plasma state of the gain stage.  The scan is ONE of dlambda_angstrom
        (wavelength shifts of the scattered light in Angstrom, > 0 = red; set_detuning's conversion) or domega (rad/s,
        negative = red), 1 .. api.SBS_MAX_SHIFTS values.  beams, raynums: the rays, as trace_paths takes them (default:
        ray_items(), every live ray of every beam); ids that name no live ray are idle items, all zeros.  gain: a gain grid
        [nbeams, ...] -- the rays' energies (uray_end) then include CBET, the spectrum does not depend on it.  ne3d: a
        caller's node table instead of the context's, for the trace and the model.
        The flow (set_flow), the gain state (set_gain_state) and the polarization mode (set_polarization, "smoothed" halves
        the gain) are read as gain_field reads them -- a "mesh" or "target" flow or state needs tabulate() first; the limit of
        set_saturation, the colours of set_detuning and the spectrum of set_bandwidth are NOT applied (a linear gain, the
        seed's shift is the scan variable).  Not modelled: pump depletion, shared-wave SBS, sidescatter, absorption of the
        scattered light.  The node tables must be filled (tabulate()).
        Returns {"gamma": float64 [nshift, nitems] (shift-major), "rays": float64 [nitems, 4] (cbet_ray_sbs: gmax, uray0,
        uray_end, then steps / imax / status -- .cpu().numpy().view(api.SBS_DTYPE)[..., 0] names them), "shifts": domega as a
        numpy array, "beams": the items' beams on the device}; out: (gamma, rays) tensors to write into."""
        self._require_fields(fields)
        if gain_params is None:
            raise ValueError("backscatter_gain needs gain_params (the model's damping, Mach ramp and plasma state)")
        shifts = api.sbs_shifts(shifts_to_domega(self.params, "backscatter_gain", dlambda_angstrom, domega, True))
        if not self._tables_filled:
            raise ValueError("backscatter_gain: the context's node tables are not filled: tabulate() first")
        self._require_tabulated("backscatter_gain", gain_params)
        if (beams is None) != (raynums is None):
            raise ValueError("backscatter_gain takes beams and raynums together, or neither (ray_items())")
        if beams is None:
            beams, raynums = self.ray_items()
        beams, raynums = api.path_items(beams, raynums)
        nitems, nshift = int(beams.size), int(shifts.size)
        if gain is not None:
            self._require_gain(gain)
        if ne3d is not None:
            _require(ne3d, (self.params.nx, self.params.ny, self.params.nz), "ne3d")
        gamma, rays = (self._out(None, (nshift, nitems)), self._out(None, (nitems, 4))) if out is None else out
        _require(gamma, (nshift, nitems), "gamma")
        _require(rays, (nitems, 4), "rays")
        d_beams, d_raynums = self._upload_items(beams, raynums)
        result = {"gamma": gamma, "rays": rays, "shifts": shifts, "beams": d_beams}
        if nitems == 0:                # (empty tensors have no address to hand over)
            return result
        api.trace_backscatter(ne3d, None, gain, d_beams, d_raynums, nitems, fields, shifts, gamma, rays, *self._tail(),
                              self.params, gain_params, self.ctx, self._stream())
        return result

    def backscatter_tally(self, result, beams=None, out=None):
        """Per beam and shift over the launched rays of a backscatter_gain result: float64 [nbeams, nshift, 4], columns
        api.SBS_TALLY_COLUMNS (sum of uray0, sum of uray0 Gamma, max of Gamma, number of rays).  beams: the items' beams
        (default: the result's own).  out: a table to MERGE into -- results of parts of a list compose; default a zeroed new
        one.  Deterministic: fixed-order sums, no atomics.  lpi.backscatter_spectrum turns the table into spectra."""
        gamma, rays = result["gamma"], result["rays"]
        nshift, nitems = gamma.shape
        nb = self.params.nbeams
        d_beams = result["beams"] if beams is None else self._upload_items(api.path_items(beams, beams)[0])[0]
        if int(d_beams.numel()) != nitems:
            raise ValueError("beams holds %d items, the result %d" % (int(d_beams.numel()), nitems))
        _require(rays, (nitems, 4), "rays")
        out = self._out(out, (nb, nshift, 4))
        if nitems == 0:
            return out
        work = torch.empty(max(api.backscatter_work_bytes(nitems, nshift, nb) // 8, 1), dtype=torch.float64, device=self.device)
        api.backscatter_tally(gamma, rays, d_beams, nitems, nshift, nb, out, work, self._stream())
        return out

    # ---- mode spectra (include/cbet_mi355x.h cbet_sph_modes) ----------------------------------
    def sph_modes(self, grid, r_edges=None, lmax=16, center=(0.0, 0.0, 0.0), geometry=False):
        """Real spherical-harmonic coefficients of a deposit grid on shells, on torch's current stream.  grid: one grid
        (new_grid()), a padded one (new_grid(zpitch=...)) or a [G, ...] stack of grids (new_grid(per_beam=True)); ignored
        with geometry=True, which projects E = 1 (the lattice's own spectrum).  r_edges: shell edges (default
        modes.default_shells(params, 32)).  Returns (coeffs [S][(lmax+1)^2], shell_energy [S], shell_nodes int64 [S]),
        with a leading [G] on the first two for a stack; modes.nonuniformity turns coeffs into sigma_l, sigma_rms."""
        from . import modes
        edges = np.ascontiguousarray(modes.default_shells(self.params, 32) if r_edges is None else r_edges, dtype=np.float64)
        edep = None if geometry else grid
        ngrids, stride, p, stack = api.grid_layout(None, self.params) if geometry else self._grid_layout(grid)
        nshell, ncoef = edges.size - 1, (lmax + 1) ** 2
        f64 = dict(dtype=torch.float64, device=self.device)
        coeffs = torch.empty((ngrids, max(nshell, 0), ncoef), **f64)
        energy = torch.empty((ngrids, max(nshell, 0)), **f64)
        nodes = torch.empty(max(nshell, 0), dtype=torch.int64, device=self.device)
        api.sph_modes(edep, ngrids, stride, p, center, edges, lmax, coeffs, energy, nodes, self._stream())
        if not stack:
            coeffs, energy = coeffs[0], energy[0]
        return coeffs, energy, nodes

    # ---- deposit on the hydro mesh (include/cbet_mi355x.h cbet_mesh_deposit) -------------------
    def deposit_on_mesh(self, grid, cells=None, subsamples=2, method=0):
        """The energy of a deposit grid binned into the cells of a spherical-polar mesh, on torch's current stream.  grid:
        as sph_modes takes it -- one grid, a padded one or a [G, ...] stack.  cells: an api.MeshCells made for this
        tracer's device (gpu=tracer.gpu); None: the dual cells of the mesh given to set_plasma_mesh
        (api.MeshCells.from_nodes), built at the first call and kept -- column k is then node k's cell.  subsamples: S in
        1 .. 4, each node's energy spread over S^3 samples of its box.  method: api.MESH_DEPOSIT_AUTO, _GLOBAL or _LDS.
        Returns (cell_energy [nr, ntheta, nphi], outside scalar tensor, cell_samples int64 [nr, ntheta, nphi]), with a
        leading [G] on the first two for a stack; sum(cell_energy) + outside = sum(grid) up to rounding."""
        if cells is None:
            if self._mesh_nodes is None:
                raise ValueError("deposit_on_mesh: no cells given and no plasma mesh is set (set_plasma_mesh)")
            if self._mesh_cells is None:
                r, theta, phi, center = self._mesh_nodes
                self._mesh_cells = api.MeshCells.from_nodes(r, theta, phi, center, gpu=self.gpu)
            cells = self._mesh_cells
        ngrids, stride, p, stack = self._grid_layout(grid)
        energy = torch.empty((ngrids,) + cells.shape, dtype=torch.float64, device=self.device)
        outside = torch.empty(ngrids, dtype=torch.float64, device=self.device)
        samples = torch.empty(cells.shape, dtype=torch.int64, device=self.device)
        api.mesh_deposit(cells, grid, ngrids, stride, p, subsamples, method, energy, outside, samples, self._stream())
        if cells.column_shift:
            energy, samples = torch.roll(energy, cells.column_shift, -1), torch.roll(samples, cells.column_shift, -1)
        if not stack:
            energy, outside = energy[0], outside[0]
        return energy, outside, samples

    def node_tables(self):
        """Copies of the context's node tables (ne3d, kappa3d) as numpy arrays, for tests."""
        n = self.params.nx * self.params.ny * self.params.nz
        a, b = self.ctx.tables()
        out = []
        for addr in (a, b):
            h = np.empty(n)
            api.moveToAndFromGPU(h, addr, 8 * n, self.gpu)
            out.append(h.reshape(self.params.nx, self.params.ny, self.params.nz))
        return out

    def close(self):
        self._drop_mesh_cells()
        self.ctx.close()


def shard_of_rank(rank, world_size):
    """(shard_index, shard_count) of a rank: rank r traces the r-th contiguous 1/world_size of the bundle list."""
    if not 0 <= rank < world_size:
        raise ValueError("rank outside [0, world_size)")
    return rank, world_size


def traced_pass(tracer, edep, rank=0, world_size=1, group=None, **launch_kw):
    """One full pass over the beams on `world_size` ranks: zero, trace this rank's share, combine."""
    edep.zero_()
    si, sc = shard_of_rank(rank, world_size)
    tracer.launch(edep, shard_index=si, shard_count=sc, **launch_kw)
    return allreduce_grid(edep, group)
