"""The CBET fixed-point iteration over ranks: cbet_fixed_point all-reduces the deposited fields,
cbet_fixed_point_slabs keeps beams and x-slabs rank-owned and exchanges between them (exchange.py).  Both drive an
`engine` that supplies the per-rank compute: _DeviceCbetEngine on a RayTracer's device, an oracle engine in the CPU
tests.  RayTracer.cbet_solve is the entry point."""
import numpy as np
import torch

from . import api
from .exchange import SegmentPlan, _event_on, _global_rank, _SlabExchanger, _wait_events
from .pipeline import all_reduce_staged, allreduce_grid


class _DeviceCbetEngine:
    """The per-rank compute of the CBET iteration on a RayTracer's device (see cbet_fixed_point and
    cbet_fixed_point_slabs).  The all-reduce loop keeps every beam's arrays over the whole grid
    (cbet_cbet_workspace_bytes: 41.2 GB at 256^3 / 60 beams); the slab-owned loop allocates, in begin_slabs, only
    its own beams over the whole grid and all beams over its own x-slab (cbet_cbet_slab_workspace_bytes)."""

    trace_streams = 4     # the beam groups of a field pass rotate over this many streams (a launch's ramp and drain beside its neighbours')

    def __init__(self, tracer, edep, gain_params, fields=None, gain=None):
        self.tr, self.edep, self.gp = tracer, edep, gain_params
        self._fields, self._gain = fields, gain
        self.change = torch.zeros(2, dtype=torch.float64, device=tracer.device)
        self.beam_gain = torch.zeros(tracer.params.nbeams, dtype=torch.float64, device=tracer.device)

    # ---- all-reduce loop: whole-grid arrays of every beam
    def begin(self):
        tr = self.tr
        self.fields = tr.new_fields() if self._fields is None else self._fields
        self.gain = tr.new_grid(per_beam=True) if self._gain is None else self._gain
        tr.tabulate()
        self.gain.zero_()

    def field_passes(self, use_gain, shard_index, shard_count, full=True):
        """full: all four fields; else the energy field (fields[0]) alone -- fields[1:4] keep the k of the last full pass."""
        (self.fields if full else self.fields[0]).zero_()
        self.tr.launch_cbet(self.fields if full else self.fields[0], self.gp, fields=True if full else "energy",
                            gain=self.gain if use_gain else None, shard_index=shard_index, shard_count=shard_count)
        return self.fields

    def update_gain(self, fields, frozen=False):
        self.change.zero_()
        self.tr.gain_field(fields, self.gain, self.gp, self.change, pair_once=True, frozen=frozen)
        return self.change

    def deposit(self, shard_index, shard_count):
        self.beam_gain.zero_()
        self.tr.launch_cbet(self.edep, self.gp, gain=self.gain, beam_gain=self.beam_gain,
                            shard_index=shard_index, shard_count=shard_count)
        return self.beam_gain

    # ---- Anderson mixing of the all-reduce loop's gain (cbet_fixed_point(mixing=depth))
    def mix_begin(self, depth):
        """2 depth + 3 gain stacks: depth + 1 slots for the held iterates y (the live `gain` is one of them, rotated by
        reference: no copy per pass), depth + 1 for the held residuals f, and x_keep, the iterate the update overwrites."""
        g = self.gain
        self._mix_depth = depth
        self._mix_y_free = [torch.empty_like(g) for _ in range(depth)]
        self._mix_f_free = [torch.empty_like(g) for _ in range(depth + 1)]
        self._mix_x = g.clone()
        self._mix_y, self._mix_f = [], []          # held, oldest first
        self._mix_row = torch.zeros(api.MIX_MAX_DEPTH + 1, dtype=torch.float64, device=g.device)
        self._mix_work = torch.empty(max(1, api.mix_work_bytes(g.numel()) // 8), dtype=torch.float64, device=g.device)
        self.mix_bytes = 8 * g.numel() * (2 * depth + 3)

    def mix_residual(self):
        """`gain` holds y = the update of x_keep: f = y - x_keep into a free slot, and its dot products with the held
        residuals and itself (device tensor [held + 1])."""
        self._mix_pending = self._mix_f_free.pop()
        api.mix_residual(self.gain, self._mix_x, self._mix_pending, self._mix_f, self._mix_row, self._mix_work,
                         stream=self.tr._stream())
        return self._mix_row[:len(self._mix_f) + 1]

    def mix_apply(self, alpha):
        """Push (gain, f), keep the newest len(alpha) entries, and make `gain` (and x_keep) their combination.  With every
        y slot held the result goes into the oldest, which retires."""
        self._mix_y.append(self.gain)
        self._mix_f.append(self._mix_pending)
        while len(self._mix_y) > len(alpha):
            self._mix_y_free.append(self._mix_y.pop(0))
            self._mix_f_free.append(self._mix_f.pop(0))
        retire = len(self._mix_y) > self._mix_depth
        out = self._mix_y[0] if retire else self._mix_y_free.pop()
        api.mix_apply(self._mix_y, alpha, out, self._mix_x, stream=self.tr._stream())
        if retire:
            self._mix_y.pop(0)
            self._mix_f_free.append(self._mix_f.pop(0))
        self.gain = out

    def mix_end(self):
        """A caller's gain= tensor holds the result (one copy, unless the live slot is that tensor); the slots are dropped."""
        if self._gain is not None and self.gain is not self._gain:
            self._gain.copy_(self.gain)
            self.gain = self._gain
        for name in ("_mix_y_free", "_mix_f_free", "_mix_x", "_mix_y", "_mix_f", "_mix_row", "_mix_work", "_mix_pending"):
            self.__dict__.pop(name, None)

    # ---- slab-owned loop: own beams [b0, b1) over the whole grid, all beams over the own planes [x0, x1)
    def begin_beams(self, b0, b1):
        """This rank's beams over the whole grid (their fields are complete here without any reduction) and the two
        trace streams the beam groups of a field pass alternate on."""
        tr, dev = self.tr, self.tr.device
        self.b0, self.b1 = b0, b1
        f64 = dict(dtype=torch.float64, device=dev)
        self.own_fields = torch.zeros((4, b1 - b0) + tr.grid_shape, **f64)
        self.gain_own = torch.zeros((b1 - b0,) + tr.grid_shape, **f64)
        self.gain = self.gain_own            # what a caller gets back: this rank's beams over the whole grid
        self.s_trace = [torch.cuda.Stream(device=dev) for _ in range(self.trace_streams)]
        self._launches = 0
        tr.tabulate()
        # the step records too, HERE and on this stream: left to the first launch they are built lazily on THAT launch's
        # trace stream, and the launches of the other rotating streams -- which only wait for ev_ready and see the host-side
        # version already bumped -- would read the table while k_step_table is still writing it (a fresh context: garbage)
        tr._prepare_step_records()
        self.ev_ready = _event_on(torch.cuda.current_stream(dev))

    def begin_slab(self, pieces):
        """All beams over this rank's planes (what its gain update reads and writes): one packed array pair per PIECE
        [(lo, hi), ...] of its share of the deposit grid -- one x-slab, or two (slab_layout "paired")."""
        tr = self.tr
        nb, gs = tr.params.nbeams, tr.grid_shape
        self.pieces = [tuple(pc) for pc in pieces]
        f64 = dict(dtype=torch.float64, device=tr.device)
        self.slab_fields = [torch.zeros((4, nb, hi - lo) + gs[1:], **f64) for lo, hi in self.pieces]
        self.gain_slab = [torch.zeros((nb, hi - lo) + gs[1:], **f64) for lo, hi in self.pieces]

    def begin_slabs(self, b0, b1, x0, x1):
        self.begin_beams(b0, b1)
        self.begin_slab([(x0, x1)])

    def trace_group(self, i0, i1, use_gain, full=True, wait=()):
        """The field pass of this rank's beams [b0 + i0, b0 + i1) -- one GROUP of a pass -- on the next of the rotating
        trace streams, after the events in `wait` (the gain of these beams having arrived).  Consecutive groups overlap
        (the drain of one launch beside the head of the next), and a finished group can be sent while the next one
        traces.  Returns the event recorded behind the launch."""
        tr = self.tr
        st = self.s_trace[self._launches % len(self.s_trace)]
        self._launches += 1
        _wait_events(st, (self.ev_ready,) + tuple(wait))
        with torch.cuda.stream(st):
            out = self.own_fields if full else self.own_fields[0]
            (out[:, i0:i1] if full else out[i0:i1]).zero_()
            tr.launch_cbet(out, self.gp, fields=True if full else "energy", gain=self.gain_own if use_gain else None,
                           beam_lo=self.b0 + i0, beam_hi=self.b0 + i1, grid_beam0=self.b0, grid_beams=self.b1 - self.b0)
            done = _event_on(st)
        return done

    def presence_counts(self):
        """int32 [X][Y][Z]: how many of this rank's beams deposited energy at each node in the pass just traced (the
        footprint the gain update's work follows)."""
        cnt = torch.zeros(self.tr.grid_shape, dtype=torch.int32, device=self.tr.device)
        for b in range(self.b1 - self.b0):
            cnt += (self.own_fields[0, b] != 0).to(torch.int32)
        return cnt

    def slab_bytes(self):
        """Device bytes this rank's slab loop holds: the arrays of begin_beams / begin_slab and, for sparse exchanges, the
        staging buffers and segment lists (the dense exchange sends from and receives into the arrays themselves)."""
        arrays = 8 * sum(t.numel() for t in [self.own_fields, self.gain_own] + list(self.slab_fields) + list(self.gain_slab))
        xch = getattr(self, "exchanger", None)
        if xch is None:
            return arrays
        plan = getattr(xch, "plan", None)
        return arrays + xch.staging_bytes() + (plan.list_bytes() if plan is not None else 0)

    def support_mask(self):
        """bool [own beams][X][Y][Z]: every node this rank's beams can ever deposit into -- their rays traced in the
        reference's bookkeeping mode (absorption = 0, def.cuh:118: the energy never decays, so no ray stops before it
        leaves the grid or runs out of steps) into beam-resolved grids.  Ray paths do not depend on the gain, so this
        footprint contains the footprint of every pass of the iteration.  Uses own_fields[1:] as scratch (call it
        before the first field pass)."""
        tr, nbr = self.tr, self.b1 - self.b0
        if nbr == 0:
            return torch.zeros((0,) + tr.grid_shape, dtype=torch.bool, device=tr.device)
        p = tr.params.copy(absorption=0, per_beam_grids=1, beam_lo=self.b0, beam_hi=self.b1, grid_beam0=self.b0, grid_beams=nbr)
        tmp = self.own_fields[1]
        tmp.zero_()
        tr._trace(tmp, p)
        mask = tmp != 0
        tmp.zero_()
        tr.counters(reset=True)       # the footprint pass is set-up, not part of the iteration's ray-step count
        return mask

    def field_passes_beams(self, use_gain, full=True):
        """The whole field pass of this rank's beams as one group; the current stream waits for it."""
        if self.b1 > self.b0:
            torch.cuda.current_stream(self.tr.device).wait_event(self.trace_group(0, self.b1 - self.b0, use_gain, full))
        return self.own_fields

    def update_gain_slab(self, frozen=False, after_piece=None):
        """The gain update of all beams over this rank's pieces; a second piece runs on a side stream beside the first (two
        small launches one after the other would each pay their own ramp and drain).  after_piece(k, event): the pieces
        then run ONE AFTER THE OTHER on the current stream, `event` recorded behind piece k -- the caller sends piece k's
        gain back while piece k + 1 updates.  (All launches are enqueued before the first call-back: enqueueing a piece's
        messages takes the host longer than the piece's update takes the device.)"""
        self.change.zero_()
        cur = torch.cuda.current_stream(self.tr.device)
        gp = _frozen(self.gp, frozen)
        serial = after_piece is not None
        done = []         # serial: an event on the current stream behind EVERY piece (an empty one too); else: the side stream's
        for k, ((lo, hi), fields, gain) in enumerate(zip(self.pieces, self.slab_fields, self.gain_slab)):
            st = cur
            if hi > lo:
                if k > 0 and not serial:
                    if not hasattr(self, "s_side"):
                        self.s_side = torch.cuda.Stream(device=self.tr.device)
                    st = self.s_side
                    st.wait_event(_event_on(cur))      # (behind the zeroing of `change` and the arrival fence)
                api.gain_field_packed(fields, None, gain, gain, self.change, lo, hi, self.tr.params, gp, self.tr.ctx, st.cuda_stream)
            if serial or st is not cur:
                done.append(_event_on(st))
        if serial:
            for k, ev in enumerate(done):
                after_piece(k, ev)
        else:
            _wait_events(cur, done)
        return self.change

    def deposit_beams(self):
        self.beam_gain.zero_()
        if self.b1 > self.b0:
            self.tr.launch_cbet(self.edep, self.gp, gain=self.gain_own, beam_gain=self.beam_gain, beam_lo=self.b0,
                                beam_hi=self.b1, grid_beam0=self.b0, grid_beams=self.b1 - self.b0)
        return self.beam_gain


def _frozen(gain_params, frozen):
    """gain_params with directions_frozen set as asked (a copy when it has to change)."""
    if bool(gain_params.directions_frozen) == bool(frozen):
        return gain_params
    g = type(gain_params).from_buffer_copy(gain_params)
    g.directions_frozen = 1 if frozen else 0
    return g


def _agree(t, group, world_size):
    """Make a small per-rank tensor that steers control flow identical on all ranks (rank 0's copy): collectives
    need not return bit-identical values everywhere, and a stop decision taken from slightly different numbers
    would leave ranks waiting in different collectives."""
    import torch.distributed as dist
    if world_size > 1:
        host = t.detach().cpu()
        dist.broadcast(host, src=_global_rank(group, 0), group=group)
        return host
    return t.detach().cpu()


class HostMixing:
    """mix_begin / mix_residual / mix_apply / mix_end over the host twins (cbet_mix_residual_host, cbet_mix_apply_host), for an
    engine of cbet_fixed_point whose `gain` lives in host memory: a numpy array (replaced by the new iterate) or a CPU
    tensor (written in place).  Mix it into the engine's class; the engine's own update may write `gain` in place or
    replace it -- every held array here is a copy."""

    @staticmethod
    def _mix_flat(g):
        a = g if isinstance(g, np.ndarray) else g.detach().numpy()
        return np.ascontiguousarray(a, dtype=np.float64).reshape(-1)

    def mix_begin(self, depth):
        self._mix_depth = depth
        self._mix_x = self._mix_flat(self.gain).copy()      # x_keep: the iterate the coming update starts from
        self._mix_y, self._mix_f = [], []                   # held, oldest first
        self.mix_bytes = 8 * self._mix_x.size * (2 * depth + 3)

    def mix_residual(self):
        y = self._mix_flat(self.gain).copy()
        f = np.empty_like(y)
        row = api.mix_residual_host(y, self._mix_x, f, self._mix_f)
        self._mix_pending = (y, f)
        return torch.from_numpy(row)

    def mix_apply(self, alpha):
        y, f = self._mix_pending
        self._mix_y.append(y)
        self._mix_f.append(f)
        del self._mix_y[:len(self._mix_y) - len(alpha)], self._mix_f[:len(self._mix_f) - len(alpha)]
        retire = len(self._mix_y) > self._mix_depth
        out = self._mix_y[0] if retire else np.empty_like(y)      # (the device engine's slot rule, aliasing included)
        api.mix_apply_host(self._mix_y, alpha, out, self._mix_x)
        if retire:
            del self._mix_y[0], self._mix_f[0]
        if isinstance(self.gain, np.ndarray):
            self.gain = self._mix_x.reshape(self.gain.shape).copy()
        else:
            self.gain.copy_(torch.from_numpy(self._mix_x).reshape(self.gain.shape))

    def mix_end(self):
        for name in ("_mix_x", "_mix_y", "_mix_f", "_mix_pending"):
            self.__dict__.pop(name, None)


def _check_mixing(mixing):
    if isinstance(mixing, bool) or not isinstance(mixing, (int, np.integer)) or not 0 <= mixing <= api.MIX_MAX_DEPTH:
        raise ValueError("mixing is the Anderson depth, an integer 0 .. %d, got %r" % (api.MIX_MAX_DEPTH, mixing))
    return int(mixing)


class _MixState:
    """The host side of the Anderson mixing of cbet_fixed_point: the Gram matrix of the held residuals,
    the restart rule and the report.  Every rank runs it on the same numbers (rank 0's Gram row), so coefficients, drops and
    restarts are identical everywhere."""

    def __init__(self, depth, engine):
        self.depth, self.engine = depth, engine
        self.gram = np.zeros((0, 0))
        self.mixed = False                 # the step that produced the current iterate combined more than one entry
        self.rep = {"depth": depth, "held": [], "restarts": 0, "dropped": 0, "residual_l2": [], "alpha": [],
                    "alpha_history": [], "bytes": int(getattr(engine, "mix_bytes", 0))}

    def note(self, row):
        """Steps 3-5 of a pass: the agreed Gram row {<f_n, f_j> for the held j, <f_n, f_n>} -> restart or not, push."""
        row = np.asarray(row, dtype=np.float64).reshape(-1)
        held, ff = self.gram.shape[0], float(row[-1])
        assert row.size == held + 1, (row.size, held)
        if self.mixed and ff > float(self.gram[-1, -1]):       # the residual grew after a mixed step: start over
            self.gram, held = np.zeros((0, 0)), 0
            row = row[-1:]
            self.rep["restarts"] += 1
        g = np.zeros((held + 1, held + 1))
        g[:held, :held] = self.gram
        g[held, :] = row
        g[:, held] = row
        self.gram = g
        self.rep["held"].append(held + 1)
        self.rep["residual_l2"].append(float(np.sqrt(ff)))

    def step(self):
        """Steps 6-7: the coefficients of the held entries, the engine's combination, the oldest entry retired when all
        depth + 1 are held (its slot takes the new iterate)."""
        alpha, dropped = api.mix_coefficients(self.gram)
        alpha = alpha[dropped:]
        self.gram = self.gram[dropped:, dropped:]
        self.rep["dropped"] += dropped
        self.engine.mix_apply(alpha)
        self.mixed = alpha.size > 1
        if self.gram.shape[0] > self.depth:
            self.gram = self.gram[1:, 1:]
        self.rep["alpha"] = [float(a) for a in alpha]
        self.rep["alpha_history"].append(self.rep["alpha"])


def _fixed_point_mixed(engine, gain_params, rank, world_size, group, depth):
    """cbet_fixed_point with Anderson mixing of depth `depth` >= 1 on the passes with frozen directions: the plain loop's
    passes, each followed by the residual pass and (unless it converged or was the last) the mixed step."""
    from .tracer import shard_of_rank
    si, sc = shard_of_rank(rank, world_size)
    force = getattr(engine, "force_collectives", False)
    engine.begin()
    rep = _new_report()
    mix = None
    try:
        for it in range(gain_params.max_passes):
            full = it < gain_params.direction_passes
            fields = engine.field_passes(it > 0, si, sc, full)
            if world_size > 1 or force:
                allreduce_grid(fields if full else fields[0], group, force)
            if not full and mix is None:
                engine.mix_begin(depth)            # (before the update: it keeps the iterate the update overwrites)
                mix = _MixState(depth, engine)
            done = _note_pass(rep, it, _agree(engine.update_gain(fields, not full), group, world_size), gain_params)
            if mix is not None:
                mix.note(_agree(engine.mix_residual(), group, world_size).numpy())
            if done:
                break
            if mix is not None and it + 1 < gain_params.max_passes:      # (the last pass leaves y_n, as the plain loop does)
                mix.step()
    finally:
        if mix is not None:
            engine.mix_end()
    rep["mixing"] = mix.rep if mix is not None else _MixState(depth, engine).rep
    return _note_balance(rep, engine.deposit(si, sc), group, world_size, force)


def cbet_fixed_point(engine, gain_params, rank=0, world_size=1, group=None, mixing=0):
    """The CBET fixed-point iteration over `world_size` ranks (parity unpinned).

    Every pass: each rank deposits the fields of ITS share of the ray bundles (the plain pass's sharding) -- all four
    in the first gain_params.direction_passes passes, which build the direction field k, the energy field alone
    afterwards (gain changes ray energies, not ray paths: k of the gain-free pass is kept) --, the deposited fields
    are summed over ranks with one all-reduce, and every rank updates the full gain coefficient from them
    (redundantly -- it needs all of it for its own rays).
    Stops when sum |dK| / sum |K| < tolerance (rank 0's value, broadcast), then runs the deposition pass and
    all-reduces the per-beam energy balance.  `engine` supplies the per-rank compute:
        begin(); field_passes(use_gain, shard_index, shard_count, full) -> fields tensor;
        update_gain(fields, frozen) -> tensor {sum |dK|, sum |K|}; deposit(shard_index, shard_count) -> beam_gain tensor
    (the device engine is RayTracer.cbet_solve's; the CPU tests drive this loop with an oracle engine).
    Returns {passes, converged, change, beam_gain, imbalance}.

    mixing = depth 1 .. 4: Anderson mixing of the gain iterate on the passes with frozen directions.
    The update's own step y = x + relax (K(x) - x) and its convergence test are unchanged; behind them the residual
    f = y - x is formed, the last depth + 1 pairs (y, f) are held, and the next pass starts from the combination
    sum alpha_j y_j whose residual combination is smallest (sum alpha_j = 1).  A residual that grows after a mixed step
    clears the history (a restart: the next step is the plain step, bit for bit); an entry the Gram matrix cannot tell
    from the newer ones is dropped.  The engine then also supplies mix_begin(depth); mix_residual() -> tensor
    {<f, f_j> for the held j, <f, f>}; mix_apply(alpha); mix_end() -- the device engine with the kernels of cbet_mix.hip,
    a host engine by mixing HostMixing in -- and HOLDS 2 depth + 3 gain stacks instead of one: 91 GB at depth 4 for
    256^3 / 60 beams (8.24 GB each), beside the 41.2 GB workspace.  Rank 0's Gram row is broadcast and every rank solves
    for the same coefficients.  The report gains "mixing": {depth, held (entries per pass), restarts, dropped,
    residual_l2 (per frozen pass), alpha (of the last step), alpha_history, bytes}."""
    if _check_mixing(mixing):
        return _fixed_point_mixed(engine, gain_params, rank, world_size, group, mixing)
    from .tracer import shard_of_rank        # (tracer.py imports this module)
    si, sc = shard_of_rank(rank, world_size)
    force = getattr(engine, "force_collectives", False)   # one rank, but every collective really runs (RCCL smoke test)
    engine.begin()
    rep = _new_report()
    for it in range(gain_params.max_passes):
        full = it < gain_params.direction_passes
        fields = engine.field_passes(it > 0, si, sc, full)
        if world_size > 1 or force:
            allreduce_grid(fields if full else fields[0], group, force)
        if _note_pass(rep, it, _agree(engine.update_gain(fields, not full), group, world_size), gain_params):
            break
    return _note_balance(rep, engine.deposit(si, sc), group, world_size, force)


def _new_report():
    return {"passes": 0, "converged": False, "change": float("inf")}


def _note_pass(rep, it, ch, gain_params):
    """The convergence bookkeeping of pass `it` from the agreed scalars ch = {sum |dK|, sum |K|}; True: converged, stop."""
    rep["passes"] = it + 1
    rep["change"] = float(ch[0] / ch[1]) if float(ch[1]) > 0 else 0.0
    rep["converged"] = rep["change"] < gain_params.tolerance
    return rep["converged"]


def _note_balance(rep, beam_gain, group, world_size, force):
    """The tail of both loops: the deposition pass's per-beam energy balance summed over ranks, and its imbalance."""
    if world_size > 1 or force:
        allreduce_grid(beam_gain, group, force)
    bg = beam_gain.cpu().numpy().copy()
    rep["beam_gain"] = bg
    rep["imbalance"] = float(abs(bg.sum()) / np.abs(bg).sum()) if np.abs(bg).sum() > 0 else 0.0
    return rep


def _numeric_layout(layout):
    """slab_layout given as a number > 1: slabs cut by modelled cost, none wider than that multiple of the equal share."""
    return isinstance(layout, (int, float)) and not isinstance(layout, bool) and float(layout) > 1.0


def _parts(total, world_size):
    """Contiguous near-equal parts of range(total): [(lo, hi)] per rank (cbet_cbet_slab_workspace_bytes uses the
    same rule).  Parts are empty when world_size > total."""
    return [((r * total) // world_size, ((r + 1) * total) // world_size) for r in range(world_size)]


def balanced_slabs(weights, world_size, widest=None):
    """Contiguous plane ranges [(lo, hi)] per rank whose summed `weights` (one per plane of the haloed grid) are as equal as
    whole planes allow; every rank gets at least one plane while there are enough.  widest: no slab wider than this many
    planes (a per-plane constant is added to the weights until that holds: the cut moves towards equal plane counts) --
    the time of a grouped send/recv is set by its largest message, i.e. by the widest slab, so work balance is bought with
    link time.  The same deterministic rule on every rank (the weights come out of an all-reduce of integers)."""
    w = np.asarray(weights, dtype=np.float64)
    X = len(w)
    if world_size >= X or not np.isfinite(w).all() or w.sum() <= 0:
        return _parts(X, world_size)

    def cut(v):
        cum = np.concatenate([[0.0], np.cumsum(v)])
        cuts = [0]
        for r in range(1, world_size):
            target = cum[-1] * r / world_size
            x = int(np.searchsorted(cum, target))
            if x > 0 and abs(cum[x - 1] - target) <= abs(cum[min(x, X)] - target):
                x -= 1
            cuts.append(min(max(x, cuts[-1] + 1), X - (world_size - r)))
        cuts.append(X)
        return [(cuts[r], cuts[r + 1]) for r in range(world_size)]

    out = cut(w)
    if widest is not None:
        widest = max(int(widest), -(-X // world_size))
        lam, mean = 0.0, w.mean()
        for _ in range(40):
            if max(hi - lo for lo, hi in out) <= widest:
                break
            lam = mean * 0.05 if lam == 0.0 else lam * 1.5
            out = cut(w + lam)
        else:
            out = _parts(X, world_size)
    return out


def slab_pieces(layout, nx_halo, world_size, weights=None):
    """Which planes of the deposit grid each rank's gain update owns: [[(lo, hi), ...] per rank].
    "equal"  : one x-slab per rank, equal plane counts (the beams cross at the centre: the central ranks' update takes
               twice the outer ranks');
    "paired" : the grid is cut into 2 W equal blocks and rank r owns block r AND block W + r -- one from the left half
               counted from the edge, one from the right half counted from the centre, i.e. a light and a heavy one: the work
               evens out (modelled cost spread 1.53 -> 1.13 at 256^3 / 60 beams / 8 ranks) while every message keeps the
               same size, so no link carries more than another (twice the messages, half as long);
    a number > 1 : one slab per rank cut by the modelled gain-update cost `weights`, none wider than that multiple of the
               equal share (balanced_slabs) -- balances better and lengthens every grouped call by the widest slab;
    "halves" : the equal slab as TWO pieces (lower and upper half of its planes): the loop updates them one after the other
               and sends the first half's gain back while the second half updates (never priced on real links)."""
    if layout == "halves":
        out = []
        for lo, hi in _parts(nx_halo, world_size):
            mid = lo + (hi - lo + 1) // 2
            out.append([(lo, mid), (mid, hi)])          # (always two, an empty one included: the ranks exchange piece by piece)
        return out
    if layout == "paired" and world_size > 1:
        blocks = _parts(nx_halo, 2 * world_size)
        return [[b for b in (blocks[r], blocks[world_size + r]) if b[1] > b[0]] or [(0, 0)] for r in range(world_size)]
    if _numeric_layout(layout) and world_size > 1 and weights is not None:
        return [[pc] for pc in balanced_slabs(weights, world_size, widest=float(layout) * nx_halo / world_size)]
    return [[pc] for pc in _parts(nx_halo, world_size)]


def gain_update_weights(counts):
    """Per-plane cost of the gain update from the number of beams present at each node (`counts`, integer [X][Y][Z], summed
    over ranks).  The pair-once kernel works in runs of 16 cells along z whose cells advance in lockstep, so a run costs what
    its most crowded cell costs, and that grows with the SQUARE of the beams there (pairs): timed on 8-plane slabs of the
    256^3 / 60-beam grid, a plane costs 0.048 ms where the runs' maxima average m^2 = 154 and 0.125 ms where they average
    284 -- 2.6 x for 1.2 x the beams per node -- and ms per plane = 6.2e-4 (mean m^2 - 78) fits to 12 %
    (scripts/gain_plane_cost.py, profiles/r4/gain_plane_cost.log).  Returns a float64 numpy array [X] (relative weights)."""
    n = counts.to(torch.float64)
    X, Y, Z = n.shape
    pad = (-Z) % 16
    m = torch.nn.functional.pad(n, (0, pad)).view(X, Y, (Z + pad) // 16, 16).max(-1).values
    return (m * m - 78.0).clamp_(min=8.0).sum((1, 2)).cpu().numpy()


def cbet_fixed_point_slabs(engine, gain_params, nbeams, nx_halo, rank=0, world_size=1, group=None, sparse=False,
                           trace_groups=4, slab_layout="equal", two_channels=False):
    """The CBET fixed-point iteration with storage, exchange and schedule sized for 8 ranks on point-to-point xGMI (SURVEY
    8(f) f1; parity unpinned; same passes and same result as cbet_fixed_point).

    Rank r traces WHOLE beams [b_r0, b_r1) -- their four fields are complete on r without any reduction -- and
    owns some planes of the deposit grid for the gain update (its PIECES, slab_pieces).  It STORES only
        its own beams over the whole grid : own_fields [4][nb_r][X][Y][Z], gain_own [nb_r][X][Y][Z]
        all beams over its own pieces     : per piece slab_fields [4][nb][x_p][Y][Z], gain_slab [nb][x_p][Y][Z]
    (cbet_cbet_slab_workspace_bytes_parts).  slab_layout says which planes.  "equal" (default): one x-slab per rank, equal
    plane counts -- the beams cross at the centre, a central plane's update costs twice an outer one's, and the central
    ranks' update takes 2.4 ms against the outer ranks' 1.2 (256^3 / 60 beams / 8 ranks) while everybody waits for it.
    "paired": every rank owns one block of the grid's left half counted from the edge and one of its right half counted
    from the centre -- a light and a heavy one, messages of equal size (twice as many, half as long): measured 1.9-2.25 ms
    on every rank (two 16-plane launches each pay their ramp and drain), i.e. 0.15 ms off the slowest.  A number > 1: one
    slab per rank cut by the modelled cost (gain_update_weights from the beams counted per node after the first field
    pass, all-reduced once), none wider than that multiple of the equal share: 1.7-2.0 ms everywhere when unlimited, but a
    grouped send/recv lasts as long as its largest message, which goes to the widest slab (1.6 x), and at the 64 GB/s the
    links are priced with that costs more than the balance saves.  Neither moves the iteration outside the noise of the
    one-GPU emulation (scripts/cbet_rank_share.py, profiles/r4/cbet_rank_share.log); the simplest stays the default.
    "halves": the equal slab updated as its lower and its upper half one after the other, the lower half's gain on its way
    back while the upper half updates.  two_channels=True: the gain's way back gets its own communicator and stream, so a
    pass's fields never queue behind gain messages.  Both are schedule changes only (same arithmetic on the same cells;
    equality tests at 2 and 3 ranks) and neither has been priced: that needs real links, the one-GPU emulation shares one
    copy engine between the "channels".

    One pass, pipelined over beam GROUPS (trace_groups of them; engine.trace_group rotates them over its trace streams):
        trace group g  ->  exchange 1 of group g's beams (while the later groups trace): my beams' fields over slab s to
        rank s, all peers of a beam in one grouped send/recv  ->  [all groups in]  gain update of ALL beams on my slab
        ->  exchange 2, group by group in the order the next pass traces them: the gain of rank q's beams over my
        slab back to q  ->  the next pass's trace of group g starts as soon as ITS gain is in.
    The two scalars of the convergence measure are all-reduced and rank 0's copy decides, while exchange 2 is already
    in flight.  At 256^3 / 60 beams / 8 ranks a rank sends 3.6 GB + 0.9 GB in the direction-building first pass and
    0.9 GB + 0.9 GB in every later one (energy field only).  sparse=True: the un-pipelined exchange of only the z-runs
    inside the beams' footprints (SegmentPlan; exact; does not pay for this physics, see profiles/r3/cbet_rank_share.log).
    `engine`: begin_beams(b0, b1); trace_group(i0, i1, use_gain, full, wait) -> event or None; presence_counts() ->
    integer [X][Y][Z]; begin_slab(pieces); attributes own_fields, gain_own, slab_fields, gain_slab (lists, one per piece);
    update_gain_slab(frozen[, after_piece]) -> tensor {sum |dK|, sum |K|} over the slab; deposit_beams() -> beam_gain.  The
    deposition grid is left un-reduced (allreduce_grid / reduce_scatter_grid)."""
    beams = _parts(nbeams, world_size)
    b0, b1 = beams[rank]
    nbr = b1 - b0
    imax = max(q1 - q0 for q0, q1 in beams)
    groups = [g for g in _parts(imax, max(1, min(trace_groups, imax))) if g[1] > g[0]]     # beam-INDEX ranges, the same on every rank
    force = getattr(engine, "force_collectives", False)   # one rank, but every collective really runs (RCCL smoke test)
    engine.begin_beams(b0, b1)
    xch = _SlabExchanger(engine.own_fields.device, group, rank, world_size, beams, force_collectives=force,
                         emulate=getattr(engine, "emulate_transport", None), two_channels=two_channels)
    engine.exchanger = xch
    on_device = engine.own_fields.is_cuda

    def cur():
        return torch.cuda.current_stream(engine.own_fields.device) if on_device else None

    def wait_here(events):
        _wait_events(cur(), events)

    def mark():
        return _event_on(cur())

    def all_reduced(t):
        return all_reduce_staged(t, group) if (world_size > 1 or force) else t

    # sparse = True: the exchanges move only the 64-byte z-runs a beam's rays can ever touch instead of dense sub-arrays.
    # Exact, but it does not pay for this physics: 73 % of the nodes are inside a beam's footprint.  (The footprint pass
    # uses the field arrays as scratch and resets the counters: before the first field pass.)
    support = engine.support_mask() if (sparse and hasattr(engine, "support_mask") and (world_size > 1 or force)) else None
    slabs, pieces, plan = None, None, None
    allocated = None    # event behind the first-pass allocation (zero-fill) of the slab arrays
    G = len(groups)
    gain_ev = [None] * G
    owed = []           # groups whose gain of the previous pass has not been sent back yet (it goes out between this pass's traces)
    updated = None
    # ONE in-order channel carries both exchanges (RCCL serialises the calls of a communicator), so the order they are
    # enqueued in is the schedule: behind the update the gain of ALL groups goes back, group by group in the order the next
    # pass traces them and before the host has even looked at the convergence scalars; group k of the next pass starts
    # tracing when ITS gain is in (k + 1 calls into the exchange) and the groups overlap on the rotating trace streams;
    # a group's fields are enqueued right behind its trace and travel while the later groups trace.  (Measured with the
    # kernel trace of scripts/cbet_rank_share.py: sending a group's gain just ahead of its own trace, interleaved with
    # the fields of earlier groups, chains trace -> fields -> gain -> trace through the one channel and stretches the
    # trace phase from 4.5 to 9 ms.)  HEAD = groups whose gain goes back before the scalars are looked at, LAG = groups
    # between a trace and the enqueueing of its fields.
    HEAD, LAG = G, 0

    def send_gain(k):
        i0, i1 = groups[k]
        return xch.gain_back(engine.gain_slab, engine.gain_own, i0, i1, after=(updated,))

    rep = _new_report()
    for it in range(gain_params.max_passes):
        full = it < gain_params.direction_passes
        comps = range(4) if full else range(1)    # after the direction-building passes only the energy field moves
        traced = [None] * G
        for k, (i0, i1) in enumerate(groups):
            if k in owed:
                gain_ev[k] = send_gain(k)
                owed.remove(k)
            j0, j1 = min(i0, nbr), min(i1, nbr)
            if j1 > j0:
                traced[k] = engine.trace_group(j0, j1, it > 0, full, wait=(gain_ev[k],))
            if slabs is not None and plan is None and k >= LAG:
                xch.fields_out(engine.own_fields, engine.slab_fields, *groups[k - LAG], comps, after=(traced[k - LAG], updated))
        if slabs is None:
            # first pass: the beams' footprints are known now -- cut the slabs, allocate them, then send everything
            wait_here(traced)
            layout = "equal" if support is not None else slab_layout     # (the sparse plan is written for one slab per rank)
            weights = None
            if _numeric_layout(layout) and world_size > 1:
                counts = all_reduced(engine.presence_counts())
                weights = gain_update_weights(counts)
                del counts
            pieces = slab_pieces(layout, nx_halo, world_size, weights)
            slabs = [pcs[0] for pcs in pieces]                            # (what the sparse plan indexes by)
            engine.begin_slab(pieces[rank])
            xch.set_slabs(pieces)
            if support is not None:
                plan = SegmentPlan(support, beams, slabs, rank, world_size, group, engine.slab_fields[0].device)
                support = None
                xch.use_plan(plan)
            # begin_slab / use_plan zero-fill their arrays on THIS stream, which has just been made to wait for every trace
            # group; the exchanges below run on the communication stream and wait for their own group's trace only -- without
            # this event group 0's fields would land in slab_fields before the (late) fill and be zeroed by it
            allocated = mark()
            first = 0
        else:
            first = G - LAG
        if plan is not None:
            xch.run_sparse(engine.own_fields, lambda s_: (slice(0, len(comps)), slice(None), slice(*slabs[s_])),
                           engine.slab_fields[0], lambda q: (slice(0, len(comps)), slice(*beams[q])), True,
                           ncomp=len(comps), after=list(traced) + [allocated])
        else:
            for k in range(first, G):
                # (`updated`: a rank without a beam in this group has no trace to wait for, and with two channels nothing
                # else keeps the peers' fields out of slab_fields while the previous update still reads them)
                xch.fields_out(engine.own_fields, engine.slab_fields, *groups[k], comps, after=(traced[k], allocated, updated))
        allocated = None
        wait_here([xch.fence()])                     # every beam's fields over my slab are in
        if xch.two_channels:
            wait_here(gain_ev)                       # ... and the previous gain has left gain_slab (one channel: in order)
        split = slab_layout == "halves" and plan is None

        def piece_done(kp, ev):
            # the gain of piece kp is final behind `ev`: all groups' share of it goes back, while the next piece updates
            for k in range(G):
                gain_ev[k] = xch.gain_back(engine.gain_slab, engine.gain_own, *groups[k], after=(ev,), only_piece=kp)
        ch = engine.update_gain_slab(not full, after_piece=piece_done) if split else engine.update_gain_slab(not full)
        updated = mark()
        # the gain of rank q's beams over my slab -> rank q; my beams' gain over slab s <- rank s.  It is due whatever the
        # convergence scalars say (the deposition pass needs the new gain too): the head goes out now
        if plan is not None:
            ev = xch.run_sparse(engine.gain_slab[0], lambda q: (slice(*beams[q]),),
                                engine.gain_own, lambda s_: (slice(None), slice(*slabs[s_])), False, after=(updated,))
            gain_ev, owed = [ev] * G, []
        elif split:
            owed = []                                # (went back piece by piece, see piece_done)
        else:
            for k in range(HEAD):
                gain_ev[k] = send_gain(k)
            owed = list(range(HEAD, G))
        if _note_pass(rep, it, _agree(all_reduced(ch), group, world_size), gain_params):
            break
    for k in list(owed):                              # no further pass: the rest of the gain goes back now
        gain_ev[k] = send_gain(k)
    wait_here(gain_ev)
    _note_balance(rep, engine.deposit_beams(), group, world_size, force)
    rep["slabs"] = pieces
    rep["groups"] = groups
    return rep
