"""The plain path's combine and pipeline: allreduce_grid / reduce_scatter_grid sum the per-rank deposition grids
(RCCL over xGMI with backend "nccl", gloo in the CPU tests), and SweepPipeline overlaps the preparation, trace and
combine of consecutive passes on one rank.  torch is plumbing here, as in tracer.py: streams, events and
torch.distributed; the work is libcbet_mi355x.so's, reached through the RayTracer the pipeline is given."""
import os

import torch

from . import api


def row_pitch(nz, pad_rows):
    """Doubles per row of a deposit grid whose rows hold nz + 2 nodes (cbet_params.edep_zpitch).  pad_rows 0: dense
    rows; 1: the next multiple of 8 doubles (whole 64-byte lines); a value above nz + 2: that pitch."""
    if int(pad_rows) > nz + 2:
        return int(pad_rows)
    return -(-(nz + 2) // 8) * 8 if pad_rows else nz + 2


def all_reduce_staged(t, group=None):
    """Sum `t` over the ranks of `group` and return the tensor that holds the sum: `t` itself, reduced in place, or --
    gloo has no device path, so stage through the host -- the reduced host copy of a device tensor (the caller copies
    back what it needs of it)."""
    import torch.distributed as dist
    if t.is_cuda and dist.get_backend(group) != "nccl":
        t = t.cpu()
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


def allreduce_grid(edep, group=None, force=False):
    """Sum the per-rank deposition grids in place (RCCL all-reduce over xGMI with backend
    "nccl"; gloo on CPU tensors in the tests).  Replaces main.cu:178-210.  No-op without an
    initialised process group.  force: run the collective on a one-rank group too (RCCL smoke test)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or force):
        total = all_reduce_staged(edep, group)
        if total is not edep:
            edep.copy_(total)
    return edep


def reduce_scatter_grid(grid, slab, group=None, async_op=False, force=False):
    """Combine the per-rank deposition grids so that rank r ends up with the SUM over ranks of x-slab r
    (`slab` = planes [r P/W, (r+1) P/W) of the plane-padded grid, P a multiple of the world size W): a
    reduce-scatter, half the xGMI traffic of the all-reduce and all a slab consumer (edepavg, a gain update, the
    host copy of a slab) needs.  RCCL with backend "nccl"; gloo (CPU tests) has no reduce-scatter for this
    layout, so there the grid is all-reduced and the slab copied out.  Returns the async work handle or None."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size(group) == 1 and not force):
        slab.copy_(grid[: slab.shape[0]])
        return None
    if dist.get_backend(group) == "nccl":
        return dist.reduce_scatter_tensor(slab, grid, op=dist.ReduceOp.SUM, group=group, async_op=async_op)
    total = all_reduce_staged(grid, group)
    r, pl = dist.get_rank(group), slab.shape[0]
    slab.copy_(total[r * pl:(r + 1) * pl])
    return None


class SweepPipeline:
    """Independent passes of the plain path on one rank, pipelined over HIP streams (the passes of a sweep do not
    feed each other: main.cu:96-232 run again on the same plasma).

    Per pass k, with two alternating buffer sets b = k % 2 (deposition grid, node tables + step records = a
    second context):
        prep stream b  : [tables b free = trace k-2 done, grid b free = combine k-2 done]  zero grid b,
                         node tables and step records (one kernel, k_plasma_records)
        trace stream b : [prep k done]  trace this rank's share of the bundles into grid b, then enqueue the combine
        RCCL stream    : reduce-scatter of grid b over xGMI (torch's process-group stream, async)
    Nothing orders trace k+1 behind trace k (each buffer set has its own streams), so pass k+1's preparation AND the
    head of its trace run beside the drain of trace k -- a launch's last half millisecond runs at low occupancy, it
    cannot be shorter than one bundle's lifetime, and that is 0.8 ms of a 3.3 ms share at 8 ranks -- and combine k
    runs beside trace k+1.  Replaces
    the serial launch -> D2H -> host sum of main.cu:166-210.  The combined result of a pass is slab r of the
    grid on rank r (reduce_scatter_grid)."""

    def __init__(self, tracer, rank=0, world_size=1, group=None, overlap_traces=None, force_collectives=False, pad_rows=None):
        self.tr, self.rank, self.world, self.group = tracer, rank, world_size, group
        self.force = force_collectives      # run the RCCL combine on one rank too (smoke test of the collective path)
        # consecutive traces overlap, at one rank too: a launch's last half millisecond runs at low occupancy, and with one
        # trace stream the next pass's preparation hides there while the next trace waits behind the drain.  With two, the
        # next trace fills the drain and the pass costs the trace's steady work plus the preparation's: 12.62 ms against
        # 12.78-12.89 with one stream at 256^3, same library.  The events around a launch then measure a
        # stretched duration (kernel_ms_in_pipeline); time_trace_alone() is the launch by itself.
        self.overlap_traces = True if overlap_traces is None else bool(overlap_traces)
        p = tracer.params
        self.ctx = [tracer.ctx, api.Context(p, tracer.gpu)]
        planes = -(-(p.nx + 2) // world_size) * world_size          # padded to a multiple of the world size
        # The private grids are this class's own, so their rows are padded to whole 64-byte lines (cbet_params.edep_zpitch).
        # With dense rows of nz + 2 = 258 doubles the pass time depends on where the grid happens to land relative to the
        # record table -- 16.9 ... 18.6 ms from one allocation to the next, reproducibly per placement (the memory channel an
        # address maps to folds address bits 7 apart: scripts/placement_sweep.py) --; with rows of 264 it does not.
        # `slabs` are views of the padded slabs with the reference's (.., ny+2, nz+2) shape.
        if pad_rows is None:
            pad_rows = int(os.environ.get("CBET_PAD_ROWS", "1"))      # 0: dense rows; 1: the next multiple of 8 doubles; > nz + 2: that pitch
        zp = row_pitch(p.nz, pad_rows)
        shape = (planes, p.ny + 2, zp)
        dev = tracer.device
        self.grids = [torch.zeros(shape, dtype=torch.float64, device=dev) for _ in range(2)]
        self.slab_store = [torch.zeros((planes // world_size,) + shape[1:], dtype=torch.float64, device=dev) for _ in range(2)]
        self.slabs = [s[..., : p.nz + 2] for s in self.slab_store]
        # one stream pair per buffer set: pass k+1 may start tracing while pass k is still draining
        self.s_prep = [torch.cuda.Stream(device=dev) for _ in range(2)]
        self.s_trace = [torch.cuda.Stream(device=dev) for _ in range(2)]
        if not self.overlap_traces:
            self.s_trace[1] = self.s_trace[0]
        # (one rank: the "combine" is a copy of the grid into the slab store, on the trace stream.  On a stream of its own,
        # like RCCL's, the next trace starts right behind this one -- and the pass takes 13.2-13.3 ms instead of 13.0: the copy
        # and the next pass's preparation then run beside the kernel's first wave generation.  Measured in round 5, not kept.)
        self.ev_prep = [torch.cuda.Event() for _ in range(2)]
        self.ev_consumed = [None, None]      # release(b): a reader's event the next combine into slab b waits for
        self.ev_trace = [None, None]
        self.work = [None, None]
        self.kernel_events = []
        from .tracer import shard_of_rank        # (tracer.py imports this module)
        si, sc = shard_of_rank(rank, world_size)
        self.launch_p = p.copy(beam_lo=0, beam_hi=p.nbeams, shard_index=si, shard_count=sc,
                               edep_zpitch=zp if pad_rows else 0)
        self.passes = 0

    def run_pass(self, timed=False):
        tr, b = self.tr, self.passes % 2
        self.passes += 1
        with torch.cuda.stream(self.s_prep[b]):
            if self.ev_trace[b] is not None:
                self.s_prep[b].wait_event(self.ev_trace[b])
            if self.work[b] is not None:
                self.work[b].wait()            # this stream waits for combine k-2 before the grid is cleared
                self.work[b] = None
            self.grids[b].zero_()
            # node tables and step records in one kernel (k_plasma_records)
            tr._prepare_plasma(self.launch_p, self.ctx[b])
            self.ev_prep[b].record()
        with torch.cuda.stream(self.s_trace[b]):
            self.s_trace[b].wait_event(self.ev_prep[b])
            if timed:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            tr._trace(self.grids[b], self.launch_p, self.ctx[b])
            if timed:
                e1.record()
                self.kernel_events.append((e0, e1))
            consumed, self.ev_consumed[b] = self.ev_consumed[b], None
            if consumed is not None:
                self.s_trace[b].wait_event(consumed)       # (behind the trace launch: only the combine waits for the reader)
            self.work[b] = reduce_scatter_grid(self.grids[b], self.slab_store[b], self.group, async_op=True, force=self.force)
            # "grid b may be cleared again": recorded AFTER the combine was enqueued -- on one rank (and with gloo) the
            # combine is a copy on this very stream, and pass k+2's grid.zero_() must not overtake it; with RCCL the
            # collective runs on the process group's stream and is waited for through its work handle
            self.ev_trace[b] = torch.cuda.Event()
            self.ev_trace[b].record()
        return b

    def wait_combined(self, b):
        """Make torch's current stream wait for the combine of buffer set b's last pass: behind it `slabs[b]` is complete (the
        RCCL collective's work handle, or the event behind the local copy)."""
        cur = torch.cuda.current_stream(self.tr.device)
        if self.work[b] is not None:
            self.work[b].wait()
        if self.ev_trace[b] is not None:
            cur.wait_event(self.ev_trace[b])

    def release(self, b):
        """A reader of `slabs[b]` on torch's current stream is done with it (enqueued so far): the next combine into that slab --
        two passes on -- waits for this point instead of relying on being later anyway."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.tr.device))
        self.ev_consumed[b] = ev

    def time_trace_alone(self, reps=3):
        """Average duration (seconds) of this rank's trace launch when NOTHING else runs beside it: with more than one
        rank the pipeline lets consecutive passes' trace kernels overlap, so the events around a launch there measure a
        stretched duration; this is the time the launch needs (what a roofline fraction has to be priced with)."""
        tr = self.tr
        self.finish()
        times = []
        with torch.cuda.stream(self.s_trace[0]):
            for _ in range(reps + 1):
                self.grids[0].zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tr._trace(self.grids[0], self.launch_p, self.ctx[0])
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e-3)
        torch.cuda.synchronize(tr.device)
        return sum(times[1:]) / reps

    def window_diagnostics(self):
        """The counters of ONE un-timed trace launch of this rank's share with cbet_params.window_stats = 1: the deposit
        windows' diagnostics (wave-steps, window misses, box-B steps, planes retired, global atomics) that the timed
        launches do not count.  Call it after counters(): it resets the contexts' counters; the last pass's slab stays."""
        tr = self.tr
        self.finish()
        self.counters(reset=True)
        scratch = torch.zeros_like(self.grids[0])
        with torch.cuda.stream(self.s_trace[0]):
            tr._trace(scratch, self.launch_p.copy(window_stats=1), self.ctx[0])
        torch.cuda.synchronize(tr.device)
        return self.ctx[0].counters(self.s_trace[0].cuda_stream, True)

    def warm(self):
        """Run the combine once on the (zero) buffers: RCCL builds its communicator, channels and staging buffers on
        the first collective of a kind -- set-up, like the reference's cudaMalloc in its Init phase (main.cu:131-152),
        not part of a pass.  No-op on one rank."""
        if self.world > 1 or self.force:
            for b in range(2):
                w = reduce_scatter_grid(self.grids[b], self.slab_store[b], self.group, async_op=True, force=self.force)
                if w is not None:
                    w.wait()
            torch.cuda.synchronize(self.tr.device)

    def finish(self):
        """Wait for everything in flight; returns the slab of the last pass (this rank's planes of the sum)."""
        for b in range(2):
            if self.work[b] is not None:
                self.work[b].wait()
                self.work[b] = None
        torch.cuda.synchronize(self.tr.device)
        return self.slabs[(self.passes - 1) % 2] if self.passes else None

    def counters(self, reset=False):
        stream = self.tr._stream()
        c0, c1 = self.ctx[0].counters(stream, reset), self.ctx[1].counters(stream, reset)
        for name, _ in api.Counters._fields_:
            setattr(c0, name, getattr(c0, name) + getattr(c1, name))
        return c0

    def close(self):
        self.finish()
        self.ctx[1].close()
