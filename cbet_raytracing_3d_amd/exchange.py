"""The slab exchange of the slab-owned CBET loop (cbet_loop.cbet_fixed_point_slabs): _SlabExchanger moves the beams'
fields to the slab owners and the gain back over point-to-point links, dense or -- with a SegmentPlan -- only the
64-byte z-runs inside the beams' footprints; the small stream / event / rank helpers the loop shares with it."""
from contextlib import nullcontext

import torch

from . import api


def _global_rank(group, r):
    """The global rank of rank r of `group` (None: the default group, whose ranks are the global ones)."""
    import torch.distributed as dist
    return r if group is None else dist.get_global_rank(group, r)


def _wait_events(stream, events):
    """Make `stream` (None: no device, nothing to order) wait for those of `events` that are not None."""
    if stream is not None:
        for ev in events:
            if ev is not None:
                stream.wait_event(ev)


def _event_on(stream):
    """An event behind everything enqueued so far on `stream` (None without a device)."""
    if stream is None:
        return None
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


class _SlabExchanger:
    """The two all-to-all exchanges of the slab-owned CBET loop over point-to-point xGMI links (RCCL send/recv; gloo in
    the CPU tests), one message per (beam, peer, component) and NO staging: the part of a beam over an x-slab is
    contiguous both in the sender's whole-grid array and in the receiver's slab array, so messages go from and into the
    arrays themselves.

    * All W - 1 peers at once: the sends of my i-th beam to every slab owner and the receives of every peer's i-th beam
      are ONE grouped send/recv (batch_isend_irecv = ncclGroupStart ... End), so all seven links of a rank carry a
      message at the same time.  Chunks are beams (and components), never peers.
    * Stream-ordered: everything runs on a communication stream that waits for the producer's event (the trace of the
      beam's group; the gain update) and hands an event to the consumer (the gain update; the next trace of the group) --
      no host synchronisation.  A group's fields travel while the next group traces; a group's gain comes back while
      the previous groups already trace the next pass.
    * gloo has no device path: device tensors are staged through the host message by message (tests only).
    Ranks without beams or planes simply post nothing; every rank walks the beam indices in the same order, so the
    sends and receives of a pair match in order."""

    def __init__(self, device, group, rank, world_size, beams, force_collectives=False, emulate=None, two_channels=False):
        import torch.distributed as dist
        self.group, self.device, self.rank, self.world, self.beams = group, torch.device(device), rank, world_size, beams
        self.cuda = self.device.type == "cuda"
        self.dist_on = dist.is_available() and dist.is_initialized()
        # emulate(exchanger, sends, recvs): a stand-in for the transport of one grouped send/recv, run on the communication
        # stream exactly where RCCL's would be (scripts/cbet_rank_share.py: one rank's schedule on one GPU, the peers'
        # data supplied and the link time priced) -- everything else of the schedule is the product's
        self.emulate = emulate
        self.nccl = self.cuda and ((self.dist_on and dist.get_backend(group) == "nccl") or emulate is not None)
        self.force = force_collectives      # one rank: the same send/recv machinery as a self-exchange (RCCL smoke test)
        self.stream = torch.cuda.Stream(device=self.device) if self.nccl else None
        # two_channels: exchange 2 (the gain's way back) gets a communicator and a stream of its own, so that a pass's fields
        # do not queue behind the previous pass's gain on one in-order channel (every rank creates the second group here, in
        # the same place of its program: new_group is collective)
        self.group2, self.stream2 = group, self.stream
        self.two_channels = False
        if two_channels and emulate is not None:
            self.stream2, self.two_channels = (torch.cuda.Stream(device=self.device) if self.nccl else None), True
        elif two_channels and self.dist_on and (world_size > 1 or force_collectives):
            self.two_channels = True
            ranks = dist.get_process_group_ranks(group) if group is not None else list(range(dist.get_world_size()))
            self.group2 = dist.new_group(ranks=ranks, backend=dist.get_backend(group))
            self.stream2 = torch.cuda.Stream(device=self.device) if self.nccl else None
        self.solo = world_size == 1
        self.peers = [rank] if (self.solo and self.force) else [r for r in range(world_size) if r != rank]
        self.slabs = None
        self.plan = None
        self.send_buf = self.recv_buf = None    # sparse exchanges only
        self.chunks = self.messages = self.bytes_sent = 0

    def set_slabs(self, pieces):
        """pieces[r] = the plane ranges [(lo, hi), ...] rank r's gain update owns (slab_pieces)."""
        self.slabs = pieces

    def staging_bytes(self):
        if self.send_buf is None or self.send_buf.device != self.device:
            return 0
        return 8 * (self.send_buf.numel() + self.recv_buf.numel())

    def _channel(self, back=False):
        """The stream an exchange is ordered on: the communication stream (RCCL) -- the second channel's for the gain's way
        back (`back`) -- or the current one (None without a device)."""
        if self.nccl:
            return self.stream2 if back else self.stream
        return torch.cuda.current_stream(self.device) if self.cuda else None

    def _enter(self, after, back=False):
        """Order what follows behind the events in `after`, on that channel."""
        _wait_events(self._channel(back), after)
        return torch.cuda.stream(self._channel(back)) if self.nccl else nullcontext()

    def _leave(self, back=False):
        """An event behind everything issued so far on that channel (None without a device)."""
        return _event_on(self._channel(back))

    def fence(self):
        return self._leave()

    def _batch(self, sends, recvs, back=False):
        """One grouped send/recv: `sends` / `recvs` are (tensor view, peer) lists of contiguous views."""
        import torch.distributed as dist
        group = self.group2 if back else self.group
        if not sends and not recvs:
            return
        if self.emulate is not None:
            self.emulate(self, sends, recvs)
            self.bytes_sent += 8 * sum(t.numel() for t, _ in sends)
            self.chunks += 1
            self.messages += len(sends) + len(recvs)
            return
        ops, late = [], []
        for t, peer in sends:
            if self.cuda and not self.nccl:
                t = t.cpu()                         # gloo: through the host (synchronises the current stream)
            ops.append(dist.P2POp(dist.isend, t, _global_rank(self.group, peer), group))
            self.bytes_sent += 8 * t.numel()
        for t, peer in recvs:
            if self.cuda and not self.nccl:
                h = torch.empty(t.shape, dtype=t.dtype, device="cpu")
                late.append((t, h))
                t = h
            ops.append(dist.P2POp(dist.irecv, t, _global_rank(self.group, peer), group))
        for req in dist.batch_isend_irecv(ops):
            req.wait()     # RCCL: the communication stream waits (no host block); gloo: the host waits
        for t, h in late:
            t.copy_(h)
        self.chunks += 1
        self.messages += len(ops)

    def fields_out(self, own, slab, i0, i1, comps, after=()):
        """Exchange 1 for the beams with index [i0, i1) of every rank: my beams' fields over rank s's pieces -> rank s, rank
        q's beams over my pieces <- rank q, component by component of `comps`.  own: [4][my beams][X][Y][Z]; slab: one
        [4][all beams][piece planes][Y][Z] per piece of mine."""
        rank, beams, pieces = self.rank, self.beams, self.slabs
        b0, b1 = beams[rank]
        with self._enter(after):
            for i in range(i0, i1):
                sends, recvs = [], []
                mine = i < b1 - b0
                for s_ in self.peers:
                    if mine:
                        sends += [(own[c, i, lo:hi], s_) for lo, hi in pieces[s_] if hi > lo for c in comps]
                    q0, q1 = beams[s_]
                    if i < q1 - q0:
                        recvs += [(slab[k][c, q0 + i], s_) for k, (lo, hi) in enumerate(pieces[rank]) if hi > lo for c in comps]
                if mine and not (self.solo and self.force):
                    for k, (lo, hi) in enumerate(pieces[rank]):
                        for c in comps:
                            if hi > lo:
                                slab[k][c, b0 + i].copy_(own[c, i, lo:hi])       # the own part never travels
                self._batch(sends, recvs)
        return self._leave()

    def gain_back(self, gain_slab, gain_own, i0, i1, after=(), only_piece=None):
        """Exchange 2 for the beams with index [i0, i1): the new gain of rank q's beams over my pieces -> rank q, my beams'
        gain over rank s's pieces <- rank s.  gain_slab: one [all beams][piece planes][Y][Z] per piece of mine; gain_own:
        [my beams][X][Y][Z].  only_piece = k: the k-th piece of EVERY rank alone (the loop sends a half slab's gain while the
        other half still updates; every rank has the same number of pieces then).  Runs on the second channel when there is
        one.  Returns the event behind it: the next pass's trace of these beams waits for it."""
        rank, beams, pieces = self.rank, self.beams, self.slabs
        b0, b1 = beams[rank]

        def want(k):
            return only_piece is None or k == only_piece
        with self._enter(after, back=True):
            for i in range(i0, i1):
                sends, recvs = [], []
                mine = i < b1 - b0
                for q in self.peers:
                    q0, q1 = beams[q]
                    if i < q1 - q0:
                        sends += [(gain_slab[k][q0 + i], q) for k, (lo, hi) in enumerate(pieces[rank]) if hi > lo and want(k)]
                    if mine:
                        recvs += [(gain_own[i, lo:hi], q) for k, (lo, hi) in enumerate(pieces[q]) if hi > lo and want(k)]
                if mine and not (self.solo and self.force):
                    for k, (lo, hi) in enumerate(pieces[rank]):
                        if hi > lo and want(k):
                            gain_own[i, lo:hi].copy_(gain_slab[k][b0 + i])
                self._batch(sends, recvs, back=True)
        return self._leave(back=True)

    # ---- the sparse form: only the 64-byte z-runs inside the beams' footprints move (SegmentPlan) --------------------
    def use_plan(self, plan):
        """Sparse exchanges: staging for the runs of ALL peers of one component at once, out and in."""
        self.plan = plan
        stage_dev = self.device if (self.nccl or not self.cuda) else torch.device("cpu")
        peers = self.peers
        n_out = 8 * max(sum(plan.own_side[s].shape[0] for s in peers), sum(plan.slab_side[q].shape[0] for q in peers))
        self.send_buf = torch.empty(n_out, dtype=torch.float64, device=stage_dev)
        self.recv_buf = torch.empty(n_out, dtype=torch.float64, device=stage_dev)

    def _pack(self, arr, stride, hy, hz, seg, out):
        n = seg.shape[0]
        if arr.is_cuda:
            api.pack_segments(arr, stride, hy, hz, seg, n, out, torch.cuda.current_stream(arr.device).cuda_stream)
        else:
            idx, valid = _pack_rows_cpu(arr, stride, hz, seg)
            out[: 8 * n].view(n, 8).copy_(arr.reshape(-1)[idx] * valid)

    def _unpack(self, arr, stride, hy, hz, seg, buf):
        n = seg.shape[0]
        if arr.is_cuda:
            api.unpack_segments(arr, stride, hy, hz, seg, n, buf, torch.cuda.current_stream(arr.device).cuda_stream)
        else:
            idx, valid = _pack_rows_cpu(arr, stride, hz, seg)
            arr.view(-1)[idx[valid]] = buf[: 8 * n].view(n, 8)[valid]

    def run_sparse(self, src, send_index, dst, recv_index, to_slabs, ncomp=0, after=()):
        """One exchange moving only the z-runs of the plan: to_slabs = exchange 1 (pack from my whole-grid array, unpack
        into my slab array), else exchange 2.  ncomp > 0: the arrays carry that many leading components.  Per component:
        the runs of ALL peers are packed into consecutive stretches of the send staging buffer, travel in one grouped
        send/recv, and are unpacked from the receive staging buffer.  Stream-ordered like the dense form."""
        import torch.distributed as dist
        plan, rank = self.plan, self.rank
        hy, hz = plan.Y, plan.Z
        out_lists, in_lists = (plan.own_side, plan.slab_side) if to_slabs else (plan.slab_side, plan.own_side)
        out_stride, in_stride = (plan.own_stride, plan.slab_stride) if to_slabs else (plan.slab_stride, plan.own_stride)
        dev_stage = self.send_buf.device == src.device
        with self._enter(after):
            if not (self.solo and self.force):
                dst[recv_index(rank)] = src[send_index(rank)]       # the own part: a dense local copy
            for c in range(max(1, ncomp)):
                s_arr = src[c] if ncomp else src
                d_arr = dst[c] if ncomp else dst
                ops, off_out, off_in, unpack = [], 0, 0, []
                for peer in self.peers:
                    seg_out, seg_in = out_lists[peer], in_lists[peer]
                    n_out, n_in = seg_out.shape[0], seg_in.shape[0]
                    if n_out:
                        sb = self.send_buf[off_out: off_out + 8 * n_out]
                        if dev_stage:
                            self._pack(s_arr, out_stride, hy, hz, seg_out, sb)
                        else:                   # gloo with device arrays: pack on the device, send from the host buffer
                            tmp = torch.empty(8 * n_out, dtype=torch.float64, device=src.device)
                            self._pack(s_arr, out_stride, hy, hz, seg_out, tmp)
                            sb.copy_(tmp)
                        ops.append(dist.P2POp(dist.isend, sb, _global_rank(self.group, peer), self.group))
                        self.bytes_sent += 64 * n_out
                        off_out += 8 * n_out
                    if n_in:
                        rb = self.recv_buf[off_in: off_in + 8 * n_in]
                        ops.append(dist.P2POp(dist.irecv, rb, _global_rank(self.group, peer), self.group))
                        unpack.append((seg_in, rb))
                        off_in += 8 * n_in
                if ops:
                    for req in dist.batch_isend_irecv(ops):
                        req.wait()
                    self.chunks += 1
                    self.messages += len(ops)
                for seg_in, rb in unpack:
                    self._unpack(d_arr, in_stride, hy, hz, seg_in, rb if dev_stage else rb.to(dst.device))
        return self._leave()


def _segment_rows(support, x0, x1):
    """Rows (beam, x - x0, y, z // 8) of the 64-byte z-runs of planes [x0, x1) in which `support` (bool
    [beams][X][Y][Z]) is set anywhere: the unit of the sparse exchange (cbet_pack_segments)."""
    nb, X, Y, Z = support.shape
    zs = (Z + 7) // 8
    sub = support[:, x0:x1]
    if zs * 8 != Z:
        sub = torch.nn.functional.pad(sub, (0, zs * 8 - Z))
    return sub.reshape(nb, x1 - x0, Y, zs, 8).any(-1).nonzero().to(torch.int32)


def _pack_rows_cpu(src, beam_stride, hz, seg):
    """torch restatement of cbet_pack_segments for host tensors (the gloo tests); returns (values [n][8], flat index, valid)"""
    zsegs = (hz + 7) // 8
    rows, run = seg[:, 0].long(), seg[:, 1].long()
    z = 8 * (run % zsegs)[:, None] + torch.arange(8)
    valid = z < hz
    idx = rows[:, None] * beam_stride + (run // zsegs)[:, None] * hz + z.clamp(max=hz - 1)
    return idx, valid


class SegmentPlan:
    """Who sends which 64-byte z-runs to whom in the slab-owned CBET loop, fixed for the life of a solve.

    `support` [own beams][X][Y][Z] marks every node this rank's beams can EVER deposit into -- the footprint of their
    rays traced to the exit of the grid whatever their energy (ray paths do not depend on the gain; which step a ray is
    absorbed at does) -- so the lists hold every entry any pass can make non-zero, and every entry of a beam's gain
    coefficient its rays can read.  For each peer s the rank keeps the runs of its beams inside slab s (what it packs
    for exchange 1 and unpacks in exchange 2), and -- received from the peers once, by send/recv -- the runs of every
    peer q's beams inside its own slab (what it unpacks in exchange 1 and packs for exchange 2)."""

    def __init__(self, support, beams, slabs, rank, world_size, group, device):
        import torch.distributed as dist
        nbr, X, Y, Z = support.shape
        self.Y, self.Z, self.zsegs = Y, Z, (Z + 7) // 8
        self.own_stride, self.slab_planes = X * Y * Z, slabs[rank][1] - slabs[rank][0]
        self.slab_stride = self.slab_planes * Y * Z
        mine = []            # per peer s: rows (b_local, x_rel, y, zs) of my beams in slab s
        for s in range(world_size):
            mine.append(_segment_rows(support, *slabs[s]).cpu())
        # the peers' rows for my slab: counts first, then the lists, point to point
        theirs = [None] * world_size
        theirs[rank] = mine[rank]
        if world_size > 1:
            cuda_nccl = dist.get_backend(group) == "nccl"
            cdev = device if cuda_nccl else "cpu"
            counts = torch.tensor([m.shape[0] for m in mine], dtype=torch.int64, device=cdev)
            allc = [torch.zeros_like(counts) for _ in range(world_size)]
            dist.all_gather(allc, counts, group=group)
            for k in range(1, world_size):
                to, frm = (rank + k) % world_size, (rank - k) % world_size
                ops, rb = [], None
                if mine[to].shape[0]:
                    ops.append(dist.P2POp(dist.isend, mine[to].to(cdev).contiguous(), _global_rank(group, to), group))
                n_in = int(allc[frm][rank])
                if n_in:
                    rb = torch.empty((n_in, 4), dtype=torch.int32, device=cdev)
                    ops.append(dist.P2POp(dist.irecv, rb, _global_rank(group, frm), group))
                if ops:
                    for req in dist.batch_isend_irecv(ops):
                        req.wait()
                if cuda_nccl:
                    torch.cuda.synchronize(device)
                theirs[frm] = rb.cpu() if rb is not None else torch.zeros((0, 4), dtype=torch.int32)
        zs = self.zsegs

        def pairs(rows, beam_offset, x_offset):
            if rows.shape[0] == 0:
                return torch.zeros((0, 2), dtype=torch.int32, device=device)
            r = rows.long()
            out = torch.stack([r[:, 0] + beam_offset, ((r[:, 1] + x_offset) * Y + r[:, 2]) * zs + r[:, 3]], 1)
            return out.to(torch.int32).contiguous().to(device)
        # what I address in MY whole-grid arrays (own_fields, gain_own): my beams, absolute planes, per peer slab
        self.own_side = [pairs(mine[s], 0, slabs[s][0]) for s in range(world_size)]
        # what I address in MY slab arrays (slab_fields, gain_slab): peer q's beams (global row), planes relative to my slab
        self.slab_side = [pairs(theirs[q], beams[q][0], 0) for q in range(world_size)]
        solo = world_size == 1          # the forced self-exchange of a one-rank group moves the rank's own part
        self.max_out = max([t.shape[0] for i, t in enumerate(self.own_side) if i != rank or solo] + [0])
        self.max_in = max([t.shape[0] for i, t in enumerate(self.slab_side) if i != rank or solo] + [0])
        self.runs_out = sum(t.shape[0] for i, t in enumerate(self.own_side) if i != rank)    # exchange 1 sends, exchange 2 receives
        self.runs_in = sum(t.shape[0] for i, t in enumerate(self.slab_side) if i != rank)    # exchange 1 receives, exchange 2 sends
        self.dense_out = nbr * (X - self.slab_planes) * Y * Z      # doubles a dense exchange would send

    def staging_elems(self):
        return 8 * max(self.max_out, self.max_in)

    def list_bytes(self):
        return 8 * (sum(t.shape[0] for t in self.own_side) + sum(t.shape[0] for t in self.slab_side))

