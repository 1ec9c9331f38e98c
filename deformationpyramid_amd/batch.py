"""The batched pair pipeline behind Registration.register_batch: a producer that prepares pairs ahead of the GPU in
index order (PairProducer: threads and queues, nothing of the device), and the lanes that keep the engines' slots filled
(_BatchCtx / _Lane: streams and events, no threads)."""
import ctypes
import queue
import threading

import numpy as np
import torch

from . import _native as N

_NOT_READY = object()


class PairProducer:
    """Runs `prepare(item, rng_state, worker) -> prepared` over `items` ahead of the consumer and delivers the results strictly in
    index order.  Item i is prepared by worker i % W and taken from that worker's queue when its turn comes: the order of
    delivery does not depend on which worker finishes first (bit-identity with sequential register() calls rests on it).

    draws(item) -> int (the native RNG replay): the raw generator draws an item consumes are known up front, so ONE stepping
    thread walks a snapshot of torch's CPU generator state from item to item (regenerations only), hands item i the state it
    starts from -- the workers replay their items from those snapshots and leave the global generator alone -- and sets the
    global generator, at the end of its walk, to where sequential register() calls would have left it.  draws=None (the
    torch-call replay, which consumes the global generator): every item goes to ONE worker with rng_state=None.
    prefetch=False: no thread at all; next() calls prepare(item, None, None) on the caller's thread.

    Protocol: bounded queues (input 8, output max(2 * resident // W, 4), `resident` being the pairs the consumer holds on the
    device); None ends a queue; an exception raised in a thread travels down the output queues as an item and is raised by
    next(); `stop` makes every bounded put give up, so no thread stays blocked once the consumer has failed."""

    def __init__(self, items, prepare, workers=3, resident=2, draws=None, prefetch=True):
        self.items, self.prepare, self.draws = items, prepare, draws
        self.W = max(1, int(workers)) if draws is not None else 1
        self.cursor = 0                                          # index of the next item to hand out
        self.stop = threading.Event()
        self.threads, self.in_q, self.out_q = [], [], []
        if prefetch:
            self.in_q = [queue.Queue(maxsize=8) for _ in range(self.W)]
            self.out_q = [queue.Queue(maxsize=max(2 * resident // self.W, 4)) for _ in range(self.W)]
            self.threads = [threading.Thread(target=self._feed, daemon=True)]
            self.threads += [threading.Thread(target=self._work, args=(w,), daemon=True) for w in range(self.W)]
            for th in self.threads:
                th.start()

    def _put(self, q, item):
        """Bounded put that gives up when the consumer has failed (so a thread never stays blocked)."""
        while not self.stop.is_set():
            try:
                q.put(item, timeout=0.1)
                return True
            except queue.Full:
                pass
        return False

    def _feed(self):
        """Hands item i to worker i % W, with the generator state it starts from (draws given: walks the generator over all items)."""
        try:
            st = torch.get_rng_state() if self.draws is not None else None
            for i, item in enumerate(self.items):
                if self.stop.is_set():
                    return
                if not self._put(self.in_q[i % self.W], (i, item, None if st is None else st.clone())):
                    return
                if st is not None and N.host_lib().ndp_rng_skip(ctypes.c_void_p(st.data_ptr()), st.numel(), self.draws(item)) != 0:
                    raise N.NdpError("ndp_rng_skip failed")
            if st is not None:
                torch.set_rng_state(st)                          # where sequential register() calls would have left it
            for q in self.in_q:
                self._put(q, None)
        except BaseException as e:                               # surface the failure in the consumer
            for q in self.out_q:
                self._put(q, e)

    def _work(self, w):
        try:
            while not self.stop.is_set():
                try:
                    task = self.in_q[w].get(timeout=0.1)
                except queue.Empty:
                    continue
                if task is None:
                    self._put(self.out_q[w], None)
                    return
                i, item, st = task
                if not self._put(self.out_q[w], (i, self.prepare(item, st, w))):
                    return
        except BaseException as e:
            self._put(self.out_q[w], e)

    def next(self, block=True):
        """(i, prepared) of the next item in index order, None after the last one; block=False: _NOT_READY when its worker has
        not delivered it yet.  Raises what a producer thread raised."""
        i = self.cursor
        if i >= len(self.items):
            return None
        if not self.threads:
            item = (i, self.prepare(self.items[i], None, None))
        else:
            try:
                item = self.out_q[i % self.W].get(block=block)
            except queue.Empty:
                return _NOT_READY
        if item is None:
            return None
        if isinstance(item, BaseException):
            raise item
        self.cursor = i + 1
        return item

    def close(self, failed=False):
        """Joins the threads.  failed=True (the consumer gave up): they must not stay blocked on a bounded queue, holding what
        they prepared -- stop them and drain what they queued first."""
        if failed:
            self.stop.set()
            for q in self.out_q + self.in_q:
                while True:
                    try:
                        q.get_nowait()
                    except queue.Empty:
                        break
        for th in self.threads:
            th.join()


class _Prepared:
    """Everything one pair needs on the device before it enters an engine slot: the raw clouds, their means, the
    freshly initialised pyramid and the sampling permutations (one pinned upload), optional landmarks."""
    __slots__ = ("src_pcd", "tgt_pcd", "means", "buf", "store", "perm_s", "perm_t", "K", "S", "T", "ldmk_s", "ldmk_t",
                 "desc", "result", "state", "index")

    def tensors(self):
        return [t for t in (self.src_pcd, self.tgt_pcd, self.means, self.buf, self.ldmk_s, self.ldmk_t) if t is not None]

    def load_job(self, slot):
        return dict(slot=slot, params=self.store, K=self.K, S=self.S, T=self.T, src=self.src_pcd, tgt=self.tgt_pcd,
                    perm_s=self.perm_s, perm_t=self.perm_t, ldmk_s=self.ldmk_s, ldmk_t=self.ldmk_t, means=self.means,
                    n_src=self.src_pcd.shape[0], n_tgt=self.tgt_pcd.shape[0])     # (the means are computed by the load call)

    def warp_job(self, store):
        return (store, self.src_pcd, self.means, self.means[4:])

    def release(self):
        """Drop the device staging once the final warp has been enqueued (the allocator keeps the memory alive for
        the streams the tensors were recorded on)."""
        self.buf = self.store = self.perm_s = self.perm_t = self.tgt_pcd = self.ldmk_s = self.ldmk_t = None
        self.src_pcd = self.means = None             # (the warp job that read them is enqueued; a per-pair device copy of the source
                                                     #  and a 512-byte allocation per pair otherwise live until the batch call returns)


class _PinRing:
    """Pinned float32 staging buffers of ONE preparing thread, reused once their upload has completed (allocated once:
    hipHostMalloc costs milliseconds), plus that thread's integer scratch for the permutation replay."""

    def __init__(self):
        self.free, self.busy, self._scratch = [], [], None

    def take(self, numel):
        while self.busy and self.busy[0][1].query():
            self.free.append(self.busy.pop(0)[0])
        for i, buf in enumerate(self.free):
            if buf.numel() == numel:
                return self.free.pop(i)
        if len(self.busy) >= 64:                                                    # bound the ring: wait for the oldest
            host, ev = self.busy.pop(0)
            ev.synchronize()
            if host.numel() == numel:
                return host
        return torch.empty(numel, dtype=torch.float32).pin_memory()

    def uploaded(self, host, stream):
        ev = torch.cuda.Event()
        ev.record(stream)
        self.busy.append((host, ev))

    def scratch(self, n):
        if self._scratch is None or self._scratch.numel() < n:
            self._scratch = torch.empty(max(n, 8192), dtype=torch.int32)
        return self._scratch


class _BatchCtx:
    """What the lanes of one register_batch call share.  producer: delivers (i, (prepared pair, event recorded behind its
    preparation or None)) in index order; main / fin_stream: the caller's stream and the stream of the final all-point warps."""
    __slots__ = ("reg", "producer", "sink", "chunk", "m", "main", "fin_stream", "total_slots", "preps", "states", "held",
                 "exhausted", "handed_out", "fin_batches")

    def __init__(self, reg, producer, n_pairs, sink, chunk, m, main, fin_stream, total_slots):
        self.reg, self.producer, self.sink, self.chunk, self.m = reg, producer, sink, chunk, m
        self.main, self.fin_stream, self.total_slots = main, fin_stream, total_slots   # total_slots: slots of all lanes
        self.preps = [None] * n_pairs                     # the pairs handed to lanes, by index
        self.states = [None] * n_pairs                    # final pair states by index (register_batch -> last_states)
        self.held = None                                  # the first delivery, held back for lane 0 (see first())
        self.exhausted = False
        self.handed_out = 0                               # pairs given to lanes so far
        self.fin_batches = 0                              # final-warp batches handed to the sink so far

    def first(self):
        """The first pair, whose shapes size the engines.  It stays with the context and goes to the first lane that asks,
        through next_pair() like every other pair."""
        self.held = self.producer.next()
        return self.held[1][0]

    def next_pair(self, stream, block=True):
        """Next pair (in index order) made visible to `stream` (a lane's stream) and to fin_stream.
        block=False: _NOT_READY when its worker has not finished it yet."""
        item, self.held = self.held, None
        if item is None:
            item = self.producer.next(block)
        if item is None or item is _NOT_READY:
            return item
        i, (p, ev) = item
        if ev is not None:
            stream.wait_event(ev)
            self.fin_stream.wait_event(ev)
        for t in p.tensors():                                # allocated on the producer's stream, consumed on these two
            t.record_stream(stream)
            t.record_stream(self.fin_stream)
        self.preps[i] = p
        p.index = i
        return i, p


class _Lane:
    """One engine on one stream.  Pipelined control: the states of chunk k are read back while chunk k+1
    runs, so the GPU never waits for the host; a slot that finishes in chunk k is refilled before chunk k+2.
    Refills of one round go up in ONE launch (k_eng_load), the final all-point warps of the pairs that
    finished in one chunk in ONE launch (k_pyramid_fwd) on the shared side stream."""

    def __init__(self, ctx, eng, stream):
        self.ctx, self.eng, self.stream = ctx, eng, stream
        self.fin_done = {}                               # slot -> event: its parameters have been consumed
        self.active, self.free = {}, list(range(eng.B))  # active: slot -> (pair index, first valid snapshot)
        self.seq, self.pending, self.done = 0, None, False

    def step(self):
        ctx, eng = self.ctx, self.eng
        jobs = []
        # Refill policy.  While the batch ramps up (fewer pairs handed out than there are slots) a lane takes what the producer
        # has ready and ticks: filling every slot first kept the GPU idle for slots x 0.45 ms at the start of each batch, lane
        # after lane.  After that it waits for the producer: in a GPU-bound run the queue is never empty, and in a producer-bound
        # one (the landmark config) ticking half-empty engines only costs launches that slow the producer down (measured both ways).
        # It never waits for more than `quota` pairs per step, so the pairs already resident keep ticking.
        ramp = ctx.handed_out < ctx.total_slots
        quota = max(4, eng.B // 16)
        while self.free and not ctx.exhausted and (ramp or len(jobs) < quota):
            idle = not self.active and self.pending is None and not jobs
            nxt = ctx.next_pair(self.stream, block=idle or not ramp)
            if nxt is None:
                ctx.exhausted = True
                break
            if nxt is _NOT_READY:
                break
            ctx.handed_out += 1
            i, p = nxt
            slot = self.free.pop()
            if slot in self.fin_done:
                self.stream.wait_event(self.fin_done.pop(slot))   # the previous tenant's parameters have been copied out for its final warp
            jobs.append(p.load_job(slot))
            self.active[slot] = (i, self.seq)            # snapshots >= seq see this pair in the slot
        if jobs:
            eng.load_jobs(jobs)
        if not self.active and self.pending is None:
            self.done = True
            return
        handle = None
        if self.active:
            eng.run_ticks(ctx.chunk)
            handle = (eng.snapshot_async(), self.seq)
            self.seq += 1
        if self.pending is not None:
            (h, hseq) = self.pending
            snap = eng.wait_snapshot(h)
            done = []
            for slot in np.nonzero(snap.level >= ctx.m)[0].tolist():   # finished (or parked) slots only
                if slot not in self.active:
                    continue
                i, valid_from = self.active[slot]
                if hseq < valid_from:
                    continue
                st = snap.state(slot)
                del self.active[slot]
                ctx.preps[i].state = st
                ctx.states[i] = st
                done.append((slot, ctx.preps[i]))
                self.free.append(slot)
            if done:
                # the snapshot proves every tick that touched these slots has completed: the final warp
                # needs no dependency on the lane's stream, only the slots' refill must wait for it
                with torch.cuda.stream(ctx.fin_stream):
                    ev = torch.cuda.Event()
                    outs = ctx.reg._finish(eng, done, freeze=True, frozen=lambda: ev.record(ctx.fin_stream))
                for (slot, p), out in zip(done, outs):
                    self.fin_done[slot] = ev
                    out.record_stream(ctx.main)
                    p.result = out
                    p.release()
                if ctx.sink is not None:
                    with torch.cuda.stream(ctx.fin_stream):           # whatever the sink enqueues is ordered behind the final warp that
                        for slot, p in done:                          # produced `warped` (it is NOT complete on the lane's stream)
                            ctx.sink(p.index, p.result, p.state)
                            p.result = None
                            ctx.preps[p.index] = None                 # a long stream holds the resident pairs only (its states: ctx.states)
                    # nobody waits on the final-warp stream in a sink stream (the sink's work is ordered on it): like the producers'
                    # side streams it is synchronised now and then, or the HIP runtime's per-command state of it grows with the stream
                    ctx.fin_batches += 1
                    if ctx.fin_batches % 64 == 0:
                        ctx.fin_stream.synchronize()
        self.pending = handle
