"""What WalkController.step_pipelined() runs on: the pair of HIP streams for tick and sim (StreamTable) and the ring of
snapshot slots the tick hands the TSID state to the sim stages through (SimPipeline).  Neither keeps a reference to the
controller: it passes its call path (`call` = WalkController._call) and its sim launch (`launch` = _sim_batch) in."""
import ctypes as C
import os
import sys
import time
import warnings

import torch

from . import _lib


def streams_overlap(device, sa, sb):
    """True if work on the two streams really runs concurrently.  HIP multiplexes its streams onto a few hardware queues
    (GPU_MAX_HW_QUEUES, 4 by default) and two streams - even two created one after the other - can share one, in which
    case tick and sim run one after the other and the pipelined step loses its overlap without any error
    (tools/stream_overlap_probe.py).  Probe: a short device-side spin on each, timed together against one alone."""
    if os.environ.get("TSIDB_NO_STREAM_PROBE") == "1" or not hasattr(torch.cuda, "_sleep") or torch.cuda.is_current_stream_capturing():
        return True
    try:
        def spin(streams, cycles=600000):   # ~0.25 ms at 2.4 GHz
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for st in streams:
                with torch.cuda.stream(st):
                    torch.cuda._sleep(cycles)
            for st in streams:
                st.synchronize()
            return time.perf_counter() - t0
        spin([sa, sb], 1000)                 # (first use of the kernel on these streams)
        one = min(spin([sa]), spin([sb]))
        both = min(spin([sa, sb]), spin([sa, sb]))
        return both < 1.6 * one
    except Exception:
        return True


def overlapping_stream(device, other, tries=6):
    """(stream, found): an ordinary stream from torch's pool that runs concurrently with `other` (one that shares its
    hardware queue would serialise tick and sim); after `tries` candidates the last one, and found = False"""
    for _ in range(tries):
        st = torch.cuda.Stream(device=device)
        if streams_overlap(device, other, st):
            return st, True
    return st, False


class StreamTable:
    """The streams the library recommends for the tick (_lib.ROLE_TICK) and the sim (_lib.ROLE_SIM) of the pipelined step
    (tsidb_stream_create): on disjoint halves of the CUs for up to 512 envs (include/tsidb.h), plain streams above.  Made on
    first use, both at once; owns the HIP streams behind the library's pair until close()."""

    def __init__(self, device):
        self.device = device
        self.streams = []     # [tick, sim]: ExternalStream wrappers of the library's streams, or two of torch's pool
        self.raw = []         # the library's stream handles behind them (none behind torch's): close() destroys them

    def get(self, role, call):
        if not self.streams:
            split = C.c_int(0)
            call("tsidb_get_option", _lib.OPT_CU_SPLIT, C.byref(split))
            if split.value:
                self.raw = [C.c_void_p(), C.c_void_p()]
                for r, hs in enumerate(self.raw):     # (r = ROLE_TICK, ROLE_SIM)
                    call("tsidb_stream_create", r, C.byref(hs))
                self.streams = [torch.cuda.ExternalStream(hs.value, device=self.device) for hs in self.raw]
                if not streams_overlap(self.device, *self.streams):
                    # the CU-masked pair does not overlap: give up the split for BOTH roles (a tick confined to half the CUs
                    # beside a sim that spans all of them is a silent regression) and say so
                    warnings.warn("tsid_control_amd: the CU-masked tick / sim streams do not run concurrently on this device; "
                                  "using ordinary streams for both (no CU split)")
                    self.close(call)
            if not self.streams:                      # no CU split for this batch size: torch's pool
                tick = torch.cuda.Stream(device=self.device)
                sim, found = overlapping_stream(self.device, tick)
                if not found:
                    warnings.warn("tsid_control_amd: no pair of HIP streams that runs concurrently was found (they share a hardware "
                                  "queue): the pipelined step will run tick and sim one after the other")
                self.streams = [tick, sim]
        return self.streams[role]

    def sim_stream_for(self, cur):
        """The sim stream of a pipelined loop that runs on `cur`: the library's (on the other half of the CUs for up to 512
        envs) when that is the tick stream, an ordinary one otherwise - a CU-masked stream is a BLOCKING stream
        (hipExtStreamCreateWithCUMask takes no flags): beside work on the legacy default stream it would serialise with it."""
        if self.streams and cur.cuda_stream == self.streams[_lib.ROLE_TICK].cuda_stream:
            return self.streams[_lib.ROLE_SIM]
        return overlapping_stream(self.device, cur)[0]

    def close(self, call):
        """Destroy the library streams nobody outside this table still holds the wrapper of.  A caller (or a captured
        graph's keep list) may hold the ExternalStream of one: that HIP stream is left alive (a leaked stream is harmless,
        a dangling one is not).  The owner drops its SimPipeline first; the three references that remain are then all
        ours: self.streams, the variable `ext` and getrefcount's argument (no zip(): it would keep a fourth)."""
        for i, hs in enumerate(self.raw):
            ext = self.streams[i]
            if sys.getrefcount(ext) <= 3:
                call("tsidb_stream_destroy", hs)
        self.streams, self.raw = [], []


class SimPipeline:
    """The sim side of step_pipelined(): the second stream and a ring of K snapshot slots.  A tick writes the TSID state it
    ends on into the next slot (next_slot); the sim stages of the pending slots are enqueued on the sim stream several at a
    time (flush) and leave one event per batch.  The tick writes its slot itself, so it must wait for the sim that read the
    slot K steps ago BEFORE it starts - with only two slots that wait held tick(t) back until sim(t - 2) was done and cost
    12 % at 4096 envs; four slots and the tick stream runs ahead as before.  Never fewer than two batches of slots: a tick
    must not overwrite a snapshot whose sim is still pending; the library numbers slots 0 .. 15."""

    def __init__(self, stream, q, v, slots):
        self.stream = stream                                   # the sim stream
        self.qring = torch.empty(slots, *q.shape, dtype=q.dtype, device=q.device)   # one allocation: a batch of sim
        self.vring = torch.empty(slots, *v.shape, dtype=v.dtype, device=v.device)   # stages names its slots by number
        self.q, self.v = list(self.qring.unbind(0)), list(self.vring.unbind(0))     # the slots
        self.pending = []                                      # slots a tick has written and no sim stage has been enqueued for
        self.forget_events()

    def __getitem__(self, name):   # bench.py reads wc._pipe["stream"]
        return getattr(self, name)

    def forget_events(self):
        """Start over at slot 0 with nothing to wait for: no event from outside a graph capture may be waited on inside
        it, and none from inside it afterwards."""
        self.par = 0                            # the slot the next tick writes
        self.done = [None] * len(self.q)        # per slot: the event of the sim batch that read it last
        self.last_wait = None                   # (stream, event) of the last cross-stream wait: not issued twice

    def next_slot(self, cur):
        """The slot for the next tick on stream `cur`, which is made to wait for the sim batch that read it a ring ago."""
        par = self.par
        self.par = (par + 1) % len(self.q)
        ev = self.done[par]
        if ev is not None and self.last_wait != (cur.cuda_stream, ev):
            # (once per batch: the slots of one batch share its event, and a cross-stream wait is a barrier packet that costs
            #  the tick stream ~10 us each - at 512 envs a fifth of the step when it was issued before every tick)
            if torch.cuda.is_current_stream_capturing() or not ev.query():   # (already complete: no packet)
                cur.wait_event(ev)
            self.last_wait = (cur.cuda_stream, ev)   # (the reference keeps the event alive: no id reuse)
        return par

    def flush(self, cur, launch, events=None):
        """Enqueue the sim stages of the pending slots (oldest first) behind what `cur` holds now: launch(slots) runs on
        the sim stream.  events[2], events[3] bracket the last sim step alone."""
        if not self.pending:
            return
        ready = cur.record_event()
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            pend = list(self.pending)
            if events:
                head, pend = pend[:-1], pend[-1:]
                if head:
                    launch(head)
                events[2].record(self.stream)
            launch(pend)
            if events:
                events[3].record(self.stream)
            done = self.stream.record_event()
        for slot in self.pending:
            self.done[slot] = done
        self.pending = []

    def join(self, cur, launch):
        """Enqueue what is pending and make `cur` wait for the sim stream."""
        self.flush(cur, launch)
        cur.wait_stream(self.stream)
