"""Host-fed inference without a host synchronisation per frame.

The reference's evaluation loop (tools/test.py:121-146, det3d/torchie/apis/train_sessd.py:88-106) takes a batch from the
DataLoader, `example_to_device`s it, runs the model and moves the detections back -- three host round trips per frame. Here the
same contract (host point clouds in, host detections out, submission order) is a three-stage pipeline:

  H2D           : pinned host points --> a device staging ring. Round 5: enqueued ON THE ENGINE'S OWN STREAM, in front of the
                  frame (copy_mode="instream"); rounds 2 - 4 used one copy stream and an event per frame the engine's stream
                  waited for (copy_mode="copystream"). Measured (scripts/hostio_probe.py, four engines on two CU-masked halves):
                  device-resident points 1942 frames/s, in-stream H2D 1909, copy stream + event 1286 (one copy stream per
                  engine 1259, copies issued a round ahead 1307): the cross-stream wait, not the copy, costs the device a
                  third of its rate -- with several frames in flight another engine's kernels cover a copy that sits in
                  stream order anyway
  engine streams: frames alternate between independent batch-1 engines (like bench.py's timed region); an engine stages the
                  points into its static input buffer and replays its captured graph; the frame appends its detections to the
                  engine's device record ring by itself
  fetch         : every `fetch_every` frames of an engine the filled part of its record ring goes D2H into pinned memory
                  (asynchronously, on that engine's stream); the host only ever waits for the fetch BEFORE the newest one,
                  which is also what bounds how far it can run ahead of the device.
"""
import numpy as np
import torch

from ._lib import check, lib


def engines_on_cu_sets(model, voxel_range, voxel_size, max_points_per_voxel, max_voxels, test_cfg, n_engines=4, sets=2, device=None,
                       tune_points=None, layout="contiguous", capture=True, records=0, **engine_kwargs):
    """The throughput configuration of round 5 as one call: `n_engines` batch-1 InferenceEngines, engine i on a stream of its own
    that is confined to CU set i % `sets` (ops.cu_masked_stream: hipExtStreamCreateWithCUMask -- a hardware queue per engine, its
    kernels on its set's compute units only), persistent stream-K launches sized for the set (engine.cu_budget). tune_points: a
    representative (P, 4) float32 device cloud -- engine 0 is autotuned on it ON ITS CU SET, the others adopt the tuning, and the
    Winograd list layers run on whole-unit shares (engines that share a set leave each other CUs that way); without it every
    engine takes engine.force_active_tiles(). capture: capture every engine's graph on its stream; records > 0: attach a device
    detection ring of that many frames first (HostFedPipeline does that itself). Returns (engines, streams).
    Measured on MI355X (profiles/r5_cu_sets_sweep.json): 4 engines on 2 sets 1950 frames/s against 1557 for two plain streams; `sets`
    must divide the chip's 8 XCDs evenly (2 or 4)."""
    import torch
    from . import ops
    from .engine import InferenceEngine
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    engines, streams = [], []
    for k in range(int(n_engines)):
        st, ncu = ops.cu_masked_stream(k % int(sets), int(sets), dev, layout=layout)
        e = InferenceEngine(model, voxel_range, voxel_size, max_points_per_voxel, max_voxels, test_cfg, 1, device=dev, **engine_kwargs)
        e.cu_budget = ncu
        engines.append(e)
        streams.append(st)
    e0 = engines[0]
    with torch.cuda.stream(streams[0]):
        if tune_points is not None:
            e0.set_points([tune_points])
            e0.enqueue()
            streams[0].synchronize()
            e0.list_share_candidates = (-1,)   # shapes are chosen among whole-unit launches: the share rule engines on a shared set run
            e0.autotune()
            e0.set_list_shares("whole")
        else:
            e0.force_active_tiles()
            e0.set_list_shares("whole")
    streams[0].synchronize()
    for e in engines[1:]:
        if tune_points is not None:
            e.adopt_tuning(e0)
        else:
            e.force_active_tiles()
            e.set_list_shares("whole")
    for e, st in zip(engines, streams):
        if records:
            e.attach_records(int(records))
        if capture:
            with torch.cuda.stream(st):
                if tune_points is not None:
                    e.set_points([tune_points])   # (the capture's warm-up frames run on a real cloud)
                e.capture()
    torch.cuda.synchronize(dev)
    return engines, streams


def pillar_engines_on_cu_sets(model, voxel_generator_cfg, test_cfg, n_engines=4, sets=2, device=None, layout="contiguous", capture=True,
                              records=0, **engine_kwargs):
    """engines_on_cu_sets for the PointPillars config: `n_engines` batch-1 PillarEngines, engine i on a stream of its own that is
    confined to CU set i % `sets` (ops.cu_masked_stream), cu_budget set to the set's size. There is nothing to tune (the engine has
    no tile lists and no autotuned layers). records > 0: a device detection ring of that many frames is attached first
    (HostFedPipeline attaches its own to engines that are not captured yet); capture: every engine's graph is captured on its
    stream. engine_kwargs go to PillarEngine (max_points, anchors, front_end). Returns (engines, streams); HostFedPipeline takes
    them as they are. `sets` must divide the chip's 8 XCDs evenly (2 or 4)."""
    from . import ops
    from .pillar_engine import PillarEngine
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    engines, streams = [], []
    for k in range(int(n_engines)):
        st, ncu = ops.cu_masked_stream(k % int(sets), int(sets), dev, layout=layout)
        e = PillarEngine(model, voxel_generator_cfg, test_cfg, 1, device=dev, **engine_kwargs)
        e.cu_budget = ncu
        engines.append(e)
        streams.append(st)
    for e, st in zip(engines, streams):
        if records:
            e.attach_records(int(records))
        if capture:
            with torch.cuda.stream(st):
                e.capture()
    torch.cuda.synchronize(dev)
    return engines, streams


class HostFedPipeline:
    def __init__(self, engines, streams=None, ring=4, fetch_every=16, eager=False, copy_mode="instream"):
        """engines: batch-1 InferenceEngines of ONE configuration (captured unless eager=True). ring: staging buffers per
        engine (frames the H2D copies may run ahead). fetch_every: frames of an engine between two D2H record fetches."""
        assert all(e.B == 1 for e in engines), "the pipeline feeds batch-1 engines"
        self.engines = list(engines)
        self.dev = self.engines[0].dev
        self.streams = list(streams) if streams is not None else [torch.cuda.Stream(self.dev) for _ in self.engines]
        self.copy_stream = torch.cuda.Stream(self.dev)
        self.ring, self.fetch_every, self.eager = int(ring), int(fetch_every), bool(eager)
        assert copy_mode in ("instream", "copystream")
        self.copy_mode = copy_mode
        self.post_max = self.engines[0].post_max * self.engines[0].num_tasks   # rows of a frame's record (every task keeps post_max)
        cap = 2 * self.fetch_every
        self._st = []
        for e in self.engines:
            if e.records is None or e.records.shape[0] != cap:
                if e.graph is not None:
                    raise RuntimeError("attach_records(%d) must precede capture(): the ring's address is baked into the graph" % cap)
                e.attach_records(cap)
            P = e.P_cap
            self._st.append(dict(
                stage=[torch.empty((P, 4), dtype=torch.float32, device=self.dev) for _ in range(self.ring)],
                pinned=[torch.empty((P, 4), dtype=torch.float32).pin_memory() for _ in range(self.ring)],
                h2d=[None] * self.ring, consumed=[None] * self.ring, submitted=0, fetched=0,
                host_rec=[torch.empty((self.fetch_every, self.post_max, 9), dtype=torch.float32).pin_memory() for _ in range(2)],
                host_cnt=[torch.empty((self.fetch_every,), dtype=torch.int32).pin_memory() for _ in range(2)],
                host_err=[torch.zeros((1,), dtype=torch.int32).pin_memory() for _ in range(2)],
                pending=[]))  # (event, buffer index, first frame of the engine, number of frames)
        self._n = 0
        self._out = {}
        self._next_out = 0
        self._base = 0      # frames submitted before the last restart (submit() returns job-global indices)
        self._idle = True   # nothing in flight: the next submit() checks the device cursors against the host's ring state
        self.nms_truncated = False   # set by finish(): the engines' sticky DI-NMS capacity flag

    def reset(self):
        """Start a new job: zero the device cursors and the sticky overflow flags (the engines must be idle). MANDATORY after
        InferenceEngine.capture() or any eager use of the engines (both advance the device cursor the host ring arithmetic
        mirrors); submit() does it by itself when it finds the pipeline idle with a cursor that is not where it left it."""
        for e, st in zip(self.engines, self._st):
            e.record_cursor.zero_()
            e.err.zero_()
            e.nms_truncated.zero_()
            st.update(submitted=0, fetched=0, pending=[], h2d=[None] * self.ring, consumed=[None] * self.ring)
        self._n, self._out, self._next_out = 0, {}, 0
        self._idle, self._base = False, 0
        torch.cuda.synchronize(self.dev)

    def _sync_cursors(self):
        """First submit() of a job (after construction, capture(), eager use of the engines, or finish()): the host ring
        arithmetic (slot = frames of this engine so far % capacity) assumes the device cursor equals the number of frames this
        pipeline submitted to the engine. capture() runs warm-up enqueues that advance the cursor, and finish() may leave
        `fetched` off a multiple of fetch_every -- so an idle pipeline restarts from a clean state instead of silently reading
        other frames' slots (round-3 advisor finding)."""
        self._idle = False
        dirty = any(int(e.record_cursor.item()) != st["submitted"] or st["fetched"] % self.fetch_every
                    for e, st in zip(self.engines, self._st))
        if dirty:
            assert not self._out, "finish() drains every frame before the pipeline goes idle"
            base = self._base + self._n   # submit() keeps returning job-global indices across the restart
            self.reset()
            self._base = base

    # ------------------------------------------------------------------
    def submit(self, points):
        """points: (P,4) float32 host array / CPU tensor (pinned memory is used in place, anything else goes through the
        pipeline's own pinned ring). Returns the frame's index; never blocks on the frame itself."""
        if self._n == 0 or self._idle:
            self._sync_cursors()
        i = self._n
        ei = i % len(self.engines)
        e, st, stream = self.engines[ei], self._st[ei], self.streams[ei]
        k = st["submitted"] % self.ring
        src = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points, np.float32))
        n = int(src.shape[0])
        if n > e.P_cap:
            raise ValueError("frame has %d points, engine capacity is %d" % (n, e.P_cap))
        if st["consumed"][k] is not None:
            # slot k was last used `ring` frames of this engine ago: its staging copy must have been read, and (when the source is
            # our own pinned buffer) its H2D must have left the host buffer
            if not src.is_pinned():
                st["h2d"][k].synchronize()
        if not src.is_pinned():
            st["pinned"][k][:n].copy_(src)
            src = st["pinned"][k][:n]
        dst = st["stage"][k][:n]
        if self.copy_mode == "copystream":
            with torch.cuda.stream(self.copy_stream):
                if st["consumed"][k] is not None:
                    self.copy_stream.wait_event(st["consumed"][k])
                dst.copy_(src, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.copy_stream)
                st["h2d"][k] = ev
        with torch.cuda.stream(stream):
            if self.copy_mode == "copystream":
                stream.wait_event(ev)
            else:
                # in stream order: the slot's previous reader (set_points of `ring` frames ago) is older than this copy
                dst.copy_(src, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(stream)
                st["h2d"][k] = ev
            e.set_points([dst])
            done = torch.cuda.Event()
            done.record(stream)
            st["consumed"][k] = done
            if self.eager:
                e.enqueue()
            else:
                e.replay()
            st["submitted"] += 1
            if st["submitted"] - st["fetched"] == self.fetch_every:
                self._fetch(ei)
        self._n += 1
        return self._base + i

    def _fetch(self, ei):
        """D2H of the frames of engine ei that are on its ring and not yet fetched (on its stream, asynchronous)."""
        e, st, stream = self.engines[ei], self._st[ei], self.streams[ei]
        lo, hi = st["fetched"], st["submitted"]
        if hi == lo:
            return
        # at most one fetch stays un-collected: collecting the older one frees its pinned buffer and throttles the host
        while len(st["pending"]) > 1:
            self._collect(ei)
        buf = (lo // self.fetch_every) & 1
        cap = e.records.shape[0]
        s0 = lo % cap
        cnt = hi - lo
        assert s0 + cnt <= cap and cnt <= self.fetch_every
        with torch.cuda.stream(stream):
            st["host_rec"][buf][:cnt].copy_(e.records[s0:s0 + cnt], non_blocking=True)
            st["host_cnt"][buf][:cnt].copy_(e.record_counts[s0:s0 + cnt], non_blocking=True)
            st["host_err"][buf].copy_(e.err, non_blocking=True)  # the STICKY overflow flag as of the newest fetched frame
            ev = torch.cuda.Event()
            ev.record(stream)
        st["pending"].append((ev, buf, lo, cnt))
        st["fetched"] = hi

    def _collect(self, ei):
        st = self._st[ei]
        ev, buf, lo, cnt = st["pending"].pop(0)
        ev.synchronize()
        if int(st["host_err"][buf][0]) != 0:
            # a sparse level overflowed in one of the frames up to this fetch: their rows were dropped, the detections are not
            # to be handed out. The flag is sticky on the device; clear it so that a new job can start after reset().
            self.engines[ei].err.zero_()
            raise RuntimeError(getattr(self.engines[ei], "err_text",
                                       "sparse level capacity overflow in a frame of engine %d up to its frame %d (job frames <= %d): "
                                       "raise `growth` or max_voxels" % (ei, lo + cnt - 1, self._base + (lo + cnt - 1) * len(self.engines) + ei)))
        rec, c = st["host_rec"][buf].numpy(), st["host_cnt"][buf].numpy()
        E = len(self.engines)
        for j in range(cnt):
            n = int(c[j])
            a = rec[j, :n].copy()
            self._out[(lo + j) * E + ei] = dict(box3d_lidar=a[:, :7], scores=a[:, 7], label_preds=a[:, 8].astype(np.int64))

    def poll(self):
        """Detections that are complete on the host, in submission order (possibly empty). Does not block."""
        for ei, st in enumerate(self._st):
            while st["pending"] and st["pending"][0][0].query():
                self._collect(ei)
        return self._drain()

    def _drain(self):
        out = []
        while self._next_out in self._out:
            out.append(self._out.pop(self._next_out))
            self._next_out += 1
        return out

    def finish(self):
        """Flush: fetch what is still on the device rings, wait, return the remaining detections in submission order."""
        for ei in range(len(self.engines)):
            self._fetch(ei)
        for ei, st in enumerate(self._st):
            while st["pending"]:
                self._collect(ei)
        for e in self.engines:
            if int(e.err.item()) != 0:  # (every fetch carries the flag; this is the belt to those braces)
                e.err.zero_()
                raise RuntimeError(getattr(e, "err_text", "sparse level capacity overflow: raise `growth` or max_voxels"))
        # DI-NMS engines (test_cfg nms_type "rotate_weighted_nms"): did any frame of the job stop its selection at post_max with
        # candidates left? Reported, never raised (the detections are the reference's keep list cut at post_max)
        self.nms_truncated = any(int(e.nms_truncated.item()) != 0 for e in self.engines)
        self._idle = True
        return self._drain()
