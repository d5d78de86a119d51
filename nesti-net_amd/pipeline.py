"""End-to-end hot path for one shape: cloud (host or device) -> multi-scale patches (HIP ball
query) -> MuPS -> gating -> top-1 expert -> normals.  This is the body of the reference's
``predict`` loop (``test_n_est_w_experts.py:129-152``) with the per-point Python
``__getitem__`` and the TF ``sess.run`` replaced by three library calls per batch."""
import ctypes

import numpy as np
import torch

from . import _lib
from .config import ARCH_MULTI, ARCH_SINGLE, NestiConfig
from .model import NestiNet
from .provider import CloudPatches


def verified_passes(est, run_once, reduce=None):
    """The loop of the reproducible mode's verified run (:meth:`NormalEstimator.run_verified`; ``dist.estimate_sharded`` passes an
    all-reduce as ``reduce``).  ``run_once()`` runs the WHOLE query set frozen; ``est.verify_flags()`` then returns the 4-float
    tensor [max_margin_err, max_dn, violations > 0, dropped > 0] of that pass, ``reduce`` folds the other ranks' in (MAX), and
    every rank takes the same decision from the same four numbers: done, or raise the thresholds to 1.5 x the maxima and run
    everything again -- at most ``1 + NESTI_GATE_WIDEN_PASSES`` passes.  The maxima of a pass are taken over a set of rows fixed by
    (thresholds, query set), so the thresholds of the next pass, and with them the result, are a function of (model, calibrated
    tau / thr, cloud, query set).  The calibrated thresholds are restored on the way out, also on error."""
    saved = est.verify_begin()
    try:
        for passes in range(1, 2 + _lib.GATE_WIDEN_PASSES):
            res = run_once()
            flags = est.verify_flags()
            if reduce is not None:
                reduce(flags)
            err, dn, violated, dropped = (float(v) for v in flags.tolist())
            if dropped > 0:
                raise _lib.NestiError("reproducible run: flagged outputs did not fit the conditioning guard's lists (guard_dropped > 0): "
                                      "the guard threshold is absurd for this shape, or the library batch too small for it")
            if not violated > 0:
                est.verify_record(passes, err, dn)
                return res
            est.verify_raise(err, dn)
        raise _lib.NestiError("reproducible run: the measured errors still exceed the thresholds after %d passes "
                              "(max_margin_err %.4g, max_dn %.4g)" % (passes, err, dn))
    finally:
        est.verify_end(saved)


class NormalEstimator:
    """``use_graph=True`` captures the forward pass of a full batch (MuPS + gate + routing + experts,
    ~250 launches whose sizes depend only on the batch size -- expert counts are read on the device) into a
    hipGraph once and replays it; only worthwhile for small batches where launch gaps matter.

    ``reproducible=True`` (``nesti_model_set_reproducible``): the gate margin and the conditioning guard's threshold are frozen, so
    ``run`` / ``run_many`` / ``estimate`` give results that do not depend on ``batch``, ``n_streams``, ``use_graph`` or on what the
    estimator ran before; :meth:`run_verified` adds the check that the default mode performs on the device."""

    def __init__(self, cfg: NestiConfig, weights, dtype="bf16", device="cuda:0", batch=4096, seed=3627473,
                 use_graph=False, n_streams=1, gate_margin=None, subsample="hash", x8_layers=None, x8_format=None,
                 reproducible=False):
        self.cfg, self.device, self.batch, self.seed = cfg, torch.device(device), int(batch), seed
        # subsample='reference': balls larger than P are thinned exactly like the reference does (scipy cKDTree traversal
        # order + ONE numpy RandomState stream over all patches in visiting order, utils/pcpnet_dataset.py:304-321), on the
        # host, ~0.5 ms per patch -- for diffing against a real reference run row by row (refsample.py).  The default 'hash'
        # is the GPU ball query with its order-independent uniform subset.
        # Since round 6 'reference' runs on the GPU: ball sizes from a count pass, the random stream replayed natively on the host
        # from those sizes (csrc/refreplay.cpp, a worker thread), the balls sorted into cKDTree's visiting order by the patch
        # kernel (patches.hip: patches_ref_kernel) -- row for row what 'reference_host' (the scipy + numpy path) produces, at
        # several times its speed.  A shape with a ball too large for the kernel's LDS sort falls back to the host path; both
        # draw from ONE native stream object, so the stream position survives the switch.
        if subsample not in ("hash", "reference", "reference_host"):
            raise ValueError("subsample must be 'hash', 'reference' or 'reference_host'")
        self.subsample = subsample
        self._ref = None
        self._ref_failed = False
        if subsample != "hash":
            from .refsample import ReferencePatchSampler, RefStream
            self._ref_stream = RefStream(seed)
            self._ref = ReferencePatchSampler(seed, stream=self._ref_stream)
        self.use_graph = bool(use_graph)
        # n_streams > 1: consecutive batches alternate between HIP streams (own scratch arena each), so one batch's partially
        # filled last workgroup rounds overlap the other's kernels
        self.n_streams = 1 if (use_graph or self._ref is not None) else max(1, int(n_streams))
        # fused mode (everything but the hipGraph and reference-subsample modes): ONE library call per batch stream
        # (nesti_estimate_normals / _multi: fused ball query + MuPS kernel, gate, routing, experts) on an arena that holds the
        # staging buffers and the forward workspace; with one stream that is one call per run
        self._fused = not self.use_graph and self._ref is None
        self.net = NestiNet(cfg, weights, dtype=dtype, device=device, max_batch=1 if self._fused else self.batch)
        if gate_margin is not None:                       # dtypes 'f16x3c' / 'f16x8c' only (calibrate.calibrate_gate_margin picks one)
            self.net.set_gate_margin(gate_margin)
        if x8_layers is not None:                         # dtypes 'f16x8' / 'f16x8c' only (NestiNet.set_x8_layers; default 0b1111)
            self.net.set_x8_layers(x8_layers)
        if x8_format is not None:                         # ... and in which format (NestiNet.set_x8_format: 6 = block-scaled e2m3, the default; 8 = e4m3)
            self.net.set_x8_format(x8_format)
        self.reproducible = bool(reproducible)
        self._has_guard = dtype in ("f16x8", "f16x8c")
        self.last_verified = None
        if self.reproducible:
            self.net.set_reproducible(True)
        S, P, E = cfg.n_scales, cfg.num_point, max(1, cfg.n_gate_out)
        self._graph = None
        if self._fused:
            nbytes = self.net.lib.nesti_estimate_workspace_bytes(self.net._handle, self.batch)
            self._arena = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            # lanes 1 .. n_streams - 1: (stream, arena); lane 0 is the caller's current stream with self._arena
            self._lanes = [(torch.cuda.Stream(device=self.device), torch.empty(nbytes, dtype=torch.uint8, device=self.device))
                           for _ in range(1, self.n_streams)]
            return
        self._lanes = []
        self._points = torch.empty((self.batch, S * P, 3), dtype=torch.float32, device=self.device)
        self._n_eff = torch.empty((self.batch, S), dtype=torch.int32, device=self.device)
        if self.use_graph:
            self._g_out = (torch.empty((self.batch, 3), dtype=torch.float32, device=self.device),
                           torch.empty((self.batch,), dtype=torch.int32, device=self.device),
                           torch.empty((self.batch, E), dtype=torch.float32, device=self.device))

    def _capture(self):
        """Warm up (sets kernel attributes, fills the workspace pointers) then capture one forward."""
        self._points.zero_()
        self._n_eff.fill_(1)
        with torch.cuda.device(self.device):
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self.net.forward(self._points, self._n_eff, out=self._g_out)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize(self.device)
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self.net.forward(self._points, self._n_eff, out=self._g_out)

    def prepare(self, pts, pidx=None, queries=None):
        """Upload a cloud and build its search grid (replaces ``load_shape``).  ``queries`` [M,3]: estimate at these positions
        instead of at cloud points (``CloudPatches``)."""
        return CloudPatches(pts, self.cfg, device=self.device, seed=self.seed, pidx=pidx, queries=queries)

    def _mask_empty(self, n_eff, normals, expert, probs, single_tower):
        """Position queries on the unfused paths: the sentinel of rows without a neighbourhood (``nesti_mask_empty_queries``), on
        the current stream, after the forward pass that wrote the rows (never inside the captured graph)."""
        with torch.cuda.device(self.device):
            _lib.check(self.net.lib.nesti_mask_empty_queries(
                _lib.ptr(n_eff), normals.shape[0], self.cfg.n_scales, _lib.ptr(normals), None if single_tower else _lib.ptr(expert),
                None if single_tower else _lib.ptr(probs), probs.shape[1], _lib.stream_ptr(torch.cuda.current_stream(self.device))),
                "nesti_mask_empty_queries")

    def run(self, cloud: CloudPatches, first=0, count=None, out=None):
        """Normals for patch rows [first, first+count) of a prepared cloud.

        Returns (normals [count,3] f32, expert [count] int32, probs [count,E] f32) on the device
        (ms_sw_n_est: expert = tower picked by the noise threshold, probs = noise_est [count,1]);
        everything is enqueued on the current stream, nothing synchronises."""
        count = cloud.patch_count - first if count is None else count
        E = max(1, self.cfg.n_gate_out)
        if out is None:
            normals = torch.empty((count, 3), dtype=torch.float32, device=self.device)
            expert = torch.empty((count,), dtype=torch.int32, device=self.device)
            probs = torch.empty((count, E), dtype=torch.float32, device=self.device)
        else:
            normals, expert, probs = out
        single_tower = self.cfg.arch in (ARCH_SINGLE, ARCH_MULTI)      # ss/ms ablations: normals only
        if first < 0 or count < 0 or first + count > cloud.patch_count:
            raise ValueError("patch rows [%d, %d) outside [0, %d)" % (first, first + count, cloud.patch_count))
        at = cloud.queries is not None
        if at and self._ref is not None:
            raise _lib.NestiError("subsample=%r reproduces the reference's subsample order, which is defined for index queries only; "
                                  "a cloud with position queries needs subsample='hash'" % self.subsample)
        if self._ref is not None:
            if self._ref_failed:
                raise _lib.NestiError("a reference-order run failed half way: the shared random stream no longer lines up with "
                                      "the reference's; create a new NormalEstimator")
            if self.subsample == "reference" and count > 0:
                return self._run_reference_gpu(cloud, first, count, normals, expert, probs, single_tower)
            return self._run_reference_order(cloud, first, count, normals, expert, probs, single_tower)
        if self._fused:
            main = torch.cuda.current_stream(self.device)
            for st, _ in self._lanes:
                st.wait_stream(main)                  # the cloud's grid (and earlier work) is ready
            # one stream: ONE call, the library walks the batches; several: one call per batch, alternating the lanes
            step = count if self.n_streams == 1 else self.batch
            done, it = 0, 0
            while done < count:
                take = min(step, count - done)
                lane = it % self.n_streams
                it += 1
                st, arena = (main, self._arena) if lane == 0 else self._lanes[lane - 1]
                r0 = first + done
                qidx = cloud.pidx[r0:r0 + take].contiguous() if cloud.pidx is not None else None
                with torch.cuda.device(self.device):
                    if at:
                        _lib.check(self.net.lib.nesti_estimate_normals_at(
                            self.net._handle, _lib.ptr(cloud.cloud), cloud.n_points, _lib.ptr(cloud.queries[r0:r0 + take]), take,
                            cloud._r, ctypes.c_uint64(cloud.seed), r0, self.batch, 0, _lib.ptr(cloud._ws), cloud._ws.numel(),
                            _lib.ptr(arena), arena.numel(), _lib.ptr(normals[done:done + take]),
                            None if single_tower else _lib.ptr(expert[done:done + take]),
                            None if single_tower else _lib.ptr(probs[done:done + take]), None,
                            ctypes.c_void_p(st.cuda_stream)), "nesti_estimate_normals_at")
                    else:
                        _lib.check(self.net.lib.nesti_estimate_normals(
                            self.net._handle, _lib.ptr(cloud.cloud), cloud.n_points, _lib.ptr(qidx), take, cloud._r,
                            ctypes.c_uint64(cloud.seed), r0, self.batch, 0, _lib.ptr(cloud._ws), cloud._ws.numel(),
                            _lib.ptr(arena), arena.numel(), _lib.ptr(normals[done:done + take]),
                            None if single_tower else _lib.ptr(expert[done:done + take]),
                            None if single_tower else _lib.ptr(probs[done:done + take]),
                            ctypes.c_void_p(st.cuda_stream)), "nesti_estimate_normals")
                if qidx is not None and lane > 0:
                    qidx.record_stream(st)
                done += take
            for st, _ in self._lanes:
                main.wait_stream(st)                  # results are ordered on the caller's stream again
            if single_tower:
                return normals, None, None
            return normals, expert, probs
        done = 0
        while done < count:
            take = min(self.batch, count - done)
            sl = slice(done, done + take)
            p, n = self._points[:take], self._n_eff[:take]
            cloud.build(first + done, take, out=(p, n))
            if self.use_graph and take == self.batch:
                if self._graph is None:
                    self._capture()
                    cloud.build(first + done, take, out=(p, n))     # capture ran on placeholder inputs
                self._graph.replay()
                normals[sl].copy_(self._g_out[0])
                expert[sl].copy_(self._g_out[1])
                probs[sl].copy_(self._g_out[2])
            else:
                self.net.forward(p, n, out=(normals[sl], expert[sl], probs[sl]))
            if at:
                self._mask_empty(n, normals[sl], expert[sl], probs[sl], single_tower)
            done += take
        if single_tower:
            return normals, None, None
        return normals, expert, probs

    # -- reproducible mode -------------------------------------------------------------------
    def run_verified(self, cloud, first=0, count=None, out=None):
        """:meth:`run` with the 1.5 x guarantee of the default mode, as a pure function of (model, calibrated tau / thr, cloud, query
        set).  SYNCHRONISES the device after every pass (it reads the counters on the host).  The range runs frozen; if a row decided
        twice shows 1.5 x its error above a threshold, tau <- max(tau, 1.5 x max_margin_err) and thr <- max(thr, 1.5 x max_dn /
        sqrt(2 x 2.5e-6)) and the WHOLE range runs again, at most ``1 + _lib.GATE_WIDEN_PASSES`` passes (then ``NestiError``, as for
        ``guard_dropped > 0``).  The calibrated thresholds are back in place afterwards; ``self.last_verified`` = {passes, tau, thr,
        max_margin_err, max_dn} of the pass whose results are returned.  Resets the model's counters.  Two calls over two halves of
        a range need not equal one call over the whole: the query sets differ."""
        if not self.reproducible:
            raise ValueError("run_verified belongs to NormalEstimator(..., reproducible=True)")
        if self.subsample != "hash":
            raise ValueError("run_verified needs subsample='hash': a second pass would draw from the shared reference stream again")
        return verified_passes(self, lambda: self.run(cloud, first, count, out))

    def _set_thresholds(self, tau, thr):
        if self.net.cascade:
            self.net.set_gate_margin(tau)
        if self._has_guard:
            self.net.set_x8_guard(thr)
        self._graph = None          # a captured forward pass carries the thresholds it was captured with

    def verify_begin(self):
        """Remember (tau, thr) and reset the three counter blocks (synchronises)."""
        torch.cuda.synchronize(self.device)
        st = self.net.reproducible_stats(reset=True)
        self._verify_thr = (st["tau"], st["thr"])
        # dtype 'f16x8c' with recheck stage 2 running (a second margin has been set): that margin is saved and restored too
        cs = self.net.cascade_stats() if getattr(self.net, "stage2", False) else {}
        self._verify_tau2 = cs["tau2"] if cs.get("stage2") else None
        return self._verify_thr

    def verify_flags(self):
        """[max_margin_err, max_dn, violations > 0, dropped > 0] of everything run since the last reset, as a 4-float device tensor --
        the first two written by the export kernels (synchronises; the counters stay, so the stats of the last pass can be read)."""
        t = torch.zeros(4, dtype=torch.float32, device=self.device)
        if self.net.cascade:
            self.net.export_gate_error(t[0:1])
        if self._has_guard:
            self.net.export_guard_error(t[1:2])
        torch.cuda.synchronize(self.device)
        st = self.net.reproducible_stats()
        t[2] = float(st["gate_violations"] + st["guard_violations"] > 0)
        t[3] = float(st["guard_dropped"] > 0)
        return t

    def verify_raise(self, max_margin_err, max_dn):
        """The thresholds of the next pass, in the device's own float32 arithmetic (the violation tests compare 1.5f x err with tau
        and 1.5f / sqrtf(2 x bar) x dn with thr: the same products here, so the row that caused a pass cannot cause the next)."""
        f = np.float32
        tau, thr = self._verify_thr
        tau = max(f(tau), f(_lib.GATE_WIDEN) * f(max_margin_err))
        if getattr(self, "_verify_tau2", None) is not None:
            # recheck stage 2 is running: its margin follows the largest error of the stage the same way (after a sharded pass
            # every rank holds the largest any rank measured: dist.py's gather carries it)
            st = self.net.cascade_stats()
            self.net.set_gate_margin2(float(max(f(st["tau2"]), f(_lib.GATE_WIDEN) * f(st["max_margin_err2"]))))
        if self._has_guard and thr >= 0.0:
            scale = f(_lib.X8_GUARD_WIDEN) / np.sqrt(f(2.0) * f(_lib.X8_GUARD_BAR))
            thr = max(f(thr), scale * f(max_dn))
        self._verify_thr = (float(tau), float(thr))
        self._set_thresholds(*self._verify_thr)
        self.net.reproducible_stats(reset=True)

    def verify_record(self, passes, max_margin_err, max_dn):
        self.last_verified = {"passes": passes, "tau": self._verify_thr[0], "thr": self._verify_thr[1],
                              "max_margin_err": max_margin_err, "max_dn": max_dn}

    def verify_end(self, saved):
        torch.cuda.synchronize(self.device)
        if getattr(self, "_verify_tau2", None) is not None:
            self.net.set_gate_margin2(self._verify_tau2)
        self._set_thresholds(*saved)

    def _prefetch(self, spans, make, consume):
        """Producer / consumer over ``spans`` with two buffers in flight: ``make(i, span)`` runs in ONE worker thread, span after
        span (the shared random stream stays in visiting order), ``consume(i, span, item)`` on the calling thread; the worker
        may run one span ahead of the span being consumed.  Whatever fails, the worker is stopped and joined before the error
        propagates, and the estimator refuses further reference-order runs (the stream position is lost)."""
        import queue
        import threading
        ready, free, stop = queue.Queue(), threading.Semaphore(2), threading.Event()

        def produce():
            try:
                for i, span in enumerate(spans):
                    free.acquire()
                    if stop.is_set():
                        return
                    ready.put(make(i, span))
            except BaseException as e:      # noqa: BLE001 -- hand the failure to the consumer instead of dying silently
                ready.put(e)

        worker = threading.Thread(target=produce, daemon=True)
        worker.start()
        ok = False
        try:
            for i, span in enumerate(spans):
                item = ready.get()
                if isinstance(item, BaseException):
                    raise item
                consume(i, span, item, free.release)
            ok = True
        finally:
            if not ok:
                self._ref_failed = True
                stop.set()
                free.release()
                free.release()
            worker.join()

    def _run_reference_order(self, cloud, first, count, normals, expert, probs, single_tower):
        """Patch rows [first, first + count) with the reference's own subsample on the HOST (scipy ball query + the replayed random
        stream, ``refsample.py``), then the usual forward pass.  The host pass of batch k + 1 runs in a worker thread while batch k is
        uploaded and goes through the GPU."""
        if getattr(cloud, "_ref_tree", None) is None:
            cloud._ref_tree = self._ref.build_tree(cloud.host_pts)
        S, P = self.cfg.n_scales, self.cfg.num_point
        pidx_host = cloud.pidx[first:first + count].cpu().numpy() if cloud.pidx is not None else None
        spans = [(done, min(self.batch, count - done)) for done in range(0, count, self.batch)]

        def make(i, span):
            done, take = span
            centers = pidx_host[done:done + take] if pidx_host is not None else np.arange(first + done, first + done + take)
            return self._ref.patches(cloud.host_pts, cloud._ref_tree, centers, cloud.r_abs, P)

        def consume(i, span, item, release):
            done, take = span
            p, n = item
            sl = slice(done, done + take)
            p_d, n_d = torch.from_numpy(p).to(self.device), torch.from_numpy(n).to(self.device).view(take, S)   # synchronous copies
            release()                           # the host buffer may be refilled
            self.net.forward(p_d, n_d, out=(normals[sl], expert[sl], probs[sl]))

        self._prefetch(spans, make, consume)
        if single_tower:
            return normals, None, None
        return normals, expert, probs

    def _run_reference_gpu(self, cloud, first, count, normals, expert, probs, single_tower):
        """The same rows on the GPU.  cKDTree's result order is ascending position in ``tree.indices``, so
        the reference's subsample needs (1) the ball sizes -- one count launch for the whole range, (2) its random stream replayed
        over those sizes in visiting order -- natively, in a worker thread, one batch ahead (``refsample.RefStream``), (3) the
        balls sorted by tree position with the picks applied -- ``patches_ref_kernel``, then the usual forward pass.  The patch
        tensors equal the host path's bit for bit (tests/test_gpu_patches.py), hence so do the normals."""
        S, P = self.cfg.n_scales, self.cfg.num_point
        cloud.ensure_tree_order()
        sizes = cloud.count_balls(first, count).cpu().numpy()                  # [count, S]; synchronises
        cap = min(int(self.net.lib.nesti_patches_ref_max_ball()), 65535)
        if int(sizes.max(initial=0)) > cap:
            # a ball too large for the kernel's LDS sort (or the uint16 pick table): this shape goes through the host path, which
            # draws from the same stream object
            return self._run_reference_order(cloud, first, count, normals, expert, probs, single_tower)
        spans = [(done, min(self.batch, count - done)) for done in range(0, count, self.batch)]
        if getattr(self, "_ref_pinned", None) is None:
            n = self.batch * S * P
            self._ref_pinned = [(torch.empty(n, dtype=torch.int16).pin_memory(), torch.empty(self.batch * S, dtype=torch.int64).pin_memory())
                                for _ in range(2)]
            self._ref_dev = [(torch.empty(n, dtype=torch.int16, device=self.device),
                              torch.empty(self.batch * S, dtype=torch.int64, device=self.device)) for _ in range(2)]
            self._ref_copy = torch.cuda.Stream(device=self.device)

        def make(i, span):
            done, take = span
            pk, off = self._ref_pinned[i & 1]
            picks, _ = self._ref_stream.picks(sizes[done:done + take].ravel(), P, out=(pk.numpy().view(np.uint16), off.numpy()))
            return len(picks)

        main = torch.cuda.current_stream(self.device)
        copied = [None, None]

        def consume(i, span, n_picks, release):
            done, take = span
            pk, off = self._ref_pinned[i & 1]
            pk_d, off_d = self._ref_dev[i & 1]
            if copied[i & 1] is not None:
                self._ref_copy.wait_event(copied[i & 1])       # the kernel that read this device slot two batches ago is done
            with torch.cuda.stream(self._ref_copy):
                pk_d[:n_picks].copy_(pk[:n_picks], non_blocking=True)
                off_d[:take * S].copy_(off[:take * S], non_blocking=True)
            self._ref_copy.synchronize()        # only the copies: the compute stream keeps running
            release()                           # the pinned slot may be refilled
            main.wait_stream(self._ref_copy)
            sl = slice(done, done + take)
            p, n = self._points[:take], self._n_eff[:take]
            cloud.build_reference_order(first + done, take, pk_d, off_d, out=(p, n))
            ev = torch.cuda.Event()
            ev.record(main)
            copied[i & 1] = ev
            self.net.forward(p, n, out=(normals[sl], expert[sl], probs[sl]))

        self._prefetch(spans, make, consume)
        if single_tower:
            return normals, None, None
        return normals, expert, probs

    def run_many(self, items):
        """Several shapes (or shards of shapes) as ONE stream of batches: ``items`` = [(cloud, first, count), ...].
        Returns one (normals, expert, probs) triple of device tensors per item (views of the concatenated outputs).
        Small shapes / shards share the gate and expert launches (``nesti_estimate_normals_multi``); results equal
        ``run`` on each item.  With ``n_streams`` > 1 the stream of rows is cut into groups of ``batch`` rows and the
        groups alternate between the HIP streams.  8^3 grid, fused mode; otherwise falls back to per-item ``run``."""
        if not self._fused or self.cfg.n_gaussians != 8:
            return [self.run(c, f, n) for c, f, n in items]
        total = sum(n for _, _, n in items)
        E = max(1, self.cfg.n_gate_out)
        single_tower = self.cfg.arch in (ARCH_SINGLE, ARCH_MULTI)
        normals = torch.empty((total, 3), dtype=torch.float32, device=self.device)
        expert = torch.empty((total,), dtype=torch.int32, device=self.device)
        probs = torch.empty((total, E), dtype=torch.float32, device=self.device)
        for cloud, first, count in items:
            if first < 0 or count < 0 or first + count > cloud.patch_count:
                raise ValueError("patch rows [%d, %d) outside [0, %d)" % (first, first + count, cloud.patch_count))
        # a library call serves index items or position items, and one stream of batches is one kind of call
        if len({c.queries is not None for c, _, _ in items}) > 1:
            raise ValueError("run_many: clouds with position queries and clouds with index queries cannot share one call; "
                             "run the two kinds separately")
        # groups of pieces (cloud, first, count): one group = one library call on one lane
        if self.n_streams == 1:
            groups = [list(items)]
        else:
            groups, cur, room = [], [], self.batch
            for cloud, first, count in items:
                while count > 0:
                    take = min(count, room)
                    cur.append((cloud, first, take))
                    first, count, room = first + take, count - take, room - take
                    if room == 0:
                        groups.append(cur)
                        cur, room = [], self.batch
            if cur:
                groups.append(cur)
        main = torch.cuda.current_stream(self.device)
        for st, _ in self._lanes:
            st.wait_stream(main)
        keep, o = [], 0
        for gi, group in enumerate(groups):
            lane = gi % self.n_streams
            st, arena = (main, self._arena) if lane == 0 else self._lanes[lane - 1]
            at = bool(group) and group[0][0].queries is not None
            arr = ((_lib.CShapePositions if at else _lib.CShapeQueries) * max(1, len(group)))()
            for i, (cloud, first, count) in enumerate(group):
                qidx = cloud.pidx[first:first + count].contiguous() if cloud.pidx is not None else None
                if qidx is not None and lane > 0:
                    qidx.record_stream(st)
                keep.append(qidx)
                arr[i].cloud_dev = cloud.cloud.data_ptr()
                arr[i].n_points = cloud.n_points
                if at:
                    arr[i].query_xyz_dev = cloud.queries[first:first + count].data_ptr() if count > 0 else None
                else:
                    arr[i].query_idx_dev = qidx.data_ptr() if qidx is not None and count > 0 else None
                arr[i].n_queries = count
                for s, r in enumerate(cloud.r_abs):
                    arr[i].r_abs[s] = r
                arr[i].seed = cloud.seed
                arr[i].query_row0 = first
                arr[i].grid_ws_dev = cloud._ws.data_ptr()
                arr[i].grid_ws_bytes = cloud._ws.numel()
            rows = sum(c for _, _, c in group)
            entry = "nesti_estimate_normals_multi_at" if at else "nesti_estimate_normals_multi"
            with torch.cuda.device(self.device):
                _lib.check(getattr(self.net.lib, entry)(
                    self.net._handle, arr, len(group), self.batch, _lib.ptr(arena), arena.numel(), _lib.ptr(normals[o:o + rows]),
                    None if single_tower else _lib.ptr(expert[o:o + rows]), None if single_tower else _lib.ptr(probs[o:o + rows]),
                    ctypes.c_void_p(st.cuda_stream)), entry)
            o += rows
        for st, _ in self._lanes:
            main.wait_stream(st)
        out, o = [], 0
        for _, _, n in items:
            out.append((normals[o:o + n], None if single_tower else expert[o:o + n], None if single_tower else probs[o:o + n]))
            o += n
        return out

    def orient(self, cloud, normals, mode="mst", viewpoint=None, k=8):
        """Orient the normals of a prepared cloud's patch rows IN PLACE (``orient.orient_device``: minimum-spanning-tree propagation,
        or ``mode='viewpoint'``), on the current stream, after everything that wrote them.  ``normals`` [patch_count, 3]: what
        :meth:`run` / :meth:`run_verified` returned for the whole range.  Positions are the cloud, ``cloud[pidx]`` or the query
        positions; the radius is the largest patch radius ``cloud.r_abs[-1]``, the scale at which the network itself looks.  Rows
        without a neighbourhood (the (0, 0, 0) sentinel) stay as they are.  Returns the stats as an int32[4] device tensor
        (``orient.stats_dict``); nothing synchronises."""
        from . import orient as _orient
        if normals.shape[0] != cloud.patch_count:
            raise ValueError("orientation needs the normals of all %d patch rows, got %d" % (cloud.patch_count, normals.shape[0]))
        if not normals.is_contiguous():
            raise ValueError("orientation works in place on a contiguous [M, 3] tensor")
        return _orient.orient_device(cloud.centre_positions(), normals, float(cloud.r_abs[-1]), k, viewpoint, mode,
                                     torch.cuda.current_stream(self.device))

    def estimate(self, pts, pidx=None, queries=None, orient=None, viewpoint=None, orient_k=8, smooth=None, outliers=None):
        """Convenience: numpy cloud in, numpy results out (synchronises).  ``queries`` [M,3]: positions instead of cloud points;
        a position without a neighbourhood comes back as normal (0, 0, 0), expert -1, probabilities 0.  ``orient`` = ``'mst'`` /
        ``'viewpoint'`` (default None: signs as the experts produced them): :meth:`orient` runs over the estimated rows, only signs
        change, and ``self.last_orient`` holds the stats dict.  ``smooth`` -- None, a number of passes or a dict of ``k``, ``iters``,
        ``angle``, ``falloff`` (``smooth.smooth_normals``) -- smooths the normals over all points before the orientation; it needs
        all points (``ValueError`` with ``pidx`` or ``queries``: the rows' neighbours would have no normal), leaves experts and
        probabilities alone, and ``self.last_smooth`` holds ``smooth_support`` and ``smooth_count`` of the last pass.  ``outliers`` --
        None, ``'statistical'`` or a dict: the filter of the preprocessing chain (``stages``), alone -- filters the cloud first: the three arrays come back with the rows of
        ``pts`` (normal 0 0 0, expert -1, probabilities 0 in the removed ones; nothing is mapped with ``queries``) and
        ``self.last_outliers`` holds ``inlier``, ``kept``, ``score`` and ``passes``; ``pidx`` with it is refused."""
        if orient not in (None, "mst", "viewpoint"):
            raise ValueError("orient must be None, 'mst' or 'viewpoint'")
        from . import smooth as _smooth, stages
        params = stages.check(None, outliers, None, pidx)
        sm = _smooth.as_params(smooth)
        if sm is not None:
            _smooth.refuse_subset(pidx, queries)
        chain = stages.run(pts, params, queries, self.device)
        cloud = self.prepare(np.asarray(chain.points, dtype=np.float32), pidx, queries)
        normals, expert, probs = self.run(cloud)
        if sm is not None:
            with torch.cuda.device(self.device):
                normals, support, count = _smooth.smooth_cloud(cloud, normals.contiguous(), sm)
        if orient is not None:
            from .orient import stats_dict
            self.last_orient = stats_dict(self.orient(cloud, normals, orient, viewpoint, orient_k))
        torch.cuda.synchronize(self.device)
        if sm is not None:
            self.last_smooth = {"smooth_support": chain.to_input(support.cpu().numpy()), "smooth_count": chain.to_input(count.cpu().numpy())}
        if chain.kept is not None:
            self.last_outliers = {"inlier": chain.keys["inlier"], "kept": chain.kept, "score": chain.keys["outlier_score"],
                                  "passes": chain.keys["outlier_passes"]}
        return tuple(None if a is None else chain.to_input(a.cpu().numpy(), fill) for a, fill in ((normals, 0), (expert, -1), (probs, 0)))

    def estimate_depth(self, depth, camera, stride=1, orient="viewpoint", orient_k=8, on_cloud=None, outliers=None):
        """Depth frame in, normal image out (``depth.py``; DESIGN.md 2 "Depth images"): back-project ``depth`` [H,W] (uint16 or
        float32) through ``camera`` (``depth.Camera``), prepare the cloud of valid pixels, estimate -- :meth:`run`, or
        :meth:`run_verified` when the estimator is reproducible -- at every valid pixel, or with ``stride`` > 1 at the valid pixels
        with ``v % stride == 0 and u % stride == 0`` (``pidx`` = their cloud rows; the neighbourhoods still come from every valid
        pixel), orient, and scatter the rows into images.  ``orient``: ``'viewpoint'`` (default; the viewpoint is the camera centre:
        the pose's translation column, or the origin), ``'mst'`` (rooted at the point nearest to the camera) or None.
        ``on_cloud(cloud)`` (optional) is called with the prepared ``CloudPatches`` before anything runs (per-frame calibration).

        Returns a dict of numpy arrays (synchronises): ``normal_map`` [H,W,3] f32 (fill 0 0 0), ``expert_map`` [H,W] int32 (fill -1)
        and ``probs_map`` [H,W,E] f32 (fill 0) -- both omitted for the single-tower models -- and per estimated pixel, in pixel
        order, ``xyz``, ``pix`` (pixel index ``v W + u``), ``normals``, ``expert``, ``probs`` (None for the single-tower models).  A
        frame without a valid pixel gives all-fill maps and empty rows without touching the network.  The cloud passes through the
        host once (``CloudPatches`` takes a host array and computes the bounding-box diagonal there).

        ``outliers`` -- None, ``'statistical'`` or a dict (``outliers.remove_outliers``; DESIGN.md 2 "Outlier removal") -- filters the
        back-projected cloud of valid pixels first, which is where a depth discontinuity leaves its flying pixels: the network and the
        orientation see the kept points alone; the rows stay those of the valid pixels, a removed one holding the maps' fill (0 0 0,
        -1, 0) in the rows and in the maps, and the dict gains ``inlier`` [rows] bool (``self.last_outliers`` holds the scores and the
        passes' statistics too).  It needs ``stride == 1`` (``ValueError``
        otherwise: a strided frame estimates at a subset of the cloud, which is ``pidx``)."""
        from . import depth as _depth
        if orient not in (None, "mst", "viewpoint"):
            raise ValueError("orient must be None, 'mst' or 'viewpoint'")
        from . import outliers as _outliers
        filt = _outliers.as_params(outliers)
        if filt is not None and int(stride) != 1:
            raise ValueError("outliers needs stride == 1: a strided frame estimates at a subset of the cloud (pidx), which the filter "
                             "does not serve yet")
        single_tower = self.cfg.arch in (ARCH_SINGLE, ARCH_MULTI)
        E = max(1, self.cfg.n_gate_out)
        dc = _depth.depth_to_cloud(depth, camera, stride=stride, device=self.device)
        H, W = dc.H, dc.W
        rows = dc.n_valid if dc.stride == 1 else dc.n_queries
        with torch.cuda.device(self.device):
            if rows == 0:
                normals = torch.empty((0, 3), dtype=torch.float32, device=self.device)
                expert = None if single_tower else torch.empty((0,), dtype=torch.int32, device=self.device)
                probs = None if single_tower else torch.empty((0, E), dtype=torch.float32, device=self.device)
                xyz, pix = dc.xyz[:0], dc.pix[:0]
            else:
                sparse = dc.stride > 1
                host_xyz = dc.xyz.cpu().numpy()
                kept = None
                if filt is not None:
                    f = _outliers.remove_outliers(host_xyz, *filt, device=self.device)
                    if not len(f["kept"]):
                        raise ValueError("outliers: the filter kept none of the %d valid pixels" % rows)
                    host_xyz = f["points"]
                    kept = torch.from_numpy(f["kept"].astype(np.int32)).to(self.device)
                    inlier = torch.from_numpy(f["inlier"]).to(self.device)
                    self.last_outliers = {key: f[key] for key in ("inlier", "kept", "score", "passes")}
                cloud = self.prepare(host_xyz, pidx=dc.qidx.cpu().numpy() if sparse else None)
                if on_cloud is not None:
                    on_cloud(cloud)
                normals, expert, probs = self.run_verified(cloud) if self.reproducible else self.run(cloud)
                if orient is not None:
                    from .orient import stats_dict
                    self.last_orient = stats_dict(self.orient(cloud, normals, orient, dc.viewpoint, orient_k))
                if kept is not None:                       # back to the rows of the valid pixels; a removed one holds the maps' fill
                    normals = _outliers.scatter_rows(normals.contiguous(), kept, rows, 0.0)
                    expert = None if expert is None else _outliers.scatter_rows(expert.contiguous(), kept, rows, -1)
                    probs = None if probs is None else _outliers.scatter_rows(probs.contiguous(), kept, rows, 0.0)
                sel = dc.qidx.long() if sparse else None
                xyz = dc.xyz[sel] if sparse else dc.xyz
                pix = dc.pix[sel].contiguous() if sparse else dc.pix
            out = {"normal_map": _depth.scatter_to_image(normals, pix, H, W, 0.0)}
            if not single_tower:
                out["expert_map"] = _depth.scatter_to_image(expert, pix, H, W, -1)
                out["probs_map"] = _depth.scatter_to_image(probs, pix, H, W, 0.0)
            out.update(xyz=xyz, pix=pix, normals=normals, expert=expert, probs=probs)
            if filt is not None:
                out["inlier"] = inlier if rows else torch.zeros(0, dtype=torch.bool, device=self.device)
            torch.cuda.synchronize(self.device)
        return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
