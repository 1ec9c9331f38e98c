"""Registration -- drop-in for the NDP path of the reference's model/registration.py.

    model = Registration(config)                       (/root/reference/model/registration.py:27-34)
    model.load_pcds(src, tgt, landmarks=None)          (:93-103)
    warped, iter_cnt, timer = model.register(visualize=False, timer=None)   (:106-123, :126-262)
    model.src_pcd                                      un-centred source on the device (eval_nolearned.py:94)

plus two extensions the reference has no counterpart for.  The fitted weights stay inside the engine; a caller that goes on
from them (joint refinement of all levels, inverting the warp) gets them as an object:

    pyramid, src_mean, tgt_mean = model.fitted_pyramid()     after register(); pyramid.warp(src - src_mean)[0] + tgt_mean

and, because the reference's loop is one pair at a time:

    results = model.register_batch([(src, tgt[, landmarks]), ...], slots=64)

which keeps `slots` pairs resident on the GPU and advances them together (engine.py).

Host work stays in torch (tensor plumbing, the CPU RNG replay of the reference's init and
randperm calls); the optimisation itself runs in libndp_hip.so.  There is no CPU fallback:
config.device must be a GPU.
"""
import collections
import ctypes
import functools
import gc

import numpy as np
import torch

from . import _native as N
from . import ops
from .batch import PairProducer, _BatchCtx, _Lane, _PinRing, _Prepared
from .engine import BatchedEngine, OptConfig
from .layout import LayerDesc
from .nets import _draw_ops, _native_rng_ok, init_pyramid_store


class Registration:
    def __init__(self, config, gemm_mode=None, nn_mode=None, nn_matrix=None, nn_cells=None, nn_cells_wide=None):
        """config: the reference's attribute-accessible config (NDP.yaml / LNDP.yaml keys).  gemm_mode / nn_mode (extension, both
        default to the engine's choice, see engine.resolve_modes): arithmetic of the level kernels' 128x128 contractions (0: fp32
        MFMA, bitwise the oracle's chain; 7: two-way fp16 splits on the fp16 MFMA), a forced shape of the nearest-neighbour kernel
        (nn_mode) or just the preference for its matrix-pipe variant where the engine picks the throughput shape (nn_matrix).
        nn_cells: the nearest-neighbour stage as the exact grid ball search (None: the engine's choice, engine.resolve_nn_cells).
        nn_cells_wide: the same search for clouds of up to 8192 points (None: the engine's choice, engine.resolve_nn_cells_wide)."""
        self.gemm_mode, self.nn_mode, self.nn_matrix, self.nn_cells, self.nn_cells_wide = gemm_mode, nn_mode, nn_matrix, nn_cells, nn_cells_wide
        self.tgt_pcd = None
        self.src_pcd = None
        self.landmarks = None
        self.config = config
        self.device = config.device
        self.deformation_model = config.deformation_model
        self._engines = {}
        self.last_state = None
        self._last_fit = None

    # ------------------------------------------------------------------ reference surface
    def load_pcds(self, src, tgt, landmarks=None):
        if isinstance(src, np.ndarray):
            src = torch.from_numpy(src)
            tgt = torch.from_numpy(tgt)
        self.src_pcd = src.to(self.device)
        self.tgt_pcd = tgt.to(self.device)
        self.landmarks = landmarks

    def load_raw_pcds_from_depth(self, source_depth_path, tgt_depth_path, K, landmarks=None):
        """Deformation graph + raw clouds of the embedded-deformation (N-ICP) baseline (registration.py:38-90)."""
        from .ed import load_raw_pcds_from_depth
        load_raw_pcds_from_depth(self, source_depth_path, tgt_depth_path, K, landmarks)

    def register(self, **kwargs):
        if self.deformation_model == "NDP":
            return self.optimize_deformation_pyramid(**kwargs)
        if self.deformation_model == "NSFP":                      # registration.py:112-113 -> (warped, None)
            from .nsfp import optimize_neural_SFlow
            kwargs.pop("timer", None)
            return optimize_neural_SFlow(self, **kwargs)
        if self.deformation_model == "Nerfies":                   # registration.py:118-119 -> (warped, None)
            from .nerfies import optimize_Nerfies
            kwargs.pop("timer", None)
            return optimize_Nerfies(self, **kwargs)
        if self.deformation_model == "ED":                        # registration.py:112-113 -> (warped sampled cloud, valid_id)
            from .ed import optimize_Embeded_deformation
            kwargs.pop("timer", None)
            return optimize_Embeded_deformation(self, **kwargs)
        if self.deformation_model == "Sinkhorn":                  # registration.py:108-109 -> (moved source samples, their indices)
            from .sinkhorn import run_optimal_transport
            kwargs.pop("timer", None)
            return run_optimal_transport(self, **kwargs)
        raise N.NdpUnservedError(f"deformation_model {self.deformation_model!r} is not served (NDP, NSFP, Nerfies, ED, Sinkhorn are)")

    def optimize_deformation_pyramid(self, visualize=False, timer=None):
        if visualize:
            raise NotImplementedError("mayavi visualisation is outside the hot path")
        prep = self._prepare(self.src_pcd, self.tgt_pcd, self.landmarks)
        self.src_pcd = prep.src_pcd
        eng = self._engine(1, prep)
        eng.load_jobs([prep.load_job(0)])
        kernel_ms = [0.0] * len(N.TICK_KERNELS) if timer is not None else None
        st = eng.run_until_done(chunk=32, kernel_ms=kernel_ms)[0]
        warped = self._finish(eng, [(0, prep)])[0]
        self.last_state = st
        self._last_fit = (eng, prep)
        iter_cnt = {lvl: int(st.evals_per_level[lvl]) for lvl in range(self.config.m)}
        if timer is not None:
            self._fill_timer(timer, kernel_ms, st, prep.K > 0)
        return warped, iter_cnt, timer

    def fitted_pyramid(self):
        """-> (pyramid, src_mean [3], tgt_mean [3]) of the last register(): the fitted weights as a Deformation_Pyramid over a COPY
        of the engine slot's [m, p_stride] block (writing into it changes nothing a later register() computes), and the two cloud
        means of registration.py:150-153, such that  pyramid.warp(src - src_mean)[0] + tgt_mean  is the cloud register() returned
        (bit for bit in the fp32 arithmetic, gemm_mode 0; register()'s own final warp otherwise runs on the fp16-split contractions).
        Its levels are nn.Modules with trainable parameters, and warp() is differentiable in them and in its points."""
        if self._last_fit is None:
            raise RuntimeError("fitted_pyramid(): no fitted pyramid yet -- call register() (deformation_model NDP) first")
        from .nets import Deformation_Pyramid
        eng, prep = self._last_fit
        c = self.config
        pyramid = Deformation_Pyramid.from_store(eng.params[0].clone(), c.depth, c.width, c.k0, c.rotation_format,
                                                 nonrigidity_est=c.w_reg > 0, motion=c.motion_type)
        return pyramid, prep.means[0:3].clone(), prep.means[4:7].clone()

    def inverse_warp(self, points, **kw):
        """Target-frame points -> the source frame of the last register(): fitted_pyramid().inverse_warp(points - tgt_mean) +
        src_mean, i.e. the x with  pyramid.warp(x - src_mean) + tgt_mean = points  (label / texture pull-back, target-side scene
        flow, cycle checks).  **kw: max_level, min_level, x0 (a first guess in the SOURCE frame, the frame of the x returned), iters, tol of
        Deformation_Pyramid.inverse_warp.  -> (x [n,3], info); info.converged says which points Newton solved.  Before any
        register() it raises like fitted_pyramid()."""
        pyramid, src_mean, tgt_mean = self.fitted_pyramid()
        pts = torch.as_tensor(points, dtype=torch.float32).to(pyramid.store.device)
        if kw.get("x0") is not None:
            kw["x0"] = (torch.as_tensor(kw["x0"], dtype=torch.float32).to(pts.device) - src_mean).contiguous()
        x, info = pyramid.inverse_warp((pts - tgt_mean).contiguous(), **kw)
        return x + src_mean, info

    @staticmethod
    def _fill_timer(timer, kernel_ms, st, has_ldmk):
        """The reference tics `lvl_warp` and `Chamfer` once per loss evaluation (only without landmarks) and `backprop` once per
        Adam step (registration.py:207-213, 234-238), and eval_nolearned.py:139-146 prints those keys.  The iteration never
        returns to the host here, so the pair's DEVICE time per kernel (HIP events around every launch, ndp_engine_run_timed) is
        apportioned: lvl_warp = level forward, Chamfer = nearest neighbours + loss / early-stop decision / dL/dx', backprop =
        the two backward kernels + gradient fold and Adam -- recorded as one tictoc per evaluation / step, so that `calls` and
        `average` mean what they mean upstream."""
        ms = dict(zip(N.TICK_KERNELS, kernel_ms))
        groups = [("backprop", (ms["k_eng_bwd2"] + ms["k_eng_bwd1"] + ms["k_eng_update"]) * 1e-3, int(st.total_steps))]
        if not has_ldmk:
            groups = [("lvl_warp", ms["k_eng_fwd"] * 1e-3, int(st.total_evals)),
                      ("Chamfer", (ms["k_eng_nn"] + ms["k_eng_loss"]) * 1e-3, int(st.total_evals))] + groups
        for key, total, calls in groups:
            for _ in range(calls):
                timer.tictoc(key, total / calls)

    # ------------------------------------------------------------------ batched extension
    def register_batch(self, pairs, slots=64, chunk=8, prefetch=True, engines=1, workers=3, sink=None):
        """pairs: sequence of (src, tgt) or (src, tgt, (ldmk_s, ldmk_t)).  Pairs are prepared in order
        (so the CPU RNG stream is consumed exactly as by sequential register() calls) and optimised
        `slots` at a time per engine, finished slots being refilled.  With prefetch=True the host-side preparation
        (RNG replay of the init and of the sampling permutations) runs ahead of the GPU in `workers` producer threads fed by
        one generator-stepping thread (see below: bit-identical to the sequential order whatever the thread count).
        engines > 1 keeps that many independent engines ticking on their own HIP streams: their launches interleave on
        the GPU, so the VALU-bound and latency-bound kernels of one overlap the MFMA-bound kernels of another.
        Returns [(warped, iter_cnt)] in input order.
        sink(i, warped, state): called (on the calling thread, in completion order) for every finished pair INSTEAD of keeping its
        result -- a long stream of pairs then holds no more than the resident ones; the call returns None.  The sink runs with the
        final-warp stream current: GPU work it enqueues on `warped` is ordered behind the kernel that writes it; a reference it keeps
        is safe to use once the call has returned."""
        pairs = list(pairs)
        if not pairs:
            return []
        self._last_fit = None                                    # the engine slots are about to be refilled
        # one engine configuration serves the whole batch: capacities from the LARGEST landmark set (landmarks are known
        # before any preparation), and the objective (w_cd / trunc_cd, registration.py:189-212) must be the same for all
        ks = [int(item[2][0].shape[0]) if len(item) > 2 and item[2] is not None else 0 for item in pairs]
        if min(ks) == 0 and max(ks) > 0:
            raise ValueError("register_batch: pairs with and without landmarks use different objectives "
                             "(registration.py:189-212); register them in separate batches")
        k_max = max(ks)
        engines = max(1, min(int(engines), len(pairs)))
        dev = self._dev()
        main = torch.cuda.current_stream(dev)
        fin_stream = self._stream("fin", dev)                    # final all-point warps overlap the ticking engines
        # Host-side preparation (the RNG replay of the reference's init and of its two randperm calls, registration.py:133-159)
        # runs ahead of the GPU.  The draw counts per pair are known up front, so ONE stepper thread walks torch's CPU generator
        # from pair to pair (regenerations only) and hands each pair the generator state it starts from; `workers` threads replay
        # their pairs from those snapshots natively (GIL released) on their own side streams -- bit-identical to sequential
        # register() calls, in any completion order.  Pair i is prepared by worker i % W and delivered in index order.
        # (No native replay: the torch-call replay consumes the global generator, so one thread prepares every pair.)
        draws = (lambda item: self._pair_draws(int(item[0].shape[0]), int(item[1].shape[0]))) if _native_rng_ok() else None
        producer = PairProducer(pairs, functools.partial(self._prepare_item, dev, collections.Counter()), workers=workers,
                                resident=slots * engines, draws=draws, prefetch=prefetch)
        B = min(slots, -(-len(pairs) // engines))
        ctx = _BatchCtx(self, producer, len(pairs), sink, chunk, self.config.m, main, fin_stream, B * engines)
        # the cyclic collector's FULL passes over thousands of live pair objects stalled every lane for 50-85 ms a few times per
        # batch (rocprofv3 trace of the bench); nothing in the loop builds reference cycles worth collecting before it ends.  Only
        # the oldest generation is held back for the duration of the call -- young collections (cheap, what other threads of the
        # application may rely on) keep running.
        gc_thr = gc.get_threshold()
        gc.set_threshold(gc_thr[0], gc_thr[1], 1 << 30)
        try:
            like = ctx.first()                                   # the first pair's shapes size the engines
            lanes = []
            for e in range(engines):
                stream = main if engines == 1 else self._stream(("lane", e), dev)
                eng = self._engine(B, like, n_hint=(self.config.samples if like.S else 0) + k_max, lane=e)
                with torch.cuda.stream(stream):
                    stream.wait_stream(main)
                    eng.park_all()
                lanes.append(_Lane(ctx, eng, stream))
            while not all(lane.done for lane in lanes):
                for lane in lanes:
                    if not lane.done:
                        with torch.cuda.stream(lane.stream):
                            lane.step()
        except BaseException:
            # a failing lane must not leave the producer blocked on the bounded queue, holding device tensors and
            # pinned buffers: stop it, drain what it queued, join it, and let every stream finish what was enqueued
            producer.close(failed=True)
            torch.cuda.synchronize(dev)
            ctx.preps = None
            raise
        finally:
            gc.set_threshold(*gc_thr)
        producer.close()
        for lane in lanes:
            main.wait_stream(lane.stream)
        main.wait_stream(fin_stream)
        self.last_states = ctx.states
        if sink is not None:
            return None
        return [(p.result, {lvl: int(p.state.evals_per_level[lvl]) for lvl in range(ctx.m)}) for p in ctx.preps]

    def _prepare_item(self, dev, count, item, rng_state, worker):
        """The producer's `prepare`: one item of register_batch -> (prepared pair, event recorded behind its preparation).
        A producer thread (worker 0, 1, ...) prepares on its own side stream with its own pinned ring; worker None is the
        calling thread (prefetch=False): in line on the current stream, no event.  count: pairs prepared per worker in this call."""
        src, tgt = item[0], item[1]
        ldmk = item[2] if len(item) > 2 else None
        if isinstance(src, np.ndarray):
            src, tgt = torch.from_numpy(src), torch.from_numpy(tgt)
        if worker is None:
            return self._prepare(src.to(dev), tgt.to(dev), ldmk), None
        side = self._stream(("side", worker), dev)
        with torch.cuda.stream(side):
            p = self._prepare(src.to(dev), tgt.to(dev), ldmk, rng_state=rng_state, ring=self._pin_ring(worker))
            ev = torch.cuda.Event()
            ev.record(side)
        # The host never waits on this stream otherwise (lanes wait on its events), and the HIP runtime keeps per-command
        # state of a stream until the host synchronises it: a long stream of pairs grew the resident set by ~4.5 KB per
        # pair (tools/stream_memory.py: 4.6 -> 1.2 KB with this).  The producer runs ahead of the GPU: the wait is idle time.
        count[worker] += 1
        if count[worker] % 64 == 0:
            side.synchronize()
        return p, ev

    # ------------------------------------------------------------------ internals
    def _stream(self, key, dev):
        if not hasattr(self, "_streams"):
            self._streams = {}
        if key not in self._streams:
            self._streams[key] = torch.cuda.Stream(dev)
        return self._streams[key]

    def _dev(self):
        d = self.device
        if isinstance(d, int):
            return torch.device("cuda", d)
        d = torch.device(d)
        if d.type != "cuda":
            raise N.NdpUnservedError(f"deformationpyramid_amd runs deformation_model {self.deformation_model!r} on the GPU only "
                                     "(config.device is CPU); there is no CPU fallback")
        return d

    def _opt_config(self, has_ldmk):
        c = self.config
        if has_ldmk:
            w_cd, trunc = float(c.w_cd), float(c.trunc_cd)                       # registration.py:189-197
        else:
            w_cd, trunc = 1.0, 1e9                                               # registration.py:212
        return OptConfig(m=c.m, k0=c.k0, iters=c.iters, lr=c.lr, max_break_count=c.max_break_count,
                         break_threshold_ratio=c.break_threshold_ratio, w_cd=w_cd, trunc=trunc,
                         w_reg=float(c.w_reg), early_stop=True)

    def _init_ops(self, descs, depth, stride):
        """ctypes draw ops of one pair's pyramid initialisation (cached per configuration)."""
        key = (tuple(descs), depth, stride)
        cache = self.__dict__.setdefault("_ops_cache", {})
        if key not in cache:
            cache[key] = N.make_draw_ops(_draw_ops(descs, depth, stride))
        return cache[key]

    def _pair_descs(self):
        c = self.config
        gate = c.w_reg > 0                                                          # registration.py:138
        desc = LayerDesc(width=c.width, n_hidden=c.depth - 1, motion=c.motion_type, rotfmt=c.rotation_format, nonrigidity=gate)
        level0 = LayerDesc(width=c.width, n_hidden=c.depth - 1, motion=c.motion_type, rotfmt=c.rotation_format)
        return desc, [level0] + [desc] * (c.m - 1)                                  # nets.py:26: level 0 never carries the gate

    def _pair_draws(self, n_src, n_tgt):
        """Raw generator draws one pair consumes: pyramid init + randperm(n_src) + randperm(n_tgt)."""
        desc, descs = self._pair_descs()
        ops_ = self._init_ops(descs, self.config.depth, (desc.param_count + 63) // 64 * 64)
        return int(N.host_lib().ndp_pair_draws(ops_, len(ops_), int(n_src), int(n_tgt)))

    def _pin_ring(self, key):
        rings = self.__dict__.setdefault("_pin_rings", {})
        if key not in rings:
            rings[key] = _PinRing()
        return rings[key]

    def _prepare(self, src_pcd, tgt_pcd, landmarks, rng_state=None, ring=None):
        """Host side of registration.py:133-164 for one pair: RNG replay of the pyramid initialisation and of the two
        sampling permutations into ONE pinned buffer, one asynchronous upload, one launch for the two cloud means.
        Centring, sampling and the slot fill itself happen on the device (k_eng_load).
        rng_state: a snapshot of torch's CPU generator state this pair starts from (the batched producer's workers; the global
        generator is then left alone), None: consume the global generator like the reference does.  ring: pinned staging ring."""
        c = self.config
        # (upstream fails deep inside knn_points / mean() on such inputs; say what is wrong instead)
        for name, cloud in (("source", src_pcd), ("target", tgt_pcd)):
            if not torch.is_tensor(cloud) or cloud.ndim != 2 or cloud.shape[1] != 3 or cloud.shape[0] < 1:
                raise ValueError(f"{name} cloud must be a [N, 3] tensor with N >= 1, got "
                                 f"{tuple(cloud.shape) if torch.is_tensor(cloud) else type(cloud).__name__}")
        if landmarks is not None:
            ls, lt = landmarks
            if ls.ndim != 2 or ls.shape[1] != 3 or tuple(ls.shape) != tuple(lt.shape) or ls.shape[0] < 1:
                raise ValueError(f"landmarks must be two [K, 3] tensors with the same K >= 1, got {tuple(ls.shape)} and {tuple(lt.shape)}")
        dev = self._dev()
        if not (1 <= c.width <= 256 and 1 <= c.depth <= 4):        # (128 / 3: the MFMA kernels; the rest: csrc/ndp_generic.inc)
            raise N.NdpError(f"width must be 1..256 and depth 1..4, got width={c.width}, depth={c.depth}")
        p = _Prepared()
        # registration.py:133-140 -- all m levels are initialised up front on the CPU generator
        p.desc, descs = self._pair_descs()                                          # engine: "levels > 0 gated"
        stride = (p.desc.param_count + 63) // 64 * 64
        n_par = c.m * stride
        samples = int(c.samples)
        ring = ring if ring is not None else self._pin_ring("main")
        host = ring.take(n_par + 2 * samples)                                      # reused pinned staging buffer
        src_pcd = src_pcd.to(dev, non_blocking=True).float().contiguous()
        tgt_pcd = tgt_pcd.to(dev, non_blocking=True).float().contiguous()
        p.src_pcd, p.tgt_pcd = src_pcd, tgt_pcd
        n_src, n_tgt = src_pcd.shape[0], tgt_pcd.shape[0]
        ns, nt = min(samples, n_src), min(samples, n_tgt)
        hi = host[n_par:].view(torch.int32)
        if _native_rng_ok():
            # init draws + both permutation prefixes in ONE native call from a generator-state snapshot (GIL released)
            own = rng_state is None
            st = torch.get_rng_state() if own else rng_state
            ops_ = self._init_ops(descs, c.depth, stride)
            store = host[:n_par].view(c.m, stride)
            for i, d in enumerate(descs):
                store[i, d.param_count:] = 0.0
            scratch = ring.scratch(max(n_src, n_tgt))
            L = N.host_lib()
            rc = L.ndp_pair_init(ctypes.c_void_p(st.data_ptr()), st.numel(), ops_, len(ops_), ctypes.c_void_p(host.data_ptr()),
                                 n_src, n_tgt, samples, ctypes.c_void_p(hi.data_ptr()), ctypes.c_void_p(hi[samples:].data_ptr()),
                                 ctypes.c_void_p(scratch.data_ptr()))
            if rc != 0:
                raise N.NdpError("ndp_pair_init failed")
            if own:                                                                 # leave the global generator where torch would
                if L.ndp_rng_skip(ctypes.c_void_p(st.data_ptr()), st.numel(), L.ndp_pair_draws(ops_, len(ops_), n_src, n_tgt)) != 0:
                    raise N.NdpError("ndp_rng_skip failed")
                torch.set_rng_state(st)
        else:
            if rng_state is not None:
                raise N.NdpError("a generator-state snapshot needs the native RNG replay (libndp_host.so)")
            init_pyramid_store(descs, c.depth, stride, out=host[:n_par].view(c.m, stride))   # nets.py:26
            perm_s = torch.randperm(n_src)                                          # :156-159 (CPU RNG)
            perm_t = torch.randperm(n_tgt)
            hi[:ns] = perm_s[:ns]
            hi[samples:samples + nt] = perm_t[:nt]
        p.buf = host.to(dev, non_blocking=True)                                    # async upload on the current stream
        ring.uploaded(host, torch.cuda.current_stream(dev))
        p.store = p.buf[:n_par].view(c.m, stride)
        di = p.buf[n_par:].view(torch.int32)
        p.perm_s, p.perm_t = di[:ns], di[samples:samples + nt]
        p.means = torch.empty(8, device=dev, dtype=torch.float32)                 # :150-153: filled by the slot's load call (ONE launch per
                                                                                   # group of up to 16 pairs instead of one per pair)
        p.ldmk_s = p.ldmk_t = None
        if landmarks is not None:
            p.ldmk_s = landmarks[0].to(dev).float().contiguous()                  # :162-164 (centred on the device)
            p.ldmk_t = landmarks[1].to(dev).float().contiguous()
            p.K = p.ldmk_s.shape[0]
            if c.w_cd > 0:
                p.S, p.T = ns, nt                                                  # :190
            else:
                p.S, p.T = 0, 0
        else:
            p.K, p.S, p.T = 0, ns, nt
        p.result = p.state = None
        return p

    def _engine(self, B, like, n_hint=0, lane=0):
        n_cap = ops.cap(max(like.K + like.S, n_hint))
        t_cap = ops.cap(max(like.T, self.config.samples if like.S else 0))
        cfg = self._opt_config(like.K > 0)
        desc = like.desc
        key = (B, n_cap, t_cap, desc, tuple(sorted(vars(cfg).items())), self.gemm_mode, self.nn_mode, self.nn_matrix, self.nn_cells, self.nn_cells_wide)
        if self._engines.get("key") != key:
            self._engines.clear()                      # one resident engine configuration at a time
            self._engines["key"] = key
        if lane not in self._engines:
            self._engines[lane] = BatchedEngine(desc, cfg, B, n_cap, t_cap, self._dev(), gemm_mode=self.gemm_mode, nn_mode=self.nn_mode, nn_matrix=self.nn_matrix, nn_cells=self.nn_cells, nn_cells_wide=self.nn_cells_wide)
        return self._engines[lane]

    def _finish(self, eng, done, freeze=False, frozen=None):
        """registration.py:253-262 for every (slot, prepared pair) of `done`, in one launch: ALL source points through
        the optimised pyramid (centring by the source mean and adding the target mean happen in the kernel).
        freeze=True first snapshots the slots' parameters -- ONE gathering copy for all of them (round 6; until then a clone per
        pair) -- so that the slots can be refilled at once: `frozen()` is called between the copy and the warp launch (the batched
        lanes record the event their refills wait for there: a refill waits for the copy, not for the warp).  The batched path
        (freeze) also takes the warp's throughput shape, eight tiles per workgroup."""
        c = self.config
        split = bool(eng.gemm_mode & 1)
        if freeze:
            stores = torch.stack([eng.params[slot] for slot, _ in done])          # [len(done), m, p_stride]
            if frozen is not None:
                frozen()
            jobs = [prep.warp_job(stores[k]) for k, (_, prep) in enumerate(done)]
        else:
            jobs = [prep.warp_job(eng.params[slot]) for slot, prep in done]
        # the final warp runs in the engine's arithmetic: fp16-split contractions with gemm_mode & 1, the fp32 MFMA otherwise
        return ops.pyramid_fwd_batch(done[0][1].desc, c.m, c.k0, jobs, device=self._dev(), split=split,
                                     tiles=8 if (freeze and split) else None)
