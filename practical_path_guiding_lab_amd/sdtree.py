"""Host-side handle of the device-resident SD-tree pair (sdTree_prev / sdTree_current).

Mirrors the method surface the reference integrator uses on its two `KDTree` objects
(takkasila/practical_path_guiding_lab src/kdtree.py; call sites in
src/path_guiding_integrator.py:100-105, 244, 301, 307, 500, 559-563, 575-586, 594, 602-608),
on top of the C ABI of libpgsd.so.  Arrays are torch CUDA tensors in planar layout:
a Vector3f[N] is a float32 tensor of shape (3, N) -- the layout Dr.Jit uses for mi.Vector3f.

PyTorch is used only as the owner of caller-side device buffers and streams.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _native as N


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _f32(t: torch.Tensor, shape) -> torch.Tensor:
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"expected contiguous CUDA float32 tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def _mask(active: Optional[torch.Tensor], n: int):
    if active is None:
        return None, None
    if active.dtype == torch.bool:
        active = active.to(torch.uint8)
    if active.dtype != torch.uint8 or not active.is_cuda or tuple(active.shape) != (n,):
        raise ValueError("mask must be a CUDA bool/uint8 tensor of shape (N,)")
    active = active.contiguous()
    return active, active.data_ptr()


def _count_ptr(count: Optional[torch.Tensor]):
    """The pointer of a device-side record count (addDataPropagate's `count`), None without one."""
    if count is None:
        return None
    if count.dtype != torch.int32 or not count.is_cuda:
        raise ValueError("count must be a CUDA int32 tensor")
    return count.data_ptr()


def _lane_ptrs(lane_index: torch.Tensor, lane_count: torch.Tensor, n: int, message: str):
    """The pointers of compactLanes' list for n lanes; `message`: what the caller says about a list that is none."""
    if lane_index.dtype != torch.int32 or lane_count.dtype != torch.int32 or lane_index.numel() < n or lane_count.numel() < 2:
        raise ValueError(message)
    return lane_index.data_ptr(), lane_count.data_ptr()


_GUIDE_LANES = "lane_index must be int32[n], lane_count int32[2] (from compactLanes)"

# Debug switch (the parity tests of the stand-alone entry points set it): synchronise the device behind every library call, so
# that a GPU fault is reported under the call that launched the faulting kernel and not under whatever synchronised next
# (round 2's memory-aperture abort surfaced in exportAccumulators, three launches later: profiles/r03/kd_descend_isa/).
SYNC_EVERY_CALL = False


class PCG32Sampler:
    """Per-lane PCG32 streams laid out like Mitsuba's `independent` sampler (state/inc arrays)."""

    def __init__(self, tree: "SDTree", n: int, seed: int = 0, lane0: int = 0):
        self.n = n
        self.state = tree._new(n, dtype=torch.int64)
        self.inc = tree._new(n, dtype=torch.int64)
        tree._seed(self, seed, lane0)


class SDTree:
    """Both reference trees behind one context: queries read sdTree_prev, recording writes
    sdTree_current; `refineAndPrepare` is path_guiding_integrator.py:566-586."""

    def __init__(self, device: int = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("SDTree needs an MI355X: torch.cuda.is_available() is False and there is no CPU path")
        self._lib = N.lib()
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        N.check(None, self._lib.pg_create(C.byref(h), device))
        self._h = h
        self.store_nee = True
        self._max_depth = 0
        self._pass_lanes = {}  # buffer set -> lanes of its most recent render pass (WavefrontScene.trace_pass; exportPassRecords)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.pg_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _new(self, *shape, dtype=torch.float32) -> torch.Tensor:
        """A fresh output tensor on this tree's device."""
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _ck(self, rc):
        N.check(self._h, rc)
        if SYNC_EVERY_CALL:  # (a fault of an asynchronous kernel then surfaces HERE, under the call that launched it)
            torch.cuda.synchronize(self.device)

    # ---- lifecycle -----------------------------------------------------------------------
    def setup(self, bbox_min, bbox_max, numRays=0, max_depth=0, sdTreeMaxDepth=10, quadTreeMaxDepth=30,
              isStoreNEERadiance=True, bsdfSamplingFraction=0.5):
        bmin = (C.c_float * 3)(*[float(v) for v in bbox_min])
        bmax = (C.c_float * 3)(*[float(v) for v in bbox_max])
        self.store_nee = bool(isStoreNEERadiance)
        self._max_depth = int(max_depth)
        self._ck(self._lib.pg_setup(self._h, bmin, bmax, int(numRays), int(max_depth), int(sdTreeMaxDepth),
                                    int(quadTreeMaxDepth), int(self.store_nee), float(bsdfSamplingFraction)))

    def setIteration(self, iteration: int, isFinalIter: bool = False):
        self._ck(self._lib.pg_set_iteration(self._h, int(iteration), int(bool(isFinalIter))))

    _SPATIAL = {"nearest": N.PG_SPATIAL_NEAREST, "stochastic": N.PG_SPATIAL_STOCHASTIC_BOX, "overlap": N.PG_SPATIAL_OVERLAP_BOX}
    _DIRECTIONAL = {"nearest": N.PG_DIRECTIONAL_NEAREST, "box": N.PG_DIRECTIONAL_BOX}

    def setSplatFilter(self, spatial: str = "nearest", directional: str = "nearest", seed: int = 0):
        """The training filters of the record boundary (pg_set_splat_filter; not in the reference): spatial "nearest" |
        "stochastic" (the position is jittered by the extent of its KD leaf) | "overlap" (the deterministic box the jitter
        estimates: the record is shared between the KD leaves a leaf-sized box around its position overlaps, by volume; no
        seed, exact integer sums whatever the order, batching or sharding), directional "nearest" | "box" (the energy is
        shared between the quadtree leaves a leaf-sized square around the direction overlaps).  addDataPropagate,
        processAndSplat and prepareProcessAndSplat follow it; setup() resets it to nearest / nearest.  While a filter is
        set, a recording render pass raises (the renderer's record list cannot be filtered) unless the scene records the
        vertices' geometry (WavefrontScene(record_geometry=True)): then the pass deposits through the filters, and the
        jitter's record number is the dense slot ray * max_depth + depth."""
        if spatial not in self._SPATIAL:
            raise ValueError(f"spatial filter must be one of {sorted(self._SPATIAL)}, got {spatial!r}")
        if directional not in self._DIRECTIONAL:
            raise ValueError(f"directional filter must be one of {sorted(self._DIRECTIONAL)}, got {directional!r}")
        self._ck(self._lib.pg_set_splat_filter(self._h, self._SPATIAL[spatial], self._DIRECTIONAL[directional],
                                               int(seed) & 0xFFFFFFFF))

    def _seed(self, sampler: PCG32Sampler, seed: int, lane0: int):
        self._ck(self._lib.pg_rng_seed(self._h, sampler.n, seed & 0xFFFFFFFF, lane0 & 0xFFFFFFFF,
                                       sampler.state.data_ptr(), sampler.inc.data_ptr(), _stream_ptr()))

    # ---- queries (kdtree.py:435-496) ------------------------------------------------------
    def getLeafNodeIndex(self, position: torch.Tensor, active: Optional[torch.Tensor] = None) -> torch.Tensor:
        n = position.shape[1]
        _f32(position, (3, n))
        m, mp = _mask(active, n)
        out = self._new(n, dtype=torch.int32)
        self._ck(self._lib.pg_get_leaf_node_index(self._h, n, position.data_ptr(), mp, out.data_ptr(), _stream_ptr()))
        return out

    def sample(self, position: torch.Tensor, sampler: PCG32Sampler, active: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, torch.Tensor]:
        n = position.shape[1]
        _f32(position, (3, n))
        m, mp = _mask(active, n)
        d = self._new(3, n)
        pdf = self._new(n)
        self._ck(self._lib.pg_sample(self._h, n, position.data_ptr(), sampler.state.data_ptr(), sampler.inc.data_ptr(),
                                     mp, d.data_ptr(), pdf.data_ptr(), _stream_ptr()))
        return d, pdf

    def pdf(self, position: torch.Tensor, direction: torch.Tensor, active: Optional[torch.Tensor] = None) -> torch.Tensor:
        n = position.shape[1]
        _f32(position, (3, n))
        _f32(direction, (3, n))
        m, mp = _mask(active, n)
        pdf = self._new(n)
        self._ck(self._lib.pg_pdf(self._h, n, position.data_ptr(), direction.data_ptr(), mp, pdf.data_ptr(), _stream_ptr()))
        return pdf

    def guideBounce(self, position, dir_nee, nee_active, select, dir_io, sampler: PCG32Sampler,
                    pdf_nee_out=None, pdf_out=None, lane_index=None, lane_count=None):
        """The three SD-tree calls of one bounce with one KD descent (pg_guide_bounce).
        lane_index/lane_count: compacted live-ray list from compactLanes (optional)."""
        self.prepareGuideBounce(position, dir_nee, nee_active, select, dir_io, sampler, pdf_nee_out, pdf_out,
                                lane_index, lane_count)()
        return self._last_bounce_out

    def prepareGuideBounce(self, position, dir_nee, nee_active, select, dir_io, sampler: PCG32Sampler,
                           pdf_nee_out=None, pdf_out=None, lane_index=None, lane_count=None):
        """Validates once and returns a zero-argument callable that launches pg_guide_bounce on the
        current stream with the argument list already marshalled (a wavefront loop re-launches the
        same buffers every bounce of every pass; per-call checks would dominate a 30 us kernel)."""
        n = position.shape[1]
        _f32(position, (3, n)); _f32(dir_nee, (3, n)); _f32(dir_io, (3, n))
        na, nap = _mask(nee_active, n)
        sl, slp = _mask(select, n)
        if pdf_nee_out is None:
            pdf_nee_out = self._new(n)
        if pdf_out is None:
            pdf_out = self._new(n)
        if (lane_index is None) != (lane_count is None):
            raise ValueError("lane_index and lane_count go together")
        lip, lcp = (None, None) if lane_index is None else _lane_ptrs(lane_index, lane_count, n, _GUIDE_LANES)
        keep = (position, dir_nee, na, sl, dir_io, sampler, pdf_nee_out, pdf_out, lane_index, lane_count)
        self._last_bounce_out = (pdf_nee_out, pdf_out)
        fn, h = self._lib.pg_guide_bounce, self._h
        args = (h, n, position.data_ptr(), dir_nee.data_ptr(), nap, slp, dir_io.data_ptr(), sampler.state.data_ptr(),
                sampler.inc.data_ptr(), pdf_nee_out.data_ptr(), pdf_out.data_ptr(), lip, lcp)
        ck = self._ck

        def launch(_keep=keep):
            ck(fn(*args, torch.cuda.current_stream().cuda_stream))
        return launch

    # ---- sample warping (include/pgsd_warp.h; not in the reference) -------------------------
    def sampleWarp(self, position: torch.Tensor, u: torch.Tensor, active: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
        """The caller's 2-D points u (float32 (2, N), in [0,1)^2) warped through the quadtree of the KD leaf that holds each
        position (pg_sample_warp): (direction (3, N), pdf (N,)).  The pdf is what pdf() returns for the direction."""
        n = position.shape[1]
        _f32(position, (3, n))
        _f32(u, (2, n))
        m, mp = _mask(active, n)
        d = self._new(3, n)
        pdf = self._new(n)
        self._ck(self._lib.pg_sample_warp(self._h, n, position.data_ptr(), u.data_ptr(), mp, d.data_ptr(), pdf.data_ptr(),
                                          _stream_ptr()))
        return d, pdf

    def invertWarp(self, position: torch.Tensor, direction: torch.Tensor, active: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
        """The inverse of sampleWarp (pg_invert_warp): (u (2, N), pdf (N,)).  A direction of zero probability has no preimage:
        its u is the limit point of the empty preimage and its pdf is 0."""
        n = position.shape[1]
        _f32(position, (3, n))
        _f32(direction, (3, n))
        m, mp = _mask(active, n)
        u = self._new(2, n)
        pdf = self._new(n)
        self._ck(self._lib.pg_invert_warp(self._h, n, position.data_ptr(), direction.data_ptr(), mp, u.data_ptr(), pdf.data_ptr(),
                                          _stream_ptr()))
        return u, pdf

    def guideBounceWarp(self, position, dir_nee, nee_active, select, dir_io, u, pdf_nee_out=None, pdf_out=None,
                        lane_index=None, lane_count=None):
        """guideBounce with the select == 2 lanes' directions warped from u (float32 (2, N)) instead of drawn from a sampler
        (pg_guide_bounce_warp)."""
        n = position.shape[1]
        _f32(position, (3, n)); _f32(dir_nee, (3, n)); _f32(dir_io, (3, n)); _f32(u, (2, n))
        na, nap = _mask(nee_active, n)
        sl, slp = _mask(select, n)
        if pdf_nee_out is None:
            pdf_nee_out = self._new(n)
        if pdf_out is None:
            pdf_out = self._new(n)
        if (lane_index is None) != (lane_count is None):
            raise ValueError("lane_index and lane_count go together")
        lip, lcp = (None, None) if lane_index is None else _lane_ptrs(lane_index, lane_count, n, _GUIDE_LANES)
        self._ck(self._lib.pg_guide_bounce_warp(self._h, n, position.data_ptr(), dir_nee.data_ptr(), nap, slp, dir_io.data_ptr(),
                                                u.data_ptr(), pdf_nee_out.data_ptr(), pdf_out.data_ptr(), lip, lcp, _stream_ptr()))
        return pdf_nee_out, pdf_out

    # ---- the BSDF sampling fraction learned per KD leaf (include/pgsd_fraction.h; not in the reference) ----------------
    _LOSS = {"kl": N.PG_FRACTION_LOSS_KL, "variance": N.PG_FRACTION_LOSS_VARIANCE}

    def fractionEnable(self, fraction0: float = 0.5, learning_rate: float = 0.01, beta1: float = 0.9, beta2: float = 0.999,
                       epsilon: float = 1e-8, l2: float = 0.01, loss: str = "kl"):
        """Switches the learned fraction on with every leaf at fraction0 (pg_fraction_enable): theta0 = log(f / (1 - f)), 0 for
        0.5.  The defaults are the publication's, chosen there for one Adam step per record; nobody has measured which
        learning rate suits the batch step of fractionStep.  setup() and load() switch the feature off."""
        if loss not in self._LOSS:
            raise ValueError(f"loss must be one of {sorted(self._LOSS)}, got {loss!r}")
        if not 0.0 < fraction0 < 1.0:
            raise ValueError("fraction0 must lie strictly between 0 and 1")
        theta0 = 0.0 if fraction0 == 0.5 else float(np.log(fraction0 / (1.0 - fraction0)))
        prm = N.pg_fraction_params(max(-20.0, min(20.0, theta0)), learning_rate, beta1, beta2, epsilon, l2, self._LOSS[loss])
        self._ck(self._lib.pg_fraction_enable(self._h, C.byref(prm)))

    def fractionDisable(self):
        self._ck(self._lib.pg_fraction_enable(self._h, None))

    def fractionQuery(self, position: torch.Tensor, active: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The BSDF sampling fraction of the KD leaf that holds each position (pg_fraction_query), float32 (N,)."""
        n = position.shape[1]
        _f32(position, (3, n))
        m, mp = _mask(active, n)
        out = self._new(n)
        self._ck(self._lib.pg_fraction_query(self._h, n, position.data_ptr(), mp, out.data_ptr(), _stream_ptr()))
        return out

    def fractionRecord(self, rec: Dict[str, torch.Tensor], count: Optional[torch.Tensor] = None):
        """Adds the records' gradients to their leaves' accumulators (pg_fraction_record).  rec: position (3, M); bsdf_pdf,
        guide_pdf, product, wo_pdf (M,); optionally is_delta (M,) bool / uint8.  count: as addDataPropagate's."""
        m = rec["position"].shape[1]
        r = N.pg_fraction_records()
        r.position = _f32(rec["position"], (3, m)).data_ptr()
        for k in ("bsdf_pdf", "guide_pdf", "product", "wo_pdf"):
            setattr(r, k, _f32(rec[k], (m,)).data_ptr())
        delta, r.is_delta = _mask(rec.get("is_delta"), m)
        self._ck(self._lib.pg_fraction_record(self._h, m, C.byref(r), _count_ptr(count), _stream_ptr()))

    def fractionStep(self):
        """One Adam step for every leaf that received records since the last one (pg_fraction_step)."""
        self._ck(self._lib.pg_fraction_step(self._h, _stream_ptr()))

    def fractionAccumulators(self) -> torch.Tensor:
        """int64 view of the gradient accumulators (n_roots * 4 words), for an element-wise sum over ranks before fractionStep."""
        p = C.c_void_p()
        n = C.c_uint64()
        self._ck(self._lib.pg_fraction_accumulators(self._h, C.byref(p), C.byref(n)))
        return _wrap_device_i64(p.value, n.value, self.device)

    def fractionState(self) -> Dict[str, np.ndarray]:
        """The per-leaf state (pg_fraction_export): theta, m, v, p1, p2 (float32), steps (uint32), acc (int64 (n_roots, 4)),
        indexed by the tree number export() writes in kdtree_quadTreeRootIndex."""
        n = int(self.sizes().n_roots)
        st = {k: np.empty(n, np.float32) for k in ("theta", "m", "v", "p1", "p2")}
        st["steps"] = np.empty(n, np.uint32)
        st["acc"] = np.empty((n, 4), np.int64)
        self._ck(self._lib.pg_fraction_export(self._h, n, *[st[k].ctypes.data for k in ("theta", "m", "v", "p1", "p2", "steps", "acc")]))
        return st

    def fractionLoadState(self, st: Dict[str, np.ndarray]):
        """Loads theta, m, v, p1, p2 and steps (pg_fraction_import); the accumulators become zero."""
        a = [np.ascontiguousarray(st[k], np.float32) for k in ("theta", "m", "v", "p1", "p2")]
        a.append(np.ascontiguousarray(st["steps"], np.uint32))
        n = a[0].shape[0]
        if any(x.shape != (n,) for x in a):
            raise ValueError("theta, m, v, p1, p2 and steps must have one entry per leaf")
        self._ck(self._lib.pg_fraction_import(self._h, n, *[x.ctypes.data for x in a]))

    # ---- light selection learned per KD leaf (include/ext/pg_lights.h; not in the reference) -------------------------------
    def lightsEnable(self, n_lights: int, delta: float = 0.1, root: bool = False):
        """Switches the learned light selection on for lights 0 .. n_lights - 1 with every leaf unlearned (pg_lights_enable).
        delta: the share of the uniform choice on a learned leaf; root: weights follow the square roots of the recorded means
        (record squared contributions for the variance-aware target).  setup() and load() switch the feature off."""
        if int(n_lights) < 1:
            raise ValueError("n_lights must be at least 1 (lightsDisable switches the feature off)")
        prm = N.pg_lights_params(float(delta), int(bool(root)), 0)
        self._ck(self._lib.pg_lights_enable(self._h, int(n_lights), C.byref(prm)))

    def lightsDisable(self):
        self._ck(self._lib.pg_lights_enable(self._h, 0, None))

    def lightsSample(self, position: torch.Tensor, u: Optional[torch.Tensor] = None, sampler: Optional[PCG32Sampler] = None,
                     active: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """A light for each position from the row of its KD leaf (pg_lights_sample): (light int32 (N,), pmf float32 (N,)).
        u: float32 (N,) in [0, 1), or None to draw one number from `sampler`.  Inactive lanes get light -1 and pmf 0."""
        n = position.shape[1]
        _f32(position, (3, n))
        if (u is None) == (sampler is None):
            raise ValueError("give either u or a sampler")
        up = None if u is None else _f32(u, (n,)).data_ptr()
        sp, ip = (None, None) if sampler is None else (sampler.state.data_ptr(), sampler.inc.data_ptr())
        if sampler is not None and sampler.n < n:
            raise ValueError("the sampler has fewer streams than there are positions")
        m, mp = _mask(active, n)
        light = self._new(n, dtype=torch.int32)
        pmf = self._new(n)
        self._ck(self._lib.pg_lights_sample(self._h, n, position.data_ptr(), up, sp, ip, mp, light.data_ptr(), pmf.data_ptr(),
                                            _stream_ptr()))
        return light, pmf

    def lightsPmf(self, position: torch.Tensor, light: torch.Tensor, active: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The probability lightsSample gives each light at each position (pg_lights_pmf), float32 (N,); light: int32 (N,)."""
        n = position.shape[1]
        _f32(position, (3, n))
        if light.dtype != torch.int32 or not light.is_cuda or not light.is_contiguous() or tuple(light.shape) != (n,):
            raise ValueError("light must be a contiguous CUDA int32 tensor of shape (N,)")
        m, mp = _mask(active, n)
        pmf = self._new(n)
        self._ck(self._lib.pg_lights_pmf(self._h, n, position.data_ptr(), light.data_ptr(), mp, pmf.data_ptr(), _stream_ptr()))
        return pmf

    def lightsRecord(self, rec: Dict[str, torch.Tensor], count: Optional[torch.Tensor] = None):
        """Adds the records' contributions to the accumulators of (leaf, light) (pg_lights_record).  rec: position (3, M), light
        int32 (M,), value (M,): the NEE contribution estimate before the division by the selection probability.  count: as
        addDataPropagate's."""
        m = rec["position"].shape[1]
        light = rec["light"]
        if light.dtype != torch.int32 or not light.is_cuda or not light.is_contiguous() or tuple(light.shape) != (m,):
            raise ValueError("light must be a contiguous CUDA int32 tensor of shape (M,)")
        r = N.pg_lights_records()
        r.position = _f32(rec["position"], (3, m)).data_ptr()
        r.light = light.data_ptr()
        r.value = _f32(rec["value"], (m,)).data_ptr()
        self._ck(self._lib.pg_lights_record(self._h, m, C.byref(r), _count_ptr(count), _stream_ptr()))

    def lightsBuild(self):
        """Every leaf that has recorded energy gets its row from its accumulators, which stay (pg_lights_build)."""
        self._ck(self._lib.pg_lights_build(self._h, _stream_ptr()))

    def lightsAccumulators(self) -> torch.Tensor:
        """int64 view of the accumulators (n_roots * n_lights * 4 words, leaf-major then light), for an element-wise sum over
        ranks before lightsBuild."""
        p = C.c_void_p()
        n = C.c_uint64()
        self._ck(self._lib.pg_lights_accumulators(self._h, C.byref(p), C.byref(n)))
        return _wrap_device_i64(p.value, n.value, self.device)

    def lightsStatus(self) -> Tuple[int, int]:
        """(n_lights, leaves that have learned a row) -- (0, 0) while the feature is off (pg_lights_status)."""
        n, k = C.c_uint32(), C.c_uint64()
        self._ck(self._lib.pg_lights_status(self._h, C.byref(n), C.byref(k)))
        return int(n.value), int(k.value)

    def lightsState(self) -> Dict[str, np.ndarray]:
        """The per-leaf state (pg_lights_export): rows uint32 (n_roots, n_lights), acc int64 (n_roots, n_lights, 4), indexed by
        the tree number export() writes in kdtree_quadTreeRootIndex."""
        n, L = int(self.sizes().n_roots), self.lightsStatus()[0]
        st = {"rows": np.empty((n, L), np.uint32), "acc": np.empty((n, L, 4), np.int64)}
        self._ck(self._lib.pg_lights_export(self._h, n, L, st["rows"].ctypes.data, st["acc"].ctypes.data))
        return st

    def lightsLoadState(self, st: Dict[str, np.ndarray]):
        """Loads the rows (pg_lights_import); the accumulators become zero."""
        rows = np.ascontiguousarray(st["rows"], np.uint32)
        if rows.ndim != 2:
            raise ValueError("rows must have shape (n_roots, n_lights)")
        self._ck(self._lib.pg_lights_import(self._h, rows.shape[0], rows.shape[1], rows.ctypes.data))

    # ---- resampled next-event estimation (include/ext/lights/pg_nee.h; not in the reference) -------------------------------
    def lightsSetGeometry(self, table: Optional[Dict[str, np.ndarray]]):
        """Gives the context the lights' geometry (pg_nee_set_lights), light j being light j of lightsEnable.  table: numpy
        arrays origin, edge_a, edge_b (L, 3), radiance (L,) (a scalar per light, such as the luminance of its emitted radiance),
        triangle (L,) bool (else a parallelogram), two_sided (L,) bool.  None, or a table of no lights, frees it.  The table
        stays through setup(), load() and refineAndPrepare(); setting it again replaces it."""
        if table is None or len(table["radiance"]) == 0:
            self._ck(self._lib.pg_nee_set_lights(self._h, 0, None, _stream_ptr()))
            return
        L = len(table["radiance"])
        words = np.zeros((L, N.PG_NEE_TABLE_WORDS), np.float32)
        for k, name in enumerate(("origin", "edge_a", "edge_b")):
            v = np.asarray(table[name], np.float32)
            if v.shape != (L, 3):
                raise ValueError(f"{name} must have shape (L, 3)")
            words[:, 3 * k:3 * k + 3] = v
        for name in ("radiance", "triangle", "two_sided"):
            if np.shape(table[name]) != (L,):
                raise ValueError(f"{name} must have shape (L,)")
        words[:, 9] = np.asarray(table["radiance"], np.float32)
        bits = words.view(np.uint32)
        bits[:, 10] = np.asarray(table["triangle"]).astype(bool)
        bits[:, 11] = np.asarray(table["two_sided"]).astype(bool)
        self._ck(self._lib.pg_nee_set_lights(self._h, L, words.ctypes.data, _stream_ptr()))

    def lightsGeometryStatus(self) -> int:
        """The number of lights of the geometry table, 0 when none is set (pg_nee_status)."""
        n = C.c_uint32()
        self._ck(self._lib.pg_nee_status(self._h, C.byref(n)))
        return int(n.value)

    def lightsResample(self, position: torch.Tensor, normal: torch.Tensor, sampler: PCG32Sampler, candidates: int = 8,
                       active: Optional[torch.Tensor] = None, return_candidates: bool = False
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Dict[str, torch.Tensor]]:
        """(light int32 (N,), point float32 (3, N), weight float32 (N,), info) (pg_nee_resample): a light and a point on it in
        proportion to the unshadowed contribution at a diffuse surface with `normal` (used as given), by resampled importance
        sampling -- `candidates` draws of a light from the row of the position's KD leaf (lightsSample's selection) and a
        uniform point on it, one kept in proportion to target over source.  Needs lightsEnable and lightsSetGeometry with the
        same number of lights.  The estimator is f(point) * weight, f the whole integrand in area measure (emitted radiance,
        BSDF, both cosines over the squared distance, and the visibility of the ONE shadow ray the host traces); weight is 0 and
        light -1 where nothing could be kept.  One kernel, one KD descent.  info: {"direction" float32 (3, N), "distance",
        "target", "source" float32 (N,), "index" int32 (N,) (the bits of a uint32: the kept candidate, 0xFFFFFFFF if none)};
        with return_candidates also {"cand_light" int32 (M, N), "cand_point" float32 (M, 3, N), "cand_target", "cand_source"
        float32 (M, N)}, what a host with another BSDF resamples itself.  Every served lane's stream advances by 4 * candidates
        draws."""
        n = position.shape[1]
        _f32(position, (3, n)); _f32(normal, (3, n))
        a = N.pg_nee_args()
        light, point, dist = self._new(n, dtype=torch.int32), self._new(3, n), self._new(n)
        a.light_out, a.point_out, a.dist_out = light.data_ptr(), point.data_ptr(), dist.data_ptr()
        d, w, info = self._resample(self._lib.pg_nee_resample, a, (N.pg_nee_params,), position, normal, sampler, candidates, active,
                                    return_candidates, lead=(("cand_light", torch.int32), ("cand_point", torch.float32, 3)))
        return light, point, w, {"direction": d, "distance": dist, **info}

    def compactLanes(self, select: torch.Tensor, nee_active: Optional[torch.Tensor] = None,
                     idx_out: Optional[torch.Tensor] = None, count_out: Optional[torch.Tensor] = None):
        """Active-ray stream compaction (pg_compact_lanes): returns (idx int32[n], counts int32[2]);
        idx[:counts[0]] are the select==2 lanes, idx[n-counts[1]:] (reversed) the other live lanes."""
        self.prepareCompactLanes(select, nee_active, idx_out, count_out)()
        return self._last_compact_out

    def prepareCompactLanes(self, select: torch.Tensor, nee_active=None, idx_out=None, count_out=None):
        n = select.shape[0]
        s, sp = _mask(select, n)
        ne, nep = _mask(nee_active, n)
        if idx_out is None:
            idx_out = self._new(max(n, 1), dtype=torch.int32)
        if count_out is None:
            count_out = torch.zeros(2, dtype=torch.int32, device=self.device)
        if count_out.numel() < 2 or count_out.dtype != torch.int32:
            raise ValueError("count_out must be int32[2]")
        self._last_compact_out = (idx_out, count_out)
        fn, h, ck = self._lib.pg_compact_lanes, self._h, self._ck
        args = (h, n, sp, nep, idx_out.data_ptr(), count_out.data_ptr())

        def launch(_keep=(s, ne, idx_out, count_out)):
            ck(fn(*args, torch.cuda.current_stream().cuda_stream))
        return launch

    # ---- recording (kdtree.py:180-225) ----------------------------------------------------
    def addDataPropagate(self, rec: Dict[str, torch.Tensor], count: Optional[torch.Tensor] = None):
        """rec: position (3,M), direction (2,M), radiance (M,), woPdf (M,), direction_nee (2,M),
        radiance_nee_lum (M,) -- the stream scatterDataIntoSDTree hands to the tree."""
        m = rec["position"].shape[1]
        r = N.pg_records()
        r.position = _f32(rec["position"], (3, m)).data_ptr()
        r.direction = _f32(rec["direction"], (2, m)).data_ptr()
        r.radiance = _f32(rec["radiance"], (m,)).data_ptr()
        r.wo_pdf = _f32(rec["woPdf"], (m,)).data_ptr()
        if self.store_nee:
            r.direction_nee = _f32(rec["direction_nee"], (2, m)).data_ptr()
            r.radiance_nee_lum = _f32(rec["radiance_nee_lum"], (m,)).data_ptr()
        self._ck(self._lib.pg_splat(self._h, m, C.byref(r), _count_ptr(count), _stream_ptr()))

    # ---- the variance-aware guiding target (include/pgsd_target.h; not in the reference) ---------------------------------
    _TARGET = {"second_moment": N.PG_TARGET_SECOND_MOMENT}

    def addSecondMoments(self, rec: Dict[str, torch.Tensor], count: Optional[torch.Tensor] = None):
        """addDataPropagate of the records' SECOND moments: radiance and radiance_nee_lum are squared (x * x in fp32, one
        rounding each; the caller's tensors are not written), every other column and the splat filters apply unchanged.
        Follow the iteration's last record (and the multi-GPU sum) by applyTarget("second_moment"), then refineAndPrepare."""
        sq = dict(rec)
        for k in ("radiance", "radiance_nee_lum"):
            if k in rec:
                sq[k] = _f32(rec[k], (rec["position"].shape[1],)) * rec[k]
        self.addDataPropagate(sq, count)

    def applyTarget(self, target: str = "second_moment"):
        """pg_target_apply: every directional leaf's sum S of sdTree_current becomes 2^-depth * sqrt(S), in place, on the current
        stream.  Once per iteration, after the last record and after the sum over ranks, before refineAndPrepare; a second
        call before the refine raises and changes nothing."""
        if target not in self._TARGET:
            raise ValueError(f"target must be one of {sorted(self._TARGET)}, got {target!r}")
        self._ck(self._lib.pg_target_apply(self._h, self._TARGET[target], _stream_ptr()))

    @property
    def targetApplied(self) -> Optional[str]:
        """The target applied to the running iteration's accumulators ("second_moment"), or None: cleared by refineAndPrepare,
        setup and load (pg_target_applied)."""
        out = C.c_int32(0)
        self._ck(self._lib.pg_target_applied(self._h, C.byref(out)))
        return next((k for k, v in self._TARGET.items() if v == out.value), None)

    # ---- radiance estimates and guided Russian roulette / splitting (include/pgsd_radiance.h; not in the reference) ------
    def radianceEnable(self, on: bool = True):
        """Switches the quadtrees' statistical weights on (pg_radiance_enable): from the next refineAndPrepare on, every
        quadtree of sdTree_prev knows how many records its energies were resolved from, and radianceEstimate /
        radianceRoulette answer.  Until then (or radianceLoadWeights) the weights are unknown and both raise.  setup() and
        load() switch the feature off."""
        self._ck(self._lib.pg_radiance_enable(self._h, int(bool(on))))

    def radianceStatus(self) -> Dict[str, object]:
        """{"enabled": bool, "valid": bool, "of_target": None | "second_moment"} (pg_radiance_status)."""
        e, v, t = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._ck(self._lib.pg_radiance_status(self._h, C.byref(e), C.byref(v), C.byref(t)))
        return {"enabled": bool(e.value), "valid": bool(v.value),
                "of_target": next((k for k, x in self._TARGET.items() if x == t.value), None)}

    def radianceWeights(self) -> np.ndarray:
        """uint64 (n_roots,): the number of records behind every quadtree of sdTree_prev (pg_radiance_export), indexed by
        the tree number export() writes in kdtree_quadTreeRootIndex."""
        n = int(self.sizes().n_roots)
        w = np.empty(n, np.uint64)
        self._ck(self._lib.pg_radiance_export(self._h, n, w.ctypes.data))
        return w

    def radianceLoadWeights(self, w):
        """Loads the weights of a tree that came from a file (pg_radiance_import), one per quadtree."""
        w = np.ascontiguousarray(w, np.uint64)
        if w.ndim != 1:
            raise ValueError("one weight per quadtree")
        self._ck(self._lib.pg_radiance_import(self._h, w.shape[0], w.ctypes.data))

    def radianceEstimate(self, position: torch.Tensor, direction: Optional[torch.Tensor] = None,
                         active: Optional[torch.Tensor] = None) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        """(L_dir, L_mean), float32 (N,) each (pg_radiance_query): the radiance arriving at `position` from `direction`, and
        its mean over the sphere.  direction=None: L_dir is None, only the mean is computed and no quadtree is walked."""
        n = position.shape[1]
        _f32(position, (3, n))
        m, mp = _mask(active, n)
        L_mean = self._new(n)
        L_dir, dp, lp = None, None, None
        if direction is not None:
            dp = _f32(direction, (3, n)).data_ptr()
            L_dir = self._new(n)
            lp = L_dir.data_ptr()
        self._ck(self._lib.pg_radiance_query(self._h, n, position.data_ptr(), dp, mp, lp, L_mean.data_ptr(), _stream_ptr()))
        return L_dir, L_mean

    def radianceRoulette(self, position: torch.Tensor, direction: torch.Tensor, weight: torch.Tensor, reference: torch.Tensor,
                         sampler: PCG32Sampler, window: float = 5.0, max_split: int = 1, active: Optional[torch.Tensor] = None
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(count int32 (N,), scale float32 (N,), L_dir float32 (N,)) (pg_radiance_rr): adjoint-driven Russian roulette and
        splitting.  weight: the paths' throughput (a luminance) behind the bounce; reference: the estimate of their pixels'
        values.  A path goes on `count` times (0: it ends) with its throughput multiplied by `scale`; E[count * scale] = 1.
        One draw of `sampler` per active lane.  max_split=1: roulette only."""
        return self._roulette(self._lib.pg_radiance_rr, position, direction, False, weight, reference, sampler, window, max_split,
                              active)

    def _roulette(self, fn, position, around, around_optional: bool, weight, reference, sampler, window, max_split, active):
        """radianceRoulette / irradianceRoulette: `fn` decides on its estimate around the direction or the normal `around`."""
        n = position.shape[1]
        _f32(position, (3, n))
        ap = None if around is None and around_optional else _f32(around, (3, n)).data_ptr()
        _f32(weight, (n,))
        _f32(reference, (n,))
        if sampler.n != n:
            raise ValueError("the sampler must have one stream per lane")
        m, mp = _mask(active, n)
        count, scale, estimate = self._new(n, dtype=torch.int32), self._new(n), self._new(n)
        prm = N.pg_rr_params(float(window), int(max_split))
        self._ck(fn(self._h, n, position.data_ptr(), ap, weight.data_ptr(), reference.data_ptr(), C.byref(prm),
                    sampler.state.data_ptr(), sampler.inc.data_ptr(), mp, count.data_ptr(), scale.data_ptr(), estimate.data_ptr(),
                    _stream_ptr()))
        return count, scale, estimate

    # ---- irradiance estimates per spatial leaf (include/pgsd_irradiance.h; not in the reference) -----------------------------
    def irradianceBuild(self):
        """Projects every quadtree of sdTree_prev onto the nine spherical harmonics up to order 2 (pg_irradiance_build): needs
        radianceEnable and known weights.  Whatever replaces the tree or its weights (refineAndPrepare, setup, load,
        radianceEnable(False), radianceLoadWeights) discards the table."""
        self._ck(self._lib.pg_irradiance_build(self._h, _stream_ptr()))

    def irradianceStatus(self) -> bool:
        """True while the table describes sdTree_prev (pg_irradiance_status)."""
        b = C.c_int32(0)
        self._ck(self._lib.pg_irradiance_status(self._h, C.byref(b)))
        return bool(b.value)

    def irradianceCoefficients(self) -> np.ndarray:
        """float32 (n_roots, 9): the coefficients of every quadtree (pg_irradiance_export), indexed like radianceWeights."""
        n = int(self.sizes().n_roots)
        k = np.empty((n, 9), np.float32)
        self._ck(self._lib.pg_irradiance_export(self._h, n, k.ctypes.data))
        return k

    def irradianceLoadCoefficients(self, k):
        """Loads the coefficients of a tree that came from a file (pg_irradiance_import), nine per quadtree."""
        k = np.ascontiguousarray(k, np.float32)
        if k.ndim != 2 or k.shape[1] != 9:
            raise ValueError("nine coefficients per quadtree")
        self._ck(self._lib.pg_irradiance_import(self._h, k.shape[0], k.ctypes.data))

    def irradianceEstimate(self, position: torch.Tensor, normal: Optional[torch.Tensor] = None,
                           active: Optional[torch.Tensor] = None) -> torch.Tensor:
        """E float32 (N,) (pg_irradiance_query): the integral of the radiance arriving at `position` against the cosine around
        `normal` (used as given: unit length is the caller's business).  normal=None: the mean over all orientations."""
        n = position.shape[1]
        _f32(position, (3, n))
        m, mp = _mask(active, n)
        np_ = _f32(normal, (3, n)).data_ptr() if normal is not None else None
        E = self._new(n)
        self._ck(self._lib.pg_irradiance_query(self._h, n, position.data_ptr(), np_, mp, E.data_ptr(), _stream_ptr()))
        return E

    def irradianceRoulette(self, position: torch.Tensor, normal: Optional[torch.Tensor], weight: torch.Tensor,
                           reference: torch.Tensor, sampler: PCG32Sampler, window: float = 5.0, max_split: int = 1,
                           active: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(count int32 (N,), scale float32 (N,), E float32 (N,)) (pg_irradiance_rr): radianceRoulette's decision on the
        irradiance estimate, before a direction is sampled.  weight: the paths' throughput with rho / pi folded in.  One draw
        of `sampler` per active lane."""
        return self._roulette(self._lib.pg_irradiance_rr, position, normal, True, weight, reference, sampler, window, max_split,
                              active)

    # ---- a whole guided bounce behind one KD descent (include/pgsd_bounce.h; not in the reference) -------------------------
    def bounce(self, position, dir_nee, nee_active, dir_io, mode=None, u_select=None, sampler: Optional[PCG32Sampler] = None,
               u=None, lanes=None, radiance: bool = False, out: Optional[Dict[str, torch.Tensor]] = None
               ) -> Dict[str, torch.Tensor]:
        """fractionQuery, the selection u_select > f, guideBounce / guideBounceWarp and radianceEstimate of the continuation
        direction as ONE kernel (pg_bounce); every output is what that sequence gives, bit for bit.
        mode: uint8 (N,) of N.PG_BOUNCE_NONE / PDF / SAMPLE / CHOOSE (None: every lane chooses on the device from its leaf's
        fraction).  u_select: float32 (N,), the numbers the CHOOSE lanes compare with the fraction (None: one draw of
        `sampler` per CHOOSE lane, PCG32 form only).  sampler: the lanes' PCG32 streams (the PCG32 form); u: float32 (2, N),
        the warp form (guideBounceWarp's u).  lanes: (lane_index, lane_count) from compactLanes(mode, nee_active).
        dir_io is written in place where a lane samples.  radiance=True also returns L_dir and L_mean (radianceEnable first).
        Returns {"select" uint8, "fraction", "pdf_nee", "pdf" float32 (N,)} (+ "L_dir", "L_mean"); `out` may bring any of these
        tensors pre-allocated (with a list, slots that are not listed keep their contents)."""
        n = position.shape[1]
        _f32(position, (3, n)); _f32(dir_nee, (3, n)); _f32(dir_io, (3, n))
        na, nap = _mask(nee_active, n)
        md, mdp = _mask(mode, n)
        a = N.pg_bounce_args()
        a.p, a.dir_nee, a.dir_io, a.nee_active, a.mode = position.data_ptr(), dir_nee.data_ptr(), dir_io.data_ptr(), nap, mdp
        if u_select is not None:
            a.u_select = _f32(u_select, (n,)).data_ptr()
        if u is not None:
            a.u = _f32(u, (2, n)).data_ptr()
        if sampler is not None:
            if sampler.n != n:
                raise ValueError("the sampler must have one stream per lane")
            a.rng_state, a.rng_inc = sampler.state.data_ptr(), sampler.inc.data_ptr()
        if lanes is not None:
            lane_index, lane_count = lanes
            a.lane_index, a.d_lane_count = _lane_ptrs(lane_index, lane_count, n,
                                                      "lanes must be (int32[n], int32[2]) (from compactLanes)")
        res = dict(out) if out else {}
        names = ("select", "fraction", "pdf_nee", "pdf") + (("L_dir", "L_mean") if radiance else ())
        for k in names:
            dt = torch.uint8 if k == "select" else torch.float32
            if k not in res:
                res[k] = torch.empty(n, dtype=dt, device=self.device)
            elif res[k].dtype != dt or not res[k].is_cuda or not res[k].is_contiguous() or tuple(res[k].shape) != (n,):
                raise ValueError(f"out[{k!r}] must be a contiguous CUDA {dt} tensor of shape ({n},)")
        a.select_out, a.fraction_out = res["select"].data_ptr(), res["fraction"].data_ptr()
        a.pdf_nee_out, a.pdf_out = res["pdf_nee"].data_ptr(), res["pdf"].data_ptr()
        if radiance:
            a.L_dir_out, a.L_mean_out = res["L_dir"].data_ptr(), res["L_mean"].data_ptr()
        self._ck(self._lib.pg_bounce(self._h, n, C.byref(a), _stream_ptr()))
        return {k: res[k] for k in names}

    # ---- product guiding for diffuse surfaces (include/pg_resample.h; not in the reference) --------------------------------
    def resampleCosine(self, position: torch.Tensor, normal: torch.Tensor, sampler: PCG32Sampler, candidates: int = 8,
                       alpha: float = 0.5, delta: float = 0.1, active: Optional[torch.Tensor] = None,
                       return_candidates: bool = False) -> Tuple[torch.Tensor, torch.Tensor, Dict[str, torch.Tensor]]:
        """(direction float32 (3, N), weight float32 (N,), info) (pg_resample_cosine): a direction in proportion to the
        tree's radiance times the cosine about `normal` (used as given), by resampled importance sampling -- `candidates`
        draws from the mixture of the cosine lobe (share `alpha`) and the tree, one kept in proportion to target over source;
        the target is the cosine times (delta / 4 pi + (1 - delta) * the tree's density).  The estimator is
        f(direction) * weight with f the whole integrand; weight is 0 where nothing could be kept.  One kernel, one KD descent.
        info: {"target", "source" float32 (N,), "index" int32 (N,) (the bits of a uint32: the kept candidate, 0xFFFFFFFF
        if none)}; with return_candidates also {"cand_dir" float32 (M, 3, N), "cand_target", "cand_source" float32 (M, N)},
        what a host with another BSDF resamples itself.  The lanes' streams advance by the candidates' draws."""
        n = position.shape[1]
        _f32(position, (3, n)); _f32(normal, (3, n))
        return self._resample(self._lib.pg_resample_cosine, N.pg_resample_args(), (N.pg_resample_params, float(alpha), float(delta), 0),
                              position, normal, sampler, candidates, active, return_candidates)

    def resampleLobe(self, position: torch.Tensor, normal: torch.Tensor, wi: torch.Tensor, roughness: torch.Tensor,
                     specular: torch.Tensor, sampler: PCG32Sampler, candidates: int = 8, alpha: float = 0.5, delta: float = 0.1,
                     active: Optional[torch.Tensor] = None,
                     return_candidates: bool = False) -> Tuple[torch.Tensor, torch.Tensor, Dict[str, torch.Tensor]]:
        """(direction float32 (3, N), weight float32 (N,), info) (pg_resample_lobe): a direction in proportion to the tree's
        radiance times a glossy lobe about `normal`, by resampled importance sampling -- `candidates` draws from the mixture
        of the lobe (share `alpha`) and the tree, one kept in proportion to target over source.  The lobe of a lane is
        specular * (the GGX visible-normal density of reflecting `wi`, the world direction towards the viewer, at `roughness`
        in [1e-3, 1]) + (1 - specular) * the clamped cosine; `roughness` and `specular` are float32 (N,), all vectors are used
        as given.  The target is the lobe times (delta / 4 pi + (1 - delta) * the tree's density).  The estimator is
        f(direction) * weight with f the whole integrand; weight is 0 where nothing could be kept, and on lanes whose inputs
        the header calls invalid.  One kernel, one KD descent.  info is resampleCosine's: {"target", "source" float32 (N,),
        "index" int32 (N,)}; with return_candidates also {"cand_dir" float32 (M, 3, N), "cand_target", "cand_source" float32
        (M, N)}.  The lanes' streams advance by the candidates' draws."""
        n = position.shape[1]
        _f32(position, (3, n)); _f32(normal, (3, n)); _f32(wi, (3, n)); _f32(roughness, (n,)); _f32(specular, (n,))
        a = N.pg_resample_lobe_args()
        a.wi, a.roughness, a.specular = wi.data_ptr(), roughness.data_ptr(), specular.data_ptr()
        return self._resample(self._lib.pg_resample_lobe, a, (N.pg_resample_params, float(alpha), float(delta), 0),
                              position, normal, sampler, candidates, active, return_candidates)

    def resampleInterface(self, position: torch.Tensor, normal: torch.Tensor, wi: torch.Tensor, roughness: torch.Tensor,
                          eta: torch.Tensor, sampler: PCG32Sampler, candidates: int = 8, alpha: float = 0.5, delta: float = 0.1,
                          active: Optional[torch.Tensor] = None,
                          return_candidates: bool = False) -> Tuple[torch.Tensor, torch.Tensor, Dict[str, torch.Tensor]]:
        """(direction float32 (3, N), weight float32 (N,), info) (pg_resample_interface): a direction in proportion to the
        tree's radiance times the two-sided lobe of a rough dielectric interface, by resampled importance sampling --
        `candidates` draws from the mixture of the lobe (share `alpha`) and the tree, one kept in proportion to target over
        source.  The lobe of a lane is the density of the renderer's rough dielectric: `wi`, the world direction towards the
        viewer on either side of the surface, reflected (share Fresnel) or refracted about a GGX visible normal at `roughness`
        in [1e-3, 1]; `normal` points to the exterior and `eta` is int_ior / ext_ior in [0.25, 4], not 1; `roughness` and `eta`
        are float32 (N,), all vectors are used as given.  The target is the lobe times (delta / 4 pi + (1 - delta) * the
        tree's density).  The estimator is f(direction) * weight with f the whole integrand; weight is 0 where nothing could
        be kept, and on lanes whose inputs the header calls invalid.  One kernel, one KD descent.  info is resampleLobe's
        {"target", "source" float32 (N,), "index" int32 (N,)} and "eta" float32 (N,): 1 for a kept direction on wi's side,
        else the relative index the path enters (eta from above, 1 / eta from below), 0 with nothing kept; with
        return_candidates also {"cand_dir" float32 (M, 3, N), "cand_target", "cand_source" float32 (M, N)}.  The lanes'
        streams advance by the candidates' draws."""
        n = position.shape[1]
        _f32(position, (3, n)); _f32(normal, (3, n)); _f32(wi, (3, n)); _f32(roughness, (n,)); _f32(eta, (n,))
        a = N.pg_resample_interface_args()
        a.wi, a.roughness, a.eta = wi.data_ptr(), roughness.data_ptr(), eta.data_ptr()
        eta_out = self._new(n)
        a.eta_out = eta_out.data_ptr()
        return self._resample(self._lib.pg_resample_interface, a, (N.pg_resample_params, float(alpha), float(delta), 0),
                              position, normal, sampler, candidates, active, return_candidates, more={"eta": eta_out})

    def exportPassRecords(self, slot: int = 0) -> Dict[str, torch.Tensor]:
        """The kept path-vertex records of the most recent render pass of buffer set `slot` (pg_render_export_records): a
        recording pass of a WavefrontScene(record_geometry=True); anything else raises.  Returns the columns addDataPropagate
        takes (plane stride n_lanes * max_depth of that pass, the records in any order) plus "slot" (int32, the bits of a
        uint32: the dense slot ray * max_depth + depth of every record) and "count" (int32[1], the number of records): addDataPropagate(rec, rec["count"]) on a tree of the same topology reproduces the pass's own
        accumulators.  Reads the pass's buffers on the current stream: with in_flight = 2 call scene.join() first; valid
        until the next pass of that buffer set."""
        S = int(self._pass_lanes.get(int(slot), 0)) * self._max_depth
        count = torch.zeros(1, dtype=torch.int32, device=self.device)
        # (never NULL, also for S = 0: the library then refuses because no pass recorded geometry, not because of a pointer)
        out, o = self._records_out(S, count.data_ptr())
        out["slot"] = self._new(S, dtype=torch.int32)
        out["count"] = count
        self._ck(self._lib.pg_render_export_records(self._h, int(slot), C.byref(o), out["slot"].data_ptr() or None,
                                                    out["count"].data_ptr(), _stream_ptr()))
        return out

    def _resample(self, fn, a, params, position, normal, sampler, candidates, active, return_candidates, more=None,
                  lead=(("cand_dir", torch.float32, 3),)):
        """What the four resampled calls share (csrc/pg_ris_dev.hpp), whose argument structs name these members alike: fills
        `a` with position, normal and the lane mask, the stream pointers, and fresh dir_out, weight_out and info's "target",
        "source", "index" (then `more`, outputs the caller has set itself); under return_candidates the candidate arrays,
        `lead` -- (key, dtype, shape of one candidate's entry of a lane) of those in front -- then "cand_target" and
        "cand_source", each filling the member key + "_out".  `params`: the parameter struct and its members behind
        `candidates`.  Calls fn and returns (dir_out's tensor, weight, info)."""
        n = position.shape[1]
        if sampler.n != n:
            raise ValueError("the sampler must have one stream per lane")
        m, mp = _mask(active, n)  # (m lives until the call is made)
        M = int(candidates)
        prm = params[0](M & 0xFFFFFFFF if M >= 0 else 0, *params[1:])
        a.p, a.normal, a.active = position.data_ptr(), normal.data_ptr(), mp
        a.rng_state, a.rng_inc = sampler.state.data_ptr(), sampler.inc.data_ptr()
        d, w = self._new(3, n), self._new(n)
        info = {"target": self._new(n), "source": self._new(n), "index": self._new(n, dtype=torch.int32), **(more or {})}
        a.dir_out, a.weight_out = d.data_ptr(), w.data_ptr()
        a.target_out, a.source_out, a.index_out = info["target"].data_ptr(), info["source"].data_ptr(), info["index"].data_ptr()
        if return_candidates and 1 <= M <= N.PG_RESAMPLE_MAX_CANDIDATES:  # (any other M is refused below, before a launch)
            for key, dtype, *shape in lead + (("cand_target", torch.float32), ("cand_source", torch.float32)):
                info[key] = self._new(M, *shape, n, dtype=dtype)
                setattr(a, key + "_out", info[key].data_ptr())
        self._ck(fn(self._h, n, C.byref(prm), C.byref(a), _stream_ptr()))
        return d, w, info

    def _records_out(self, S: int, null=None):
        """The six columns addDataPropagate takes, fresh and S records long, and the pg_records_out that points at them (`null`:
        what stands for the pointer of an empty column)."""
        out = {"position": self._new(3, S), "direction": self._new(2, S), "radiance": self._new(S), "woPdf": self._new(S),
               "direction_nee": self._new(2, S), "radiance_nee_lum": self._new(S)}
        o = N.pg_records_out()
        for (field, _), t in zip(o._fields_, out.values()):  # (the struct's members in the order of the columns)
            setattr(o, field, t.data_ptr() or null)
        return out, o

    def _dense(self, rec: Dict[str, torch.Tensor], S: int) -> N.pg_dense_records:
        d = N.pg_dense_records()
        act = rec["active"]
        if act.dtype == torch.bool:
            act = act.to(torch.uint8)
        rec["_active_u8"] = act.contiguous()
        d.active = rec["_active_u8"].data_ptr()
        d.position = _f32(rec["position"], (3, S)).data_ptr()
        d.direction = _f32(rec["direction"], (2, S)).data_ptr()
        d.bsdf = _f32(rec["bsdf"], (3, S)).data_ptr()
        d.throughput_bsdf = _f32(rec["throughputBsdf"], (3, S)).data_ptr()
        d.throughput_radiance = _f32(rec["throughputRadiance"], (3, S)).data_ptr()
        d.radiance_nee = _f32(rec["radiance_nee"], (3, S)).data_ptr()
        d.direction_nee = _f32(rec["direction_nee"], (2, S)).data_ptr()
        d.wo_pdf = _f32(rec["woPdf"], (S,)).data_ptr()
        return d

    def processRecords(self, num_rays: int, max_depth: int, Lfinal: torch.Tensor, rec: Dict[str, torch.Tensor]):
        """processPathData + the filter of scatterDataIntoSDTree (path_guiding_integrator.py:434-497)."""
        S = num_rays * max_depth
        _f32(Lfinal, (3, num_rays))
        d = self._dense(rec, S)
        out, o = self._records_out(S)
        count = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._ck(self._lib.pg_process_records(self._h, num_rays, max_depth, Lfinal.data_ptr(), C.byref(d), C.byref(o),
                                              count.data_ptr(), _stream_ptr()))
        return out, count

    def processAndSplat(self, num_rays: int, max_depth: int, Lfinal: torch.Tensor, rec: Dict[str, torch.Tensor]):
        self.prepareProcessAndSplat(num_rays, max_depth, Lfinal, rec)()

    def prepareProcessAndSplat(self, num_rays: int, max_depth: int, Lfinal: torch.Tensor, rec: Dict[str, torch.Tensor]):
        S = num_rays * max_depth
        _f32(Lfinal, (3, num_rays))
        d = self._dense(rec, S)
        fn, h, ck = self._lib.pg_process_and_splat, self._h, self._ck
        args = (h, num_rays, max_depth, Lfinal.data_ptr(), C.byref(d))

        def launch(_keep=(Lfinal, rec, d)):
            ck(fn(*args, torch.cuda.current_stream().cuda_stream))
        return launch

    # ---- refinement ---------------------------------------------------------------------
    def refineAndPrepare(self):
        self._ck(self._lib.pg_refine_and_swap(self._h, _stream_ptr()))

    def accumulators(self) -> torch.Tensor:
        """int64 view of sdTree_current's accumulators for torch.distributed.all_reduce (RCCL)."""
        p = C.c_void_p()
        n = C.c_uint64()
        self._ck(self._lib.pg_accumulators(self._h, C.byref(p), C.byref(n)))
        return _wrap_device_i64(p.value, n.value, self.device)

    def sortPlaces(self, keys: torch.Tensor, live: Optional[int] = None) -> torch.Tensor:
        """pg_sort_places: the ordering step of a sorted bounce by itself -- keys: uint16-valued places' keys (an int16 / uint16
        tensor of n entries on this device); returns the uint32 places (as int32 bits) in key order for the first `live` places."""
        n = int(keys.numel())
        k = keys.contiguous()
        if k.element_size() != 2:
            raise TypeError("keys: a 16-bit tensor")
        out = torch.full((n,), -1, dtype=torch.int32, device=self.device)
        d_live = None
        if live is not None:
            d_live = torch.tensor([int(live)], dtype=torch.int32, device=self.device)
        self._ck(self._lib.pg_sort_places(self._h, n, k.data_ptr(), None if d_live is None else d_live.data_ptr(), out.data_ptr(), _stream_ptr()))
        return out

    def bsdfProbe(self, materials: torch.Tensor, index: torch.Tensor, wi: torch.Tensor, wo: torch.Tensor, u: torch.Tensor,
                  level: int = 3):
        """pg_bsdf_probe: the renderer's BSDF layer by itself, for tests -- materials (n_mat, 16) float32, index (n,) int32,
        wi, wo, u (n,3) float32, all on this device; returns (value (n,3), pdf (n,), sampled wo (n,3), sample pdf (n,),
        weight (n,3), eta (n,), delta (n,) int32) as a kernel of feature level `level` computes them."""
        f = lambda t: t.to(torch.float32).contiguous()
        m, a, b, r = f(materials), f(wi), f(wo), f(u)
        idx = index.to(torch.int32).contiguous()
        n = int(idx.numel())
        if m.dim() != 2 or m.shape[1] != 16 or a.shape != (n, 3) or b.shape != (n, 3) or r.shape != (n, 3):
            raise ValueError("materials must be (n_mat,16); wi, wo and u (n,3); index (n,)")
        new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)
        value, pdf, swo, spdf, weight, eta = new(n, 3), new(n), new(n, 3), new(n), new(n, 3), new(n)
        delta = torch.zeros(n, dtype=torch.int32, device=self.device)
        self._ck(self._lib.pg_bsdf_probe(self._h, n, m.shape[0], m.data_ptr(), idx.data_ptr(), a.data_ptr(), b.data_ptr(), r.data_ptr(),
                                         int(level), value.data_ptr(), pdf.data_ptr(), swo.data_ptr(), spdf.data_ptr(),
                                         weight.data_ptr(), eta.data_ptr(), delta.data_ptr(), _stream_ptr()))
        return value, pdf, swo, spdf, weight, eta, delta

    def vertexProbe(self, materials: torch.Tensor, lanes: Dict[str, torch.Tensor], out: Dict[str, torch.Tensor], level: int,
                    frac: float, guided: bool, record: bool, store_nee: bool, rr_depth: int) -> None:
        """pg_vertex_probe: the renderer's bookkeeping of one path vertex by itself, for tests -- materials (n_mat, 16) float32;
        lanes: the columns of pg_vertex_lanes by name, out: those of pg_vertex_out by name (include/pgsd.h), contiguous tensors
        on this device of the header's types (uint32 as int32 bits, uint64 as int64 bits); the outputs are written in place."""
        m = materials.to(torch.float32).contiguous()
        if m.dim() != 2 or m.shape[1] != 16:
            raise ValueError("materials must be (n_mat,16)")
        n = int(lanes["flags"].numel())
        li, oo = N.pg_vertex_lanes(), N.pg_vertex_out()
        for struct, cols in ((li, lanes), (oo, out)):
            for name, _ in struct._fields_:
                t = cols[name]
                if not t.is_contiguous() or t.device != m.device:
                    raise ValueError(name + ": a contiguous tensor on the tree's device")
                setattr(struct, name, t.data_ptr())
        self._ck(self._lib.pg_vertex_probe(self._h, n, m.shape[0], m.data_ptr(), int(level), C.byref(li), float(frac), int(bool(guided)),
                                           int(bool(record)), int(bool(store_nee)), int(rr_depth), C.byref(oo), _stream_ptr()))

    def headProbe(self, lanes: Dict[str, torch.Tensor], out: Dict[str, torch.Tensor], max_depth: int, frac: float,
                  guided: bool) -> None:
        """pg_head_probe: the renderer's head of one path vertex by itself, for tests -- lanes: the columns of pg_head_lanes by
        name, out: those of pg_head_out by name (include/pgsd.h), contiguous tensors on this device of the header's types
        (uint32 as int32 bits, uint64 as int64 bits); the outputs are written in place.  Needs a scene."""
        n = int(lanes["prim"].numel())
        li, oo = N.pg_head_lanes(), N.pg_head_out()
        for struct, cols in ((li, lanes), (oo, out)):
            for name, _ in struct._fields_:
                t = cols[name]
                if not t.is_contiguous() or t.device != self.device:
                    raise ValueError(name + ": a contiguous tensor on the tree's device")
                setattr(struct, name, t.data_ptr())
        self._ck(self._lib.pg_head_probe(self._h, n, C.byref(li), int(max_depth), float(frac), int(bool(guided)), C.byref(oo),
                                         _stream_ptr()))

    def packAccumulators(self) -> torch.Tensor:
        """sdTree_current's accumulators in the 24-byte exchange format (pg_exchange_pack, on the current stream): the int64
        tensor a host-side collective sums instead of accumulators() -- a quarter fewer bytes; unpackAccumulators() writes
        the sums back."""
        p = C.c_void_p()
        n = C.c_uint64()
        self._ck(self._lib.pg_exchange_pack(self._h, C.byref(p), C.byref(n), _stream_ptr()))
        return _wrap_device_i64(p.value, n.value, self.device)

    def unpackAccumulators(self) -> None:
        self._ck(self._lib.pg_exchange_unpack(self._h, _stream_ptr()))

    def commInfo(self):
        """(ranks, rank) as RCCL reports them for this tree's communicator (ncclCommCount, ncclCommUserRank)."""
        n, r = C.c_int32(-1), C.c_int32(-1)
        self._ck(self._lib.pg_comm_info(self._h, C.byref(n), C.byref(r)))
        return int(n.value), int(r.value)

    # ---- the library's own exchange (pg_comm_*, pg_allreduce: RCCL bound at run time) ----------
    def commUniqueId(self) -> bytes:
        buf = (C.c_uint8 * 128)()
        self._ck(self._lib.pg_comm_unique_id(self._h, buf))
        return bytes(buf)

    def commInit(self, n_ranks: int, rank: int, unique_id: bytes) -> None:
        """ncclCommInitRank on this tree's device: collective over the n_ranks callers."""
        if len(unique_id) != 128:
            raise ValueError("unique_id: 128 bytes from commUniqueId() of rank 0")
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._ck(self._lib.pg_comm_init(self._h, int(n_ranks), int(rank), buf))

    def commDestroy(self) -> None:
        self._ck(self._lib.pg_comm_destroy(self._h))

    def allReduce(self) -> None:
        """In-place sum of sdTree_current's accumulators over the ranks (pg_allreduce), asynchronous on
        the current stream; call before refineAndPrepare on every rank."""
        self._ck(self._lib.pg_allreduce(self._h, _stream_ptr()))

    # ---- import / export in the reference's npz schema (kdtree.py:539-602) -----------------
    def sizes(self) -> N.pg_tree_sizes:
        s = N.pg_tree_sizes()
        self._ck(self._lib.pg_export_sizes(self._h, C.byref(s)))
        return s

    def export(self) -> Dict[str, np.ndarray]:
        s = self.sizes()
        a = {name: np.empty((getattr(s, size), width) if width > 1 else getattr(s, size), dtype)
             for name, _, dtype, size, width in _TREE_COLUMNS}
        c = _columns(a)
        self._ck(self._lib.pg_export(self._h, C.byref(s), C.byref(c)))
        a["kdtree_isLeaf"] = a["kdtree_isLeaf"].astype(bool)
        a["quadtree_isLeaf"] = a["quadtree_isLeaf"].astype(bool)
        a["kdtree_maxLeafSize"] = np.float64(c.kd_max_leaf_size)
        a["kdtree_maxDepth"] = np.int64(c.kd_max_depth)
        a["quadtree_maxDepth"] = np.int64(c.quad_max_depth)
        a["quadtree_isStoreNEERadiance"] = np.bool_(c.quad_store_nee)
        return a

    def load(self, d: Dict[str, np.ndarray]):
        a = {name: np.ascontiguousarray(d[name], dtype) for name, _, dtype, _, _ in _TREE_COLUMNS}
        c = _columns(a)
        c.kd_max_leaf_size = float(d["kdtree_maxLeafSize"])
        c.kd_max_depth = int(d["kdtree_maxDepth"])
        c.quad_max_depth = int(d["quadtree_maxDepth"])
        c.quad_store_nee = int(bool(d["quadtree_isStoreNEERadiance"]))
        s = N.pg_tree_sizes(a["kdtree_depth"].shape[0], a["quadtree_depth"].shape[0], a["quadtree_rootNodeIndex"].shape[0])
        self._ck(self._lib.pg_import(self._h, C.byref(s), C.byref(c)))
        self.store_nee = bool(c.quad_store_nee)

    def saveToFile(self, fileName: str):  # kdtree.py:539-602
        np.savez_compressed(fileName, **self.export())

    def loadFromFile(self, fileName: str):  # path_guiding_integrator.py:597-608
        self.load(dict(np.load(fileName)))

    def exportAccumulators(self):
        s = self.sizes()
        kd = np.empty(s.n_kd, np.uint64)
        lo = np.empty(s.n_quad, np.uint64)
        hi = np.empty(s.n_quad, np.int64)
        self._ck(self._lib.pg_export_accumulators(self._h, C.byref(s), kd.ctypes.data, lo.ctypes.data, hi.ctypes.data))
        return kd, lo, hi

    def stats(self) -> N.pg_stats:
        st = N.pg_stats()
        self._ck(self._lib.pg_get_stats(self._h, C.byref(st)))
        return st

    def enableKernelTiming(self, on: bool = True):
        self._ck(self._lib.pg_enable_kernel_timing(self._h, int(on)))

    def readKernelTiming(self, reset: bool = True) -> N.pg_kernel_timing:
        kt = N.pg_kernel_timing()
        self._ck(self._lib.pg_read_kernel_timing(self._h, C.byref(kt), int(reset)))
        return kt

    def evalMath(self, which: str, x: torch.Tensor) -> torch.Tensor:
        """The library's deterministic fp32 exp/log/erf/erfinv/sin/cos, element-wise (pg_math_eval)."""
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(x)
        self._ck(self._lib.pg_math_eval(self._h, ("exp", "log", "erf", "erfinv", "sin", "cos").index(which), x.numel(),
                                        x.data_ptr(), out.data_ptr(), _stream_ptr()))
        return out

    def renderLiveCounts(self, max_depth: int):
        """Paths alive after each bounce of the last rendered pass (pg_render_live_counts)."""
        out = (C.c_uint32 * int(max_depth))()
        self._ck(self._lib.pg_render_live_counts(self._h, out, int(max_depth)))
        return [int(v) for v in out]

    def enableDepthCounters(self, on=True):
        """on: False / True, or 2 -- a probe build's phase stamps alone (pg_read_shade_phases), no counters' atomics."""
        self._ck(self._lib.pg_enable_depth_counters(self._h, int(on)))

    def readShadePhases(self, reset: bool = True):
        """pg_read_shade_phases: (compiled_in, waves, [cycles of the seven phases of k_wave_shade]) -- zeros unless the library
        is the probe build (csrc/Makefile `probe`, libpgsd_phases.so)."""
        out = (C.c_uint64 * 10)()
        self._ck(self._lib.pg_read_shade_phases(self._h, out, int(reset)))
        return bool(out[0]), int(out[1]), [int(out[2 + i]) for i in range(7)]

    def readDepthCounters(self, reset: bool = True) -> N.pg_depth_counters:
        dc = N.pg_depth_counters()
        self._ck(self._lib.pg_read_depth_counters(self._h, C.byref(dc), int(reset)))
        return dc


# The columns of a tree in the reference's npz schema: (npz name, member of pg_tree_columns -- or (member, index) of an array of
# pointers --, dtype, the member of pg_tree_sizes that counts its rows, values per row).  export, load and _columns walk it.
_TREE_COLUMNS = [
    ("kdtree_bbox_min", "kd_bbox_min", np.float32, "n_kd", 3), ("kdtree_bbox_max", "kd_bbox_max", np.float32, "n_kd", 3),
    ("kdtree_depth", "kd_depth", np.uint32, "n_kd", 1), ("kdtree_vertCount", "kd_vert_count", np.float32, "n_kd", 1),
    ("kdtree_isLeaf", "kd_is_leaf", np.uint8, "n_kd", 1), ("kdtree_quadTreeRootIndex", "kd_quad_root_index", np.uint32, "n_kd", 1),
    ("kdtree_child_left_index", "kd_child_left", np.uint32, "n_kd", 1),
    ("kdtree_child_right_index", "kd_child_right", np.uint32, "n_kd", 1),
    ("quadtree_rootNodeIndex", "quad_root_node_index", np.uint32, "n_roots", 1),
    ("quadtree_bbox_min", "quad_bbox_min", np.float32, "n_quad", 2),
    ("quadtree_bbox_max", "quad_bbox_max", np.float32, "n_quad", 2),
    ("quadtree_depth", "quad_depth", np.uint32, "n_quad", 1), ("quadtree_irradiance", "quad_irradiance", np.float32, "n_quad", 1),
    ("quadtree_isLeaf", "quad_is_leaf", np.uint8, "n_quad", 1),
    ("quadtree_refinementThreshold", "quad_threshold", np.float32, "n_quad", 1),
] + [("quadtree_child_%d_index" % (k + 1), ("quad_child", k), np.uint32, "n_quad", 1) for k in range(4)]


def _columns(a: Dict[str, np.ndarray]) -> N.pg_tree_columns:
    c = N.pg_tree_columns()
    for name, member, _, _, _ in _TREE_COLUMNS:
        if isinstance(member, tuple):
            getattr(c, member[0])[member[1]] = a[name].ctypes.data
        else:
            setattr(c, member, a[name].ctypes.data)
    return c


class _DevMem:
    """Minimal __cuda_array_interface__ carrier so torch can alias library-owned device memory."""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {
            "shape": (n,), "typestr": "<i8", "data": (ptr, False), "version": 2, "strides": None,
        }


def _wrap_device_i64(ptr: int, n: int, device) -> torch.Tensor:
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=device)
    return torch.as_tensor(_DevMem(ptr, n), device=device)
