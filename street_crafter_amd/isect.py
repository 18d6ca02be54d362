"""Host side of the intersection stage: a3 `isect_tiles` and a4 `isect_offset_encode` (kernels: csrc/isect_bin.hip for the
tile-bucketed route, csrc/isect.hip + the radix sort for the reference-shaped one).

The module also holds what this stage shares with `rendering.py`, which imports it from here: the A/B switches
(`_SWITCH`), everything the operators remember between calls (`_STATE`) and the small argument helpers.  Read the
bucketed route top to bottom: `_MetaSlot` (how the counts reach the host), `_PendingIsect` (a call whose counts nobody
has looked at yet), `_BinCall` (one call: count -> predicted launch -> settle), `_isect_tiles_bin` (the driver).
"""
from __future__ import annotations

import collections
import math
import os
import threading
import weakref
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from .lazy import LazyTensor as _LazyTensor


def _env_on(name: str, default: bool = True) -> bool:
    v = os.environ.get(name)
    return default if v is None or v == "" else v not in ("0", "false", "False", "off", "no")


class _Switches:
    """The A/B switches of the operators: ONE object, every attribute settable through its set_* function (here and in
    rendering.py) and initialised from the environment, so that a user who cannot touch code can still turn a behaviour
    off.  None of them changes a result, except the last one (tests/test_call_history_gpu.py flips each of them between two
    calls of one frame shape, and between a training step's forward and backward, and compares with cold-state renders).
        SC_DEFER_ISECT=0   isect_tiles waits for the frame's intersection count inside the call (set_deferred_isect)
        SC_LAZY_IDS=0      isect_tiles' isect_ids are written by the sort instead of on first read (set_lazy_isect_ids)
      -> with BOTH off, flatten_ids / isect_ids are ordinary, fully written tensors the moment isect_tiles returns: what a
         caller needs who hands them to foreign C++ / DLPack consumers without a torch call in between
        SC_PLANAR_OUTPUT=0 render_colors interleaved under no_grad too (set_planar_output)
        SC_TILE_ORDER=0    no dispatch list for the rasterizer (set_tile_order)
        SC_VIEW_SLOTS=0    one work hint for all views (set_view_slots)
        SC_PACKED_RECORDS=0  the fused forward writes the four per-splat arrays instead of packed records (set_packed_records)
        SC_FUSED_TRAIN=1   OFF by default (set_fused_training): `rasterization()` with a leaf that requires grad runs its
                           per-Gaussian part as one forward and ONE backward kernel (sc_projection_sh_fwd / _bwd) instead of
                           the operator composition.  The one switch that changes gradients, within rounding: the forward
                           is bit-identical, the backward sums the same terms in another order and recomputes the
                           compensation instead of reading the stored one."""
    __slots__ = ("tile_order", "lazy_ids", "view_slots", "packed_records", "defer_isect", "planar_out", "fused_train")

    def __init__(self):
        self.tile_order = _env_on("SC_TILE_ORDER")
        self.lazy_ids = _env_on("SC_LAZY_IDS")
        self.view_slots = _env_on("SC_VIEW_SLOTS")
        self.packed_records = _env_on("SC_PACKED_RECORDS")
        self.defer_isect = _env_on("SC_DEFER_ISECT")
        self.planar_out = _env_on("SC_PLANAR_OUTPUT")
        self.fused_train = _env_on("SC_FUSED_TRAIN", False)

    def flip(self, name: str, value: bool) -> bool:
        prev = getattr(self, name)
        setattr(self, name, bool(value))
        return prev


def _predicted_capacities(history, bucket_cap) -> Tuple[int, int, int]:
    """(capacity, rec_capacity, super_capacity) the next isect_tiles of a frame shape launches its scatter + sort with
    before the host has read the counts, from the sizes in `history`: 12.5 % head-room over the largest of them (a rig's
    cameras are rendered in turn and see different amounts of the scene: sized by the previous call alone, every switch
    to a fuller view missed the prediction and paid the host round trip + a second launch).  Head-room alone must not
    cross `bucket_cap`, the capacity of the one-workgroup bucket sort: provisioned above it, every frame also launches
    the split kernel and ~10 k idle segment workgroups -- 8-10 us at the training resolution, whose largest bucket sits
    just below it.  A frame that does exceed it fails the device-side check and is relaunched with exact sizes, and the
    history then provisions for it."""
    mi, mr, ms = map(max, zip(*history))
    ms_pred = ms + ms // 8 + 64
    if ms <= bucket_cap < ms_pred:
        ms_pred = bucket_cap
    return mi + mi // 8 + 4096, mr + mr // 8 + 4096, ms_pred


class _OperatorState:
    """Everything the operators remember BETWEEN calls, in one place (round 3 had eleven module-level tables).  Every
    entry is a hint the kernels verify on the device or that only orders work: dropping any of it (reset_state) never
    changes a result.  All tables are keyed by the device index first; `reset(device)` forgets one device's entries.
      prediction  (device, C, N, tile_size, tile_width, tile_height) -> (capacity, rec_capacity, super_capacity) the next
                  isect_tiles of this frame shape launches its scatter + sort with, before the host has read the counts
      history     same key -> the sizes of the last `history_len` calls (the prediction covers the largest of them)
      last_meta   same key -> (n_isects, n_records, largest super-tile) of the last call (diagnostics, tests)
      tile_work   (device, C, N, tile_width, tile_height) -> int32 [view slots, C * tiles]: what every tile walked the last
                  time a frame of this shape was rasterized (the rasterizer's scheduling hint)
      view_registry  device -> int32 [sc_view_registry_words()]: the device-side table forward axis -> view slot
      stats       how often the predicted sizes held (bench.py reports it)"""
    KEYS_MAX = 64        # frame shapes remembered in prediction / history / last_meta (pruned together)

    def __init__(self):
        self.prediction, self.history, self.last_meta = {}, {}, {}
        self.history_len = 8     # (tools/exp_camera_rig.py sets 1 for its A/B: round 2's first form)
        self.tile_work, self.view_registry = {}, {}
        self.stats = {"calls": 0, "speculative_ok": 0, "exact_relaunch": 0}
        self.bucket_cap = {}     # "v": sc_isect_bin_bucket_capacity()
        self.sched_sizes = {}    # tiles -> (words of the work-hint buffer, items of the dispatch list)

    def tables(self):
        return (("predictions", self.prediction), ("history", self.history), ("last_meta", self.last_meta),
                ("tile_work", self.tile_work), ("view_registry", self.view_registry))

    def reset(self, idx=None) -> dict:
        dropped = {}
        for name, table in self.tables():
            keys = [k for k in table if idx is None or (k[0] if isinstance(k, tuple) else k) == idx]
            for k in keys:
                table.pop(k, None)
            dropped[name] = len(keys)
        return dropped

    def record(self, key, sizes, bucket_cap):
        """An isect_tiles call of frame shape `key` had `sizes` = (n_isects, n_records, largest super-tile)."""
        hist = self.history.get(key)
        if hist is None:
            hist = self.history[key] = collections.deque(maxlen=self.history_len)
            while len(self.history) > self.KEYS_MAX:
                # one key per distinct (device, C, N, tile grid): densification changes N every 100 training iterations
                # (train.py:292-310), so all three per-shape tables are pruned together, oldest shape first
                old = next(iter(self.history))
                for table in (self.history, self.prediction, self.last_meta):
                    table.pop(old, None)
        hist.append(sizes)
        self.last_meta[key] = sizes
        self.prediction[key] = _predicted_capacities(hist, bucket_cap)


_SWITCH = _Switches()
_STATE = _OperatorState()

# "bin"  : tile-bucketed count + in-LDS per-tile sort (default once available)
# "radix": reference-shaped count -> emit -> device-wide radix sort
_ISECT_MODE = {"mode": "bin"}


def set_isect_mode(mode: str) -> str:
    assert mode in ("bin", "radix")
    prev = _ISECT_MODE["mode"]
    _ISECT_MODE["mode"] = mode
    return prev


def set_lazy_isect_ids(enabled: bool) -> bool:
    """isect_tiles' `isect_ids` on the tile-bucketed path: True (default) = a LazyTensor filled on first use
    (street_crafter_amd/lazy.py: the reference's path never reads it), False = written by the sort as before.
    Returns the previous setting."""
    return _SWITCH.flip("lazy_ids", enabled)


def set_deferred_isect(enabled: bool) -> bool:
    """isect_tiles' host wait for the frame's intersection count: True (default) = deferred to the first observation of
    `flatten_ids` / `isect_ids` (normally inside rasterize_to_pixels, by when the count has long arrived: lazy.py), False =
    inside isect_tiles as before.  Applies when a prediction of the buffer sizes exists (from the second call of a frame
    shape on).  Results are identical either way.  Returns the previous setting."""
    return _SWITCH.flip("defer_isect", enabled)


# ------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------
def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: Tensor):
    """The current HIP stream of the tensor's device as a raw handle.  (torch.cuda.current_stream builds a Stream
    object: ~4 us a call, seven calls a frame; small scenes are bound by this wrapper's host time.)"""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(t.device.index if t.device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


def _req(t: Tensor, name: str, dtype=torch.float32):
    # (the common case first: small frames are bound by the host time of these wrappers)
    if type(t) is Tensor and t.dtype is dtype and t.is_cuda and t.is_contiguous():
        return t
    if not isinstance(t, Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on a HIP device (got {t.device}); "
                           "street_crafter_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def _ws(nbytes: int, device) -> Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


_WARNED = set()


def _warn_once(key, msg, *args):
    """One WARNING per process and key (logging, logger "street_crafter_amd")."""
    if key not in _WARNED:
        _WARNED.add(key)
        import logging
        logging.getLogger("street_crafter_amd").warning(msg, *args)


# ------------------------------------------------------------------------------------------
# a3 isect_tiles  (renderer.py:243-252)
# ------------------------------------------------------------------------------------------
@torch.no_grad()
def isect_tiles(means2d: Tensor, radii: Tensor, depths: Tensor, tile_size: int, tile_width: int,
                tile_height: int, sort: bool = True, packed: bool = False,
                n_cameras: Optional[int] = None, camera_ids: Optional[Tensor] = None,
                gaussian_ids: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (tiles_per_gauss i32[C,N], isect_ids i64[I] (sorted), flatten_ids i32[I])."""
    if packed:
        raise NotImplementedError("packed=True is not supported (reference passes packed=False)")
    view_cams = getattr(means2d, "_sc_viewmats", None)
    # (detach only what autograd tracks: a detach is ~2 us of host time, and small frames are bound by this wrapper)
    means2d = _req(means2d.detach() if means2d.requires_grad else means2d, "means2d")
    radii = _req(radii, "radii", torch.int32)
    depths = _req(depths.detach() if depths.requires_grad else depths, "depths")
    C, N = radii.shape
    assert means2d.shape == (C, N, 2), means2d.shape
    assert depths.shape == (C, N), depths.shape
    if n_cameras is not None:
        assert int(n_cameras) == C, (n_cameras, C)
    st = _stream(means2d)
    mode = _ISECT_MODE["mode"] if sort else "radix"
    if mode == "bin":
        res = _isect_tiles_bin(means2d, radii, depths, C, N, tile_size, tile_width, tile_height, st,
                               viewmats=view_cams, defer=True)
        if res is not None:
            return res[:3]
    return _isect_tiles_radix(means2d, radii, depths, C, N, tile_size, tile_width, tile_height, sort, st)


def _isect_tiles_radix(means2d, radii, depths, C, N, tile_size, tile_width, tile_height, sort, st):
    """The reference-shaped route: count -> emit -> device-wide radix sort (sort=False, frames outside the bucketed
    path's limits, and the on-GPU cross-check of the bucketed route).  Its entry points have no counterpart in the
    binding layer: they are called through the ctypes table on either host route."""
    lib = _lib.load()
    dev = means2d.device
    tiles_per_gauss = torch.empty((C, N), dtype=torch.int32, device=dev)
    total_dev = torch.empty(1, dtype=torch.int64, device=dev)
    wsb = lib.sc_isect_workspace_bytes(C * N)
    ws = _ws(wsb, dev)
    _lib.check(lib.sc_isect_count(_p(means2d), _p(radii), C, N, int(tile_size), int(tile_width),
                                  int(tile_height), _p(tiles_per_gauss), _p(total_dev), _p(ws), ws.numel(), st),
               "sc_isect_count")
    n_isects = int(total_dev.item())    # the one unavoidable D2H read (sizes the outputs)
    _check_isect_count(n_isects, C, N, tile_width, tile_height)
    isect_ids = torch.empty(n_isects, dtype=torch.int64, device=dev)
    flatten_ids = torch.empty(n_isects, dtype=torch.int32, device=dev)
    if n_isects:
        _lib.check(lib.sc_isect_emit(_p(means2d), _p(radii), _p(depths), C, N, int(tile_size), int(tile_width),
                                     int(tile_height), _p(tiles_per_gauss), n_isects, _p(isect_ids),
                                     _p(flatten_ids), _p(ws), ws.numel(), st), "sc_isect_emit")
        if sort:
            n_tiles = tile_width * tile_height
            tile_bits = int(math.floor(math.log2(n_tiles))) + 1
            cam_bits = int(math.floor(math.log2(C))) + 1
            tmp_k = torch.empty_like(isect_ids)
            tmp_v = torch.empty_like(flatten_ids)
            sws = _ws(lib.sc_radix_sort_workspace_bytes(n_isects), dev)
            _lib.check(lib.sc_radix_sort_pairs_u64_i32(_p(isect_ids), _p(flatten_ids), _p(tmp_k), _p(tmp_v),
                                                       n_isects, 32 + tile_bits + cam_bits, _p(sws),
                                                       sws.numel(), st), "sc_radix_sort_pairs_u64_i32")
    return tiles_per_gauss, isect_ids, flatten_ids


def _check_isect_count(n_isects, C, N, tile_width, tile_height):
    """isect_offsets / positions in flatten_ids are int32, as in gsplat (which wraps around silently here)."""
    if n_isects > 0x7fffffff:
        raise RuntimeError(f"isect_tiles: {n_isects} tile intersections exceed the int32 range of isect_offsets "
                           f"({C} cameras x {N} Gaussians on {tile_width}x{tile_height} tiles); render fewer "
                           "cameras per call or cull the scene")


def _view_registry(dev) -> Optional[Tensor]:
    """The device-side table forward axis -> view slot of `dev` (sc_isect_bin_count looks the frame's camera up in
    it, no host round trip), or None when the dispatch list / the slots are off."""
    if not (_SWITCH.view_slots and _SWITCH.tile_order):
        return None
    reg = _STATE.view_registry.get(dev.index)
    if reg is None:
        reg = _STATE.view_registry[dev.index] = torch.zeros(_lib.load().sc_view_registry_words(), dtype=torch.int32, device=dev)
    return reg


def _tile_work(dev, C, N, tile_width, tile_height) -> Tensor:
    """The rasterizer's per-tile work hint of this frame shape AND Gaussian count: the foreground and the sky pass
    of a novel-view frame have the same frame shape and must not feed each other's dispatch list.  At most 8
    buffers are kept (densification changes N every few hundred training steps)."""
    key = (dev.index, int(C), int(N), int(tile_width), int(tile_height))
    t = _STATE.tile_work.pop(key, None)
    if t is None:
        # one bank of C * tiles words per view slot (the kernels pick the bank: sc_common.h)
        t = torch.zeros(_lib.load().sc_view_slots() * int(C) * int(tile_width) * int(tile_height), dtype=torch.int32,
                        device=dev)
        while len(_STATE.tile_work) >= 8:
            _STATE.tile_work.pop(next(iter(_STATE.tile_work)))
    _STATE.tile_work[key] = t                  # (re-inserted: dicts keep insertion order, the first key is the oldest)
    return t


class _MetaSlot:
    """Where the count phase of one (host thread, device) reports its sizes: `host`, a pinned int64[8] the device writes
    directly, then a sequence number -- no D2H copy, no event on the stream (include/*.h); its numpy `view` and address `ptr`;
    `seq` of the thread's latest call; `pending`: weakly, that call's _PendingIsect while nobody has looked at its counts."""
    __slots__ = ("host", "view", "ptr", "seq", "pending")

    def __init__(self, host):
        self.host, self.view, self.ptr, self.seq, self.pending = host, host.numpy(), host.data_ptr(), 0, None

    def settle_pending(self, warn_key, warn_msg):
        """Settles the call whose counts nobody has looked at yet, if any; its error becomes one warning here."""
        pending, self.pending = self.pending and self.pending(), None
        if pending is not None:
            try:
                pending.resolve()
            except Exception as e:      # noqa: BLE001  (kept on the pending call: its own tensors raise it when looked at)
                _warn_once(warn_key, warn_msg, type(e).__name__, e)


_PINNED_META = threading.local()   # .slots: device index -> _MetaSlot of THIS host thread


class _PendingIsect:
    """The part of one isect_tiles call that needs the frame's counts on the host: wait, check of the predicted launch
    (exact relaunch when it was too small), bookkeeping for the next prediction, and the final length of the two id
    tensors.  Shared by the `flatten_ids` and `isect_ids` LazyTensors of the call (each holds it; it holds them weakly)
    and by the pinned meta slot of the host thread (weakly): the next isect_tiles call of the thread settles it first,
    because the slot's words are overwritten by every count phase."""
    __slots__ = ("settle", "flat_ref", "ids_ref", "done", "lock", "flat_plain", "error", "__weakref__")

    def __init__(self, settle):
        self.settle, self.flat_ref, self.ids_ref = settle, None, None
        self.done, self.lock, self.flat_plain, self.error = False, threading.Lock(), None, None

    def resolve(self, _tensor=None):
        with self.lock:
            if self.done:
                return
            if self.error is not None:         # (e.g. more than 2^31 - 1 intersections: every observation says so)
                raise self.error
            settle, self.settle = self.settle, None
            try:
                fids, ids_buf, after = settle()
            except BaseException as e:
                self.error = e
                raise
            self.flat_plain = fids
            with torch._C.DisableTorchFunctionSubclass():
                for ref, src in ((self.flat_ref, fids), (self.ids_ref, ids_buf)):
                    t = ref() if ref is not None else None
                    if t is not None and src is not None:
                        t.set_(src)
                        t.__dict__["_sc_resolve"] = None      # (settled through the other tensor / the next call)
            self.done = True
            if after is not None:
                after()


def _bin_launch_ran(capacities, n_isects, n_records, max_super) -> bool:
    """True iff a bucket scatter + sort launched with `capacities` = (capacity, rec_capacity, super_capacity)
    passed the device-side size check, i.e. ran in full.  Must mirror the kernels' test
    (`meta[0] > capacity || meta[2] > rec_capacity || meta[3] > super_capacity`, isect_bin.hip) exactly:
    sc_isect_bin_sort hands the kernels the SAME unrounded numbers it is given."""
    return n_isects <= capacities[0] and n_records <= capacities[1] and max_super <= capacities[2]


class _BinCall:
    """One call of the tile-bucketed route behind its count phase.  `pred`: the sizes its scatter + sort were launched with
    before the counts were known (None: no such launch).  `settle()` waits for the counts: that launch ran in full -- it has
    consumed the bucket cursors and must never be repeated -- or one launch with the exact sizes follows.  Settled inside
    the call, or on the first observation of the outputs (`deferred()`)."""
    __slots__ = ("b", "st", "dev", "inputs", "depths", "C", "N", "grid", "offsets", "meta_dev", "ws0", "slot", "seq",
                 "eager_ids", "key", "pred", "ids", "fids", "flat", "n_isects", "ids_ref")

    def __init__(self, b, st, inputs, C, N, grid, offsets, meta_dev, ws0, slot, eager_ids):
        self.b, self.st, self.dev = b, st, offsets.device                  # the binding, the producing stream
        self.inputs, self.depths, self.C, self.N, self.grid = inputs, inputs[2], C, N, grid     # (means2d, radii, depths)
        self.offsets, self.meta_dev, self.ws0, self.slot, self.seq = offsets, meta_dev, ws0, slot, slot.seq
        self.eager_ids, self.key = eager_ids, (self.dev.index, C, N, *grid)    # grid: (tile_size, tile_width, tile_height)
        self.pred = self.ids = self.fids = self.flat = self.n_isects = self.ids_ref = None

    def read_meta(self):
        # wait for the sequence number (a spin in C that holds no GIL); if the GPU is far behind (or something went
        # wrong) fall back to a plain synchronising copy after 2 s
        if self.b.wait_i64(self.slot.ptr + 32, self.seq, 2_000_000) != 0:
            # (the settle may run under another current stream than `st` -- the thread's next isect_tiles, reset_state -- and
            #  a copy on THAT stream would not be ordered behind the count kernels: wait for the producer's stream first)
            torch.cuda.ExternalStream(self.st, device=self.dev).synchronize()
            return tuple(int(v) for v in self.meta_dev.cpu().tolist())
        return tuple(map(int, self.slot.view[:4]))

    def launch(self, capacities):        # scatter + sort with (capacity, rec_capacity, super_capacity) -> rc
        rc, self.ids, self.fids = self.b.isect_bin_sort(
            *self.inputs, *self.grid, self.offsets, self.meta_dev, self.ws0, int(capacities[0]), int(capacities[1]),
            int(capacities[2]), bool(self.eager_ids), self.st)
        return rc

    def settle(self):
        """Everything that needs the frame's counts on the host.  -> n_isects, with `flat` the frame's flatten_ids, or
        None when the frame is outside the tile-bucketed path's limits (the caller takes the reference-shaped route)."""
        n_isects, _, n_records, max_super = self.read_meta()     # the one host wait of a frame; GPU already has work
        C, N, st, (_, tile_width, tile_height) = self.C, self.N, self.st, self.grid
        _check_isect_count(n_isects, C, N, tile_width, tile_height)
        # the device ran the predicted launch iff ALL THREE of its checks passed; `_bin_launch_ran` restates those
        # checks exactly (a launch that ran in full has consumed the bucket cursors: it must never be repeated)
        ran = self.pred is not None and _bin_launch_ran(self.pred, n_isects, n_records, max_super)
        _STATE.stats["calls"] += 1
        if self.pred is not None:
            _STATE.stats["speculative_ok" if ran else "exact_relaunch"] += 1
        if not ran:
            if self.pred is not None:     # a predicted launch was enqueued and (by the device's own check) did nothing:
                # belt and braces, the cursors are re-zeroed before the exact-size launch all the same
                _lib.check(_lib.load().sc_isect_bin_reset_cursors(_p(self.ws0), C * N, C, tile_width, tile_height, st),
                           "sc_isect_bin_reset_cursors")
            if _stream(self.offsets) != st:      # (settled late, under another current stream: allocate where the kernels run)
                with torch.cuda.stream(torch.cuda.ExternalStream(st, device=self.dev)):
                    rc = self.launch((n_isects, n_records, max_super))
                # whoever settles reads the lists next, on ITS stream: whatever it did to wait for the producer's stream came
                # before this launch was enqueued there
                self.order_current_behind_producer()
            else:
                rc = self.launch((n_isects, n_records, max_super))
            if rc == _lib.SC_EUNSUPPORTED:
                return None
            _lib.check(rc, "sc_isect_bin_sort")
        cap = _STATE.bucket_cap.get("v") or _STATE.bucket_cap.setdefault("v", int(_lib.load().sc_isect_bin_bucket_capacity()))
        _STATE.record(self.key, (n_isects, n_records, max_super), cap)
        self.flat, self.n_isects = self.fids[:n_isects], n_isects
        self.inputs = self.meta_dev = self.ws0 = None     # (nothing launches any more; fill_ids must not keep the workspace)
        return n_isects

    def order_current_behind_producer(self):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.ExternalStream(self.st, device=self.dev))
        torch.cuda.current_stream(self.dev).wait_event(ev)

    def fill_ids(self, buf):
        # isect_ids: allocated now, written on first use (one kernel, from flatten_ids / offsets / depths)
        cur = _stream(buf)
        if cur != self.st:            # filled from another stream than the one that sorted: order them
            self.order_current_behind_producer()
        _lib.check(_lib.load().sc_isect_ids_rebuild(self.flat.data_ptr(), self.offsets.data_ptr(), self.depths.data_ptr(),
                                                    self.C, self.N, self.grid[1], self.grid[2], self.n_isects,
                                                    buf.data_ptr(), cur), "sc_isect_ids_rebuild")

    def file_offsets(self, isect_ids=None):
        # the bucket scan already IS isect_offset_encode's result: remember it on the tensor object so the caller's next call
        # (renderer.py:253) does not re-read the 8 B x I key array (no argument: the deferred isect_ids, if alive, again
        # after its set_, which has bumped the version the offsets were filed under)
        isect_ids = self.ids_ref() if isect_ids is None else isect_ids
        if isect_ids is not None:
            with torch._C.DisableTorchFunctionSubclass():
                isect_ids._sc_offsets = (self.offsets, self.C, self.grid[1], self.grid[2], isect_ids._version)

    def deferred(self):
        """-> (isect_ids, flatten_ids) of a length to come.  The predicted scatter + sort are enqueued; the wait for the
        counts, the check of the prediction and the true length of the two id tensors are settled on their first observation
        (lazy.py) -- on the reference's path inside rasterize_to_pixels, three torch calls later, when the counts have arrived."""
        pending = _PendingIsect(self.settle_deferred)
        flatten_ids = _LazyTensor(self.fids[:0], None, pending.resolve)
        isect_ids = _LazyTensor(torch.empty(0, dtype=torch.int64, device=self.dev), self.fill_ids, pending.resolve)
        pending.flat_ref, pending.ids_ref = weakref.ref(flatten_ids), weakref.ref(isect_ids)
        self.slot.pending, self.ids_ref = weakref.ref(pending), pending.ids_ref
        self.file_offsets(isect_ids)
        return isect_ids, flatten_ids

    def settle_deferred(self):      # -> _PendingIsect.resolve: (flatten_ids, isect_ids' buffer, what to run behind set_)
        n_isects = self.settle()
        if n_isects is not None:
            return self.flat, torch.empty(n_isects, dtype=torch.int64, device=self.dev), self.file_offsets
        # outside the bucketed path's limits after all: the reference-shaped route, now
        # (called directly: switching the process-wide mode around a nested isect_tiles would send a concurrent
        #  call of another host thread down the radix route too -- ADVICE r3)
        with torch.cuda.stream(torch.cuda.ExternalStream(self.st, device=self.dev)):
            _, ids, flat = _isect_tiles_radix(*self.inputs, self.C, self.N, *self.grid, True, self.st)
        if _stream(self.offsets) != self.st:
            self.order_current_behind_producer()
        isect_ids = self.ids_ref()
        if isect_ids is not None:
            isect_ids.__dict__["_sc_fill"] = None          # (the radix route has written the keys)
        return flat, ids, self.file_offsets


def _isect_tiles_bin(means2d, radii, depths, C, N, tile_size, tile_width, tile_height, st, want_ids=True,
                     viewmats=None, defer=False):
    """-> (tiles_per_gauss, isect_ids | None, flatten_ids, isect_offsets), or None when the shape is outside
    the tile-bucketed path's limits.  want_ids=False skips the 8 B x I key array altogether (the fused
    rasterization() forward never reads it).  Host threads do not serialise each other: the count phase reports
    its sizes through a pinned slot + sequence number per (host thread, device), and the wait for it releases
    the GIL (sc_wait_i64) -- a host that renders two frames in flight from two threads keeps launching one frame
    while it waits for the other's counts (tests/test_gpu_parity.py::test_two_host_threads_render_on_one_device).
    defer: see set_deferred_isect (the wait, the check of the predicted launch and the outputs' lengths move to the first
    observation of the outputs; only the public isect_tiles asks for it)."""
    dev = means2d.device
    b = _lib.binding()         # (allocates every output of the count phase, and of each sort launch, in its one call)
    slots = _PINNED_META.__dict__.setdefault("slots", {})
    slot = slots.get(dev.index)
    if slot is None:         # meta (output sizes) comes back through host-mapped pinned memory
        slot = slots[dev.index] = _MetaSlot(torch.zeros(8, dtype=torch.int64, pin_memory=True))
    slot.settle_pending("settle_prev", "isect_tiles: settling the previous, never observed call failed (%s: %s); its own "
                        "tensors raise the error when they are looked at")
    slot.seq += 1
    grid = (int(tile_size), int(tile_width), int(tile_height))
    # the rasterizer's dispatch order (longest-running tiles first) is built here, beside the count kernels, from
    # what every tile walked the last time (tile_size 16: the wave-per-tile rasterizer)
    want_order = _SWITCH.tile_order and grid[0] == 16
    work = _tile_work(dev, C, N, tile_width, tile_height) if want_order else None
    registry = None
    if (want_order and viewmats is not None and viewmats.device == dev and viewmats.dtype == torch.float32
            and viewmats.is_contiguous() and viewmats.shape == (C, 4, 4)):
        registry = _view_registry(dev)
    if registry is None:
        viewmats = None
    rc, tiles_per_gauss, offsets, meta_dev, ws0, order = b.isect_bin_count(
        means2d, radii, depths, *grid, work, viewmats, registry, bool(want_order), slot.ptr, slot.seq, st)
    if want_order:
        offsets._sc_sched = (order, work)          # travels with isect_offsets to rasterize_to_pixels
    if rc == _lib.SC_EUNSUPPORTED:     # -> reference-shaped route
        return None
    if rc:
        _lib.check(rc, "sc_isect_bin_count")
    eager_ids = want_ids and not _SWITCH.lazy_ids
    call = _BinCall(b, st, (means2d, radii, depths), C, N, grid, offsets, meta_dev, ws0, slot, eager_ids)
    pred = _STATE.prediction.get(call.key)
    if pred is not None:
        rc = call.launch(pred)
        if rc == 0:
            call.pred = pred
        elif rc != _lib.SC_EUNSUPPORTED:            # (unsupported is treated as "no predicted launch")
            _lib.check(rc, "sc_isect_bin_sort")
    if defer and call.pred is not None and want_ids and not eager_ids and _SWITCH.defer_isect:
        return (tiles_per_gauss, *call.deferred(), offsets)
    n_isects = call.settle()
    if n_isects is None:
        return None
    isect_ids = None
    if want_ids:
        isect_ids = (call.ids[:n_isects] if eager_ids
                     else _LazyTensor(torch.empty(n_isects, dtype=torch.int64, device=dev), call.fill_ids))
        call.file_offsets(isect_ids)
    return tiles_per_gauss, isect_ids, call.flat, offsets


# ------------------------------------------------------------------------------------------
# a4 isect_offset_encode  (renderer.py:253)
# ------------------------------------------------------------------------------------------
@torch.no_grad()
def isect_offset_encode(isect_ids: Tensor, n_cameras: int, tile_width: int, tile_height: int) -> Tensor:
    lib = _lib.load()
    cached = getattr(isect_ids, "_sc_offsets", None)
    if cached is not None and cached[1:4] == (int(n_cameras), int(tile_width), int(tile_height)):
        # still the keys isect_tiles produced?  A LazyTensor knows whether anything has seen its contents (no torch
        # call needed to ask: an attribute read through a tensor subclass costs ~4 us of host time); an ordinary
        # tensor (eager keys) is checked by its version counter
        if (isect_ids.__dict__.get("_sc_touched") is None if type(isect_ids) is _LazyTensor
                else isect_ids._version == cached[4]):
            return cached[0]
    isect_ids = _req(isect_ids, "isect_ids", torch.int64)
    dev = isect_ids.device
    offsets = torch.empty((n_cameras, tile_height, tile_width), dtype=torch.int32, device=dev)
    _lib.check(lib.sc_isect_offsets(_p(isect_ids), isect_ids.numel(), int(n_cameras), int(tile_width),
                                    int(tile_height), _p(offsets), _stream(isect_ids)), "sc_isect_offsets")
    return offsets
