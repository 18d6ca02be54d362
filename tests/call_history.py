"""Scripted call HISTORIES of the operators: a step vocabulary, named programs, a seeded generator, a model of the host-side
bookkeeping, and the runner that executes a step on the GPU.

The operators keep state between calls (street_crafter_amd/isect.py `_STATE`, `_PINNED_META`; the attributes filed on
`isect_ids` / `isect_offsets`); `reset_state()` promises that none of it is ever needed for a correct result.  The property
tests/test_call_history_gpu.py holds the code to: EVERY call of a history returns, bit for bit, what the same call returns
from a cold state.  tests/test_call_history_cpu.py checks this module on its own (no GPU is needed to import it).

  Step          a frozen record: kind, scene spec, camera spec, frame size, options
  PROGRAMS      hand-written histories with the transitions each declares; `transitions(program)` computes them
  random_program(seed, n_steps)
  HostModel     what the Python side should do with the sizes (n_isects, n_records, max_super) of each call: the arithmetic is
                the real `_predicted_capacities` / `_bin_launch_ran` of isect.py, only the bookkeeping is restated
  Runner        executes steps (imports the GPU pieces lazily)
"""
from __future__ import annotations

import collections
import dataclasses
import math
import random
from typing import Dict, List, Optional, Tuple

import numpy as _np

from street_crafter_amd.isect import _bin_launch_ran, _predicted_capacities

DEVICE = 0
BUCKET_CAP = 3584            # sc_isect_bin_bucket_capacity(); the GPU test asserts that the library says the same
HISTORY_LEN, KEYS_MAX, WORK_MAX = 8, 64, 8
N_RANGE, W_RANGE, H_RANGE = (300, 20000), (64, 320), (48, 208)

# scene shapes: keyword arguments of the builder in street_crafter_amd.scenes
SHAPES = {
    "wide": {},
    "near": dict(z_range=(1.0, 30.0), scale_range=(0.02, 0.3)),
    "culled": dict(z_range=(2000.0, 3000.0)),                         # beyond the far plane: nothing survives the projection
    # everything within ~2 px of the principal point: at 96x96 that is the middle of ONE 2x2 super-tile, which then holds
    # every Gaussian of the scene -- the smallest scene whose largest super-tile crosses the bucket capacity has n > 3584
    "cluster": dict(x_span=0.01, y_span=0.01, z_range=(4.0, 40.0), scale_range=(0.005, 0.02)),
}
# views: yaw about +y; how full the frame is for a scene that fills the front view (the synthetic size tables use it)
VIEWS = {"front": (0.0, "full"), "side": (0.9, "sparse"), "away": (math.pi, "empty")}
VIEWS.update({f"rig{i}": (-0.675 + 0.15 * i, "full") for i in range(10)})        # 8.6 degrees apart: no two share a view slot

# training cases of oracle/param_grad_f64.py used here: id -> (C, N, width, height)
TRAIN_CASES = {"plain": (1, 2500, 160, 96), "deg0": (1, 2000, 160, 96), "two_cameras": (2, 2500, 160, 96)}
TRAIN_ROUTES = ("operators", "rasterization")

SWITCHES = {          # name -> (module attribute path, default, the other value)
    "tile_order": ("rendering.set_tile_order", True, False),
    "view_slots": ("rendering.set_view_slots", True, False),
    "lazy_isect_ids": ("rendering.set_lazy_isect_ids", True, False),
    "deferred_isect": ("rendering.set_deferred_isect", True, False),
    "planar_output": ("rendering.set_planar_output", True, False),
    "packed_records": ("rendering.set_packed_records", True, False),
    "isect_mode": ("rendering.set_isect_mode", "bin", "radix"),
    "fast_binding": ("_lib.set_fast_binding", True, False),
    "fused_training": ("rendering.set_fused_training", False, True),
    "native_autograd": ("rendering.set_native_autograd", True, False),
}
OBSERVE = ("now", "after_next", "after_reset", "never", "other_stream")
ENCODE = ("before_touch", "after_touch", "after_inplace_write")
KINDS = ("frame", "operators", "fused", "novel", "grouped", "train_fwd", "train_bwd", "switch", "reset")


@dataclasses.dataclass(frozen=True)
class SceneSpec:
    builder: str            # a function of street_crafter_amd.scenes
    n: int
    seed: int
    shape: str = "wide"


@dataclasses.dataclass(frozen=True)
class Step:
    kind: str
    scene: Optional[SceneSpec] = None
    view: Optional[str] = None
    size: Optional[Tuple[int, int]] = None          # (width, height)
    opts: Tuple[Tuple[str, object], ...] = ()

    def opt(self, name, default=None):
        return dict(self.opts).get(name, default)

    def __str__(self):
        parts = [self.kind]
        if self.scene is not None:
            parts.append(f"{self.scene.builder}(n={self.scene.n}, seed={self.scene.seed}, {self.scene.shape})")
        if self.view is not None:
            parts.append(self.view)
        if self.size is not None:
            parts.append("%dx%d" % self.size)
        parts += [f"{k}={v}" for k, v in self.opts]
        return " ".join(parts)


def _o(**kw):
    return tuple(sorted(kw.items()))


def frame(scene, view="front", size=(160, 96)):
    return Step("frame", scene, view, size)


def operators(scene, view="front", size=(160, 96), observe="now", encode="before_touch"):
    return Step("operators", scene, view, size, _o(observe=observe, encode=encode))


def fused(scene, view="front", size=(160, 96), render_mode="RGB+ED", rasterize_mode="antialiased", sh=True, C=1, tile_size=16):
    return Step("fused", scene, view, size, _o(render_mode=render_mode, rasterize_mode=rasterize_mode, sh=sh, C=C, tile_size=tile_size))


def novel(n, n_sky, seed=1, view="front", size=(160, 96)):
    return Step("novel", SceneSpec("make_street_scene", n, seed), view, size, _o(n_sky=n_sky))


def grouped(scene, view="front", size=(160, 96)):
    return Step("grouped", scene, view, size)


def train_fwd(case, route="operators", tag="a"):
    return Step("train_fwd", opts=_o(case=case, route=route, tag=tag))


def train_bwd(tag="a"):
    return Step("train_bwd", opts=_o(tag=tag))


def switch(name, value):
    return Step("switch", opts=_o(name=name, value=value))


def reset(device=None):
    return Step("reset", opts=_o(device=device))


def scene(n, seed=1, shape="wide"):
    return SceneSpec("make_scene", n, seed, shape)


# ------------------------------------------------------------------------------------------------------------------------
# which isect_tiles calls a step makes
# ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Call:
    key: tuple               # (device, C, N, tile_size, tile_width, tile_height)
    public: bool             # through the public isect_tiles (may be deferred) or the fused forward's direct call
    fullness: str            # "full" | "sparse" | "empty" | "over": what the synthetic size tables are made from


def _key(C, N, size, tile_size=16):
    return (DEVICE, C, N, tile_size, math.ceil(size[0] / tile_size), math.ceil(size[1] / tile_size))


def _fullness(step):
    if step.scene is not None and step.scene.shape == "culled":
        return "empty"
    if step.scene is not None and step.scene.shape == "cluster":
        return "over" if step.scene.n > BUCKET_CAP else "full"
    return VIEWS[step.view][1]


def calls_of(step: Step) -> List[Call]:
    """The bucketed-route isect calls of a step under the default switches, in order."""
    k = step.kind
    if k in ("frame", "operators", "grouped"):
        return [Call(_key(1, step.scene.n, step.size), True, _fullness(step))]
    if k == "fused":
        ts = step.opt("tile_size")
        direct = step.opt("sh") and step.opt("render_mode") in ("RGB+D", "RGB+ED") and ts == 16
        return [Call(_key(step.opt("C"), step.scene.n, step.size, ts), not direct, _fullness(step))]
    if k == "novel":
        n, ns, f = step.scene.n, step.opt("n_sky"), _fullness(step)
        return [Call(_key(1, n, step.size), True, f), Call(_key(1, ns, step.size), True, f), Call(_key(1, n + ns, step.size), False, f)]
    if k == "train_fwd":
        C, N, W, H = TRAIN_CASES[step.opt("case")]
        return [Call(_key(C, N, (W, H)), True, "full")]
    return []


def synthetic_sizes(call: Call) -> Tuple[int, int, int]:
    """(n_isects, n_records, max_super) shaped like the programs' views, for the CPU tests."""
    N = call.key[1] * call.key[2]
    return {"full": (4 * N, 2 * N, min(N // 4, BUCKET_CAP - 100)), "sparse": (N, N // 2, N // 16), "empty": (0, 0, 0),
            "over": (4 * N, 2 * N, BUCKET_CAP + 500)}[call.fullness]


# ------------------------------------------------------------------------------------------------------------------------
# the host model
# ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Settled:
    origin: int              # index of the step that made the call
    at: int                  # index of the step during which it was settled
    key: tuple
    event: str               # "first" | "speculative_ok" | "exact_relaunch"
    settler: Optional[str]   # "self" | "successor" | "reset" | "other_stream" | "observer" | None (dropped, never settled)
    deferred: bool


class HostModel:
    """Replays the bookkeeping of `_OperatorState`, `_MetaSlot.pending` and `reset_state` on the sizes of each call.
    `step(i, step, sizes)` -> (events of the step's own calls, the calls SETTLED during this step): the stats delta of the
    step is what the settled list says.  Three switches exist only to be broken by the CPU tests."""

    def __init__(self, bucket_cap=BUCKET_CAP, key_without_n=False, ignore_max_super=False, successor_settles=True):
        self.cap, self.key_without_n, self.ignore_max_super, self.successor_settles = bucket_cap, key_without_n, ignore_max_super, successor_settles
        self.prediction, self.history, self.last_meta, self.tile_work = {}, {}, {}, collections.OrderedDict()
        self.pending = None              # (origin, key, pred, sizes, finish_after_step | None)
        self.switches = {k: v[1] for k, v in SWITCHES.items()}
        self.pruned, self.evicted = set(), set()
        self.returned_to_pruned = self.returned_to_evicted = 0

    # -- bookkeeping ------------------------------------------------------------------------------------------------
    def _k(self, key):
        return key[:2] + key[3:] if self.key_without_n else key

    def _record(self, key, sizes):
        k = self._k(key)
        hist = self.history.get(k)
        if hist is None:
            hist = self.history[k] = collections.deque(maxlen=HISTORY_LEN)
            while len(self.history) > KEYS_MAX:
                old = next(iter(self.history))
                for table in (self.history, self.prediction, self.last_meta):
                    table.pop(old, None)
                self.pruned.add(old)
        hist.append(sizes)
        self.last_meta[k] = sizes
        self.prediction[k] = _predicted_capacities(hist, self.cap)

    def _work(self, key):
        k = (key[0], key[1], key[2], key[4], key[5])
        if k in self.tile_work:
            self.tile_work.move_to_end(k)
            return
        if k in self.evicted:
            self.returned_to_evicted += 1
            self.evicted.discard(k)
        while len(self.tile_work) >= WORK_MAX:
            self.evicted.add(self.tile_work.popitem(last=False)[0])
        self.tile_work[k] = True

    def _settle(self, origin, at, key, pred, sizes, settler, deferred):
        if pred is None:
            event = "first"
        else:
            ran = _bin_launch_ran(pred, sizes[0], sizes[1], 0 if self.ignore_max_super else sizes[2])
            event = "speculative_ok" if ran else "exact_relaunch"
        self._record(key, sizes)
        return Settled(origin, at, key, event, settler, deferred)

    def _settle_pending(self, at, settler):
        origin, key, pred, sizes, _ = self.pending
        self.pending = None
        return self._settle(origin, at, key, pred, sizes, settler, True)

    def reset(self, device=None):
        for table in (self.prediction, self.history, self.last_meta, self.tile_work):
            for k in [k for k in table if device is None or k[0] == device]:
                del table[k]

    # -- one step ----------------------------------------------------------------------------------------------------
    def step(self, i: int, step: Step, sizes: List[Tuple[int, int, int]]):
        own, settled = [], []
        if step.kind == "switch":
            self.switches[step.opt("name")] = step.opt("value")
        elif step.kind == "reset":
            if self.pending is not None:
                settled.append(self._settle_pending(i, "reset"))
            self.reset(step.opt("device"))
        calls = calls_of(step) if self.switches["isect_mode"] == "bin" else []
        observe = step.opt("observe", "now")
        for call, sz in zip(calls, sizes):
            if self.pending is not None and self.successor_settles:
                settled.append(self._settle_pending(i, "successor"))
            if self.switches["tile_order"] and call.key[3] == 16:
                self._work(call.key)
            k = self._k(call.key)
            if k in self.pruned and k not in self.prediction:
                self.returned_to_pruned += 1
                self.pruned.discard(k)
            pred = self.prediction.get(k)
            deferred = (pred is not None and call.public and self.switches["lazy_isect_ids"] and self.switches["deferred_isect"])
            if not deferred:
                s = self._settle(i, i, call.key, pred, sz, "self", False)
            else:
                if self.pending is not None:                    # (only a broken model gets here: the slot is overwritten)
                    settled.append(self._settle_pending(i, "observer"))
                self.pending = (i, call.key, pred, sz, i + 1 if observe == "after_next" else None)
                if observe == "never":
                    self.pending = None
                    s = Settled(i, i, call.key, "speculative_ok" if _bin_launch_ran(pred, *sz) else "exact_relaunch", None, True)
                elif observe == "after_next":
                    s = None
                elif observe == "after_reset":
                    s = self._settle_pending(i, "reset")
                    self.reset(None)
                else:
                    s = self._settle_pending(i, "other_stream" if observe == "other_stream" else "self")
            if s is not None:
                own.append(s)
                if s.settler is not None:
                    settled.append(s)
            if observe == "after_reset" and not deferred:
                self.reset(None)
        if self.pending is not None and self.pending[4] == i:          # the held outputs are looked at after this step
            settled.append(self._settle_pending(i, "observer"))
        return own, settled

    @staticmethod
    def stats_delta(settled):
        d = {"calls": len(settled), "speculative_ok": 0, "exact_relaunch": 0}
        for s in settled:
            if s.event != "first":
                d[s.event] += 1
        return d


def replay(program, sizes_of=None, **model_kw):
    """-> (model, [(own, settled)] per step) with `sizes_of(step)` -> sizes per call (default: the synthetic table)."""
    model = HostModel(**model_kw)
    sizes_of = sizes_of or (lambda st: [synthetic_sizes(c) for c in calls_of(st)])
    return model, [model.step(i, st, sizes_of(st)) for i, st in enumerate(program)]


def event_sequence(program, **model_kw):
    _, out = replay(program, **model_kw)
    return [tuple((s.origin, s.event, s.settler) for s in settled) for _, settled in out]


# ------------------------------------------------------------------------------------------------------------------------
# transitions
# ------------------------------------------------------------------------------------------------------------------------
RANK = {"empty": 0, "sparse": 1, "full": 2, "over": 3}
ALL_TRANSITIONS = frozenset(
    ["key_call_1", "key_call_2", "key_call_9", "fuller_after_emptier", "emptier_after_fuller", "other_scene_same_key",
     "culled_before_full", "culled_after_full", "over_capacity_after_below",
     "encode_before_touch", "encode_after_touch", "encode_after_inplace_write",
     "tile_work_evicted_and_back", "prediction_pruned_and_back", "registry_takeover_and_back", "c2_between_c1",
     "tile8_between_tile16", "tile32_between_tile16", "infer_between_fwd_bwd_same_scene", "infer_between_fwd_bwd_other_scene",
     "two_fwd_reverse_bwd", "novel_between_frames", "grouped_between_frames"]
    + [f"deferred_{fate}:{how}" for fate in ("dropped", "after_next", "after_reset", "other_stream") for how in ("held", "missed")]
    + [f"switch:{name}" for name in SWITCHES])
LEFT_OUT = ("radix_fallback_between_bucketed",)      # no shape within the size cap makes sc_isect_bin_* answer -3 (see the summary)
_FATE = {"never": "dropped", "after_next": "after_next", "after_reset": "after_reset", "other_stream": "other_stream"}


def _train_scene(case):
    return {"plain": scene(2500, 2, "near")}.get(case)


def transitions(program, sizes_of=None) -> frozenset:
    """The transitions a program contains, from its step list alone (sizes: the synthetic table of the views, or
    `sizes_of(step)`: the GPU test hands in the measured ones and must find the same set)."""
    out = set()
    model, events = replay(program, sizes_of)
    n_calls, last, prev_step_of_key = collections.Counter(), {}, {}
    views_seen, open_train, fwd_order = [], {}, []
    flips = {}                 # switch name -> [key of the call before the flip, flipped-state call seen, flipped back]
    for i, (st, (own, settled)) in enumerate(zip(program, events)):
        calls = calls_of(st)
        for c in calls:
            n_calls[c.key] += 1
            if n_calls[c.key] in (1, 2, 9):
                out.add(f"key_call_{n_calls[c.key]}")
            if c.key in last:
                p, pst = last[c.key], prev_step_of_key[c.key]
                if RANK[c.fullness] > RANK[p.fullness]:
                    out.add("fuller_after_emptier")
                if RANK[c.fullness] < RANK[p.fullness]:
                    out.add("emptier_after_fuller")
                if st.scene is not None and pst.scene is not None and st.scene != pst.scene:
                    out.add("other_scene_same_key")
                    if p.fullness == "empty" and c.fullness == "full":
                        out.add("culled_before_full")
                    if p.fullness == "full" and c.fullness == "empty":
                        out.add("culled_after_full")
                    if c.fullness == "over" and p.fullness != "over":
                        out.add("over_capacity_after_below")
            last[c.key], prev_step_of_key[c.key] = c, st
        for s in own:
            if s.deferred and st.kind == "operators" and st.opt("observe") in _FATE:
                out.add(f"deferred_{_FATE[st.opt('observe')]}:{'held' if s.event == 'speculative_ok' else 'missed'}")
        for s in settled:
            if s.settler == "successor" and program[s.origin].opt("observe") == "after_next":
                if program[i].kind != "switch" and calls and calls[0].key != s.key:
                    out.add(f"deferred_after_next:{'held' if s.event == 'speculative_ok' else 'missed'}")
        if st.kind == "operators" and st.opt("observe") == "now":
            enc = st.opt("encode")
            if enc != "after_inplace_write" or not model_switch_at(program, i, "lazy_isect_ids"):
                out.add(f"encode_{enc}")
        # 9, 10: another C / tile size between two tile-16 C=1 calls of one frame size
        if i >= 1 and i + 1 < len(program) and st.kind == "fused":
            a, b = calls_of(program[i - 1]), calls_of(program[i + 1])
            if a and b and a[0].key == b[0].key and a[0].key[1] == 1 and a[0].key[3] == 16 and st.size == program[i - 1].size:
                if st.opt("C") == 2:
                    out.add("c2_between_c1")
                if st.opt("tile_size") in (8, 32):
                    out.add(f"tile{st.opt('tile_size')}_between_tile16")
        if i >= 1 and i + 1 < len(program) and st.kind in ("novel", "grouped"):
            a, b = program[i - 1], program[i + 1]
            if a.kind == b.kind == "frame" and a.size == b.size == st.size:
                out.add(f"{st.kind}_between_frames")
        # 8: nine or more far-apart views under one key, then the first again
        if st.kind == "frame" and st.view.startswith("rig"):
            if st.view in views_seen and len(set(views_seen)) >= 9 and views_seen[0] == st.view:
                out.add("registry_takeover_and_back")
            views_seen.append(st.view)
        # 11: every switch flipped between two calls of one key, and flipped back
        if st.kind == "switch":
            name, value = st.opt("name"), st.opt("value")
            if value != SWITCHES[name][1]:
                prev = next((calls_of(p)[0].key for p in reversed(program[:i]) if calls_of(p)), None)
                flips[name] = [prev, None]
            elif name in flips and flips[name][1]:
                # flipped back: the key's next call follows (a backward IS the second call of its own forward's key)
                nxt = next((calls_of(p)[0].key for p in program[i + 1:] if calls_of(p)), None)
                if flips[name][1] == "bwd" or nxt == flips[name][0]:
                    out.add(f"switch:{name}")
        for name, f in flips.items():
            touched = calls or st.kind == "train_bwd"
            if touched and model_switch_at(program, i, name) != SWITCHES[name][1]:
                if st.kind == "train_bwd":
                    f[1] = "bwd"
                elif calls and calls[0].key == f[0]:
                    f[1] = f[1] or "call"
        # 12: training and inference interleaved
        if st.kind == "train_fwd":
            open_train[st.opt("tag")] = (i, st.opt("case"))
            fwd_order.append(st.opt("tag"))
        if st.kind == "train_bwd":
            j, case = open_train.pop(st.opt("tag"))
            C, N, W, H = TRAIN_CASES[case]
            for mid in program[j + 1:i]:
                if mid.kind == "frame" and calls_of(mid)[0].key == _key(C, N, (W, H)):
                    same = mid.scene == _train_scene(case)
                    out.add("infer_between_fwd_bwd_same_scene" if same else "infer_between_fwd_bwd_other_scene")
            if any(k < j for k, _ in open_train.values()):          # the later forward's backward comes first
                out.add("two_fwd_reverse_bwd")
    if model.returned_to_evicted:
        out.add("tile_work_evicted_and_back")
    if model.returned_to_pruned:
        out.add("prediction_pruned_and_back")
    return frozenset(out)


def model_switch_at(program, i, name):
    """The value of a switch while step i runs."""
    v = SWITCHES[name][1]
    for st in program[:i]:
        if st.kind == "switch" and st.opt("name") == name:
            v = st.opt("value")
    return v


def check_well_formed(program):
    """Forward/backward pairs matched, switches balanced, sizes within the cap, options that go together."""
    open_train, state = {}, {k: v[1] for k, v in SWITCHES.items()}
    for i, st in enumerate(program):
        assert st.kind in KINDS, (i, st)
        if st.scene is not None:
            assert N_RANGE[0] <= st.scene.n <= N_RANGE[1], (i, str(st))
            assert st.scene.shape in SHAPES and st.view in VIEWS, (i, str(st))
            assert W_RANGE[0] <= st.size[0] <= W_RANGE[1] and H_RANGE[0] <= st.size[1] <= H_RANGE[1], (i, str(st))
            if st.scene.shape == "cluster" and st.scene.n > BUCKET_CAP:
                assert st.scene.n <= BUCKET_CAP + 512, (i, "the smallest builder that crosses the capacity")
        if st.kind == "novel":
            assert N_RANGE[0] <= st.opt("n_sky") <= N_RANGE[1], (i, str(st))
        if st.kind == "operators":
            assert st.opt("observe") in OBSERVE and st.opt("encode") in ENCODE, (i, str(st))
            assert not (i and st.opt("observe") == program[i - 1].opt("observe") == "after_next"), (i, "one held step at a time")
            if st.opt("observe") != "now":           # the encode variants look at the keys, which settles the call at once
                assert st.opt("encode") == "before_touch", (i, str(st))
        if st.kind == "switch":
            name, value = st.opt("name"), st.opt("value")
            assert value in SWITCHES[name][1:], (i, str(st))
            state[name] = value
        if st.kind == "train_fwd":
            assert st.opt("case") in TRAIN_CASES and st.opt("route") in TRAIN_ROUTES and st.opt("tag") not in open_train, (i, str(st))
            # (the rasterization route of tests/test_param_grad_rows_gpu.py asserts the operator composition)
            assert not (st.opt("route") == "rasterization" and state["fused_training"]), (i, str(st))
            assert state["isect_mode"] == "bin", (i, str(st))
            open_train[st.opt("tag")] = i
        if st.kind == "train_bwd":
            assert st.opt("tag") in open_train, (i, str(st))
            del open_train[st.opt("tag")]
    assert not open_train, open_train
    assert state == {k: v[1] for k, v in SWITCHES.items()}, state
    assert program[-1].opt("observe", "now") != "after_next"
    return True


# ------------------------------------------------------------------------------------------------------------------------
# the named programs
# ------------------------------------------------------------------------------------------------------------------------
A = scene(2500, 1)
A2 = scene(2500, 2)
A_CULLED = scene(2500, 1, "culled")
B = scene(500, 3)
SMALL = (64, 48)


def _flip(name, *between):
    return [switch(name, SWITCHES[name][2]), *between, switch(name, SWITCHES[name][1])]


def _rig_history():
    p = [frame(A)] * 9                                            # first, second ... ninth call of a key
    p += [frame(A, "side"), reset(), frame(A, "side"), frame(A), frame(A2), frame(A_CULLED), frame(A)]
    p += [fused(A, C=2), frame(A), fused(A, tile_size=8), frame(A), fused(A, tile_size=32), frame(A)]
    p += [operators(A, "side", observe="after_next"), frame(B, size=SMALL), operators(A, observe="after_next"), frame(B, size=SMALL)]
    p += [reset(DEVICE), frame(A_CULLED), frame(A), frame(A, "away"), frame(A)]
    return p


def _deferred_fates():
    M = [scene(3001 + i, 4) for i in range(4)]
    p = [frame(A), frame(A), operators(A, observe="never"), frame(A), operators(A, observe="after_next"), frame(B, size=SMALL),
         operators(A, observe="after_reset"), frame(A), frame(A), operators(A, observe="other_stream")]
    p += [frame(M[0], "side"), operators(M[0], observe="never"), frame(M[0], "side")]
    p += [frame(M[1], "side"), operators(M[1], observe="after_next"), frame(B, size=SMALL)]
    p += [frame(M[2], "side"), operators(M[2], observe="other_stream")]
    p += [frame(M[3], "side"), operators(M[3], observe="after_reset")]
    p += [frame(A), operators(A), operators(A, encode="after_touch")]
    p += _flip("lazy_isect_ids", operators(A, encode="after_inplace_write"))
    p += [frame(A)]
    return p


def _evictions():
    k0 = scene(500, 3)
    p = [frame(k0, size=SMALL)] * 2 + [frame(scene(501 + i, 3), size=SMALL) for i in range(9)] + [frame(k0, size=SMALL)]
    p += [novel(1000 + 20 * i, 301 + i, size=SMALL) for i in range(22)]           # three keys each: 66 in all
    p += [frame(k0, size=SMALL)] * 2
    return p


def _switches():
    per = {"tile_order": frame(A), "view_slots": frame(A), "lazy_isect_ids": operators(A), "deferred_isect": operators(A),
           "planar_output": frame(A), "packed_records": fused(A), "isect_mode": frame(A), "fast_binding": frame(A),
           "fused_training": fused(A), "native_autograd": frame(A)}
    p = [frame(A)]
    for name, st in per.items():
        p += _flip(name, st) + [st]
    return p


def _training():
    S, S2 = scene(2500, 2, "near"), scene(2500, 5, "near")
    p = [frame(S), frame(S)]
    p += [train_fwd("plain"), frame(S), train_bwd(), train_fwd("plain"), frame(S2), train_bwd()]
    p += [train_fwd("two_cameras", "rasterization", "a"), train_fwd("plain", "operators", "b"), train_bwd("b"), train_bwd("a")]
    p += [train_fwd("two_cameras"), *_flip("native_autograd", train_bwd())]
    p += [train_fwd("plain"), *_flip("fast_binding", train_bwd())]
    p += [train_fwd("two_cameras", "rasterization"), *_flip("fused_training", fused(S), train_bwd())]
    p += [train_fwd("deg0"), reset(), train_bwd(), frame(S)]
    return p


def _mixed():
    R, W, CL = scene(1000, 6), scene(3900, 7), scene(3900, 7, "cluster")
    p = [frame(A), novel(3000, 300), frame(A), grouped(A), frame(A)]
    p += [frame(R, f"rig{i}", SMALL) for i in range(10)] + [frame(R, "rig0", SMALL)]
    p += [frame(W, size=(96, 96)), frame(W, size=(96, 96)), frame(CL, size=(96, 96)), frame(CL, size=(96, 96)), frame(W, size=(96, 96))]
    p += [fused(A, render_mode="RGB+D", rasterize_mode="classic"), fused(A, render_mode="RGB", sh=False),
          fused(A, render_mode="ED", sh=False, rasterize_mode="classic"), frame(A)]
    p += [reset(), frame(A, "side"), frame(A), frame(A)]
    return p


def _t(*names):
    return frozenset(names)


PROGRAMS: Dict[str, Tuple[List[Step], frozenset]] = {
    "rig_history": (_rig_history(), _t(
        "key_call_1", "key_call_2", "key_call_9", "fuller_after_emptier", "emptier_after_fuller", "other_scene_same_key",
        "culled_before_full", "culled_after_full", "c2_between_c1", "tile8_between_tile16", "tile32_between_tile16",
        "deferred_after_next:held")),
    "deferred_fates": (_deferred_fates(), _t(
        "key_call_1", "key_call_2", "key_call_9", "fuller_after_emptier", "emptier_after_fuller", "encode_before_touch", "encode_after_touch",
        "encode_after_inplace_write", "switch:lazy_isect_ids",
        *[f"deferred_{f}:{h}" for f in ("dropped", "after_next", "after_reset", "other_stream") for h in ("held", "missed")])),
    "evictions": (_evictions(), _t("key_call_1", "key_call_2", "tile_work_evicted_and_back", "prediction_pruned_and_back")),
    "switches": (_switches(), _t("key_call_1", "key_call_2", "key_call_9", "encode_before_touch", *[f"switch:{n}" for n in SWITCHES])),
    "training": (_training(), _t(
        "key_call_1", "key_call_2", "key_call_9", "infer_between_fwd_bwd_same_scene",
        "infer_between_fwd_bwd_other_scene", "two_fwd_reverse_bwd", "switch:native_autograd", "switch:fast_binding",
        "switch:fused_training")),
    "mixed": (_mixed(), _t(
        "key_call_1", "key_call_2", "key_call_9", "fuller_after_emptier", "other_scene_same_key", "over_capacity_after_below",
        "emptier_after_fuller", "registry_takeover_and_back", "novel_between_frames", "grouped_between_frames")),
}
SEEDS = (11, 23, 47)
RANDOM_STEPS = 40


def random_program(seed: int, n_steps: int = RANDOM_STEPS) -> List[Step]:
    """A seeded history over the same vocabulary: every train_fwd gets a later train_bwd, every switch is flipped back."""
    rng = random.Random(seed)
    scenes = [A, A2, A_CULLED, scene(2500, 2, "near")]
    p, open_tags, flipped = [], [], []
    while len(p) < n_steps:
        left = n_steps - len(p)
        if left <= len(open_tags) + len(flipped):                 # wind down: backwards first, then the switches
            p.append(train_bwd(open_tags.pop()) if open_tags else switch(flipped[-1], SWITCHES[flipped.pop()][1]))
            continue
        r = rng.random()
        sc, view = rng.choice(scenes), rng.choice(("front", "front", "side", "away"))
        if r < 0.25:
            p.append(frame(sc, view))
        elif r < 0.45:
            obs = rng.choice(OBSERVE)
            if obs == "after_next" and (left <= len(open_tags) + len(flipped) + 1 or (p and p[-1].opt("observe") == "after_next")):
                obs = "now"
            p.append(operators(sc, view, observe=obs, encode=rng.choice(ENCODE) if obs == "now" else "before_touch"))
        elif r < 0.6:
            mode, sh = rng.choice((("RGB+ED", True), ("RGB+D", True), ("RGB", True), ("D", False), ("RGB", False)))
            p.append(fused(sc, view, render_mode=mode, sh=sh, rasterize_mode=rng.choice(("classic", "antialiased")),
                           C=rng.choice((1, 1, 2)), tile_size=rng.choice((16, 16, 8, 32))))
        elif r < 0.66:
            p.append(novel(2500, 300 + rng.randrange(4), view=view))
        elif r < 0.72:
            p.append(grouped(sc, view))
        elif r < 0.8 and left >= len(open_tags) + len(flipped) + 3:
            tag = next(t for t in "abc" if t not in open_tags) if len(open_tags) < 3 else None
            radix, fused_on = "isect_mode" in flipped, "fused_training" in flipped
            if tag is not None and not radix:
                case = rng.choice(tuple(TRAIN_CASES))
                route = "operators" if fused_on else rng.choice(TRAIN_ROUTES)
                p.append(train_fwd(case, route, tag))
                open_tags.append(tag)
        elif r < 0.86 and open_tags:
            p.append(train_bwd(open_tags.pop(rng.randrange(len(open_tags)))))
        elif r < 0.95 and left >= len(open_tags) + len(flipped) + 3:
            name = rng.choice(tuple(SWITCHES))
            if name in flipped:
                flipped.remove(name)
                p.append(switch(name, SWITCHES[name][1]))
            else:
                flipped.append(name)
                p.append(switch(name, SWITCHES[name][2]))
        elif r >= 0.95:
            p.append(reset(rng.choice((None, DEVICE))))
    return p


def first_difference(cold, warm):
    """None, or a sentence about the first output that differs."""
    if sorted(cold) != sorted(warm):
        return f"outputs {sorted(set(cold) ^ set(warm))} exist on one side only"
    for name, a in cold.items():
        b = warm[name]
        if a.shape != b.shape or a.dtype != b.dtype:
            return f"{name}: cold {a.dtype}{list(a.shape)}, warm {b.dtype}{list(b.shape)}"
        ab, bb = a.reshape(-1).view(_np.uint8), b.reshape(-1).view(_np.uint8)
        if not _np.array_equal(ab, bb):
            at = int(_np.flatnonzero(ab != bb)[0]) // a.dtype.itemsize
            n = int((a.reshape(-1) != b.reshape(-1)).sum())
            return f"{name}: element {at} of {a.size} cold {a.reshape(-1)[at]!r} warm {b.reshape(-1)[at]!r} ({n} elements differ)"
    return None


# ------------------------------------------------------------------------------------------------------------------------
# the runner (needs the GPU)
# ------------------------------------------------------------------------------------------------------------------------
FRAME_KEYS = ("rgb", "acc", "depth", "_radii", "_means2d", "_depths", "_conics", "_compensations", "_tiles_per_gauss",
              "_flatten_ids", "_isect_ids", "_isect_offsets", "_colors", "_render_colors", "_render_alphas")


def content_of(step: Step) -> Step:
    """What decides a step's OUTPUTS: the tag of a training step is only a name."""
    if step.kind == "train_fwd":
        return dataclasses.replace(step, opts=_o(case=step.opt("case"), route=step.opt("route"), tag="a"))
    return step


def has_outputs(step: Step) -> bool:
    return step.kind in ("frame", "operators", "fused", "novel", "grouped", "train_fwd")


class Runner:
    """Executes steps.  `run(step)` -> {output name: numpy array} (None for an `after_next` step, whose outputs
    `finish_held()` hands out once the next step has run); `sizes` holds what `_STATE.last_meta` said for the step's calls."""
    DEV = "cuda"

    def __init__(self, cold=False):
        import torch
        import gsplat.rendering as ops
        from street_crafter_amd import _lib, rendering
        self.torch, self.ops, self.rendering, self._lib = torch, ops, rendering, _lib
        self.cold = cold
        self.held = None
        self.train = {}                # tag -> (case, leaves, viewspace points, loss)
        self.judged = []               # (tag, case) of the backwards judged
        self.sizes = []
        self.touched_switches = {}     # name -> the value found at the first flip
        self.scenes, self.side = {}, None

    # -- inputs -----------------------------------------------------------------------------------------------------
    def scene(self, spec: SceneSpec, n_sky=None):
        key = (spec, n_sky)
        if key not in self.scenes:
            from street_crafter_amd import scenes
            build = getattr(scenes, spec.builder)
            if spec.builder == "make_street_scene":
                fg, sky = build(spec.n, n_sky=n_sky, seed=spec.seed)
                self.scenes[key] = (fg.to(self.DEV), sky.to(self.DEV))
            else:
                self.scenes[key] = build(spec.n, seed=spec.seed, **SHAPES[spec.shape]).to(self.DEV)
        return self.scenes[key]

    def camera(self, view, size, extra_yaw=0.0):
        from street_crafter_amd.scenes import make_camera
        W, H = size
        return make_camera(W, H, 0.9 * W, 0.9 * W, yaw=VIEWS[view][0] + extra_yaw).to(self.DEV)

    def host(self, t):
        import numpy as np
        if hasattr(t, "plain"):
            t = t.plain()
        return np.ascontiguousarray(t.detach().contiguous().cpu().numpy())

    def _hosted(self, named):
        return {k: self.host(v) for k, v in named.items() if v is not None}

    def _read_sizes(self, step):
        meta = self.rendering._STATE.last_meta
        self.sizes = [meta.get(c.key) for c in calls_of(step)]

    # -- steps ------------------------------------------------------------------------------------------------------
    def run(self, step: Step):
        out = getattr(self, "_" + step.kind)(step)
        if step.opt("observe") != "after_reset":
            self._read_sizes(step)
        return out

    def _frame(self, st):
        from harness.caller import render_gaussians
        with self.torch.no_grad():
            out = render_gaussians(self.scene(st.scene), self.camera(st.view, st.size), return_intermediates=True)
            return self._hosted({k: out[k] for k in FRAME_KEYS})

    def _operators(self, st):
        torch, ops = self.torch, self.ops
        sc, cam = self.scene(st.scene), self.camera(st.view, st.size)
        W, H = st.size
        tw, th = math.ceil(W / 16), math.ceil(H / 16)
        observe, encode = st.opt("observe"), st.opt("encode")
        with torch.no_grad():
            V, K = cam.viewmat[None].contiguous(), cam.K[None].contiguous()
            radii, m2, d, con, comp = ops.fully_fused_projection(sc.means, None, sc.quats, sc.scales, V, K, W, H, packed=False,
                                                                 near_plane=cam.znear, far_plane=cam.zfar, calc_compensations=True)
            op = (sc.opacities[None, :, 0] * comp).contiguous()
            tpg, ids, fids = ops.isect_tiles(m2, radii, d, 16, tw, th, packed=False, n_cameras=1)
            named = dict(radii=radii, means2d=m2, depths=d, conics=con, compensations=comp, tiles_per_gauss=tpg)
            if observe == "never":
                del ids, fids                  # dropped unobserved: nobody ever settles this call
                return self._hosted(named)
            if encode == "after_touch":
                named["first_key"] = ids[:1].clone()
            elif encode == "after_inplace_write":
                ids.add_(0)
            offs = ops.isect_offset_encode(ids, 1, tw, th)

            def finish():
                # (asked again, possibly after someone else has settled the call and re-pointed the keys: still the frame's)
                named["isect_offsets_asked_again"] = ops.isect_offset_encode(ids, 1, tw, th)
                dirs = sc.means[None] - cam.camera_center
                cols = ops.spherical_harmonics(sc.sh_degree, dirs, sc.sh[None], masks=radii > 0)
                cols = torch.cat((torch.clamp_min(cols + 0.5, 0.0), d[..., None]), dim=-1)
                rc, ra = ops.rasterize_to_pixels(m2, con, cols, op, W, H, 16, offs, fids, backgrounds=None, packed=False)
                named.update(isect_offsets=offs, flatten_ids=fids, isect_ids=ids, colors=cols, render_colors=rc, render_alphas=ra)
                return self._hosted(named)

            if observe == "after_next" and not self.cold:
                self.held = finish
                return None
            if observe == "after_reset":
                if self.cold:
                    self._read_sizes(st)
                self.rendering.reset_state()
                return finish()
            if observe == "other_stream":
                cur = torch.cuda.current_stream()
                if self.side is None:
                    self.side = torch.cuda.Stream()
                self.side.wait_stream(cur)           # what a caller owes its own tensors; the late relaunch is the library's
                with torch.cuda.stream(self.side):
                    out = finish()
                cur.wait_stream(self.side)
                return out
            return finish()

    def finish_held(self):
        with self.torch.no_grad():
            finish, self.held = self.held, None
            return finish()

    def _fused(self, st):
        torch = self.torch
        sc, C, W, H = self.scene(st.scene), st.opt("C"), *st.size
        cams = [self.camera(st.view, st.size, 0.2 * c) for c in range(C)]
        V, K = torch.stack([c.viewmat for c in cams]).contiguous(), torch.stack([c.K for c in cams]).contiguous()
        ctr = torch.stack([c.camera_center for c in cams]).contiguous()
        colors = sc.sh if st.opt("sh") else torch.sigmoid(sc.sh[:, 0, :]).contiguous()
        with torch.no_grad():
            rc, ra, meta = self.ops.rasterization(
                sc.means, sc.quats, sc.scales, sc.opacities.reshape(-1), colors, V, K, W, H, near_plane=cams[0].znear,
                far_plane=cams[0].zfar, sh_degree=sc.sh_degree if st.opt("sh") else None, tile_size=st.opt("tile_size"),
                render_mode=st.opt("render_mode"), rasterize_mode=st.opt("rasterize_mode"), camera_centers_=ctr)
            named = dict(render_colors=rc, render_alphas=ra)
            for k in ("radii", "means2d", "depths", "tiles_per_gauss", "flatten_ids", "isect_offsets", "conics", "opacities", "colors"):
                named[k] = meta[k]
            if dict.__contains__(meta, "isect_ids"):       # (the fused forward's meta would make them with one more isect call)
                named["isect_ids"] = meta["isect_ids"]
            return self._hosted(named)

    def _novel(self, st):
        torch = self.torch
        from harness.caller import render_novel_view
        from street_crafter_amd.layers import novel_view_frame
        fg, sky = self.scene(st.scene, st.opt("n_sky"))
        cam = self.camera(st.view, st.size)
        with torch.no_grad():
            two = render_novel_view(fg, sky, cam, return_intermediates=True)
            named = {k: two[k] for k in FRAME_KEYS}
            named.update({"sky" + k: two["_sky"][k] for k in FRAME_KEYS})
            cat = lambda a, b: torch.cat([a, b]).contiguous()
            one = novel_view_frame(cat(fg.means, sky.means), cat(fg.quats, sky.quats), cat(fg.scales, sky.scales),
                                   cat(fg.opacities, sky.opacities).reshape(-1), cat(fg.sh, sky.sh), cam.viewmat, cam.K,
                                   cam.width, cam.height, fg.n, near_plane=cam.znear, far_plane=cam.zfar,
                                   sh_degree=fg.sh_degree, camera_center=cam.camera_center)
            named.update({"one_pass_" + k: one[k] for k in ("rgb", "acc", "depth")})
            return self._hosted(named)

    def _grouped(self, st):
        from harness.caller import render_all
        sc = self.scene(st.scene)
        gid = (self.torch.arange(sc.n, device=self.DEV) % 3 == 0).to(self.torch.uint8)
        with self.torch.no_grad():
            return self._hosted(render_all(sc, self.camera(st.view, st.size), gid, grouped=True))

    def _train_fwd(self, st):
        import test_param_grad_rows_gpu as PGT
        table, _ = PGT.build_refs()
        p, _ = table[st.opt("case")]
        fwd = {"operators": PGT._forward_operators, "rasterization": PGT._forward_rasterization}[st.opt("route")]
        L, vp, loss = fwd(self.ops, p)
        if not self.cold:
            self.train[st.opt("tag")] = (st.opt("case"), L, vp, loss)
        return self._hosted({"loss": loss})

    def _train_bwd(self, st):
        import test_param_grad_rows_gpu as PGT
        case, L, vp, loss = self.train.pop(st.opt("tag"))
        loss.backward()
        self.torch.cuda.synchronize()
        table, K = PGT.build_refs()
        p, ref = table[case]
        PGT._judge_step(f"history: {case} {st.opt('tag')}", p, ref, K, L, vp)       # the module's own bar, unchanged
        self.judged.append((st.opt("tag"), case))

    def _setter(self, name):
        mod, fn = SWITCHES[name][0].split(".")
        return getattr(getattr(self, mod if mod != "_lib" else "_lib"), fn)

    def _switch(self, st):
        name = st.opt("name")
        prev = self._setter(name)(st.opt("value"))
        self.touched_switches.setdefault(name, prev)

    def restore_switches(self):
        while self.touched_switches:
            name, value = self.touched_switches.popitem()
            self._setter(name)(value)

    def _reset(self, st):
        self.rendering.reset_state(st.opt("device"))
