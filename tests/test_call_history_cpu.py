"""No-GPU checks of tests/call_history.py: the programs contain the transitions they declare (computed, not typed in), the
generator is deterministic and well formed, the host model does the bookkeeping of street_crafter_amd/isect.py on synthetic
size tables, and three deliberately broken MODELS -- never broken library code -- are told apart by the named programs."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_history as H  # noqa: E402


@pytest.mark.parametrize("name", list(H.PROGRAMS))
def test_named_program_contains_what_it_declares(name):
    program, declared = H.PROGRAMS[name]
    assert 25 <= len(program) <= 60, len(program)
    assert H.check_well_formed(program)
    got = H.transitions(program)
    assert got == declared, (sorted(got - declared), sorted(declared - got))


def test_named_programs_cover_every_transition():
    union = frozenset().union(*(declared for _, declared in H.PROGRAMS.values()))
    assert union == H.ALL_TRANSITIONS, sorted(H.ALL_TRANSITIONS ^ union)
    assert H.LEFT_OUT == ("radix_fallback_between_bucketed",)
    # every kind, observation, encode variant and switch of the vocabulary is used by some named program
    steps = [st for program, _ in H.PROGRAMS.values() for st in program]
    assert {st.kind for st in steps} == set(H.KINDS)
    assert {st.opt("observe") for st in steps if st.kind == "operators"} == set(H.OBSERVE)
    assert {st.opt("encode") for st in steps if st.kind == "operators"} == set(H.ENCODE)
    assert {st.opt("name") for st in steps if st.kind == "switch"} == set(H.SWITCHES)
    assert {(st.opt("case"), st.opt("route")) for st in steps if st.kind == "train_fwd"} >= {("two_cameras", "rasterization"), ("plain", "operators")}


def test_eviction_program_has_65_distinct_keys_at_the_smallest_frame():
    program, _ = H.PROGRAMS["evictions"]
    keys = {c.key for st in program for c in H.calls_of(st)}
    assert len(keys) > H.KEYS_MAX and all(k[3:] == (16, 4, 3) for k in keys)
    assert len({k[2] for k in keys}) == len(keys)                   # all values of N


def test_train_cases_match_the_oracle_cases():
    from oracle import param_grad_f64 as PG
    for case, (C, N, W, H_) in H.TRAIN_CASES.items():
        spec = PG.CASES[case]
        assert case in PG.CASE_IDS and len(spec["cams"]) == C and spec["scene"]["n"] == N
        assert (spec["cams"][0]["width"], spec["cams"][0]["height"]) == (W, H_)
    s = H._train_scene("plain")
    assert PG.CASES["plain"]["scene"] == dict(n=s.n, seed=s.seed, **H.SHAPES[s.shape])


@pytest.mark.parametrize("seed", H.SEEDS)
def test_generator_is_deterministic_and_well_formed(seed):
    a, b = H.random_program(seed), H.random_program(seed)
    assert a == b and len(a) == H.RANDOM_STEPS
    assert H.check_well_formed(a)
    assert a != H.random_program(seed + 1)
    H.replay(a)                                           # the model takes every step of the vocabulary
    assert len({st.kind for st in a}) >= 5


def test_generator_pairs_and_restores_at_any_length():
    for seed in range(40):
        for n in (12, 25, 40):
            assert H.check_well_formed(H.random_program(seed, n))


# ---- the host model on synthetic size tables --------------------------------------------------------------------------
def _events(model, key_step, table):
    out = []
    for i, sizes in enumerate(table):
        own, settled = model.step(i, key_step, [sizes])
        out.append(own[0].event)
    return out


def test_model_head_room():
    st = H.frame(H.scene(5000, 1))
    base = (10000, 6000, 400)
    cap, rec, sup = 10000 + 1250 + 4096, 6000 + 750 + 4096, 400 + 50 + 64
    assert _events(H.HostModel(), st, [base, base]) == ["first", "speculative_ok"]
    assert _events(H.HostModel(), st, [base, (cap, rec, sup)]) == ["first", "speculative_ok"]
    for over in ((cap + 1, rec, sup), (cap, rec + 1, sup), (cap, rec, sup + 1)):
        assert _events(H.HostModel(), st, [base, over]) == ["first", "exact_relaunch"], over
    # the prediction covers the LARGEST of the last eight calls: a fuller view is remembered across seven emptier ones ...
    small = (100, 50, 10)
    assert _events(H.HostModel(), st, [base] + [small] * 7 + [base]) == ["first"] + ["speculative_ok"] * 8
    # ... and is forgotten by the eighth
    assert _events(H.HostModel(), st, [base] + [small] * 8 + [base])[-1] == "exact_relaunch"


def test_model_clamps_the_head_room_at_the_bucket_capacity():
    st = H.frame(H.scene(5000, 1))
    below = (10000, 6000, 3300)                     # 3300 + 412 + 64 would provision 3776 > 3584
    assert _events(H.HostModel(), st, [below, (10000, 6000, H.BUCKET_CAP)]) == ["first", "speculative_ok"]
    assert _events(H.HostModel(), st, [below, (10000, 6000, H.BUCKET_CAP + 1)]) == ["first", "exact_relaunch"]
    # a frame that did exceed it is provisioned for with head-room again
    over = (10000, 6000, 4000)
    assert _events(H.HostModel(), st, [over, (10000, 6000, 4500)]) == ["first", "speculative_ok"]


def test_model_prunes_the_oldest_shape_first():
    m = H.HostModel()
    steps = [H.frame(H.scene(300 + i, 1), size=(64, 48)) for i in range(H.KEYS_MAX + 1)]
    for i, st in enumerate(steps):
        m.step(i, st, [(100, 50, 10)])
    assert len(m.history) == len(m.prediction) == len(m.last_meta) == H.KEYS_MAX
    assert H.calls_of(steps[0])[0].key not in m.prediction and H.calls_of(steps[1])[0].key in m.prediction
    own, _ = m.step(99, steps[1], [(100, 50, 10)])
    assert own[0].event == "speculative_ok"
    own, _ = m.step(100, steps[0], [(100, 50, 10)])
    assert own[0].event == "first" and m.returned_to_pruned == 1
    # ... which pushed the next oldest out: oldest by FIRST call, the use a moment ago does not count
    assert H.calls_of(steps[1])[0].key not in m.prediction and H.calls_of(steps[2])[0].key in m.prediction


def test_model_keeps_eight_hint_buffers_lru():
    m = H.HostModel()
    steps = [H.frame(H.scene(300 + i, 1), size=(64, 48)) for i in range(9)]
    for i, st in enumerate(steps[:8]):
        m.step(i, st, [(100, 50, 10)])
    m.step(8, steps[0], [(100, 50, 10)])             # used again: the second shape is now the oldest
    m.step(9, steps[8], [(100, 50, 10)])
    assert (0, 1, 301, 4, 3) in m.evicted and (0, 1, 300, 4, 3) in m.tile_work
    m.step(10, steps[1], [(100, 50, 10)])
    assert m.returned_to_evicted == 1


def test_model_resets_per_device():
    m = H.HostModel()
    for dev in (0, 1):
        m._record((dev, 1, 1000, 16, 4, 3), (100, 50, 10))
        m._work((dev, 1, 1000, 16, 4, 3))
    m.reset(1)
    assert list(m.prediction) == [(0, 1, 1000, 16, 4, 3)] and list(m.tile_work) == [(0, 1, 1000, 4, 3)]
    m.reset(None)
    assert not m.prediction and not m.history and not m.last_meta and not m.tile_work


def test_model_next_call_settles_the_pending_one():
    a, b = H.scene(3000, 1), H.scene(500, 3)
    program = [H.frame(a), H.operators(a, observe="after_next"), H.frame(b, size=(64, 48)), H.operators(a, observe="never"),
               H.operators(a, observe="after_reset"), H.frame(a)]
    _, out = H.replay(program)
    assert [[(s.origin, s.event, s.settler) for s in settled] for _, settled in out] == [
        [(0, "first", "self")], [], [(1, "speculative_ok", "successor"), (2, "first", "self")], [],
        [(4, "speculative_ok", "reset")], [(5, "first", "self")]]
    assert H.HostModel.stats_delta(out[2][1]) == {"calls": 2, "speculative_ok": 1, "exact_relaunch": 0}
    assert out[3][0][0].settler is None                            # dropped: in nobody's statistics


# ---- discrimination: the programs are not vacuous ----------------------------------------------------------------------
@pytest.mark.parametrize("broken", [dict(key_without_n=True), dict(ignore_max_super=True), dict(successor_settles=False)],
                         ids=["keyed_without_N", "max_super_ignored", "pending_not_settled_by_next_call"])
def test_a_broken_model_is_told_apart_by_a_named_program(broken):
    differs = [name for name, (program, _) in H.PROGRAMS.items()
               if H.event_sequence(program) != H.event_sequence(program, **broken)]
    print(broken, "->", differs)
    assert differs


# ---- the comparison itself ------------------------------------------------------------------------------------------------
def test_first_difference_is_bitwise_and_names_the_element():
    import numpy as np
    a = {"x": np.arange(6, dtype=np.float32).reshape(2, 3), "ids": np.arange(4, dtype=np.int64)}
    same = {k: v.copy() for k, v in a.items()}
    assert H.first_difference(a, same) is None
    b = {k: v.copy() for k, v in a.items()}
    b["x"][1, 1] = np.nextafter(np.float32(4.0), np.float32(5.0))            # one ulp
    assert H.first_difference(a, b).startswith("x: element 4 of 6")
    z = {"x": a["x"].copy() * 0, "ids": a["ids"]}
    nz = {"x": -z["x"], "ids": a["ids"]}                                     # -0.0 == 0.0, but not bit for bit
    assert H.first_difference(z, nz) is not None
    nan = {"x": np.full((2, 3), np.nan, np.float32), "ids": a["ids"]}
    assert H.first_difference(nan, {k: v.copy() for k, v in nan.items()}) is None
    assert "int64[3]" in H.first_difference(a, {"x": a["x"], "ids": a["ids"][:3]})       # a shorter id list
    assert "one side only" in H.first_difference(a, {"x": a["x"]})
