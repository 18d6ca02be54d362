"""Call HISTORIES against cold-state renders: every call of a scripted history returns, bit for bit, what the same call
returns right after `reset_state()` -- the promise `reset_state()` and the A/B switches make (tests/call_history.py has the
vocabulary, the programs and the host model).

Per program: a cold pass (each distinct step alone, from a reset state, outputs copied to the host), then ONE warm pass of
the whole program.  After every warm step
  * every forward output equals the cold one as bytes (planar / interleaved forms by value, lengths of the id lists included);
  * a training step's gradients pass `test_param_grad_rows_gpu._judge_step`: the float64 references and the per-row bar of
    that module, unchanged -- a warm step passes exactly the bar a cold step passes;
  * the delta of `_STATE.stats` equals what `HostModel` says from the COLD sizes, and the prediction / history / hint tables
    hold what the model holds: a program really mispredicted, deferred and relaunched where it claims to;
  * nothing was logged on "street_crafter_amd".
A failure names the program, the step and the first differing output, and prints the prefix that reproduces it."""
import logging
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_history as H  # noqa: E402

_COLD = {}          # step content -> (outputs, sizes): computed once, shared by every test of the module, never changed


def _rendering():
    from street_crafter_amd import _lib, rendering
    _lib.load()
    assert int(_lib.load().sc_isect_bin_bucket_capacity()) == H.BUCKET_CAP
    return rendering


def _cold(step):
    content = H.content_of(step)
    if content not in _COLD:
        rendering = _rendering()
        rendering.reset_state()
        runner = H.Runner(cold=True)
        out = runner.run(content)
        torch.cuda.synchronize()
        assert all(s is not None for s in runner.sizes), (str(content), runner.sizes)
        for a in out.values():
            a.setflags(write=False)
        _COLD[content] = (out, list(runner.sizes))
        rendering.reset_state()
    return _COLD[content]


def _fail(name, program, i, what):
    prefix = "\n".join(f"  {j:2d}  {st}" for j, st in enumerate(program[:i + 1]))
    pytest.fail(f"program {name!r}, step {i} ({program[i]}): {what}\nthe prefix that reproduces it:\n{prefix}", pytrace=False)


def _run_history(name, program, caplog):
    rendering = _rendering()
    H.check_well_formed(program)
    for st in program:                                   # the cold pass, under the default switches
        if H.has_outputs(st):
            _cold(st)
    rendering.reset_state()
    model, runner, report = H.HostModel(), H.Runner(), []
    compared = [0, 0]                                    # output arrays, bytes
    stats, state = rendering._STATE.stats, rendering._STATE
    caplog.clear()
    try:
        with caplog.at_level(logging.WARNING, logger="street_crafter_amd"):
            for i, st in enumerate(program):
                before = dict(stats)
                try:
                    out = runner.run(st)
                except AssertionError as e:              # (a training step judged against its float64 reference)
                    _fail(name, program, i, f"{type(e).__name__}: {e}")
                if runner.held is not None and st.opt("observe") != "after_next":
                    held = runner.finish_held()          # the previous step's outputs, looked at only now
                    diff = H.first_difference(_cold(program[i - 1])[0], held)
                    compared[0], compared[1] = compared[0] + len(held), compared[1] + sum(a.nbytes for a in held.values())
                    if diff:
                        _fail(name, program, i - 1, "observed after the next call: " + diff)
                elif runner.held is not None and i and program[i - 1].opt("observe") == "after_next":
                    _fail(name, program, i, "two after_next steps in a row are not supported by the runner")
                if out is not None:
                    diff = H.first_difference(_cold(st)[0], out)
                    compared[0], compared[1] = compared[0] + len(out), compared[1] + sum(a.nbytes for a in out.values())
                    if diff:
                        _fail(name, program, i, diff)
                own, settled = model.step(i, st, _cold(st)[1] if H.has_outputs(st) else [])
                delta = {k: stats[k] - before[k] for k in before}
                if delta != H.HostModel.stats_delta(settled):
                    _fail(name, program, i, f"stats moved by {delta}, the host model says {H.HostModel.stats_delta(settled)} "
                                            f"from {[(s.origin, s.event, s.settler) for s in settled]}")
                if state.prediction != model.prediction or list(state.history) != list(model.history):
                    _fail(name, program, i, "the prediction / history tables are not the host model's: "
                                            f"{sorted(set(state.prediction.items()) ^ set(model.prediction.items()))[:4]}")
                if [list(h) for h in state.history.values()] != [list(h) for h in model.history.values()]:
                    _fail(name, program, i, "the size histories are not the host model's")
                if list(state.tile_work) != list(model.tile_work):
                    _fail(name, program, i, f"hint buffers {list(state.tile_work)}, the host model keeps {list(model.tile_work)}")
                if caplog.records:
                    _fail(name, program, i, f"logged: {[r.getMessage() for r in caplog.records]}")
                report.append((own, settled))
        assert not runner.train and runner.held is None
        assert compared[0] >= sum(H.has_outputs(st) for st in program)
        print(f"[history] {name}: {compared[0]} output arrays ({compared[1] / 1e6:.1f} MB) equal to their cold renders")
    finally:
        runner.restore_switches()
        runner.train.clear()
        rendering.reset_state()
    return model, report


def _counts(model, report):
    settled = [s for _, ss in report for s in ss]
    c = {e: sum(s.event == e for s in settled) for e in ("first", "speculative_ok", "exact_relaunch")}
    c["late_relaunch"] = sum(s.event == "exact_relaunch" and s.deferred and s.settler != "self" for s in settled)
    c["by_successor"] = sum(s.settler == "successor" for s in settled)
    c["dropped"] = sum(s.settler is None for own, _ in report for s in own)
    c["evicted_and_back"], c["pruned_and_back"] = model.returned_to_evicted, model.returned_to_pruned
    return c


@pytest.mark.parametrize("name", list(H.PROGRAMS))
def test_named_history_equals_cold_renders(name, caplog):
    program, declared = H.PROGRAMS[name]
    t0 = time.time()
    model, report = _run_history(name, program, caplog)
    print(f"[history] {name}: {len(program)} steps, {len({H.content_of(s) for s in program if H.has_outputs(s)})} cold renders, "
          f"{time.time() - t0:.1f} s; model events {_counts(model, report)}")
    # the transitions the program declares, now from the MEASURED sizes: it mispredicts where it says it does
    measured = H.transitions(program, lambda st: _cold(st)[1] if H.has_outputs(st) else [])
    assert measured == declared, (sorted(measured - declared), sorted(declared - measured))


@pytest.mark.parametrize("seed", H.SEEDS)
def test_seeded_history_equals_cold_renders(seed, caplog):
    program = H.random_program(seed)
    t0 = time.time()
    model, report = _run_history(f"random_program({seed})", program, caplog)
    print(f"[history] seed {seed}: {len(program)} steps, {time.time() - t0:.1f} s; model events {_counts(model, report)}")


def test_the_named_histories_really_mispredict_defer_and_evict():
    """Conditions on the programs, from the measured cold sizes (the cold renders are shared with the tests above)."""
    total = {}
    for name, (program, _) in H.PROGRAMS.items():
        model, report = H.replay(program, lambda st: _cold(st)[1] if H.has_outputs(st) else [])
        c = _counts(model, report)
        print(f"[history] {name}: {c}")
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    print(f"[history] all named programs: {total}")
    assert total["exact_relaunch"] >= 6 and total["late_relaunch"] >= 2, total
    assert total["by_successor"] >= 4, total
    assert total["evicted_and_back"] >= 1 and total["pruned_and_back"] >= 1, total
    # the one over-capacity step: its largest super-tile is above the bucket capacity, its predecessors' below
    mixed = H.PROGRAMS["mixed"][0]
    over = [i for i, st in enumerate(mixed) if st.scene is not None and st.scene.shape == "cluster"]
    assert over and _cold(mixed[over[0]])[1][0][2] > H.BUCKET_CAP >= _cold(mixed[over[0] - 1])[1][0][2]
    assert _cold(mixed[over[0]])[1][0][2] <= H.BUCKET_CAP + 512          # ... and it is the smallest builder that does
