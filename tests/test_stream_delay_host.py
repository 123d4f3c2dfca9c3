"""Host logic of the delay injector (tests/_delay.py), no GPU: where a launch program may be cut, that a delayed run issues
every record exactly once and in order with one delay on the right stream, that ``delayed_calls`` fires once at the call it was
asked for, and that every patch is gone afterwards.  ``lib.call`` is a recorder throughout: nothing is launched."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _delay  # noqa: E402

HANDLES = (0x1000, 0x2000, 0x3000, 0x4000)


@pytest.fixture(scope="module")
def compiled():
    import models
    from avid_hip import plan
    m = models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128]).train()
    pl = plan.Plan(m, (4, 3, 8, 64, 64), (4, 1, 40, 100), torch.device("cpu"), True, True, True)
    for k, h in enumerate(HANDLES):
        pl.streams[k] = h
    return pl


@pytest.fixture
def recorder(monkeypatch):
    from avid_hip import lib
    calls = []

    def call(name, *args):
        calls.append((name,) + args)
        return ("returned", name)
    monkeypatch.setattr(lib, "call", call)
    return calls


def _handle(v):
    return v.value if isinstance(v, C.c_void_p) else v


def _ranges(calls):
    return [(c[2], c[3]) for c in calls if c[0] == "avid_program_run"]


def _spins(calls):
    return [(c[1], _handle(c[2])) for c in calls if c[0] == "avid_probe_spin"]


def test_cuts_hold_zero_and_the_index_behind_every_wait(compiled):
    from avid_hip import plan
    pl = compiled
    for prog, n in ((pl.fwd_prog, pl.n_fwd), (pl.bwd_prog, pl.n_bwd)):
        cuts = _delay.program_cuts(prog, n)
        waits = [k for k in range(n) if prog[k].op == plan.OP_WAIT]
        assert waits, "a four-stream program without a wait"
        assert cuts[0] == 0 and cuts == sorted(set(cuts))
        assert all(k + 1 in cuts for k in waits)
        assert all(0 <= k <= n for k in cuts)
        assert not any(k < n and prog[k].op == plan.OP_WGRAD_ITEM for k in cuts)
        assert len(cuts) > len(waits) + 1                    # the evenly spaced ones
    assert any(pl.bwd_prog[k].op == plan.OP_WGRAD_ITEM for k in range(pl.n_bwd))     # (the rule above had something to refuse)


def test_an_evenly_spaced_cut_on_a_group_item_moves_to_the_group():
    from avid_hip import plan

    class Rec:
        def __init__(self, op):
            self.op = op
    ops_ = [plan.OP_CONV_FWD] * 18                           # evenly spaced: 2, 4, ..., 16
    ops_[3], ops_[4], ops_[5], ops_[6] = plan.OP_WGRAD_GROUP, plan.OP_WGRAD_ITEM, plan.OP_WGRAD_ITEM, plan.OP_WGRAD_ITEM
    ops_[7] = plan.OP_WAIT
    ops_[15], ops_[16], ops_[17] = plan.OP_WGRAD_GROUP, plan.OP_WGRAD_ITEM, plan.OP_WGRAD_ITEM
    assert _delay.program_cuts([Rec(o) for o in ops_], 18) == [0, 2, 3, 8, 10, 12, 14, 15]
    ops_[17] = plan.OP_WAIT                                  # a wait as the last record: the cut behind it is the program's end
    assert _delay.program_cuts([Rec(o) for o in ops_], 18)[-1] == 18


@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("stream_index", [0, 1, 2, 3])
def test_a_delayed_run_issues_every_record_once_with_one_delay(compiled, recorder, which, stream_index):
    pl = compiled
    prog, n = (pl.fwd_prog, pl.n_fwd) if which == "fwd" else (pl.bwd_prog, pl.n_bwd)
    other, n_other = (pl.bwd_prog, pl.n_bwd) if which == "fwd" else (pl.fwd_prog, pl.n_fwd)
    for cut in _delay.program_cuts(prog, n):
        del recorder[:]
        with _delay.delayed_programs(stream_index, cut, 7.5, which) as fired:
            pl._run(prog, 0, n)
            pl._run(other, 0, n_other)                       # the other program passes through
        ranges = _ranges(recorder)
        mine = [r for c, r in zip([c for c in recorder if c[0] == "avid_program_run"], ranges) if c[1] is prog]
        assert [r for r in mine if r[0] != r[1]] == [r for r in ((0, cut), (cut, n)) if r[0] != r[1]], (cut, mine)
        assert ranges[-1] == (0, n_other) and recorder[-1][1] is other
        assert _spins(recorder) == [(7500, HANDLES[stream_index])] and fired.spins == 1
        # the delay sits between the two halves
        names = [c[0] for c in recorder[:-1]]
        assert names == ["avid_program_run"] * (cut > 0) + ["avid_probe_spin"] + ["avid_program_run"] * (cut < n)


def test_segments_tile_their_range_and_a_cut_outside_injects_nothing(compiled, recorder):
    pl = compiled
    n = pl.n_bwd
    cuts = _delay.program_cuts(pl.bwd_prog, n)
    inner = [c for c in cuts if 0 < c < n]
    a, b = inner[len(inner) // 3], inner[2 * len(inner) // 3]
    segments = [(0, a), (a, b), (b, n)]
    for cut in cuts:
        del recorder[:]
        with _delay.delayed_programs(2, cut, 5, "bwd") as fired:
            for begin, end in segments:
                pl._run(pl.bwd_prog, begin, end)
        ranges = [r for r in _ranges(recorder) if r[0] != r[1]]
        assert ranges[0][0] == 0 and ranges[-1][1] == n
        assert all(x[1] == y[0] for x, y in zip(ranges, ranges[1:])), (cut, ranges)      # tiled exactly once, in order
        assert fired.spins == 1 and len(_spins(recorder)) == 1, (cut, _spins(recorder))
    # one segment alone: a cut outside it issues no delay and leaves the call as it was
    for cut in (0, b, n):
        del recorder[:]
        with _delay.delayed_programs(2, cut, 5, "bwd") as fired:
            pl._run(pl.bwd_prog, a, b)
        assert _ranges(recorder) == [(a, b)] and not _spins(recorder) and fired.spins == 0, cut


def test_visit_selects_one_run_of_the_program(compiled, recorder):
    pl = compiled
    cut = _delay.program_cuts(pl.fwd_prog, pl.n_fwd)[2]
    with _delay.delayed_programs(1, cut, 5, "fwd", visit=1) as fired:
        for _ in range(3):
            pl._run(pl.fwd_prog, 0, pl.n_fwd)
    assert _ranges(recorder) == [(0, pl.n_fwd), (0, cut), (cut, pl.n_fwd), (0, pl.n_fwd)]
    assert fired.spins == 1 and _spins(recorder) == [(5000, HANDLES[1])]


def test_spin_chains_launches_of_at_most_fifty_milliseconds(recorder):
    assert _delay.spin(HANDLES[0], 120) == 3
    assert _spins(recorder) == [(50000, HANDLES[0]), (50000, HANDLES[0]), (20000, HANDLES[0])]
    del recorder[:]
    assert _delay.spin(C.c_void_p(HANDLES[3]), 50) == 1 and _spins(recorder) == [(50000, HANDLES[3])]
    from avid_hip import lib
    assert all(us < 100000 for us, _ in _spins(recorder))
    assert lib.SIGNATURES["avid_probe_spin"][1][0] is C.c_int


def test_delay_length():
    assert _delay.delay_ms(0.2) == 5.0 and _delay.delay_ms(4.0) == 12.0 and _delay.delay_ms(50.0) == 150.0
    with pytest.raises(ValueError):
        _delay.delay_ms(50.1)


class _Stream:
    def __init__(self, h):
        self.cuda_stream = h


@pytest.fixture
def fake_set(monkeypatch):
    from avid_hip import streams
    ss = streams.StreamSet(*[_Stream(h) for h in HANDLES], {"probed": False})
    monkeypatch.setattr(streams, "current_set", lambda device: ss)
    return ss


SEQUENCE = ["avid_conv_fwd_workspace_bytes", "avid_conv_fwd", "avid_conv_uses_wino", "avid_bn_fwd_train", "avid_conv_kernel_name",
            "avid_last_error", "avid_program_run", "avid_conv_takes_in_affine", "avid_stream_wait", "avid_wino_configure",
            "avid_debug_presplit_launches", "avid_adam_flat", "avid_conv_fwd_stats_rows"]
LAUNCHING = ["avid_conv_fwd", "avid_bn_fwd_train", "avid_program_run", "avid_stream_wait", "avid_adam_flat"]


def test_delayed_calls_fires_once_at_the_nth_launching_call(recorder, fake_set):
    from avid_hip import lib
    dev = torch.device("cpu")
    assert [n for n in SEQUENCE if _delay.launches(n)] == LAUNCHING
    with _delay.delayed_calls(0, None, 5, device=dev) as dry:
        for name in SEQUENCE:
            lib.call(name, 1, 2)
    assert dry.count == len(LAUNCHING) and dry.names == LAUNCHING and dry.spins == 0 and not _spins(recorder)
    for nth in range(len(LAUNCHING)):
        for stream_index in range(4):
            del recorder[:]
            with _delay.delayed_calls(stream_index, nth, 5, device=dev) as fired:
                got = [lib.call(name, 1, 2) for name in SEQUENCE]
            assert got == [("returned", name) for name in SEQUENCE]           # what lib.call returns
            names = [c[0] for c in recorder]
            at = names.index("avid_probe_spin")
            assert names[:at] + names[at + 1:] == SEQUENCE and names[at + 1] == LAUNCHING[nth]
            assert names[:at].count(LAUNCHING[nth]) == 0
            assert _spins(recorder) == [(5000, HANDLES[stream_index])] and fired.spins == 1 and fired.count == len(LAUNCHING)
    del recorder[:]
    with _delay.delayed_calls(0, len(LAUNCHING), 5, device=dev) as fired:      # past the last call: nothing
        for name in SEQUENCE:
            lib.call(name)
    assert fired.spins == 0 and not _spins(recorder)


def test_every_patch_is_restored_also_after_an_exception(recorder, fake_set):
    from avid_hip import lib, plan
    run0, call0 = plan.Programs._run, lib.call
    with _delay.delayed_programs(0, 0, 5, "fwd"):
        assert plan.Programs._run is not run0
    assert plan.Programs._run is run0
    with pytest.raises(KeyError):
        with _delay.delayed_programs(0, 0, 5, "fwd"):
            raise KeyError("x")
    assert plan.Programs._run is run0
    with _delay.delayed_calls(0, 0, 5, device=torch.device("cpu")):
        assert lib.call is not call0
    assert lib.call is call0
    with pytest.raises(KeyError):
        with _delay.delayed_calls(0, 0, 5, device=torch.device("cpu")):
            lib.call("avid_conv_fwd")
            raise KeyError("x")
    assert lib.call is call0

    def boom(name, *args):
        if name == "avid_probe_spin":
            raise RuntimeError("spin failed")
    lib.call = boom
    try:
        with pytest.raises(RuntimeError):
            with _delay.delayed_calls(0, 0, 5, device=torch.device("cpu")):
                lib.call("avid_conv_fwd")
        assert lib.call is boom
    finally:
        lib.call = call0
