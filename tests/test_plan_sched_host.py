"""Launch-plan schedules, edge by edge, without a GPU: lic_plan_sched_host (the stream assignment of lic_plan_create,
the list scheduler of lic_plan_tune, add_events and the command-list builder of lic_plan_replay, on a caller's DAG)
against the vector-clock model of tests/plan_sched_ref.py.  The eager-equality tests of test_gpu_plan.py see a missing
wait only when the race is lost on that run; the model sees it always."""
import os

import pytest

import plan_sched_ref as R
from plan_sched_ref import LAUNCH, RECORD, WAIT, EV_FIRST, EV_FORK, EV_JOIN

SEEDS = {g: 200 for g in R.GENERATORS}
SEEDS[R.single] = 20   # (one operation: nothing but its duration and flags varies)
# every schedule the library can make of a DAG: (mode, streams, wide_min_us)
SCHEDULES = [(R.CAPTURE_ORDER, 3, 0.0)] + [(R.LIST_SCHEDULE, ns, wm) for ns in (1, 2, 3) for wm in R.WIDE_MIN_US]


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _cases(seeds_per_generator):
    for gen in R.GENERATORS:
        for seed in range(min(SEEDS[gen], seeds_per_generator)):
            yield gen, seed, gen(seed)


@pytest.mark.parametrize("gen", R.GENERATORS, ids=lambda g: g.__name__)
def test_every_schedule_honours_every_edge(lib, gen):
    """every generator over its seeds; capture order and the list scheduler at 1, 2 and 3 streams for each wide_min_us of
    lic_plan_tune; each replayed with 0, 1 and 2 side streams: the model finds nothing"""
    waits = implied = lists = largest = 0
    for seed in range(SEEDS[gen]):
        dag = gen(seed)
        largest = max(largest, dag.n)
        for mode, ns, wm in SCHEDULES:
            for n_sides in (0, 1, 2):
                cmds = R.host_commands(lib, dag, mode, ns, wm, n_sides)
                bad, stats = R.violations(dag, cmds, n_sides)
                assert not bad, (gen.__name__, seed, mode, ns, wm, n_sides, bad[:3])
                assert max(stats["streams"]) <= min(n_sides, 2 if mode == R.CAPTURE_ORDER else ns - 1)
                lists += 1
                if n_sides == 2:   # (folded replays make more waits no-ops; the figure is for distinct streams)
                    waits += stats["waits"]
                    implied += stats["implied_waits"]
    # a figure for later work on the replay's host time, not a requirement
    print(f"\n{gen.__name__}: {lists} command lists (largest DAG {largest} operations), on three distinct streams "
          f"{waits} waits, {implied} of them implied by earlier waits")


def test_generators_cover_what_they_claim():
    sizes = {g: [g(s).n for s in range(SEEDS[g])] for g in R.GENERATORS}
    assert max(sizes[R.sparse_random]) >= 200 and max(sizes[R.training_step]) >= 150 and set(sizes[R.single]) == {1}
    roots = [sum(1 for p in R.several_roots(s).preds if not p) for s in range(20)]
    assert min(roots) >= 2
    d = R.training_step(3)
    assert any(f & R.FILLER for f in d.flags) and any(f & R.WIDE for f in d.flags) and not all(f & R.WIDE for f in d.flags)
    assert 0.5 <= min(d.us) and max(max(R.sparse_random(s).us) for s in range(50)) > 200.0
    assert max(len(p) for s in range(20) for p in R.fan(s).preds) >= 20        # fan-in


def test_host_entry_validates_its_arguments(lib):
    import ctypes as C
    n = C.c_int64()
    ptr, idx, us, fl = (C.c_int32 * 3)(0, 0, 1), (C.c_int32 * 1)(0), (C.c_double * 2)(1.0, 1.0), (C.c_int32 * 2)()
    ok = (2, ptr, idx, us, fl, 1, 3, 25.0, 2)
    assert lib.lic_plan_sched_host(*ok, 0, C.byref(n), None, None) == 0 and n.value == 9
    buf = (C.c_int32 * 27)()
    assert lib.lic_plan_sched_host(*ok, 9, C.byref(n), buf, None) == 0
    assert lib.lic_plan_sched_host(*ok, 8, C.byref(n), buf, None) == -4            # LIC_ERR_WORKSPACE
    assert lib.lic_plan_sched_host(*ok, 9, C.byref(n), None, None) == -1
    assert lib.lic_plan_sched_host(*ok, 9, None, buf, None) == -1
    for bad in ((0,) + ok[1:], ok[:1] + (None,) + ok[2:], ok[:3] + (None,) + ok[4:], ok[:4] + (None,) + ok[5:],
                ok[:5] + (2,) + ok[6:], ok[:6] + (0,) + ok[7:], ok[:6] + (4,) + ok[7:], ok[:8] + (3,), ok[:8] + (-1,)):
        assert lib.lic_plan_sched_host(*bad, 9, C.byref(n), buf, None) == -1, bad
    forward = (C.c_int32 * 1)(1)                                                     # a predecessor that is not earlier
    assert lib.lic_plan_sched_host(2, ptr, forward, us, fl, 0, 3, 0.0, 2, 9, C.byref(n), buf, None) == -1
    assert lib.lic_plan_commands(None, 1, 0, C.byref(n), None) == -1
    assert lib.lic_plan_dag(None, 0, 0, None, None, None, None, None, None) == -1


# ---- the model would notice ------------------------------------------------------------------------------------------

def _mutant_cases(lib, seeds=12):
    """valid lists to mutate: every generator, capture order and one list schedule, two and three physical streams"""
    for gen, seed, dag in _cases(seeds):
        for mode, ns, wm in (SCHEDULES[0], SCHEDULES[-2]):
            for n_sides in (1, 2):
                cmds = R.host_commands(lib, dag, mode, ns, wm, n_sides)
                assert not R.violations(dag, cmds, n_sides)[0]
                yield dag, cmds, n_sides


def _rules(dag, cmds, n_sides):
    return {rule for rule, _ in R.violations(dag, cmds, n_sides)[0]}


def test_mutant_without_any_wait(lib):
    """all waits removed: an edge is reported exactly when some edge crosses physical streams, and work on a side stream
    is no longer joined (with everything on the caller's stream the waits were for idle streams: still valid)"""
    seen = {True: 0, False: 0}
    for dag, cmds, n_sides in _mutant_cases(lib):
        mutant = [c for c in cmds if c[0] != WAIT]
        assert len(mutant) < len(cmds)
        on = R.stream_of(cmds)
        crosses = any(on[q] != on[k] for q, k in dag.edges())
        rules = _rules(dag, mutant, n_sides)
        assert ("edge" in rules) == crosses, (dag.preds, mutant)
        assert ("marker" in rules) == any(s != 0 for s in on.values())
        seen[crosses] += 1
    assert seen[True] >= 20 and seen[False] >= 20, seen


def test_mutant_launch_before_its_predecessor(lib):
    done = 0
    for dag, cmds, n_sides in _mutant_cases(lib):
        if not dag.edges():
            continue
        q, k = dag.edges()[len(dag.edges()) // 2]
        ik = cmds.index(next(c for c in cmds if c[0] == LAUNCH and c[2] == k))
        mutant = cmds[:ik] + cmds[ik + 1:]
        iq = mutant.index(next(c for c in mutant if c[0] == LAUNCH and c[2] == q))
        mutant.insert(iq, cmds[ik])
        rules = _rules(dag, mutant, n_sides)
        assert "issue-order" in rules and "edge" in rules, (q, k, rules)
        done += 1
    assert done >= 100


def test_mutant_wait_for_an_event_recorded_later(lib):
    done = 0
    for dag, cmds, n_sides in _mutant_cases(lib):
        waits = [i for i, c in enumerate(cmds) if c[0] == WAIT]
        i = waits[(len(waits) - 1) // 2]                  # (not the last one: that is a join's)
        later = [c[2] for c in cmds[i + 1:] if c[0] == RECORD]
        assert later                                       # (the joins at the least)
        mutant = list(cmds)
        mutant[i] = (WAIT, cmds[i][1], later[0])
        assert "wait-without-record" in _rules(dag, mutant, n_sides)
        done += 1
    assert done >= 100


def test_mutant_event_recorded_twice(lib):
    done = 0
    for dag, cmds, n_sides in _mutant_cases(lib):
        records = [c for c in cmds if c[0] == RECORD]
        again = records[len(records) // 2]
        mutant = cmds + [(RECORD, 0, again[2])]
        assert "record-twice" in _rules(dag, mutant, n_sides)
        done += 1
    assert done >= 100


def test_diamond_on_two_streams_by_hand(lib):
    """0 -> 1 -> 3 on the caller's stream, 0 -> 2 -> 3 through the side stream: the list written out by hand is what the
    library issues; without the wait that carries 0 -> 2, or the one that carries 2 -> 3, the model names that edge"""
    dag = R.Dag([[], [0], [0], [1, 2]])
    e0, e1 = EV_FIRST, EV_FIRST + 1
    by_hand = [(RECORD, 0, EV_FORK), (WAIT, 1, EV_FORK),
               (LAUNCH, 0, 0), (RECORD, 0, e0), (LAUNCH, 0, 1),
               (WAIT, 1, e0), (LAUNCH, 1, 2), (RECORD, 1, e1),
               (WAIT, 0, e1), (LAUNCH, 0, 3),
               (RECORD, 1, EV_JOIN), (WAIT, 0, EV_JOIN)]
    assert R.host_commands(lib, dag, R.CAPTURE_ORDER, n_sides=1) == by_hand
    assert R.check(dag, by_hand, 1)["implied_waits"] == 0
    for wait, edge in (((WAIT, 1, e0), "0 -> 2"), ((WAIT, 0, e1), "2 -> 3")):
        mutant = [c for c in by_hand if c != wait]
        assert len(mutant) == len(by_hand) - 1
        bad = R.violations(dag, mutant, 1)[0]
        assert {rule for rule, _ in bad} == {"edge"} and all(edge in why for _, why in bad), bad
    # the fork's wait is implied here: the side stream's first operation waits for operation 0 anyway
    assert not _rules(dag, [c for c in by_hand if c != (WAIT, 1, EV_FORK)], 1)
    # on one stream the same schedule is four launches and the (no-op) waits and records between them
    one = R.host_commands(lib, dag, R.CAPTURE_ORDER, n_sides=0)
    assert [c for c in one if c[0] == LAUNCH] == [(LAUNCH, 0, k) for k in range(4)] and R.check(dag, one, 0)["implied_waits"] == 2


def test_fork_keeps_a_root_on_a_side_stream_behind_the_previous_replay(lib):
    """two independent 50 us operations: the list scheduler starts the second one on the side stream, where only the
    fork's wait orders it after what precedes the plan on the caller's stream"""
    dag = R.Dag([[], []], [50.0, 50.0], [0, 0])
    cmds = R.host_commands(lib, dag, R.LIST_SCHEDULE, 2, 1e30, 1)
    assert cmds == [(RECORD, 0, EV_FORK), (WAIT, 1, EV_FORK), (LAUNCH, 0, 0), (LAUNCH, 1, 1),
                    (RECORD, 1, EV_JOIN), (WAIT, 0, EV_JOIN)]
    R.check(dag, cmds, 1)
    assert _rules(dag, [c for c in cmds if c != (WAIT, 1, EV_FORK)], 1) == {"replay-order"}
    assert _rules(dag, [c for c in cmds if c != (WAIT, 0, EV_JOIN)], 1) == {"marker", "replay-order"}


# ---- the schedule is useful, not only safe ---------------------------------------------------------------------------

def test_single_chain_stays_on_one_stream_without_events(lib):
    for seed in range(10):
        dag = R.single_chain(seed)
        for mode, ns, wm in SCHEDULES:
            cmds, info = R.host_commands(lib, dag, mode, ns, wm, 2, with_info=True)
            assert set(R.stream_of(cmds).values()) == {0} and info == {"on_side": 0, "events": 0}
            assert not [c for c in cmds if c[0] != LAUNCH and c[2] >= EV_FIRST]


def test_two_chains_behind_a_fork_take_two_streams(lib):
    """a root, then two independent chains of 50 us operations (long against the 6 us a cross-stream edge is charged)"""
    for length in (1, 5, 30):
        preds, chains = [[]], ([], [])
        for i in range(length):
            for c in (0, 1):
                preds.append([chains[c][-1] if chains[c] else 0])
                chains[c].append(len(preds) - 1)
        dag = R.Dag(preds, [50.0] * len(preds), [0] * len(preds))
        for mode, ns, wm in [s for s in SCHEDULES if s[0] == R.CAPTURE_ORDER or s[1] >= 2]:
            cmds = R.host_commands(lib, dag, mode, ns, wm, 2)
            on = R.stream_of(cmds)
            sa, sb = {on[k] for k in chains[0]}, {on[k] for k in chains[1]}
            assert len(sa) == 1 and len(sb) == 1 and sa != sb, (length, mode, ns, wm, on)
            R.check(dag, cmds, 2)


def test_filler_beside_a_chain_goes_to_the_last_stream(lib):
    """0 -> 1 -> 2 -> 4 with 3 hanging off 1: flagged as the batched reduction it takes the last stream (the first side
    stream is the high-priority one), unflagged the first free one"""
    preds = [[], [0], [1], [1], [2]]
    for flag, n_sides, want in ((R.FILLER, 2, 2), (0, 2, 1), (R.FILLER, 1, 1), (R.FILLER, 0, 0)):
        dag = R.Dag(preds, [5.0] * 5, [0, 0, 0, flag, 0])
        cmds = R.host_commands(lib, dag, R.CAPTURE_ORDER, n_sides=n_sides)
        on = R.stream_of(cmds)
        assert on[3] == want and all(on[k] == 0 for k in (0, 1, 2, 4)), (flag, n_sides, on)
        R.check(dag, cmds, n_sides)


def test_same_input_same_list_and_counts_as_lic_plan_info_reports_them(lib):
    """info[4] = operations not on `main`, info[5] = cross-stream events (include/lic.h): both can be read off the list
    of a replay on three distinct streams"""
    for gen, seed, dag in _cases(15):
        for mode, ns, wm in SCHEDULES:
            cmds, info = R.host_commands(lib, dag, mode, ns, wm, 2, with_info=True)
            assert R.host_commands(lib, dag, mode, ns, wm, 2) == cmds
            stats = R.check(dag, cmds, 2)
            assert info == {"on_side": stats["on_side"], "events": stats["events"]}, (gen.__name__, seed, mode, ns, wm)
            waited = {c[2] for c in cmds if c[0] == WAIT and c[2] >= EV_FIRST}
            assert waited == {c[2] for c in cmds if c[0] == RECORD and c[2] >= EV_FIRST}   # no event without a waiter
