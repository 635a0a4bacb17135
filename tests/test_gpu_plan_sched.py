"""The schedules of real launch plans, edge by edge: the DAG (lic_plan_dag) and the command list a replay issues
(lic_plan_commands) are read back from plans of a captured diamond, of the training step and of the forward pass, and
held to the vector-clock model of tests/plan_sched_ref.py -- before and after lic_plan_tune, with 0, 1 and 2 side
streams.  The candidates lic_plan_tune measured and dropped are rebuilt from the read-back DAG and its measured times by
lic_plan_sched_host and checked as well.  test_gpu_plan.py compares results with the eager step, which shows a missing
wait only when the race is lost; this file needs no race."""
import ctypes as C

import pytest
import torch

import plan_sched_ref as R

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _info(lib, plan):
    from neural_image_compression_amd import _lib as L
    info = (C.c_int64 * 7)()
    L.check(lib.lic_plan_info(plan, info), "lic_plan_info")
    return dict(zip(("nodes", "kernels", "memsets", "memcpys", "on_side_stream", "events", "tuned"), list(info)))


def _check_plan(lib, plan, dag, ns):
    """the schedule in use: valid with 0, 1 and 2 side streams, lic_plan_info agrees with the list, and it is one of the
    schedules lic_plan_sched_host makes of the read-back DAG (capture order, or a list schedule when a tuned one is kept)"""
    info = _info(lib, plan)
    assert info["nodes"] == dag.n
    lists = {n_sides: R.plan_commands(lib, plan, n_sides) for n_sides in (0, 1, 2)}
    for n_sides, cmds in lists.items():
        stats = R.check(dag, cmds, n_sides)
        print(f"  {n_sides} side streams: {stats}")
    stats = R.check(dag, lists[2], 2)
    assert (info["on_side_stream"], info["events"]) == (stats["on_side"], stats["events"]), (info, stats)
    for n_sides in (0, 1, 2):
        if info["tuned"]:
            made = [R.host_commands(lib, dag, R.LIST_SCHEDULE, ns, wm, n_sides) for wm in R.WIDE_MIN_US]
        else:
            made = [R.host_commands(lib, dag, R.CAPTURE_ORDER, n_sides=n_sides)]
        assert lists[n_sides] in made, (n_sides, info)
    return info


def _check_candidates(lib, dag, ns):
    """what lic_plan_tune replayed six times each, kept or not: the list schedules of the DAG with its measured times"""
    assert min(dag.us) >= 0.5 and max(dag.us) < 1e6, (min(dag.us), max(dag.us))
    for wm in R.WIDE_MIN_US:
        for n_sides in (0, 1, 2):
            stats = R.check(dag, R.host_commands(lib, dag, R.LIST_SCHEDULE, ns, wm, n_sides), n_sides)
        print(f"  candidate wide_min_us {wm:g}: {stats}")


def test_diamond_capture_reads_back_as_captured_and_every_schedule_is_valid():
    """The capture of test_gpu_plan.py's diamond.  Under capture every launch depends on the one before it on its stream,
    and wait_stream adds an edge, not a node.  Main stream: x * 2 (1 kernel, nothing before it), 20 x (mul, add) = 40;
    there the side stream forks off: a + 1 and 10 x (mul, add) = 21; main goes on with a * 3, the fill of zeros_like and
    c + z = 3; main waits for the side stream and adds b + c = 1.  66 operations; exactly one without a predecessor (x * 2),
    exactly one with two successors (the last of `a`: a + 1 on the side, a * 3 on main), exactly one with two
    predecessors (b + c: after c + z and after the last of `b`), and nothing with more than two of either."""
    _need_gpu()
    from neural_image_compression_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    x = torch.arange(1 << 20, device=dev, dtype=torch.float32)
    side_cap = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        main = torch.cuda.current_stream()
        a = x * 2.0
        for _ in range(20):
            a = a * 1.0001 + 1.0
        side_cap.wait_stream(main)
        with torch.cuda.stream(side_cap):
            b = a + 1.0
            for _ in range(10):
                b = b * 0.5 + 3.0
        c = a * 3.0
        z = torch.zeros_like(c)
        c = c + z
        main.wait_stream(side_cap)
        e = b + c
    plan = C.c_void_p()
    L.check(lib.lic_plan_create(C.c_void_p(g.raw_cuda_graph()), C.byref(plan)), "lic_plan_create")
    try:
        dag, kinds = R.plan_dag(lib, plan)
        n_succ = [0] * dag.n
        for q, _ in dag.edges():
            n_succ[q] += 1
        n_pred = [len(p) for p in dag.preds]
        print(f"diamond: {dag.n} operations, {len(dag.edges())} edges")
        assert dag.n == 66 and set(kinds) <= {0, 1} and kinds.count(1) <= 1
        assert n_pred.count(0) == 1 and n_pred.count(2) == 1 and max(n_pred) == 2
        assert n_succ.count(2) == 1 and max(n_succ) == 2 and n_succ.count(0) == 1
        assert n_pred[0] == 0 and n_pred[-1] == 2 and n_succ[-1] == 0 and n_succ.index(2) == 40
        assert dag.us == [0.0] * dag.n and not any(f & R.FILLER for f in dag.flags)
        assert all(f & R.WIDE for k, f in enumerate(dag.flags) if kinds[k] == 0)   # (1 M elements: thousands of workgroups)
        info = _check_plan(lib, plan, dag, 3)
        # (at the fork the side stream's 21 launches + b + c are the longer way to go: they stay, and a * 3, the fill and c + z move)
        assert not info["tuned"] and info["on_side_stream"] == 3 and info["events"] == 2
        s_main, s_side, s_side2 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
        sides = (C.c_void_p * 2)(s_side.cuda_stream, s_side2.cuda_stream)
        r = (C.c_double * 4)()
        L.check(lib.lic_plan_tune(plan, C.c_void_p(s_main.cuda_stream), sides, 2, r), "lic_plan_tune")
        torch.cuda.synchronize()
        timed, _ = R.plan_dag(lib, plan)
        assert timed.preds == dag.preds and timed.flags == dag.flags
        info = _check_plan(lib, plan, timed, 3)
        assert info["tuned"] == int(r[3])
        _check_candidates(lib, timed, 3)
        # the buffers' sizes are checked
        sizes, n_cmds = (C.c_int64 * 2)(), C.c_int64()
        ptr, idx = (C.c_int32 * 67)(), (C.c_int32 * 66)()
        kind, flags, us = (C.c_int32 * 66)(), (C.c_int32 * 66)(), (C.c_double * 66)()
        assert lib.lic_plan_dag(plan, 65, 66, sizes, ptr, idx, kind, flags, us) == -4 and list(sizes) == [66, 66]
        assert lib.lic_plan_dag(plan, 66, 65, sizes, ptr, idx, kind, flags, us) == -4
        assert lib.lic_plan_dag(plan, 66, 66, sizes, ptr, idx, kind, flags, None) == -1
        assert lib.lic_plan_dag(plan, 66, 66, None, ptr, idx, kind, flags, us) == -1
        assert lib.lic_plan_commands(plan, 3, 0, C.byref(n_cmds), None) == -1
        assert lib.lic_plan_commands(plan, 1, 0, C.byref(n_cmds), None) == 0 and n_cmds.value > 66
        small = (C.c_int32 * (3 * 66))()
        assert lib.lic_plan_commands(plan, 1, 66, C.byref(n_cmds), small) == -4
        assert lib.lic_plan_commands(plan, 1, 66, C.byref(n_cmds), None) == -1
    finally:
        lib.lic_plan_destroy(plan)
    del e


def _as_dag(d):
    return R.Dag(d["preds"], d["us"], [(R.WIDE if w else 0) | (R.FILLER if f else 0) for w, f in zip(d["wide"], d["filler"])])


@pytest.mark.parametrize("precision,M,K,tune", [("bf16", 128, 3, False), ("bf16", 128, 3, True),
                                                ("fp32", 64, 1, False), ("fp32", 64, 1, True)])
def test_step_plan_schedules_are_valid(precision, M, K, tune):
    """the training step's plan (B=4, 128 x 128): the schedule in use with 0, 1 and 2 side streams, and after a tune the
    three candidates it measured"""
    _need_gpu()
    import neural_image_compression_amd as nic
    from neural_image_compression_amd.plan import StepPlan
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    m = nic.JointAutoregressiveHierarchical(M, K).to(dev)
    if precision == "bf16":
        m.set_precision("bf16")
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.rand(4, 3, 128, 128, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    plan = StepPlan(m, nic.rd_loss, 0.01, x, tune=tune)
    try:
        d = plan.dag()
        dag = _as_dag(d)
        print(f"{precision} step: {dag.n} operations, {len(dag.edges())} edges, {sum(d['filler'])} fillers, "
              f"{sum(d['wide'])} wide, tuning {plan.tuning}")
        assert dag.n == plan.info["nodes"] and d["kind"].count("kernel") == plan.info["kernels"] > 100
        assert [tuple(c) for c in plan.commands(2)] == R.plan_commands(plan._lib, plan._plan, 2)
        # the bf16 step forks its batched reductions off beside the chains; the fp32 step reduces right away
        assert (sum(d["filler"]) > 0) == (precision == "bf16")
        assert all(k == "kernel" for k, f in zip(d["kind"], d["filler"]) if f)
        info = _check_plan(plan._lib, plan._plan, dag, 3)
        assert info == plan.info and info["on_side_stream"] > 10
        if tune:
            assert info["tuned"] == int(plan.tuning["tuned_kept"])
            _check_candidates(plan._lib, dag, 3)
        else:
            assert d["us"] == [0.0] * dag.n
            if precision == "bf16":   # capture order sends the batched reduction forked off beside a chain to the last stream
                on = R.stream_of(plan.commands(2))
                print(f"  fillers on streams {sorted(on[k] for k, f in enumerate(d['filler']) if f)}")
                assert 2 in {on[k] for k, f in enumerate(d["filler"]) if f}
    finally:
        plan.close()


def test_forward_plan_schedules_are_valid():
    """plan.ForwardPlan (two streams): capture order, then tuned on its own two streams"""
    _need_gpu()
    import neural_image_compression_amd as nic
    from neural_image_compression_amd import _lib as L
    from neural_image_compression_amd.functional import _stream
    from neural_image_compression_amd.plan import ForwardPlan
    dev = torch.device("cuda:0")
    torch.manual_seed(8)
    m = nic.JointAutoregressiveHierarchical(128, 3).to(dev)
    m.set_precision("bf16")
    x = torch.rand(2, 3, 128, 128, device=dev).contiguous(memory_format=torch.channels_last)
    fp = ForwardPlan(m, x, training=True)
    try:
        dag = _as_dag(fp.dag())
        print(f"forward: {dag.n} operations, {len(dag.edges())} edges")
        assert dag.n == fp.info["nodes"] and fp.info["kernels"] >= 15
        assert _check_plan(fp._lib, fp._plan, dag, 2) == fp.info
        r = (C.c_double * 4)()
        L.check(fp._lib.lic_plan_tune(fp._plan, _stream(), fp._sides, 1, r), "lic_plan_tune")
        torch.cuda.synchronize()
        timed = _as_dag(fp.dag())
        assert timed.preds == dag.preds
        assert _check_plan(fp._lib, fp._plan, timed, 2)["tuned"] == int(r[3])
        _check_candidates(fp._lib, timed, 2)
    finally:
        fp.close()
