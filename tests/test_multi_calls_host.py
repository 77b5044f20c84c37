"""The multi-GPU layer's call order without a GPU ("Host code: one copy of each rule"): csrc/rt_multi.cpp on top of a recording runtime
(tests/tools/multi_shim.cpp) runs the scripts of tests/tools/multi_calls_main.cpp -- every transport, layout and entry point, and the injected failures --
and what it enqueues, on which stream and current device, in which order, with which offsets and sizes, is held line for line to the logs under
tests/golden/multi_calls/.  Those were recorded from the file as it was BEFORE its rules were brought to one copy each and are never regenerated from
the file under test (tests/tools/multi_calls_lab.py --record takes the older file).  The runtime's ledger also checks every release.  The same program
built with -fsanitize=address,undefined is a command of its own, `python tests/tools/multi_calls_lab.py --sanitize`: a CPU-only check, not part of the suite."""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import multi_calls_lab as L  # noqa: E402

RT_ERR_DEVICE = -3
STEADY = [f"steady/{name}" for name in (
    "direct_dense_rgba32f", "parts_dense_rgba32f", "copy_dense_rgba32f", "self_dense_rgba32f", "rccl_dense_rgba32f", "ten_dense_rgba32f", "rccl_dense_rgba8",
    "copy_bandwise_rgba32f", "copy_sparse_rgba32f", "self_bandwise_rgba32f", "self_sparse_rgba32f", "rccl_bandwise_rgba32f", "rccl_sparse_rgba32f")]
FAILURES = [f"fail/{name}" for name in ("render_third_context", "send_second_frame", "send_second_gbuffer", "group_end", "debug_multi_fail_copy")]
CREATE = [f"create/{fn}" for fn in ("hipMalloc", "hipEventCreateWithFlags", "rt_create", "hipStreamCreateWithFlags", "hipEventCreate")] + \
         [f"create_sparse/{fn}" for fn in ("hipMalloc", "hipHostMalloc")] + [f"setup/{fn}" for fn in ("hipMalloc", "hipEventCreateWithFlags", "hipHostMalloc")]


def test_the_program_runs_every_script_and_every_ledger_is_clean():
    logs = L.logs()
    assert logs["exit status"] == ["0"], logs["exit status"]   # (its exit status counts the ledgers' complaints; anything on stderr follows it)
    assert sorted(n for n in logs if n != "exit status") == sorted(STEADY + FAILURES + CREATE)
    assert L.fixture_names() == sorted(STEADY + FAILURES + CREATE)
    for name in STEADY + FAILURES + CREATE:
        verdicts = [l for l in logs[name] if l.startswith("ledger:")]
        assert verdicts and set(verdicts) == {"ledger: clean"}, (name, verdicts)
    for name in STEADY:
        assert sum(l.startswith("> ") for l in logs[name]) == 14 and not any(l.startswith("< -") for l in logs[name]), name


@pytest.mark.parametrize("name", STEADY + FAILURES)
def test_log_is_the_recorded_one_line_for_line(name):
    got, want = L.pinned(L.logs()[name]), L.fixture(name)
    at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, f"{name}, line {at + 1}: {got[at] if at < len(got) else '(end)'!r}, recorded {want[at] if at < len(want) else '(end)'!r}"
    assert len(want) > 10


def test_the_recorded_layouts_take_the_branches_they_are_there_for():
    """The fixtures themselves: the rccl layout really issues RCCL pairs between three devices (a trace of a fake runtime -- no hardware has run that
    branch), the rehearsal copies, `ten` has contexts without rows, the sparse headers make the messages differ in size."""
    rccl = L.fixture("steady/rccl_dense_rgba32f")
    assert {re.search(r"dev=(\d)", l).group(1) for l in rccl if l.startswith("rt_render ")} == {"0", "1", "2"}
    assert sum(l.startswith("ncclSend ") for l in rccl) == sum(l.startswith("ncclRecv ") for l in rccl) > 0
    assert any(l.startswith("hipMemcpyPeerAsync ") for l in rccl)
    copy = L.fixture("steady/copy_dense_rgba32f")
    assert not any(l.startswith("nccl") for l in copy) and any(" D2D" in l for l in copy)
    assert any(l.startswith("hipMemcpy2DAsync ") for l in L.fixture("steady/rccl_bandwise_rgba32f"))
    ten = L.fixture("steady/ten_dense_rgba32f")
    assert sum(l.startswith("rt_render ") for l in ten) == 5 * 10
    assert sum(l.startswith("rt_render_gbuffer ") for l in ten) == 2 * 8   # contexts 8 and 9 own no row: skipped for planes only
    sparse = L.fixture("steady/rccl_sparse_rgba32f")
    assert len({re.search(r"bytes=(\d+)", l).group(1) for l in sparse if l.startswith("ncclSend ")}) > 2


@pytest.mark.parametrize("name", ["fail/send_second_frame", "fail/send_second_gbuffer", "fail/group_end"])
def test_a_failure_inside_a_group_still_closes_it(name):
    log = L.logs()[name]
    failed = next(i for i, l in enumerate(log) if l.startswith(f"< {RT_ERR_DEVICE} "))
    starts = [i for i, l in enumerate(log[:failed]) if l.startswith("ncclGroupStart ")]
    ends = [i for i, l in enumerate(log[:failed]) if l.startswith("ncclGroupEnd ")]
    assert len(starts) == len(ends) == 1 and starts[0] < ends[0] == failed - 1, log[:failed + 1]


@pytest.mark.parametrize("name", FAILURES)
def test_a_failed_object_refuses_the_next_call_and_still_releases_everything(name):
    log = L.logs()[name]
    codes = [l for l in log if l.startswith("< ")]
    assert codes[0].startswith(f"< {RT_ERR_DEVICE} ") and codes[-1] == "< 0"   # the failed call ... rt_multi_destroy
    assert codes[1].startswith(f'< {RT_ERR_DEVICE} "rt_multi_set_scene_status: an earlier call on this object failed') and "destroy it and create a new one" in codes[1]
    frame = [l for l in log if l.startswith("~ ")]
    assert len(frame) == 1 and frame[0].startswith(f'~ rt_render_multi: {RT_ERR_DEVICE} "rt_render_multi: ') and "destroy it and create a new one" in frame[0]
    assert log[-1] == "ledger: clean"


@pytest.mark.parametrize("name", CREATE)
def test_a_partial_object_is_released_and_the_message_names_the_failed_call(name):
    """The k-th call of one function fails, for every k up to success, in rt_create_multi (create/, create_sparse/) and in the first scene update, G-buffer
    and extents call, which set their state up (setup/).  Every k: RT_ERR_DEVICE (rt_create: the context's own code, which is that one here) and an empty
    ledger.  Neither the order in which an object is put together nor its teardown is pinned, so the error texts are held to the recorded ones as a sorted
    list: each names the HIP call that failed, as it did before the members owned their handles."""
    log = [l for l in L.logs()[name] if l.startswith("k=")]
    assert [l.split(":")[0] for l in log] == [f"k={k}" for k in range(1, len(log) + 1)]
    assert "created after" in log[-1] or log[-1].endswith(": all set up"), log[-1]
    want = L.fixture(name)
    assert L.texts(L.logs()[name]) == want and len(want) >= (6 if name in ("create/hipMalloc", "create/rt_create") else 12 if name == "create/hipEventCreateWithFlags" else 1)
    fn = name.split("/")[1]
    for line in log[:-1]:
        assert f" {RT_ERR_DEVICE} \"" in line and line.endswith('injected failure"') and (fn + "(" in line or fn == "rt_create"), line


def test_the_file_keeps_no_second_copy_of_a_rule():
    """A loose guard on the source text next to the logs, which are the check: the member groups, the second guard and the hand-written teardown stay gone."""
    src = re.sub(r"//[^\n]*", "", open(L.PRODUCT).read())
    assert src.count("ncclGroupEnd(") == 1 and src.count("hipEventElapsedTime(") == 1 and "FailGuard" not in src
    assert not re.search(r"\b[gx]_(local|gathered|ev_\w+|ready|parts|merged)\b", re.sub(r'"[^"\n]*"', '""', src))   # (the error texts keep the old names)
    destroy = src[src.index('extern "C" int rt_multi_destroy'):src.index("static int create_impl")]
    assert "hipFree" not in destroy and "hipEventDestroy" not in destroy and "delete m;" in destroy
