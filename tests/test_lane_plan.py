"""The ordering of overlapped persistent launches without a GPU: csrc/rt_plan.h lane_plan, the one function that
says which lane and buffer set a launch takes and what it waits for, and lane_advance, the one function that says
what a launch leaves in the context's LaneState for the next. tests/native/lane_plan_dump.cpp runs both: its stateful
mode holds the LaneState across launches exactly as a context does (render<R> in csrc/rt_render.hip calls the same two
functions), so nothing of the bookkeeping is repeated here."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "cpu-ray-tracing-implementation_amd", "csrc")
KEYS = ("overlap", "lane", "set", "sync_prev", "wait_resolve", "record_inputs", "wait_inputs")
STATE = ("n", "inputs_written", "prev_overlapped", "stale0", "stale1")
CALL = dict(knob=1, device_out=1, persist=1, shared_scratch=0, second_set=1)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lane") / "lane_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe,
                    os.path.join(REPO, "tests", "native", "lane_plan_dump.cpp")], check=True)

    def answers(lines):
        out = subprocess.run([exe], input="".join(lines), check=True, capture_output=True, text=True).stdout
        return [[int(v) for v in row.split()] for row in out.splitlines()]

    def run(**q):
        d = dict(CALL, n=0, inputs_written=0, prev_overlapped=0, stale0=0, stale1=0, pending=0, caller=0, prev=0)
        assert set(q) <= set(d)
        d.update(q)
        return dict(zip(KEYS, answers(["L " + " ".join(str(int(v)) for v in d.values()) + "\n"])[0]))
    run.answers = answers
    return run


class Ctx:
    """A context's launches, one stateful line each. The lanes' state lives in the dump program (all lines so far are
    replayed into a fresh process per launch); this keeps only what is outside it: the mirror of pending / pend_stream."""

    def __init__(self, ask):
        self.ask, self.lines, self.reported = ask, [], dict.fromkeys(STATE, 0)
        self.pending, self.prev = 0, 0

    @property
    def n(self):
        return self.reported["n"]

    def launch(self, caller=0, write=False, **kw):
        assert set(kw) <= set(CALL)
        d = dict(CALL, **kw, pending=self.pending, caller=caller, prev=self.prev, write=write)
        self.lines.append("S " + " ".join(str(int(v)) for v in d.values()) + "\n")
        row = self.ask.answers(self.lines)[-1]
        self.reported = dict(zip(STATE, row[len(KEYS):]))
        self.pending, self.prev = 1, caller
        return dict(zip(KEYS, row))


def test_first_two_launches_and_steady_state(ask):
    c = Ctx(ask)
    a = c.launch(write=True)  # the first render queues the scene, the camera and the pixel map on its stream
    assert a == dict(overlap=1, lane=0, set=0, sync_prev=0, wait_resolve=0, record_inputs=1, wait_inputs=1)
    b = c.launch()
    # no earlier user of set 1; lane 1 is not behind the first launch's inputs event yet
    assert b == dict(overlap=1, lane=1, set=1, sync_prev=0, wait_resolve=0, record_inputs=0, wait_inputs=1)
    for n in range(2, 9):  # steady state: nothing on the caller's stream but the resolve of launch n - 2
        p = c.launch()
        assert p == dict(overlap=1, lane=n & 1, set=n & 1, sync_prev=0, wait_resolve=1, record_inputs=0,
                         wait_inputs=0), n


def test_an_input_write_is_waited_for_by_both_lanes_once(ask):
    c = Ctx(ask)
    for _ in range(4):
        c.launch()
    p = c.launch(write=True)
    assert (p["lane"], p["wait_resolve"], p["record_inputs"], p["wait_inputs"]) == (0, 1, 1, 1)
    p = c.launch()  # the other lane reads the same inputs
    assert (p["lane"], p["wait_resolve"], p["record_inputs"], p["wait_inputs"]) == (1, 1, 0, 1)
    for _ in range(3):
        p = c.launch()
        assert (p["record_inputs"], p["wait_inputs"]) == (0, 0)
    # two writes in a row: the second event makes the first lane stale again
    c.launch(write=True)
    p = c.launch(write=True)
    assert (p["record_inputs"], p["wait_inputs"]) == (1, 1)
    p = c.launch()
    assert (p["record_inputs"], p["wait_inputs"]) == (0, 1)
    p = c.launch()
    assert (p["record_inputs"], p["wait_inputs"]) == (0, 0)


def test_a_stream_change_waits_on_the_host(ask):
    c = Ctx(ask)
    for _ in range(3):
        assert c.launch(caller=7)["sync_prev"] == 0
    p = c.launch(caller=9)  # the outstanding work is on stream 7: the host waits first; lanes and sets go on in turn
    assert (p["overlap"], p["lane"], p["set"], p["sync_prev"], p["wait_resolve"]) == (1, 1, 1, 1, 1)
    p = c.launch(caller=9)
    assert (p["sync_prev"], p["wait_resolve"]) == (0, 1)
    assert ask(pending=0, caller=3, prev=7)["sync_prev"] == 0  # nothing outstanding: no wait


@pytest.mark.parametrize("off", [dict(knob=0), dict(second_set=0), dict(device_out=0), dict(persist=0),
                                 dict(shared_scratch=1)],
                         ids=["knob_off", "allocation_fallback", "host_output", "wavefront", "wide_spill"])
def test_serial_cases(ask, off):
    c = Ctx(ask)
    for n in range(4):
        p = c.launch(write=n == 0, **off)  # the chain on the caller's stream: set 0, no event
        assert p == dict(overlap=0, lane=0, set=0, sync_prev=0, wait_resolve=0, record_inputs=0, wait_inputs=0)
    assert c.n == 0
    assert c.launch(caller=5, **off)["sync_prev"] == 1  # the wait for another stream's work is the serial chain's too


def test_a_serial_launch_between_overlapped_ones_is_waited_for(ask):
    c = Ctx(ask)
    for _ in range(3):
        c.launch()
    assert c.launch(knob=0)["overlap"] == 0  # wrote set 0 on the caller's stream
    p = c.launch()
    assert (p["overlap"], p["lane"], p["record_inputs"], p["wait_inputs"], p["wait_resolve"]) == (1, 1, 1, 1, 1)
    p = c.launch()
    assert (p["lane"], p["record_inputs"], p["wait_inputs"]) == (0, 0, 1)


def test_serial_launches_after_overlapped_ones_leave_the_lanes_as_they_were(ask):
    # read off render<R>: a serial launch clears prev_overlapped and inputs_written (it runs on the stream the inputs
    # were queued on) and touches neither the lanes' launch count nor their staleness
    c = Ctx(ask)
    for _ in range(4):
        c.launch()
    c.launch(write=True)  # lane 0 records the inputs event and waits for it: lane 1 is stale
    assert c.reported == dict(n=5, inputs_written=0, prev_overlapped=1, stale0=0, stale1=1)
    assert c.launch(knob=0)["overlap"] == 0
    lone = dict(n=5, inputs_written=0, prev_overlapped=0, stale0=0, stale1=1)
    assert c.reported == lone
    assert c.launch(knob=0, write=True)["overlap"] == 0  # a write, and another serial launch
    assert c.reported == lone
    # ... and the lanes go on from there: the next overlapped launch is the sixth, behind a new inputs event
    p = c.launch()
    assert p == dict(overlap=1, lane=1, set=1, sync_prev=0, wait_resolve=1, record_inputs=1, wait_inputs=1)
    assert c.reported == dict(n=6, inputs_written=0, prev_overlapped=1, stale0=1, stale1=0)
