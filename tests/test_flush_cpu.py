"""The capacities behind the flush loops of the scan's record buffers (lime_amd/csrc/lime_kernels.hip: flush_direct, put_rec,
score_small3), restated from the library's exported constants.  Every `while (waiting + batch > capacity) flush` loop of a scorer ends
after one flush because a flush that makes room leaves at most room_left records and the largest batch one call adds fits behind them;
the kernels static_assert the same sums.  The flush at a window's top may leave more (top_left), which no such loop may rely on."""
import ctypes as C
import os
import re

from lime_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Queue(C.Structure):
    _fields_ = [("cap", C.c_uint32), ("cap_short", C.c_uint32), ("room_left", C.c_uint32), ("top_left", C.c_uint32)]


def _queue():
    q = Queue()
    _lib.load().lime_scan_queue(C.byref(q))
    return q


def test_every_batch_fits_behind_what_a_room_flush_leaves():
    q = _queue()
    assert (q.cap, q.cap_short) == (286, 160)
    assert q.room_left == 15                                              # whole lines of 16 records leave
    assert q.room_left + 64 <= q.cap_short <= q.cap                       # put_rec: one record per lane
    assert q.room_left + 256 <= q.cap                                     # score_small3, EBWT=0: 64 clusters x 4 pairs at once
    assert 256 + 2 * 15 <= q.cap                                          # ... and its `halves` rule (pairs + 2 x 15 > cap) never splits them
    assert q.room_left + 128 <= q.cap_short                               # score_small3, EBWT=1: a half is 64 clusters x 2 pair slots
    assert 128 + 2 * 15 <= q.cap_short                                    # ... and whatever the rule does not split fits too


def test_what_the_window_top_leaves_is_not_what_the_loops_rely_on():
    """with batches of 64 at the window's top up to 63 records wait: a half batch of the short queue would NOT fit behind them, so the
    scorers' loops may only ever call the room flush -- and flush_direct takes its form from a compile-time argument at every call site"""
    q = _queue()
    assert q.top_left == 63 and q.top_left + 128 > q.cap_short
    src = open(os.path.join(ROOT, "lime_amd", "csrc", "lime_kernels.hip")).read()
    calls = re.findall(r"flush_direct\(\w+, a, (FLUSH_\w+)", src)
    assert sorted(set(calls)) == ["FLUSH_FINAL", "FLUSH_ROOM", "FLUSH_TOP"] and calls.count("FLUSH_TOP") == 1 and calls.count("FLUSH_FINAL") == 1
    for m in re.finditer(r"while \([^;]*\) flush_direct\(\w+, a, (FLUSH_\w+)", src):
        assert m.group(1) == "FLUSH_ROOM", m.group(0)
