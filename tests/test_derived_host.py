"""`video2music_amd/_derived.py` on the CPU: the one keyed cache every table derived from the parameters goes through.  CPU tensors, the
wait (`_derived.ready`) replaced by a recorder: hit and miss, publish after the wait, one build per raced miss, the three modes
(`wait=False`, `keep=False`, `into=` / `publish`), one entry per role, nesting; and a search of the package for a second spelling of
the key or the lock."""
import pathlib
import re
import threading

import pytest
import torch

from tests import helpers_weight_follow as W
from tests.test_weight_follow_host import TOY_THRESHOLD, toy_case
from video2music_amd import _derived
from video2music_amd._derived import Derived

GUARD_S = 10.0          # a thread that has not finished by then is stuck: the test fails, it does not hang


@pytest.fixture
def waits(monkeypatch):
    """The calls of `_derived.ready`, one list of sources each."""
    calls = []
    monkeypatch.setattr(_derived, "ready", lambda srcs: calls.append(list(srcs)))
    return calls


class Counted:
    """build() -> a fresh tensor derived from `srcs`; counts its calls."""

    def __init__(self, *srcs):
        self.srcs, self.n = srcs, 0

    def __call__(self):
        self.n += 1
        return torch.cat([t.detach().reshape(-1) for t in self.srcs]) * 2.0


def joined(*threads):
    for t in threads:
        t.start()
    for t in threads:
        t.join(GUARD_S)
    assert not any(t.is_alive() for t in threads), f"a thread is still running after {GUARD_S} s"


def test_hit_returns_the_stored_object(waits):
    w, d = torch.ones(3), Derived()
    build = Counted(w)
    first = d.get("r", (w,), build)
    assert d.get("r", (w,), build) is first and build.n == 1 and len(waits) == 1 and waits[0][0] is w
    assert torch.equal(first, torch.full((3,), 2.0)) and d.roles() == ["r"]


@pytest.mark.parametrize("kind", [k for k in W.KINDS if k != "v_cpu_roundtrip"])
def test_every_write_torch_can_see_is_a_miss(waits, kind):
    case, path = toy_case("correct")                 # the toy whose copy goes through Derived.get
    for keys in (["w"], ["b"], None):
        W.follows(case, case.model("cpu"), path, W.KINDS[kind], keys=keys, threshold=TOY_THRESHOLD, device="cpu")
    assert waits, "the toy did not go through Derived.get"


def test_the_role_is_not_visible_inside_the_wait(monkeypatch):
    w, d, seen = torch.ones(3), Derived(), []
    monkeypatch.setattr(_derived, "ready", lambda srcs: seen.append(d.roles()))
    d.get("r", (w,), Counted(w))
    assert seen == [[]] and d.roles() == ["r"], f"roles inside the wait: {seen}"


def test_a_second_thread_blocks_until_the_wait_is_over(monkeypatch):
    w, d = torch.ones(3), Derived()
    build, reader_started, reader_done, inside, got = Counted(w), threading.Event(), threading.Event(), [], []

    def reader():
        reader_started.set()
        got.append(d.get("r", (w,), build))
        reader_done.set()

    t = threading.Thread(target=reader)

    def ready(srcs):
        t.start()
        assert reader_started.wait(GUARD_S)
        inside.append(reader_done.wait(0.2))         # (the one short wait of the file: a blocked reader lets it run out)

    monkeypatch.setattr(_derived, "ready", ready)
    first = d.get("r", (w,), build)
    t.join(GUARD_S)
    assert not t.is_alive(), f"the reader is still blocked {GUARD_S} s after the entry was published"
    assert inside == [False], "a second thread's get returned while the builder was still waiting"
    assert got[0] is first and build.n == 1


def test_a_raced_miss_builds_once(waits):
    w, d = torch.ones(3), Derived()
    barrier, got, n = threading.Barrier(2), [], [0]

    def build():
        n[0] += 1
        return w * 2.0

    def worker():
        barrier.wait(GUARD_S)                        # both threads have missed nothing yet; they reach get together
        got.append(d.get("r", (w,), build))

    joined(threading.Thread(target=worker), threading.Thread(target=worker))
    assert n[0] == 1 and len(got) == 2 and got[0] is got[1] and len(waits) == 1


def test_a_raced_miss_whose_build_waits_on_the_other_thread_builds_once(waits):
    """The build itself waits until the second thread has entered get: that one must block on the lock, then take the first one's entry."""
    w, d = torch.ones(3), Derived()
    second_in, got, n = threading.Event(), {}, [0]

    def build():
        n[0] += 1
        assert second_in.wait(GUARD_S)
        return w * 2.0

    def first():
        got[1] = d.get("r", (w,), build)

    def second():
        second_in.set()
        got[2] = d.get("r", (w,), build)

    t1 = threading.Thread(target=first)
    t1.start()
    joined(threading.Thread(target=second))
    t1.join(GUARD_S)
    assert not t1.is_alive() and n[0] == 1 and got[1] is got[2] and len(waits) == 1


def test_keep_false_builds_for_this_call_alone(waits):
    w, d = torch.ones(3), Derived()
    build = Counted(w)
    a, b = d.get("r", (w,), build, keep=False), d.get("r", (w,), build, keep=False)
    assert a is not b and build.n == 2 and waits == [] and d.roles() == []
    stored = d.get("r", (w,), build)
    assert d.get("r", (w,), build, keep=False) is stored and build.n == 3 and len(waits) == 1 and d.roles() == ["r"]
    w.add_(1.0)                                      # a miss on a stored entry: built for the call, the entry stays as it is
    assert d.get("r", (w,), build, keep=False) is not stored and d.entries()["r"][1] is stored and len(waits) == 1


def test_wait_false_stores_without_the_wait(waits):
    w, d = torch.ones(3), Derived()
    build = Counted(w)
    first = d.get("r", (w,), build, wait=False)
    assert d.get("r", (w,), build, wait=False) is first and d.get("r", (w,), build) is first
    assert build.n == 1 and waits == [] and d.roles() == ["r"]


def test_into_and_publish(waits):
    ws, d, pending = [torch.full((2,), float(i)) for i in range(4)], Derived(), {}
    builds = [Counted(w) for w in ws]
    vals = [d.get(("t", i), (w,), b, into=pending) for i, (w, b) in enumerate(zip(ws, builds))]
    assert [b.n for b in builds] == [1] * 4 and waits == [] and d.roles() == []
    assert d.get(("t", 0), (ws[0],), builds[0], into=pending) is vals[0] and builds[0].n == 1      # the pending entry, not a rebuild
    other = Counted(ws[1])                           # a reader outside this table build sees nothing of it yet: it builds its own
    assert d.get(("t", 1), (ws[1],), other, keep=False) is not vals[1] and other.n == 1 and d.roles() == []
    d.publish(pending)
    assert len(waits) == 1 and {id(t) for t in waits[0]} == {id(w) for w in ws}
    assert sorted(d.roles()) == [("t", i) for i in range(4)]
    assert all(d.get(("t", i), (w,), b) is v for i, (w, b, v) in enumerate(zip(ws, builds, vals)))
    assert [b.n for b in builds] == [1] * 4 and len(waits) == 1
    again = {}                                       # the next table build finds every role: nothing pending, nothing to publish
    assert d.get(("t", 2), (ws[2],), builds[2], into=again) is vals[2] and again == {}
    d.publish(again)
    assert len(waits) == 1


def test_publish_of_nothing_calls_nothing(waits):
    d = Derived()
    d.publish({})
    assert waits == [] and d.roles() == []


def test_one_entry_per_role(waits):
    """Storage X, then Y, then X again with a moved version (the EMA swap): every step rebuilds, and one entry stays."""
    p, d = torch.nn.Parameter(torch.zeros(3)), Derived()
    x, y = torch.ones(3), torch.full((3,), 5.0)
    build = Counted(p)
    p.data = x
    vx = d.get("r", (p,), build)
    p.data = y
    vy = d.get("r", (p,), build)
    x.mul_(3.0)                                      # through the alias: no counter of p moves while y is attached
    p.data = x
    vx2 = d.get("r", (p,), build)
    assert build.n == 3 and torch.equal(vx, torch.full((3,), 2.0)) and torch.equal(vy, torch.full((3,), 10.0))
    assert torch.equal(vx2, torch.full((3,), 6.0)) and d.roles() == ["r"] and d.entries()["r"][1] is vx2
    d.drop()
    assert d.roles() == []
    assert d.get("r", (p,), build) is not vx2 and build.n == 4      # the same signature, dropped: rebuilt all the same


def test_nested_get_inside_a_build(waits):
    w, inner, outer, got = torch.ones(3), Derived(), Derived(), []

    def build_outer():
        return inner.get("in", (w,), lambda: w * 2.0) + outer.get("side", (w,), lambda: w * 3.0)

    joined(threading.Thread(target=lambda: got.append(outer.get("out", (w,), build_outer))))
    assert torch.equal(got[0], torch.full((3,), 5.0)) and inner.roles() == ["in"] and sorted(outer.roles()) == ["out", "side"]
    assert len(waits) == 3


def test_ready_leaves_cpu_tensors_alone():
    _derived.ready([torch.ones(2)])                  # (no device to synchronise: must not reach for one)


def test_one_spelling_of_the_key_and_the_lock():
    """The (storage pointer, version) pair and the lock exist in `_derived.py` alone: a cache that spells its own is a copy of the
    protocol, with its bugs available again.  (`self._version` of video_regression.py is the Mamba gate's version, another thing.)"""
    root = pathlib.Path(_derived.__file__).parent
    files = sorted(root.rglob("*.py"))
    assert len(files) > 20
    for f in files:
        if f.name == "_derived.py" and f.parent == root:
            continue
        text = f.read_text()
        versions = [m.group(0) for m in re.finditer(r"\b(\w+)\._version\b", text) if m.group(1) != "self"]
        assert not versions, f"{f.relative_to(root)}: {versions}: take the key from _derived.signature"
        assert "DERIVED_LOCK" not in text, f"{f.relative_to(root)} names DERIVED_LOCK: go through _derived.Derived"
    own = (root / "_derived.py").read_text()
    assert "._version" in own and "DERIVED_LOCK" in own
