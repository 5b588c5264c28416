"""graphed.GraphCache, the bucket cache behind StepCache and both paths of autograph.AutoGraph, with fake steps: a budget
of graphs (not keys), least-recently-used eviction where a hit refreshes the key, the first step that takes the batch, the
counters and the first-visit bookkeeping."""
import pytest


class _Step:
    def __init__(self, name, fits=True):
        self.name, self.fits, self.loads = name, fits, 0

    def load(self):
        self.loads += 1
        if not self.fits:
            raise ValueError("does not fit")


def _cache(max_graphs):
    from mesm_amd.graphed import GraphCache
    return GraphCache(max_graphs)


def _load(s):
    s.load()


def test_the_budget_counts_graphs_not_keys():
    c = _cache(3)
    c.add("a", lambda: _Step("a0"))
    c.add("a", lambda: _Step("a1"))
    c.add("b", lambda: _Step("b0"))
    assert list(c.steps) == ["a", "b"] and sum(len(v) for v in c.steps.values()) == 3
    c.add("c", lambda: _Step("c0"))  # two keys only, but three graphs: "a" (both of its graphs) goes
    assert list(c.steps) == ["b", "c"]
    assert [s.name for s in c.steps["b"] + c.steps["c"]] == ["b0", "c0"]


def test_least_recently_used_eviction_and_a_hit_refreshes_the_key():
    c = _cache(2)
    c.add("a", lambda: _Step("a0"))
    c.add("b", lambda: _Step("b0"))
    assert c.find("a", _load).name == "a0"  # "a" is now the most recent
    c.add("c", lambda: _Step("c0"))
    assert list(c.steps) == ["a", "c"]
    c.steps["a"][0].fits = False
    assert c.find("a", _load) is None  # a miss does not refresh
    c.add("d", lambda: _Step("d0"))
    assert list(c.steps) == ["c", "d"]


def test_find_returns_the_first_step_that_takes_the_batch():
    c = _cache(8)
    steps = [_Step("s0", fits=False), _Step("s1"), _Step("s2")]
    for s in steps:
        c.add("k", lambda s=s: s)
    assert c.find("k", _load) is steps[1]
    assert [s.loads for s in steps] == [1, 1, 0]
    assert c.find("other", _load) is None
    for s in steps:
        s.fits = False
    assert c.find("k", _load) is None and [s.loads for s in steps] == [2, 2, 1]


def test_counters():
    c = _cache(2)
    assert (c.captures, c.replays) == (0, 0)
    for k in "abc":
        c.add(k, lambda k=k: _Step(k))
    c.find("c", _load)
    assert (c.captures, c.replays) == (3, 0)  # replays are counted by the owner, which knows when a replay happened

    def failing():
        raise RuntimeError("capture failed")
    with pytest.raises(RuntimeError):
        c.add("d", failing)
    assert c.captures == 3 and "d" not in c.steps


def test_first_visit_bookkeeping():
    c = _cache(4)
    assert c.first_visit("k") and not c.first_visit("k")
    # visits counted per shape: another key of the same shape is no first visit
    assert c.first_visit(("s", True), "s") and not c.first_visit(("s", False), "s")
    c.add("g", lambda: _Step("g0"))
    assert not c.first_visit("g")  # a key with graphs
    c.drop()
    assert not c.steps and not c.seen and c.first_visit("k")
    c.seen.add("x")
    c.drop()  # nothing captured: the visits stay
    assert "x" in c.seen
