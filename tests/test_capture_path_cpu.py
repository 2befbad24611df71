"""the sampling side has ONE capture path (lion_amd/chain.py::CapturedStep; training.py keeps its forward+backward graphs):
no other module of the package begins a graph capture of its own."""
import glob
import os

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lion_amd")


def test_graph_capture_lives_in_chain_and_training_only():
    found = {}
    for path in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True):
        text = open(path).read()
        hits = [s for s in ("CUDAGraph(", "capture_begin", "torch.cuda.graph(") if s in text]
        if hits:
            found[os.path.relpath(path, PKG)] = hits
    assert set(found) <= {"chain.py", "training.py"}, found
    assert "chain.py" in found
    assert "GraphedChain" not in open(os.path.join(PKG, "ode.py")).read()


def test_lru_of_captured_objects():
    """chain.LRU (ChainCache, ode.graph_for): a usable hit is kept and becomes the most recent, an unusable one is dropped
    before its replacement is built, and the least recently used entry leaves beyond the capacity"""
    from lion_amd.chain import LRU
    built = []

    def build(tag):
        def make():
            assert tag[0] not in cache._entries      # the stale entry is gone before the new one is built
            built.append(tag)
            return tag
        return make
    cache = LRU(capacity=2)
    a = cache.lookup("a", lambda e: True, build(["a", 0]))
    assert cache.lookup("a", lambda e: True, build(["a", 1])) is a and len(built) == 1
    a2 = cache.lookup("a", lambda e: False, build(["a", 2]))
    assert a2 == ["a", 2] and len(cache._entries) == 1
    cache.lookup("b", lambda e: True, build(["b", 0]))
    cache.lookup("a", lambda e: True, build(["a", 3]))          # a is now the most recent
    cache.lookup("c", lambda e: True, build(["c", 0]))          # b leaves
    assert list(cache._entries) == ["a", "c"] and list(cache._entries.values()) == [a2, ["c", 0]]
    cache.clear()
    assert len(cache._entries) == 0
