"""The evaluation loops of evaluate.py without a GPU and without the library: the worker pool on a null context (every item
once, input order, the caller's thread for one worker, a failing job), where every scene of a batch starts, and the per-scene
splitting and the laziness of ``predict`` / ``decode`` over a stub model that returns hand-made three-scene graphs."""
import contextlib
import threading
import time

import pytest
import torch

import vlsat_amd  # noqa: F401
from vlsat_amd import evaluate as EV, metrics as M


class Stub:
    """What the loops ask of a model.  ``graphs``: what ``predict_graph`` / ``decode_graph`` return; the calls are recorded."""

    def __init__(self, graphs=None):
        self.graphs, self.calls = graphs, []

    def replicas(self, k):
        return [Stub(self.graphs) for _ in range(k)]

    def predict_graph(self, obj_points, obj_2d_feats, edge_indices, descriptor, batch_ids=None, fc_sizes=None, **args):
        self.calls.append(("predict_graph", obj_points, args))
        return self.graphs

    def decode_graph(self, obj_points, obj_2d_feats, edge_indices, descriptor, batch_ids=None, fc_sizes=None, **args):
        self.calls.append(("decode_graph", obj_points, args))
        return self.graphs[0], (self.graphs[1] if obj_2d_feats is not None else None)


def null_context(dev, own):
    return contextlib.nullcontext()


def run_pool(items, workers, job):
    """``_run_pool`` on the null context, on a thread of the test's so that a pool which never returns fails the test instead of
    hanging it: (the exception it raised or None)."""
    box = []

    def call():
        try:
            EV._run_pool(Stub(), items, None, workers, job, null_context)
            box.append(None)
        except BaseException as ex:
            box.append(ex)

    if workers == 1:                          # (one worker runs in the caller's thread: keep the test's thread the caller)
        call()
    else:
        t = threading.Thread(target=call, daemon=True)
        t.start()
        t.join(timeout=60)
        assert not t.is_alive(), "the pool did not return"
    return box[0]


def racing(n, taken=None):
    """0 .. n-1 from a plain generator that gives the interpreter a reason to switch threads while it runs: two threads in it at
    once -- an item taken outside the lock -- raise ``ValueError: generator already executing``."""
    for i in range(n):
        time.sleep(0)
        if taken is not None:
            taken.append(i)
        yield i


# ---------------------------------------------------------------- the pool
@pytest.mark.parametrize("workers", (1, 2, 5))
@pytest.mark.parametrize("n", (0, 1, 37))
def test_pool_hands_every_item_to_a_job_exactly_once(workers, n):
    seen, lock = [], threading.Lock()

    def job(k, model, item):
        assert 0 <= k < workers and isinstance(model, Stub)
        with lock:
            seen.append((k, item))

    assert run_pool(racing(n), workers, job) is None
    assert sorted(i for _, i in seen) == list(range(n))


@pytest.mark.parametrize("workers", (1, 2, 5))
@pytest.mark.parametrize("n", (0, 1, 37))
def test_pool_results_stored_by_index_sort_into_input_order(workers, n):
    results = {}

    def job(k, model, item):
        results[item[0]] = item[1]

    payload = [f"item{i}" for i in range(n)]
    assert run_pool(enumerate(payload[i] for i in racing(n)), workers, job) is None
    assert [results[i] for i in sorted(results)] == payload


def test_pool_gives_every_worker_its_own_model():
    models, lock = {}, threading.Lock()

    def job(k, model, item):
        with lock:
            models.setdefault(k, set()).add(id(model))

    assert run_pool(racing(37), 5, job) is None
    assert all(len(v) == 1 for v in models.values())
    assert len({next(iter(v)) for v in models.values()}) == len(models)


def test_pool_with_one_worker_runs_in_the_calling_thread():
    idents = set()
    assert run_pool(racing(5), 1, lambda k, m, item: idents.add(threading.get_ident())) is None
    assert idents == {threading.get_ident()}


class Boom(Exception):
    pass


@pytest.mark.parametrize("exc", (Boom("item 7"), KeyboardInterrupt()))
def test_pool_reraises_a_jobs_exception_and_stops_taking_items(exc):
    taken = []

    def job(k, model, item):
        if item == 7:
            raise exc

    assert run_pool(racing(37, taken), 2, job) is exc
    assert 7 in taken and len(taken) < 37


def test_pool_reraises_in_the_calling_thread_with_one_worker():
    exc, taken = Boom("item 7"), []

    def job(k, model, item):
        if item == 7:
            raise exc

    assert run_pool(racing(37, taken), 1, job) is exc
    assert taken == list(range(8))


# ---------------------------------------------------------------- where every scene starts
def three_scene_batch():
    """Scenes of 2, 3 and 1 nodes with their fully connected edge lists of 2, 6 and 0 edges, as the loader collates them."""
    edges = [(0, 1), (1, 0), (2, 3), (2, 4), (3, 2), (3, 4), (4, 2), (4, 3)]
    return {"obj_points": torch.zeros(6, 3, 4), "obj_2d_feats": torch.zeros(6, 8), "descriptor": torch.zeros(6, 11),
            "edge_indices": torch.tensor(edges, dtype=torch.int64), "batch_ids": torch.tensor([0, 0, 1, 1, 1, 2]).view(-1, 1)}


def test_scene_starts_of_a_batch_whose_last_scene_has_no_edges():
    node, edge = EV._scene_starts(three_scene_batch(), 3)
    assert node == [0, 2, 5, 6]
    assert edge == [0, 2, 8, 8]
    assert EV._scene_starts(three_scene_batch(), 3, nodes=False) == (None, [0, 2, 8, 8])


def test_scene_starts_of_a_batch_whose_middle_scene_has_no_edges():
    b = three_scene_batch()
    b["batch_ids"] = torch.tensor([0, 0, 1, 2, 2, 2]).view(-1, 1)
    b["edge_indices"] = torch.tensor([(0, 1), (1, 0), (3, 4), (3, 5), (4, 3), (4, 5), (5, 3), (5, 4)])
    assert EV._scene_starts(b, 3) == ([0, 2, 3, 6], [0, 2, 2, 8])


# ---------------------------------------------------------------- decode / predict over a stub model
I32 = torch.int32


def decoded_three_scenes(shift=0):
    """A three-scene DecodedGraph over three_scene_batch(): max_rel = 3, two labels per node; ``shift`` tells two branches apart."""
    labels = (torch.arange(12, dtype=I32).view(6, 2) + shift)
    probs = torch.arange(12, dtype=torch.float32).view(6, 2) / 16 + shift
    rels = torch.tensor([[[0, 3], [1, 5], [-1, -1]],
                         [[2, 1], [7, 2], [-1, -1]],
                         [[-1, -1], [-1, -1], [-1, -1]]], dtype=I32)
    rels[..., 1] += shift * (rels[..., 1] >= 0)
    score = torch.tensor([[.9, .8, 0.], [.7, .6, 0.], [0., 0., 0.]]) + shift
    return M.DecodedGraph(labels, probs, rels, score, torch.tensor([2, 2, 0], dtype=I32), torch.tensor([2, 5, 0], dtype=I32))


def expect_decoded(g, shift, edge, pred, score, n_valid, n_total, nodes):
    lo, hi = nodes
    assert torch.equal(g.edge, torch.tensor([edge], dtype=I32))
    assert torch.equal(g.pred, torch.tensor([pred], dtype=I32))
    assert torch.equal(g.score, torch.tensor([score]) + shift)
    assert torch.equal(g.n_valid, torch.tensor([n_valid], dtype=I32)) and torch.equal(g.n_total, torch.tensor([n_total], dtype=I32))
    assert torch.equal(g.labels, torch.arange(2 * lo, 2 * hi, dtype=I32).view(-1, 2) + shift)
    assert torch.equal(g.label_probs, torch.arange(2 * lo, 2 * hi, dtype=torch.float32).view(-1, 2) / 16 + shift)


@pytest.mark.parametrize("use_2d", (True, False))
def test_decode_splits_a_batch_into_its_scenes(use_2d):
    m = Stub((decoded_three_scenes(), decoded_three_scenes(shift=1)))
    out = list(EV.decode(m, [three_scene_batch()], use_2d=use_2d, threshold=0.25))
    assert len(out) == 3 and m.calls[0][0] == "decode_graph" and m.calls[0][2] == {"threshold": 0.25}
    for br, shift in ((0, 0), (1, 1)):
        if br == 1 and not use_2d:
            assert all(pair[1] is None for pair in out)
            continue
        p = lambda *ks: [k + shift if k >= 0 else k for k in ks]
        expect_decoded(out[0][br], shift, [0, 1, -1], p(3, 5, -1), [.9, .8, 0.], 2, 2, (0, 2))
        expect_decoded(out[1][br], shift, [0, 5, -1], p(1, 2, -1), [.7, .6, 0.], 2, 5, (2, 5))      # rows rebased by 2, -1 kept
        expect_decoded(out[2][br], shift, [-1, -1, -1], [-1, -1, -1], [0., 0., 0.], 0, 0, (5, 6))


def scene_graph_three_scenes(shift=0):
    """A three-scene SceneGraph over three_scene_batch(): top_k = 2; columns (edge, sub_cls, obj_cls, pred)."""
    trip = torch.tensor([[[1, 10, 11, 3], [0, 11, 10, 4]],
                         [[6, 12, 13, 5], [-1, -1, -1, -1]],
                         [[-1, -1, -1, -1], [-1, -1, -1, -1]]], dtype=I32)
    trip[..., 3] += shift * (trip[..., 3] >= 0)
    return M.SceneGraph(trip, torch.tensor([[.5, .25], [.125, 0.], [0., 0.]]) + shift, torch.tensor([2, 1, 0], dtype=I32))


def test_predict_splits_a_batch_into_its_scenes():
    m = Stub((scene_graph_three_scenes(), scene_graph_three_scenes(shift=1)))
    out = list(EV.predict(m, [three_scene_batch()], top_k=2))
    assert len(out) == 3 and m.calls[0][0] == "predict_graph" and m.calls[0][2] == {"top_k": 2}
    want = (([1, 0], [10, 11], [11, 10], [3, 4], [.5, .25], 2),
            ([4, -1], [12, -1], [13, -1], [5, -1], [.125, 0.], 1),                                  # row 6 rebased by 2, -1 kept
            ([-1, -1], [-1, -1], [-1, -1], [-1, -1], [0., 0.], 0))
    for pair, (edge, sub, obj, pred, score, n_valid) in zip(out, want):
        for g, shift in zip(pair, (0, 1)):
            assert torch.equal(g.edge, torch.tensor([edge], dtype=I32))
            assert torch.equal(g.sub_cls, torch.tensor([sub], dtype=I32)) and torch.equal(g.obj_cls, torch.tensor([obj], dtype=I32))
            assert torch.equal(g.pred, torch.tensor([[k + shift if k >= 0 else k for k in pred]], dtype=I32))
            assert torch.equal(g.score, torch.tensor([score]) + shift)
            assert torch.equal(g.n_valid, torch.tensor([n_valid], dtype=I32))


def one_scene_batch():
    b = three_scene_batch()
    del b["batch_ids"]
    return b


def test_a_one_scene_batch_without_batch_ids_is_yielded_as_the_model_returned_it():
    d = M.DecodedGraph(torch.zeros(6, 2, dtype=I32), torch.zeros(6, 2), torch.full((1, 3, 2), -1, dtype=I32), torch.zeros(1, 3),
                       torch.zeros(1, dtype=I32), torch.zeros(1, dtype=I32))
    (g3, g2), = list(EV.decode(Stub((d, d)), [one_scene_batch()]))
    assert g3 is d and g2 is d
    (g3, g2), = list(EV.decode(Stub((d, d)), [one_scene_batch()], use_2d=False))
    assert g3 is d and g2 is None
    s = M.SceneGraph(torch.full((1, 2, 4), -1, dtype=I32), torch.zeros(1, 2), torch.zeros(1, dtype=I32))
    (g3, g2), = list(EV.predict(Stub((s, s)), [one_scene_batch()]))
    assert g3 is s and g2 is s


@pytest.mark.parametrize("loop,graphs", (("decode", decoded_three_scenes), ("predict", scene_graph_three_scenes)))
def test_serial_loops_touch_the_next_batch_only_after_the_scenes_of_this_one(loop, graphs):
    m, made = Stub((graphs(), graphs())), []

    def batches():
        for i in range(2):
            made.append(i)
            yield three_scene_batch()

    it = getattr(EV, loop)(m, batches())
    assert made == [] and m.calls == []                       # a generator: nothing runs before the first next()
    next(it)
    assert made == [0] and len(m.calls) == 1
    next(it), next(it)
    assert made == [0] and len(m.calls) == 1
    next(it)
    assert made == [0, 1] and len(m.calls) == 2
    assert len(list(it)) == 2


@pytest.mark.parametrize("loop", ("decode", "predict", "merged"))
def test_workers_without_a_device_is_refused_at_the_first_next(loop):
    m = Stub()
    it = getattr(EV, loop)(m, [three_scene_batch()], workers=1)
    with pytest.raises(ValueError, match=rf"{loop}\(workers > 0\) needs the device"):
        next(it)
    assert m.calls == []


def test_calibrate_workers_without_a_device_is_refused_when_called():
    with pytest.raises(ValueError, match=r"calibrate\(workers > 0\) needs the device"):
        EV.calibrate(Stub(), [three_scene_batch()], workers=1)
