"""``progen_amd.engine.SlotEngine`` on the CPU (fp32, the tiny config of
tests/test_serve_device_sampling.py): requests of different lengths share
one decode batch, each at its own position, and every request gets the
tokens ``sample_cached_batch`` gives it when it runs alone.

Staggered requests are compared with single-request runs of another batch
size. That is exact here: on this config a row's tokens do not depend on its
batch companions (checked for row 0 alone and with 2 and 5 others, greedy and
top_k=25 with seeds 0..5, in fp32 and fp64: 24 of 24 runs identical)."""

import threading

import pytest
import torch

from progen_amd import ProGenBase, ProGenConfig
from progen_amd.decode import sample_cached_batch
from progen_amd.engine import SlotEngine

PRIMES = [[0, 35, 32, 77], [0, 35, 32, 71, 65], [0, 40],
          [0, 35, 32, 77, 75, 86, 76]]


@pytest.fixture(scope="module")
def model():
    cfg = ProGenConfig(num_tokens=256, dim=16, depth=2, dim_head=8, heads=2,
                       window_size=8, seq_len=64, global_mlp_depth=1)
    torch.manual_seed(5)
    return ProGenBase(cfg).eval()


def _alone(model, primes, length, top_k=None, seed=None):
    return sample_cached_batch(model, [torch.tensor(p) for p in primes],
                               length, top_k=top_k, seed=seed, fused=True,
                               device_sampling=True)


_WANT = {}


def _want(model, key, *args, **kw):
    """References are computed once and shared."""
    if key not in _WANT:
        _WANT[key] = _alone(model, *args, **kw)
    return _WANT[key].clone()


@pytest.mark.parametrize("top_k,seed", [(None, None), (25, 123)])
def test_one_ragged_request_equals_sample_cached_batch(model, top_k, seed):
    want = _want(model, ("ragged", top_k, seed), PRIMES, 48, top_k, seed)
    engine = SlotEngine(model, 4)
    ticket = engine.submit(PRIMES, 48, top_k=top_k, seed=seed)
    assert not ticket.done
    engine.run_until_idle()
    assert ticket.done and ticket.slots == [0, 1, 2, 3]
    assert torch.equal(ticket.wait(), want)


STAGGERED = [(PRIMES[0], 24), (PRIMES[1], 40), (PRIMES[2], 32)]


def _staggered(model, check_every, top_k=None, seed=None):
    engine = SlotEngine(model, 2, check_every=check_every)
    tickets = [engine.submit([p], n, top_k=top_k, seed=seed)
               for p, n in STAGGERED]
    engine.run_until_idle()
    return engine, tickets


@pytest.mark.parametrize("top_k,seed", [(None, None), (25, 7)])
def test_staggered_requests_reuse_a_freed_slot(model, top_k, seed):
    engine, tickets = _staggered(model, 16, top_k, seed)
    for i, ((p, n), t) in enumerate(zip(STAGGERED, tickets)):
        want = _want(model, ("stag", i, top_k, seed), [p], n, top_k, seed)
        assert t.result.shape == (1, n)
        assert torch.equal(t.wait(), want), i
    assert tickets[0].slots == [0] and tickets[1].slots == [1]
    # the shortest request frees slot 0 first and the third one takes it
    assert tickets[2].slots == [0]
    # two slots were busy for most of the run
    assert 0.5 < engine.occupied_slot_steps / (2 * engine.steps) <= 1.0


def test_results_do_not_depend_on_check_every(model):
    runs = [[t.wait() for t in _staggered(model, ce, 25, 7)[1]]
            for ce in (1, 16, 64)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


def test_a_row_that_samples_its_second_pad_retires_and_frees_its_slot(model):
    # find a seeded request that ends early on this model, then check that
    # the engine hands its slot to the next request in the queue
    length = 64
    early = None
    for seed in range(40):
        out = _alone(model, [PRIMES[0]], length, 25, seed)[0]
        pad = (out[1:] == 0).nonzero()
        if len(pad) and int(pad[0]) + 1 < length - 8:
            early = seed
            break
    assert early is not None, "no early finisher among 40 seeds"
    want_a = _alone(model, [PRIMES[0]], length, 25, early)
    end = int((want_a[0, 1:] == 0).nonzero()[0]) + 1   # index of the 2nd pad
    assert not want_a[0, end:].any()
    engine = SlotEngine(model, 1, check_every=1)
    a = engine.submit([PRIMES[0]], length, top_k=25, seed=early)
    b = engine.submit([PRIMES[1]], 24)
    engine.run_until_idle()
    assert torch.equal(a.wait(), want_a)
    assert torch.equal(b.wait(), _alone(model, [PRIMES[1]], 24))
    assert a.slots == [0] and b.slots == [0]
    # a stopped at its second pad: the slot ran ``end`` steps for it, not 63
    assert engine.steps == end + 23


def test_more_rows_than_slots_queue_and_complete(model):
    primes = PRIMES + PRIMES[:3]
    engine = SlotEngine(model, 3)
    ticket = engine.submit(primes, 32, top_k=25, seed=11)
    engine.run_until_idle()
    out = ticket.wait()
    # stream i belongs to row i of the request wherever it ran: each row is
    # that row of the whole request decoded in one batch
    want = _alone(model, primes, 32, 25, 11)
    assert torch.equal(out, want)
    assert sorted(set(ticket.slots)) == [0, 1, 2]
    assert ticket.slots[:3] == [0, 1, 2]


def test_eight_threads_get_their_own_answers(model):
    jobs = [(PRIMES[i % 4], 24 + 4 * i, 25, 100 + i) for i in range(8)]
    want = [_alone(model, [p], n, k, s) for p, n, k, s in jobs]
    got = [None] * 8
    with SlotEngine(model, 3, check_every=4) as engine:
        def work(i):
            p, n, k, s = jobs[i]
            got[i] = engine.generate([p], n, top_k=k, seed=s)
        threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    for i in range(8):
        assert torch.equal(got[i], want[i]), i
    with pytest.raises(RuntimeError, match="closed"):
        engine.submit([PRIMES[0]], 8)


def test_generate_without_a_worker_runs_the_loop_itself(model):
    engine = SlotEngine(model, 2)
    out = engine.generate([PRIMES[2]], 16)
    assert torch.equal(out, _alone(model, [PRIMES[2]], 16))


@pytest.mark.parametrize("kw", [
    dict(length=0), dict(length=65), dict(length=4),     # prime fills it
    dict(top_k=-1), dict(top_k=257), dict(seed=-1), dict(seed=2 ** 63),
    dict(primes=[]), dict(primes=[[0, 300]]),
])
def test_a_bad_request_is_refused_before_any_slot_changes(model, kw):
    engine = SlotEngine(model, 2)
    args = dict(primes=[PRIMES[0]], length=32, top_k=None, seed=None)
    args.update(kw)
    with pytest.raises(ValueError):
        engine.submit(**args)
    assert not engine._queue and engine._active == [None, None]
    assert engine.steps == 0
    with pytest.raises(TypeError):
        engine.submit([PRIMES[0]], 32, generator=torch.Generator())


def test_bad_engine_arguments_are_refused(model):
    with pytest.raises(ValueError):
        SlotEngine(model, 0)
    with pytest.raises(ValueError):
        SlotEngine(model, 2, check_every=0)
