"""GPU: the admit prefill kernels (progen_amd/ops/hip/prefill_admit.hip) and
``SlotEngine(prefill=True)`` on them.

The kernels have no tolerance of their own: they are prefill.hip's bodies
with the cache row and the row count read from device memory, so their
full-sequence outputs have the bits of ``rope_qkv`` and of the no-admit
call, the cache rows they store have the bits of those outputs, and every
other element of the caches keeps the NaN bits it held. The caches are the
first S = 3 rows of a 4-row allocation, so that a batch row that names slot
S is a checked no-op inside owned memory. The gate LN is also held to the
fp64 oracle within kernel_oracle's ``ln`` bound.

The engine is held to ``decode.prefill``: a prefilled admission, captured or
eager, launches the kernels of an eager ``decode.prefill`` of one row at the
same shapes, so the slot's cache rows, halos and history rows have its bits,
and the tokens are those of ``sample_cached_batch(prefill=True)`` at one slot
and of a hand-driven prefill + slot-step loop at two.
"""

import functools
import types

import pytest
import torch

import kernel_oracle as K
from progen_amd import decode
from progen_amd.ops import dispatch, functional as OF, reference as R

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]

DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def admit_dev(*rows):
    return torch.tensor(rows, dtype=torch.long).to(DEV)


def nan_cache(*shape):
    """(the 4-row allocation, its first 3 rows as the kernels' cache)"""
    full = torch.full((4,) + shape, NAN, dtype=BF, device=DEV)
    return full, full[:3]


# ---------------------------------------------------------------------------
# prefill_rope_kv with admit
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("Np", [64, 256])
@pytest.mark.parametrize("c", [1, 63, "Np"])
def test_rope_kv_with_admit(Np, c):
    Rb, H, Nc = 2, 2, 256
    c = Np if c == "Np" else c
    g = torch.Generator().manual_seed(40 + Np)
    qkv = torch.randn(Rb, Np, 3 * H * 64, generator=g).to(BF).to(DEV)
    sin, cos = (t.to(DEV) for t in K.rope_tables(Nc))
    want = dispatch.ext().rope_qkv(qkv, sin, cos)
    heads = want.view(Rb, Np, 3, H, 64)

    # batch row 0 -> slot 2, rows < c; batch row 1 names no slot, then slot S
    for second in ([-1, Np], [3, Np]):
        k_full, k_cache = nan_cache(H, Nc, 64)
        v_full, v_cache = nan_cache(H, Nc, 64)
        rot = dispatch.ext_prefill().prefill_rope_kv(
            qkv, sin, cos, k_cache, v_cache, Np,
            admit=admit_dev([2, c], second))
        assert torch.equal(bits(rot), bits(want))
        for name, full, which in (("k", k_full, 1), ("v", v_full, 2)):
            expect = torch.full_like(full, NAN)
            expect[2, :, :c] = heads[0, :c, which].transpose(0, 1)
            assert torch.equal(bits(full), bits(expect)), (name, second)


# ---------------------------------------------------------------------------
# prefill_gate_ln with admit
# ---------------------------------------------------------------------------

# d2 = 64: the single-pass path; 3072: the re-reading one
@pytest.mark.parametrize("d2", [64, 3072])
@pytest.mark.parametrize("Np", [64, 256])
@pytest.mark.parametrize("c", [1, 63, "Np"])
def test_gate_ln_with_admit(d2, Np, c):
    Rb, Nc = 2, 256
    c = Np if c == "Np" else c
    g = torch.Generator().manual_seed(50 + d2 + Np)
    x = torch.randn(Rb, Np, 2 * d2, generator=g)
    x[..., :d2] = 5 * x[..., :d2] + 3        # the half that must not be read
    x = x.to(BF)
    w = (1 + 0.25 * torch.randn(d2, generator=g)).to(BF)
    plain = dispatch.ext_prefill().prefill_gate_ln(
        x.to(DEV), w.to(DEV), torch.zeros(Rb, Nc, d2, dtype=BF, device=DEV),
        Np, 1e-5)
    oracle = R.layernorm_nobias(x[..., d2:].double(), w.double(), 1e-5)

    for second in ([-1, Np], [3, Np]):
        full, hist = nan_cache(Nc, d2)
        got = dispatch.ext_prefill().prefill_gate_ln(
            x.to(DEV), w.to(DEV), hist, Np, 1e-5,
            admit=admit_dev([2, c], second))
        assert got.shape == (Rb, Np, d2) and got.is_contiguous()
        err = K.row_err(got, oracle)
        emu, bound = K.bounds("ln", "bf16")["y"]
        print(f"ADMIT|gate_ln|d2={d2}|Np={Np}|c={c}|{emu:.3e}|{bound:.3e}|"
              f"{err:.3e}")
        assert err <= bound
        assert torch.equal(bits(got), bits(plain))
        expect = torch.full_like(full, NAN)
        expect[2, :c] = got[0, :c]
        assert torch.equal(bits(full), bits(expect)), second


# ---------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _model(ff_glu=False):
    # the model of tests/test_gpu_decode_slots.py (its third layer is an SGU
    # one); ``ff_glu``: the variant with GLU feed-forwards
    from progen_amd import ProGenBase, ProGenConfig
    cfg = ProGenConfig(num_tokens=256, dim=256, depth=3, heads=4,
                       dim_head=64, window_size=64, seq_len=256,
                       ff_glu=ff_glu, global_mlp_depth=1)
    torch.manual_seed(3)
    m = ProGenBase(cfg).to(device="cuda", dtype=BF).eval()
    m.rotary_sin = m.rotary_sin.float()
    m.rotary_cos = m.rotary_cos.float()
    return m


def _prime(n, seed=0):
    g = torch.Generator().manual_seed(900 + 3 * n + seed)
    return torch.randint(1, 256, (n,), generator=g)


def _cache_tensors(cache):
    """(name, tensor, dimension of a slot's tensor its positions run along,
    or None for the halos)"""
    out = [(f"k{i}", t, 1) for i, t in enumerate(cache.k)]
    out += [(f"v{i}", t, 1) for i, t in enumerate(cache.v)]
    out += [(f"gate_hist{i}", t, 0) for i, t in enumerate(cache.gate_hist)
            if t is not None]
    out += [(f"attn_prev{i}", t, None) for i, t in enumerate(cache.attn_prev)]
    out += [(f"ff_prev{i}", t, None) for i, t in enumerate(cache.ff_prev)]
    return out


def _admit_only(engine):
    """One engine cycle whose steps do nothing: the state an admission
    leaves. Returns the call that puts the steps back."""
    if engine._graph is not None:
        real = engine._graph
        engine._graph = types.SimpleNamespace(replay=lambda: None)
        engine.cycle()

        def restore():
            engine._graph = real
    else:
        engine._step = lambda: None
        engine.cycle()

        def restore():
            del engine._step
    return restore


@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
@pytest.mark.parametrize("ff_glu", [False, True], ids=["gelu", "glu"])
def test_a_prefilled_admission_leaves_the_bits_of_decode_prefill(ff_glu,
                                                                 graph):
    from progen_amd.engine import SlotEngine
    m = _model(ff_glu)
    L = m.cfg.seq_len
    engine = SlotEngine(m, 2, graph=graph, fused_linear=True, prefill=True,
                        prefill_rows=1, prefill_min_tokens=8)
    engine.cycle()          # nothing queued: builds and captures only
    assert len(engine._pf_graphs) == (len(engine._buckets) if graph else 0)
    # P - 1 prefilled positions, into slot 0 and, behind a stepped filler
    # request admitted in the same cycle, into slot 1
    for n, b in ((8, 0), (63, 1), (64, 0), (65, 1)):
        prime = _prime(n + 1)
        # only copies may touch the engine's tensors between replays
        for _name, t, _dim in _cache_tensors(engine.cache):
            t.copy_(torch.full(t.shape, NAN, dtype=BF))
        nan = {name: bits(t) for name, t, _d in _cache_tensors(engine.cache)}
        if b == 1:
            engine.submit([_prime(3, 1)], 6)
        ticket = engine.submit([prime], n + 3)
        before = engine.prefills
        restore = _admit_only(engine)
        assert ticket.slots == [b] and engine.prefills == before + 1

        one = decode.DecodeCache(m, batch=1)
        decode.prefill(m, prime[None, :n], one)
        for (name, got, dim), (_n, want, _d) in zip(
                _cache_tensors(engine.cache), _cache_tensors(one)):
            other = 1 - b
            assert torch.equal(bits(got[other]), nan[name][other]), \
                (name, n, "the other slot")
            if dim is None:
                assert torch.equal(bits(got[b]), bits(want[0])), (name, n)
                continue
            assert torch.equal(bits(got[b].narrow(dim, 0, n)),
                               bits(want[0].narrow(dim, 0, n))), (name, n)
            assert torch.equal(bits(got[b].narrow(dim, n, L - n)),
                               nan[name][b].narrow(dim, n, L - n)), \
                (name, n, "rows past the prime")
        assert engine.pos.tolist()[b] == n
        assert engine.token.tolist()[b] == int(prime[n])
        restore()
        engine.run_until_idle()
        assert torch.equal(ticket.wait()[0, :n + 1], prime)


FAST = dict(graph=True, fused=True, fused_linear=True, device_sampling=True)


@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
def test_one_slot_equals_sample_cached_batch_with_prefill(graph):
    from progen_amd.engine import SlotEngine
    m = _model()
    engine = SlotEngine(m, 1, graph=graph, fused_linear=True, prefill=True,
                        prefill_min_tokens=8)
    for n, top_k, seed in ((20, None, None), (70, 25, 13)):
        prime = _prime(n, 2)
        assert decode.prefill_supported(m, n - 1, DEV)
        want = decode.sample_cached_batch(m, [prime], n + 40, top_k=top_k,
                                          seed=seed, prefill=True, **FAST)
        before = engine.prefills
        got = engine.generate([prime], n + 40, top_k=top_k, seed=seed)
        assert engine.prefills == before + 1
        assert torch.equal(got, want), (n, top_k, seed)


def _hand_driven(m, prime, length, slot):
    """Eager ``decode.prefill`` of prime[:P-1] into a 1-row cache, its rows
    copied into row ``slot`` of a 2-row cache, then ``forward_step_slots`` +
    ``decode_sample_slots`` with the other row idle, greedy."""
    P, L = len(prime), m.cfg.seq_len
    n = P - 1
    one = decode.DecodeCache(m, batch=1)
    decode.prefill(m, prime[None, :n], one)
    two = decode.DecodeCache(m, batch=2)
    for (_name, dst, dim), (_n, src, _d) in zip(_cache_tensors(two),
                                                _cache_tensors(one)):
        if dim is None:
            dst[slot].copy_(src[0])
        else:
            dst[slot].narrow(dim, 0, n).copy_(src[0].narrow(dim, 0, n))
    pos = torch.full((2,), -1, dtype=torch.long)
    token = torch.zeros(2, dtype=torch.long)
    seq = torch.zeros(2, L, dtype=torch.long)
    pads = torch.zeros(2, dtype=torch.long)
    ctl = torch.zeros(2, len(OF.SLOT_CTL), dtype=torch.long)
    pos[slot], token[slot] = n, prime[n]
    seq[slot, :P] = prime
    pads[slot] = int((prime == 0).sum())
    ctl[slot] = torch.tensor([P, length, 0, -1, 0])
    pos, token, seq, pads, ctl = (t.to(DEV) for t in
                                  (pos, token, seq, pads, ctl))
    for _ in range(length):
        if int(pos[slot]) < 0:
            break
        logits = decode.forward_step_slots(m, token, two, pos,
                                           fused_linear=True)
        OF.decode_sample_slots(logits, pos, token, seq, pads, ctl)
    assert int(pos[slot]) < 0
    out = seq[slot, :length].cpu()
    after_eos = (out == 0).long().cumsum(dim=-1) > 1
    return out * (~after_eos).long()


@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
def test_two_slots_staggered_equal_a_hand_driven_loop(graph):
    from progen_amd.engine import SlotEngine
    m = _model()
    engine = SlotEngine(m, 2, graph=graph, fused_linear=True, prefill=True,
                        prefill_min_tokens=8)
    work = [(_prime(20, 4), 40), (_prime(12, 5), 56), (_prime(30, 6), 48)]
    tickets = [engine.submit([p], n) for p, n in work]
    engine.run_until_idle()
    assert engine.prefills == 3
    assert [t.slots for t in tickets] == [[0], [1], [0]]
    for t, (p, n) in zip(tickets, work):
        want = _hand_driven(m, p, n, t.slots[0])
        assert torch.equal(t.wait()[0], want), (t.slots, n)
