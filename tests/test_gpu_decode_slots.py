"""GPU: the slot kernels (progen_amd/ops/hip/decode_slots.hip) and the slot
engine (progen_amd/engine.py).

The three forward slot kernels have NO tolerance: they are the bodies of the
scalar kernels instantiated with a position per row, so row b of a slot
launch must equal, bit for bit, row b of the scalar kernel launched on a
clone with pos = pos[b] — the output, the written cache / prev / hist row,
and h. Every cache row a step must not read holds NaN before the launch (as
in tests/test_gpu_decode_fused.py), and so does all of an idle row's cache.

The slot sampler equals the scalar sampler bit for bit under uniform
controls, and ``reference.decode_sample_slots`` token for token under per-row
ones — every row, none left out: over the three logit families x 40 draws x
three vocabularies (2160 stochastic rows) the fp64 gap between the best two
scores (``gap64``) is never under 2.1e-3 on the CPU, against the 1e-4
near-tie line of tests/test_gpu_decode_sample.py.

The engine runs the model of tests/test_gpu_decode_sample.py. A request that
fills every slot from position 0 has the batch size, the body and the rows
of ``sample_cached_batch``, so identical logits: ties cannot matter. No test
launches with pos >= N.
"""

import pytest
import torch

import decode_sample_cases as C
from progen_amd.ops import dispatch
from progen_amd.ops import functional as OF
from progen_amd.ops import reference as R

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]

DTYPES = [torch.bfloat16, torch.float32]
NAN = float("nan")


def bits(t):
    """Raw bits, so that NaNs compare equal to themselves."""
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def dev_pos(pos):
    return torch.tensor(pos, dtype=torch.long).cuda()


# ---- dec_attn_slots ---------------------------------------------------------

# the last two: short bands, where some of the 32 lane groups or whole waves
# have no row (tests/decode_oracle.py)
ATTN = [(64, 256, [0, 63, 64, 200]), (64, 256, [-1, 127, 128, 255]),
        (256, 512, [255, 256, 511, -1]), (64, 256, [1, 7, 8, 33]),
        (64, 256, [9, 31, 32, -1])]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("window,N,pos", ATTN,
                         ids=[f"w{w}-N{n}-{i}"
                              for i, (w, n, _) in enumerate(ATTN)])
def test_attn_slots_rows_equal_the_scalar_kernel(window, N, pos, dtype):
    B, H = 4, 2
    g = torch.Generator().manual_seed(N + window)
    sin, cos = R.fixed_pos_embedding(N, 64)
    sin, cos = sin.float().cuda(), cos.float().cuda()
    qkv = torch.randn(B, 3 * H * 64, generator=g).to(dtype).cuda()
    k0 = torch.full((B, H, N, 64), NAN)
    v0 = torch.full((B, H, N, 64), NAN)
    for b, p in enumerate(pos):
        if p < 0:
            continue
        w0 = (p // window) * window
        start = max(w0 - window, 0)
        k0[b, :, start:p] = torch.randn(H, p - start, 64, generator=g)
        v0[b, :, start:p] = torch.randn(H, p - start, 64, generator=g)
    k0, v0 = k0.to(dtype).cuda(), v0.to(dtype).cuda()

    ks, vs = k0.clone(), v0.clone()
    out = dispatch.ext_decode_slots().dec_attn_slots(
        qkv, sin, cos, dev_pos(pos), ks, vs, window)
    for b, p in enumerate(pos):
        if p < 0:
            assert not out[b].any(), "idle row output"
            assert same(ks[b], k0[b]) and same(vs[b], v0[b]), "idle caches"
            continue
        kc, vc = k0.clone(), v0.clone()
        want = dispatch.ext_decode().dec_attn(qkv, sin, cos, dev_pos(p), kc,
                                              vc, window)
        assert torch.isfinite(want[b]).all(), (b, p)
        assert same(out[b], want[b]), ("out", b, p)
        assert same(ks[b], kc[b]) and same(vs[b], vc[b]), ("cache", b, p)
        assert torch.isfinite(ks[b, :, p]).all()


# ---- dec_sgu_slots -----------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("d2", [64, 320])
def test_sgu_slots_rows_equal_the_scalar_kernel(d2, dtype):
    N, pos = 256, [0, 1, 31, 32, 255, -1]
    B = len(pos)
    g = torch.Generator().manual_seed(d2)
    h = torch.randn(B, 2 * d2, generator=g).to(dtype).cuda()
    gw = torch.randn(d2, generator=g).to(dtype).cuda()
    w = (torch.randn(N, N, generator=g) / 16).to(dtype).cuda()
    bias = torch.randn(N, 1, generator=g).to(dtype).cuda()
    hist0 = torch.full((B, N, d2), NAN)
    for b, p in enumerate(pos):
        if p > 0:
            hist0[b, :p] = torch.randn(p, d2, generator=g)
    hist0 = hist0.to(dtype).cuda()

    hs = hist0.clone()
    out = dispatch.ext_decode_slots().dec_sgu_slots(h, gw, hs, w, bias,
                                                    dev_pos(pos), 1e-5)
    for b, p in enumerate(pos):
        if p < 0:
            assert not out[b].any(), "idle row output"
            assert same(hs[b], hist0[b]), "idle history"
            continue
        hc = hist0.clone()
        want = dispatch.ext_decode().dec_sgu(h, gw, hc, w, bias, dev_pos(p),
                                             1e-5)
        assert torch.isfinite(want[b]).all(), (b, p)
        assert same(out[b], want[b]), ("out", b, p)
        assert same(hs[b], hc[b]), ("hist", b, p)


# ---- dec_ln_shift_slots ------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("use_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("shift,use_prev", [(True, True), (False, True),
                                            (False, False)],
                         ids=["shift", "noshift", "noprev"])
@pytest.mark.parametrize("D", [128, 4096])
def test_ln_shift_slots_rows_equal_the_scalar_kernel(D, shift, use_prev,
                                                     use_res, dtype):
    pos = [0, 5, -1]
    g = torch.Generator().manual_seed(D)
    h0 = torch.randn(3, D, generator=g).to(dtype).cuda()
    res = torch.randn(3, D, generator=g).to(dtype).cuda() if use_res else None
    gw = torch.randn(D, generator=g).to(dtype).cuda()
    prev0 = torch.randn(3, D, generator=g)
    prev0[0] = NAN      # the slot's last request: never read at position 0
    prev0 = prev0.to(dtype).cuda() if use_prev else None

    hs = h0.clone()
    ps = prev0.clone() if use_prev else None
    y = dispatch.ext_decode_slots().dec_ln_shift_slots(
        hs, res, gw, ps, dev_pos(pos), shift, 1e-5)
    hc = h0.clone()
    pc = None
    if use_prev:
        pc = prev0.clone()
        pc[0] = 0       # what position 0 reads
    want = dispatch.ext_decode().dec_ln_shift(hc, res, gw, pc, shift, 1e-5)
    assert torch.isfinite(want[:2]).all()
    for b in (0, 1):
        assert same(y[b], want[b]), ("y", b)
        assert same(hs[b], hc[b]), ("h", b)
        if use_prev:
            assert same(ps[b], pc[b]), ("prev", b)
    assert not y[2].any(), "idle row output"
    assert same(hs[2], h0[2]), "idle h"
    if use_prev:
        assert same(ps[2], prev0[2]), "idle prev"


# ---- dec_sample_slots --------------------------------------------------------

L = 32


def _sample_slots(t, pos, ctl, st, device, fn):
    _seed, seq, _lens, pads, token = [x.clone().to(device) for x in st]
    pos = torch.tensor(pos, dtype=torch.long).to(device)
    u = torch.full(t.shape, -1.0, dtype=torch.float32, device=device)
    fn(t.to(device), pos, token, seq, pads,
       torch.tensor(ctl, dtype=torch.long).to(device), u)
    return [x.cpu() for x in (seq, pads, token, u, pos)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("V,top_k,seed", [(256, 25, 11), (1000, 0, 5),
                                          (7, 3, -1)])
def test_sample_slots_with_uniform_controls_is_the_scalar_kernel(V, top_k,
                                                                 seed, dtype):
    B, p = 8, 5
    t = C.make_logits("normal", B, V, top_k, 1).to(dtype)
    lens = [0, 9, 0, 3, 7, 0, 6, 31]
    st = C.state(B, L, lens=lens, seed=max(seed, 0))
    seed_t, seq, lens_t, pads, token = [x.clone().cuda() for x in st]
    u = torch.full((B, V), -1.0, device="cuda")
    OF.decode_sample(t.cuda(), torch.tensor(p).cuda(), seed_t, seq, lens_t,
                     pads, token, top_k, seed < 0, u)
    ctl = [[lens[b], L, top_k, seed, b] for b in range(B)]
    got = _sample_slots(t, [p] * B, ctl, st, "cuda", OF.decode_sample_slots)
    for a, b_, name in zip(got, (seq, pads, token, u),
                           ("seq", "pads", "token", "u_out")):
        assert torch.equal(a, b_.cpu()), name
    assert got[4].tolist() == [p + 1] * B


PER_ROW = dict(
    pos=[0, 1, 2, 5, 9, 30, 0, -1],
    seed=[11, 11, 12, 2 ** 63 - 1, -1, 0, 11, 11],
    stream=[0, 1, 0, 3, 2, 7, 0, 1],
    len=[0, 0, 0, 8, 0, 0, 0, 0],
    limit=[32, 32, 4, 32, 32, 32, 32, 32],
)


def _per_row_ctl(V):
    top_k = [0, 1, 3, min(25, V), 0, 2, min(64, V), 5]
    return [[PER_ROW["len"][b], PER_ROW["limit"][b], top_k[b],
             PER_ROW["seed"][b], PER_ROW["stream"][b]] for b in range(8)]


@pytest.mark.parametrize("V", [7, 256, 1000])
def test_sample_slots_per_row_controls_match_the_reference(V):
    ctl = _per_row_ctl(V)
    pos = PER_ROW["pos"]
    st = C.state(8, L)
    for fam in C.FAMILIES:
        for draw in range(40):
            t = C.make_logits(fam, 8, V, min(25, V), draw)
            t[6] = t[0]
            want = _sample_slots(t, pos, ctl, st, "cpu",
                                 R.decode_sample_slots)
            for dtype in DTYPES:
                case = (fam, draw, dtype)
                got = _sample_slots(t.to(dtype), pos, ctl, st, "cuda",
                                    OF.decode_sample_slots)
                seq, pads, token, u, after = got
                assert torch.equal(u, want[3]), ("u_out", case)
                assert torch.equal(token, want[2]), ("token", case,
                                                     token, want[2])
                assert torch.equal(seq, want[0]), ("seq", case)
                assert torch.equal(pads, want[1]), ("pads", case)
                assert after.tolist() == [1, 2, -1, 6, 10, -1, 1, -1], case
                assert after.tolist() == want[4].tolist()
                # row 3 is still inside its prime: the token stays
                assert int(seq[3, 6]) == 7 and int(token[3]) == 7
                assert float(u[3].min()) >= 0.0     # it drew all the same
                # row 4 is greedy and row 7 idle: neither drew
                assert float(u[4].max()) == -1.0
                assert float(u[7].max()) == -1.0
                assert torch.equal(seq[7], st[1][7]) and int(token[7]) == -1 \
                    and int(pads[7]) == 0
                # rows 0 and 6: same logits, seed, stream and position
                assert torch.equal(u[0], u[6])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_a_greedy_row_that_samples_its_second_pad_retires(dtype):
    V = 256
    t = C.make_logits("normal", 2, V, 0, 3)
    t[:, 0] = 39.0                       # token 0 wins
    st = C.state(2, L)
    st[3] = torch.tensor([1, 0])         # pads
    ctl = [[0, L, 0, -1, 0], [0, L, 0, -1, 0]]
    seq, pads, token, _u, pos = _sample_slots(
        t.to(dtype), [4, 4], ctl, st, "cuda", OF.decode_sample_slots)
    assert token.tolist() == [0, 0] and seq[:, 5].tolist() == [0, 0]
    assert pads.tolist() == [2, 1] and pos.tolist() == [-1, 5]


# ---- the engine --------------------------------------------------------------

def _model():
    from progen_amd import ProGenBase, ProGenConfig
    cfg = ProGenConfig(num_tokens=256, dim=256, depth=3, heads=4,
                       dim_head=64, window_size=64, seq_len=256,
                       ff_glu=False, global_mlp_depth=1)
    torch.manual_seed(3)
    m = ProGenBase(cfg).to(device="cuda", dtype=torch.bfloat16).eval()
    m.rotary_sin = m.rotary_sin.float()
    m.rotary_cos = m.rotary_cos.float()
    return m


def _primes():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(1, 256, (n,), generator=g) for n in (9, 5, 2, 12)]


FAST = dict(graph=True, fused=True, fused_linear=True, device_sampling=True)
LENGTH = 64


@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
def test_engine_full_request_equals_sample_cached_batch(graph):
    from progen_amd.decode import sample_cached_batch
    from progen_amd.engine import SlotEngine
    m = _model()
    engine = SlotEngine(m, 4, graph=graph, fused_linear=True)
    for top_k, seed in ((None, None), (25, 13)):
        want = sample_cached_batch(m, _primes(), LENGTH, top_k=top_k,
                                   seed=seed, **FAST)
        ticket = engine.submit(_primes(), LENGTH, top_k=top_k, seed=seed)
        engine.run_until_idle()
        assert ticket.slots == [0, 1, 2, 3]
        assert torch.equal(ticket.wait(), want), (top_k, seed)


def _staggered(m, graph, check_every):
    from progen_amd.engine import SlotEngine
    engine = SlotEngine(m, 2, graph=graph, fused_linear=True,
                        check_every=check_every)
    tickets = [engine.submit([p], n)
               for p, n in zip(_primes()[:3], (24, 40, 32))]
    engine.run_until_idle()
    return tickets


@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
def test_engine_staggered_requests_reuse_a_slot(graph):
    from progen_amd.decode import sample_cached_batch
    m = _model()
    tickets = _staggered(m, graph, 16)
    assert [t.slots for t in tickets] == [[0], [1], [0]]
    filler = _primes()[3]
    for t, p, n in zip(tickets, _primes()[:3], (24, 40, 32)):
        # the same batch size, with the request in the row it ran in
        rows = [filler, filler]
        rows[t.slots[0]] = p
        want = sample_cached_batch(m, rows, n, **FAST)[t.slots[0]]
        assert torch.equal(t.wait()[0], want), (t.slots, n)
    every_step = _staggered(m, graph, 1)
    for a, b in zip(tickets, every_step):
        assert torch.equal(a.wait(), b.wait()), "check_every 1 vs 16"
