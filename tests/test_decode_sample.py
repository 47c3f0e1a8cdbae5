"""Device sampling on the CPU: the Philox stream, ``reference.decode_sample``
against the host sampler it has to reproduce, and the decode loop with
``device_sampling=True`` (where the reference runs in place of the HIP
kernel of progen_amd/ops/hip/decode_sample.hip)."""

import numpy as np
import pytest
import torch

import decode_sample_cases as C
from progen_amd import decode
from progen_amd.config import ProGenConfig
from progen_amd.models.progen import ProGenBase
from progen_amd.ops import functional as OF
from progen_amd.ops import reference as R

VS = (2, 255, 256, 320, 1024)
KS = (0, 1, 2, 25, "V")
MUTANTS = ("kth_included", "excluded_neg_inf", "noise_unmasked",
           "ties_to_last")


def _hex(s):
    return [int(x, 16) for x in s.split()]


# ---- Philox ---------------------------------------------------------------

@pytest.mark.parametrize("counter,key,want", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000",
     "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff",
     "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0",
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    out = R.philox4x32_10(np.array(_hex(counter)), np.array(_hex(key)))
    assert [int(x) for x in out] == _hex(want)


def test_uniform_layout_is_counter_j_w_b_and_word_i_is_index_4j_plus_i():
    seed, w, B, V = (5 << 32) | 9, 11, 3, 10
    u = R.decode_sample_uniform(seed, w, B, V)
    assert u.shape == (B, V) and u.dtype == torch.float32
    for b in range(B):
        for j in range(3):
            x = R.philox4x32_10(np.array([j, w, b, 0]), np.array([9, 5]))
            for i in range(4):
                if 4 * j + i < V:
                    assert float(u[b, 4 * j + i]) == (int(x[i]) >> 8) * 2.0 ** -24


def test_uniforms_are_in_the_unit_interval_and_streams_differ():
    u = R.decode_sample_uniform(1, 1, 4, 1024)
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert 0.45 < float(u.mean()) < 0.55
    assert not torch.equal(u[0], u[1])                              # rows
    assert not torch.equal(u, R.decode_sample_uniform(1, 2, 4, 1024))  # pos
    assert not torch.equal(u, R.decode_sample_uniform(2, 1, 4, 1024))  # seed
    assert not torch.equal(u, R.decode_sample_uniform(1 << 32, 1, 4, 1024))
    assert torch.equal(u, R.decode_sample_uniform(1, 1, 4, 1024))


# ---- the reference against select_top_k + gumbel + argmax -------------------

def _cases():
    for V in VS:
        for k in KS:
            k = V if k == "V" else k
            if k > V:
                continue
            for fam in C.FAMILIES:
                yield fam, V, k


def _reference_tokens(t, k, seed, w, greedy=False):
    B, V = t.shape
    seed_t, seq, lens, pads, token = C.state(B, w + 2, seed=seed)
    u = torch.full((B, V), -1.0)
    R.decode_sample(t, torch.tensor(w - 1), seed_t, seq, lens, pads, token,
                    k, greedy, u)
    return token, u


@pytest.fixture(scope="module")
def sampled():
    """Every case once: (family, V, k) -> (logits, u, reference tokens)."""
    out = {}
    for fam, V, k in _cases():
        t = C.make_logits(fam, 4, V, k, seed=1)
        token, u = _reference_tokens(t, k, seed=1, w=3)
        out[fam, V, k] = (t, u, token)
    return out


def test_reference_equals_the_host_sampler_on_the_same_uniforms(sampled):
    for (fam, V, k), (t, u, token) in sampled.items():
        assert torch.equal(u, R.decode_sample_uniform(1, 3, 4, V))
        want = C.first_argmax(C.host_scores(t, u, k))
        assert torch.equal(token, want), (fam, V, k, token, want)


def test_k_equal_one_selects_nothing_and_gives_the_first_index(sampled):
    for (fam, V, k), (_t, _u, token) in sampled.items():
        if k == 1:
            assert token.tolist() == [0] * 4, (fam, V)


def test_all_selected_scores_negative_gives_the_first_excluded_index(sampled):
    for (fam, V, k), (t, _u, token) in sampled.items():
        if fam != "negative" or k == 0:
            continue
        mask, _ = R.select_top_k(t, k)
        first_excluded = (~mask).float().argmax(dim=-1)
        assert torch.equal(token, first_excluded), (V, k)


def test_ties_at_the_threshold_select_fewer_than_k(sampled):
    for (fam, V, k), (t, _u, _tok) in sampled.items():
        if fam == "ties" and k >= 1 and V >= 4:
            kth = t.topk(k, dim=-1).values[:, -1:]
            # k = V: the threshold is the smallest entry, tied with one more
            assert int((t == kth).sum(dim=-1).min()) >= (2 if k == V else 3), \
                (V, k)
            mask, _ = R.select_top_k(t, k)
            assert int(mask.sum(dim=-1).max()) < k, (V, k)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_inputs_tell_each_mutant_from_the_reference(sampled, mutant):
    changed = 0
    for (fam, V, k), (t, u, token) in sampled.items():
        got = C.first_argmax(C.host_scores(t, u, k, mutant=mutant), mutant)
        changed += int((got != token).sum())
    assert changed > 0, mutant


def test_greedy_is_the_first_argmax_without_noise_or_mask():
    t = C.make_logits("ties", 4, 320, 1, seed=2)
    token, u = _reference_tokens(t, 25, seed=1, w=3, greedy=True)
    assert torch.equal(token, t.argmax(dim=-1))
    assert float(u.min()) == -1.0      # no uniforms drawn, u_out untouched


def test_bf16_logits_are_read_as_their_fp32_values():
    t = C.make_logits("normal", 3, 255, 3, seed=3)
    a, _ = _reference_tokens(t, 3, seed=4, w=2)
    b, _ = _reference_tokens(t.bfloat16(), 3, seed=4, w=2)
    assert torch.equal(a, b)


# ---- in-place effects -----------------------------------------------------

def test_prime_override_and_pad_counting():
    # row 0 samples; row 1 keeps a prime token; row 2 keeps a prime 0 (a
    # pad); row 3 samples a 0 (k = 1 always gives index 0)
    t = C.make_logits("normal", 4, 256, 1, seed=5)
    t[0, 17] = 39.0
    t[:3, 0] = -39.0
    seed_t, seq, lens, pads, token = C.state(4, 8, lens=[2, 5, 5, 0])
    seq[2, 3] = 0
    pads[:] = torch.tensor([0, 1, 0, 1])
    R.decode_sample(t, torch.tensor(2), seed_t, seq, lens, pads, token, 0,
                    True)
    assert seq[:, 3].tolist() == [17, 7, 0, int(t[3].argmax())]
    assert token.tolist() == seq[:, 3].tolist()
    assert pads.tolist() == [0, 1, 1, 1 + int(t[3].argmax() == 0)]
    other = torch.ones(4, 8, dtype=torch.bool)
    other[:, 3] = False
    assert (seq[other] == 7).all()
    R.decode_sample(t, torch.tensor(3), seed_t, seq, lens, pads, token, 1,
                    False)
    assert seq[:, 4].tolist() == [0, 7, 7, 0]      # lens = 5 covers w = 4
    assert pads.tolist()[0] == 1 and pads.tolist()[1:3] == [1, 1]


@pytest.mark.parametrize("pos,touched", [(-1, False), (5, True), (6, False),
                                         (7, False)])
def test_position_guard(pos, touched):
    """L = 7: w = L - 1 (pos 5) is the last position written; pos -1 and
    w >= L leave every tensor as it was."""
    t = C.make_logits("normal", 2, 256, 25, seed=6)
    seed_t, seq, lens, pads, token = C.state(2, 7)
    u = torch.full((2, 256), -1.0)
    before = [x.clone() for x in (seq, lens, pads, token, u)]
    OF.decode_sample(t, torch.tensor(pos), seed_t, seq, lens, pads, token,
                     25, False, u)
    same = all(torch.equal(a, b)
               for a, b in zip(before, (seq, lens, pads, token, u)))
    assert same == (not touched)
    if touched:
        assert (token >= 0).all() and torch.equal(seq[:, 6], token)


# ---- the decode loop ------------------------------------------------------

def _tiny():
    torch.manual_seed(7)
    cfg = ProGenConfig(num_tokens=256, dim=16, depth=3, dim_head=8, heads=2,
                       window_size=8, seq_len=48, global_mlp_depth=1)
    return ProGenBase(cfg).eval()


def _primes():
    g = torch.Generator().manual_seed(3)
    return [torch.randint(1, 256, (n,), generator=g) for n in (9, 4, 1)]


@pytest.mark.parametrize("fused,fused_linear", [(False, False), (True, False),
                                                (True, True)])
def test_greedy_device_sampling_equals_the_host_loop(fused, fused_linear):
    m = _tiny()
    want = decode.sample_cached_batch(m, _primes(), 40)
    got = decode.sample_cached_batch(m, _primes(), 40, fused=fused,
                                     fused_linear=fused_linear,
                                     device_sampling=True)
    assert torch.equal(got, want)
    assert all(torch.equal(got[i, :len(p)], p)
               for i, p in enumerate(_primes()))


def _hand_loop(m, primes, length, top_k, seed):
    B = len(primes)
    seq = torch.zeros(B, length, dtype=torch.long)
    for i, p in enumerate(primes):
        seq[i, :len(p)] = p
    lens = torch.tensor([len(p) for p in primes])
    pads = (seq[:, 0] == 0).long()
    token = seq[:, 0].clone()
    seed_t = torch.tensor([seed])
    cache = decode.DecodeCache(m, batch=B)
    for p in range(length - 1):
        logits = decode.forward_step(m, token, cache)
        R.decode_sample(logits, torch.tensor(p), seed_t, seq, lens, pads,
                        token, top_k, False)
    return seq * (~((seq == 0).long().cumsum(dim=-1) > 1)).long()


def test_stochastic_run_equals_a_hand_written_loop_over_the_reference():
    m = _tiny()
    want = _hand_loop(m, _primes(), 40, 25, seed=11)
    got = decode.sample_cached_batch(m, _primes(), 40, top_k=25,
                                     device_sampling=True, seed=11)
    assert torch.equal(got, want)
    # no top-k: gumbel-max over the whole row
    want = _hand_loop(m, _primes(), 40, 0, seed=11)
    got = decode.sample_cached_batch(m, _primes(), 40, device_sampling=True,
                                     seed=11)
    assert torch.equal(got, want)


def test_output_does_not_depend_on_check_every_and_stops_early(monkeypatch):
    m = _tiny()
    # BOS-primed rows and k = 1 (token 0 every step): every row has its
    # second pad after one step
    primes = [torch.tensor([0, 5, 6]), torch.tensor([0])]
    steps = {}
    real = decode.forward_step

    def counting(*a, **k):
        steps["n"] = steps.get("n", 0) + 1
        return real(*a, **k)
    monkeypatch.setattr(decode, "forward_step", counting)
    outs = []
    for ce in (1, 16, 40):
        steps["n"] = 0
        outs.append(decode.sample_cached_batch(
            m, primes, 40, top_k=1, device_sampling=True, seed=2,
            check_every=ce))
        # done after 3 steps; the host sees it at its next look
        assert steps["n"] == {1: 3, 16: 16, 40: 39}[ce], ce
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert outs[0][0].tolist() == [0, 5, 6] + [0] * 37
    # and on a run that samples real tokens
    outs = [decode.sample_cached_batch(m, _primes(), 40, top_k=25,
                                       device_sampling=True, seed=5,
                                       check_every=ce) for ce in (1, 16, 40)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_same_seed_same_output_another_seed_differs():
    m = _tiny()
    a = decode.sample_cached_batch(m, _primes(), 40, top_k=25,
                                   device_sampling=True, seed=1)
    b = decode.sample_cached_batch(m, _primes(), 40, top_k=25,
                                   device_sampling=True, seed=1)
    c = decode.sample_cached_batch(m, _primes(), 40, top_k=25,
                                   device_sampling=True, seed=2)
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_top_k_without_a_seed_draws_one_from_the_global_generator():
    m = _tiny()
    torch.manual_seed(21)
    a = decode.sample_cached_batch(m, _primes(), 40, top_k=25,
                                   device_sampling=True)
    torch.manual_seed(21)
    b = decode.sample_cached_batch(m, _primes(), 40, top_k=25,
                                   device_sampling=True)
    assert torch.equal(a, b)
    assert not torch.equal(
        a, decode.sample_cached_batch(m, _primes(), 40, device_sampling=True))


def test_arguments_are_checked():
    m = _tiny()
    g = torch.Generator().manual_seed(0)
    with pytest.raises(ValueError, match="generator"):
        decode.sample_cached_batch(m, _primes(), 40, generator=g,
                                   device_sampling=True)
    with pytest.raises(ValueError, match="generator"):
        decode.sample_cached(m, _primes()[0], 40, generator=g,
                             device_sampling=True)
    for bad in (-1, 2 ** 63):
        with pytest.raises(ValueError, match="seed"):
            decode.sample_cached_batch(m, _primes(), 40, seed=bad,
                                       device_sampling=True)
    with pytest.raises(ValueError, match="check_every"):
        decode.sample_cached_batch(m, _primes(), 40, device_sampling=True,
                                   check_every=0)
    with pytest.raises(ValueError, match="device_sampling"):
        decode.sample_cached_batch(m, _primes(), 40, seed=1)
    assert decode.sample_cached_batch(
        m, _primes(), 40, seed=2 ** 63 - 1, device_sampling=True).shape == (3, 40)


def test_sample_cached_delegates_to_row_zero_of_the_batch():
    m = _tiny()
    prime = _primes()[0]
    want = decode.sample_cached_batch(m, [prime], 40, top_k=25,
                                      device_sampling=True, seed=9)[0]
    got = decode.sample_cached(m, prime, 40, top_k=25, device_sampling=True,
                               seed=9)
    assert torch.equal(got, want)
    bos = torch.cat((torch.zeros(1, dtype=torch.long), prime))
    want = decode.sample_cached_batch(m, [bos], 40, top_k=25,
                                      device_sampling=True, seed=9)[0]
    got = decode.sample_cached(m, prime, 40, top_k=25, add_bos=True,
                               device_sampling=True, seed=9)
    assert torch.equal(got, want)
    assert got[0] == 0 and torch.equal(got[1:10], prime)
    # no top-k, no seed: greedy, the host batch decoder's own greedy output
    assert torch.equal(
        decode.sample_cached(m, prime, 40, add_bos=True, device_sampling=True),
        decode.sample_cached_batch(m, [bos], 40)[0])


def test_cli_flags():
    from click.testing import CliRunner
    import sample
    import serve
    r = CliRunner().invoke(sample.main, ["--device-sampling"])
    assert r.exit_code == 2 and "--device-sampling needs --cached" in r.output
    for cmd in (sample.main, serve.main):
        assert any("--device-sampling" in p.opts for p in cmd.params)
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                        "tools", "bench_decode.py")
    spec = importlib.util.spec_from_file_location("bench_decode_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse_args(["--graph", "--device-sampling", "--top-k", "25"])
    assert args.device_sampling and args.top_k == 25 and args.check_every == 16
    off = mod.parse_args(["--top-k", "25"])
    assert not off.device_sampling and off.top_k == 25   # both arms take it
    # the host arm's sampler is the host loop's: select_top_k + gumbel
    t = C.make_logits("negative", 3, 256, 25, seed=1)
    g = torch.Generator().manual_seed(4)
    got = mod.host_sample(t, 25, g)
    g = torch.Generator().manual_seed(4)
    noise = R.gumbel_noise(t.shape, generator=g)
    mask, rows = R.select_top_k(t, 25)
    assert torch.equal(got, (rows + noise * mask).argmax(dim=-1))
    assert torch.equal(mod.host_sample(t, 0, g), t.argmax(dim=-1))


def test_device_sampler_state_is_copied_from_the_host():
    # the capture itself needs a GPU (tests/test_gpu_decode_sample.py); the
    # sampler state and its host-side contract do not
    seq = torch.zeros(2, 8, dtype=torch.long)
    seq[0, :2] = torch.tensor([0, 4])
    s = decode.DeviceSampler(seq, [2, 0], 25, 3, "cpu")
    assert s.pads.tolist() == [1, 1] and s.seed.tolist() == [3]
    assert s.top_k == 25 and not s.greedy
    assert decode.DeviceSampler(seq, [2, 0], None, None, "cpu").greedy
    s.seq[0, 0] = 9
    assert seq[0, 0] == 0                      # the caller's tensor is not used
