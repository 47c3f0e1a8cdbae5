"""Measure decode latency/throughput of the cached decoder on the
FLAGSHIP ProGen-1.2B config (dim 1536, depth 36, heads 24, dh 64,
wsz 256 — the same architecture as bench.py's headline; the r01 decode
numbers were mislabeled on a different 2048/24/dh128 model, VERDICT r1
weak #8).

Modes: eager per-token step, hipGraph-captured step (--graph), batched
(--batch N), fused decode kernels (--fused, with or without --graph),
and on top of --fused the decode linear kernel (--fused-linear).
Sampling: on the host (the default: logits down, token up, every step) or
on the device (--device-sampling: the sampler runs in the step, the host
downloads the pad counts every --check-every steps); greedy, or top-k
gumbel-max with --top-k K in either arm.
Serving metric: ms/token (batch 1) and tokens/s aggregate.

With --prime-len N it measures whole requests instead, through the public
samplers (``sample_cached`` at batch 1, ``sample_cached_batch`` above): the
time from the call to the first sampled token after an N-token prime, and
the rate of tokens 2..--tokens; --prefill builds the prime's cache with one
forward (``decode.prefill``) instead of one step per prime token.

With --slots N it measures the slot engine (``progen_amd.engine``), which
always runs graph-or-eager + fused + device sampling. Alone, --slots N
compares one step of the engine's N-row batch with the scalar-position step
(``GraphedDecodeStep`` with its sampler) at the same batch and positions,
alternating the two --repeats times. With --requests M it serves M
single-prime requests of seeded ragged lengths, all waiting at time 0:
through the engine with N slots, or with --slots 0 one
``sample_cached_batch`` per request in sequence, as serve.py runs them under
its lock; it reports the wall time, generated tokens/s, the request latency
percentiles and the engine's mean slot occupancy. --slot-prefill turns on the
engine's prefill at admission (--prefill-rows, --prefill-min-tokens), and
--prime-range LO HI draws the primes from LO..HI instead of 4..64, the drawn
64..512 then counting the tokens generated after the prime.

Usage (GPU box):  python tools/bench_decode.py [--tokens 128] [--graph] [--fused [--fused-linear]] [--batch 8] [--device-sampling] [--top-k 25]
                  python tools/bench_decode.py --prime-len 512 [--prefill] --graph --fused --fused-linear [--batch 8]
                  python tools/bench_decode.py --slots 16 --graph --fused --fused-linear --device-sampling --top-k 25 [--requests 64 [--slot-prefill] [--prime-range 64 512]]
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from progen_amd import ProGenBase
from progen_amd.config import ProGenConfig
from progen_amd.decode import (DecodeCache, DeviceSampler, GraphedDecodeStep,
                               forward_step, forward_step_fused,
                               sample_cached, sample_cached_batch)
from progen_amd.engine import SlotEngine
from progen_amd.ops import reference as R


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--fused", action="store_true",
                    help="step on the fused decode kernels")
    ap.add_argument("--fused-linear", action="store_true",
                    help="with --fused: projections on the decode linear "
                         "kernel")
    ap.add_argument("--device-sampling", action="store_true",
                    help="sample in the step, on the device; the host only "
                         "downloads the pad counts")
    ap.add_argument("--top-k", type=int, default=0,
                    help="top-k gumbel-max sampling in either arm "
                         "(0: greedy argmax)")
    ap.add_argument("--check-every", type=int, default=16,
                    help="with --device-sampling: steps between pad-count "
                         "downloads")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--prime-len", type=int, default=0,
                    help="measure whole requests with a prime of this many "
                         "tokens: time to the first sampled token, then the "
                         "rate of tokens 2..--tokens (0: the step benchmark)")
    ap.add_argument("--prefill", action="store_true",
                    help="with --prime-len: one forward over the prime "
                         "instead of one decode step per prime token")
    ap.add_argument("--repeats", type=int, default=5,
                    help="with --prime-len: timed requests of each kind; "
                         "the median is reported")
    ap.add_argument("--slots", type=int, default=None,
                    help="measure the slot engine with this many slots: its "
                         "step against the scalar step, or with --requests "
                         "a workload (0: the workload one request at a time)")
    ap.add_argument("--requests", type=int, default=0,
                    help="with --slots: serve this many single-prime requests "
                         "of seeded prime lengths 4..64 and lengths 64..512")
    ap.add_argument("--slot-prefill", action="store_true",
                    help="with --slots N >= 1: the engine prefills a prime "
                         "at admission instead of teacher-forcing it")
    ap.add_argument("--prefill-rows", type=int, default=1,
                    help="with --slot-prefill: primes per prefill forward")
    ap.add_argument("--prefill-min-tokens", type=int, default=None,
                    help="with --slot-prefill: fewest prime positions worth "
                         "a forward (default: the engine's)")
    ap.add_argument("--prime-range", type=int, nargs=2, default=None,
                    metavar=("LO", "HI"),
                    help="with --requests: prime lengths LO..HI instead of "
                         "4..64; the drawn 64..512 is then the number of "
                         "tokens after the prime, cut at seq_len")
    args = ap.parse_args(argv)
    if args.slot_prefill and not args.slots:
        ap.error("--slot-prefill needs --slots N >= 1")
    if args.prime_range is not None and (
            not args.requests or
            not 1 <= args.prime_range[0] <= args.prime_range[1]):
        ap.error("--prime-range needs --requests and 1 <= LO <= HI")
    if args.slots is not None:
        if not (args.fused and args.device_sampling) or args.prefill \
                or args.prime_len:
            ap.error("--slots needs --fused and --device-sampling, and "
                     "takes neither --prefill nor --prime-len")
        if args.slots < 0 or (args.slots == 0 and not args.requests):
            ap.error("--slots must be >= 1, or 0 with --requests")
    elif args.requests:
        ap.error("--requests needs --slots")
    if args.prefill and not args.prime_len:
        ap.error("--prefill needs --prime-len")
    if args.prime_len < 0 or args.repeats < 1:
        ap.error("--prime-len must be >= 0 and --repeats >= 1")
    if args.fused_linear and not args.fused:
        ap.error("--fused-linear needs --fused")
    if args.top_k < 0 or args.check_every < 1:
        ap.error("--top-k must be >= 0 and --check-every >= 1")
    return args


def host_sample(logits, top_k, gen):
    """The host arm's sampler, as decode.sample_cached_batch runs it: the
    logits come down, no device kernel runs."""
    rows = logits.cpu().float()
    if not top_k:
        return rows.argmax(dim=-1)
    noise = R.gumbel_noise(rows.shape, generator=gen)
    mask, rows = R.select_top_k(rows, top_k)
    return (rows + noise * mask).argmax(dim=-1)


def flagship():
    # flagship ProGen-1.2B (configs/model/progen_1b.toml)
    cfg = ProGenConfig(num_tokens=256, dim=1536, depth=36, heads=24,
                       dim_head=64, window_size=256, seq_len=1024,
                       global_mlp_depth=2)
    torch.manual_seed(0)
    m = ProGenBase(cfg).to(device="cuda", dtype=torch.bfloat16).eval()
    m.rotary_sin = m.rotary_sin.float()
    m.rotary_cos = m.rotary_cos.float()
    return m


def run(m, args):
    """One measurement on the model ``m``; returns ms per step."""
    B = args.batch
    cache = DecodeCache(m, batch=B)
    tok = torch.randint(1, 256, (B,), device="cuda")
    gen = torch.Generator().manual_seed(args.seed)

    if args.device_sampling:
        mode, t0 = _run_device_sampling(m, args, cache, tok)
    elif args.graph:
        # a couple of eager steps as prefill, then capture
        for _ in range(2):
            logits = forward_step(m, tok, cache)
            tok = logits.argmax(dim=-1)
        tok = tok.cpu()
        g = GraphedDecodeStep(m, cache, start_pos=cache.pos,
                              fused=args.fused,
                              fused_linear=args.fused_linear)
        # pure-replay rule: sampling runs on the HOST (memcpys only
        # between replays — an eager device argmax kernel between them
        # would poison replay; --device-sampling puts the sampler INSIDE
        # the graph instead)
        for _ in range(args.warmup):
            tok = host_sample(g.step(tok), args.top_k, gen)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.tokens):
            tok = host_sample(g.step(tok), args.top_k, gen)
        torch.cuda.synchronize()
        mode = "graphed"
    else:
        if args.fused:
            pos_dev = torch.zeros((), dtype=torch.long, device="cuda")

            def step(tok):
                logits = forward_step_fused(m, tok, cache, pos_dev,
                                            fused_linear=args.fused_linear)
                pos_dev.add_(1)
                cache.pos += 1
                return logits
        else:
            def step(tok):
                return forward_step(m, tok, cache)
        if args.top_k:
            def pick(logits):
                return host_sample(logits, args.top_k, gen).cuda()
        else:
            def pick(logits):
                return logits.argmax(dim=-1)
        for _ in range(args.warmup):
            tok = pick(step(tok))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.tokens):
            tok = pick(step(tok))
        torch.cuda.synchronize()
        mode = "eager"
    if args.fused:
        mode += "+fused"
    if args.fused_linear:
        mode += "+linear"
    if args.device_sampling:
        mode += f"+devsample/{args.check_every}"
    if args.top_k:
        mode += f"+top{args.top_k}"
    dt = time.perf_counter() - t0
    n = args.tokens * B
    print(f"decode[{mode}, batch {B}]: {args.tokens} steps in {dt:.3f}s -> "
          f"{n / dt:.1f} tok/s aggregate, {1e3 * dt / args.tokens:.2f} ms/step "
          f"(ProGen-1.2B flagship config, bf16, cached)")
    return 1e3 * dt / args.tokens


def _run_device_sampling(m, args, cache, tok):
    """The --device-sampling arm: warm-up and timed steps with the sampler
    in the step; returns (mode, t0) with the clock started after warm-up.
    Rows never finish early here (the loop is timed to --tokens steps
    whatever is sampled): the pad counts are downloaded, not acted on."""
    B = args.batch
    total = args.warmup + args.tokens
    if 2 + total >= m.cfg.seq_len:
        raise SystemExit("--warmup + --tokens must stay below seq_len - 2")
    seq = torch.zeros(B, m.cfg.seq_len, dtype=torch.long)
    for p in range(2):  # a couple of eager steps as prefill
        seq[:, p] = tok.cpu()
        tok = forward_step(m, tok, cache).argmax(dim=-1)
    seq[:, 2] = tok.cpu()
    sampler = DeviceSampler(seq, [3] * B, args.top_k or None,
                            args.seed if args.top_k else None, "cuda")
    if args.graph:
        g = GraphedDecodeStep(m, cache, start_pos=cache.pos, fused=args.fused,
                              fused_linear=args.fused_linear, sampler=sampler)
        g.token.copy_(tok.cpu())
        run_steps = g.replay
        mode = "graphed"
    else:
        token = tok.clone()
        pos_dev = torch.full((), cache.pos, dtype=torch.long, device="cuda")

        def run_steps(n):
            for _ in range(n):
                if args.fused:
                    logits = forward_step_fused(
                        m, token, cache, pos_dev,
                        fused_linear=args.fused_linear)
                    cache.pos += 1
                else:
                    logits = forward_step(m, token, cache)
                sampler.sample(logits, pos_dev, token)
                pos_dev.add_(1)
        mode = "eager"

    def chunks(n):
        done = 0
        while done < n:
            c = min(args.check_every, n - done)
            run_steps(c)
            done += c
            sampler.pads.cpu()  # the loop's only download

    chunks(args.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    chunks(args.tokens)
    torch.cuda.synchronize()
    return mode, t0


def run_prime(m, args):
    """Whole requests with an ``args.prime_len``-token prime, as the samplers
    serve them: returns (median ms to the first sampled token, median ms per
    token for tokens 2..--tokens). A request for one token ends when that
    token is on the host; one for --tokens tokens adds the decode steps, and
    the difference of the two is their time. With --graph both include the
    capture of the step."""
    B, N = args.batch, args.prime_len
    if N + args.tokens > m.cfg.seq_len or args.tokens < 2:
        raise SystemExit("--prime-len + --tokens must stay within seq_len "
                         "and --tokens above 1")
    with torch.no_grad():
        # a request that samples its second pad ends early: rule token 0 out
        m.to_logits.bias[0] = -1e4
    g = torch.Generator().manual_seed(args.seed)
    primes = torch.randint(1, 256, (B, N), generator=g)
    kw = dict(graph=args.graph, fused=args.fused,
              fused_linear=args.fused_linear, prefill=args.prefill,
              top_k=args.top_k or None)
    if args.device_sampling:
        kw.update(device_sampling=True, check_every=args.check_every,
                  seed=args.seed if args.top_k else None)

    def request(length):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if B == 1:
            out = sample_cached(m, primes[0], length, **kw)
        else:
            out = sample_cached_batch(m, list(primes), length, **kw)
        torch.cuda.synchronize()
        assert bool((out[..., :length] != 0).all()), "a request ended early"
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(max(1, min(args.warmup, 2))):    # every shape, both kinds
        request(N + 1)
        request(N + args.tokens)
    first, rest = [], []
    for _ in range(args.repeats):
        t1 = request(N + 1)
        tn = request(N + args.tokens)
        first.append(t1)
        rest.append((tn - t1) / (args.tokens - 1))
    ttft, per_tok = statistics.median(first), statistics.median(rest)
    mode = ("graphed" if args.graph else "eager") + \
        ("+fused" if args.fused else "") + \
        ("+linear" if args.fused_linear else "") + \
        ("+devsample" if args.device_sampling else "") + \
        ("+prefill" if args.prefill else "")
    print(f"request[{mode}, batch {B}, prime {N}]: first token after "
          f"{ttft:.1f} ms (min {min(first):.1f}, max {max(first):.1f}), "
          f"tokens 2..{args.tokens} at {per_tok:.2f} ms/token "
          f"(median of {args.repeats}; ProGen-1.2B flagship config, bf16)")
    return ttft, per_tok


def _spread(xs):
    return (f"median {statistics.median(xs):.3f}, min {min(xs):.3f}, "
            f"max {max(xs):.3f}")


def run_slot_step(m, args):
    """The slot step against the scalar-position step at batch --slots, all
    rows active at equal positions, the two alternating --repeats times on
    the same model; returns (scalar, slot) median ms per step. A timed block
    is --tokens steps with a download every --check-every steps in both arms:
    the scalar loop's pad counts, the engine's positions."""
    B, T = args.slots, args.tokens
    if 3 + args.warmup + T * args.repeats >= m.cfg.seq_len:
        raise SystemExit("--warmup + --tokens * --repeats must stay below "
                         "seq_len - 3")
    with torch.no_grad():
        m.to_logits.bias[0] = -1e4   # no row may finish early
    g = torch.Generator().manual_seed(args.seed)
    primes = torch.randint(1, 256, (B, 3), generator=g)
    seed = args.seed if args.top_k else None

    # scalar arm: as sample_cached_batch builds it, stepped from position 0
    # through the prime like the engine's rows
    seq = torch.zeros(B, m.cfg.seq_len, dtype=torch.long)
    seq[:, :3] = primes
    cache = DecodeCache(m, batch=B)
    sampler = DeviceSampler(seq, [3] * B, args.top_k or None, seed, "cuda")
    if args.graph:
        graphed = GraphedDecodeStep(m, cache, start_pos=0, fused=True,
                                    fused_linear=args.fused_linear,
                                    sampler=sampler)
        graphed.token.copy_(seq[:, 0].contiguous())
        scalar_steps = graphed.replay
    else:
        token = seq[:, 0].contiguous().cuda()
        pos_dev = torch.zeros((), dtype=torch.long).cuda()

        def scalar_steps(n):
            for _ in range(n):
                logits = forward_step_fused(m, token, cache, pos_dev,
                                            fused_linear=args.fused_linear)
                sampler.sample(logits, pos_dev, token)
                pos_dev.add_(1)

    def scalar_block(n):
        done = 0
        while done < n:
            c = min(args.check_every, n - done)
            scalar_steps(c)
            done += c
            sampler.pads.cpu()
        return done

    engine = SlotEngine(m, B, graph=args.graph,
                        fused_linear=args.fused_linear,
                        check_every=args.check_every)
    engine.submit(list(primes), m.cfg.seq_len, top_k=args.top_k or None,
                  seed=seed)

    def slot_block(n):
        # whole engine cycles: up to check_every - 1 steps more than n
        start = engine.steps
        while engine.steps - start < n:
            engine.cycle()
        return engine.steps - start

    def timed(block, n):
        """ms per step over the steps the block really ran."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ran = block(n)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / ran

    scalar_block(args.warmup)
    slot_block(args.warmup)
    scalar, slot = [], []
    for _ in range(args.repeats):
        scalar.append(timed(scalar_block, T))
        slot.append(timed(slot_block, T))
    mode = ("graphed" if args.graph else "eager") + "+fused" + \
        ("+linear" if args.fused_linear else "") + \
        f"+devsample/{args.check_every}" + \
        (f"+top{args.top_k}" if args.top_k else "")
    print(f"step[{mode}, batch {B}] scalar position: {_spread(scalar)} "
          f"ms/step; slot positions: {_spread(slot)} ms/step "
          f"({args.repeats} alternating blocks of {T} steps; ProGen-1.2B "
          "flagship config, bf16)")
    return statistics.median(scalar), statistics.median(slot)


def slot_workload(args, seq_len):
    """The --requests workload: (prime, length) per request, seeded. Prime
    lengths 4..64, lengths 64..512 and never past seq_len. With
    --prime-range LO HI the primes have LO..HI tokens (below seq_len) and the
    drawn 64..512 counts the tokens after the prime."""
    g = torch.Generator().manual_seed(args.seed)
    lo, hi = args.prime_range or (4, 64)
    out = []
    for _ in range(args.requests):
        n = min(int(torch.randint(lo, hi + 1, (1,), generator=g)), seq_len - 1)
        length = int(torch.randint(64, 513, (1,), generator=g))
        if args.prime_range is not None:
            length += n
        length = max(min(length, seq_len), n + 1)
        out.append((torch.randint(1, 256, (n,), generator=g), length))
    return out


def lo_hi(args):
    return "{}..{}".format(*args.prime_range)


def run_slot_workload(m, args):
    """Serve the workload once, every request waiting at time 0; returns
    (wall seconds, generated tokens/s). ``--slots 0``: one
    ``sample_cached_batch`` per request in sequence, its cache and capture
    included, as serve.py runs them under its lock."""
    with torch.no_grad():
        m.to_logits.bias[0] = -1e4   # every request runs to its length
    work = slot_workload(args, m.cfg.seq_len)
    generated = sum(length - len(p) for p, length in work)
    top_k = args.top_k or None
    seeds = [args.seed + i for i in range(len(work))] if top_k else \
        [None] * len(work)
    latency = []
    occupancy = None
    if args.slots:
        engine = SlotEngine(m, args.slots, graph=args.graph,
                            fused_linear=args.fused_linear,
                            check_every=args.check_every,
                            prefill=args.slot_prefill,
                            prefill_rows=args.prefill_rows,
                            prefill_min_tokens=args.prefill_min_tokens)
        # the engine's one cache and capture belong to the server's start,
        # not to a request: built before the clock starts and reported apart
        # (the sequential arm pays a cache and a capture inside every request)
        torch.cuda.synchronize()
        tb = time.perf_counter()
        engine.generate([work[0][0]], len(work[0][0]) + 2, top_k=top_k,
                        seed=seeds[0])
        torch.cuda.synchronize()
        build_s = time.perf_counter() - tb
        steps0, occ0 = engine.steps, engine.occupied_slot_steps
        pf0 = engine.prefills
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tickets = [engine.submit([p], length, top_k=top_k, seed=s)
                   for (p, length), s in zip(work, seeds)]
        engine.run_until_idle()
        wall = time.perf_counter() - t0
        for t, (p, length) in zip(tickets, work):
            assert bool((t.wait() != 0).all()), "a request ended early"
            latency.append(t.finished - t0)
        occupancy = (engine.occupied_slot_steps - occ0) / \
            ((engine.steps - steps0) * args.slots)
    else:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for (p, length), s in zip(work, seeds):
            out = sample_cached_batch(
                m, [p], length, top_k=top_k, graph=args.graph, fused=True,
                fused_linear=args.fused_linear, device_sampling=True, seed=s,
                check_every=args.check_every)
            assert bool((out != 0).all()), "a request ended early"
            latency.append(time.perf_counter() - t0)
        wall = time.perf_counter() - t0
    latency.sort()
    p50 = latency[len(latency) // 2]
    p95 = latency[min(len(latency) - 1, int(0.95 * len(latency)))]
    mode = ("graphed" if args.graph else "eager") + "+fused" + \
        ("+linear" if args.fused_linear else "") + \
        (f"+top{args.top_k}" if args.top_k else "")
    arm = f"engine, {args.slots} slots" if args.slots else \
        "one request at a time"
    if args.slot_prefill:
        arm += (f", prefill at admission (rows {engine.prefill_rows}, min "
                f"{engine.prefill_min_tokens}): {engine.prefills - pf0} "
                f"forwards, {engine.steps - steps0} steps")
    elif args.slots:
        arm += f", {engine.steps - steps0} steps"
    if args.prime_range is not None:
        arm += f"; primes {lo_hi(args)}"
    occ = "" if occupancy is None else \
        (f", mean slot occupancy {occupancy:.2f}; engine build + capture + "
         f"first request {build_s:.2f} s, not in the wall time")
    print(f"workload[{mode}; {arm}]: {len(work)} requests, {generated} "
          f"generated tokens in {wall:.2f} s -> {generated / wall:.1f} tok/s, "
          f"latency p50 {p50:.2f} s p95 {p95:.2f} s{occ} "
          "(ProGen-1.2B flagship config, bf16)")
    return wall, generated / wall


def main():
    args = parse_args()
    if args.slots is not None:
        if args.requests:
            run_slot_workload(flagship(), args)
        else:
            run_slot_step(flagship(), args)
    elif args.prime_len:
        run_prime(flagship(), args)
    else:
        run(flagship(), args)


if __name__ == "__main__":
    main()
