"""Measure the slot engine's prefill at admission (``SlotEngine(prefill=True)``)
on the flagship config, bf16, graph + fused linear, top-k 25: the numbers of
profiles/engine_prefill.md.

  --ttft       time from ``submit`` to the first sampled token of a request
               admitted into an engine of --slots slots whose other slots are
               decoding, per prime length, flag off against flag on: two
               engines in one process, alternating, --repeats runs each, both
               looking at the positions after every step (check_every 1);
  --stall      what a prefilled admission costs the other slots, per bucket:
               a cycle that admits one prime of the bucket (copies, one
               replay of its prefill graph, one step, one look) against the
               cycles next to it (one step, one look);
  --workloads  tools/bench_decode.py's --requests workload at 8, 16 and 32
               slots over the prime ranges 4..64 and 64..512, flag off and
               flag on (and --prefill-rows 4 on the long range), --repeats
               runs each.

Usage (GPU box):  python tools/bench_engine_prefill.py --ttft --stall
                  python tools/bench_engine_prefill.py --workloads --repeats 3
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import bench_decode
from progen_amd import decode
from progen_amd.engine import SlotEngine

PRIMES = (8, 16, 64, 256, 512)
TOP_K = 25


def _spread(xs):
    return (f"median {statistics.median(xs):.2f}, min {min(xs):.2f}, "
            f"max {max(xs):.2f}")


def _engine(m, slots, prefill, min_tokens=1, rows=1):
    return SlotEngine(m, slots, graph=True, fused_linear=True, check_every=1,
                      prefill=prefill, prefill_rows=rows,
                      prefill_min_tokens=min_tokens)


FILLERS = {}    # engine -> tickets of its filler requests


def _top_up(engine, g, seed):
    """Keep all slots but one decoding: stepped three-token primes that run
    to seq_len."""
    live = [t for t in FILLERS.get(engine, []) if not t.done]
    for i in range(engine.slots - 1 - len(live)):
        live.append(engine.submit(
            [torch.randint(1, 256, (3,), generator=g)], engine.cfg.seq_len,
            top_k=TOP_K, seed=seed + i))
    FILLERS[engine] = live
    engine.cycle()


def _first_token_ms(engine, prime):
    """ms from submit until the request's one sampled token is on the host."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ticket = engine.submit([prime], len(prime) + 1, top_k=TOP_K, seed=1)
    while not ticket.done:
        engine.cycle()
    return 1e3 * (ticket.finished - t0)


def run_ttft(m, args):
    g = torch.Generator().manual_seed(args.seed)
    off, on = _engine(m, args.slots, False), _engine(m, args.slots, True)
    for e in (off, on):           # build, capture, and a first request each
        _top_up(e, g, 100)
        _first_token_ms(e, torch.randint(1, 256, (9,), generator=g))
    for n in PRIMES:
        prime = torch.randint(1, 256, (n,), generator=g)
        t_off, t_on = [], []
        for i in range(args.repeats):
            for e, ts in ((off, t_off), (on, t_on)):
                _top_up(e, g, 1000 * n + 10 * i)
                ts.append(_first_token_ms(e, prime))
        print(f"ttft[{args.slots} slots, prime {n}] stepped: {_spread(t_off)} "
              f"ms; prefilled: {_spread(t_on)} ms ({args.repeats} alternating "
              "runs)", flush=True)
    return on


def run_stall(m, args, engine=None):
    g = torch.Generator().manual_seed(args.seed)
    engine = engine or _engine(m, args.slots, True)
    _top_up(engine, g, 200)
    _first_token_ms(engine, torch.randint(1, 256, (9,), generator=g))

    def cycle_ms():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        engine.cycle()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    seq_len = engine.cfg.seq_len
    unit = decode._prefill_len(m, 1, "cuda")
    for np_ in range(unit, seq_len + 1, unit):
        # the most positions the bucket holds; the prime has n + 1 tokens
        n = min(np_, seq_len - 2)
        admit, plain = [], []
        for i in range(args.repeats):
            _top_up(engine, g, 300 + 10 * i)
            plain.append(cycle_ms())
            before = engine.prefills
            ticket = engine.submit(
                [torch.randint(1, 256, (n + 1,), generator=g)], n + 2,
                top_k=TOP_K, seed=2)
            admit.append(cycle_ms())
            assert engine.prefills == before + 1 and ticket.done
            plain.append(cycle_ms())
        print(f"stall[{args.slots} slots, {n} positions, bucket {np_}]: "
              f"admitting cycle {_spread(admit)} ms; plain cycle "
              f"{_spread(plain)} ms", flush=True)


def run_workloads(m, args):
    base = ["--fused", "--fused-linear", "--device-sampling", "--graph",
            "--top-k", str(TOP_K), "--requests", "64",
            "--seed", str(args.seed)]
    arms = [("short", [], []), ("short", [], ["--slot-prefill"]),
            ("long", ["--prime-range", "64", "512"], []),
            ("long", ["--prime-range", "64", "512"], ["--slot-prefill"]),
            ("long", ["--prime-range", "64", "512"],
             ["--slot-prefill", "--prefill-rows", "4"])]
    if args.min_tokens is not None:
        for _n, _r, flags in arms:
            if flags:
                flags += ["--prefill-min-tokens", str(args.min_tokens)]
    for slots in args.workload_slots:
        for _ in range(args.repeats):
            for _name, prange, flags in arms:
                a = bench_decode.parse_args(
                    base + ["--slots", str(slots)] + prange + flags)
                bench_decode.run_slot_workload(m, a)
                sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ttft", action="store_true")
    ap.add_argument("--stall", action="store_true")
    ap.add_argument("--workloads", action="store_true")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--workload-slots", type=int, nargs="+",
                    default=[8, 16, 32])
    ap.add_argument("--min-tokens", type=int, default=None,
                    help="--workloads: prefill_min_tokens of the flag-on arms")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    m = bench_decode.flagship()
    with torch.no_grad():
        m.to_logits.bias[0] = -1e4   # no request ends early
    on = run_ttft(m, args) if args.ttft else None
    if args.stall:
        run_stall(m, args, on)
    if args.workloads:
        run_workloads(m, args)


if __name__ == "__main__":
    main()
