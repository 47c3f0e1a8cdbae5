"""Time the decode linear kernel against F.linear (+ GLU/GELU kernel) on
the flagship's eight projection shapes (bf16).

Each arm of each shape is captured in a hipGraph and replayed back to
back, timed with device events around the replays, so the figure holds the
kernel and its dependent-launch boundary, not the host. In the decode step
a weight is read once per token between 2.4 GB of others, so the graph
holds one call on each of enough copies of the weight (at least 640 MB, at
most 256 copies) that a replay does not find them in the 256 MB last-level
cache. Reports us per call and algorithmic bytes/s (weight + bias + x +
out, each once) for both arms.

Usage (GPU box):  python tools/bench_decode_linear.py [--batch 1] [--replays 20] [--rounds 3]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from progen_amd.ops import functional as OF

# (K, N, act, bias, where the flagship has it)
SHAPES = [
    (1536, 4608, "none", False, "to_qkv"),
    (1536, 1536, "none", True, "to_out"),
    (1536, 12288, "glu", True, "proj_in (GLU)"),
    (1536, 6144, "gelu", True, "proj_in (SGU layer)"),
    (3072, 3072, "none", True, "sgu.proj_out"),
    (6144, 1536, "none", True, "proj_out (GLU)"),
    (3072, 1536, "none", True, "proj_out (SGU layer)"),
    (1536, 256, "none", True, "to_logits"),
]


def torch_one(x, w, b, act):
    h = F.linear(x, w, b)
    if act == "glu":
        return OF.glu_gelu(h)
    return OF.gelu(h) if act == "gelu" else h


def over_copies(one):
    def fn(x, ws, b, act):
        return [one(x, w, b, act) for w in ws][-1]
    return fn


def graph_of(fn, *args):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn(*args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn(*args)
    return g, out


def time_us(g, replays):
    for _ in range(10):
        g.replay()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(replays):
        g.replay()
    end.record()
    torch.cuda.synchronize()
    return 1e3 * start.elapsed_time(end) / replays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    B = args.batch
    # measure the kernel at every batch it accepts, whatever the routing
    # limit of the decode step is set to
    OF.DEC_LINEAR_MAX_B = OF.DEC_LINEAR_KERNEL_MAX_B
    torch.manual_seed(0)
    print(f"decode_linear bench, batch {B}, bf16, {args.rounds} interleaved "
          f"rounds of {args.replays} graph replays")
    for K, N, act, bias, name in SHAPES:
        assert OF.decode_linear_supported(B, K, N, act, torch.bfloat16), \
            "shape does not route to the kernel"
        x = torch.randn(B, K, device="cuda").bfloat16()
        w = (torch.randn(N, K, device="cuda") * K ** -0.5).bfloat16()
        copies = max(1, min(256, -(-640_000_000 // (2 * N * K))))
        ws = [w.clone() for _ in range(copies)]
        b = torch.randn(N, device="cuda").bfloat16() if bias else None
        gk, ok = graph_of(over_copies(OF.decode_linear), x, ws, b, act)
        gt, ot = graph_of(over_copies(torch_one), x, ws, b, act)
        n_out = N // 2 if act == "glu" else N
        nbytes = 2 * (N * K + (N if bias else 0) + B * K + B * n_out)
        tk, tt = [], []
        for _ in range(args.rounds):
            tk.append(time_us(gk, args.replays) / copies)
            tt.append(time_us(gt, args.replays) / copies)
        # the captured outputs hold values only once the graphs have run
        err = ((ok.float() - ot.float()).abs().max() /
               ot.float().abs().max()).item()
        fk = " ".join(f"{t:.2f}" for t in tk)
        ft = " ".join(f"{t:.2f}" for t in tt)
        print(f"K={K} N={N} act={act} bias={int(bias)} [{name}] "
              f"{nbytes / 1e6:.2f} MB x {copies} copies | kernel us: {fk} "
              f"({nbytes / min(tk) / 1e6:.2f} TB/s best) | "
              f"F.linear us: {ft} ({nbytes / min(tt) / 1e6:.2f} TB/s best) | "
              f"max diff / max {err:.1e}")


if __name__ == "__main__":
    main()
