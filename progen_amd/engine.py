"""Continuous batching for the cached decoder: one persistent decode batch
whose rows ("slots") serve different requests at different positions.

``sample_cached_batch`` decodes one request per call: its rows share one
position, a finished row computes a dead tail until the last row is done,
and every call builds its own cache and captures its own graph. The engine
keeps ONE ``DecodeCache`` of ``slots`` rows and one step — captured once
with ``graph=True`` — that advances every occupied slot at its own position
(``decode.forward_step_slots`` + ``OF.decode_sample_slots``). Requests are
admitted into free slots and retired as they finish while the other slots
keep decoding.

    engine = SlotEngine(model, slots=16, graph=True, fused_linear=True)
    engine.start()                       # one worker thread owns the GPU
    out = engine.generate([prime], 256, top_k=25, seed=7)   # any thread
    engine.close()

Per slot the device holds a position ``pos`` (-1: idle), the next input
``token``, the sequence ``seq``, the pad count ``pads`` and the sampler's
controls ``ctl = [len, limit, top_k, seed, stream]``. The sampler owns the
position advance and the retirement (pos <- -1 after the second pad or the
last position), so a finished row stops inside the same replay.

Only copies between replays (profiles/r01_graph_interleave_bug.md): admission
is five host-to-device copies into the slot's contiguous row views, ``pos``
last, and polling is a device-to-host copy of ``pos`` and of the finished
``seq`` rows. No fill, index or arithmetic kernel ever runs on the engine's
tensors outside the step and the prefill graphs below; the eager engine runs
the same code. By default a prime is teacher-forced through the step
(``len``), sharing those steps with the other slots' generation.

``prefill=True`` fills a prime's cache rows at admission instead, with one
forward over the prime (``decode.prefill_rows``), so that the first sampled
token is one step away instead of one step per prime token. Under the
copies-only rule that forward is a graph of its own, one per bucket of prime
lengths (the multiples of ``decode._prefill_len``'s unit up to seq_len) over
static (prefill_rows, Np) token buffers, all captured in ``_build`` before
anything is replayed. The slot and the row count of each batch row reach the
kernels through device memory (``admit``, ops/hip/prefill_admit.hip), as do
the places of the token-shift halos (``src``, ``live``). An admission is then
four host-to-device copies, one replay, and the five copies of a plain
admission with the slot entering at the prime's last position: a prime of P
tokens is prefilled for positions [0, P-1) and the shared step samples the
first new token from prime[P-1], as ``sample_cached_batch(prefill=True)``
does. A prime shorter than ``prefill_min_tokens`` + 1, or with two pad
tokens (it retires inside its prime), is teacher-forced as without the flag.

A slot's caches are never cleared. A request starts at position 0, where
the token shift reads zeros, and the attention band and the SGU prefix only
reach rows the request wrote itself; a prefilled request wrote rows
[0, P-1) and its halos, and a step writes its row before any step reads it,
so what rows >= P-1 still hold of an earlier request is never read.

Threads: ``submit`` is thread-safe and never blocks on the device. Every
device call — allocation, capture, copies, steps — is made by ONE thread:
the worker after ``start()``, else the thread that calls
``run_until_idle()``. Nothing touches the device before the first of those.
"""

from __future__ import annotations

import collections
import threading
import time
from typing import List, Optional

import torch

from . import decode
from .decode import DecodeCache, forward_step_slots
from .models.progen import ProGenBase
from .ops import functional as OF


# fewest prime positions (prime length - 1) that ``SlotEngine(prefill=True)``
# prefills at admission. NOT yet measured through the engine
# (profiles/engine_prefill.md lists the measurement that sets it: the
# shortest prime at which the time to the first token wins by more than the
# spread at 8 slots and the short-prime workload's wall time is not worse
# than flag-off by more than its spread). Until then it is
# ``decode.PREFILL_MIN_TOKENS``'s value, the crossover of one eager prefill
# against the captured step at batch 1 and 8 (profiles/decode_prefill.md).
PREFILL_MIN_TOKENS = 8


class Ticket:
    """One submitted request: ``rows`` sequences of ``length`` tokens.

    ``wait()`` blocks until every row is in and returns ``result``, the
    (rows, length) int64 tensor, zeroed after each row's second pad as
    ``sample_cached_batch`` returns it. ``slots[i]`` is the slot row i ran
    in (None until admitted). ``submitted`` / ``finished`` are
    ``time.perf_counter()`` stamps."""

    def __init__(self, rows: int, length: int):
        self.rows = rows
        self.length = length
        self.result = torch.zeros(rows, length, dtype=torch.long)
        self.slots: List[Optional[int]] = [None] * rows
        self.error: Optional[BaseException] = None
        self.submitted = time.perf_counter()
        self.finished: Optional[float] = None
        self._left = rows
        self._event = threading.Event()

    @property
    def done(self) -> bool:
        return self._event.is_set()

    def wait(self, timeout: Optional[float] = None) -> torch.Tensor:
        if not self._event.wait(timeout):
            raise TimeoutError("request still decoding")
        if self.error is not None:
            raise RuntimeError("the engine failed while this request was "
                               "queued or decoding") from self.error
        return self.result

    def _finish(self, error: Optional[BaseException] = None) -> None:
        self.error = error
        self.finished = time.perf_counter()
        self._event.set()


class _Row:
    """A queued or active row: its ticket, its index there, the host copy of
    what admission uploads, and an upper bound on the steps it still needs."""

    def __init__(self, ticket, index, seq_row, ctl_row):
        self.ticket = ticket
        self.index = index
        self.seq_row = seq_row      # (1, seq_len) int64
        self.ctl_row = ctl_row      # (1, 5) int64
        # positions 0 .. limit - 2 are stepped; a one-token request still
        # takes the step in which the sampler retires it
        self.steps_left = max(int(ctl_row[0, 1]) - 1, 1)
        self.prime_len = int(ctl_row[0, 0])
        self.prime_pads = int((seq_row[0, :self.prime_len] == 0).sum())


class SlotEngine:
    """Continuous-batching decoder over ``slots`` rows of one cache (module
    docstring). ``graph``: capture the step once, on a GPU. ``fused_linear``:
    run its projections on the decode linear kernel. ``check_every``: steps
    between two looks at the positions; results do not depend on it.

    ``prefill``: fill a prime's cache rows with one forward at admission
    (module docstring) instead of teacher-forcing it; ``prefill_rows``: primes
    one such forward takes; ``prefill_min_tokens``: the fewest positions
    worth a forward (None: ``PREFILL_MIN_TOKENS``). The tokens are those of
    the engine without it up to the rounding of a full forward against the
    steps. ValueError where ``decode.prefill_supported`` refuses the model at
    every length (fp32 on a GPU).

    On a GPU the model must be what the slot kernels serve — bf16 or fp32,
    dim_head 64, a vocabulary of 2..1024, windows and SGU widths that are
    multiples of 64 — else ValueError: the engine never falls back."""

    def __init__(self, model: ProGenBase, slots: int, *, graph: bool = False,
                 fused_linear: bool = False, check_every: int = 16,
                 prefill: bool = False, prefill_rows: int = 1,
                 prefill_min_tokens: Optional[int] = None):
        if slots < 1:
            raise ValueError(f"slots must be >= 1, got {slots}")
        if check_every < 1:
            raise ValueError(f"check_every must be >= 1, got {check_every}")
        if prefill_rows < 1:
            raise ValueError(f"prefill_rows must be >= 1, got {prefill_rows}")
        if prefill_min_tokens is None:
            prefill_min_tokens = PREFILL_MIN_TOKENS
        if prefill_min_tokens < 1:
            raise ValueError("prefill_min_tokens must be >= 1, got "
                             f"{prefill_min_tokens}")
        self.model = model
        self.cfg = model.cfg
        self.slots = int(slots)
        self.check_every = int(check_every)
        self.fused_linear = bool(fused_linear)
        p = next(model.parameters())
        self.device = p.device
        self.graph = bool(graph) and self.device.type == "cuda"
        if self.device.type == "cuda":
            self._check_supported(p.dtype)
        self.prefill = bool(prefill)
        self.prefill_rows = int(prefill_rows)
        self.prefill_min_tokens = int(prefill_min_tokens)
        # padded lengths of the prefill forwards, ascending
        self._buckets: List[int] = []
        if self.prefill:
            unit = decode._prefill_len(model, 1, self.device)
            self._buckets = list(range(unit, self.cfg.seq_len + 1, unit))
            if not any(decode.prefill_supported(model, n, self.device)
                       for n in self._buckets):
                raise ValueError(
                    "SlotEngine: prefill=True, but decode.prefill_supported "
                    f"refuses this model on {self.device} at every length "
                    "(on a GPU: bf16, dim_head 64, window and SGU width "
                    f"multiples of 64, {unit} padded rows within seq_len "
                    f"{self.cfg.seq_len})")
        self._lock = threading.Condition()
        self._queue = collections.deque()            # _Row, FIFO
        self._active: List[Optional[_Row]] = [None] * self.slots
        self._owner: Optional[int] = None            # thread of device calls
        self._worker: Optional[threading.Thread] = None
        self._closing = False
        self._error: Optional[BaseException] = None
        self._ready = False
        # what the loop did, for the benchmark: steps run, and slot-steps
        # that had a request in them (a slot counts until the poll that
        # frees it)
        self.steps = 0
        self.occupied_slot_steps = 0
        # prefill forwards run, and prime positions they covered
        self.prefills = 0
        self.prefilled_positions = 0

    def _check_supported(self, dtype) -> None:
        cfg = self.cfg
        bad = []
        if dtype not in (torch.bfloat16, torch.float32):
            bad.append(f"dtype {dtype} (bf16 or fp32)")
        if cfg.dim_head != 64:
            bad.append(f"dim_head {cfg.dim_head} (64)")
        if not 2 <= cfg.num_tokens <= OF.DEC_SAMPLE_MAX_V:
            bad.append(f"vocabulary {cfg.num_tokens} "
                       f"(2..{OF.DEC_SAMPLE_MAX_V})")
        if cfg.dim % 16 != 0:
            bad.append(f"dim {cfg.dim} (a multiple of 16)")
        for attn, ff in self.model.layers:
            if attn.window_size % 64 or cfg.seq_len % attn.window_size:
                bad.append(f"window {attn.window_size} (a multiple of 64 "
                           "that divides seq_len)")
                break
        for _attn, ff in self.model.layers:
            if ff.sgu is not None and ff.sgu.norm_weight.shape[0] % 64:
                bad.append(f"SGU width {ff.sgu.norm_weight.shape[0]} "
                           "(a multiple of 64)")
                break
        if bad:
            raise ValueError("SlotEngine: the slot kernels do not serve this "
                             "model on a GPU: " + "; ".join(bad))

    # ---- requests (any thread) ---------------------------------------------

    def submit(self, primes, length: int, top_k: Optional[int] = None,
               seed: Optional[int] = None) -> Ticket:
        """Queue one request of ``len(primes)`` rows and return its ticket at
        once. ``primes``: 1-D int sequences (ragged); ``length``: tokens per
        row, prime included, in [1, seq_len] and longer than every prime.
        ``top_k=None, seed=None`` is greedy; ``seed`` in [0, 2^63) keys the
        sampler's Philox stream (row i of the request draws stream i, wherever
        it lands); ``top_k`` without a seed draws one here, on the host, from
        torch's global generator. Raises ValueError, before anything changes,
        on a request it cannot serve."""
        cfg = self.cfg
        primes = [torch.as_tensor(p).long().flatten().cpu() for p in primes]
        if not primes:
            raise ValueError("submit: no primes")
        length = int(length)
        if not 1 <= length <= cfg.seq_len:
            raise ValueError(f"length must be in [1, {cfg.seq_len}], "
                             f"got {length}")
        for p in primes:
            if p.shape[0] >= length:
                raise ValueError(f"prime of {p.shape[0]} tokens leaves "
                                 f"nothing to generate in {length}")
            if p.numel() and not (0 <= int(p.min())
                                  and int(p.max()) < cfg.num_tokens):
                raise ValueError("prime tokens must be in "
                                 f"[0, {cfg.num_tokens})")
        if top_k is not None and not 0 <= int(top_k) <= cfg.num_tokens:
            raise ValueError(f"top_k must be in [0, {cfg.num_tokens}], "
                             f"got {top_k}")
        if seed is not None and not 0 <= int(seed) < 2 ** 63:
            raise ValueError(f"seed must be in [0, 2^63), got {seed}")
        if top_k is not None and seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,)))
        k = 0 if top_k is None else int(top_k)
        s = -1 if seed is None else int(seed)

        ticket = Ticket(len(primes), length)
        rows = []
        for i, p in enumerate(primes):
            seq_row = torch.zeros(1, cfg.seq_len, dtype=torch.long)
            seq_row[0, :p.shape[0]] = p
            ctl_row = torch.tensor([[p.shape[0], length, k, s, i]],
                                   dtype=torch.long)
            rows.append(_Row(ticket, i, seq_row, ctl_row))
        with self._lock:
            if self._error is not None:
                raise RuntimeError("the engine has failed") from self._error
            if self._closing:
                raise RuntimeError("the engine is closed")
            self._queue.extend(rows)
            self._lock.notify_all()
        return ticket

    def generate(self, primes, length: int, top_k: Optional[int] = None,
                 seed: Optional[int] = None) -> torch.Tensor:
        """``submit`` and wait: the (rows, length) result. On a started
        engine any thread may call it; otherwise the caller runs the loop."""
        ticket = self.submit(primes, length, top_k=top_k, seed=seed)
        if self._worker is None:
            self.run_until_idle()
        return ticket.wait()

    # ---- the loop (one thread) -----------------------------------------------

    def run_until_idle(self) -> None:
        """Run the loop in the calling thread until nothing is queued or
        active. Not on a started engine: its worker owns the device."""
        if self._worker is not None:
            raise RuntimeError("run_until_idle on a started engine; its "
                               "worker thread runs the loop")
        self._own()
        try:
            while self._busy():
                self.cycle()
        except BaseException as e:
            self._fail(e)
            raise

    def start(self) -> "SlotEngine":
        """Run the loop on one worker thread, which also builds the device
        state and captures the graph; it sleeps while nothing is queued or
        active."""
        with self._lock:
            if self._worker is not None:
                return self
            if self._owner is not None:
                raise RuntimeError("this engine already ran its loop on "
                                   "another thread")
            self._worker = threading.Thread(target=self._serve,
                                            name="slot-engine", daemon=True)
        self._worker.start()
        return self

    def close(self) -> None:
        """Finish what is queued and active, then stop the worker."""
        with self._lock:
            self._closing = True
            self._lock.notify_all()
        if self._worker is not None:
            self._worker.join()

    def __enter__(self):
        return self.start()

    def __exit__(self, *exc):
        self.close()

    def _serve(self) -> None:
        try:
            self._own()
            while True:
                with self._lock:
                    while not self._closing and not self._busy():
                        self._lock.wait()
                    if not self._busy():
                        return
                self.cycle()
        except BaseException as e:  # noqa: BLE001 - handed to the tickets
            self._fail(e)

    def _busy(self) -> bool:
        return bool(self._queue) or any(r is not None for r in self._active)

    def _own(self) -> None:
        me = threading.get_ident()
        if self._owner is None:
            self._owner = me
        elif self._owner != me:
            raise RuntimeError("one thread owns every device call of a "
                               "SlotEngine; this is another one")
        if not self._ready:
            self._build()
            self._ready = True

    def _fail(self, e: BaseException) -> None:
        with self._lock:
            self._error = e
            rows = list(self._queue) + [r for r in self._active
                                        if r is not None]
            self._queue.clear()
            self._active = [None] * self.slots
        for t in {r.ticket for r in rows}:
            t._finish(e)

    @torch.no_grad()
    def _build(self) -> None:
        """Device state, every slot idle, and the capture. All initial values
        arrive by host-to-device copy."""
        dev, S, L = self.device, self.slots, self.cfg.seq_len
        self.cache = DecodeCache(self.model, batch=S, device=dev)
        self.pos = torch.full((S,), -1, dtype=torch.long).to(dev, copy=True)
        self.token = torch.zeros(S, dtype=torch.long).to(dev, copy=True)
        self.seq = torch.zeros(S, L, dtype=torch.long).to(dev, copy=True)
        self.pads = torch.zeros(S, dtype=torch.long).to(dev, copy=True)
        self.ctl = torch.zeros(S, len(OF.SLOT_CTL),
                               dtype=torch.long).to(dev, copy=True)
        # prefill at admission: static inputs of the forwards, one token
        # buffer per bucket; no batch row admits anything yet
        R = self.prefill_rows
        self._pf_tokens = {
            n: torch.zeros(R, n, dtype=torch.long).to(dev, copy=True)
            for n in self._buckets}
        self._pf_admit = torch.tensor([[-1, 0]] * R,
                                      dtype=torch.long).to(dev, copy=True)
        self._pf_src = torch.zeros(S, dtype=torch.long).to(dev, copy=True)
        self._pf_live = torch.full((S,), -1,
                                   dtype=torch.long).to(dev, copy=True)
        self._graph = None
        self._pf_graphs = {}
        if not self.graph:
            return
        # every slot is idle and no batch row admits: warm-up and capture
        # change no cache, halo, sequence or position, so there is nothing to
        # snapshot and restore. Every graph is captured before the first
        # replay of any.
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._step()
                for n in self._buckets:
                    self._prefill_forward(n)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self._step()
        for n in self._buckets:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._prefill_forward(n)
            self._pf_graphs[n] = g
        torch.cuda.synchronize()

    def _step(self) -> None:
        logits = forward_step_slots(self.model, self.token, self.cache,
                                    self.pos, fused_linear=self.fused_linear)
        OF.decode_sample_slots(logits, self.pos, self.token, self.seq,
                               self.pads, self.ctl)

    def _prefill_forward(self, n: int) -> None:
        decode.prefill_rows(self.model, self._pf_tokens[n], self.cache,
                            self._pf_admit, self._pf_src, self._pf_live)

    def _admit(self, b: int, row: _Row, at: int = 0) -> None:
        """Start ``row`` in slot ``b`` at position ``at`` (0, or past the
        positions a prefill covered): copies into the slot's row views, the
        position last."""
        token = row.seq_row[:, at].contiguous()              # (1,)
        self.seq[b:b + 1].copy_(row.seq_row)
        self.token[b:b + 1].copy_(token)
        # positions 0 .. at are written at entry and count where they are pads
        self.pads[b:b + 1].copy_(
            (row.seq_row[:, :at + 1] == 0).sum(dim=1))
        self.ctl[b:b + 1].copy_(row.ctl_row)
        self.pos[b:b + 1].copy_(torch.full((1,), at, dtype=torch.long))
        row.steps_left -= at

    def _prefill_bucket(self, row: _Row) -> Optional[int]:
        """The padded length of the forward that prefills ``row``'s prime, or
        None when the row is teacher-forced: prefill is off, the prime is too
        short to be worth a forward, it retires inside its prime (two pads),
        or no bucket holds it."""
        n = row.prime_len - 1
        if not self.prefill or n < self.prefill_min_tokens \
                or row.prime_pads > 1:
            return None
        return next((np_ for np_ in self._buckets if np_ >= n), None)

    def _admit_prefilled(self, np_: int, chunk) -> None:
        """One prefill forward of ``np_`` padded rows for the
        (slot, row) pairs of ``chunk``, at most ``prefill_rows`` of them, then
        their admission at the last prime position."""
        R, S = self.prefill_rows, self.slots
        tokens = torch.zeros(R, np_, dtype=torch.long)
        admit = torch.tensor([[-1, 0]] * R, dtype=torch.long)
        src = torch.zeros(S, dtype=torch.long)
        live = torch.full((S,), -1, dtype=torch.long)
        for r, (b, row) in enumerate(chunk):
            n = row.prime_len - 1
            tokens[r, :n] = row.seq_row[0, :n]
            admit[r, 0], admit[r, 1] = b, n
            src[b], live[b] = r * np_ + n - 1, 0
            self.prefilled_positions += n
        self._pf_tokens[np_].copy_(tokens)
        self._pf_admit.copy_(admit)
        self._pf_src.copy_(src)
        self._pf_live.copy_(live)
        if self._graph is not None:
            self._pf_graphs[np_].replay()
        else:
            self._prefill_forward(np_)
        self.prefills += 1
        for b, row in chunk:
            self._admit(b, row, at=row.prime_len - 1)

    @torch.no_grad()
    def cycle(self) -> None:
        """One pass of the loop: admit, step, look. ``run_until_idle`` and
        the worker call it; so may a caller that drives the loop itself, from
        the owning thread and while something is queued or active."""
        self._own()
        if not self._busy():
            return
        # 1. admit queued rows, FIFO, into the lowest free slots
        with self._lock:
            admitted = []
            for b in range(self.slots):
                if not self._queue:
                    break
                if self._active[b] is None:
                    row = self._queue.popleft()
                    self._active[b] = row
                    row.ticket.slots[row.index] = b
                    admitted.append((b, row))
        groups = {}                     # bucket -> [(slot, row)]
        for b, row in admitted:
            np_ = self._prefill_bucket(row)
            if np_ is None:
                self._admit(b, row)
            else:
                groups.setdefault(np_, []).append((b, row))
        for np_, group in sorted(groups.items()):
            for i in range(0, len(group), self.prefill_rows):
                self._admit_prefilled(np_, group[i:i + self.prefill_rows])

        # 2. step: as many as the longest active row can still need
        active = [r for r in self._active if r is not None]
        n = max(1, min(self.check_every,
                       max(r.steps_left for r in active)))
        if self._graph is not None:
            for _ in range(n):
                self._graph.replay()
        else:
            for _ in range(n):
                self._step()
        for r in active:
            r.steps_left -= n
        self.steps += n
        self.occupied_slot_steps += n * len(active)

        # 3. look at the positions; a live slot below 0 has finished
        pos = self.pos.cpu().tolist()
        finished = []
        for b, row in enumerate(self._active):
            if row is None or pos[b] >= 0:
                continue
            out = self.seq[b:b + 1].cpu()[0, :row.ticket.length]
            after_eos = (out == 0).long().cumsum(dim=-1) > 1
            row.ticket.result[row.index] = out * (~after_eos).long()
            finished.append((b, row))
        done = []
        with self._lock:
            for b, row in finished:
                self._active[b] = None
                row.ticket._left -= 1
                if row.ticket._left == 0:
                    done.append(row.ticket)
        for t in done:
            t._finish()
