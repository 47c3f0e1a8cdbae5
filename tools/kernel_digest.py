"""sha256 of every output of the row kernels on the seeded inputs of
tests/test_gpu_kernel_edges.py, to show that a change of their source left
every bit where it was.

    python tools/kernel_digest.py OUT.json        # needs the GPU
    python tools/kernel_digest.py --compare A.json B.json

The first form calls the entry points of progen_amd._C — of the tree this
file lies in — on every case the ln_shift, ln_shift_res, glu, gelu, ce,
fused_adamw and grad_sumsq tests use, built by tests/kernel_oracle.py and
run by the tests' own ``run_*`` helpers, and writes {"family|case|output":
sha256}. Copied into a checkout of another commit it digests that commit's
kernels; the second form compares two such files and exits 1 if they
differ.

grad_sumsq joins its block partials with atomicAdd, in the order the
hardware takes them: only its one-block case (numel 8) is compared by
digest. For the large numel each file records the error against the fp64
sum and the bound of the test, and the comparison wants both within it.
"""

import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SUMSQ_BY_DIGEST = 8     # numel of the single-block case


def sha(t):
    import torch
    raw = t.detach().contiguous().cpu().view(-1).view(torch.uint8)
    return hashlib.sha256(raw.numpy().tobytes()).hexdigest()


def digest():
    import kernel_oracle as K
    import test_gpu_kernel_edges as T

    out, sumsq = {}, {}

    def put(family, case, tensors):
        for name, t in tensors.items():
            out[f"{family}|{case}|{name}"] = sha(t)

    for dn in T.DTYPES:
        dt = K._dt(dn)
        for case in K.ln_cases(dt):
            put(K.ln_family(case), case, T.run_ln(case))
        for case in K.glu_cases(dt):
            put("glu", case, T.run_act("glu", case))
        for case in K.gelu_cases(dt):
            put("gelu", case, T.run_act("gelu", case))
        for case in K.ce_cases(dt):
            put("ce", case, T.run_ce(case))
        for sharded in (False, True):
            put("adamw", (dn, sharded), T.run_adamw(dn, sharded)[1])
        for numel in K.SUMSQ_NUMEL:
            x = K.sumsq_inputs(dn, numel)
            got = T.C().grad_sumsq(T.cu(x))
            if numel == SUMSQ_BY_DIGEST:
                put("sumsq", (dn, numel), dict(sumsq=got))
            else:
                sumsq[f"{dn}|{numel}"] = dict(
                    value=float(got), err=K.elem_err(got, K.sumsq_oracle(x)),
                    bound=K.bounds("sumsq", dn)["sumsq"][1])
    return dict(digests=out, sumsq=sumsq)


def compare(path_a, path_b):
    a, b = (json.load(open(p)) for p in (path_a, path_b))
    da, db = a["digests"], b["digests"]
    bad = sorted(k for k in da.keys() | db.keys() if da.get(k) != db.get(k))
    for k in bad:
        print(f"DIFFERS|{k}|{da.get(k)}|{db.get(k)}")
    families = sorted({k.split("|")[0] for k in da})
    for f in families:
        n = sum(k.startswith(f + "|") for k in da)
        d = sum(k.startswith(f + "|") for k in bad)
        print(f"DIGEST|{f}|{n} outputs|{d} differ")
    for path, r in ((path_a, a), (path_b, b)):
        for k, v in sorted(r["sumsq"].items()):
            ok = v["err"] <= v["bound"]
            print(f"SUMSQ|{path}|{k}|value {v['value']!r}|err {v['err']:.3e}"
                  f"|bound {v['bound']:.3e}|{'ok' if ok else 'MISSED'}")
            if not ok:
                bad.append(k)
    if a["sumsq"].keys() != b["sumsq"].keys():
        bad.append("sumsq keys")
    print(f"{len(da)} digests in {path_a}, {len(db)} in {path_b}: "
          + ("EQUAL" if not bad else f"{len(bad)} DIFFER"))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    result = digest()
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(f"{len(result['digests'])} digests -> {sys.argv[1]}")
