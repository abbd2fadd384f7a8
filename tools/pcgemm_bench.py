"""Per-class timing of the per-channel GEMM: the scatter-staging, the
wide-store and the full-line kernel, alternating in one process.  Run on
an MI355X:

    python tools/pcgemm_bench.py [--batches 6 5] [--rounds 3] [--iters 20]

The nine classes are the calls one training step makes at n=256, m=128,
D=256 (ops/hip_autograd.py: _TriMixFn, _OuterSumFn).  "near" means the
contraction axis is the memory-near one of the operand (k-stride D),
"far" the other (k-stride n*D).  GB/s is the compulsory traffic — each
operand read once, the output written once — over the median time.
Every class is first checked: wide-store bit-for-bit against scatter
staging, full-line against it to bf16 rounding.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from alphafold2_amd.ops.hip_autograd import _pcg


def time_fn(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def classes(n, m):
    """(label, operand kinds, M, N, K, a_m, a_k, b_n, b_k, alpha); kind
    'p' is a pair tensor (b, n, n, D), 'm' an MSA-side one (b, m, n, D)."""
    a = 1.0 / m
    return [
        ("tri_out_fwd  near/near", "pp", n, n, n, 1, 2, 1, 2, 1.0),
        ("tri_in_fwd   far/far", "pp", n, n, n, 2, 1, 2, 1, 1.0),
        ("tri_out_dL   near/far", "pp", n, n, n, 1, 2, 2, 1, 1.0),
        ("tri_out_dR   far/far", "pp", n, n, n, 2, 1, 2, 1, 1.0),
        ("tri_in_dL    near/far", "pp", n, n, n, 1, 2, 2, 1, 1.0),
        ("tri_in_dR    near/near", "pp", n, n, n, 1, 2, 1, 2, 1.0),
        ("outer_fwd    far/far", "mm", n, n, m, 2, 1, 2, 1, a),
        ("outer_dL     near/near", "mp", m, n, n, 1, 2, 1, 2, a),
        ("outer_dR     near/far", "mp", m, n, n, 1, 2, 2, 1, a),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[6, 5])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('-n', type=int, default=256)
    ap.add_argument('-m', type=int, default=128)
    ap.add_argument('-D', type=int, default=256)
    args = ap.parse_args()
    n, m, D = args.n, args.m, args.D
    gen = torch.Generator(device='cuda').manual_seed(0)
    for b in args.batches:
        shape = {'p': (b, n, n, D), 'm': (b, m, n, D)}
        print(f"batch {b}, n={n}, m={m}, D={D}: ms per call, median "
              f"[min max] of {args.rounds} alternating rounds of "
              f"{args.iters} calls")
        print(f"{'class':24s} {'MB':>6s} {'scatter_ms':>22s} {'GB/s':>6s} "
              f"{'wide_ms':>22s} {'GB/s':>6s} {'line_ms':>22s} {'GB/s':>6s} "
              f"{'s/line':>6s}")
        tot = {1: 0., 2: 0., 3: 0.}
        for label, kinds, M, N, K, a_m, a_k, b_n, b_k, alpha in classes(n, m):
            A, B = (torch.randn(shape[k], device='cuda', dtype=torch.bfloat16,
                                generator=gen) for k in kinds)
            run = lambda v: _pcg(A, B, M, N, K, a_m, a_k, b_n, b_k,
                                 alpha=alpha, variant=v)
            ref = run(1)
            assert torch.equal(ref, run(2)), label
            diff = (run(3).float() - ref.float()).abs()
            assert (diff <= 2.0 ** -7 * ref.float().abs() + 1e-2).all(), label
            ts = {1: [], 2: [], 3: []}
            for _ in range(args.rounds):
                for v in (1, 2, 3):
                    ts[v].append(time_fn(lambda: run(v), args.iters))
            nbytes = 2 * b * D * (M * K + N * K + M * N)
            cells = []
            for v in (1, 2, 3):
                t = sorted(ts[v])
                med = t[len(t) // 2]
                tot[v] += med
                cells.append(f"{med:8.3f} [{t[0]:5.3f} {t[-1]:5.3f}] "
                             f"{nbytes / med / 1e6:6.0f}")
            r = sorted(ts[1])[len(ts[1]) // 2] / sorted(ts[3])[len(ts[3]) // 2]
            print(f"{label:24s} {nbytes / 1e6:6.0f} {cells[0]} {cells[1]} "
                  f"{cells[2]} {r:6.2f}", flush=True)
            del A, B
        # a 12-block trunk runs every class 12 times per training step
        print(f"sum of the nine medians: scatter {tot[1]:.3f} ms, "
              f"wide {tot[2]:.3f} ms, line {tot[3]:.3f} ms "
              f"(x12 per step of a 12-block trunk)\n",
              flush=True)


if __name__ == '__main__':
    main()
