"""Per-class timing of the weight-gradient GEMM dW = dY^T X: the r02
atomic-drain kernel, the streaming kernel without and with the column sum,
and the library GEMM without and with the separate bias reduction,
alternating in one process.  Run on an MI355X:

    python tools/wgrad_bench.py [--batches 5 6] [--rounds 3] [--iters 20]

The classes are the Linear weight gradients of one training step at n=256,
m=128 (pair rows Rp = b*n*n, MSA rows Rm = b*m*n): the seven of
tools/ffgemm_bench.py plus the attention-bias projection (Rp, 8, 256), the
outer-mean projection (Rm, 512, 256) and the packed triangle-multiplication
projection (Rp, 1280, 256).  GB/s is the compulsory read —
dY and X once, 2 K (M + N) bytes — over the median time, and "share" that
rate over the 6.3 TB/s the HBM delivers.  "ahead" says whether the
streaming kernel beat both the r02 kernel and the library GEMM in every
round (and, with the column sum, the GEMM plus reduction).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from alphafold2_amd.ops.dispatch import _load_ext

HBM_GBS = 6300.


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


def classes(b, n, m):
    """(label, K, M, N) with dY (K, M) and X (K, N)."""
    rp, rm = b * n * n, b * m * n
    return [
        ('ff1_wgrad_msa', rm, 2048, 256),
        ('ff1_wgrad_pair', rp, 2048, 256),
        ('ff2_wgrad_pair', rp, 256, 1024),
        ('qkvg_wgrad', rp, 2048, 256),
        ('out_wgrad', rp, 256, 512),
        ('trimul_out_wgrad', rp, 256, 256),
        ('gating_wgrad', rp, 512, 256),
        ('attn_bias_wgrad', rp, 8, 256),
        ('outer_proj_wgrad', rm, 512, 256),
        ('trimul_proj_wgrad', rp, 1280, 256),
    ]


LEGS = ['r02', 'stream', 'stream+cs', 'gemm', 'gemm+sum']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[5, 6])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('-n', type=int, default=256)
    ap.add_argument('-m', type=int, default=128)
    args = ap.parse_args()
    ext = _load_ext()
    assert ext is not None, "the gfx950 extension must load"
    gen = torch.Generator(device='cuda').manual_seed(0)
    for b in args.batches:
        print(f"batch {b}, n={args.n}, m={args.m}: ms per call, median "
              f"[min max] of {args.rounds} alternating rounds of "
              f"{args.iters} calls; GB/s and share of {HBM_GBS:.0f} GB/s "
              f"for the streaming kernel")
        print(f"{'class':18s} {'K':>7s} {'M':>5s} {'N':>5s} {'MB':>5s} "
              + ' '.join(f"{leg:>21s}" for leg in LEGS)
              + f" {'GB/s':>6s} {'share':>6s} {'cs GB/s':>7s} {'ahead':>6s} "
              f"{'cs ahead':>8s}")
        for label, K, M, N in classes(b, args.n, args.m):
            dy = torch.randn(K, M, device='cuda', dtype=torch.bfloat16,
                             generator=gen)
            x = torch.randn(K, N, device='cuda', dtype=torch.bfloat16,
                            generator=gen)
            fns = {
                'r02': lambda: ext.wgrad_v1(dy, x),
                'stream': lambda: ext.wgrad(dy, x),
                'stream+cs': lambda: ext.wgrad_colsum(dy, x),
                'gemm': lambda: dy.t() @ x,
                'gemm+sum': lambda: (dy.t() @ x, dy.sum(dim=0)),
            }
            # the legs agree to the bf16 rounding of the library result
            ref = fns['gemm']().float()
            dw, cs = fns['stream+cs']()
            tol = 2.0 ** -7 * ref.abs() + 1e-3 * K ** 0.5
            assert ((dw - ref).abs() <= tol).all(), label
            assert ((fns['r02']() - ref).abs() <= tol).all(), label
            # (the two streaming legs may split K differently: the column
            # sums count against the cap on the partials)
            assert ((fns['stream']() - ref).abs() <= tol).all(), label
            assert ((cs - dy.float().sum(0)).abs()
                    <= 1e-3 * K ** 0.5).all(), label
            ts = {leg: [] for leg in LEGS}
            for _ in range(args.rounds):
                for leg in LEGS:
                    ts[leg].append(time_fn(fns[leg], args.iters))
            med = {leg: sorted(t)[len(t) // 2] for leg, t in ts.items()}
            nbytes = 2 * K * (M + N)
            cells = ' '.join(
                f"{med[leg]:8.3f} [{min(ts[leg]):5.3f} {max(ts[leg]):5.3f}]"
                for leg in LEGS)
            ahead = all(s < r and s < g for s, r, g in
                        zip(ts['stream'], ts['r02'], ts['gemm']))
            cs_ahead = all(s < g for s, g in
                           zip(ts['stream+cs'], ts['gemm+sum']))
            gbs = nbytes / med['stream'] / 1e6
            print(f"{label:18s} {K:7d} {M:5d} {N:5d} {nbytes / 1e6:5.0f} "
                  f"{cells} {gbs:6.0f} {gbs / HBM_GBS:6.2f} "
                  f"{nbytes / med['stream+cs'] / 1e6:7.0f} "
                  f"{'yes' if ahead else 'no':>6s} "
                  f"{'yes' if cs_ahead else 'no':>8s}", flush=True)
            del dy, x
        print(flush=True)


if __name__ == '__main__':
    main()
