"""Layer-level A/B of the fused SE(3) refiner attention core (K15) against
the eager composition, on one SE3RefinerLayer at the config-4 shape
(b=1, n=384, dim 256, heads 4, dim_head 16, fp32).  Run on an MI355X:

    python tools/se3_bench.py

Fused and eager run in one process, alternating, `--rounds` times; each
figure is the mean of `--iters` calls after warmup.  Reported: forward +
backward (every parameter, h, x and edges require grad), forward under
no_grad, and torch.cuda.max_memory_allocated of each leg.  A single
forward + backward at `--mem-n` (default 1024) is added for the memory
figure at a long crop.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from alphafold2_amd.models.equivariant import SE3RefinerLayer
from alphafold2_amd.ops import dispatch


def time_fn(fn, iters, warmup=10):
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


def make(n, dim, heads, dim_head):
    torch.manual_seed(0)
    layer = SE3RefinerLayer(dim, heads=heads, dim_head=dim_head,
                            edge_dim=dim).cuda().train()
    torch.nn.init.normal_(layer.coors_head.weight, std=0.1)
    h = torch.randn(1, n, dim, device='cuda', requires_grad=True)
    x = (3 * torch.randn(1, n, 3, device='cuda')).requires_grad_(True)
    edges = torch.randn(1, n, n, dim, device='cuda', requires_grad=True)
    mask = torch.ones(1, n, dtype=torch.bool, device='cuda')
    mask[0, -n // 16:] = False
    return layer, h, x, edges, mask


def legs(layer, h, x, edges, mask):
    params = list(layer.parameters()) + [h, x, edges]

    def fwd_bwd():
        ho, xo = layer(h, x, edges=edges, mask=mask)
        torch.autograd.grad(ho.sum() + xo.sum(), params)

    def fwd():
        with torch.no_grad():
            layer(h, x, edges=edges, mask=mask)

    return fwd_bwd, fwd


def with_path(fused, fn, *args, **kwargs):
    prev = os.environ.get('AF2AMD_SE3_FUSED')
    os.environ['AF2AMD_SE3_FUSED'] = '1' if fused else '0'
    try:
        return fn(*args, **kwargs)
    finally:
        if prev is None:
            del os.environ['AF2AMD_SE3_FUSED']
        else:
            os.environ['AF2AMD_SE3_FUSED'] = prev


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=384)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--heads', type=int, default=4)
    ap.add_argument('--dim-head', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--mem-n', type=int, default=1024,
                    help='length of the single memory-only run (0 = skip)')
    args = ap.parse_args()
    assert dispatch.hip_ops_available()

    layer, h, x, edges, mask = make(args.n, args.dim, args.heads,
                                    args.dim_head)
    assert dispatch.se3_core_fusable(h, edges, heads=args.heads,
                                     dim_head=args.dim_head)
    fwd_bwd, fwd = legs(layer, h, x, edges, mask)
    print(f'SE3_BENCH shape b=1 n={args.n} dim={args.dim} '
          f'heads={args.heads} dim_head={args.dim_head} fp32, '
          f'mean of {args.iters} calls')
    for r in range(args.rounds):
        for name, fused in (('fused', True), ('eager', False)):
            t_fb = with_path(fused, time_fn, fwd_bwd, args.iters)
            t_f = with_path(fused, time_fn, fwd, args.iters)
            m_fb = with_path(fused, peak_mib, fwd_bwd)
            m_f = with_path(fused, peak_mib, fwd)
            print(f'SE3_BENCH round={r} {name}: fwd+bwd={t_fb:.3f} ms '
                  f'fwd(no_grad)={t_f:.3f} ms peak_above_inputs: '
                  f'fwd+bwd={m_fb:.1f} MiB fwd={m_f:.1f} MiB', flush=True)

    if args.mem_n:
        del layer, h, x, edges, mask, fwd_bwd, fwd
        torch.cuda.empty_cache()
        layer, h, x, edges, mask = make(args.mem_n, args.dim, args.heads,
                                        args.dim_head)
        fwd_bwd, _ = legs(layer, h, x, edges, mask)
        for name, fused in (('fused', True), ('eager', False)):
            m = with_path(fused, peak_mib, fwd_bwd)
            print(f'SE3_BENCH n={args.mem_n} {name}: fwd+bwd '
                  f'peak_above_inputs={m:.1f} MiB', flush=True)


if __name__ == '__main__':
    main()
