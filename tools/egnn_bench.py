"""Layer-level A/B of the fused EGNN edge-message core (K16) against the
eager composition, on one EGNNLayer at the config-5 shape (b=1, n=512,
dim = edge dim = 256, fp32).  Run on an MI355X:

    python tools/egnn_bench.py

Fused and eager run in one process, alternating, `--rounds` times; each
figure is the mean of `--iters` calls after warmup.  Reported: forward +
backward (every parameter, h, x and edges require grad), forward under
no_grad, and torch.cuda.max_memory_allocated of each leg above its
inputs.  A single forward + backward at `--mem-n` (default 1024) is added
for the memory figure at a long crop.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from alphafold2_amd.models.equivariant import EGNNLayer
from alphafold2_amd.ops import dispatch


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


def make(n, dim):
    torch.manual_seed(0)
    layer = EGNNLayer(dim, edge_dim=dim).cuda().train()
    # zero-initialised: give the coordinate path something to do
    torch.nn.init.normal_(layer.coors_mlp[-1].weight, std=0.02)
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
    prev = os.environ.get('AF2AMD_EGNN_FUSED')
    os.environ['AF2AMD_EGNN_FUSED'] = '1' if fused else '0'
    try:
        return fn(*args, **kwargs)
    finally:
        if prev is None:
            del os.environ['AF2AMD_EGNN_FUSED']
        else:
            os.environ['AF2AMD_EGNN_FUSED'] = prev


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--mem-n', type=int, default=1024,
                    help='length of the single memory-only run (0 = skip)')
    args = ap.parse_args()
    assert dispatch.hip_ops_available()

    layer, h, x, edges, mask = make(args.n, args.dim)
    assert with_path(True, dispatch.egnn_core_fusable, h, edges, m_dim=64)
    fwd_bwd, fwd = legs(layer, h, x, edges, mask)
    print(f'EGNN_BENCH shape b=1 n={args.n} dim={args.dim} '
          f'edge_dim={args.dim} m_dim=64 fp32, mean of {args.iters} calls')
    for r in range(args.rounds):
        for name, fused in (('fused', True), ('eager', False)):
            t_fb = with_path(fused, time_fn, fwd_bwd, args.iters)
            t_f = with_path(fused, time_fn, fwd, args.iters)
            m_fb = with_path(fused, peak_mib, fwd_bwd)
            m_f = with_path(fused, peak_mib, fwd)
            print(f'EGNN_BENCH round={r} {name}: fwd+bwd={t_fb:.3f} ms '
                  f'fwd(no_grad)={t_f:.3f} ms peak_above_inputs: '
                  f'fwd+bwd={m_fb:.1f} MiB fwd={m_f:.1f} MiB', flush=True)

    if args.mem_n:
        del layer, h, x, edges, mask, fwd_bwd, fwd
        torch.cuda.empty_cache()
        layer, h, x, edges, mask = make(args.mem_n, args.dim)
        fwd_bwd, _ = legs(layer, h, x, edges, mask)
        for name, fused in (('fused', True), ('eager', False)):
            m = with_path(fused, peak_mib, fwd_bwd)
            print(f'EGNN_BENCH n={args.mem_n} {name}: fwd+bwd '
                  f'peak_above_inputs={m:.1f} MiB', flush=True)


if __name__ == '__main__':
    main()
