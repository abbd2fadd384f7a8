"""Old against new for the three backward reductions of r10, alternating in
one process.  Run on an MI355X:

    python tools/reduce_bench.py [--batches 5 6] [--rounds 3] [--iters 20]

* pair-rep backward at the flagship shape (b, 256, 256, 256) bf16, 65-row
  table: the library composition (two wide sums, an fp32 copy, a zero
  fill and an index_add with float atomics) against `ext.pairrep_bwd`.
  Floor: one read of dy.
* dQ + dBias on the stored-dS path at the four biased classes of
  docs/KERNELS.md "Attention backward: stored dS": `attn_bwd` with the
  two kernels (dQ from dS, then the dBias sum) against the fused kernel
  with the launcher's own entries per block.  Both legs run the same
  dK/dV kernel first, so the difference of the two columns is the
  difference of the dQ + dBias part; its kernel times come from
  torch.profiler in the same process.  Floor: dS + K + dQ + dbias bytes
  once (the two kernels read dS twice).
* the fold at the (nb, C) of the ten weight-gradient classes (as
  wgrad_stream picks its K slots with one block per CU) and of the three
  column-sum callers: the scalar body against the 16-byte body.  Floor:
  the partial bytes once.

Every class is first checked between its legs.  Times are ms per call,
median [min max] of the rounds; "floor" is bytes over 5 TB/s, "x floor"
the new leg's median over it, and "ahead" says whether the new leg beat
the old one in every round.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from alphafold2_amd.ops.dispatch import _load_ext
from alphafold2_amd.ops.hip_autograd import _pairrep_bwd_composed

FLOOR_BPS = 5e12
H = 8


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


def ab(fns, rounds, iters):
    """{leg: [ms per round]} with the legs alternating."""
    ts = {leg: [] for leg in fns}
    for _ in range(rounds):
        for leg, fn in fns.items():
            ts[leg].append(time_fn(fn, iters))
    return ts


def med(t):
    return sorted(t)[len(t) // 2]


def cell(t):
    return f"{med(t):8.4f} [{min(t):6.4f} {max(t):6.4f}]"


def row(label, ts, nbytes, extra=''):
    old, new = ts['old'], ts['new']
    floor = nbytes / FLOOR_BPS * 1e3
    ahead = all(n < o for n, o in zip(new, old))
    print(f"{label:34s} {nbytes / 1e6:8.1f} {cell(old)} {cell(new)} "
          f"{floor:7.4f} {med(new) / floor:7.2f} "
          f"{'yes' if ahead else 'no':>5s}{extra}", flush=True)


HEAD = (f"{'class':34s} {'MB':>8s} {'old ms':>24s} {'new ms':>24s} "
        f"{'floor':>7s} {'x floor':>7s} {'ahead':>5s}")


def bench_pairrep(ext, args, gen):
    print("pair-rep backward: library composition (old) against "
          "ext.pairrep_bwd (new)")
    print(HEAD)
    V = 65
    for b in args.batches:
        n, d = args.n, 256
        dy = torch.randn(b, n, n, d, device='cuda', generator=gen) \
            .to(torch.bfloat16)
        i = torch.arange(n, device='cuda')
        rel = ((i[:, None] - i[None, :]).clamp(-32, 32) + 32) \
            .expand(b, n, n).contiguous()
        assert ext.pairrep_bwd_covers(dy, V), "flagship shape not covered"
        fns = {'old': lambda: _pairrep_bwd_composed(dy, rel, V),
               'new': lambda: ext.pairrep_bwd(dy, rel, V)}
        for o, w in zip(fns['old'](), fns['new']()):
            tol = 2.0 ** -7 * o.float().abs() + 1e-2 * n ** 0.5
            assert ((o.float() - w.float()).abs() <= tol).all()
        row(f"pairrep_bwd b={b} clamp(i-j)", ab(fns, args.rounds, args.iters),
            dy.numel() * 2)
        rel = torch.randint(0, V, (b, n, n), device='cuda', generator=gen)
        row(f"pairrep_bwd b={b} random rel", ab(fns, args.rounds, args.iters),
            dy.numel() * 2)
        del dy, rel
    print(flush=True)


def attn_classes(b, n, m):
    """(label, B, Lq, Lk, bias_repeat) of docs/KERNELS.md."""
    return [('msa_row', b * m, n, n, m),
            ('triangle_out', b * n, n, n, n),
            ('triangle_in', b * n, n, n, n),
            ('bias_repeat_1', 64, n, n, 1)]


def kernel_ms(fn, iters, names):
    """Device ms per call of the kernels whose name holds one of `names`."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = {k: 0. for k in names}
    for ev in prof.key_averages():
        for k in names:
            if k in ev.key:
                out[k] += getattr(ev, 'device_time_total',
                                  getattr(ev, 'cuda_time_total', 0.)) \
                    / 1e3 / iters
    return out


def bench_dq_dbias(ext, args, gen):
    print("attn_bwd on the stored-dS path: dQ kernel + dBias sum kernel "
          "(old) against the fused kernel (new); kernel ms per call from "
          "torch.profiler: dq + sum | fused + fold")
    print(HEAD + "   kernels old | new")
    b = args.batches[0]
    rnd = lambda *s: torch.randn(*s, device='cuda', generator=gen) \
        .to(torch.bfloat16)
    for label, B, Lq, Lk, r in attn_classes(b, args.n, args.m):
        q, k, v, dout = (rnd(B, H, Lq, 64) for _ in range(4))
        bias = rnd(B // r, H, Lq, Lk)
        out, lse = ext.attn_fwd(q, k, v, bias, None, r, 0.125)[:2]

        def bwd(epb):
            return ext.attn_bwd(dout, q, k, v, out, lse, bias, None, r, 0.125,
                                True, dq_entries_per_block=epb)
        fns = {'old': lambda: bwd(0), 'new': lambda: bwd(None)}
        o, w = fns['old'](), fns['new']()
        assert torch.equal(o[0], w[0]), f"{label}: dq differs"
        tol = 2.0 ** -7 * o[3].abs() + 1e-2 * r ** 0.5
        assert ((o[3] - w[3]).abs() <= tol).all(), f"{label}: dbias"
        del o, w
        ko = kernel_ms(fns['old'], 5, ['dq_from_ds', 'dbias_sum'])
        kn = kernel_ms(fns['new'], 5, ['dq_dbias', 'colsum_fold'])
        nbytes = B * H * Lq * Lk * 2 + 2 * B * H * Lk * 64 * 2 \
            + (B // r) * H * Lq * Lk * 4
        row(f"{label} ({B},{Lq},{Lk},{r})", ab(fns, args.rounds, args.iters),
            nbytes, f"   {sum(ko.values()):.4f} | {sum(kn.values()):.4f}"
            f" = {kn['dq_dbias']:.4f} + {kn['colsum_fold']:.4f}")
        del q, k, v, dout, bias, out, lse
    print("(the ms columns are whole attn_bwd calls, dK/dV included: "
          "'x floor' there is not the fused kernel's; set the kernels "
          "column against the floor)")
    print(flush=True)


def fold_classes(b, n, m, cus):
    """(label, nb, C): the K slots wgrad_stream picks with one block per CU
    (256 x 256 tiles, 64 MB cap on the partials), and the column-sum
    callers at the device's grid."""
    rp, rm = b * n * n, b * m * n
    out = []
    for label, K, M, N, cs in [
            ('ff1_wgrad_msa', rm, 2048, 256, True),
            ('ff1_wgrad_pair', rp, 2048, 256, True),
            ('ff2_wgrad_pair', rp, 256, 1024, True),
            ('qkvg_wgrad', rp, 2048, 256, False),
            ('out_wgrad', rp, 256, 512, True),
            ('trimul_out_wgrad', rp, 256, 256, True),
            ('gating_wgrad', rp, 512, 256, True),
            ('attn_bias_wgrad', rp, 8, 256, False),
            ('outer_proj_wgrad', rm, 512, 256, True),
            ('trimul_proj_wgrad', rp, 1280, 256, True)]:
        rowlen = M * N + (M if cs else 0)
        tiles = -(-M // 256) * -(-N // 256)
        slots = max(1, cus // tiles)
        slots = min(slots, -(-K // 32), max(1, (64 << 20) // (rowlen * 4)))
        if tiles > 1 and slots > 8:
            slots -= slots % 8
        out.append((label, slots, rowlen))
    out += [('geglu_colsum pair (H2=2048)', 7 * cus, 2048),
            ('geglu_colsum msa (H2=2048)', 7 * cus, 2048),
            ('gate_colsum (C=512)', 8 * cus, 512)]
    return [(label, min(nb, 2048), C) for label, nb, C in out]


def bench_fold(ext, args, gen):
    print("fold of (nb, C) fp32 partials: scalar body (old) against the "
          "16-byte body (new)")
    print(HEAD)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for label, nb, C in fold_classes(args.batches[0], args.n, args.m, cus):
        part = torch.randn(nb, C, device='cuda', generator=gen)
        fns = {'old': lambda: ext.colsum_fold(part, v1=True),
               'new': lambda: ext.colsum_fold(part)}
        o, w = fns['old'](), fns['new']()
        bound = nb * 2.0 ** -23 * part.abs().sum(0)
        assert ((o - w).abs() <= bound).all(), label
        row(f"{label} ({nb},{C})", ab(fns, args.rounds, args.iters),
            part.numel() * 4)
        del part
    print(flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[5, 6])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('-n', type=int, default=256)
    ap.add_argument('-m', type=int, default=128)
    ap.add_argument('--only', choices=['pairrep', 'dq', 'fold'], default=None)
    args = ap.parse_args()
    ext = _load_ext()
    assert ext is not None, "the gfx950 extension must load"
    gen = torch.Generator(device='cuda').manual_seed(0)
    print(f"ms per call, median [min max] of {args.rounds} alternating "
          f"rounds of {args.iters} calls; floor = MB over "
          f"{FLOOR_BPS / 1e12:.0f} TB/s", flush=True)
    if args.only in (None, 'pairrep'):
        bench_pairrep(ext, args, gen)
    if args.only in (None, 'dq'):
        bench_dq_dbias(ext, args, gen)
    if args.only in (None, 'fold'):
        bench_fold(ext, args, gen)


if __name__ == '__main__':
    main()
