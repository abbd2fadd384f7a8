"""Kernel-level timing of the fused attention + pcgemm ops across the
trunk's real shape classes (stable within-run numbers, independent of
full-bench box noise).  Run on an MI355X:

    python tools/attn_bench.py

`--dropout P` instead prints, per shape class and in the same run, the
forward+backward time of the fused kernels without dropout, of the
fused kernels with attention-probability dropout P, and of the eager
dropout composition (ops/eager.py with the bias repeated), the latter
on a batch cut to `--eager-batch` folded rows so that its (B, h, n, n)
tensors fit, with its time scaled to the full batch.

`--ds-ab` times the attention backward, in one process and alternating,
through the float-atomic dBias path (`ds_scratch_bytes=0`) and through
the stored-dS path, at the batch-5 trunk shapes (MSA row, both
triangles, MSA column, and one bias_repeat = 1 shape), and splits each
backward into its kernels (delta, dK/dV, dQ, dBias sum, fills) with
torch.profiler.  The MSA column has no bias and runs the same kernels
on both settings: its two figures show the noise of the comparison.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from alphafold2_amd.ops.dispatch import _load_ext
from alphafold2_amd.ops.hip_autograd import _pcg


def time_fn(fn, iters=30, warmup=5):
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


def attn_shapes(b=5, n=256, m=128, h=8, d=64):
    # (label, B, Lq, Lk, bias_repeat(None=no bias))
    return [
        ("msa_row", b * m, n, n, m),
        ("msa_col", b * n, m, m, None),
        ("tri_out", b * n, n, n, n),
        ("tri_in", b * n, n, n, n),
    ]


def dropout_ab(ext, p, eager_batch):
    """Within-run A/B of one training step of the attention core."""
    from alphafold2_amd.ops import eager
    h, d = 8, 64
    scale = d ** -0.5
    print(f"{'shape':8s} {'fused_ms':>9s} {'drop_ms':>9s} {'drop/fused':>10s} "
          f"{'eager_ms':>9s} {'eager/drop':>10s}   (fwd+bwd, dropout={p}; "
          f"eager measured at B={eager_batch} and scaled)")
    for label, B, Lq, Lk, brep in attn_shapes():
        mk = lambda *s: torch.randn(*s, device='cuda', dtype=torch.bfloat16)
        q, k, v = mk(B, h, Lq, d), mk(B, h, Lk, d), mk(B, h, Lk, d)
        bias = mk(B // brep, h, Lq, Lk) if brep else None
        dout = mk(B, h, Lq, d)
        r, need_db = brep or 1, bias is not None

        def fused(pd):
            kw = dict(dropout_p=pd) if pd > 0 else {}
            res = ext.attn_fwd(q, k, v, bias, None, r, scale, **kw)
            if pd > 0:
                kw['rng_state'] = res[2]
            ext.attn_bwd(dout, q, k, v, res[0], res[1], bias, None, r,
                         scale, need_db, **kw)

        t_plain = time_fn(lambda: fused(0.), iters=15)
        t_drop = time_fn(lambda: fused(p), iters=15)

        # eager composition on a reduced batch (whole bias-repeat groups)
        Be = min(B, eager_batch)
        re_ = min(r, Be)
        Be = Be // re_ * re_
        qe, ke, ve = (t[:Be].clone().requires_grad_(True) for t in (q, k, v))
        be = bias[:max(1, Be // re_)].clone().requires_grad_(True) \
            if brep else None
        de = dout[:Be]

        def eager_step():
            b = be.repeat_interleave(re_, dim=0) if be is not None else None
            out = eager.attention_core(qe, ke, ve, bias=b, dropout=p,
                                       training=True)
            out.backward(de)
            for t in (qe, ke, ve, be):
                if t is not None:
                    t.grad = None

        t_eager = time_fn(eager_step, iters=5, warmup=2) * (B / Be)
        print(f"{label:8s} {t_plain:9.3f} {t_drop:9.3f} "
              f"{t_drop / t_plain:10.2f} {t_eager:9.3f} "
              f"{t_eager / t_drop:10.2f}")


def _kernel_ms(fn, iters=5):
    """{kernel family: ms per call} of fn from torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    fams = [('dkv', 'attn_bwd_dkv_kernel'),
            ('dq', 'attn_bwd_dq_from_ds_kernel'),
            ('dq', 'attn_bwd_dq_kernel'), ('sum', 'attn_dbias_sum_kernel'),
            ('delta', 'attn_delta_kernel')]
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        t = getattr(ev, 'device_time_total', None)
        if t is None:
            t = ev.cuda_time_total
        if t <= 0:
            continue
        fam = next((f for f, n in fams if n in ev.key), 'other')
        out[fam] = out.get(fam, 0.) + t / 1e3 / iters
    return out


def ds_ab(ext, rounds, iters):
    """Within-run A/B of the attention backward: float-atomic dBias
    against the stored-dS path, alternating `rounds` times."""
    h, d = 8, 64
    scale = d ** -0.5
    shapes = attn_shapes() + [("bias_r1", 64, 256, 256, 1)]
    print(f"{'shape':8s} {'path':7s} {'bwd_ms':>8s} {'min':>8s} {'max':>8s} "
          f"{'TF':>6s}   kernels (ms per call, torch.profiler)")
    for label, B, Lq, Lk, brep in shapes:
        mk = lambda *s: torch.randn(*s, device='cuda', dtype=torch.bfloat16)
        q, k, v = mk(B, h, Lq, d), mk(B, h, Lk, d), mk(B, h, Lk, d)
        bias = mk(B // brep, h, Lq, Lk) if brep else None
        dout = mk(B, h, Lq, d)
        r, need_db = brep or 1, bias is not None
        out, lse = ext.attn_fwd(q, k, v, bias, None, r, scale)
        paths = {
            'atomic': lambda: ext.attn_bwd(dout, q, k, v, out, lse, bias,
                                           None, r, scale, need_db,
                                           ds_scratch_bytes=0),
            'ds': lambda: ext.attn_bwd(dout, q, k, v, out, lse, bias, None,
                                       r, scale, need_db,
                                       ds_scratch_bytes=2 << 30),
        }
        times = {name: [] for name in paths}
        for _ in range(rounds):
            for name, fn in paths.items():
                times[name].append(time_fn(fn, iters=iters, warmup=2))
        gb = 10e-12 * B * h * Lq * Lk * d
        for name, fn in paths.items():
            ts = sorted(times[name])
            med = ts[len(ts) // 2]
            try:
                km = _kernel_ms(fn)
            except Exception as exc:  # the breakdown is extra: say why
                km = {'profiler failed': repr(exc)}
            extra = ''
            if name == 'ds' and need_db and 'dq' in km:
                gbytes = B * h * (Lq * Lk + Lk * d + Lq * d) * 2 / 1e9
                extra = f"  dq_stream={gbytes / (km['dq'] / 1e3):.0f} GB/s"
            ks = ' '.join(f"{f}={t:.3f}" if isinstance(t, float)
                          else f"{f}: {t}" for f, t in sorted(km.items()))
            print(f"{label:8s} {name:7s} {med:8.3f} {ts[0]:8.3f} "
                  f"{ts[-1]:8.3f} {gb / (med / 1e3):6.1f}   {ks}{extra}",
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dropout', type=float, default=0.,
                    help='A/B the fused dropout kernels against the fused '
                         'no-dropout kernels and the eager composition')
    ap.add_argument('--eager-batch', type=int, default=128,
                    help='folded batch rows the eager composition runs on')
    ap.add_argument('--ds-ab', action='store_true',
                    help='A/B the backward: float-atomic dBias against the '
                         'stored-dS path, alternating in one process')
    ap.add_argument('--rounds', type=int, default=3,
                    help='--ds-ab: alternations per shape')
    ap.add_argument('--iters', type=int, default=10,
                    help='--ds-ab: timed calls per alternation')
    args = ap.parse_args()
    ext = _load_ext()
    assert ext is not None
    if args.ds_ab:
        return ds_ab(ext, args.rounds, args.iters)
    if args.dropout > 0.:
        return dropout_ab(ext, args.dropout, args.eager_batch)
    h, d = 8, 64
    print(f"{'shape':8s} {'fwd_ms':>8s} {'fwd_TF':>7s} {'bwd_ms':>8s} {'bwd_TF':>7s}")
    for label, B, Lq, Lk, brep in attn_shapes():
        mk = lambda *s: torch.randn(*s, device='cuda', dtype=torch.bfloat16)
        q, k, v = mk(B, h, Lq, d), mk(B, h, Lk, d), mk(B, h, Lk, d)
        bias = mk(B // brep, h, Lq, Lk) if brep else None
        scale = d ** -0.5
        out, lse = ext.attn_fwd(q, k, v, bias, None, brep or 1, scale)
        dout = mk(B, h, Lq, d)

        fwd = lambda: ext.attn_fwd(q, k, v, bias, None, brep or 1, scale)
        bwd = lambda: ext.attn_bwd(dout, q, k, v, out, lse, bias, None,
                                   brep or 1, scale, bias is not None)
        t_f = time_fn(fwd)
        t_b = time_fn(bwd, iters=15)
        gf = 4e-12 * B * h * Lq * Lk * d
        gb = 10e-12 * B * h * Lq * Lk * d  # 5 matmul-equivalents
        print(f"{label:8s} {t_f:8.3f} {gf / (t_f / 1e3):7.1f} "
              f"{t_b:8.3f} {gb / (t_b / 1e3):7.1f}")

    # pcgemm: trimul fwd shape at b=5, n=256, d=256
    b, n, D = 5, 256, 256
    L = torch.randn(b, n, n, D, device='cuda', dtype=torch.bfloat16)
    R = torch.randn(b, n, n, D, device='cuda', dtype=torch.bfloat16)
    f = lambda: _pcg(L, R, n, n, n, 1, 2, 1, 2)
    t = time_fn(f, iters=20)
    tf = (2e-12 * b * n * n * n * D) / (t / 1e3)
    print(f"{'pcgemm':8s} {t:8.3f} {tf:7.1f}")
    # einsum comparison
    g = lambda: torch.einsum('bikd,bjkd->bijd', L, R)
    t2 = time_fn(g, iters=20)
    tf2 = (2e-12 * b * n * n * n * D) / (t2 / 1e3)
    print(f"{'einsum':8s} {t2:8.3f} {tf2:7.1f}")


if __name__ == '__main__':
    main()
