"""A/B of the template pointwise attention kernels (K5) against the path
they replace, at the user-sized shape (b=1, P=256^2, T=4, H=8, bf16, head
dim 64 and again 32).  Run on an MI355X:

    python tools/tplattn_bench.py

Legs, alternating in one process, `--rounds` times, each figure the mean
of `--iters` calls after warmup:

* new:   ops.template_pointwise_attention (the pointwise kernels)
* off:   the same call with AF2AMD_TEMPLATE_POOL_FUSED=0: from the same
         q / kv, the fold to (b*P, H, 1|T, d) with the permute copy it
         needs, then the flash kernels (with their pad at d < 64)
* flash: the flash kernels alone on operands folded beforehand, for
         reference: the model's own switch-off path permutes the
         templates before to_kv (a dim-wide copy) instead of kv

Reported: forward, forward + backward, backward alone; the bytes each leg
must move, counted from shapes; the achieved TB/s of the new kernels.
Then a whole training step of the model with templates (flagship dims, 4
templates, `--steps` steps) with the switch on and off.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from alphafold2_amd import ops
from alphafold2_amd.ops import dispatch

SWITCH = 'AF2AMD_TEMPLATE_POOL_FUSED'


def time_fn(fn, iters, warmup=5):
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


def with_switch(on, fn, *args, **kwargs):
    prev = os.environ.get(SWITCH)
    os.environ[SWITCH] = '1' if on else '0'
    try:
        return fn(*args, **kwargs)
    finally:
        if prev is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = prev


def op_legs(b, P, T, H, d):
    g = torch.Generator(device='cuda').manual_seed(0)

    def randn(*s):
        return torch.randn(*s, device='cuda', generator=g,
                           dtype=torch.float32).to(torch.bfloat16)

    C = H * d
    q = randn(b, P, C).requires_grad_(True)
    kv = randn(b, T, P, 2 * C).requires_grad_(True)
    w = randn(b, P, C)
    key_mask = torch.ones(b, T, P, dtype=torch.bool, device='cuda')
    key_mask[:, T - 1, P // 2:] = False
    query_mask = torch.ones(b, P, dtype=torch.bool, device='cuda')
    assert dispatch.template_pool_fusable(
        q, kv, heads=H, dim_head=d, num_templates=T, drop_p=0.)

    def op():
        return ops.template_pointwise_attention(
            q, kv, H, key_mask=key_mask, query_mask=query_mask)

    # the flash kernels alone: operands folded once, outside the timing
    with torch.no_grad():
        qf = q.reshape(b * P, 1, H, d).transpose(1, 2)
        kf, vf = (t.permute(0, 2, 1, 3).reshape(b * P, T, H, d)
                  .transpose(1, 2) for t in kv.chunk(2, dim=-1))
        kmf = key_mask.permute(0, 2, 1).reshape(b * P, T).contiguous()
    qf, kf, vf = (t.detach().requires_grad_(True) for t in (qf, kf, vf))
    wf = w.reshape(b * P, 1, H, d).transpose(1, 2)

    def flash():
        return ops.attention_core(qf, kf, vf, context_mask=kmf)

    def legs(fwd, leaves, up):
        def f():
            with torch.no_grad():
                fwd()

        def fb():
            torch.autograd.grad(fwd(), leaves, up)

        return f, fb

    return {'new': (True, *legs(op, (q, kv), w)),
            'off': (False, *legs(op, (q, kv), w)),
            'flash': (False, *legs(flash, (qf, kf, vf), wf))}


def bytes_moved(b, P, T, H, d):
    """Bytes each leg must move, from shapes (bf16).  U = one q-sized
    tensor.  new: forward reads q and T x (k, v) and writes out; backward
    reads q, out, dout and T x (k, v) and writes dq and T x (dk, dv).
    The flash kernels move the same operands, padded to 64 channels when
    d < 64 (pad and slice are copies of their own, forward and backward);
    'off' adds the permute copy of k and v and its backward."""
    U = b * P * H * d * 2
    pad = 64 / d
    new_f, new_b = (2 + 2 * T) * U, (4 + 4 * T) * U
    flash_f, flash_b = new_f * pad, new_b * pad
    if d < 64:
        # F.pad of q, k, v (read U-sized, write padded), slice of out
        # stays a view; backward of the pad reads padded, writes U-sized
        flash_f += (1 + 2 * T) * U * (1 + pad)
        flash_b += (1 + 2 * T) * U * (1 + pad)
    off_f = flash_f + 2 * (2 * T) * U
    off_b = flash_b + 2 * (2 * T) * U
    return {'new': (new_f, new_b), 'flash': (flash_f, flash_b),
            'off': (off_f, off_b)}


def bench_op(b, P, T, H, d, rounds, iters):
    legs = op_legs(b, P, T, H, d)
    nbytes = bytes_moved(b, P, T, H, d)
    print(f'TPL_BENCH shape b={b} P={P} T={T} H={H} d={d} bf16, mean of '
          f'{iters} calls')
    for name, (f, bw) in nbytes.items():
        print(f'TPL_BENCH d={d} bytes {name}: fwd={f / 1e9:.3f} GB '
              f'bwd={bw / 1e9:.3f} GB')
    for r in range(rounds):
        for name, (on, f, fb) in legs.items():
            t_f = with_switch(on, time_fn, f, iters)
            t_fb = with_switch(on, time_fn, fb, iters)
            line = (f'TPL_BENCH d={d} round={r} {name}: fwd={t_f:.3f} ms '
                    f'fwd+bwd={t_fb:.3f} ms bwd={t_fb - t_f:.3f} ms')
            if name == 'new':
                nf, nb = nbytes['new']
                line += (f' | fwd {nf / t_f / 1e9:.2f} TB/s, bwd '
                         f'{nb / (t_fb - t_f) / 1e9:.2f} TB/s')
            print(line, flush=True)


def bench_model(args):
    from alphafold2_amd import Alphafold2
    from alphafold2_amd.data import synthetic_batch
    torch.manual_seed(0)
    model = Alphafold2(dim=args.dim, depth=args.depth, heads=args.heads,
                       dim_head=args.dim_head,
                       max_seq_len=max(2048, args.crop_len)).cuda().train()
    # to_out starts at zero: give the pooling an effect and a gradient
    torch.nn.init.normal_(model.template_pointwise_attn.to_out.weight,
                          std=0.02)
    b, n, T = args.batch, args.crop_len, args.templates
    batch = synthetic_batch(b, n, args.msa_depth, device='cuda', seed=42)
    g = torch.Generator(device='cuda').manual_seed(1)
    tf = torch.randn(b, T, n, n, 32, device='cuda', generator=g)
    tm = torch.ones(b, T, n, dtype=torch.bool, device='cuda')
    tm[:, T - 1, n - n // 8:] = False

    def step():
        model.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            ret = model(batch['seq'], batch['msa'], mask=batch['mask'],
                        msa_mask=batch['msa_mask'], templates_feats=tf,
                        templates_mask=tm)
            loss = ret.distance.float().pow(2).mean() \
                + ret.msa_mlm_loss.float()
        loss.backward()

    print(f'TPL_BENCH model dim={args.dim} depth={args.depth} '
          f'heads={args.heads} dim_head={args.dim_head} crop={n} '
          f'msa={args.msa_depth} batch={b} templates={T}, bf16 autocast, '
          f'eager launches, mean of {args.steps} steps')
    for r in range(args.rounds):
        for name, on in (('new', True), ('off', False)):
            t = with_switch(on, time_fn, step, args.steps, warmup=2)
            print(f'TPL_BENCH model round={r} {name}: step={t:.1f} ms',
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--crop-len', type=int, default=256)
    ap.add_argument('--templates', type=int, default=4)
    ap.add_argument('--heads', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--steps', type=int, default=10,
                    help='steps of the whole-model leg (0 = skip)')
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--depth', type=int, default=12)
    ap.add_argument('--dim-head', type=int, default=64)
    ap.add_argument('--msa-depth', type=int, default=128)
    ap.add_argument('--batch', type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    assert dispatch.hip_ops_available()

    P = args.crop_len ** 2
    for d in (64, 32):
        bench_op(1, P, args.templates, args.heads, d, args.rounds,
                 args.iters)
        torch.cuda.empty_cache()
    if args.steps:
        bench_model(args)


if __name__ == '__main__':
    main()
