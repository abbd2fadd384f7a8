#!/usr/bin/env python3
"""Flagship training benchmark — driver contract.

Measures the BASELINE.json headline metric: training samples/sec of the
Evoformer trunk (distogram objective) at crop_len=256, msa=128, depth=12,
dim=256 / heads 8 / dim_head 64 (the reference README's model config),
bf16 compute, synthetic data, random-init weights.

Single process per GPU; for --gpus N the driver launches this under
torch.distributed.run with one rank per GPU over RCCL.  `value` is the
whole-job aggregate samples/sec across all ranks (weak scaling: per-GPU
work fixed as N grows).

A plain run does only what the headline figure needs: set up, warm up,
time --steps steps, print the JSON result line.  --dump-outputs DIR
additionally writes the last timed step's outputs as .npy files;
--full adds the secondary figures (peak HBM).
"""
import argparse
import json
import os
import time

import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument('--gpus', type=int, default=1)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--dim', type=int, default=256)
    p.add_argument('--depth', type=int, default=12)
    p.add_argument('--crop-len', type=int, default=256)
    p.add_argument('--msa-depth', type=int, default=128)
    p.add_argument('--batch', type=int, default=6,
                   help='per-GPU batch size (6 fills ~210 GB of the '
                        '288 GB HBM3E without activation checkpointing; '
                        'measured the within-box throughput optimum: '
                        '7.59 samples/s vs 7.49 at b5, 7.55 at b7)')
    p.add_argument('--heads', type=int, default=8)
    p.add_argument('--dim-head', type=int, default=64)
    p.add_argument('--dtype', type=str, default='bf16',
                   choices=['bf16', 'fp32'])
    p.add_argument('--reversible', action='store_true',
                   help='use the reversible trunk execution mode')
    p.add_argument('--structure-module', type=str, default='none',
                   choices=['none', 'ipa', 'se3', 'egnn'],
                   help='BASELINE configs 4-5: train with coordinate '
                        'prediction through the given structure module '
                        '(adds a distance-matrix coord loss)')
    p.add_argument('--predict-angles', action='store_true',
                   help='add the theta/phi/omega anglegram heads + loss')
    p.add_argument('--structure-depth', type=int, default=4,
                   help='structure module refinement iterations')
    p.add_argument('--no-graph', action='store_true',
                   help='disable hipGraph step capture')
    p.add_argument('--checkpoint-blocks', action='store_true',
                   help='enable per-block activation checkpointing '
                        '(needed only when activations exceed HBM; '
                        'costs a full forward recompute)')
    p.add_argument('--checkpoint-ffs', action='store_true',
                   help='selective FF-only checkpointing: frees the '
                        '8x-dim GEGLU hiddens (the bulk of activation '
                        'memory) at a 2-GEMM recompute cost — pushes '
                        'per-GPU batch beyond 6')
    p.add_argument('--device', type=str, default=None)
    p.add_argument('--dump-outputs', type=str, default=None, metavar='DIR',
                   help='after the timed steps write what the last timed '
                        'step returned (loss, distogram logits, coords / '
                        'angle logits when predicted) as DIR/<name>.npy, '
                        'float32; inputs are seeded, so two builds can be '
                        'compared output for output')
    p.add_argument('--full', action='store_true',
                   help='also report what the headline figure does not '
                        'need (peak HBM of the step)')
    return p.parse_args()


# --dump-outputs writes at most this many bytes of array data in all
DUMP_BUDGET_BYTES = 60 * 10**6


def dump_outputs(dirname, tensors, budget=DUMP_BUDGET_BYTES):
    """Write each tensor as dirname/<name>.npy in float32.  The byte
    budget is shared smallest-first; a tensor larger than its share is
    written as a 1-D sample of its flattened values at sorted indices
    drawn without replacement from a generator seeded with 0, so the
    same shape always yields the same sample."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    arrays = sorted(((name, t.detach().float().cpu().numpy())
                     for name, t in tensors.items()),
                    key=lambda kv: kv[1].nbytes)
    left = budget
    for i, (name, a) in enumerate(arrays):
        share = left // (len(arrays) - i)
        if a.nbytes > share:
            idx = np.random.default_rng(0).choice(
                a.size, share // a.itemsize, replace=False)
            idx.sort()
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, name + '.npy'), a)
        left -= a.nbytes


def main():
    args = parse_args()

    from alphafold2_amd import Alphafold2
    from alphafold2_amd.data import synthetic_batch
    from alphafold2_amd.parallel import DataParallelEngine, init_distributed
    from alphafold2_amd.utils import get_bucketed_distance_matrix

    rank, world_size, local_rank = init_distributed()
    if args.device is not None:
        device = torch.device(args.device)
    elif torch.cuda.is_available():
        device = torch.device('cuda', local_rank)
        torch.cuda.set_device(device)
    else:
        device = torch.device('cpu')

    # hipBLASLt solution selection from the committed TunableOp cache
    # (measured +3.4% whole-step on gfx950; tuning stays OFF — unknown
    # shapes just use the default heuristics).  Opt out / take control
    # by setting PYTORCH_TUNABLEOP_ENABLED yourself.
    if device.type == 'cuda' \
            and os.environ.get('PYTORCH_TUNABLEOP_ENABLED') is None:
        tuned = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                             'alphafold2_amd', 'runtime',
                             'tunableop_gfx950.csv')
        if os.path.exists(tuned):
            torch.cuda.tunable.enable(True)
            torch.cuda.tunable.tuning_enable(False)
            torch.cuda.tunable.read_file(tuned)

    is_dist = world_size > 1 or os.environ.get('AF2AMD_FORCE_DIST') == '1'
    dist = torch.distributed if is_dist else None

    torch.manual_seed(1234 + rank)

    want_coords = args.structure_module != 'none'
    model = Alphafold2(
        dim=args.dim,
        depth=args.depth,
        heads=args.heads,
        dim_head=args.dim_head,
        max_seq_len=max(2048, args.crop_len),
        reversible=args.reversible,
        checkpoint_blocks=('ff' if args.checkpoint_ffs
                           else args.checkpoint_blocks),
        predict_coords=want_coords,
        predict_angles=args.predict_angles,
        structure_module_type=(args.structure_module if want_coords
                               else 'ipa'),
        structure_module_depth=args.structure_depth,
    ).to(device)
    model.train()

    engine = DataParallelEngine(model, bucket_cap_mb=64)

    # hipGraph capture of the whole step removes the launch-bound host
    # path (~260 ms/step at this config); capturable Adam required.
    # DDP steps capture too (RCCL collectives are hipGraph-capturable;
    # validated via the AF2AMD_FORCE_DIST single-GPU rehearsal) —
    # AF2AMD_GRAPH_DDP=0 opts out.
    use_graph = (device.type == 'cuda' and not args.no_graph
                 and (not is_dist
                      or os.environ.get('AF2AMD_GRAPH_DDP', '1') == '1'))
    try:
        # single fused multi-tensor Adam kernel (ROCm-supported)
        optimizer = torch.optim.Adam(model.parameters(), lr=3e-4,
                                     capturable=use_graph, fused=True)
    except (RuntimeError, ValueError):
        optimizer = torch.optim.Adam(model.parameters(), lr=3e-4,
                                     capturable=use_graph, foreach=True)

    use_bf16 = args.dtype == 'bf16' and device.type == 'cuda'

    batch = synthetic_batch(args.batch, args.crop_len, args.msa_depth,
                            device=device, seed=42 + rank)
    seq, msa = batch['seq'], batch['msa']
    mask, msa_mask = batch['mask'], batch['msa_mask']
    target = get_bucketed_distance_matrix(batch['coords'], mask)
    coords_target = batch['coords']
    target_dmat = torch.cdist(coords_target, coords_target) \
        if want_coords else None
    if args.predict_angles:
        from alphafold2_amd import constants
        gen = torch.Generator(device='cpu').manual_seed(24 + rank)
        angle_targets = {
            name: torch.randint(0, buckets,
                                (args.batch, args.crop_len, args.crop_len),
                                generator=gen).to(device)
            for name, buckets in (('theta', constants.THETA_BUCKETS),
                                  ('phi', constants.PHI_BUCKETS),
                                  ('omega', constants.OMEGA_BUCKETS))}

    # --dump-outputs: what the step hands back besides the loss, copied
    # into buffers of their own that every step overwrites.  Holding on
    # to the step's own tensors instead would change how the allocator
    # lays out the step's activations, and on MI355X that changed both
    # the step time (+3%) and the values of later steps; with the copies
    # the step allocates exactly what it does without the option.  The
    # buffers are allocated in the first (eager) step, so a captured
    # step only records the copies.
    outputs = {}

    def keep(name, t):
        if name not in outputs:
            outputs[name] = torch.empty_like(t)
        outputs[name].copy_(t.detach())

    def step():
        optimizer.zero_grad(set_to_none=not use_graph)
        if use_bf16:
            ctx = torch.autocast('cuda', dtype=torch.bfloat16,
                                 cache_enabled=not use_graph)
        else:
            import contextlib
            ctx = contextlib.nullcontext()
        with ctx:
            if want_coords:
                coords, ret = model(seq, msa, mask=mask, msa_mask=msa_mask,
                                    return_aux_logits=True)
            else:
                ret = model(seq, msa, mask=mask, msa_mask=msa_mask)
            logits = ret.distance.permute(0, 3, 1, 2)
            loss = torch.nn.functional.cross_entropy(
                logits.float(), target, ignore_index=-100)
            if ret.msa_mlm_loss is not None:
                loss = loss + ret.msa_mlm_loss.float()
            if want_coords:
                # alignment-free coordinate loss (distance-matrix MSE,
                # reference train_end2end intent) — graph-capturable,
                # no host-synced Kabsch in the hot loop
                pred_dmat = torch.cdist(coords.float(), coords.float())
                loss = loss + torch.nn.functional.smooth_l1_loss(
                    pred_dmat, target_dmat)
            if args.predict_angles:
                for name, tgt in angle_targets.items():
                    alog = getattr(ret, f'{name}_logits')
                    loss = loss + 0.1 * torch.nn.functional.cross_entropy(
                        alog.permute(0, 3, 1, 2).float(), tgt)
        if args.dump_outputs:
            keep('distance_logits', ret.distance)
            if want_coords:
                keep('coords', coords)
            if args.predict_angles:
                for name in angle_targets:
                    keep(f'{name}_logits', getattr(ret, f'{name}_logits'))
        loss.backward()
        engine.finalize()
        optimizer.step()
        return loss

    def sync(more_steps=False):
        if device.type == 'cuda':
            if more_steps and use_graph:
                # Known issue (README): a device or stream synchronize
                # BETWEEN two replays of the captured step leaves every
                # later replay with a NaN loss at the flagship config
                # (measured on MI355X / ROCm 7.0.2; a host sleep, or no
                # wait at all, does not).  Cause not found, so wait for
                # the warmup replays by polling an event instead.
                done = torch.cuda.Event()
                done.record()
                while not done.query():
                    time.sleep(0.001)
            else:
                torch.cuda.synchronize()
        if is_dist:
            dist.barrier()

    if use_graph:
        from alphafold2_amd.runtime import GraphedTrainStep
        graphed = GraphedTrainStep(step, warmup=max(2, args.warmup))
        if rank == 0:
            print(f"# hipGraph capture: {graphed.graphed}"
                  + (f" ({graphed.capture_error})" if not graphed.graphed
                     else ""), flush=True)
        step = graphed

    for _ in range(args.warmup):
        step()
    sync(more_steps=True)
    if args.full and rank == 0 and device.type == 'cuda':
        peak = torch.cuda.max_memory_allocated(device) / 2**30
        total = torch.cuda.get_device_properties(device).total_memory / 2**30
        print(f"# peak HBM: {peak:.1f} / {total:.0f} GiB", flush=True)

    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    sync()
    elapsed = time.perf_counter() - t0

    # each rank has its own inputs; rank 0's outputs are the ones written
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dict(outputs, loss=loss))

    # max over ranks = whole-job wall time
    if is_dist:
        t = torch.tensor([elapsed], device=device if device.type == 'cuda'
                         else 'cpu', dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()

    ms_per_step = elapsed / args.steps * 1000.0
    samples_per_sec = (args.batch * world_size * args.steps) / elapsed

    if rank == 0:
        print(json.dumps({
            "metric": "training samples/sec (crop_len=256, msa=128, depth=12)",
            "value": samples_per_sec,
            "unit": "samples/sec",
            "n_gpus": world_size,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {
                "model": f"alphafold2 evoformer dim={args.dim} depth={args.depth} "
                         f"heads={args.heads} dim_head={args.dim_head}"
                         + (" reversible" if args.reversible else "")
                         + (f" structure={args.structure_module}"
                            f"x{args.structure_depth}" if want_coords else "")
                         + (" angles" if args.predict_angles else ""),
                "global_batch": args.batch * world_size,
                "seq_len": args.crop_len,
                "msa_depth": args.msa_depth,
                "parallelism": f"dp{world_size}",
            },
        }))

    if is_dist:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
