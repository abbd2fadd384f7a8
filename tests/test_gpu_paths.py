"""GPU integration tests for the non-default execution paths:
reversible trunk, equivariant structure modules, hipGraph capture."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_reversible_trunk_gpu_bf16():
    from alphafold2_amd import Alphafold2
    from alphafold2_amd.data import synthetic_batch
    torch.manual_seed(0)
    model = Alphafold2(dim=64, depth=2, heads=2, dim_head=32,
                       reversible=True).cuda().train()
    b = synthetic_batch(1, 48, 8, device='cuda', seed=0)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        ret = model(b['seq'], b['msa'], mask=b['mask'], msa_mask=b['msa_mask'])
        loss = ret.distance.float().pow(2).mean() + ret.msa_mlm_loss.float()
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    n_grads = sum(1 for p in model.parameters() if p.grad is not None)
    assert n_grads > 50


@pytest.mark.parametrize("kind", ["egnn", "se3"])
def test_equivariant_structure_gpu(kind):
    from alphafold2_amd import Alphafold2
    from alphafold2_amd.data import synthetic_batch
    torch.manual_seed(0)
    model = Alphafold2(dim=64, depth=1, heads=2, dim_head=32,
                       predict_coords=True, structure_module_type=kind,
                       structure_module_depth=2).cuda().train()
    b = synthetic_batch(1, 32, 4, device='cuda', seed=0)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        coords, ret = model(b['seq'], b['msa'], mask=b['mask'],
                            msa_mask=b['msa_mask'], return_aux_logits=True)
        loss = coords.float().pow(2).mean() + ret.msa_mlm_loss.float()
    loss.backward()
    torch.cuda.synchronize()
    assert coords.shape == (1, 32, 3)
    assert torch.isfinite(loss)


def test_graphed_train_step():
    from alphafold2_amd import Alphafold2
    from alphafold2_amd.data import synthetic_batch
    from alphafold2_amd.runtime import GraphedTrainStep
    from alphafold2_amd.utils import get_bucketed_distance_matrix
    torch.manual_seed(0)
    model = Alphafold2(dim=64, depth=2, heads=2, dim_head=64,
                       checkpoint_blocks=False).cuda().train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True,
                           foreach=True)
    b = synthetic_batch(1, 64, 8, device='cuda', seed=0)
    tgt = get_bucketed_distance_matrix(b['coords'], b['mask'])

    def step():
        opt.zero_grad(set_to_none=False)
        with torch.autocast('cuda', dtype=torch.bfloat16,
                            cache_enabled=False):
            ret = model(b['seq'], b['msa'], mask=b['mask'],
                        msa_mask=b['msa_mask'])
            loss = torch.nn.functional.cross_entropy(
                ret.distance.permute(0, 3, 1, 2).float(), tgt,
                ignore_index=-100)
        loss.backward()
        opt.step()
        return loss

    g = GraphedTrainStep(step, warmup=2)
    assert g.graphed, f"capture failed: {g.capture_error}"
    l0 = float(g())
    for _ in range(5):
        li = float(g())
    torch.cuda.synchronize()
    assert li < l0, "loss must decrease across graph replays (optimizer runs)"


def test_sidechain_builder_gpu():
    from alphafold2_amd.utils import sidechain_container
    torch.manual_seed(0)
    seqs = torch.randint(0, 20, (2, 64), device='cuda')
    bb = torch.randn(2, 64 * 4, 3, device='cuda', requires_grad=True)
    atom_mask = torch.tensor([1] * 4 + [0] * 10)
    out = sidechain_container(seqs, bb, atom_mask=atom_mask)
    assert out.shape == (2, 64, 14, 3)
    assert out.is_cuda
    out.sum().backward()
    assert torch.isfinite(bb.grad).all()


def test_templates_path_gpu():
    """Template cross-attention (Lq=1 pointwise) through the fused path."""
    from alphafold2_amd import Alphafold2
    torch.manual_seed(0)
    model = Alphafold2(dim=64, depth=1, heads=2, dim_head=64,
                       templates_dim=32,
                       templates_angles_feats_dim=32).cuda().train()
    seq = torch.randint(0, 21, (2, 16), device='cuda')
    mask = torch.ones_like(seq).bool()
    msa = torch.randint(0, 21, (2, 3, 16), device='cuda')
    msa_mask = torch.ones_like(msa).bool()
    tf = torch.randn(2, 3, 16, 16, 32, device='cuda')
    ta = torch.randn(2, 3, 16, 32, device='cuda')
    tm = torch.ones(2, 3, 16, device='cuda').bool()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        ret = model(seq, msa, mask=mask, msa_mask=msa_mask,
                    templates_feats=tf, templates_angles=ta,
                    templates_mask=tm)
        loss = ret.distance.float().pow(2).mean() + ret.msa_mlm_loss.float()
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)


def test_step_timer_and_trace(tmp_path):
    from alphafold2_amd.runtime import StepTimer, profile_trace
    t = StepTimer()
    x = torch.randn(512, 512, device='cuda')
    with profile_trace(str(tmp_path / 'trace.json')):
        for _ in range(3):
            with t:
                (x @ x).sum().item()
    s = t.summary()
    assert s['steps'] == 3 and s['mean_ms'] > 0
    assert (tmp_path / 'trace.json').exists()


def test_overfit_single_batch_gpu_bf16():
    """bf16 + HIP kernels end to end: overfit one batch on the GPU."""
    from alphafold2_amd import Alphafold2
    from alphafold2_amd.data import synthetic_batch
    from alphafold2_amd.utils import get_bucketed_distance_matrix
    torch.manual_seed(0)
    model = Alphafold2(dim=128, depth=2, heads=2, dim_head=64,
                       checkpoint_blocks=False).cuda().train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    b = synthetic_batch(1, 64, 8, device='cuda', seed=0)
    tgt = get_bucketed_distance_matrix(b['coords'], b['mask'])

    losses = []
    for _ in range(30):
        opt.zero_grad()
        with torch.autocast('cuda', dtype=torch.bfloat16):
            ret = model(b['seq'], b['msa'], mask=b['mask'],
                        msa_mask=b['msa_mask'])
            loss = torch.nn.functional.cross_entropy(
                ret.distance.permute(0, 3, 1, 2).float(), tgt,
                ignore_index=-100)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    torch.cuda.synchronize()
    assert losses[-1] < losses[0] * 0.7, (losses[0], losses[-1])


@pytest.mark.timeout(420)
def test_ddp_rccl_graph_rehearsal():
    """Single-GPU rehearsal of the multi-GPU driver path: a 1-rank RCCL
    process group with the full DDP engine (broadcast, bucketed async
    all-reduce, finalize) captured inside a hipGraph — validates the
    AF2AMD_GRAPH_DDP=1 default without a multi-GPU lease."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env['AF2AMD_FORCE_DIST'] = '1'
    env['MASTER_ADDR'] = '127.0.0.1'
    env['MASTER_PORT'] = '29517'
    out = subprocess.run(
        [sys.executable, 'bench.py', '--dim', '64', '--depth', '2',
         '--crop-len', '64', '--msa-depth', '16', '--batch', '1',
         '--steps', '3', '--warmup', '2'],
        cwd=root, capture_output=True, text=True, timeout=400, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert '# hipGraph capture: True' in out.stdout, out.stdout[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith('{')][-1]
    d = json.loads(line)
    assert d['value'] > 0


def test_padded_batch_hip_eager_parity():
    """End-to-end fwd+bwd on a PADDED batch, HIP ops vs forced eager.

    The model runs in fp32 WITHOUT autocast, and the fused attention
    kernel is bf16-only, so attention takes the eager composition in
    BOTH runs (dispatch warns about it): this test covers LayerNorm,
    gating, GEGLU and the other fp32-capable HIP ops on a padded batch,
    not the fused attention's "fully-masked rows output 0" deviation.
    That is covered by tests/test_attention_paths.py (kernel level and
    test_axial_attention_padded_runs_fused_kernel).  Parity is asserted
    at VALID positions, and the loss (masked downstream) must match."""
    import os
    from alphafold2_amd import Alphafold2
    from alphafold2_amd.ops import dispatch

    torch.manual_seed(0)
    model = Alphafold2(dim=64, depth=2, heads=2, dim_head=64).cuda()
    model.train()
    seq = torch.randint(0, 21, (2, 48), device='cuda')
    msa = torch.randint(0, 21, (2, 6, 48), device='cuda')
    mask = torch.ones(2, 48, dtype=torch.bool, device='cuda')
    mask[0, 37:] = False                       # padded tail, item 0
    msa_mask = torch.ones(2, 6, 48, dtype=torch.bool, device='cuda')
    msa_mask[0, 4:] = False                    # padded MSA rows, item 0
    msa_mask[0, :, 37:] = False

    def run(force_eager):
        prev = dispatch._FORCE_EAGER
        dispatch._FORCE_EAGER = force_eager
        try:
            torch.manual_seed(7)
            m = Alphafold2(dim=64, depth=2, heads=2, dim_head=64)
            m.load_state_dict(model.state_dict())
            m = m.cuda().float().train()
            ret = m(seq, msa, mask=mask, msa_mask=msa_mask)
            valid = mask[:, :, None] & mask[:, None, :]
            loss = ret.distance[valid].float().pow(2).mean()
            loss.backward()
            g = torch.cat([p.grad.reshape(-1) for p in m.parameters()
                           if p.grad is not None])
            return ret.distance.detach(), loss.detach(), g
        finally:
            dispatch._FORCE_EAGER = prev

    d_hip, l_hip, g_hip = run(False)
    d_eag, l_eag, g_eag = run(True)

    valid = (mask[:, :, None] & mask[:, None, :])
    dv = (d_hip[valid] - d_eag[valid]).abs().max().item()
    assert dv < 5e-2, dv
    assert (l_hip - l_eag).abs().item() < 1e-3 * (1 + l_eag.abs().item())
    denom = g_eag.abs().max().item() + 1e-6
    assert (g_hip - g_eag).abs().max().item() / denom < 6e-2


def test_ipa_fused_core_parity():
    """K7 inference path: the fused fp32 IPA core matches the eager
    einsum composition exactly (same module, grad on vs off)."""
    from alphafold2_amd.models.ipa import InvariantPointAttention
    torch.manual_seed(0)
    b, n, d = 2, 64, 256
    ipa = InvariantPointAttention(dim=d, heads=8).cuda().float().eval()
    x = torch.randn(b, n, d, device='cuda')
    pair = torch.randn(b, n, n, d, device='cuda')
    # proper rotations
    a = torch.randn(b, n, 3, 3, device='cuda')
    q, _ = torch.linalg.qr(a)
    det = torch.det(q)
    q[..., 0] = q[..., 0] * det[..., None]
    t = torch.randn(b, n, 3, device='cuda')

    with torch.no_grad():
        out_fused = ipa(x, pair, rotations=q, translations=t)
    with torch.enable_grad():
        out_eager = ipa(x, pair, rotations=q, translations=t)
    err = (out_fused - out_eager).abs().max().item()
    assert err < 1e-4, err

    # masked / grad-enabled configs fall back (no crash, same result)
    mask = torch.ones(b, n, dtype=torch.bool, device='cuda')
    with torch.no_grad():
        out_m = ipa(x, pair, rotations=q, translations=t, mask=mask)
    assert (out_m - out_eager).abs().max().item() < 1e-4
