"""Fused IPA core (K7) in training: forward + backward parity against
the eager module in float64, padding masks, reachability from the
model's own configurations, hipGraph capture (no host sync) and the LDS
bound.

Reference: the eager composition (`dispatch._FORCE_EAGER`) in float64 on
the same device.  Each case also runs the eager module in fp32; its
error against fp64 is the yardstick, printed next to the fused error.
Errors are relative to the reference gradient's max-abs.

Gradient tolerances are ten times the eager-fp32 error measured on an
MI355X at these shapes (docs/KERNELS.md, K7 section); the forward
tolerance is the project's 1e-4 absolute on the module output.
"""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4

# largest eager-fp32-vs-fp64 error (relative to max-abs) measured on the
# MI355X over the six bare-module cases of this file, per gradient
EAGER_FP32_ERR = {
    'point_weights': 1.07e-6,
    'to_scalar_q.weight': 9.5e-7,
    'to_scalar_k.weight': 9.5e-7,
    'to_scalar_v.weight': 6.4e-7,
    'to_point_q.weight': 6.4e-7,
    'to_point_k.weight': 6.9e-7,
    'to_point_v.weight': 6.7e-7,
    'to_pairwise_attn_bias.0.weight': 1.66e-6,
    'to_pairwise_attn_bias.0.bias': 9.4e-8,
    'to_out.weight': 6.6e-7,
    'to_out.bias': 1.7e-7,
    'x': 5.7e-7,
    'pair': 6.9e-7,
    'rotations': 4.1e-7,
    'translations': 4.7e-7,
}
# ten times that; the other IPABlock parameters (norms, transition), which
# the model case also compares, get ten times the largest entry
GRAD_TOL = {k: 10 * v for k, v in EAGER_FP32_ERR.items()}
GRAD_TOL['default'] = 10 * max(EAGER_FP32_ERR.values())

# sum_j dL[h, j] == 0 for every softmax row, so the bias Linear's bias
# gradient is rounding noise around zero in every leg; it is judged
# against the scale of that Linear's weight gradient instead of its own
_ZERO_SUM = 'to_pairwise_attn_bias.0.bias'
_ZERO_SUM_SCALE = 'to_pairwise_attn_bias.0.weight'


def _tol(name):
    return GRAD_TOL.get(name, GRAD_TOL['default'])


def _inputs(b, n, d, seed):
    """randn x / pair / translations and QR-orthonormalised proper
    rotations, drawn as test_ipa_fused_core_parity does."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(b, n, d, device='cuda', generator=g)
    pair = torch.randn(b, n, n, d, device='cuda', generator=g)
    a = torch.randn(b, n, 3, 3, device='cuda', generator=g)
    q, _ = torch.linalg.qr(a)
    q[..., 0] = q[..., 0] * torch.det(q)[..., None]
    t = torch.randn(b, n, 3, device='cuda', generator=g)
    w = torch.randn(b, n, d, device='cuda', generator=g)
    return x, pair, q, t, w


def _run_ipa(state, heads, d, inputs, mask, leg):
    """One forward + backward of a bare InvariantPointAttention in train
    mode.  leg: 'fused' (fp32, dispatch as shipped), 'eager32' or
    'eager64' (both with _FORCE_EAGER).  Returns (out, grads) in fp64."""
    from alphafold2_amd.models.ipa import InvariantPointAttention
    from alphafold2_amd.ops import dispatch

    dtype = torch.float64 if leg == 'eager64' else torch.float32
    prev = dispatch._FORCE_EAGER
    dispatch._FORCE_EAGER = leg != 'fused'
    try:
        ipa = InvariantPointAttention(dim=d, heads=heads)
        ipa.load_state_dict(state)
        ipa = ipa.cuda().to(dtype).train()
        # fresh leaves per leg: .to() of an fp32 tensor is the tensor itself
        x, pair, rot, t, w = (v.detach().to(dtype).clone() for v in inputs)
        leaves = {'x': x, 'pair': pair, 'rotations': rot,
                  'translations': t}
        for v in leaves.values():
            v.requires_grad_(True)
        out = ipa(x, pair, rotations=rot, translations=t, mask=mask)
        (out * w).sum().backward()
        grads = {k: p.grad.double() for k, p in ipa.named_parameters()}
        grads.update({k: v.grad.double() for k, v in leaves.items()})
        return out.detach().double(), grads
    finally:
        dispatch._FORCE_EAGER = prev


def _rel_errors(grads, ref):
    errs = {}
    for k, r in ref.items():
        scale = ref[_ZERO_SUM_SCALE] if k == _ZERO_SUM else r
        errs[k] = ((grads[k] - r).abs().max()
                   / scale.abs().max().clamp_min(1e-30)).item()
    return errs


def _check_case(tag, b, n, heads, d, mask, expect_nonzero=True):
    from alphafold2_amd.models.ipa import InvariantPointAttention
    torch.manual_seed(0)
    state = InvariantPointAttention(dim=d, heads=heads).state_dict()
    # softplus(point_weights) = 1 on every head at init; spread the heads
    # so a per-head indexing slip cannot hide behind equal weights
    state['point_weights'] = state['point_weights'] \
        + torch.linspace(-0.5, 0.5, heads)
    inputs = _inputs(b, n, d, seed=1)

    out64, g64 = _run_ipa(state, heads, d, inputs, mask, 'eager64')
    out32, g32 = _run_ipa(state, heads, d, inputs, mask, 'eager32')
    outf, gf = _run_ipa(state, heads, d, inputs, mask, 'fused')

    fwd_eager = (out32 - out64).abs().max().item()
    fwd_fused = (outf - out64).abs().max().item()
    e_eager = _rel_errors(g32, g64)
    e_fused = _rel_errors(gf, g64)
    print(f'IPA_ERR {tag} forward abs: eager32={fwd_eager:.3e} '
          f'fused={fwd_fused:.3e} tol={FWD_TOL:.1e}')
    for k in g64:
        print(f'IPA_ERR {tag} {k}: eager32={e_eager[k]:.3e} '
              f'fused={e_fused[k]:.3e} tol={_tol(k):.1e}')

    assert torch.isfinite(outf).all()
    assert fwd_fused < FWD_TOL, fwd_fused
    for k in g64:
        assert torch.isfinite(gf[k]).all(), k
        if expect_nonzero and k != _ZERO_SUM:
            assert g64[k].abs().max().item() > 0, k
        assert e_fused[k] < _tol(k), (k, e_fused[k], _tol(k))
    return outf, out64


@pytest.mark.parametrize('b,n,heads,d', [
    (2, 37, 8, 64),     # less than one wave of columns
    (1, 70, 1, 128),    # crosses a wave boundary, the model's head count
    (1, 300, 8, 256),   # n > block size: every strided loop runs twice
    (1, 70, 2, 384),    # pair dim > block size
])
def test_core_forward_backward_parity(b, n, heads, d):
    _check_case(f'core({b},{n},{heads},{d})', b, n, heads, d, None)


def test_masked_padded_tail():
    """Batch entry 0 has its last 5 positions padded, entry 1 is all
    true.  Parity holds on every row; padded rows are finite and equal
    eager's uniform-attention result."""
    b, n = 2, 37
    mask = torch.ones(b, n, dtype=torch.bool, device='cuda')
    mask[0, -5:] = False
    outf, out64 = _check_case('mask_tail', b, n, 8, 64, mask)
    pad_err = (outf[0, -5:] - out64[0, -5:]).abs().max().item()
    assert pad_err < FWD_TOL, pad_err


def test_masked_single_valid_position():
    b, n = 1, 70
    mask = torch.zeros(b, n, dtype=torch.bool, device='cuda')
    mask[0, 11] = True
    # a one-hot softmax row has dL == 0 exactly, so the logit-side
    # gradients (q/k projections, bias Linear, point weights) are zero in
    # every leg; the value-side ones are not
    _check_case('mask_single', b, n, 1, 128, mask, expect_nonzero=False)


def _count_core_calls(monkeypatch):
    from alphafold2_amd.ops import hip_autograd
    calls = []
    real = hip_autograd.hip_ipa_core

    def counted(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(hip_autograd, 'hip_ipa_core', counted)
    return calls


def test_fused_core_reachable_in_training(monkeypatch):
    """heads=1 (the model's default), grad enabled and a padded mask:
    the fused core is taken, and the backward kernel exists."""
    from alphafold2_amd.models.ipa import InvariantPointAttention
    from alphafold2_amd.ops import dispatch

    ext = dispatch._load_ext()
    assert hasattr(ext, 'ipa_core_bwd')
    calls = _count_core_calls(monkeypatch)

    b, n, d = 1, 37, 64
    torch.manual_seed(0)
    ipa = InvariantPointAttention(dim=d, heads=1).cuda().train()
    x, pair, rot, t, w = _inputs(b, n, d, seed=2)
    x.requires_grad_(True)
    mask = torch.ones(b, n, dtype=torch.bool, device='cuda')
    mask[0, -4:] = False
    with torch.enable_grad():
        out = ipa(x, pair, rotations=rot, translations=t, mask=mask)
    (out * w).sum().backward()
    assert len(calls) == 1
    assert x.grad is not None and torch.isfinite(x.grad).all()
    assert ipa.to_point_k.weight.grad.abs().max().item() > 0


def test_through_the_model():
    """Alphafold2 at its default structure_module_heads=1: coords and
    every ipa_block gradient, fused vs _FORCE_EAGER."""
    from alphafold2_amd import Alphafold2
    from alphafold2_amd.data import synthetic_batch
    from alphafold2_amd.ops import dispatch

    kwargs = dict(dim=64, depth=1, heads=2, dim_head=32,
                  predict_coords=True, structure_module_depth=2)
    torch.manual_seed(0)
    model = Alphafold2(**kwargs)
    # init_zero_ leaves to_out at zero, which makes every core gradient
    # exactly zero: give it weights so the comparison is not vacuous
    torch.manual_seed(3)
    torch.nn.init.normal_(model.ipa_block.attn.to_out.weight, std=0.02)
    state = model.state_dict()

    batch = synthetic_batch(1, 32, 4, device='cuda', seed=0)
    mask = batch['mask'].clone()
    mask[:, 26:] = False
    msa_mask = batch['msa_mask'].clone()
    msa_mask[:, :, 26:] = False
    w = torch.randn(1, 32, 3, device='cuda',
                    generator=torch.Generator('cuda').manual_seed(4))

    def run(force_eager):
        prev = dispatch._FORCE_EAGER
        dispatch._FORCE_EAGER = force_eager
        try:
            m = Alphafold2(**kwargs)
            m.load_state_dict(state)
            m = m.cuda().float().train()
            # train mode draws the MSA masking noise: same draw in both legs
            torch.manual_seed(7)
            coords = m(batch['seq'], batch['msa'], mask=mask,
                       msa_mask=msa_mask)
            (coords * w).sum().backward()
            grads = {k: p.grad.double()
                     for k, p in m.ipa_block.named_parameters()}
            return coords.detach().double(), grads
        finally:
            dispatch._FORCE_EAGER = prev

    c_f, g_f = run(False)
    c_e, g_e = run(True)
    c_err = (c_f - c_e).abs().max().item()
    print(f'IPA_ERR model coords abs: fused-vs-eager={c_err:.3e} '
          f'tol={FWD_TOL:.1e}')
    errs = {}
    for k, r in g_e.items():
        name = k[len('attn.'):] if k.startswith('attn.') else k
        scale = g_e['attn.' + _ZERO_SUM_SCALE] if name == _ZERO_SUM else r
        errs[k] = ((g_f[k] - r).abs().max()
                   / scale.abs().max().clamp_min(1e-30)).item()
        print(f'IPA_ERR model {k}: fused-vs-eager={errs[k]:.3e} '
              f'tol={_tol(name):.1e}')
    assert g_e['attn.to_pairwise_attn_bias.0.weight'].abs().max() > 0
    assert g_e['attn.to_point_k.weight'].abs().max() > 0
    assert g_f['attn.to_pairwise_attn_bias.0.weight'].abs().max() > 0
    assert g_f['attn.to_point_k.weight'].abs().max() > 0
    assert c_err < FWD_TOL, c_err
    for k in g_e:
        name = k[len('attn.'):] if k.startswith('attn.') else k
        assert errs[k] < _tol(name), (k, errs[k], _tol(name))


def test_no_host_sync_under_graph_capture():
    """One IPABlock forward + backward with a padded mask captures into
    a hipGraph (a host sync in the gate would make capture raise) and
    the replay reproduces the uncaptured result."""
    from alphafold2_amd.models.ipa import IPABlock
    from alphafold2_amd.runtime.graphed import GraphedTrainStep

    b, n, d = 1, 37, 64
    torch.manual_seed(0)
    block = IPABlock(dim=d, heads=1).cuda().train()
    x, pair, rot, t, w = _inputs(b, n, d, seed=5)
    mask = torch.ones(b, n, dtype=torch.bool, device='cuda')
    mask[0, -6:] = False
    params = list(block.parameters())

    def step():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()
        out = block(x, pairwise_repr=pair, rotations=rot, translations=t,
                    mask=mask)
        loss = (out * w).sum()
        loss.backward()
        return loss

    loss_ref = step().detach().clone()
    grads_ref = [p.grad.clone() for p in params]
    torch.cuda.synchronize()

    graphed = GraphedTrainStep(step, warmup=2, fallback=False)
    assert graphed.graphed
    for p in params:
        p.grad.fill_(float('nan'))      # the replay must rewrite them
    loss = graphed()
    torch.cuda.synchronize()
    torch.testing.assert_close(loss, loss_ref, rtol=1e-5, atol=1e-6)
    for p, g in zip(params, grads_ref):
        torch.testing.assert_close(p.grad, g, rtol=1e-5, atol=1e-6)


def _bwd_row_lds_bytes(heads, n, pair_dim):
    # mirrors bwd_row_lds_bytes in ops/hip/ipacore.hip
    return 4 * (heads * pair_dim + 2 * heads * n + 4 * heads * 12
                + heads * 16 + 4 * heads)


def test_lds_bound_falls_back_to_eager(monkeypatch):
    from alphafold2_amd.models.ipa import InvariantPointAttention
    from alphafold2_amd.ops import dispatch

    ext = dispatch._load_ext()
    # the bound is the last n whose row-side backward fits the device:
    # never beyond the 160 KiB of LDS a gfx950 CU has, never below what
    # the device reports as usable by any block
    n8 = ext.ipa_core_max_n(8)
    lds_basic = torch.cuda.get_device_properties(0).shared_memory_per_block
    print(f'IPA_LDS max_n(8)={n8} max_n(1)={ext.ipa_core_max_n(1)} '
          f'shared_memory_per_block={lds_basic}')
    assert _bwd_row_lds_bytes(8, n8, 512) <= 160 * 1024
    assert _bwd_row_lds_bytes(8, n8 + 1, 512) > lds_basic
    assert ext.ipa_core_max_n(1) > n8
    assert ext.ipa_core_max_n(8, 64) > n8

    b, n, d = 1, 37, 64
    torch.manual_seed(0)
    ipa = InvariantPointAttention(dim=d, heads=8).cuda().train()
    x, pair, rot, t, _ = _inputs(b, n, d, seed=6)

    def run():
        return ipa(x, pair, rotations=rot, translations=t).detach()

    prev = dispatch._FORCE_EAGER
    dispatch._FORCE_EAGER = True
    try:
        out_eager = run()
    finally:
        dispatch._FORCE_EAGER = prev

    monkeypatch.setattr(ext, 'ipa_core_max_n', lambda *a, **k: n - 1)
    calls = _count_core_calls(monkeypatch)
    dispatch._warned.difference_update(
        {k for k in dispatch._warned if k[0] == 'ipa_core'})
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        out = run()
    assert len(calls) == 0
    assert any('ipa_core' in str(c.message) and 'LDS' in str(c.message)
               for c in caught), [str(c.message) for c in caught]
    torch.testing.assert_close(out, out_eager, rtol=0, atol=0)
