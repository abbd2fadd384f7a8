"""Fused EGNN edge-message core (K16): forward + backward parity against
the eager layer in float64, pair masks, the gate's fallbacks, reachability
from the model, hipGraph capture, what the forward keeps, and the
unchanged CPU path.

Reference: the eager layer (`dispatch._FORCE_EAGER`) in float64 on the
same device.  Each case also runs the eager layer in fp32; its error
against fp64 is the yardstick, printed next to the fused error as
`EGNN_ERR` lines.  Errors are relative to the reference's max-abs.

Gradient tolerances are ten times the largest eager-fp32 error measured
on an MI355X over the bare-layer cases of this file (docs/KERNELS.md, K16
section); the forward tolerance is the project's 1e-4 absolute.  The `x`
gradient is the exception: eager's own error there (EAGER_FP32_X_ERR) is
the diagonal cancellation of +-u/sqrt(eps), which the fused backward
skips, so `x` is held to ten times the largest eager error among the
other gradients.

The kernels stage the whole first-layer edge weight in LDS, which covers
edge dims 64 to 256; 384 is therefore a fallback case here, not a parity
case.  They tile the keys, so there is no bound on n to test.
"""
import json
import os
import warnings

import pytest
import torch

gpu = pytest.mark.gpu

FWD_TOL = 1e-4

# largest eager-fp32-vs-fp64 error (relative to max-abs) measured on the
# MI355X over the seven bare-layer cases of this file, per gradient
EAGER_FP32_ERR = {
    'edge_mlp.0.weight': 2.32e-6,
    'edge_mlp.0.bias': 6.47e-7,
    'edge_mlp.2.weight': 5.26e-6,
    'edge_mlp.2.bias': 6.66e-7,
    'node_mlp.0.weight': 6.39e-7,
    'node_mlp.0.bias': 5.07e-7,
    'node_mlp.2.weight': 4.73e-7,
    'node_mlp.2.bias': 1.36e-7,
    'coors_mlp.0.weight': 9.77e-6,
    'coors_mlp.0.bias': 1.93e-7,
    'coors_mlp.2.weight': 5.05e-6,
    'coors_mlp.2.bias': 1.41e-7,
    'h': 6.14e-7,
    'edges': 9.03e-7,
}
# eager's own x-gradient error over the same cases: the diagonal
# cancellation, recorded for comparison and not used as a tolerance
EAGER_FP32_X_ERR = 3.05e-5

GRAD_TOL = {k: 10 * v for k, v in EAGER_FP32_ERR.items()}
GRAD_TOL['x'] = 10 * max(EAGER_FP32_ERR.values())

# test_through_the_model: the eager-fp32-vs-fp64 error of every structure
# module gradient, measured on the MI355X in that test.  Same rule, ten
# times eager's error, but the bare-layer figures above do not carry over
# to layer 0 there: the model starts from x = to_points(h), points that
# nearly coincide, and the fp32 rounding of that Linear's output (outside
# the core, identical in the fused and the eager leg) is a relative error
# of about 1e-4 in rel_ij = x_i - x_j, which every gradient of the
# coordinate path inherits whatever computes it.  The bare-layer cases use
# well separated points (3 * randn) and do not see it.  Each key is held
# to ten times the larger of its bare-layer and its model figure.
# to_points belongs to the structure module, not to the layer, so it has
# a model figure only.
MODEL_EAGER_FP32_ERR = {
    'layers.0.edge_mlp.0.weight': 2.14e-5,
    'layers.0.edge_mlp.0.bias': 2.38e-5,
    'layers.0.edge_mlp.2.weight': 1.88e-5,
    'layers.0.edge_mlp.2.bias': 2.24e-5,
    'layers.0.node_mlp.0.weight': 3.03e-7,
    'layers.0.node_mlp.0.bias': 1.93e-7,
    'layers.0.node_mlp.2.weight': 1.99e-7,
    'layers.0.node_mlp.2.bias': 1.32e-7,
    'layers.0.coors_mlp.0.weight': 1.72e-5,
    'layers.0.coors_mlp.0.bias': 1.53e-4,
    'layers.0.coors_mlp.2.weight': 4.67e-5,
    'layers.0.coors_mlp.2.bias': 1.19e-4,
    'layers.1.edge_mlp.0.weight': 5.60e-7,
    'layers.1.edge_mlp.0.bias': 7.22e-8,
    'layers.1.edge_mlp.2.weight': 5.56e-7,
    'layers.1.edge_mlp.2.bias': 1.01e-7,
    'layers.1.coors_mlp.0.weight': 6.33e-7,
    'layers.1.coors_mlp.0.bias': 4.96e-7,
    'layers.1.coors_mlp.2.weight': 7.20e-7,
    'layers.1.coors_mlp.2.bias': 3.62e-7,
    'to_points.weight': 1.86e-3,
    'to_points.bias': 5.14e-3,
}


def _model_tol(key):
    short = key.split('.', 2)[2] if key.startswith('layers.') else key
    return 10 * max(MODEL_EAGER_FP32_ERR[key], EAGER_FP32_ERR.get(short, 0.))


_NONZERO = ('edge_mlp.0.weight', 'edge_mlp.2.weight', 'coors_mlp.0.weight',
            'coors_mlp.2.weight', 'x', 'edges')


def _liven(layer, seed):
    """coors_mlp[-1] is zero-initialised, which would leave the whole
    coordinate path without gradient.  Small enough that the summed
    update stays far below clamp_coors."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        layer.coors_mlp[-1].weight.copy_(
            0.05 * torch.randn(layer.coors_mlp[-1].weight.shape, generator=g))
        layer.coors_mlp[-1].bias.fill_(0.02)


def _make_state(dim, edge_dim, m_dim=64, seed=0):
    from alphafold2_amd.models.equivariant import EGNNLayer
    torch.manual_seed(seed)
    layer = EGNNLayer(dim, edge_dim=edge_dim, m_dim=m_dim)
    _liven(layer, seed + 100)
    return layer.state_dict()


def _inputs(b, n, dim, edge_dim, seed, device='cuda'):
    g = torch.Generator(device=device).manual_seed(seed)

    def randn(*s):
        return torch.randn(*s, device=device, generator=g)

    return dict(h=randn(b, n, dim), x=3 * randn(b, n, 3),
                edges=randn(b, n, n, edge_dim), w_h=randn(b, n, dim),
                w_x=randn(b, n, 3))


def _run_layer(state, dim, edge_dim, inputs, mask, leg):
    """One forward + backward of a bare EGNNLayer in train mode.
    leg: 'fused' (fp32, dispatch as shipped), 'eager32' or 'eager64'
    (both with _FORCE_EAGER).  Returns (h_out, x_out, grads) in fp64."""
    from alphafold2_amd.models.equivariant import EGNNLayer
    from alphafold2_amd.ops import dispatch

    dtype = torch.float64 if leg == 'eager64' else torch.float32
    prev = dispatch._FORCE_EAGER
    dispatch._FORCE_EAGER = leg != 'fused'
    try:
        layer = EGNNLayer(dim, edge_dim=edge_dim)
        layer.load_state_dict(state)
        layer = layer.cuda().to(dtype).train()
        # fresh leaves per leg: .to() of an fp32 tensor is the tensor itself
        t = {k: v.detach().to(dtype).clone() for k, v in inputs.items()}
        leaves = {k: t[k].requires_grad_(True) for k in ('h', 'x', 'edges')}
        h_out, x_out = layer(t['h'], t['x'], edges=t['edges'], mask=mask)
        ((h_out * t['w_h']).sum() + (x_out * t['w_x']).sum()).backward()
        grads = {k: p.grad.double() for k, p in layer.named_parameters()}
        grads.update({k: v.grad.double() for k, v in leaves.items()})
        if leg == 'eager64':
            # the clamp's kink is not what is under test: a clamped
            # component would read exactly clamp_coors here
            moved = (x_out - t['x']).abs().max().item()
            assert moved < 0.9 * layer.clamp_coors, moved
        return h_out.detach().double(), x_out.detach().double(), grads
    finally:
        dispatch._FORCE_EAGER = prev


def _rel_errors(grads, ref):
    return {k: ((grads[k] - r).abs().max()
                / r.abs().max().clamp_min(1e-30)).item()
            for k, r in ref.items()}


def _count_core_calls(monkeypatch):
    from alphafold2_amd.ops import hip_autograd
    calls = []
    real = hip_autograd.hip_egnn_core

    def counted(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(hip_autograd, 'hip_egnn_core', counted)
    return calls


def _mask_none(b, n):
    return None


def _mask_tail9(b, n):
    m = torch.ones(b, n, dtype=torch.bool, device='cuda')
    m[-1, -9:] = False
    return m


def _mask_single(b, n):
    m = torch.zeros(b, n, dtype=torch.bool, device='cuda')
    m[0, 11] = True
    return m


def _mask_second_empty(b, n):
    m = torch.ones(b, n, dtype=torch.bool, device='cuda')
    m[1] = False
    return m


CASES = [
    # tag, b, n, dim, E, mask
    ('plain', 2, 19, 64, 64, _mask_none),        # under one key tile
    ('ragged', 1, 70, 128, 128, _mask_none),     # crosses a tile, ragged tail
    ('tiles', 1, 150, 256, 256, _mask_none),     # several tiles, widest W_e
    ('dim_ne_e', 1, 37, 32, 64, _mask_none),     # dim != E
    ('tail9', 2, 37, 64, 64, _mask_tail9),
    ('single', 1, 70, 64, 64, _mask_single),
    ('empty', 2, 19, 64, 64, _mask_second_empty),
]


@gpu
@pytest.mark.parametrize('tag,b,n,dim,edge_dim,make_mask', CASES,
                         ids=[c[0] for c in CASES])
def test_layer_forward_backward_parity(monkeypatch, tag, b, n, dim, edge_dim,
                                       make_mask):
    state = _make_state(dim, edge_dim)
    inputs = _inputs(b, n, dim, edge_dim, seed=1)
    mask = make_mask(b, n)
    calls = _count_core_calls(monkeypatch)

    h64, x64, g64 = _run_layer(state, dim, edge_dim, inputs, mask, 'eager64')
    h32, x32, g32 = _run_layer(state, dim, edge_dim, inputs, mask, 'eager32')
    assert len(calls) == 0
    hf, xf, gf = _run_layer(state, dim, edge_dim, inputs, mask, 'fused')
    assert len(calls) == 1

    fwd = {'h_out': ((h32 - h64).abs().max().item(),
                     (hf - h64).abs().max().item()),
           'x_out': ((x32 - x64).abs().max().item(),
                     (xf - x64).abs().max().item())}
    e_eager = _rel_errors(g32, g64)
    e_fused = _rel_errors(gf, g64)
    name = f'{tag}({b},{n},{dim},{edge_dim})'
    for k, (ee, ef) in fwd.items():
        print(f'EGNN_ERR {name} {k} abs: eager32={ee:.3e} fused={ef:.3e} '
              f'tol={FWD_TOL:.1e}')
    for k in g64:
        print(f'EGNN_ERR {name} {k}: eager32={e_eager[k]:.3e} '
              f'fused={e_fused[k]:.3e} tol={GRAD_TOL[k]:.1e} '
              f'refmax={g64[k].abs().max().item():.3e}')

    assert torch.isfinite(hf).all() and torch.isfinite(xf).all()
    for k, (_, ef) in fwd.items():
        assert ef < FWD_TOL, (k, ef)
    for k in g64:
        assert torch.isfinite(gf[k]).all(), k
        if g64[k].abs().max().item() == 0:
            assert gf[k].abs().max().item() == 0, k
        else:
            assert e_fused[k] < GRAD_TOL[k], (k, e_fused[k], GRAD_TOL[k])
    if tag != 'single':
        for k in _NONZERO:
            assert g64[k].abs().max().item() > 0, k


@gpu
@pytest.mark.parametrize('what,kwargs,needle', [
    ('no_edges', dict(edge_dim=0), 'edges=None'),
    ('m_dim', dict(m_dim=32), 'm_dim=32'),
    ('edge_dim', dict(edge_dim=96), 'edge dim 96'),
    ('float64', dict(dtype=torch.float64), 'float64'),
    # widths the LDS copy of the first-layer weight does not cover
    ('e384', dict(dim=384, edge_dim=384, n=37), 'edge dim 384'),
    ('e512', dict(edge_dim=512), 'edge dim 512'),
])
def test_gate_falls_back_and_names_the_predicate(monkeypatch, what, kwargs,
                                                 needle):
    from alphafold2_amd.models.equivariant import EGNNLayer
    from alphafold2_amd.ops import dispatch

    dim = kwargs.get('dim', 64)
    edge_dim = kwargs.get('edge_dim', 64)
    m_dim = kwargs.get('m_dim', 64)
    dtype = kwargs.get('dtype', torch.float32)
    b, n = 1, kwargs.get('n', 19)
    torch.manual_seed(0)
    layer = EGNNLayer(dim, edge_dim=edge_dim, m_dim=m_dim)
    _liven(layer, 1)
    layer = layer.cuda().to(dtype)
    t = _inputs(b, n, dim, max(edge_dim, 1), seed=2)
    h, x = t['h'].to(dtype), t['x'].to(dtype)
    edges = t['edges'].to(dtype) if edge_dim else None

    calls = _count_core_calls(monkeypatch)
    dispatch._warned.difference_update(
        {k for k in dispatch._warned if k[0] == 'egnn_core'})
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        with torch.no_grad():
            h1, x1 = layer(h, x, edges=edges)
            layer(h, x, edges=edges)            # warns once, not per call
    assert len(calls) == 0
    msgs = [str(c.message) for c in caught
            if issubclass(c.category, RuntimeWarning)
            and 'egnn_core' in str(c.message)]
    assert len(msgs) == 1 and needle in msgs[0], msgs

    prev = dispatch._FORCE_EAGER
    dispatch._FORCE_EAGER = True
    try:
        with torch.no_grad():
            h2, x2 = layer(h, x, edges=edges)
    finally:
        dispatch._FORCE_EAGER = prev
    torch.testing.assert_close(h1, h2, rtol=0, atol=0)
    torch.testing.assert_close(x1, x2, rtol=0, atol=0)


@gpu
def test_gate_is_silent_on_a_supported_configuration(monkeypatch):
    from alphafold2_amd.models.equivariant import EGNNLayer
    from alphafold2_amd.ops import dispatch

    torch.manual_seed(0)
    layer = EGNNLayer(64, edge_dim=64).cuda()
    t = _inputs(1, 19, 64, 64, seed=2)
    calls = _count_core_calls(monkeypatch)
    dispatch._warned.difference_update(
        {k for k in dispatch._warned if k[0] == 'egnn_core'})
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        with torch.no_grad():
            layer(t['h'], t['x'], edges=t['edges'])
        monkeypatch.setenv('AF2AMD_EGNN_FUSED', '0')
        with torch.no_grad():
            layer(t['h'], t['x'], edges=t['edges'])
    assert len(calls) == 1           # the toggle turned the second call off
    assert not [c for c in caught if 'egnn_core' in str(c.message)]


@gpu
def test_through_the_model(monkeypatch):
    """Alphafold2 with structure_module_type='egnn' and a padded mask:
    the fused core runs once per layer and coords agree with
    _FORCE_EAGER.  Every structure_module gradient of the fused model is
    compared, as in the bare-layer cases, against fp64: the eager
    structure module in float64 on the very inputs the model fed it (the
    model casts to fp32 in front of the structure module, so it cannot
    run in fp64 as a whole).  Forced-eager fp32, against the fp64
    reference of its own inputs, is printed next to it.  Then the same
    model under bf16 autocast."""
    from alphafold2_amd import Alphafold2
    from alphafold2_amd.data import synthetic_batch
    from alphafold2_amd.ops import dispatch

    kwargs = dict(dim=64, depth=1, heads=2, dim_head=32,
                  predict_coords=True, structure_module_type='egnn',
                  structure_module_depth=2)
    torch.manual_seed(0)
    model = Alphafold2(**kwargs)
    for k, layer in enumerate(model.structure_module.layers):
        _liven(layer, 3 + k)
    state = model.state_dict()

    batch = synthetic_batch(1, 32, 4, device='cuda', seed=0)
    mask = batch['mask'].clone()
    mask[:, 26:] = False
    msa_mask = batch['msa_mask'].clone()
    msa_mask[:, :, 26:] = False
    w = torch.randn(1, 32, 3, device='cuda',
                    generator=torch.Generator('cuda').manual_seed(4))
    calls = _count_core_calls(monkeypatch)

    def sm_grads(sm):
        # coords do not depend on the last layer's h update, so its
        # node_mlp gets no gradient in eager
        return {k: p.grad.double() for k, p in sm.named_parameters()
                if p.grad is not None}

    def run(force_eager, autocast=False):
        prev = dispatch._FORCE_EAGER
        dispatch._FORCE_EAGER = force_eager
        fed = {}
        try:
            m = Alphafold2(**kwargs)
            m.load_state_dict(state)
            m = m.cuda().float().train()
            m.structure_module.register_forward_pre_hook(
                lambda mod, args, kw: fed.update(args=args, kw=kw),
                with_kwargs=True)
            # train mode draws the MSA masking noise: same draw in both legs
            torch.manual_seed(7)
            with torch.autocast('cuda', dtype=torch.bfloat16,
                                enabled=autocast):
                coords = m(batch['seq'], batch['msa'], mask=mask,
                           msa_mask=msa_mask)
                loss = (coords.float() * w).sum()
            loss.backward()
            return (coords.detach().double(), sm_grads(m.structure_module),
                    loss.detach(), fed)
        finally:
            dispatch._FORCE_EAGER = prev

    def reference64(fed):
        prev = dispatch._FORCE_EAGER
        dispatch._FORCE_EAGER = True
        try:
            m = Alphafold2(**kwargs)
            m.load_state_dict(state)
            sm = m.structure_module.cuda().double().train()
            single, pair = (t.detach().double() for t in fed['args'])
            assert fed['kw']['coords'] is None
            _, coords = sm(single, pair, mask=fed['kw']['mask'])
            (coords * w.double()).sum().backward()
            return sm_grads(sm)
        finally:
            dispatch._FORCE_EAGER = prev

    c_f, g_f, _, fed_f = run(False)
    assert len(calls) == 2
    c_e, g_e, _, fed_e = run(True)
    assert len(calls) == 2
    # _FORCE_EAGER also switches the trunk's kernels, so each leg gets
    # the fp64 reference of what its own trunk produced
    g64 = reference64(fed_f)
    g64_e = reference64(fed_e)
    assert g64.keys() == g_e.keys()
    assert g64.keys() <= g_f.keys()
    for k in g_f.keys() - g64.keys():
        assert g_f[k].abs().max().item() == 0, k
    c_err = (c_f - c_e).abs().max().item()
    print(f'EGNN_ERR model coords abs: fused-vs-eager={c_err:.3e} '
          f'tol={FWD_TOL:.1e}')

    e_fused, e_eager = _rel_errors(g_f, g64), _rel_errors(g_e, g64_e)
    tols = {k: _model_tol(k) for k in g64}
    for k in g64:
        print(f'EGNN_ERR model {k}: eager32={e_eager[k]:.3e} '
              f'fused={e_fused[k]:.3e} tol={tols[k]:.1e}')
    assert g64['layers.0.edge_mlp.0.weight'].abs().max() > 0
    assert g_f['layers.0.edge_mlp.0.weight'].abs().max() > 0
    assert g_f['layers.1.coors_mlp.2.weight'].abs().max() > 0
    assert c_err < FWD_TOL, c_err
    for k in g64:
        if g64[k].abs().max().item() == 0:
            assert g_f[k].abs().max().item() == 0, k
        else:
            assert e_fused[k] < tols[k], (k, e_fused[k], tols[k])

    _, _, loss, _ = run(False, autocast=True)
    assert len(calls) == 4
    assert torch.isfinite(loss).item()


@gpu
def test_capture_replays_bit_for_bit():
    """The layer's forward + backward captures into a hipGraph (a host
    sync in the gate would make capture raise); two replays reproduce the
    uncaptured outputs and gradients exactly, since every output of the
    kernels has one writer and a fixed summation order."""
    from alphafold2_amd.models.equivariant import EGNNLayer
    from alphafold2_amd.runtime.graphed import GraphedTrainStep

    b, n, dim = 1, 70, 64
    layer = EGNNLayer(dim, edge_dim=dim)
    layer.load_state_dict(_make_state(dim, dim))
    layer = layer.cuda().train()
    t = _inputs(b, n, dim, dim, seed=5)
    mask = torch.ones(b, n, dtype=torch.bool, device='cuda')
    mask[0, -6:] = False
    leaves = [t[k].requires_grad_(True) for k in ('h', 'x', 'edges')]
    params = list(layer.parameters()) + leaves
    out_h = torch.zeros(b, n, dim, device='cuda')
    out_x = torch.zeros(b, n, 3, device='cuda')

    def step():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()
        h_out, x_out = layer(t['h'], t['x'], edges=t['edges'], mask=mask)
        out_h.copy_(h_out.detach())
        out_x.copy_(x_out.detach())
        loss = (h_out * t['w_h']).sum() + (x_out * t['w_x']).sum()
        loss.backward()
        return loss

    step()
    ref_h, ref_x = out_h.clone(), out_x.clone()
    ref_grads = [p.grad.clone() for p in params]
    torch.cuda.synchronize()

    graphed = GraphedTrainStep(step, warmup=2, fallback=False)
    assert graphed.graphed
    for _ in range(2):
        for p in params:
            p.grad.fill_(float('nan'))      # the replay must rewrite them
        out_h.fill_(float('nan'))
        out_x.fill_(float('nan'))
        graphed()
        torch.cuda.synchronize()
        assert torch.equal(out_h, ref_h)
        assert torch.equal(out_x, ref_x)
        for p, r in zip(params, ref_grads):
            assert torch.equal(p.grad, r)


@gpu
def test_forward_keeps_nothing_of_pair_size(monkeypatch):
    """With grad enabled the Function saves its inputs only: no
    (b, n, n, .) tensor other than `edges`.  A no_grad forward equals the
    grad-mode forward bit for bit, and a contiguous x at an offset that
    is only 4-byte aligned is accepted."""
    from alphafold2_amd.models.equivariant import EGNNLayer

    b, n, dim = 1, 19, 64
    torch.manual_seed(0)
    layer = EGNNLayer(dim, edge_dim=dim)
    _liven(layer, 1)
    layer = layer.cuda()
    t = _inputs(b, n, dim, dim, seed=2)
    with torch.no_grad():
        h_ng, x_ng = layer(t['h'], t['x'], edges=t['edges'])

    saved = []
    with torch.autograd.graph.saved_tensors_hooks(
            lambda s: saved.append(s) or s, lambda s: s):
        h_g, x_g = layer(t['h'], t['x'], edges=t['edges'])
    assert torch.equal(h_ng, h_g.detach()) and torch.equal(x_ng, x_g.detach())
    pair_sized = [s for s in saved
                  if s.dim() == 4 and tuple(s.shape[:3]) == (b, n, n)]
    assert saved
    assert all(s.data_ptr() == t['edges'].data_ptr() for s in pair_sized), \
        [tuple(s.shape) for s in pair_sized]

    # x one float into its storage: contiguous, 4-byte aligned only
    x_off = torch.cat([t['x'].new_zeros(1), t['x'].flatten()])[1:] \
        .view_as(t['x'])
    assert x_off.is_contiguous() and x_off.data_ptr() % 16 != 0
    with torch.no_grad():
        h_o, x_o = layer(t['h'], x_off, edges=t['edges'])
    assert torch.equal(h_o, h_ng) and torch.equal(x_o, x_ng)


def test_cpu_path_is_unchanged():
    """CPU tensors never reach the gate's warning, and the layer's CPU
    output equals the values recorded before the fused branch existed:
    EGNNLayer(16, edge_dim=16) at (b, n) = (1, 8), seed 0, live
    coors_mlp[-1], last two residues masked."""
    from alphafold2_amd.models.equivariant import EGNNLayer
    from alphafold2_amd.ops import dispatch

    b, n, dim = 1, 8, 16
    torch.manual_seed(0)
    layer = EGNNLayer(dim, edge_dim=dim)
    with torch.no_grad():
        layer.coors_mlp[-1].weight.copy_(0.1 * torch.randn(1, 64))
        layer.coors_mlp[-1].bias.fill_(0.25)
    h = torch.randn(b, n, dim)
    x = 3 * torch.randn(b, n, 3)
    edges = torch.randn(b, n, n, dim)
    mask = torch.ones(b, n, dtype=torch.bool)
    mask[0, -2:] = False

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        assert dispatch.egnn_core_fusable(h, edges, m_dim=64) is False
        assert dispatch.egnn_core_fusable(h, None, m_dim=32) is False
        with torch.no_grad():
            h_out, x_out = layer(h, x, edges=edges, mask=mask)
    assert not [c for c in caught if 'egnn_core' in str(c.message)]

    path = os.path.join(os.path.dirname(__file__), 'golden',
                        'egnn_layer_cpu.json')
    with open(path) as f:
        golden = json.load(f)

    def unhex(vals, like):
        return torch.tensor([float.fromhex(v) for v in vals],
                            dtype=torch.float64).reshape(like.shape)

    assert torch.equal(h_out.double(), unhex(golden['h_out'], h_out))
    assert torch.equal(x_out.double(), unhex(golden['x_out'], x_out))
