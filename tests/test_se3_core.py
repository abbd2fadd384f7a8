"""Fused SE(3) refiner attention core (K15): forward + backward parity
against the eager layer in float64, key masks, the gate's fallbacks,
reachability from the model, hipGraph capture, the LDS bound and the
unchanged CPU path.

Reference: the eager layer (`dispatch._FORCE_EAGER`) in float64 on the
same device.  Each case also runs the eager layer in fp32; its error
against fp64 is the yardstick, printed next to the fused error as
`SE3_ERR` lines.  Errors are relative to the reference's max-abs.

Gradient tolerances are ten times the largest eager-fp32 error measured
on an MI355X over the bare-layer cases of this file (docs/KERNELS.md, K15
section); the forward tolerance is the project's 1e-4 absolute.  The `x`
gradient is the exception: eager's own error there (EAGER_FP32_X_ERR) is
the diagonal cancellation of +-u/sqrt(eps), which the fused backward
skips, so `x` is held to ten times the largest eager error among the
other gradients.
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
    'norm.weight': 3.91e-7,
    'norm.bias': 5.53e-7,
    'to_q.weight': 9.15e-7,
    'to_k.weight': 1.07e-6,
    'to_v.weight': 7.71e-7,
    'edge_bias.weight': 5.72e-6,
    'edge_bias.bias': 2.15e-8,
    'to_out.weight': 1.10e-6,
    'to_out.bias': 1.43e-7,
    'coors_head.weight': 6.41e-7,
    'coors_head.bias': 4.12e-6,
    'ff.0.weight': 7.32e-7,
    'ff.0.bias': 4.26e-7,
    'ff.2.weight': 6.29e-7,
    'ff.2.bias': 1.36e-7,
    'h': 4.84e-7,
    'edges': 9.59e-7,
}
# eager's own x-gradient error over the same cases: the diagonal
# cancellation, recorded for comparison and not used as a tolerance
EAGER_FP32_X_ERR = 6.51e-4

GRAD_TOL = {k: 10 * v for k, v in EAGER_FP32_ERR.items()}
GRAD_TOL['x'] = 10 * max(EAGER_FP32_ERR.values())

# to_points belongs to the structure module, not to the layer, so no
# bare-layer case measures it.  Its gradient is the sum of every layer's
# x gradient at the near-coincident initial points to_points itself
# produces, where rel / |rel| amplifies the fp32 rounding of x in any
# implementation.  Same rule as above: ten times the eager-fp32-vs-fp64
# error measured on the MI355X in test_through_the_model.
MODEL_EAGER_FP32_ERR = {
    'to_points.weight': 8.46e-5,
    'to_points.bias': 3.65e-5,
}
MODEL_GRAD_TOL = {k: 10 * v for k, v in MODEL_EAGER_FP32_ERR.items()}

# sum_j dL[h, j] == 0 for every softmax row, so the bias Linear's bias
# gradient is rounding noise around zero in every leg; it is judged
# against the scale of that Linear's weight gradient instead of its own
_ZERO_SUM = 'edge_bias.bias'
_ZERO_SUM_SCALE = 'edge_bias.weight'


def _make_state(dim, heads, dim_head, seed=0):
    """State dict of an SE3RefinerLayer with a live coordinate head:
    coors_head is zero-initialised, which would leave the dxh path
    without gradient."""
    from alphafold2_amd.models.equivariant import SE3RefinerLayer
    torch.manual_seed(seed)
    layer = SE3RefinerLayer(dim, heads=heads, dim_head=dim_head,
                            edge_dim=dim)
    with torch.no_grad():
        layer.coors_head.weight.copy_(0.1 * torch.randn(heads, dim))
        layer.coors_head.bias.copy_(torch.linspace(-.5, .5, heads))
    return layer.state_dict()


def _inputs(b, n, dim, seed, device='cuda'):
    g = torch.Generator(device=device).manual_seed(seed)

    def randn(*s):
        return torch.randn(*s, device=device, generator=g)

    return dict(h=randn(b, n, dim), x=3 * randn(b, n, 3),
                edges=randn(b, n, n, dim), w_h=randn(b, n, dim),
                w_x=randn(b, n, 3))


def _run_layer(state, dim, heads, dim_head, inputs, mask, leg):
    """One forward + backward of a bare SE3RefinerLayer in train mode.
    leg: 'fused' (fp32, dispatch as shipped), 'eager32' or 'eager64'
    (both with _FORCE_EAGER).  Returns (h_out, x_out, grads) in fp64."""
    from alphafold2_amd.models.equivariant import SE3RefinerLayer
    from alphafold2_amd.ops import dispatch

    dtype = torch.float64 if leg == 'eager64' else torch.float32
    prev = dispatch._FORCE_EAGER
    dispatch._FORCE_EAGER = leg != 'fused'
    try:
        layer = SE3RefinerLayer(dim, heads=heads, dim_head=dim_head,
                                edge_dim=dim)
        layer.load_state_dict(state)
        layer = layer.cuda().to(dtype).train()
        # fresh leaves per leg: .to() of an fp32 tensor is the tensor itself
        t = {k: v.detach().to(dtype).clone() for k, v in inputs.items()}
        leaves = {k: t[k].requires_grad_(True) for k in ('h', 'x', 'edges')}
        h_out, x_out = layer(t['h'], t['x'], edges=t['edges'], mask=mask)
        ((h_out * t['w_h']).sum() + (x_out * t['w_x']).sum()).backward()
        grads = {k: p.grad.double() for k, p in layer.named_parameters()}
        grads.update({k: v.grad.double() for k, v in leaves.items()})
        return h_out.detach().double(), x_out.detach().double(), grads
    finally:
        dispatch._FORCE_EAGER = prev


def _rel_errors(grads, ref):
    errs = {}
    for k, r in ref.items():
        scale = ref[_ZERO_SUM_SCALE] if k == _ZERO_SUM else r
        errs[k] = ((grads[k] - r).abs().max()
                   / scale.abs().max().clamp_min(1e-30)).item()
    return errs


def _count_core_calls(monkeypatch):
    from alphafold2_amd.ops import hip_autograd
    calls = []
    real = hip_autograd.hip_se3_core

    def counted(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(hip_autograd, 'hip_se3_core', counted)
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
    # tag, b, n, H, dh, dim=E, mask
    ('plain', 2, 37, 4, 16, 64, _mask_none),         # under one wave of keys
    ('wave', 1, 70, 4, 32, 128, _mask_none),         # crosses a wave
    ('block', 1, 300, 8, 32, 256, _mask_none),       # n > block width
    ('e384', 1, 70, 1, 64, 384, _mask_none),         # E not 2^k, heads=1
    ('tail9', 2, 37, 8, 16, 64, _mask_tail9),
    ('single', 1, 70, 4, 16, 64, _mask_single),
    ('empty', 2, 37, 4, 16, 64, _mask_second_empty),
]


@gpu
@pytest.mark.parametrize('tag,b,n,heads,dh,dim,make_mask', CASES,
                         ids=[c[0] for c in CASES])
def test_layer_forward_backward_parity(monkeypatch, tag, b, n, heads, dh,
                                       dim, make_mask):
    state = _make_state(dim, heads, dh)
    inputs = _inputs(b, n, dim, seed=1)
    mask = make_mask(b, n)
    calls = _count_core_calls(monkeypatch)

    h64, x64, g64 = _run_layer(state, dim, heads, dh, inputs, mask, 'eager64')
    h32, x32, g32 = _run_layer(state, dim, heads, dh, inputs, mask, 'eager32')
    assert len(calls) == 0
    hf, xf, gf = _run_layer(state, dim, heads, dh, inputs, mask, 'fused')
    assert len(calls) == 1

    fwd = {'h_out': ((h32 - h64).abs().max().item(),
                     (hf - h64).abs().max().item()),
           'x_out': ((x32 - x64).abs().max().item(),
                     (xf - x64).abs().max().item())}
    e_eager = _rel_errors(g32, g64)
    e_fused = _rel_errors(gf, g64)
    name = f'{tag}({b},{n},{heads},{dh},{dim})'
    for k, (ee, ef) in fwd.items():
        print(f'SE3_ERR {name} {k} abs: eager32={ee:.3e} fused={ef:.3e} '
              f'tol={FWD_TOL:.1e}')
    for k in g64:
        print(f'SE3_ERR {name} {k}: eager32={e_eager[k]:.3e} '
              f'fused={e_fused[k]:.3e} tol={GRAD_TOL[k]:.1e}')

    assert torch.isfinite(hf).all() and torch.isfinite(xf).all()
    for k, (_, ef) in fwd.items():
        assert ef < FWD_TOL, (k, ef)
    for k in g64:
        assert torch.isfinite(gf[k]).all(), k
        if g64[k].abs().max().item() == 0:
            # e.g. to_q / to_k / edge_bias with a single valid key: a
            # one-hot softmax row has dL == 0 exactly
            assert gf[k].abs().max().item() == 0, k
        else:
            assert e_fused[k] < GRAD_TOL[k], (k, e_fused[k], GRAD_TOL[k])
    if tag == 'single':
        for k in ('to_q.weight', 'to_k.weight', 'edge_bias.weight',
                  'edge_bias.bias'):
            assert g64[k].abs().max().item() == 0, k
    else:
        for k in ('to_q.weight', 'edge_bias.weight', 'x', 'edges',
                  'coors_head.weight'):
            assert g64[k].abs().max().item() > 0, k


@gpu
@pytest.mark.parametrize('what,kwargs,needle', [
    ('heads', dict(heads=9), 'heads=9'),
    ('dim_head', dict(dim_head=18), 'dim_head=18'),
    ('edge_dim', dict(dim=96), 'edge dim 96'),
    ('float64', dict(dtype=torch.float64), 'float64'),
    ('no_edges', dict(edges=False), 'edges=None'),
])
def test_gate_falls_back_and_names_the_predicate(monkeypatch, what, kwargs,
                                                 needle):
    from alphafold2_amd.models.equivariant import SE3RefinerLayer
    from alphafold2_amd.ops import dispatch

    heads = kwargs.get('heads', 4)
    dim_head = kwargs.get('dim_head', 16)
    dim = kwargs.get('dim', 64)
    dtype = kwargs.get('dtype', torch.float32)
    b, n = 1, 19
    torch.manual_seed(0)
    layer = SE3RefinerLayer(dim, heads=heads, dim_head=dim_head,
                            edge_dim=dim).cuda().to(dtype)
    t = _inputs(b, n, dim, seed=2)
    h, x = t['h'].to(dtype), t['x'].to(dtype)
    edges = t['edges'].to(dtype) if kwargs.get('edges', True) else None

    calls = _count_core_calls(monkeypatch)
    dispatch._warned.difference_update(
        {k for k in dispatch._warned if k[0] == 'se3_core'})
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        with torch.no_grad():
            h1, x1 = layer(h, x, edges=edges)
            layer(h, x, edges=edges)            # warns once, not per call
    assert len(calls) == 0
    msgs = [str(c.message) for c in caught
            if issubclass(c.category, RuntimeWarning)
            and 'se3_core' in str(c.message)]
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
    from alphafold2_amd.models.equivariant import SE3RefinerLayer
    from alphafold2_amd.ops import dispatch

    torch.manual_seed(0)
    layer = SE3RefinerLayer(64, heads=4, dim_head=16, edge_dim=64).cuda()
    t = _inputs(1, 19, 64, seed=2)
    calls = _count_core_calls(monkeypatch)
    dispatch._warned.difference_update(
        {k for k in dispatch._warned if k[0] == 'se3_core'})
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        with torch.no_grad():
            layer(t['h'], t['x'], edges=t['edges'])
        monkeypatch.setenv('AF2AMD_SE3_FUSED', '0')
        with torch.no_grad():
            layer(t['h'], t['x'], edges=t['edges'])
    assert len(calls) == 1           # the toggle turned the second call off
    assert not [c for c in caught if 'se3_core' in str(c.message)]


@gpu
def test_through_the_model(monkeypatch):
    """Alphafold2 with structure_module_type='se3' and a padded mask:
    the fused core runs once per layer and coords agree with
    _FORCE_EAGER.  Every structure_module gradient of the fused model is
    compared, as in the bare-layer cases, against fp64: the eager
    structure module in float64 on the very inputs the model fed it (the
    model casts to fp32 in front of the structure module, so it cannot
    run in fp64 as a whole).  Forced-eager fp32, against the fp64
    reference of its own inputs, is printed next to it; it is no
    reference here, since its x gradient carries the diagonal
    cancellation from layer 1 into every layer-0 gradient.  Then the
    same model under bf16 autocast."""
    from alphafold2_amd import Alphafold2
    from alphafold2_amd.data import synthetic_batch
    from alphafold2_amd.ops import dispatch

    kwargs = dict(dim=64, depth=1, heads=2, dim_head=32,
                  predict_coords=True, structure_module_type='se3',
                  structure_module_depth=2)
    torch.manual_seed(0)
    model = Alphafold2(**kwargs)
    # coors_head starts at zero, which leaves the dxh path without
    # gradient: give it weights so the comparison is not vacuous
    torch.manual_seed(3)
    for layer in model.structure_module.layers:
        torch.nn.init.normal_(layer.coors_head.weight, std=0.1)
        torch.nn.init.normal_(layer.coors_head.bias, std=0.3)
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
        # to_out / ff (and in eager to_v) get no gradient
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
    # the fused Function returns a gradient for every input that requires
    # one, so where eager leaves None (last layer's to_v) it gives zeros
    assert g64.keys() <= g_f.keys()
    for k in g_f.keys() - g64.keys():
        assert g_f[k].abs().max().item() == 0, k
    c_err = (c_f - c_e).abs().max().item()
    print(f'SE3_ERR model coords abs: fused-vs-eager={c_err:.3e} '
          f'tol={FWD_TOL:.1e}')

    def short(k):       # 'layers.0.to_q.weight' -> 'to_q.weight'
        return k.split('.', 2)[2] if k.startswith('layers.') else k

    def rel_errors(grads, ref):
        errs = {}
        for k, r in ref.items():
            scale = ref[k.replace(_ZERO_SUM, _ZERO_SUM_SCALE)] \
                if short(k) == _ZERO_SUM else r
            errs[k] = ((grads[k] - r).abs().max()
                       / scale.abs().max().clamp_min(1e-30)).item()
        return errs

    e_fused, e_eager = rel_errors(g_f, g64), rel_errors(g_e, g64_e)
    tols = {k: MODEL_GRAD_TOL.get(k) or GRAD_TOL[short(k)] for k in g64}
    for k in g64:
        print(f'SE3_ERR model {k}: eager32={e_eager[k]:.3e} '
              f'fused={e_fused[k]:.3e} tol={tols[k]:.1e}')
    assert g64['layers.0.edge_bias.weight'].abs().max() > 0
    assert g_f['layers.0.edge_bias.weight'].abs().max() > 0
    assert g_f['layers.1.coors_head.weight'].abs().max() > 0
    assert c_err < FWD_TOL, c_err
    for k in g64:
        assert e_fused[k] < tols[k], (k, e_fused[k], tols[k])

    _, _, loss, _ = run(False, autocast=True)
    assert len(calls) == 4
    assert torch.isfinite(loss).item()


@gpu
def test_capture_replays_bit_for_bit():
    """The layer's forward + backward captures into a hipGraph (a host
    sync in the gate would make capture raise); two replays reproduce the
    uncaptured outputs and gradients exactly, since every output of the
    three kernels has one writer and a fixed summation order.  The gate
    answers the same in the warmup and under capture, so no GEMM runs
    for the first time while capturing."""
    from alphafold2_amd.models.equivariant import SE3RefinerLayer
    from alphafold2_amd.runtime.graphed import GraphedTrainStep

    b, n, heads, dh, dim = 1, 70, 4, 16, 64
    layer = SE3RefinerLayer(dim, heads=heads, dim_head=dh, edge_dim=dim)
    layer.load_state_dict(_make_state(dim, heads, dh))
    layer = layer.cuda().train()
    t = _inputs(b, n, dim, seed=5)
    mask = torch.ones(b, n, dtype=torch.bool, device='cuda')
    mask[0, -6:] = False
    leaves = [t[k].requires_grad_(True) for k in ('h', 'x', 'edges')]
    params = list(layer.parameters()) + leaves
    # static buffers, as a captured training step has them: outputs are
    # copied out and gradients accumulate into .grad tensors that exist
    # before the capture (runtime/graphed.py)
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
def test_probabilities_are_saved_only_for_a_backward(monkeypatch):
    """A (b,H,n,n) is written when a gradient will be asked for, not in
    a no_grad forward of a layer whose parameters require grad; and a
    contiguous operand at an offset that is not 16-byte aligned is
    accepted."""
    from alphafold2_amd.models.equivariant import SE3RefinerLayer
    from alphafold2_amd.ops import dispatch

    ext = dispatch._load_ext()
    seen = []
    real = ext.se3_core_fwd

    def recording(*args, **kwargs):
        seen.append(kwargs['save_attn'])
        return real(*args, **kwargs)

    monkeypatch.setattr(ext, 'se3_core_fwd', recording)
    torch.manual_seed(0)
    layer = SE3RefinerLayer(64, heads=4, dim_head=16, edge_dim=64).cuda()
    t = _inputs(1, 19, 64, seed=2)
    with torch.no_grad():
        h_ng, x_ng = layer(t['h'], t['x'], edges=t['edges'])
    h_g, x_g = layer(t['h'], t['x'], edges=t['edges'])
    assert seen == [False, True]
    assert torch.equal(h_ng, h_g.detach()) and torch.equal(x_ng, x_g.detach())

    # x one float into its storage: contiguous, 4-byte aligned only
    x_off = torch.cat([t['x'].new_zeros(1), t['x'].flatten()])[1:] \
        .view_as(t['x'])
    assert x_off.is_contiguous() and x_off.data_ptr() % 16 != 0
    with torch.no_grad():
        h_o, x_o = layer(t['h'], x_off, edges=t['edges'])
    assert torch.equal(h_o, h_ng) and torch.equal(x_o, x_ng)


def _bwd_row_lds_bytes(heads, n, dim_head, edge_dim):
    # mirrors bwd_row_lds_bytes in ops/hip/se3core.hip
    npad = (n + 3) & ~3
    return 4 * (heads * edge_dim + heads * dim_head + 2 * heads * npad
                + 256 + 4 * 3 * heads + 4 * heads)


@gpu
def test_lds_bound_falls_back_to_eager():
    """One past se3_core_max_n through the gate only: stride-0 views
    stand in for the inputs, nothing is launched."""
    from alphafold2_amd.ops import dispatch

    ext = dispatch._load_ext()
    props = torch.cuda.get_device_properties(0)
    # what one block may use, opt-in included: the limit the host code
    # checks its launches against
    limit = max(props.shared_memory_per_block,
                getattr(props, 'shared_memory_per_block_optin', 0))
    n8 = ext.se3_core_max_n(8, 64, 512)
    print(f'SE3_LDS max_n(8,64,512)={n8} '
          f'max_n(4,16,256)={ext.se3_core_max_n(4, 16, 256)} '
          f'lds_limit={limit}')
    # the bound is exactly the last n (rows are padded to 4 floats) whose
    # row-side backward, the largest user, fits that limit
    for heads, dh, e in ((8, 64, 512), (4, 16, 256), (1, 64, 512),
                         (8, 64, 64)):
        bound = ext.se3_core_max_n(heads, dh, e)
        assert bound % 4 == 0 and bound > 0
        assert _bwd_row_lds_bytes(heads, bound, dh, e) <= limit
        assert _bwd_row_lds_bytes(heads, bound + 1, dh, e) > limit
    assert ext.se3_core_max_n(1, 64, 512) > n8
    assert ext.se3_core_max_n(8, 64, 64) > n8

    z = torch.zeros(1, device='cuda')
    dispatch._warned.difference_update(
        {k for k in dispatch._warned if k[0] == 'se3_core'})
    for n, expect in ((n8, True), (n8 + 1, False)):
        h = z.expand(1, n, 512)
        edges = z.expand(1, n, n, 512)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            ok = dispatch.se3_core_fusable(h, edges, heads=8, dim_head=64)
        msgs = [str(c.message) for c in caught if 'se3_core' in str(c.message)]
        assert ok is expect
        if expect:
            assert not msgs, msgs
        else:
            assert len(msgs) == 1 and f'n={n}' in msgs[0], msgs


def test_cpu_path_is_unchanged():
    """CPU tensors never reach the gate's warning, and the layer's CPU
    output equals the values recorded before the fused branch existed:
    SE3RefinerLayer(16, heads=2, dim_head=16, edge_dim=16) at
    (b, n) = (1, 8), seed 0, live coors_head, last two keys masked."""
    from alphafold2_amd.models.equivariant import SE3RefinerLayer
    from alphafold2_amd.ops import dispatch

    b, n, heads, dh, dim = 1, 8, 2, 16, 16
    torch.manual_seed(0)
    layer = SE3RefinerLayer(dim, heads=heads, dim_head=dh, edge_dim=dim)
    with torch.no_grad():
        layer.coors_head.weight.copy_(0.1 * torch.randn(heads, dim))
        layer.coors_head.bias.copy_(torch.linspace(-.5, .5, heads))
    h = torch.randn(b, n, dim)
    x = 3 * torch.randn(b, n, 3)
    edges = torch.randn(b, n, n, dim)
    mask = torch.ones(b, n, dtype=torch.bool)
    mask[0, -2:] = False

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        assert dispatch.se3_core_fusable(h, edges, heads=heads,
                                         dim_head=dh) is False
        assert dispatch.se3_core_fusable(h, None, heads=9,
                                         dim_head=18) is False
        with torch.no_grad():
            h_out, x_out = layer(h, x, edges=edges, mask=mask)
    assert not [c for c in caught if 'se3_core' in str(c.message)]

    path = os.path.join(os.path.dirname(__file__), 'golden',
                        'se3_layer_cpu.json')
    with open(path) as f:
        golden = json.load(f)

    def unhex(vals, like):
        return torch.tensor([float.fromhex(v) for v in vals],
                            dtype=torch.float64).reshape(like.shape)

    assert torch.equal(h_out.double(), unhex(golden['h_out'], h_out))
    assert torch.equal(x_out.double(), unhex(golden['x_out'], x_out))
