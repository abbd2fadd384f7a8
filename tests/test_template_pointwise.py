"""Template pointwise attention (K5): the public op against the folded
`attention_core` call, `Attention.pointwise_context` against the module's
`forward`, the gate, and on the GPU the kernels' forward + backward parity,
strided operands, fallbacks, the model, hipGraph capture and what the
Function keeps for the backward.

Error rule of the GPU parity tests.  The reference is the eager
composition (`eager.attention_core` on the hand-folded operands) in
float64 on the same device, from the same storage-rounded inputs.  The
same composition in the kernel's storage type gives the yardstick: its
error against fp64.  Both are printed as `TPL_ERR` lines, as absolute
max-abs differences next to the reference's max-abs.

* bf16: fused error <= max(2 x eager-bf16 error, 2^-8 x max-abs of the
  reference).  The kernel rounds once where eager rounds after every op;
  the floor is one bf16 ulp of the largest value.
* fp32: fused error <= max(10 x eager-fp32 error, 1e-6 x max-abs).

Measured on an MI355X: docs/KERNELS.md, K5 section.
"""
import warnings

import pytest
import torch

gpu = pytest.mark.gpu

MASK_CASES = ('none', 'key', 'both', 'both_edge')
# the all-masked position and the masked query of 'both_edge': (batch, p)
ALL_MASKED_POS = (0, 5)
MASKED_QUERY = (1, 7)


def _masks(case, b, T, P, device):
    """(key_mask (b, T, P), query_mask (b, P)) of a mask case.  Every
    position keeps template 0 visible, so that only 'both_edge' has a row
    without a live logit."""
    if case == 'none':
        return None, None
    g = torch.Generator().manual_seed(11)
    key = torch.rand(b, T, P, generator=g) > 0.4
    key[:, 0] = True
    if case == 'key':
        return key.to(device), None
    query = torch.ones(b, P, dtype=torch.bool)
    if case == 'both_edge':
        key[ALL_MASKED_POS[0], :, ALL_MASKED_POS[1]] = False
        query[MASKED_QUERY] = False
    return key.to(device), query.to(device)


def _inputs(b, P, T, H, d, dtype, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, P, H * d, generator=g)
    kv = torch.randn(b, T, P, 2 * H * d, generator=g)
    w = torch.randn(b, P, H * d, generator=g)
    return tuple(t.to(dtype).to(device) for t in (q, kv, w))


def _folded_eager(q, kv, heads, key_mask, query_mask):
    """eager.attention_core on the hand-folded operands.  A key mask
    without a query mask gets an all-true one: eager applies the key mask
    only next to a query mask."""
    from alphafold2_amd.ops import eager
    b, P, C = q.shape
    T, d = kv.shape[1], C // heads
    qf = q.reshape(b * P, 1, heads, d).transpose(1, 2)
    k, v = kv[..., :C], kv[..., C:]
    kf, vf = (t.permute(0, 2, 1, 3).reshape(b * P, T, heads, d)
              .transpose(1, 2) for t in (k, v))
    km = qm = None
    if key_mask is not None:
        km = key_mask.permute(0, 2, 1).reshape(b * P, T)
        qm = torch.ones(b * P, 1, dtype=torch.bool, device=q.device)
    if query_mask is not None:
        qm = query_mask.reshape(b * P, 1)
    out = eager.attention_core(qf, kf, vf, mask=qm, context_mask=km)
    return out.transpose(1, 2).reshape(b, P, C)


def _fwd_bwd(fn, q, kv, w, dtype=None):
    """out, dq, dkv of fn(q, kv) under the upstream gradient w, as fp64."""
    dtype = dtype or q.dtype
    q = q.detach().to(dtype).clone().requires_grad_(True)
    kv = kv.detach().to(dtype).clone().requires_grad_(True)
    out = fn(q, kv)
    dq, dkv = torch.autograd.grad(out, (q, kv), w.to(dtype))
    return {'out': out.detach().double(), 'dq': dq.double(),
            'dkv': dkv.double()}


def _check_edge_rows(res, kv, w, heads, unit):
    """The all-masked position and the masked query on their own: uniform
    weights, no gradient through the masked logits, dv = dout / T.  `unit`
    is the relative rounding step of the storage type's results."""
    C = res['out'].shape[-1]
    T = kv.shape[1]
    kv, w = kv.double(), w.double()
    for bi, p in (ALL_MASKED_POS, MASKED_QUERY):
        v = kv[bi, :, p, C:]
        assert (res['out'][bi, p] - v.mean(0)).abs().max() \
            <= unit * v.abs().max()
        assert torch.count_nonzero(res['dq'][bi, p]) == 0
        assert torch.count_nonzero(res['dkv'][bi, :, p, :C]) == 0
        dv = res['dkv'][bi, :, p, C:]
        assert (dv - w[bi, p] / T).abs().max() <= unit * w[bi, p].abs().max()
    for t in res.values():
        assert torch.isfinite(t).all()


# ---------------------------------------------------------------- CPU tests


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('case', MASK_CASES)
def test_op_matches_folded_call_cpu(case, dtype):
    from alphafold2_amd import ops
    b, P, T, H, d = 2, 49, 3, 2, 32
    q, kv, w = _inputs(b, P, T, H, d, dtype, 'cpu')
    km, qm = _masks(case, b, T, P, 'cpu')
    got = _fwd_bwd(lambda q, kv: ops.template_pointwise_attention(
        q, kv, H, key_mask=km, query_mask=qm), q, kv, w)
    ref = _fwd_bwd(lambda q, kv: _folded_eager(q, kv, H, km, qm), q, kv, w)
    for name in ref:
        assert (got[name] - ref[name]).abs().max() <= 1e-6, name
    if case == 'both_edge':
        _check_edge_rows(got, kv, w, H, 1e-6)


def _folded_module_call(attn, x, context, query_mask, key_mask):
    b, P, dim = x.shape
    T = context.shape[1]
    out = attn(x.reshape(b * P, 1, dim),
               context=context.permute(0, 2, 1, 3).reshape(b * P, T, dim),
               mask=query_mask.reshape(b * P, 1),
               context_mask=key_mask.permute(0, 2, 1).reshape(b * P, T))
    return out.reshape(b, P, dim)


def _live_attention(dim, heads, dim_head, dropout=0.):
    """An Attention whose zero-initialised to_out and gate weights are
    replaced, so that every parameter gets a gradient."""
    from alphafold2_amd.models.evoformer import Attention
    torch.manual_seed(0)
    attn = Attention(dim, heads=heads, dim_head=dim_head, dropout=dropout)
    with torch.no_grad():
        torch.nn.init.normal_(attn.to_out.weight, std=0.2)
        torch.nn.init.normal_(attn.to_out.bias, std=0.2)
        torch.nn.init.normal_(attn.gating.weight, std=0.2)
    return attn


def test_method_matches_module_cpu():
    b, P, T, dim, H, d = 2, 49, 3, 24, 2, 32
    attn = _live_attention(dim, H, d)
    keys = list(attn.state_dict().keys())
    assert keys == ['to_q.weight', 'to_kv.weight', 'to_out.weight',
                    'to_out.bias', 'gating.weight', 'gating.bias']
    g = torch.Generator().manual_seed(1)
    x = torch.randn(b, P, dim, generator=g)
    context = torch.randn(b, T, P, dim, generator=g)
    w = torch.randn(b, P, dim, generator=g)
    km, qm = _masks('both_edge', b, T, P, 'cpu')
    params = list(attn.parameters())

    def run(fn):
        out = fn(attn, x, context, qm, km)
        return [out.detach(), *torch.autograd.grad(out, params, w)]

    got = run(lambda a, *args: a.pointwise_context(*args))
    ref = run(_folded_module_call)
    for name, a, r in zip(['out'] + keys, got, ref):
        assert (a - r).abs().max() <= 1e-6 * max(1., r.abs().max()), name
    assert list(attn.state_dict().keys()) == keys


def test_gate_cpu(monkeypatch):
    from alphafold2_amd.ops import dispatch
    q = torch.randn(1, 4, 64)
    kv = torch.randn(1, 3, 4, 128)
    kw = dict(heads=2, dim_head=32, num_templates=3, drop_p=0.)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert dispatch.template_pool_fusable(q, kv, **kw) is False
        monkeypatch.setenv('AF2AMD_TEMPLATE_POOL_FUSED', '0')
        assert dispatch.template_pool_fusable(q, kv, **kw) is False
    assert dispatch.TEMPLATE_POOL_MAX_TEMPLATES == 16


# ---------------------------------------------------------------- GPU tests

# (P, T, H, d): one position per wave at (256, 4, 8, 64); one-lane groups
# at d = 8; at (50, 10, 3, 32) a position takes 12 lanes, so positions
# straddle waves and the last wave has a tail
SHAPES = [(49, 3, 2, 64), (256, 4, 8, 64), (49, 1, 1, 8), (50, 10, 3, 32),
          (33, 16, 2, 16)]


def _count_calls(monkeypatch):
    from alphafold2_amd.ops import hip_autograd
    calls = []
    real = hip_autograd.hip_template_pointwise

    def counting(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(hip_autograd, 'hip_template_pointwise', counting)
    return calls


def _bound(dtype, eager_err, ref_max):
    if dtype == torch.bfloat16:
        return max(2 * eager_err, 2. ** -8 * ref_max)
    return max(10 * eager_err, 1e-6 * ref_max)


def _parity(tag, dtype, fused, eager_s, ref):
    for name, r in ref.items():
        ref_max = r.abs().max().item()
        e_f = (fused[name] - r).abs().max().item()
        e_e = (eager_s[name] - r).abs().max().item()
        print(f'TPL_ERR {tag} {name}: fused={e_f:.3e} eager={e_e:.3e} '
              f'ref_max={ref_max:.3e}')
    for name, r in ref.items():
        ref_max = r.abs().max().item()
        e_f = (fused[name] - r).abs().max().item()
        e_e = (eager_s[name] - r).abs().max().item()
        assert e_f <= _bound(dtype, e_e, ref_max), (tag, name, e_f, e_e)


@gpu
@pytest.mark.parametrize('case', MASK_CASES)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32],
                         ids=['bf16', 'fp32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bare_op_parity_gpu(shape, dtype, case, monkeypatch):
    from alphafold2_amd import ops
    P, T, H, d = shape
    b = 2
    q, kv, w = _inputs(b, P, T, H, d, dtype, 'cuda')
    km, qm = _masks(case, b, T, P, 'cuda')
    calls = _count_calls(monkeypatch)
    fused = _fwd_bwd(lambda q, kv: ops.template_pointwise_attention(
        q, kv, H, key_mask=km, query_mask=qm), q, kv, w)
    assert len(calls) == 1, 'the pointwise kernels must take this shape'

    def eager(q, kv):
        return _folded_eager(q, kv, H, km, qm)

    ref = _fwd_bwd(eager, q, kv, w, dtype=torch.float64)
    eager_s = _fwd_bwd(eager, q, kv, w)
    tag = f'{"x".join(map(str, shape))} {str(dtype)[6:]} {case}'
    _parity(tag, dtype, fused, eager_s, ref)
    if case == 'both_edge':
        # fp32: (T - 1) additions, the 1 / l multiply and 1 / T itself
        unit = 2. ** -8 if dtype == torch.bfloat16 else (T + 2) * 2. ** -24
        _check_edge_rows(fused, kv, w, H, unit)


@gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32],
                         ids=['bf16', 'fp32'])
def test_strided_operands_gpu(dtype):
    """q and kv as channel-dense, 16-byte aligned slices of wider buffers:
    the same bits as with contiguous copies, and no copy on the way."""
    from alphafold2_amd.ops.hip_autograd import hip_template_pointwise
    b, P, T, H, d = 2, 49, 3, 2, 32
    C = H * d
    g = torch.Generator().manual_seed(5)
    q_buf = torch.randn(b, P, C + 16, generator=g).to(dtype).cuda()
    kv_buf = torch.randn(b, T, P, 2 * C + 24, generator=g).to(dtype).cuda()
    w = torch.randn(b, P, C, generator=g).to(dtype).cuda()
    km, qm = _masks('both_edge', b, T, P, 'cuda')

    def run(q, kv):
        q = q.detach().requires_grad_(True)
        kv = kv.detach().requires_grad_(True)
        out = hip_template_pointwise(q, kv, H, key_mask=km, query_mask=qm)
        return [out.detach(), *torch.autograd.grad(out, (q, kv), w)]

    q_s, kv_s = q_buf[..., 8:8 + C], kv_buf[..., 8:8 + 2 * C]
    assert q_s.stride(1) != C and kv_s.stride(2) != 2 * C
    strided = run(q_s, kv_s)
    dense = run(q_s.contiguous(), kv_s.contiguous())
    for name, a, r in zip(['out', 'dq', 'dkv'], strided, dense):
        assert torch.equal(a, r), name

    q_c, kv_c = q_s.contiguous(), kv_s.contiguous()
    # base pointer off by one element
    with pytest.raises(RuntimeError, match='16-byte'):
        hip_template_pointwise(q_buf[..., 1:1 + C], kv_c, H)
    with pytest.raises(RuntimeError, match='16-byte'):
        hip_template_pointwise(q_c, kv_buf[..., 1:1 + 2 * C], H)
    # row stride that is no multiple of 16 bytes
    odd = torch.zeros(b, P, C + 1, dtype=dtype, device='cuda')[..., :C]
    with pytest.raises(RuntimeError, match='16 bytes'):
        hip_template_pointwise(odd, kv_c, H)
    # strided channels
    wide = torch.zeros(b, P, 2 * C, dtype=dtype, device='cuda')[..., ::2]
    with pytest.raises(RuntimeError, match='dense'):
        hip_template_pointwise(wide, kv_c, H)
    wide_kv = torch.zeros(b, T, P, 4 * C, dtype=dtype,
                          device='cuda')[..., ::2]
    with pytest.raises(RuntimeError, match='dense'):
        hip_template_pointwise(q_c, wide_kv, H)
    torch.cuda.synchronize()


def _no_template_pool_warning(record):
    assert not [w for w in record if 'template_pool' in str(w.message)]


@gpu
@pytest.mark.parametrize('name,shape,switch', [
    ('d24', (49, 3, 2, 24), None),
    ('T17', (33, 17, 2, 32), None),
    ('switch0', (49, 3, 2, 32), '0'),
])
def test_gate_declines_to_flash_path_gpu(name, shape, switch, monkeypatch):
    """Outside the gate the op returns through the folded attention_core
    call, which is the flash kernels here: correct results, the new
    Function does not run, and nothing warns about 'template_pool'."""
    from alphafold2_amd import ops
    from alphafold2_amd.ops import dispatch
    P, T, H, d = shape
    b, dtype = 2, torch.bfloat16
    if switch is not None:
        monkeypatch.setenv('AF2AMD_TEMPLATE_POOL_FUSED', switch)
    monkeypatch.setattr(dispatch, '_warned', set())
    q, kv, w = _inputs(b, P, T, H, d, dtype, 'cuda')
    km, qm = _masks('key', b, T, P, 'cuda')
    calls = _count_calls(monkeypatch)
    assert not dispatch.template_pool_fusable(
        q, kv, heads=H, dim_head=d, num_templates=T, drop_p=0.)
    with warnings.catch_warnings(record=True) as record:
        warnings.simplefilter('always')
        got = _fwd_bwd(lambda q, kv: ops.template_pointwise_attention(
            q, kv, H, key_mask=km, query_mask=qm), q, kv, w)
    _no_template_pool_warning(record)
    assert not calls

    def eager(q, kv):
        return _folded_eager(q, kv, H, km, qm)

    ref = _fwd_bwd(eager, q, kv, w, dtype=torch.float64)
    eager_s = _fwd_bwd(eager, q, kv, w)
    _parity(f'fallback {name}', dtype, got, eager_s, ref)


@gpu
def test_gate_dropout_and_eager_ending_gpu(monkeypatch):
    """Active attention dropout in training: pointwise_context declines
    without a warning (forward's flash path has the dropout); in eval the
    same module takes the new path.  fp64, where today's path ends in the
    eager composition, is the one decline that warns."""
    from alphafold2_amd.ops import dispatch
    b, P, T, dim, H, d = 2, 49, 3, 32, 2, 32
    monkeypatch.setattr(dispatch, '_warned', set())
    attn = _live_attention(dim, H, d, dropout=0.25).cuda().bfloat16()
    x = torch.randn(b, P, dim, device='cuda', dtype=torch.bfloat16)
    context = torch.randn(b, T, P, dim, device='cuda', dtype=torch.bfloat16)
    km, qm = _masks('both', b, T, P, 'cuda')
    calls = _count_calls(monkeypatch)
    with warnings.catch_warnings(record=True) as record:
        warnings.simplefilter('always')
        attn.train()
        assert attn.pointwise_context(x, context, qm, km) is None
        assert not calls
        out = _folded_module_call(attn, x, context, qm, km)
        assert torch.isfinite(out).all() and not calls
        attn.eval()
        assert attn.pointwise_context(x, context, qm, km) is not None
        assert len(calls) == 1
    _no_template_pool_warning(record)

    q64 = torch.randn(1, 4, 64, device='cuda', dtype=torch.float64)
    kv64 = torch.randn(1, 3, 4, 128, device='cuda', dtype=torch.float64)
    with pytest.warns(RuntimeWarning, match='template_pool'):
        assert not dispatch.template_pool_fusable(
            q64, kv64, heads=2, dim_head=32, num_templates=3, drop_p=0.)


@gpu
def test_through_the_model_gpu(monkeypatch):
    """Alphafold2 with templates, a template mask that hides one
    template's tail and a padded sequence mask, bf16 autocast, train mode.
    The new Function runs with the switch on and not with it off; the
    error of ret.distance and of the template gradients against the fp64
    eager model is at most twice that of the switch-off leg (the parent's
    path)."""
    from alphafold2_amd import Alphafold2
    from alphafold2_amd.ops import dispatch
    kwargs = dict(dim=64, depth=1, heads=2, dim_head=32, templates_dim=32,
                  templates_angles_feats_dim=32)
    b, n, T = 2, 16, 3
    torch.manual_seed(0)
    model = Alphafold2(**kwargs)
    # to_out starts at zero, which would leave the pooling without effect
    # and its projections without gradient
    with torch.no_grad():
        torch.nn.init.normal_(model.template_pointwise_attn.to_out.weight,
                              std=0.2)
    state = model.state_dict()

    g = torch.Generator().manual_seed(2)
    seq = torch.randint(0, 21, (b, n), generator=g).cuda()
    msa = torch.randint(0, 21, (b, 3, n), generator=g).cuda()
    tf = torch.randn(b, T, n, n, 32, generator=g).cuda()
    ta = torch.randn(b, T, n, 32, generator=g).cuda()
    mask = torch.ones(b, n, dtype=torch.bool, device='cuda')
    mask[1, 13:] = False
    msa_mask = mask[:, None, :].expand(b, 3, n).contiguous()
    tm = torch.ones(b, T, n, dtype=torch.bool, device='cuda')
    tm[:, 2, 10:] = False
    calls = _count_calls(monkeypatch)

    def run(leg):
        ref = leg == 'ref'
        monkeypatch.setenv('AF2AMD_TEMPLATE_POOL_FUSED',
                           '0' if leg == 'off' else '1')
        monkeypatch.setattr(dispatch, '_FORCE_EAGER', ref)
        m = Alphafold2(**kwargs)
        m.load_state_dict(state)
        m = m.cuda().to(torch.float64 if ref else torch.float32).train()
        # train mode draws the MSA masking noise: same draw in every leg
        torch.manual_seed(7)
        feats = tf.double() if ref else tf
        angles = ta.double() if ref else ta
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=not ref):
            ret = m(seq, msa, mask=mask, msa_mask=msa_mask,
                    templates_feats=feats, templates_angles=angles,
                    templates_mask=tm)
            loss = ret.distance.double().pow(2).mean()
        loss.backward()
        res = {'distance': ret.distance.detach().double()}
        for k, p in m.named_parameters():
            if k.startswith(('template_pointwise_attn.',
                             'to_template_embed.')):
                res[k] = p.grad.double()
        return res

    n0 = len(calls)
    fused = run('on')
    assert len(calls) == n0 + 1, 'the pointwise kernels must run'
    off = run('off')
    assert len(calls) == n0 + 1, 'the switch must turn them off'
    ref = run('ref')
    assert len(calls) == n0 + 1

    errs = {}
    for k, r in ref.items():
        scale = r.abs().max().item()
        assert scale > 0, k
        errs[k] = ((fused[k] - r).abs().max().item() / scale,
                   (off[k] - r).abs().max().item() / scale)
        print(f'TPL_ERR model {k}: fused={errs[k][0]:.3e} '
              f'switch_off={errs[k][1]:.3e}')
    for k, (e_f, e_o) in errs.items():
        assert e_f <= 2 * e_o, (k, e_f, e_o)


@gpu
def test_graph_capture_gpu():
    from alphafold2_amd.ops.hip_autograd import hip_template_pointwise
    b, P, T, H, d = 1, 49, 3, 2, 64
    q, kv, w = _inputs(b, P, T, H, d, torch.bfloat16, 'cuda')
    q.requires_grad_(True)
    kv.requires_grad_(True)
    km, qm = _masks('both', b, T, P, 'cuda')

    def step():
        out = hip_template_pointwise(q, kv, H, key_mask=km, query_mask=qm)
        return [out, *torch.autograd.grad(out, (q, kv), w)]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        want = [t.detach().clone() for t in step()]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for name, a, r in zip(['out', 'dq', 'dkv'], static, want):
            assert torch.equal(a, r), name


@gpu
def test_saved_tensors_gpu():
    """Forward keeps q, kv, out and lse: no padded or permuted copy at
    d = 32, and nothing else with a T * P extent."""
    from alphafold2_amd.ops.hip_autograd import hip_template_pointwise
    b, P, T, H, d = 2, 49, 3, 2, 32
    q, kv, _ = _inputs(b, P, T, H, d, torch.bfloat16, 'cuda')
    q.requires_grad_(True)
    kv.requires_grad_(True)
    km, qm = _masks('both', b, T, P, 'cuda')
    out = hip_template_pointwise(q, kv, H, key_mask=km, query_mask=qm)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 4
    s_q, s_kv, s_out, s_lse = saved
    assert s_q.data_ptr() == q.data_ptr() and s_q.shape == q.shape
    assert s_kv.data_ptr() == kv.data_ptr() and s_kv.shape == kv.shape
    assert s_out.data_ptr() == out.data_ptr()
    assert s_lse.shape == (b, P, H) and s_lse.dtype == torch.float32
    # the masks stay the caller's own memory
    ctx = out.grad_fn
    assert ctx.key_mask.data_ptr() == km.data_ptr()
    assert ctx.query_mask.data_ptr() == qm.data_ptr()
