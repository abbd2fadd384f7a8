"""Gated self-attention as one autograd unit, and the column sums that
ride on elementwise backward kernels.

`attn_gate_bwd` is the gate backward of gated attention in one pass: dO
contiguous, dgate written into the gate slice of the packed gradient,
delta = rowsum(dO * O) for `attn_bwd`, and the column sum of dgate (the
gating-bias gradient) from per-block partials folded in a fixed order.
`_GatedAttentionUnitFn` owns projection, attention and gate, so the
packed projection has one consumer.  `geglu_bwd_colsum` is `geglu_bwd`
plus the column sum of what it writes (the FF1 bias gradient).

Reference and bound are those of tests/test_attention_ds_path.py: one
plain-torch reference evaluated in float64 and in bf16, and

    E_kernel <= 2 * E_floor + 2**-8 * max|ref64|

Each bound check prints `EVIDENCE case output E_kernel E_floor ratio
bound` before it asserts.  delta keeps attn_delta_kernel's lane mapping
and summation order, so it is tested for equality (through attn_bwd,
which does not return it) as well as by the bound.
"""
import warnings
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16 = torch.bfloat16


# ---------------------------------------------------------------------------
# reference and bound (conventions of tests/test_attention_ds_path.py)


def ref_attention(q, k, v, bias, key_mask, scale, bias_repeat=1,
                  keep=None, rescale=1.0):
    """softmax(q k^T * scale + repeat_interleave(bias) + key mask), then
    dropout by the explicit `keep` mask and `rescale`, times v, in the
    dtype of its inputs.  A row whose keys are all masked gives 0."""
    s = torch.einsum('bhid,bhjd->bhij', q, k) * scale
    if bias is not None:
        s = s + bias.repeat_interleave(bias_repeat, dim=0)
    if key_mask is not None:
        s = s.masked_fill(~key_mask.bool()[:, None, None, :], float('-inf'))
    p = s.softmax(dim=-1).nan_to_num(0.)
    if keep is not None:
        p = p * keep.to(p.dtype) * rescale
    return torch.einsum('bhij,bhjd->bhid', p, v)


class _Bound:
    """Collects the bound checks of one case: prints every figure, then
    `done()` fails if any output exceeded its bound."""

    def __init__(self, case):
        self.case = case
        self.failed = []

    def check(self, name, kern, r64, r16):
        assert kern.shape == r64.shape, (name, kern.shape, r64.shape)
        assert torch.isfinite(kern).all(), f"{name} not finite"
        ek = (kern.double() - r64).abs().max().item()
        ef = (r16.double() - r64).abs().max().item()
        bound = 2.0 * ef + 2.0 ** -8 * r64.abs().max().item()
        ratio = ek / ef if ef > 0 else float('nan')
        print(f"EVIDENCE {self.case} {name} E_kernel={ek:.3e} "
              f"E_floor={ef:.3e} ratio={ratio:.2f} bound={bound:.3e}")
        if not ek <= bound:
            self.failed.append(f"{name}: E_kernel {ek:.3e} > bound "
                               f"{bound:.3e} (E_floor {ef:.3e})")

    def done(self):
        assert not self.failed, f"{self.case}: " + "; ".join(self.failed)


def _randn(*shape, gen=None):
    return torch.randn(*shape, device=DEV, generator=gen).to(BF16)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


@pytest.fixture(scope="module")
def ext():
    from alphafold2_amd.ops.dispatch import _load_ext
    e = _load_ext()
    assert e is not None, "extension must load on GPU box"
    return e


# ---------------------------------------------------------------------------
# 1. the kernel alone


def ref_gate_bwd(dy, o, g, H):
    """dO, dg, delta (B, H, L), column sum of dg — in the inputs' dtype.
    dy, o, g are (B, L, H * 64)."""
    B, L, C = dy.shape
    s = torch.sigmoid(g)
    d_o = dy * s
    dg = dy * o * s * (1 - s)
    delta = (d_o * o).view(B, L, H, 64).sum(-1).permute(0, 2, 1)
    return d_o, dg, delta, dg.sum(dim=(0, 1))


# (2, 65, 2): rows no multiple of the rows per block; (3, 200, 1): one
# head, 8-lane rows; (1, 64, 8): 64-lane rows, 16 partial rows;
# (1, 8229, 8): more rows than the capped grid covers in one sweep
# (2048 blocks x 4 rows), so the grid-stride loop runs
KERNEL_SHAPES = [(2, 65, 2), (3, 200, 1), (1, 64, 8), (1, 8229, 8)]

_KCASES = {}


def _kernel_case(B, L, H):
    key = (B, L, H)
    if key not in _KCASES:
        g = _gen(100 + L)
        C = H * 64
        packed = _randn(B, L, 4 * C, gen=g)
        dy = _randn(B, L, C, gen=g)
        out = _randn(B, L, H, 64, gen=g).permute(0, 2, 1, 3)
        gate = packed.narrow(-1, 3 * C, C)
        o2 = out.permute(0, 2, 1, 3).reshape(B, L, C)
        refs = tuple(
            ref_gate_bwd(dy.to(dt), o2.to(dt), gate.to(dt), H)
            for dt in (torch.float64, BF16))
        _KCASES[key] = (dict(packed=packed, dy=dy, out=out, gate=gate,
                             o2=o2), refs)
    return _KCASES[key]


def _run_gate(ext, c, want_colsum=True):
    C = c['dy'].shape[-1]
    buf = torch.full_like(c['packed'], float('nan'))
    rets = ext.attn_gate_bwd(c['dy'], c['out'], c['gate'],
                             buf.narrow(-1, 3 * C, C), want_colsum)
    return buf, rets


@pytest.mark.parametrize("B,L,H", KERNEL_SHAPES)
def test_gate_kernel(ext, B, L, H):
    c, (r64, r16) = _kernel_case(B, L, H)
    C = H * 64
    dx, dg = ext.gatemul_bwd(c['dy'], c['o2'], c['gate'], C, 4 * C)
    buf, rets = _run_gate(ext, c)
    assert len(rets) == 3
    d_o, delta, colsum = rets
    torch.cuda.synchronize()
    assert d_o.shape == c['out'].shape and d_o.stride() == c['out'].stride()
    assert torch.equal(d_o.permute(0, 2, 1, 3).reshape(B, L, C), dx), "dO"
    assert torch.equal(buf[..., 3 * C:], dg), "dg"
    assert torch.isnan(buf[..., :3 * C]).all(), "q/k/v blocks were written"
    assert delta.dtype == torch.float32 and delta.shape == (B, H, L)
    assert colsum.dtype == torch.float32 and colsum.shape == (C,)
    bd = _Bound(f"gate[{B}x{L}x{H}]")
    bd.check('delta', delta, r64[2], r16[2])
    bd.check('colsum', colsum, r64[3], r16[3])
    bd.done()
    # without the option: the same dO, dg and delta, no third result
    buf2, rets2 = _run_gate(ext, c, want_colsum=False)
    assert len(rets2) == 2
    assert torch.equal(rets2[0], d_o) and torch.equal(rets2[1], delta)
    assert torch.equal(buf2[..., 3 * C:], dg)


@pytest.mark.parametrize("B,L,H", KERNEL_SHAPES[:3])
def test_gate_kernel_delta_is_attn_bwd_s(ext, B, L, H):
    """attn_bwd with the kernel's delta gives exactly what it gives with
    its own attn_delta_kernel, with and without a bias gradient."""
    c, _ = _kernel_case(B, L, H)
    C = H * 64
    g = _gen(200 + L)

    def view(off):
        return c['packed'].narrow(-1, off, C).view(B, L, H, 64) \
            .permute(0, 2, 1, 3)

    q, k, v = view(0), view(C), view(2 * C)
    bias = _randn(B, H, L, L, gen=g)
    out, lse = ext.attn_fwd(q, k, v, bias, None, 1, 0.125)
    cc = dict(c, out=out)
    _, (d_o, delta) = _run_gate(ext, cc, want_colsum=False)
    for need_dbias in (True, False):
        own = ext.attn_bwd(d_o, q, k, v, out, lse, bias, None, 1, 0.125,
                           need_dbias)
        got = ext.attn_bwd(d_o, q, k, v, out, lse, bias, None, 1, 0.125,
                           need_dbias, delta=delta)
        for name, a, b in zip(['dq', 'dk', 'dv', 'dbias'], own, got):
            assert torch.equal(a, b), (name, need_dbias)


def test_gate_kernel_colsum_deterministic(ext):
    c, _ = _kernel_case(1, 8229, 8)
    a = _run_gate(ext, c)[1][2]
    b = _run_gate(ext, c)[1][2]
    assert torch.equal(a, b), "column sum differs between launches"


def test_gate_kernel_operand_checks(ext):
    c, _ = _kernel_case(2, 65, 2)
    C = 128
    buf = torch.empty_like(c['packed'])
    dg = buf.narrow(-1, 3 * C, C)
    with pytest.raises(RuntimeError):      # out not in (B, L, h, 64) memory
        ext.attn_gate_bwd(c['dy'], c['out'].contiguous(), c['gate'], dg)
    with pytest.raises(RuntimeError):      # rows not 16-byte aligned
        ext.attn_gate_bwd(c['dy'], c['out'], c['gate'],
                          buf.narrow(-1, 3 * C - 4, C))
    with pytest.raises(RuntimeError):      # wrong dtype
        ext.attn_gate_bwd(c['dy'].float(), c['out'], c['gate'], dg)
    with pytest.raises(RuntimeError):      # delta of the wrong size
        q = c['out']
        lse = torch.zeros(2, 2, 65, device=DEV)
        ext.attn_bwd(q, q, q, q, q, lse, None, None, 1, 0.125, False,
                     delta=torch.zeros(2, 2, 64, device=DEV))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 2. the whole unit against the separate path, through Attention

DIM, HEADS = 128, 2
PARAMS = ['to_q.weight', 'to_kv.weight', 'to_out.weight', 'to_out.bias',
          'gating.weight', 'gating.bias']


def _module(p_drop):
    from alphafold2_amd.models.evoformer import Attention
    torch.manual_seed(5)
    m = Attention(dim=DIM, heads=HEADS, dim_head=64, dropout=p_drop)
    # gating and to_out are initialised to identity / zero: give them
    # values so every gradient is non-trivial
    torch.nn.init.normal_(m.to_out.weight, std=DIM ** -0.5)
    torch.nn.init.normal_(m.to_out.bias, std=0.1)
    torch.nn.init.normal_(m.gating.weight, std=DIM ** -0.5)
    torch.nn.init.normal_(m.gating.bias, std=0.5)
    return m.to(DEV).train()


def ref_module(x, wq, wkv, wg, bg, wo, bo, abias, mask, r, keep, rescale):
    """Attention.forward in plain torch, in the dtype of its inputs."""
    B, L, _ = x.shape
    q = x @ wq.T
    k, v = (x @ wkv.T).chunk(2, dim=-1)
    gate = x @ wg.T + bg

    def split(t):
        return t.view(B, L, HEADS, 64).permute(0, 2, 1, 3)

    o = ref_attention(split(q), split(k), split(v), abias, mask, 0.125, r,
                      keep, rescale)
    o = o.permute(0, 2, 1, 3).reshape(B, L, -1) * torch.sigmoid(gate)
    return o @ wo.T + bo


def _run_module(ext, m, c, unit, seed):
    from alphafold2_amd.ops import dispatch
    for p in m.parameters():
        p.grad = None
    x = c['x'].clone().requires_grad_(True)
    ab = c['abias'].clone().requires_grad_(c['bias_grad'])
    torch.cuda.manual_seed(seed)
    with mock.patch.object(dispatch, '_GATED_ATTN_UNIT', unit), \
            mock.patch.object(ext, 'attn_gate_bwd',
                              wraps=ext.attn_gate_bwd) as gate_spy, \
            mock.patch.object(ext, 'gatemul_bwd',
                              wraps=ext.gatemul_bwd) as gm_spy:
        with torch.autocast('cuda', dtype=BF16):
            y = m(x, mask=c['mask'], attn_bias=ab, attn_bias_repeat=c['r'])
        loss = (y.float() * c['cot']).sum()
        loss.backward()
    torch.cuda.synchronize()
    assert (gate_spy.call_count, gm_spy.call_count) == \
        ((1, 0) if unit else (0, 1)), "wrong path for the switch"
    grads = {n: m.get_parameter(n).grad.clone() for n in PARAMS}
    return loss.detach(), y.detach(), x.grad, ab.grad, grads


UNIT_CASES = {
    # B, L, bias_repeat, masked, dropout, bias needs grad
    'repeat2': (2, 40, 2, False, 0., True),
    'masked': (3, 72, 1, True, 0., True),
    'dropout': (2, 72, 1, False, 0.25, True),
    'bias_nograd': (2, 40, 2, False, 0., False),
}


@pytest.mark.parametrize("case", list(UNIT_CASES))
def test_unit_matches_separate_path(ext, case):
    B, L, r, masked, p, bias_grad = UNIT_CASES[case]
    g = _gen(300 + L + B)
    m = _module(p)
    c = dict(x=torch.randn(B, L, DIM, device=DEV, generator=g),
             abias=_randn(B // r, HEADS, L, L, gen=g), r=r, mask=None,
             cot=torch.randn(B, L, DIM, device=DEV, generator=g),
             bias_grad=bias_grad)
    if masked:
        mask = torch.rand(B, L, device=DEV, generator=g) > 0.2
        mask[:, 0] = True
        mask[1, :] = False          # one fully masked entry
        c['mask'] = mask
    seed = 41
    new = _run_module(ext, m, c, True, seed)
    old = _run_module(ext, m, c, False, seed)
    assert torch.equal(new[0], old[0]), "loss"
    assert torch.equal(new[1], old[1]), "output"
    assert torch.equal(new[2], old[2]), "input gradient"
    if bias_grad:
        assert torch.equal(new[3], old[3]), "dbias"
    else:
        assert new[3] is None and old[3] is None
    for n in PARAMS[:-1]:
        assert torch.equal(new[4][n], old[4][n]), n

    # gating-bias gradient: by the bound, against plain torch
    keep, rescale = None, 1.0
    if p > 0.:
        # the state the module's forward drew after manual_seed(seed)
        from alphafold2_amd.ops.hip_autograd import hip_attention_core
        torch.cuda.manual_seed(seed)
        t = _randn(1, 1, 64, 64, gen=g)
        st = hip_attention_core(t, t, t, dropout_p=p,
                                return_rng_state=True)[1]
        keep = ext.attn_dropout_mask(st, B, HEADS, L, L, p)
        thresh = min(255, max(1, int(p * 256 + 0.5)))
        rescale = 256.0 / (256 - thresh)
    leaves = [c['x']] + [m.get_parameter(n).detach() for n in
                         ['to_q.weight', 'to_kv.weight', 'gating.weight',
                          'gating.bias', 'to_out.weight', 'to_out.bias']]
    leaves = [t.to(BF16) for t in leaves]   # what the kernels are given
    refs = []
    for dt in (torch.float64, BF16):
        xs = [t.to(dt).requires_grad_(True) for t in leaves]
        y = ref_module(*xs, c['abias'].to(dt), c['mask'], r, keep, rescale)
        refs.append(torch.autograd.grad(y, xs[4], c['cot'].to(dt))[0])
    for name, got in (('unit', new[4]), ('separate', old[4])):
        bd = _Bound(f"unit[{case}]")
        bd.check(f'dgating_bias_{name}', got['gating.bias'], *refs)
        if name == 'unit':
            bd.done()


def test_unit_conditions_fall_back(ext):
    """tie_dim, an fp32 input outside autocast and cross-attention keep
    the separate Functions: the unit's kernel is not launched."""
    m = _module(0.)
    g = _gen(77)
    x = torch.randn(4, 40, DIM, device=DEV, generator=g)
    with mock.patch.object(ext, 'attn_gate_bwd',
                           wraps=ext.attn_gate_bwd) as gate_spy:
        with torch.autocast('cuda', dtype=BF16):
            m(x.clone().requires_grad_(True), tie_dim=4).sum().backward()
            m(x.clone().requires_grad_(True), context=x).sum().backward()
        with warnings.catch_warnings():
            # fp32 attention is the eager composition, announced (once
            # per process) by the dispatch's RuntimeWarning
            warnings.simplefilter('ignore', RuntimeWarning)
            m(x.clone().requires_grad_(True)).sum().backward()
        assert gate_spy.call_count == 0
        with torch.autocast('cuda', dtype=BF16):
            m(x.clone().requires_grad_(True)).sum().backward()
        assert gate_spy.call_count == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 3. geglu_bwd with the column sum


def ref_geglu_bwd(dy, x):
    xs = x.detach().clone().requires_grad_(True)
    a, gt = xs.chunk(2, dim=-1)
    y = a * torch.nn.functional.gelu(gt)
    di = torch.autograd.grad(y, xs, dy)[0]
    return di, di.sum(dim=0)


# 37 x 2*64: 32 rows per block sweep, a partial last block;
# 1000 x 2*2048: the widest row the option covers, one row per sweep
@pytest.mark.parametrize("rows,H", [(37, 64), (1000, 2048)])
def test_geglu_bwd_colsum(ext, rows, H):
    g = _gen(400 + rows)
    x = _randn(rows, 2 * H, gen=g)
    dy = _randn(rows, H, gen=g)
    assert H <= ext.geglu_bwd_colsum_max_h()
    plain = ext.geglu_bwd(dy, x)
    di, colsum = ext.geglu_bwd_colsum(dy, x)
    assert torch.equal(di, plain), "di"
    assert colsum.dtype == torch.float32 and colsum.shape == (2 * H,)
    r64 = ref_geglu_bwd(dy.double(), x.double())
    r16 = ref_geglu_bwd(dy, x)
    bd = _Bound(f"geglu_colsum[{rows}x{2 * H}]")
    bd.check('colsum', colsum, r64[1], r16[1])
    bd.done()
    assert torch.equal(ext.geglu_bwd_colsum(dy, x)[1], colsum), \
        "column sum differs between launches"
    with pytest.raises(RuntimeError):
        ext.geglu_bwd_colsum(dy, _randn(rows, 2 * 4096, gen=g))
    with pytest.raises(RuntimeError):
        ext.geglu_bwd_colsum(dy.float(), x.float())


def test_ff1_geglu_bias_grad_uses_colsum(ext):
    """_FF1GegluFn takes its bias gradient from the kernel's column sum:
    tested by the bound against plain torch."""
    from alphafold2_amd.ops.hip_autograd import hip_ff1_geglu
    g = _gen(500)
    rows, d, N = 300, 128, 1024
    x = _randn(rows, d, gen=g)
    w = (_randn(N, d, gen=g).float() * d ** -0.5).to(BF16)
    b = _randn(N, gen=g)
    dy = _randn(rows, N // 2, gen=g)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    with mock.patch.object(ext, 'geglu_bwd_colsum',
                           wraps=ext.geglu_bwd_colsum) as spy:
        out = hip_ff1_geglu(*leaves)
        dx, dw, db = torch.autograd.grad(out, leaves, dy)
    assert spy.call_count == 1
    refs = []
    for dt in (torch.float64, BF16):
        xs = [t.to(dt).requires_grad_(True) for t in (x, w, b)]
        a, gt = (xs[0] @ xs[1].T + xs[2]).chunk(2, dim=-1)
        y = a * torch.nn.functional.gelu(gt)
        refs.append(torch.autograd.grad(y, xs[2], dy.to(dt))[0])
    bd = _Bound("ff1_geglu_db")
    bd.check('db', db, *refs)
    bd.done()
