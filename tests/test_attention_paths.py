"""Fused attention as the model calls it: packed, strided, padded.

Every parity assertion compares a kernel result with one plain-torch
reference (`ref_attention`, below) evaluated in float64, and bounds the
kernel's error by the error the ORDINARY bf16 torch composition of the
same reference makes on the same inputs:

    E_kernel = max|kernel.double() - ref(float64 inputs)|
    E_floor  = max|ref(bf16 inputs).double() - ref(float64 inputs)|
    assert E_kernel <= 2 * E_floor + 2**-8 * max|ref64|

The factor 2 is the usual flash-attention allowance (P and dS are
rounded to bf16 at other points than in the eager composition); the
additive term is one bf16 half-ulp of the largest reference value.
Each check prints `EVIDENCE case output E_kernel E_floor ratio` before
it asserts; docs/EVIDENCE.md holds the measured table.
"""
import os
import subprocess
import sys
import tempfile
import warnings
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16 = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ext():
    from alphafold2_amd.ops.dispatch import _load_ext
    e = _load_ext()
    assert e is not None, "extension must load on GPU box"
    return e


# ---------------------------------------------------------------------------
# reference and bound


def ref_attention(q, k, v, bias, key_mask, scale, bias_repeat=1,
                  tie_dim=None):
    """softmax(q k^T * scale + repeat_interleave(bias) + key mask) v in
    the dtype of its inputs.  A row whose keys are all masked gives 0
    (docs/PARITY.md); tie_dim replaces each query by its group mean."""
    if tie_dim is not None:
        B = q.shape[0]
        q = q.reshape(B // tie_dim, tie_dim, *q.shape[1:]) \
             .mean(dim=1, keepdim=True) \
             .expand(-1, tie_dim, -1, -1, -1).reshape(q.shape)
    s = torch.einsum('bhid,bhjd->bhij', q, k) * scale
    if bias is not None:
        s = s + bias.repeat_interleave(bias_repeat, dim=0)
    if key_mask is not None:
        s = s.masked_fill(~key_mask.bool()[:, None, None, :], float('-inf'))
    p = s.softmax(dim=-1).nan_to_num(0.)
    return torch.einsum('bhij,bhjd->bhid', p, v)


def _ref_grads(fn, leaves, dout, dtype):
    """[out, d leaf_0, d leaf_1, ...] of fn(*leaves) under `dout`, with
    every leaf converted (exactly, from bf16) to `dtype`."""
    xs = [t.detach().to(dtype).requires_grad_(True) for t in leaves]
    out = fn(*xs)
    gs = torch.autograd.grad(out, xs, dout.to(dtype), allow_unused=True)
    return [out.detach()] + [torch.zeros_like(x) if g is None else g
                             for x, g in zip(xs, gs)]


class _Bound:
    """Collects the bound checks of one case: prints every figure, then
    `done()` fails if any output exceeded its bound."""

    def __init__(self, case):
        self.case = case
        self.failed = []

    def check(self, name, kern, r64, r16, ref_max=None):
        assert kern.shape == r64.shape, (name, kern.shape, r64.shape)
        ek = (kern.double() - r64).abs().max().item()
        ef = (r16.double() - r64).abs().max().item()
        if ref_max is None:
            ref_max = r64.abs().max().item()
        bound = 2.0 * ef + 2.0 ** -8 * ref_max
        ratio = ek / ef if ef > 0 else float('nan')
        print(f"EVIDENCE {self.case} {name} E_kernel={ek:.3e} "
              f"E_floor={ef:.3e} ratio={ratio:.2f} bound={bound:.3e}")
        if not ek <= bound:
            self.failed.append(f"{name}: E_kernel {ek:.3e} > bound "
                               f"{bound:.3e} (E_floor {ef:.3e})")

    def check_all(self, names, kern, fn, leaves, dout):
        r64 = _ref_grads(fn, leaves, dout, torch.float64)
        r16 = _ref_grads(fn, leaves, dout, BF16)
        for i, name in enumerate(names):
            self.check(name, kern[i], r64[i], r16[i])

    def done(self):
        assert not self.failed, f"{self.case}: " + "; ".join(self.failed)


NAMES = ['out', 'dq', 'dk', 'dv', 'dbias']


def _randn(*shape, gen=None):
    return torch.randn(*shape, device=DEV, generator=gen).to(BF16)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _run_core(q, k, v, bias, mask, dout, bias_repeat=1, scale=None,
              tie_dim=None):
    """[out, dq, dk, dv, dbias] from hip_attention_core."""
    from alphafold2_amd.ops.hip_autograd import hip_attention_core
    xs = [t.detach().clone().requires_grad_(True)
          for t in (q, k, v, bias) if t is not None]
    b = xs[3] if bias is not None else None
    out = hip_attention_core(xs[0], xs[1], xs[2], bias=b, mask=mask,
                             tie_dim=tie_dim, bias_repeat=bias_repeat,
                             scale=scale)
    out.backward(dout)
    return [out.detach()] + [x.grad for x in xs]


def _core_fn(mask, scale, bias_repeat=1, tie_dim=None):
    return lambda q, k, v, bias=None: ref_attention(
        q, k, v, bias, mask, scale, bias_repeat, tie_dim)


# ---------------------------------------------------------------------------
# shared inputs (also fed to the split-dK/dV child process)


def _dbias_inputs(r, Lq, Lk, use_mask, seed=4):
    g = _gen(seed)
    B, h = 2 * r, 2
    c = dict(q=_randn(B, h, Lq, 64, gen=g), k=_randn(B, h, Lk, 64, gen=g),
             v=_randn(B, h, Lk, 64, gen=g),
             bias=_randn(B // r, h, Lq, Lk, gen=g),
             dout=_randn(B, h, Lq, 64, gen=g), r=r, mask=None)
    if use_mask:
        m = torch.rand(B, Lk, device=DEV, generator=g) > 0.2
        m[:, 0] = True
        c['mask'] = m
    return c


def _tile_mask_inputs(seed=6):
    """(B, Lq, Lk) = (6, 130, 200); one whole-tile mask pattern per batch
    entry: leading tile, every trailing tile, middle tile, one valid key,
    all valid, none valid."""
    g = _gen(seed)
    B, h, Lq, Lk = 6, 2, 130, 200
    m = torch.ones(B, Lk, dtype=torch.bool, device=DEV)
    m[0, :64] = False
    m[1, 64:] = False
    m[2, 64:128] = False
    m[3, :199] = False
    m[5, :] = False
    return dict(q=_randn(B, h, Lq, 64, gen=g), k=_randn(B, h, Lk, 64, gen=g),
                v=_randn(B, h, Lk, 64, gen=g),
                bias=_randn(B, h, Lq, Lk, gen=g),
                dout=_randn(B, h, Lq, 64, gen=g), r=1, mask=m)


def _check_dbias_case(case, c, kern):
    bd = _Bound(case)
    bd.check_all(NAMES, kern, _core_fn(c['mask'], 0.125, c['r']),
                 [c['q'], c['k'], c['v'], c['bias']], c['dout'])
    bd.done()


def _check_tile_mask_case(case, c, kern):
    """The bound per batch entry, plus the exact-zero properties of the
    entry with no valid key and of masked bias columns.

    Per entry, E_kernel and E_floor are taken over that entry alone; the
    additive half-ulp term stays that of the whole output tensor, as the
    bound defines it.  An entry-local term would be 0 for dq, dk and
    dbias of the one-valid-key entry (softmax over one key has zero
    gradient; reference and bf16 floor are both exactly 0), which no
    kernel that forms delta and dP in different fp32 summation orders
    can meet (see test_one_hot_routing_backward)."""
    leaves = [c['q'], c['k'], c['v'], c['bias']]
    fn = _core_fn(c['mask'], 0.125, 1)
    r64 = _ref_grads(fn, leaves, c['dout'], torch.float64)
    r16 = _ref_grads(fn, leaves, c['dout'], BF16)
    bd = _Bound(case)
    for b in range(c['q'].shape[0]):
        for i, name in enumerate(NAMES):
            bd.check(f"{name}[{b}]", kern[i][b], r64[i][b], r16[i][b],
                     ref_max=r64[i].abs().max().item())
    for i, name in enumerate(NAMES):
        assert torch.isfinite(kern[i]).all(), f"{name} not finite"
    out, dq, dk, dv, dbias = kern
    for name, t in zip(NAMES[:4], (out, dq, dk, dv)):
        assert (t[5] == 0).all(), f"{name} of the fully masked entry != 0"
    masked_cols = ~c['mask'][:, None, None, :].expand_as(dbias)
    assert (dbias[masked_cols] == 0).all(), "dbias != 0 at a masked column"
    bd.done()


# ---------------------------------------------------------------------------
# 1. packed path


def _packed_inputs(B, L, r, W, seed=1):
    g = _gen(seed)
    h = 2
    mask = torch.rand(B, L, device=DEV, generator=g) > 0.2
    mask[:, 0] = True
    mask[0, 40:] = False          # padded tail
    mask[1, :] = False            # fully masked entry
    return dict(packed=_randn(B, L, W, gen=g),
                bias=_randn(B // r, h, L, L, gen=g), mask=mask,
                dout=_randn(B, h, L, 64, gen=g),
                dgate=_randn(B, L, 128, gen=g))


def _packed_ref_fn(mask, r, B, L):
    def fn(packed, bias):
        def view(off):
            return packed[..., off:off + 128].reshape(B, L, 2, 64) \
                .permute(0, 2, 1, 3)
        return ref_attention(view(0), view(128), view(256), bias, mask,
                             0.125, r)
    return fn


@pytest.mark.parametrize("W", [384, 512])
@pytest.mark.parametrize("B,L,r", [(6, 72, 3), (2, 200, 1)])
def test_packed_attention_parity(ext, B, L, r, W):
    """hip_attention_packed: q/k/v are channel slices of one (B, L, W)
    tensor, dq/dk/dv land in slices of one grad buffer."""
    from alphafold2_amd.ops.hip_autograd import hip_attention_packed
    c = _packed_inputs(B, L, r, W)
    packed = c['packed'].clone().requires_grad_(True)
    bias = c['bias'].clone().requires_grad_(True)
    out = hip_attention_packed(packed, 2, 128, bias, c['mask'], r)
    out.backward(c['dout'])

    bd = _Bound(f"packed[B={B},L={L},r={r},W={W}]")
    bd.check_all(['out', 'dpacked', 'dbias'],
                 [out.detach(), packed.grad, bias.grad],
                 _packed_ref_fn(c['mask'], r, B, L),
                 [c['packed'], c['bias']], c['dout'])
    if W > 384:
        assert (packed.grad[..., 384:] == 0).all(), \
            "unused gate block must get exactly zero gradient"
    assert torch.isfinite(packed.grad).all()
    assert (out.detach()[1] == 0).all(), "fully masked entry must output 0"
    bd.done()


@pytest.mark.parametrize("B,L,r", [(6, 72, 3), (2, 200, 1)])
def test_packed_attention_gated_parity(ext, B, L, r):
    """The module path: the gate block of the same packed tensor feeds
    hip_gatemul, so packed.grad's gate block is the gatemul gradient and
    autograd sums it with the attention's zero-filled block."""
    from alphafold2_amd.ops.hip_autograd import (hip_attention_packed,
                                                 hip_gatemul)
    c = _packed_inputs(B, L, r, 512, seed=2)
    packed = c['packed'].clone().requires_grad_(True)
    bias = c['bias'].clone().requires_grad_(True)
    out = hip_attention_packed(packed, 2, 128, bias, c['mask'], r)
    y = hip_gatemul(out.transpose(1, 2).reshape(B, L, 128),
                    packed.narrow(-1, 384, 128))
    y.backward(c['dgate'])

    attn = _packed_ref_fn(c['mask'], r, B, L)

    def fn(p, b):
        o = attn(p, b).transpose(1, 2).reshape(B, L, 128)
        return o * torch.sigmoid(p[..., 384:])

    bd = _Bound(f"packed_gated[B={B},L={L},r={r}]")
    bd.check_all(['y', 'dpacked', 'dbias'],
                 [y.detach(), packed.grad, bias.grad], fn,
                 [c['packed'], c['bias']], c['dgate'])
    assert torch.isfinite(packed.grad).all()
    bd.done()


# ---------------------------------------------------------------------------
# 2. dq_out / dk_out / dv_out write discipline


def test_bwd_out_views_write_discipline(ext):
    """attn_bwd writing through views into a NaN-filled (B, L, 512)
    buffer overwrites the q/k/v blocks completely, never touches the
    gate block, and gives bit-identical values to the plain call."""
    g = _gen(20)
    B, L, h = 2, 130, 2
    packed = _randn(B, L, 512, gen=g)
    bias = _randn(B, h, L, L, gen=g)
    mask = torch.rand(B, L, device=DEV, generator=g) > 0.2
    mask[:, 0] = True
    mask_u8 = mask.to(torch.uint8)
    dout = _randn(B, h, L, 64, gen=g)

    def view(t, off):
        return t.narrow(-1, off, 128).view(B, L, h, 64).permute(0, 2, 1, 3)

    q, k, v = view(packed, 0), view(packed, 128), view(packed, 256)
    out, lse = ext.attn_fwd(q, k, v, bias, mask_u8, 1, 0.125)
    plain = ext.attn_bwd(dout, q, k, v, out, lse, bias, mask_u8, 1, 0.125,
                         False)
    buf = torch.full_like(packed, float('nan'))
    ext.attn_bwd(dout, q, k, v, out, lse, bias, mask_u8, 1, 0.125, False,
                 dq_out=view(buf, 0), dk_out=view(buf, 128),
                 dv_out=view(buf, 256))
    torch.cuda.synchronize()
    assert not torch.isnan(buf[..., :384]).any(), "q/k/v block not covered"
    assert torch.isnan(buf[..., 384:]).all(), "gate block was written"
    for i, name in enumerate(['dq', 'dk', 'dv']):
        assert torch.equal(view(buf, 128 * i), plain[i]), name


# ---------------------------------------------------------------------------
# 3. strided q/k/v through hip_attention_core


def test_strided_qkv_parity(ext):
    """q a permuted view of (B, Lq, h*64); k, v the halves of one
    (B, Lk, 2*h*64) tensor (the to_kv(...).chunk(2) layout)."""
    from alphafold2_amd.ops.hip_autograd import hip_attention_core
    g = _gen(30)
    B, Lq, Lk, h = 3, 130, 72, 2
    qb0 = _randn(B, Lq, h * 64, gen=g)
    kvb0 = _randn(B, Lk, 2 * h * 64, gen=g)
    bias = _randn(B, h, Lq, Lk, gen=g)
    mask = torch.rand(B, Lk, device=DEV, generator=g) > 0.2
    mask[:, 0] = True
    dout = _randn(B, h, Lq, 64, gen=g)

    def views(qb, kvb):
        q = qb.reshape(B, Lq, h, 64).permute(0, 2, 1, 3)
        k = kvb[..., :h * 64].reshape(B, Lk, h, 64).permute(0, 2, 1, 3)
        v = kvb[..., h * 64:].reshape(B, Lk, h, 64).permute(0, 2, 1, 3)
        return q, k, v

    qb = qb0.clone().requires_grad_(True)
    kvb = kvb0.clone().requires_grad_(True)
    bs = bias.clone().requires_grad_(True)
    q, k, v = views(qb, kvb)
    assert not q.is_contiguous() and not k.is_contiguous() \
        and not v.is_contiguous()
    out = hip_attention_core(q, k, v, bias=bs, mask=mask)
    with torch.no_grad():
        out_c = hip_attention_core(q.contiguous(), k.contiguous(),
                                   v.contiguous(), bias=bias, mask=mask)
    assert torch.equal(out, out_c), \
        "strided and contiguous forward must be bit-identical"
    out.backward(dout)

    def fn(qb_, kvb_, b_):
        return ref_attention(*views(qb_, kvb_), b_, mask, 0.125)

    bd = _Bound("strided[3,130,72]")
    bd.check_all(['out', 'dq_base', 'dkv_base', 'dbias'],
                 [out.detach(), qb.grad, kvb.grad, bs.grad], fn,
                 [qb0, kvb0, bias], dout)
    bd.done()


# ---------------------------------------------------------------------------
# 4. dBias under bias_repeat


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("Lq,Lk", [(72, 72), (130, 72)])
@pytest.mark.parametrize("r", [1, 4])
def test_dbias_bias_repeat_parity(ext, r, Lq, Lk, use_mask):
    """All four gradients with bias (B / r, h, Lq, Lk): the dBias
    reference is autograd's gradient of the UN-repeated bias through
    repeat_interleave (the kernel's atomic fold over the axial dim)."""
    c = _dbias_inputs(r, Lq, Lk, use_mask)
    kern = _run_core(c['q'], c['k'], c['v'], c['bias'], c['mask'],
                     c['dout'], bias_repeat=r)
    _check_dbias_case(f"dbias[r={r},Lq={Lq},Lk={Lk},mask={int(use_mask)}]",
                      c, kern)


# ---------------------------------------------------------------------------
# 5. tied query with bias


def test_tied_query_with_bias_parity(ext):
    """B = 12, tie_dim = 6, bias_repeat = 4: batch / q_repeat and
    batch / bias_repeat are both live and different."""
    g = _gen(50)
    B, h, n, tie, r = 12, 2, 72, 6, 4
    q, k, v = (_randn(B, h, n, 64, gen=g) for _ in range(3))
    bias = _randn(B // r, h, n, n, gen=g)
    mask = torch.rand(B, n, device=DEV, generator=g) > 0.2
    mask[:, 0] = True
    dout = _randn(B, h, n, 64, gen=g)
    kern = _run_core(q, k, v, bias, mask, dout, bias_repeat=r, tie_dim=tie)
    bd = _Bound("tied_bias[B=12,tie=6,r=4]")
    bd.check_all(NAMES, kern, _core_fn(mask, 0.125, r, tie),
                 [q, k, v, bias], dout)
    dq = kern[1].reshape(B // tie, tie, h, n, 64)
    assert (dq == dq[:, :1]).all(), "dq must be constant in a tie group"
    bd.done()


# ---------------------------------------------------------------------------
# 6. whole masked tiles


def test_whole_masked_tiles(ext):
    c = _tile_mask_inputs()
    kern = _run_core(c['q'], c['k'], c['v'], c['bias'], c['mask'],
                     c['dout'])
    _check_tile_mask_case("tiles[6,130,200]", c, kern)


# ---------------------------------------------------------------------------
# 7. non-default scale, narrow head


@pytest.mark.parametrize("scale", [0.05, 1.0])
def test_explicit_scale_parity(ext, scale):
    g = _gen(70)
    B, h, Lq, Lk = 2, 2, 130, 72
    q, k, v = (_randn(B, h, Lq, 64, gen=g), _randn(B, h, Lk, 64, gen=g),
               _randn(B, h, Lk, 64, gen=g))
    bias = _randn(B, h, Lq, Lk, gen=g)
    dout = _randn(B, h, Lq, 64, gen=g)
    kern = _run_core(q, k, v, bias, None, dout, scale=scale)
    bd = _Bound(f"scale[{scale}]")
    bd.check_all(NAMES, kern, _core_fn(None, scale), [q, k, v, bias], dout)
    bd.done()


def test_narrow_head_explicit_scale_parity(ext):
    """dh = 32 runs zero-padded on the 64-wide tile; the explicit scale
    must reach the kernel unchanged."""
    g = _gen(71)
    B, h, Lq, Lk, scale = 2, 2, 72, 130, 0.3
    q, k, v = (_randn(B, h, Lq, 32, gen=g), _randn(B, h, Lk, 32, gen=g),
               _randn(B, h, Lk, 32, gen=g))
    bias = _randn(B, h, Lq, Lk, gen=g)
    mask = torch.rand(B, Lk, device=DEV, generator=g) > 0.2
    mask[:, 0] = True
    dout = _randn(B, h, Lq, 32, gen=g)
    kern = _run_core(q, k, v, bias, mask, dout, scale=scale)
    bd = _Bound("narrow_head[dh=32,scale=0.3]")
    bd.check_all(NAMES, kern, _core_fn(mask, scale), [q, k, v, bias], dout)
    bd.done()


# ---------------------------------------------------------------------------
# 8. one-hot routing: index exactness with derived bounds


def _perm(Lq, Lk, boundary):
    pi = (7 * torch.arange(Lq, device=DEV) + 3) % Lk
    if boundary:
        pi[:6] = torch.tensor([0, 63, 64, 127, 128, 199], device=DEV)
    return pi


def _routing_inputs(Lq, Lk, boundary, use_mask, seed):
    g = _gen(seed)
    B, h = 2, 2
    q = (0.1 * torch.randn(B, h, Lq, 64, device=DEV, generator=g)).to(BF16)
    k = (0.1 * torch.randn(B, h, Lk, 64, device=DEV, generator=g)).to(BF16)
    v = _randn(B, h, Lk, 64, gen=g)
    dout = _randn(B, h, Lq, 64, gen=g)
    pi = _perm(Lq, Lk, boundary)
    bias = torch.zeros(B, h, Lq, Lk, device=DEV, dtype=BF16)
    bias[:, :, torch.arange(Lq, device=DEV), pi] = 32.
    mask = None
    if use_mask:
        # remove only keys no query routes to
        mask = torch.rand(B, Lk, device=DEV, generator=g) > 0.5
        mask[:, pi] = True
    return q, k, v, bias, mask, dout, pi


@pytest.mark.parametrize("use_mask", [False, True])
def test_one_hot_routing_forward(ext, use_mask):
    """bias[i, pi(i)] = 32 makes P[i, pi(i)] round to exactly 1 and the
    leak from all other keys (<= 200 e^-32) vanish below a bf16 ulp of
    any v entry: out[i] must be v[pi(i)] to output rounding.  The first
    six queries route to the tile-boundary keys."""
    q, k, v, bias, mask, dout, pi = _routing_inputs(130, 200, True,
                                                    use_mask, 80)
    kern = _run_core(q, k, v, bias, mask, dout)
    want = v[:, :, pi].double()
    err = (kern[0].double() - want).abs()
    assert (err <= 2.0 ** -8 * want.abs() + 1e-6).all(), err.max().item()


@pytest.mark.parametrize("use_mask", [False, True])
def test_one_hot_routing_backward(ext, use_mask):
    """Pure permutation pi(i) = (7 i + 3) mod 200: dv[pi(i)] = dout[i] to
    output rounding, and dq, dk, dbias vanish up to the fp32
    accumulation-order difference between delta and the MFMA dP
    (<= 64 * 16 * 2^-24 ~ 6e-5 before the |k| <= 0.5 scaling).  Every
    key is a target here, so the mask removes none and only selects the
    masked kernel variant."""
    q, k, v, bias, mask, dout, pi = _routing_inputs(200, 200, False,
                                                    use_mask, 81)
    assert pi.unique().numel() == 200
    out, dq, dk, dv, dbias = _run_core(q, k, v, bias, mask, dout)
    want = dout.double()
    err = (dv[:, :, pi].double() - want).abs()
    assert (err <= 2.0 ** -8 * want.abs() + 1e-6).all(), err.max().item()
    for name, t in (('dq', dq), ('dk', dk), ('dbias', dbias)):
        assert t.abs().max().item() <= 1e-3, (name, t.abs().max().item())


# ---------------------------------------------------------------------------
# 9. module-level padded run with proof that the fused kernel ran


def test_axial_attention_padded_runs_fused_kernel():
    """AxialAttention on a padded batch under bf16 autocast: the packed
    fused kernel must be ENTERED (spy) with no eager-composition
    warning, and output and gradients must lie within the bound of the
    fp32 eager module at valid positions (floor: eager under autocast)."""
    from alphafold2_amd.models.evoformer import AxialAttention
    from alphafold2_amd.ops import dispatch, hip_autograd

    torch.manual_seed(9)
    ref = AxialAttention(dim=128, heads=2, dim_head=64, row_attn=True,
                         col_attn=False, accept_edges=True)
    torch.nn.init.normal_(ref.attn.to_out.weight, std=128 ** -0.5)
    torch.nn.init.normal_(ref.attn.to_out.bias, std=0.1)
    torch.nn.init.normal_(ref.attn.gating.weight, std=128 ** -0.5)
    torch.nn.init.normal_(ref.attn.gating.bias, std=0.5)
    ref = ref.to(DEV)
    x0 = torch.randn(2, 6, 72, 128, device=DEV)
    e0 = torch.randn(2, 72, 72, 128, device=DEV)
    mask = torch.ones(2, 6, 72, dtype=torch.bool, device=DEV)
    mask[0, :, 50:] = False       # padded tail, item 0
    mask[0, 4:] = False           # two fully masked rows
    seq_valid = mask.any(dim=1)
    pair_valid = seq_valid[:, :, None] & seq_valid[:, None, :]
    names = ['out', 'dx', 'dedges'] + [n for n, _ in ref.named_parameters()]

    def run(force_eager, autocast):
        m = AxialAttention(dim=128, heads=2, dim_head=64, row_attn=True,
                           col_attn=False, accept_edges=True).to(DEV)
        m.load_state_dict(ref.state_dict())
        m.train()
        x = x0.clone().requires_grad_(True)
        e = e0.clone().requires_grad_(True)
        prev = dispatch._FORCE_EAGER
        dispatch._FORCE_EAGER = force_eager
        try:
            with torch.autocast('cuda', dtype=BF16, enabled=autocast):
                out = m(x, edges=e, mask=mask)
            loss = out[mask].float().pow(2).mean()
            loss.backward()
        finally:
            dispatch._FORCE_EAGER = prev
        return [out.detach()[mask].float(), x.grad[mask], e.grad[pair_valid]] \
            + [p.grad for _, p in m.named_parameters()]

    warned = set(dispatch._warned)
    dispatch._warned.clear()
    try:
        with mock.patch.object(
                hip_autograd, 'hip_attention_packed',
                wraps=hip_autograd.hip_attention_packed) as spy, \
                warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            kern = run(False, True)
    finally:
        dispatch._warned.update(warned)
    assert spy.call_count >= 1, "the packed fused kernel was never entered"
    eager_warn = [str(w.message) for w in caught
                  if issubclass(w.category, RuntimeWarning)
                  and 'EAGER composition' in str(w.message)]
    assert not eager_warn, eager_warn

    r32 = run(True, False)
    floor = run(True, True)
    bd = _Bound("axial_padded")
    for name, kt, rt, ft in zip(names, kern, r32, floor):
        assert torch.isfinite(kt).all(), name
        bd.check(name, kt, rt.double(), ft)
    bd.done()


# ---------------------------------------------------------------------------
# 10. split dK/dV kernels (AF2AMD_SPLIT_DKV=1, read once per process)

_CHILD = r'''
import sys
import torch
from alphafold2_amd.ops.hip_autograd import hip_attention_core
cases = torch.load(sys.argv[1])
res = {}
for name, c in cases.items():
    xs = [c[n].cuda().requires_grad_(True) for n in ('q', 'k', 'v', 'bias')]
    mask = c['mask'].cuda() if c['mask'] is not None else None
    out = hip_attention_core(xs[0], xs[1], xs[2], bias=xs[3], mask=mask,
                             bias_repeat=c['r'])
    out.backward(c['dout'].cuda())
    torch.cuda.synchronize()
    res[name] = [out.detach().cpu()] + [x.grad.cpu() for x in xs]
torch.save(res, sys.argv[2])
'''


def test_split_dkv_parity(ext):
    """The split dV / dK(+dBias) kernels on the bias_repeat = 4 masked
    cases and the whole-masked-tile case, in one child process."""
    cases = {'dbias72': _dbias_inputs(4, 72, 72, True),
             'dbias130': _dbias_inputs(4, 130, 72, True),
             'tiles': _tile_mask_inputs()}
    env = dict(os.environ)
    env['AF2AMD_SPLIT_DKV'] = '1'
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, 'in.pt'), os.path.join(tmp, 'out.pt')
        torch.save({n: {k: (t.cpu() if torch.is_tensor(t) else t)
                        for k, t in c.items()} for n, c in cases.items()},
                   fin)
        subprocess.run([sys.executable, '-c', _CHILD, fin, fout], env=env,
                       cwd=ROOT, timeout=120, check=True)
        res = torch.load(fout)
    kern = {n: [t.to(DEV) for t in ts] for n, ts in res.items()}
    _check_dbias_case("split_dbias[r=4,Lq=72,Lk=72,mask=1]",
                      cases['dbias72'], kern['dbias72'])
    _check_dbias_case("split_dbias[r=4,Lq=130,Lk=72,mask=1]",
                      cases['dbias130'], kern['dbias130'])
    _check_tile_mask_case("split_tiles[6,130,200]", cases['tiles'],
                          kern['tiles'])


# ---------------------------------------------------------------------------
# host-side operand checks: each raises before any launch


def _small_call(ext, **over):
    """Arguments of a valid attn_fwd call, with overrides."""
    g = _gen(90)
    B, h, L = 4, 2, 72
    a = dict(q=_randn(B, h, L, 64, gen=g), k=_randn(B, h, L, 64, gen=g),
             v=_randn(B, h, L, 64, gen=g), bias=_randn(2, h, L, L, gen=g),
             mask=torch.ones(B, L, dtype=torch.uint8, device=DEV),
             bias_repeat=2, scale=0.125)
    a.update(over)
    return a


def _fwd(ext, a):
    return ext.attn_fwd(a['q'], a['k'], a['v'], a['bias'], a['mask'],
                        a['bias_repeat'], a['scale'])


def _bwd(ext, a, out, lse, dout, **kw):
    return ext.attn_bwd(dout, a['q'], a['k'], a['v'], out, lse, a['bias'],
                        a['mask'], a['bias_repeat'], a['scale'], False, **kw)


@pytest.mark.parametrize("bad", [
    dict(k=torch.float32), dict(v=torch.float16), dict(bias=torch.float32),
    dict(bias_shape=(4, 2, 72, 72)), dict(bias_shape=(2, 2, 72, 64)),
    dict(bias_shape=(2, 1, 72, 72)), dict(bias_repeat=3)])
def test_attn_fwd_rejects_mismatched_operands(ext, bad):
    a = _small_call(ext)
    for key, val in bad.items():
        if key == 'bias_shape':
            a['bias'] = torch.zeros(*val, device=DEV, dtype=BF16)
        elif key == 'bias_repeat':
            a['bias_repeat'] = val
        else:
            a[key] = a[key].to(val)
    with pytest.raises(RuntimeError):
        _fwd(ext, a)


def test_attn_bwd_rejects_mismatched_operands(ext):
    a = _small_call(ext)
    out, lse = _fwd(ext, a)
    dout = torch.ones_like(out)
    _bwd(ext, a, out, lse, dout)           # the valid call passes
    with pytest.raises(RuntimeError):
        _bwd(ext, a, out, lse, dout.float())
    for key in ('k', 'v', 'bias'):
        b = dict(a)
        b[key] = a[key].float()
        with pytest.raises(RuntimeError):
            _bwd(ext, b, out, lse, dout)
    b = dict(a, bias=a['bias'][:1])
    with pytest.raises(RuntimeError):
        _bwd(ext, b, out, lse, dout)
    b = dict(a, bias=None)
    with pytest.raises(RuntimeError):      # need_dbias without a bias
        ext.attn_bwd(dout, b['q'], b['k'], b['v'], out, lse, None,
                     b['mask'], 1, 0.125, True)

    def buf(t):
        return torch.empty_like(t.contiguous())

    dq, dk, dv = buf(a['q']), buf(a['k']), buf(a['v'])
    _bwd(ext, a, out, lse, dout, dq_out=dq, dk_out=dk, dv_out=dv)
    with pytest.raises(RuntimeError):      # not given together
        _bwd(ext, a, out, lse, dout, dq_out=dq)
    with pytest.raises(RuntimeError):
        _bwd(ext, a, out, lse, dout, dq_out=dq, dk_out=dk)
    with pytest.raises(RuntimeError):      # wrong dtype
        _bwd(ext, a, out, lse, dout, dq_out=dq.float(), dk_out=dk,
             dv_out=dv)
    with pytest.raises(RuntimeError):      # wrong shape
        _bwd(ext, a, out, lse, dout, dq_out=dq, dk_out=dk[:, :, :64],
             dv_out=dv)
    torch.cuda.synchronize()
