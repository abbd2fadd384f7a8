"""Attention-probability dropout inside the fused attention kernels.

The keep mask is a pure function of (seed, offset) and the position
(docs/PARITY.md, ops/hip/attn_dropout.h):

    Philox4x32-10, key = seed, counter = (offset, subsequence),
    subsequence = (bh * ceil(Lq/4) + (i>>2)) * ceil(Lk/4) + (j>>2),
    element (i, j) = byte (j&3) of output word (i&3),
    keep iff byte >= T,  T = clamp(round(256 p), 1, 255),
    kept probabilities are scaled by 256 / (256 - T).

`np_keep_mask` below is that definition in numpy.  It is checked, on any
machine, against tests/golden/attn_dropout_philox.json, which
tools/philox_check.cpp wrote from at::Philox4_32 alone; on the GPU the
mask the kernels use (`ext.attn_dropout_mask`, the same device function
the forward and backward kernels call) is compared with it bit for bit.

Parity uses the conventions of tests/test_attention_paths.py: one
plain-torch reference, here with the explicit keep mask and rescale,
evaluated in float64 and in bf16, and the bound

    E_kernel <= 2 * E_floor + 2**-8 * max|ref64|

Each check prints `EVIDENCE case output E_kernel E_floor ratio bound`
before it asserts; docs/EVIDENCE.md holds the measured table.
"""
import json
import math
import os
import warnings
from unittest import mock

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

DEV = 'cuda'
BF16 = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'attn_dropout_philox.json')


@pytest.fixture(scope="module")
def ext():
    from alphafold2_amd.ops.dispatch import _load_ext
    e = _load_ext()
    assert e is not None, "extension must load on GPU box"
    return e


# ---------------------------------------------------------------------------
# the definition, in numpy


def np_philox4x32_10(seed, subseq, offset):
    """First 128-bit output of Philox4x32-10 per subsequence: (..., 4)
    uint32 words.  32x32-bit products are formed in uint64."""
    u = np.uint64
    lo32, s32 = u(0xffffffff), u(32)
    subseq = np.asarray(subseq, dtype=np.uint64)
    c = [np.full_like(subseq, offset & 0xffffffff),
         np.full_like(subseq, offset >> 32), subseq & lo32, subseq >> s32]
    k0, k1 = seed & 0xffffffff, seed >> 32
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c[0], u(0xCD9E8D57) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ u(k0), p1 & lo32,
             (p0 >> s32) ^ c[3] ^ u(k1), p0 & lo32]
        k0 = (k0 + 0x9E3779B9) & 0xffffffff
        k1 = (k1 + 0xBB67AE85) & 0xffffffff
    return np.stack(c, axis=-1).astype(np.uint32)


def drop_threshold(p):
    return min(255, max(1, int(math.floor(p * 256 + 0.5))))


def np_keep_mask(seed, offset, BH, Lq, Lk, T):
    """(BH, Lq, Lk) uint8 keep mask by the definition."""
    H4, W4 = (Lq + 3) // 4, (Lk + 3) // 4
    bh, ib, jb = np.meshgrid(np.arange(BH, dtype=np.uint64),
                             np.arange(H4, dtype=np.uint64),
                             np.arange(W4, dtype=np.uint64), indexing='ij')
    blocks = np_philox4x32_10(seed, (bh * np.uint64(H4) + ib) * np.uint64(W4)
                              + jb, offset)            # (BH, H4, W4, 4)
    i, j = np.arange(Lq)[:, None], np.arange(Lk)[None, :]
    words = blocks[:, i >> 2, j >> 2, i & 3]           # (BH, Lq, Lk)
    byte = (words >> (8 * (j & 3)).astype(np.uint32)) & np.uint32(0xff)
    return (byte >= T).astype(np.uint8)


def test_numpy_reference_matches_philox_engine():
    """No GPU: the numpy definition against vectors and a keep mask that
    tools/philox_check.cpp produced from at::Philox4_32(seed,
    subsequence, offset), across the 32-bit boundaries of all three."""
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert len(gold['vectors']) >= 20
    for seed, sub, off, words in gold['vectors']:
        got = np_philox4x32_10(int(seed), np.uint64(int(sub)), int(off))
        assert got.tolist() == words, (seed, sub, off)
    m = gold['mask']
    want = np.array([int(ch) for ch in m['keep']], dtype=np.uint8) \
        .reshape(m['BH'], m['Lq'], m['Lk'])
    got = np_keep_mask(int(m['seed']), int(m['offset']), m['BH'], m['Lq'],
                       m['Lk'], m['T'])
    assert np.array_equal(got, want)
    for p, t in gold['threshold'].items():
        assert drop_threshold(float(p)) == t, p


# ---------------------------------------------------------------------------
# reference and bound (conventions of tests/test_attention_paths.py)


def ref_attention(q, k, v, bias, key_mask, scale, bias_repeat=1,
                  tie_dim=None, keep=None, rescale=1.0):
    """softmax(q k^T * scale + repeat_interleave(bias) + key mask), then
    dropout by the explicit `keep` mask (B, h, Lq, Lk) and `rescale`,
    times v; in the dtype of its inputs.  A row whose keys are all
    masked gives 0; tie_dim replaces each query by its group mean."""
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
    if keep is not None:
        p = p * keep.to(p.dtype) * rescale
    return torch.einsum('bhij,bhjd->bhid', p, v)


def _ref_grads(fn, leaves, dout, dtype):
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


def _state(seed, offset):
    return torch.tensor([seed, offset], dtype=torch.int64, device=DEV)


STATES = [(1234, 12), (0x5eed5eed12345, 2 ** 32 + 8)]


def _rescale(p):
    return 256.0 / (256 - drop_threshold(p))


def _drop_fn(ext, rng_state, shape, p, mask, scale, bias_repeat=1,
             tie_dim=None):
    """Reference closure with the mask dumped from `rng_state`."""
    keep = ext.attn_dropout_mask(rng_state, *shape, p)
    return lambda q, k, v, bias=None: ref_attention(
        q, k, v, bias, mask, scale, bias_repeat, tie_dim, keep, _rescale(p))


def _run_core(q, k, v, bias, mask, dout, **kw):
    """[out, dq, dk, dv, dbias] from hip_attention_core, then whatever
    else it returned (the rng_state under return_rng_state)."""
    from alphafold2_amd.ops.hip_autograd import hip_attention_core
    xs = [t.detach().clone().requires_grad_(True)
          for t in (q, k, v, bias) if t is not None]
    b = xs[3] if bias is not None else None
    ret = hip_attention_core(xs[0], xs[1], xs[2], bias=b, mask=mask, **kw)
    out, rest = (ret[0], list(ret[1:])) if isinstance(ret, tuple) \
        else (ret, [])
    out.backward(dout)
    return [out.detach()] + [x.grad for x in xs], rest


# ---------------------------------------------------------------------------
# 1. mask definition


@gpu
@pytest.mark.parametrize("p", [0.25, 0.1])
@pytest.mark.parametrize("seed,offset", STATES)
def test_mask_definition(ext, seed, offset, p):
    """attn_dropout_mask == the numpy definition, bit for bit, at lengths
    that are no multiple of 4 and an offset above 2^32."""
    B, H, Lq, Lk = 2, 3, 70, 130
    got = ext.attn_dropout_mask(_state(seed, offset), B, H, Lq, Lk, p)
    assert got.dtype == torch.uint8 and got.shape == (B, H, Lq, Lk)
    want = np_keep_mask(seed, offset, B * H, Lq, Lk, drop_threshold(p))
    assert np.array_equal(got.cpu().numpy().reshape(B * H, Lq, Lk), want)


# ---------------------------------------------------------------------------
# 2. core parity, forward and backward


def _core_inputs(seed=3):
    g = _gen(seed)
    B, h, Lq, Lk, r = 4, 2, 130, 200, 2
    mask = torch.ones(B, Lk, dtype=torch.bool, device=DEV)
    mask[0, 150:] = False         # padded tail
    mask[1, :] = False            # fully masked entry
    mask[3] = torch.rand(Lk, device=DEV, generator=g) > 0.2
    mask[3, 0] = True
    return dict(q=_randn(B, h, Lq, 64, gen=g), k=_randn(B, h, Lk, 64, gen=g),
                v=_randn(B, h, Lk, 64, gen=g),
                bias=_randn(B // r, h, Lq, Lk, gen=g), mask=mask,
                dout=_randn(B, h, Lq, 64, gen=g), r=r)


@gpu
@pytest.mark.parametrize("p", [0.25, 0.1])
@pytest.mark.parametrize("seed,offset", STATES)
def test_core_parity(ext, seed, offset, p):
    """(B, h, Lq, Lk) = (4, 2, 130, 200): forward tile boundary at 128,
    ragged dQ and KV tails, bias_repeat = 2 with dbias, a padded tail and
    one fully masked entry whose outputs are exactly 0."""
    c = _core_inputs()
    st = _state(seed, offset)
    kern, _ = _run_core(c['q'], c['k'], c['v'], c['bias'], c['mask'],
                        c['dout'], bias_repeat=c['r'], dropout_p=p,
                        rng_state=st)
    assert st.tolist() == [seed, offset], "a given rng_state is read only"
    fn = _drop_fn(ext, st, (4, 2, 130, 200), p, c['mask'], 0.125, c['r'])
    bd = _Bound(f"drop_core[p={p},offset={offset}]")
    bd.check_all(NAMES, kern, fn, [c['q'], c['k'], c['v'], c['bias']],
                 c['dout'])
    for name, t in zip(NAMES[:4], kern[:4]):
        assert (t[1] == 0).all(), f"{name} of the fully masked entry != 0"
    masked_cols = ~c['mask'].reshape(2, 2, 200).any(dim=1)
    dbias = kern[4]
    assert (dbias.permute(0, 3, 1, 2)[masked_cols] == 0).all(), \
        "dbias != 0 at a column masked in its whole repeat group"
    bd.done()


@gpu
@pytest.mark.parametrize("p", [0.25, 0.1])
def test_core_parity_no_bias_no_mask(ext, p):
    g = _gen(5)
    q, k, v, dout = (_randn(2, 2, 64, 64, gen=g) for _ in range(4))
    st = _state(*STATES[0])
    kern, _ = _run_core(q, k, v, None, None, dout, dropout_p=p, rng_state=st)
    bd = _Bound(f"drop_plain64[p={p}]")
    bd.check_all(NAMES[:4], kern,
                 _drop_fn(ext, st, (2, 2, 64, 64), p, None, 0.125),
                 [q, k, v], dout)
    bd.done()


# ---------------------------------------------------------------------------
# 3. other entry points; the state is drawn from the default generator
# and the reference mask is dumped from the state that comes back


@gpu
def test_tied_query_dropout_parity(ext):
    """tie_dim = 2 with bias: one mean query per group, but every batch
    entry drops its own positions (as the eager composition does)."""
    g = _gen(50)
    B, h, n, tie, r, p = 4, 2, 72, 2, 2, 0.25
    q, k, v = (_randn(B, h, n, 64, gen=g) for _ in range(3))
    bias = _randn(B // r, h, n, n, gen=g)
    mask = torch.rand(B, n, device=DEV, generator=g) > 0.2
    mask[:, 0] = True
    dout = _randn(B, h, n, 64, gen=g)
    kern, (st,) = _run_core(q, k, v, bias, mask, dout, bias_repeat=r,
                            tie_dim=tie, dropout_p=p, return_rng_state=True)
    keep = ext.attn_dropout_mask(st, B, h, n, n, p)
    assert not torch.equal(keep[0], keep[1]), \
        "members of a tie group must not share a mask"
    bd = _Bound("drop_tied[B=4,tie=2,r=2]")
    bd.check_all(NAMES, kern, _drop_fn(ext, st, (B, h, n, n), p, mask, 0.125,
                                       r, tie), [q, k, v, bias], dout)
    dq = kern[1].reshape(B // tie, tie, h, n, 64)
    assert (dq == dq[:, :1]).all(), "dq must be constant in a tie group"
    bd.done()


@gpu
def test_packed_dropout_parity(ext):
    """W = 512 packed projection with a gate block: gradient slices
    written, gate slice exactly zero."""
    from alphafold2_amd.ops.hip_autograd import hip_attention_packed
    g = _gen(1)
    B, L, r, h, p = 6, 72, 3, 2, 0.25
    mask = torch.rand(B, L, device=DEV, generator=g) > 0.2
    mask[:, 0] = True
    mask[0, 40:] = False
    mask[1, :] = False
    packed0 = _randn(B, L, 512, gen=g)
    bias0 = _randn(B // r, h, L, L, gen=g)
    dout = _randn(B, h, L, 64, gen=g)
    packed = packed0.clone().requires_grad_(True)
    bias = bias0.clone().requires_grad_(True)
    out, st = hip_attention_packed(packed, h, 128, bias, mask, r,
                                   dropout_p=p, return_rng_state=True)
    out.backward(dout)
    keep = ext.attn_dropout_mask(st, B, h, L, L, p)

    def fn(pk, b):
        def view(off):
            return pk[..., off:off + 128].reshape(B, L, 2, 64) \
                .permute(0, 2, 1, 3)
        return ref_attention(view(0), view(128), view(256), b, mask, 0.125,
                             r, None, keep, _rescale(p))

    bd = _Bound("drop_packed[B=6,L=72,r=3,W=512]")
    bd.check_all(['out', 'dpacked', 'dbias'],
                 [out.detach(), packed.grad, bias.grad], fn,
                 [packed0, bias0], dout)
    assert (packed.grad[..., 384:] == 0).all(), \
        "unused gate block must get exactly zero gradient"
    assert (out.detach()[1] == 0).all(), "fully masked entry must output 0"
    bd.done()


@gpu
def test_narrow_head_dropout_parity(ext):
    """dh = 32 runs zero-padded on the 64-wide tile; dropout_p and the
    state pass through the padding recursion."""
    g = _gen(71)
    B, h, Lq, Lk, p = 2, 2, 72, 130, 0.1
    q, k, v = (_randn(B, h, Lq, 32, gen=g), _randn(B, h, Lk, 32, gen=g),
               _randn(B, h, Lk, 32, gen=g))
    bias = _randn(B, h, Lq, Lk, gen=g)
    mask = torch.rand(B, Lk, device=DEV, generator=g) > 0.2
    mask[:, 0] = True
    dout = _randn(B, h, Lq, 32, gen=g)
    kern, (st,) = _run_core(q, k, v, bias, mask, dout, dropout_p=p,
                            return_rng_state=True)
    bd = _Bound("drop_narrow_head[dh=32]")
    bd.check_all(NAMES, kern,
                 _drop_fn(ext, st, (B, h, Lq, Lk), p, mask, 32 ** -0.5),
                 [q, k, v, bias], dout)
    bd.done()


# ---------------------------------------------------------------------------
# 4. statistics and state


@gpu
@pytest.mark.parametrize("p", [0.25, 0.1])
def test_keep_fraction_and_independence(ext, p):
    keep = ext.attn_dropout_mask(_state(*STATES[0]), 2, 2, 256, 256, p)
    n = keep.numel()
    p_eff = drop_threshold(p) / 256
    assert abs(p_eff - p) <= 2.0 ** -9
    sigma = math.sqrt(p_eff * (1 - p_eff) / n)
    frac = keep.float().mean().item()
    print(f"EVIDENCE keep_fraction[p={p}] frac={frac:.5f} "
          f"want={1 - p_eff:.5f} sigma={sigma:.2e}")
    assert abs(frac - (1 - p_eff)) <= 5 * sigma
    flat = keep.reshape(4, -1)
    for a in range(4):
        for b in range(a + 1, 4):
            assert not torch.equal(flat[a], flat[b]), (a, b)


def _fwd_bwd(ext, c, p):
    out, lse, st = ext.attn_fwd(c['q'], c['k'], c['v'], c['bias'], None, 1,
                                0.125, dropout_p=p)
    dq, dk, dv = ext.attn_bwd(c['dout'], c['q'], c['k'], c['v'], out, lse,
                              c['bias'], None, 1, 0.125, False, dropout_p=p,
                              rng_state=st)
    return [out, dq, dk, dv], st


@gpu
def test_offset_advances_and_seed_reproduces(ext):
    g = _gen(8)
    B, h, L, p = 2, 2, 130, 0.25
    c = dict(q=_randn(B, h, L, 64, gen=g), k=_randn(B, h, L, 64, gen=g),
             v=_randn(B, h, L, 64, gen=g), bias=_randn(B, h, L, L, gen=g),
             dout=_randn(B, h, L, 64, gen=g))
    torch.cuda.manual_seed(77)
    r1, s1 = _fwd_bwd(ext, c, p)
    r2, s2 = _fwd_bwd(ext, c, p)
    assert s1[0].item() == 77 and s2[0].item() == 77
    assert s2[1].item() > s1[1].item(), "the offset must advance per call"
    m1 = ext.attn_dropout_mask(s1, B, h, L, L, p)
    m2 = ext.attn_dropout_mask(s2, B, h, L, L, p)
    assert not torch.equal(m1, m2)
    assert not torch.equal(r1[0], r2[0])
    torch.cuda.manual_seed(77)
    r3, s3 = _fwd_bwd(ext, c, p)
    assert torch.equal(s3, s1)
    for name, a, b in zip(NAMES, r1, r3):
        assert torch.equal(a, b), f"{name} differs after the same seed"


# ---------------------------------------------------------------------------
# 5. off means off


@gpu
def test_dropout_off_is_todays_call(ext):
    from alphafold2_amd.ops import dispatch
    from alphafold2_amd.ops.hip_autograd import hip_attention_core
    g = _gen(9)
    B, h, L = 2, 2, 130
    q, k, v = (_randn(B, h, L, 64, gen=g) for _ in range(3))
    bias = _randn(B, h, L, L, gen=g)
    mask = torch.rand(B, L, device=DEV, generator=g) > 0.2
    mask[:, 0] = True
    m8 = mask.to(torch.uint8)
    dout = _randn(B, h, L, 64, gen=g)

    base = ext.attn_fwd(q, k, v, bias, m8, 1, 0.125)
    off = ext.attn_fwd(q, k, v, bias, m8, 1, 0.125, dropout_p=0.0)
    assert len(base) == 2 and len(off) == 2
    assert torch.equal(base[0], off[0]) and torch.equal(base[1], off[1])
    g0 = ext.attn_bwd(dout, q, k, v, base[0], base[1], bias, m8, 1, 0.125,
                      False)
    g1 = ext.attn_bwd(dout, q, k, v, base[0], base[1], bias, m8, 1, 0.125,
                      False, dropout_p=0.0)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)

    want = hip_attention_core(q, k, v, bias=bias, mask=mask)
    assert torch.equal(want, hip_attention_core(q, k, v, bias=bias,
                                                mask=mask, dropout_p=0.))
    assert torch.equal(want, dispatch.attention_core(
        q, k, v, bias=bias, mask=mask, dropout=0.25, training=False))
    assert torch.equal(want, dispatch.attention_core(
        q, k, v, bias=bias, mask=mask, dropout=0., training=True))


@gpu
def test_dropout_operand_checks(ext):
    """Each bad rng_state / dropout_p raises before any launch."""
    g = _gen(10)
    q, k, v = (_randn(1, 1, 64, 64, gen=g) for _ in range(3))
    st = _state(1, 0)

    def fwd(p, s):
        return ext.attn_fwd(q, k, v, None, None, 1, 0.125, dropout_p=p,
                            rng_state=s)

    out, lse, _ = fwd(0.5, st)
    for p, s in [(1.0, st), (-0.1, st), (0.5, st.to(torch.int32)),
                 (0.5, st.cpu()), (0.5, torch.zeros(3, dtype=torch.int64,
                                                    device=DEV))]:
        with pytest.raises(RuntimeError):
            fwd(p, s)
        with pytest.raises(RuntimeError):
            ext.attn_bwd(out, q, k, v, out, lse, None, None, 1, 0.125, False,
                         dropout_p=p, rng_state=s)
    with pytest.raises(RuntimeError):      # backward needs the state
        ext.attn_bwd(out, q, k, v, out, lse, None, None, 1, 0.125, False,
                     dropout_p=0.5)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 6. model level: Attention with dropout runs the fused kernels


def _attention_module(seed=11):
    from alphafold2_amd.models.evoformer import Attention
    torch.manual_seed(seed)
    m = Attention(dim=128, heads=2, dim_head=64, dropout=0.25)
    # to_out is zero-initialised: give it weight so the output depends
    # on the attention at all
    torch.nn.init.normal_(m.to_out.weight, std=128 ** -0.5)
    torch.nn.init.normal_(m.gating.weight, std=128 ** -0.5)
    return m.to(DEV, BF16)


@gpu
@pytest.mark.parametrize("cross", [False, True])
def test_attention_module_dropout_runs_fused(ext, cross):
    import alphafold2_amd.ops as ops_pkg
    from alphafold2_amd.ops import dispatch, hip_autograd
    m = _attention_module().train()
    g = _gen(12)
    x = _randn(3, 72, 128, gen=g)
    ctx = _randn(3, 50, 128, gen=g) if cross else None
    seen = []
    real_fwd = ext.attn_fwd

    def spy_fwd(*a, **kw):
        seen.append(kw.get('dropout_p', 0.0))
        return real_fwd(*a, **kw)

    warned = set(dispatch._warned)
    dispatch._warned.clear()
    try:
        with mock.patch.object(ext, 'attn_fwd', spy_fwd), \
                mock.patch.object(
                    ops_pkg, 'attention_core_packed',
                    wraps=dispatch.attention_core_packed) as packed_spy, \
                mock.patch.object(
                    hip_autograd, 'hip_attention_packed',
                    wraps=hip_autograd.hip_attention_packed) as hip_spy, \
                warnings.catch_warnings():
            # an eager fallback announces itself with a RuntimeWarning
            warnings.simplefilter('error', RuntimeWarning)
            xs = x.clone().requires_grad_(True)
            y1 = m(xs, context=ctx)
            y1.float().pow(2).mean().backward()
            y2 = m(x, context=ctx)
    finally:
        dispatch._warned.update(warned)
    assert len(seen) == 2 and all(p == 0.25 for p in seen), seen
    if not cross:
        assert packed_spy.call_count == 2 and hip_spy.call_count == 2, \
            "self-attention with dropout must take the packed path"
    assert torch.isfinite(y1).all() and torch.isfinite(xs.grad).all()
    assert not torch.equal(y1, y2), "two training calls must differ"

    m.eval()
    seen.clear()
    with mock.patch.object(ext, 'attn_fwd', spy_fwd), torch.no_grad():
        e1, e2 = m(x, context=ctx), m(x, context=ctx)
    assert torch.equal(e1, e2), ".eval() must be deterministic"
    assert seen == [0.0, 0.0], seen


# ---------------------------------------------------------------------------
# 7. recompute under activation checkpointing


@gpu
def test_checkpoint_recompute_reproduces_mask(ext):
    """preserve_rng_state restores the generator before the recompute,
    so the recomputed forward draws the same (seed, offset): gradients
    equal those of the un-checkpointed run from the same seed."""
    from torch.utils.checkpoint import checkpoint
    m = _attention_module().train()
    x = _randn(3, 72, 128, gen=_gen(13))

    def run(use_ckpt):
        m.zero_grad(set_to_none=True)
        torch.cuda.manual_seed(21)
        xs = x.clone().requires_grad_(True)
        y = checkpoint(m, xs, use_reentrant=False, preserve_rng_state=True) \
            if use_ckpt else m(xs)
        y.float().pow(2).mean().backward()
        return [y.detach(), xs.grad] + [p.grad.clone()
                                        for p in m.parameters()]

    plain, ckpt = run(False), run(True)
    assert plain[1].abs().max() > 0
    names = ['y', 'dx'] + [n for n, _ in m.named_parameters()]
    for name, a, b in zip(names, plain, ckpt):
        assert torch.equal(a, b), f"{name} differs under checkpointing"
    # and the seed matters: another seed gives another mask
    torch.cuda.manual_seed(22)
    assert not torch.equal(m(x), plain[0])


# ---------------------------------------------------------------------------
# 8. graph capture


@gpu
def test_graph_capture_replays_draw_new_masks(ext):
    """Forward + backward of hip_attention_core with dropout in one
    torch.cuda.graph: every replay reads the advanced offset, so replays
    differ, and each meets the bound against the reference built from
    its own rng_state."""
    from alphafold2_amd.ops.hip_autograd import hip_attention_core
    g = _gen(14)
    B, h, Lq, Lk, r, p = 2, 2, 130, 72, 2, 0.25
    q, k, v = (_randn(B, h, Lq, 64, gen=g), _randn(B, h, Lk, 64, gen=g),
               _randn(B, h, Lk, 64, gen=g))
    bias = _randn(B // r, h, Lq, Lk, gen=g)
    dout = _randn(B, h, Lq, 64, gen=g)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v, bias)]

    def step():
        out, st = hip_attention_core(leaves[0], leaves[1], leaves[2],
                                     bias=leaves[3], bias_repeat=r,
                                     dropout_p=p, return_rng_state=True)
        grads = torch.autograd.grad(out, leaves, dout)
        return [out, *grads], st

    torch.cuda.manual_seed(31)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_res, static_st = step()

    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append(([t.detach().clone() for t in static_res],
                        static_st.clone()))
    (res1, st1), (res2, st2) = replays
    assert st1[0].item() == 31 and st2[0].item() == 31
    assert st2[1].item() > st1[1].item(), (st1.tolist(), st2.tolist())
    assert not torch.equal(res1[0], res2[0]), "replays must differ"
    for i, (res, st) in enumerate(replays):
        bd = _Bound(f"drop_graph_replay{i}")
        bd.check_all(NAMES, res,
                     _drop_fn(ext, st, (B, h, Lq, Lk), p, None, 0.125, r),
                     [q, k, v, bias], dout)
        bd.done()
