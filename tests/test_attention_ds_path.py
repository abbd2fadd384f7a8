"""Attention backward through the stored-dS path.

With a bias gradient wanted, `attn_bwd` lets the dK/dV kernel store its
bf16 dS tile to a scratch ([batch*head][kv][q], whole 64x64 tiles),
forms dQ = scale * dS K from that scratch and sums dS over each
bias_repeat group into dbias with one writer per element
(docs/KERNELS.md, "Attention backward: stored dS").  `ds_scratch_bytes`
caps the scratch: above the cap the three kernels run over consecutive
batch slices; 0 selects the float-atomic path.

Reference and bound are those of tests/test_attention_paths.py: one
plain-torch reference evaluated in float64 and in bf16, and

    E_kernel <= 2 * E_floor + 2**-8 * max|ref64|

Each check prints `EVIDENCE case output E_kernel E_floor ratio bound`
before it asserts; docs/EVIDENCE.md holds the measured table.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16 = torch.bfloat16
H = 2
ONE_SLICE = 1 << 30      # far above every scratch these shapes need


@pytest.fixture(scope="module")
def ext():
    from alphafold2_amd.ops.dispatch import _load_ext
    e = _load_ext()
    assert e is not None, "extension must load on GPU box"
    return e


# ---------------------------------------------------------------------------
# reference and bound (conventions of tests/test_attention_paths.py)


def ref_attention(q, k, v, bias, key_mask, scale, bias_repeat=1,
                  tie_dim=None, keep=None, rescale=1.0):
    """softmax(q k^T * scale + repeat_interleave(bias) + key mask), then
    dropout by the explicit `keep` mask and `rescale`, times v, in the
    dtype of its inputs.  A row whose keys are all masked gives 0;
    tie_dim replaces each query by its group mean."""
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

    def done(self):
        assert not self.failed, f"{self.case}: " + "; ".join(self.failed)


NAMES = ['out', 'dq', 'dk', 'dv', 'dbias']


def _randn(*shape, gen=None):
    return torch.randn(*shape, device=DEV, generator=gen).to(BF16)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _entry_bytes(Lq, Lk, h=H):
    """Scratch bytes of one batch entry: h bf16 planes of whole tiles."""
    pad = lambda n: (n + 63) // 64 * 64
    return h * pad(Lq) * pad(Lk) * 2


def _inputs(B, r, Lq, Lk, use_mask, seed=7):
    """The mask has a random part, one whole masked kv tile (entry 0,
    keys 0..63) and one fully masked batch entry (the last)."""
    g = _gen(seed)
    c = dict(q=_randn(B, H, Lq, 64, gen=g), k=_randn(B, H, Lk, 64, gen=g),
             v=_randn(B, H, Lk, 64, gen=g),
             bias=_randn(B // r, H, Lq, Lk, gen=g),
             dout=_randn(B, H, Lq, 64, gen=g), r=r, mask=None)
    if use_mask:
        m = torch.rand(B, Lk, device=DEV, generator=g) > 0.2
        m[:, Lk - 1] = True
        m[0, :64] = False
        m[B - 1, :] = False
        c['mask'] = m
    return c


_CASES = {}
_REFS = {}


def _case(B, r, Lq, Lk, use_mask):
    """Inputs and their float64 / bf16 references (scale 0.125), computed
    once and shared by the tests that use the same case."""
    key = (B, r, Lq, Lk, use_mask)
    if key not in _CASES:
        c = _inputs(B, r, Lq, Lk, use_mask)
        fn = lambda q, k, v, b: ref_attention(q, k, v, b, c['mask'], 0.125, r)
        leaves = [c['q'], c['k'], c['v'], c['bias']]
        _CASES[key] = c
        _REFS[key] = (_ref_grads(fn, leaves, c['dout'], torch.float64),
                      _ref_grads(fn, leaves, c['dout'], BF16))
    return _CASES[key], _REFS[key]


def _run(ext, c, ds_bytes, scale=0.125, q=None, q_repeat=1, **kw):
    """[out, dq, dk, dv, dbias] of attn_fwd + attn_bwd with need_dbias."""
    q = c['q'] if q is None else q
    m8 = c['mask'].to(torch.uint8) if c['mask'] is not None else None
    fkw = dict(q_repeat=q_repeat)
    if 'dropout_p' in kw:
        fkw.update(dropout_p=kw['dropout_p'], rng_state=kw['rng_state'])
    out, lse = ext.attn_fwd(q, c['k'], c['v'], c['bias'], m8, c['r'], scale,
                            **fkw)[:2]
    rets = ext.attn_bwd(c['dout'], q, c['k'], c['v'], out, lse, c['bias'],
                        m8, c['r'], scale, True, q_repeat=q_repeat,
                        ds_scratch_bytes=ds_bytes, **kw)
    assert rets[3].dtype == torch.float32
    assert rets[3].shape == c['bias'].shape
    return [out, *rets]


def _check(case, kern, refs, names=NAMES):
    r64, r16 = refs
    bd = _Bound(case)
    for name in names:
        i = NAMES.index(name)
        bd.check(name, kern[i], r64[i], r16[i])
    bd.done()


# ---------------------------------------------------------------------------
# 1. partial tiles, more than four kv tiles, repeat groups, masks


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("r", [1, 3, 8])
@pytest.mark.parametrize("Lq,Lk", [(40, 72), (130, 264), (72, 330)])
def test_ds_path_parity(ext, Lq, Lk, r, use_mask):
    c, refs = _case(2 * r, r, Lq, Lk, use_mask)
    kern = _run(ext, c, ONE_SLICE)
    if use_mask:
        for name, t in zip(NAMES[:4], kern[:4]):
            assert (t[-1] == 0).all(), f"{name} of the masked entry != 0"
        if r == 1:  # a repeat group of one: its masked keys get no dbias
            assert (kern[4][0, :, :, :64] == 0).all(), "dbias at masked keys"
            assert (kern[4][-1] == 0).all(), "dbias of the masked entry"
    _check(f"ds[{Lq}x{Lk},r={r},mask={int(use_mask)}]", kern, refs)


# ---------------------------------------------------------------------------
# 2. slicing


@pytest.mark.parametrize("entries", [4, 1])
def test_ds_path_slices(ext, entries):
    """B = 6, r = 3.  A cap of 4 entries gives slices [0, 4) and [4, 6):
    the first ends inside repeat group 1, the second is partial and adds
    to that group.  A cap of 1 entry gives six slices.  dq, dk and dv do
    not depend on the slicing; dbias is summed in another order."""
    Lq, Lk = 130, 264
    c, refs = _case(6, 3, Lq, Lk, True)
    one = _run(ext, c, ONE_SLICE)
    # a cap that is no multiple of the entry size rounds down
    cap = entries * _entry_bytes(Lq, Lk) + _entry_bytes(Lq, Lk) // 2
    cut = _run(ext, c, cap)
    for i in (1, 2, 3):
        assert torch.equal(cut[i], one[i]), NAMES[i]
    _check(f"ds_slices[entries={entries}]", cut, refs)


# ---------------------------------------------------------------------------
# 3. the scratch is not initialised


@pytest.mark.parametrize("Lq,Lk", [(40, 72), (130, 264)])
def test_ds_path_poisoned_scratch(ext, Lq, Lk):
    """The caching allocator hands the scratch a block that held NaNs:
    every element a consumer reads must have been written."""
    c, refs = _case(6, 3, Lq, Lk, True)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    # a block of the scratch's size, and (a scratch under 1 MiB comes out
    # of the allocator's 2 MiB small-block segments, behind the call's
    # other small tensors) two such segments
    poison = [torch.full((n,), float('nan'), device=DEV, dtype=BF16)
              for n in [6 * _entry_bytes(Lq, Lk) // 2] + 4 * [1 << 19]]
    del poison
    kern = _run(ext, c, ONE_SLICE)
    for name, t in zip(NAMES, kern):
        assert torch.isfinite(t).all(), f"{name} not finite"
    _check(f"ds_poison[{Lq}x{Lk}]", kern, refs)


# ---------------------------------------------------------------------------
# 4. determinism


def test_ds_path_deterministic(ext):
    c, _ = _case(16, 8, 130, 264, False)
    a = _run(ext, c, ONE_SLICE)
    b = _run(ext, c, ONE_SLICE)
    assert torch.equal(a[1], b[1]), "dq differs between launches"
    assert torch.equal(a[4], b[4]), "dbias differs between launches"


# ---------------------------------------------------------------------------
# 5. tied query


def test_ds_path_tied_query_with_bias(ext):
    """B = 12, tie_dim = 6, bias_repeat = 4 (the case of
    test_tied_query_with_bias_parity): the new dQ kernel writes one dQ
    per batch entry, folded over the tie group as the autograd function
    folds it."""
    g = _gen(50)
    B, n, tie, r = 12, 72, 6, 4
    q, k, v = (_randn(B, H, n, 64, gen=g) for _ in range(3))
    bias = _randn(B // r, H, n, n, gen=g)
    mask = torch.rand(B, n, device=DEV, generator=g) > 0.2
    mask[:, 0] = True
    dout = _randn(B, H, n, 64, gen=g)
    c = dict(q=q, k=k, v=v, bias=bias, dout=dout, r=r, mask=mask)
    qm = q.reshape(B // tie, tie, H, n, 64).mean(dim=1).contiguous()
    kern = _run(ext, c, ONE_SLICE, q=qm, q_repeat=tie)
    dq = kern[1].reshape(B // tie, tie, H, n, 64) \
        .sum(dim=1, keepdim=True).div_(tie) \
        .expand(B // tie, tie, H, n, 64).reshape(B, H, n, 64)
    kern[1] = dq
    fn = lambda q, k, v, b: ref_attention(q, k, v, b, mask, 0.125, r, tie)
    leaves = [q, k, v, bias]
    _check("ds_tied[B=12,tie=6,r=4]", kern,
           (_ref_grads(fn, leaves, dout, torch.float64),
            _ref_grads(fn, leaves, dout, BF16)))


# ---------------------------------------------------------------------------
# 6. dropout: the stored dS carries it, the dQ kernel knows nothing of it


def test_ds_path_dropout(ext):
    p, r, B, Lq, Lk = 0.25, 4, 8, 130, 72
    c = _inputs(B, r, Lq, Lk, True, seed=9)
    st = torch.tensor([1234, 12], dtype=torch.int64, device=DEV)
    kern = _run(ext, c, ONE_SLICE, dropout_p=p, rng_state=st)
    keep = ext.attn_dropout_mask(st, B, H, Lq, Lk, p)
    thresh = min(255, max(1, int(p * 256 + 0.5)))
    rescale = 256.0 / (256 - thresh)
    fn = lambda q, k, v, b: ref_attention(q, k, v, b, c['mask'], 0.125, r,
                                          None, keep, rescale)
    leaves = [c['q'], c['k'], c['v'], c['bias']]
    _check("ds_dropout[p=0.25,r=4]", kern,
           (_ref_grads(fn, leaves, c['dout'], torch.float64),
            _ref_grads(fn, leaves, c['dout'], BF16)))


# ---------------------------------------------------------------------------
# 7. a scale that is no power of two (applied to dQ after the product)


def test_ds_path_explicit_scale(ext):
    c = _inputs(6, 3, 130, 264, True, seed=11)
    kern = _run(ext, c, ONE_SLICE, scale=0.3)
    fn = lambda q, k, v, b: ref_attention(q, k, v, b, c['mask'], 0.3, 3)
    leaves = [c['q'], c['k'], c['v'], c['bias']]
    _check("ds_scale[0.3]", kern,
           (_ref_grads(fn, leaves, c['dout'], torch.float64),
            _ref_grads(fn, leaves, c['dout'], BF16)))


# ---------------------------------------------------------------------------
# 8. dq_out / dk_out / dv_out: slices of one packed buffer


def test_ds_path_out_views_write_discipline(ext):
    g = _gen(20)
    B, L, r = 4, 130, 2
    packed = _randn(B, L, 512, gen=g)
    bias = _randn(B // r, H, L, L, gen=g)
    mask_u8 = (torch.rand(B, L, device=DEV, generator=g) > 0.2) \
        .to(torch.uint8)
    mask_u8[:, 0] = 1
    dout = _randn(B, H, L, 64, gen=g)

    def view(t, off):
        return t.narrow(-1, off, 128).view(B, L, H, 64).permute(0, 2, 1, 3)

    q, k, v = view(packed, 0), view(packed, 128), view(packed, 256)
    out, lse = ext.attn_fwd(q, k, v, bias, mask_u8, r, 0.125)
    plain = ext.attn_bwd(dout, q, k, v, out, lse, bias, mask_u8, r, 0.125,
                         True, ds_scratch_bytes=ONE_SLICE)
    buf = torch.full_like(packed, float('nan'))
    got = ext.attn_bwd(dout, q, k, v, out, lse, bias, mask_u8, r, 0.125, True,
                       dq_out=view(buf, 0), dk_out=view(buf, 128),
                       dv_out=view(buf, 256), ds_scratch_bytes=ONE_SLICE)
    torch.cuda.synchronize()
    assert not torch.isnan(buf[..., :384]).any(), "q/k/v block not covered"
    assert torch.isnan(buf[..., 384:]).all(), "gate block was written"
    for i, name in enumerate(['dq', 'dk', 'dv']):
        assert torch.equal(view(buf, 128 * i), plain[i]), name
    assert torch.equal(got[3], plain[3]), "dbias"


# ---------------------------------------------------------------------------
# 9. the float-atomic path stays selectable


def test_legacy_atomic_path(ext):
    c, refs = _case(6, 3, 130, 264, True)
    _check("ds_legacy[130x264,r=3]", _run(ext, c, 0), refs)


# ---------------------------------------------------------------------------
# 10. graph capture


def test_ds_path_graph_capture(ext):
    """Forward and backward of ops.attention_core_packed with bias and
    r = 4 in one torch.cuda.graph: the replay gives what the uncaptured
    step gave (scratch and dbias are allocated inside the capture)."""
    from alphafold2_amd import ops
    g = _gen(60)
    B, L, r = 8, 72, 4
    packed = _randn(B, L, 384, gen=g).requires_grad_(True)
    bias = _randn(B // r, H, L, L, gen=g).requires_grad_(True)
    dout = _randn(B, H, L, 64, gen=g)

    def step():
        out = ops.attention_core_packed(packed, H, 128, bias=bias,
                                        bias_repeat=r)
        assert out is not None, "packed attention must take the HIP path"
        return [out, *torch.autograd.grad(out, [packed, bias], dout)]

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
        for name, a, b in zip(['out', 'dpacked', 'dbias'], static, want):
            assert torch.equal(a, b), name
