"""dBias out of the dQ-from-dS kernel (`attn_bwd_dq_dbias_kernel`).

On the stored-dS path `attn_bwd` forms dQ and the dBias sum in one kernel:
a block owns a q tile, a (repeat group, head) and a chunk of consecutive
batch entries of that group, writes dQ per entry as the dQ-only kernel
does and keeps the fp32 sum of the dS it staged; with more than one chunk
per group the chunks' partial sums are folded in order.  The trailing
argument `dq_entries_per_block` gives the entries per block (None:
automatic, 0: the two kernels, dQ then the sum).

dQ must not depend on the chunking, the slicing or the path, bit for bit.
dBias is held to the bound of tests/test_attention_ds_path.py, whose
helpers are copied here: one plain-torch reference evaluated in float64
and in bf16, and

    E_kernel <= 2 * E_floor + 2**-8 * max|ref64|
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16 = torch.bfloat16
H = 2
ONE_SLICE = 1 << 30      # far above every scratch these shapes need
# Lq x Lk: one partial q tile and two kv tiles; three q tiles and five kv
# tiles (a kv tile count beyond what automatic fuses), both ragged
SHAPES = [(40, 72), (130, 264)]


@pytest.fixture(scope="module")
def ext():
    from alphafold2_amd.ops.dispatch import _load_ext
    e = _load_ext()
    assert e is not None, "extension must load on GPU box"
    return e


# ---------------------------------------------------------------------------
# reference and bound (conventions of tests/test_attention_ds_path.py)


def ref_attention(q, k, v, bias, key_mask, scale, bias_repeat=1,
                  tie_dim=None):
    """softmax(q k^T * scale + repeat_interleave(bias) + key mask) v in the
    dtype of its inputs.  A row whose keys are all masked gives 0; tie_dim
    replaces each query by its group mean."""
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


def _inputs(B, r, Lq, Lk, seed=7):
    """The mask has a random part, one whole masked kv tile (entry 0,
    keys 0..63) and one fully masked batch entry (the last)."""
    g = _gen(seed)
    c = dict(q=_randn(B, H, Lq, 64, gen=g), k=_randn(B, H, Lk, 64, gen=g),
             v=_randn(B, H, Lk, 64, gen=g),
             bias=_randn(B // r, H, Lq, Lk, gen=g),
             dout=_randn(B, H, Lq, 64, gen=g), r=r)
    m = torch.rand(B, Lk, device=DEV, generator=g) > 0.2
    m[:, Lk - 1] = True
    m[0, :64] = False
    m[B - 1, :] = False
    c['mask'] = m
    return c


_CASES = {}
_REFS = {}
_TWO = {}


def _case(B, r, Lq, Lk):
    """Inputs, their float64 / bf16 references (scale 0.125) and the
    result of the two-kernel path, computed once and shared."""
    key = (B, r, Lq, Lk)
    if key not in _CASES:
        c = _inputs(B, r, Lq, Lk)
        fn = lambda q, k, v, b: ref_attention(q, k, v, b, c['mask'], 0.125, r)
        leaves = [c['q'], c['k'], c['v'], c['bias']]
        _CASES[key] = c
        _REFS[key] = (_ref_grads(fn, leaves, c['dout'], torch.float64),
                      _ref_grads(fn, leaves, c['dout'], BF16))
    return _CASES[key], _REFS[key]


def _run(ext, c, ds_bytes, epb, q=None, q_repeat=1):
    """[out, dq, dk, dv, dbias] of attn_fwd + attn_bwd with need_dbias."""
    q = c['q'] if q is None else q
    m8 = c['mask'].to(torch.uint8)
    out, lse = ext.attn_fwd(q, c['k'], c['v'], c['bias'], m8, c['r'], 0.125,
                            q_repeat=q_repeat)[:2]
    rets = ext.attn_bwd(c['dout'], q, c['k'], c['v'], out, lse, c['bias'],
                        m8, c['r'], 0.125, True, q_repeat=q_repeat,
                        ds_scratch_bytes=ds_bytes, dq_entries_per_block=epb)
    assert rets[3].dtype == torch.float32
    assert rets[3].shape == c['bias'].shape
    return [out, *rets]


def _two_kernels(ext, B, r, Lq, Lk):
    key = (B, r, Lq, Lk)
    if key not in _TWO:
        _TWO[key] = _run(ext, _case(*key)[0], ONE_SLICE, 0)
    return _TWO[key]


def _check(case, kern, refs, names=NAMES):
    r64, r16 = refs
    bd = _Bound(case)
    for name in names:
        i = NAMES.index(name)
        bd.check(name, kern[i], r64[i], r16[i])
    bd.done()


# ---------------------------------------------------------------------------
# 1. chunks that do not divide the group, one chunk per group, automatic


@pytest.mark.parametrize("B,r,epb", [(6, 3, 1), (6, 3, 2), (6, 3, 3),
                                     (6, 3, None), (16, 8, 3)])
@pytest.mark.parametrize("Lq,Lk", SHAPES)
def test_dq_dbias_chunks(ext, Lq, Lk, B, r, epb):
    """r = 3: one entry per block (three chunks), two (a full and a
    partial chunk), three (one chunk, dbias stored by the block itself);
    r = 8 with three entries per block (3 + 3 + 2).  None is the launcher's
    own choice (at Lk = 264 that is the two kernels)."""
    c, refs = _case(B, r, Lq, Lk)
    two = _two_kernels(ext, B, r, Lq, Lk)
    kern = _run(ext, c, ONE_SLICE, epb)
    for i in (0, 1, 2, 3):
        assert torch.equal(kern[i], two[i]), \
            f"{NAMES[i]} differs from the two-kernel path"
    for name, t in zip(NAMES[:4], kern[:4]):
        assert (t[-1] == 0).all(), f"{name} of the masked entry != 0"
    _check(f"dq_dbias[{Lq}x{Lk},B={B},r={r},epb={epb}]", kern, refs)
    again = _run(ext, c, ONE_SLICE, epb)
    assert torch.equal(again[4], kern[4]), "dbias differs between launches"
    assert torch.equal(again[1], kern[1]), "dq differs between launches"


def test_two_kernel_path_in_bound(ext):
    """The path that `dq_entries_per_block=0` (and AF2AMD_DQ_DBIAS_FUSED=0)
    selects is the one the other tests compare dq against."""
    for Lq, Lk in SHAPES:
        _, refs = _case(6, 3, Lq, Lk)
        _check(f"dq_dbias_two[{Lq}x{Lk}]", _two_kernels(ext, 6, 3, Lq, Lk),
               refs)


# ---------------------------------------------------------------------------
# 2. a slice boundary and a chunk boundary inside one group


@pytest.mark.parametrize("Lq,Lk", SHAPES)
def test_dq_dbias_slices_and_chunks(ext, Lq, Lk):
    """B = 6, r = 3, a cap of 4 entries, 2 entries per block.  Slice
    [0, 4) holds group 0 (chunks {0, 1}, {2}) and entry 3 of group 1 (a
    chunk of one and an empty one, which must store zeros); slice [4, 6)
    continues group 1 with one chunk and adds to what the first stored."""
    c, refs = _case(6, 3, Lq, Lk)
    two = _two_kernels(ext, 6, 3, Lq, Lk)
    cap = 4 * _entry_bytes(Lq, Lk) + _entry_bytes(Lq, Lk) // 2
    cut = _run(ext, c, cap, 2)
    for i in (1, 2, 3):
        assert torch.equal(cut[i], two[i]), NAMES[i]
    _check(f"dq_dbias_slices[{Lq}x{Lk}]", cut, refs)
    # one entry per slice and per block: every group is continued twice
    one = _run(ext, c, _entry_bytes(Lq, Lk), 1)
    assert torch.equal(one[1], two[1]), "dq"
    _check(f"dq_dbias_slices1[{Lq}x{Lk}]", one, refs)
    # a cap of 5 entries with one entry per block: slice [0, 5) ends
    # inside group 1 with an empty third chunk, slice [5, 6) is one block
    cap5 = 5 * _entry_bytes(Lq, Lk)
    five = _run(ext, c, cap5, 1)
    assert torch.equal(five[1], two[1]), "dq"
    _check(f"dq_dbias_slices5[{Lq}x{Lk}]", five, refs)


def test_dq_dbias_continued_group_is_folded(ext):
    """B = 8, r = 4, a cap of 6 entries, one entry per block: slice [6, 8)
    continues group 1 with two chunks, so the fold adds to what slice
    [0, 6) left there."""
    Lq, Lk = 40, 72
    c, refs = _case(8, 4, Lq, Lk)
    two = _two_kernels(ext, 8, 4, Lq, Lk)
    cut = _run(ext, c, 6 * _entry_bytes(Lq, Lk), 1)
    for i in (1, 2, 3):
        assert torch.equal(cut[i], two[i]), NAMES[i]
    _check("dq_dbias_continued[40x72]", cut, refs)


# ---------------------------------------------------------------------------
# 3. neither the scratch nor the partial sums are initialised


@pytest.mark.parametrize("Lq,Lk", SHAPES)
def test_dq_dbias_poisoned_allocator(ext, Lq, Lk):
    """The caching allocator hands the scratch and the partials blocks that
    held NaNs: every element a consumer reads must have been written."""
    c, refs = _case(6, 3, Lq, Lk)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    part_elems = 3 * 2 * H * Lq * Lk * 2     # fp32 partials, in bf16 units
    poison = [torch.full((n,), float('nan'), device=DEV, dtype=BF16)
              for n in [6 * _entry_bytes(Lq, Lk) // 2, part_elems]
              + 4 * [1 << 19]]
    del poison
    kern = _run(ext, c, ONE_SLICE, 1)
    for name, t in zip(NAMES, kern):
        assert torch.isfinite(t).all(), f"{name} not finite"
    _check(f"dq_dbias_poison[{Lq}x{Lk}]", kern, refs)


# ---------------------------------------------------------------------------
# 4. tied query


def test_dq_dbias_tied_query_with_bias(ext):
    """B = 12, tie_dim = 6, bias_repeat = 4, two entries per block: one dQ
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
    kern = _run(ext, c, ONE_SLICE, 2, q=qm, q_repeat=tie)
    two = _run(ext, c, ONE_SLICE, 0, q=qm, q_repeat=tie)
    assert torch.equal(kern[1], two[1]), "dq differs from the two kernels"
    dq = kern[1].reshape(B // tie, tie, H, n, 64) \
        .sum(dim=1, keepdim=True).div_(tie) \
        .expand(B // tie, tie, H, n, 64).reshape(B, H, n, 64)
    kern[1] = dq
    fn = lambda q, k, v, b: ref_attention(q, k, v, b, mask, 0.125, r, tie)
    leaves = [q, k, v, bias]
    _check("dq_dbias_tied[B=12,tie=6,r=4]", kern,
           (_ref_grads(fn, leaves, dout, torch.float64),
            _ref_grads(fn, leaves, dout, BF16)))


# ---------------------------------------------------------------------------
# 5. graph capture


def test_dq_dbias_graph_capture(ext):
    """Forward and backward of ops.attention_core_packed with bias and
    r = 4 in one torch.cuda.graph (the launcher's own entries per block:
    partial sums and their fold are allocated and launched inside the
    capture): the replay gives what the uncaptured step gave."""
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


def test_dq_entries_per_block_negative_is_refused(ext):
    c, _ = _case(6, 3, 40, 72)
    with pytest.raises(RuntimeError, match="dq_entries_per_block"):
        _run(ext, c, ONE_SLICE, -1)
