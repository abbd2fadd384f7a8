"""Pair-representation backward from one read of dy (`ext.pairrep_bwd`).

dleft[b,i] = sum_j dy[b,i,j], dright[b,j] = sum_i dy[b,i,j] and
demb[v] = sum of dy[b,i,j] over rel[b,i,j] == v, each an fp32 sum rounded
once to dy's dtype.  A block owns a 32 x 32 tile of (i, j); partial sums
per tile are folded in a fixed order, so the result is the same on every
run.  References are float64 from the rounded inputs; the bound per
gradient is that of test_pair_rep_autograd_float64,

    err <= 2**-8 * |ref| + 1e-5 * S + 1e-6,

with S the same sum over |dy|.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
V = 65                    # rows of the flagship's relative-position table
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
# (b, n, d) the kernel covers:
# (1, 1, 8)      a single element, 4 of 64 threads active
# (2, 7, 8), (2, 7, 384)   one ragged tile; 192 threads
# (2, 33, 264)   2 x 2 tiles with a last tile of one row / column; 132 of
#                192 threads active; the table takes 68,640 B of LDS
# (2, 70, 64)    3 x 3 tiles, ragged last tile
# (1, 33, 256)   the flagship's d: a 66,560 B table (LDS beyond 64 KiB)
SHAPES = [(1, 1, 8), (2, 7, 8), (2, 7, 384), (2, 33, 264), (2, 70, 64),
          (1, 33, 256)]
# outside the gate: d above 1024 (and a table beyond a block's LDS)
FALLBACK_SHAPE = (1, 3, 2048)
NAMES = ['dleft', 'dright', 'demb']


@pytest.fixture(scope="module")
def ext():
    from alphafold2_amd.ops.dispatch import _load_ext
    e = _load_ext()
    assert e is not None, "extension must load on GPU box"
    return e


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _rels(b, n, gen, rows=V):
    """Index tensors that together use row 0 and row rows - 1 of the table
    (as tests/test_distbucket_pairrep.py makes them), one that sends every
    element to a single row, and the model's clamp(i - j) form."""
    rel = torch.randint(0, rows, (b, n, n), device=DEV, generator=gen)
    if rel.numel() == 1:
        rels = [torch.zeros_like(rel), torch.full_like(rel, rows - 1)]
    else:
        rel.view(-1)[0] = 0
        rel.view(-1)[-1] = rows - 1
        rels = [rel]
    rels.append(torch.full_like(rel, rows // 2))
    half = (rows - 1) // 2
    i = torch.arange(n, device=DEV)
    rels.append(((i[:, None] - i[None, :]).clamp(-half, half) + half)
                .expand(b, n, n).contiguous())
    return rels


def _ref64(dy, rel, rows=V):
    """[dleft, dright, demb] in float64."""
    d = dy.shape[-1]
    x = dy.double()
    demb = torch.zeros(rows, d, device=DEV, dtype=torch.float64)
    demb.index_add_(0, rel.reshape(-1), x.reshape(-1, d))
    return [x.sum(2), x.sum(1), demb]


def _check_bound(case, got, dy, rel, rows=V):
    ref = _ref64(dy, rel, rows)
    S = _ref64(dy.double().abs(), rel, rows)
    for name, g, want, s in zip(NAMES, got, ref, S):
        assert g.dtype == dy.dtype and g.shape == want.shape, name
        err = (g.double() - want).abs()
        bound = 2.0 ** -8 * want.abs() + 1e-5 * s + 1e-6
        print(f"EVIDENCE {case} {name} max err {err.max().item():.3e} "
              f"max err/bound {(err / bound).max().item():.3e}")
        bad = ~(err <= bound)
        assert not bad.any(), \
            f"{case} {name}: {int(bad.sum())} off, max err " \
            f"{err.max().item():.3e}"


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pairrep_bwd(ext, dtype, b, n, d):
    gen = _gen(5)
    for ri, rel in enumerate(_rels(b, n, gen)):
        case = f"pairrep_bwd[{b},{n},{d},{str(dtype)[6:]},rel{ri}]"
        dy = torch.randint(-8, 9, (b, n, n, d), device=DEV,
                           generator=gen).to(dtype)
        assert ext.pairrep_bwd_covers(dy, V), case
        got = ext.pairrep_bwd(dy, rel, V)
        for name, g, want in zip(NAMES, got, _ref64(dy, rel)):
            assert torch.equal(g, want.to(dtype)), f"{case} {name} (ints)"

        dy = torch.randn(b, n, n, d, device=DEV, generator=gen).to(dtype)
        got = ext.pairrep_bwd(dy, rel, V)
        _check_bound(case, got, dy, rel)
        again = ext.pairrep_bwd(dy, rel, V)
        for name, g, a in zip(NAMES, got, again):
            assert torch.equal(g, a), f"{case} {name}: two runs differ"


def test_pairrep_bwd_small_table(ext):
    """A table of five rows (the V of tests/test_distbucket_pairrep.py)."""
    gen = _gen(6)
    b, n, d, rows = 2, 7, 8, 5
    for rel in _rels(b, n, gen, rows):
        dy = torch.randn(b, n, n, d, device=DEV, generator=gen) \
            .to(torch.bfloat16)
        _check_bound("pairrep_bwd[V=5]", ext.pairrep_bwd(dy, rel, rows), dy,
                     rel, rows)


def test_pairrep_bwd_composition_path(ext):
    """The library composition that AF2AMD_PAIRREP_BWD_V1=1 selects, called
    directly on a shape the kernel covers: the same bound."""
    from alphafold2_amd.ops.hip_autograd import _pairrep_bwd_composed
    gen = _gen(7)
    b, n, d = 2, 33, 264
    dy = torch.randn(b, n, n, d, device=DEV, generator=gen) \
        .to(torch.bfloat16)
    for rel in _rels(b, n, gen):
        _check_bound("pairrep_bwd_v1", _pairrep_bwd_composed(dy, rel, V), dy,
                     rel)


def test_pairrep_bwd_fallback_outside_gate(ext):
    """d = 2048 is outside the gate (d <= 1024; its 65-row table would need
    532 KB of LDS): hip_pair_rep's backward takes the composition and
    keeps the bound; the kernel itself refuses the shape."""
    from alphafold2_amd.ops.hip_autograd import hip_pair_rep
    b, n, d = FALLBACK_SHAPE
    gen = _gen(8)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen) \
        .to(torch.bfloat16)
    left, right, emb, dy = rnd(b, n, d), rnd(b, n, d), rnd(V, d), \
        rnd(b, n, n, d)
    assert not ext.pairrep_bwd_covers(dy, V)
    with pytest.raises(RuntimeError, match="not covered"):
        ext.pairrep_bwd(dy, torch.zeros(b, n, n, device=DEV,
                                        dtype=torch.long), V)
    for rel in _rels(b, n, gen):
        leaves = [t.clone().requires_grad_(True) for t in (left, right, emb)]
        hip_pair_rep(*leaves, rel).backward(dy)
        _check_bound("pairrep_bwd_fallback", [t.grad for t in leaves], dy,
                     rel)


def test_pairrep_autograd_takes_the_kernel(ext):
    """hip_pair_rep's backward on a covered shape gives bit for bit what
    ext.pairrep_bwd gives (the wrapper passes dy and rel through)."""
    from alphafold2_amd.ops.hip_autograd import hip_pair_rep
    b, n, d = 2, 33, 264
    gen = _gen(9)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen) \
        .to(torch.bfloat16)
    left, right, emb, dy = rnd(b, n, d), rnd(b, n, d), rnd(V, d), \
        rnd(b, n, n, d)
    rel = _rels(b, n, gen)[0]
    leaves = [t.clone().requires_grad_(True) for t in (left, right, emb)]
    hip_pair_rep(*leaves, rel).backward(dy)
    for name, t, want in zip(NAMES, leaves, ext.pairrep_bwd(dy, rel, V)):
        assert torch.equal(t.grad, want), name
