"""distbucket.hip and pairrep.hip against float64, over every dtype and
the block / chunk geometries of their launchers.

dist_buckets returns integers: a pair may differ from the float64 buckets
only if its float64 distance lies within the fp32 error of the kernel's
arithmetic (three subtractions, three squares, a sum and a sqrt:
8 * 2**-24 relative) of a boundary.  pairrep_fwd is one fp32 sum of three
terms and one output rounding: bit-exact on integer inputs,
T * |ref| + 1e-6 on random ones.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10,
       torch.float32: 1e-5}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


@pytest.fixture(scope="module")
def ext():
    from alphafold2_amd.ops.dispatch import _load_ext
    e = _load_ext()
    assert e is not None, "extension must load on GPU box"
    return e


# ---------------------------------------------------------------------------
# dist_buckets


def _dist64(coords):
    c = coords.double()
    return (c[:, :, None, :] - c[:, None, :, :]).pow(2).sum(-1).sqrt()


# (3, 131, 3): 51483 pairs, 202 blocks of 256 with a short last one and
# n dividing neither the block nor the wave; (1, 1, 3): a single pair
@pytest.mark.parametrize("nbounds", [36, 1])
@pytest.mark.parametrize("b,n", [(3, 131), (1, 1)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dist_buckets_random(ext, dtype, b, n, nbounds):
    g = torch.Generator(device=DEV).manual_seed(0)
    coords = (6 * torch.randn(b, n, 3, device=DEV, generator=g)).to(dtype)
    bounds = torch.linspace(2, 20, 37, device=DEV)[:-1] if nbounds == 36 \
        else torch.tensor([8.0], device=DEV)
    out = ext.dist_buckets(coords, bounds)
    d = _dist64(coords)
    ref = torch.bucketize(d, bounds.double())
    assert out.dtype == torch.long and out.shape == ref.shape
    assert out.min().item() >= 0 and out.max().item() <= nbounds
    exempt = ((d[..., None] - bounds.double()).abs()
              <= 8 * 2.0 ** -24 * d[..., None]).any(-1)
    share = exempt.double().mean().item()
    assert share <= 1e-3, f"exempt share {share}"
    wrong = (out != ref) & ~exempt
    assert not wrong.any(), f"{int(wrong.sum())} pairs off a boundary differ"
    # the diagonal is distance 0, below every boundary
    assert (torch.diagonal(out, dim1=1, dim2=2) == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_dist_buckets_exact_ties(ext, dtype):
    """Integer lattice coordinates: squared distances are exact integers
    in fp32, about 6 % of the pairs sit exactly on an integer boundary,
    and sqrt of a perfect square is exact: no pair is exempt."""
    g = torch.Generator(device=DEV).manual_seed(1)
    coords = torch.randint(-6, 7, (2, 40, 3), device=DEV, generator=g) \
        .to(dtype)
    bounds = torch.arange(1, 16, device=DEV, dtype=torch.float32)
    d = _dist64(coords)
    ties = (d[..., None] == bounds.double()).any(-1).double().mean().item()
    assert ties > 0.02, ties
    out = ext.dist_buckets(coords, bounds)
    assert torch.equal(out, torch.bucketize(d, bounds.double()))


# ---------------------------------------------------------------------------
# pairrep_fwd

V = 5
# chunks = d / 8 eight-wide column chunks per row, 256 threads:
# (1, 1, 8):    1 chunk, 256 rows per step, a single row
# (2, 7, 8):    the same with 249 idle threads
# (2, 7, 384):  48 chunks do not divide 256: 5 rows per step, 16 threads
#               repeat a row; 7 rows = one full step and a short one
# (1, 3, 2048): 256 chunks, one row per step
# (2, 33, 264): 33 chunks, 7 rows per step, 33 % 7 != 0
PAIRREP_SHAPES = [(1, 1, 8), (2, 7, 8), (2, 7, 384), (1, 3, 2048),
                  (2, 33, 264)]


def _rels(b, n, gen):
    """Index tensors that together use row 0 and row V - 1 of the table."""
    rel = torch.randint(0, V, (b, n, n), device=DEV, generator=gen)
    if rel.numel() == 1:
        return [torch.zeros_like(rel), torch.full_like(rel, V - 1)]
    rel.view(-1)[0] = 0
    rel.view(-1)[-1] = V - 1
    return [rel]


def _pairrep64(left, right, emb, rel):
    return left.double()[:, :, None, :] + right.double()[:, None, :, :] \
        + emb.double()[rel]


@pytest.mark.parametrize("b,n,d", PAIRREP_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pairrep_fwd(ext, dtype, b, n, d):
    gen = torch.Generator(device=DEV).manual_seed(2)
    ints = lambda *s: torch.randint(-8, 9, s, device=DEV,
                                    generator=gen).to(dtype)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen).to(dtype)
    for rel in _rels(b, n, gen):
        left, right, emb = ints(b, n, d), ints(b, n, d), ints(V, d)
        out = ext.pairrep_fwd(left, right, emb, rel)
        assert out.dtype == dtype and out.shape == (b, n, n, d)
        assert torch.equal(out, _pairrep64(left, right, emb, rel).to(dtype))

        left, right, emb = rnd(b, n, d), rnd(b, n, d), rnd(V, d)
        out = ext.pairrep_fwd(left, right, emb, rel)
        ref = _pairrep64(left, right, emb, rel)
        err = (out.double() - ref).abs()
        bad = ~(err <= TOL[dtype] * ref.abs() + 1e-6)
        assert not bad.any(), \
            f"{int(bad.sum())} elements off, max err {err.max().item():.3e}"


def test_pair_rep_autograd_float64(ext):
    """hip_pair_rep backward (row / column sums and an fp32 index_add,
    each rounded to bf16 once) against float64 autograd."""
    from alphafold2_amd.ops.hip_autograd import hip_pair_rep
    b, n, d = 2, 7, 384
    gen = torch.Generator(device=DEV).manual_seed(3)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen) \
        .to(torch.bfloat16)
    left, right, emb, dy = rnd(b, n, d), rnd(b, n, d), rnd(V, d), \
        rnd(b, n, n, d)
    (rel,) = _rels(b, n, gen)

    l1, r1, e1 = (t.clone().requires_grad_(True) for t in (left, right, emb))
    out = hip_pair_rep(l1, r1, e1, rel)
    out.backward(dy)
    l2, r2, e2 = (t.double().requires_grad_(True)
                  for t in (left, right, emb))
    ref = l2[:, :, None, :] + r2[:, None, :, :] + e2[rel]
    ref.backward(dy.double())
    # the same graph on |dy| gives each gradient's sum of absolute terms
    l3, r3, e3 = (t.double().requires_grad_(True)
                  for t in (left, right, emb))
    (l3[:, :, None, :] + r3[:, None, :, :] + e3[rel]) \
        .backward(dy.double().abs())

    err = (out.detach().double() - ref.detach()).abs()
    assert (err <= 2.0 ** -8 * ref.detach().abs() + 1e-6).all()
    for name, got, want, S in (("dleft", l1.grad, l2.grad, l3.grad),
                               ("dright", r1.grad, r2.grad, r3.grad),
                               ("demb", e1.grad, e2.grad, e3.grad)):
        assert got.dtype == torch.bfloat16 and got.shape == want.shape
        err = (got.double() - want).abs()
        bad = ~(err <= 2.0 ** -8 * want.abs() + 1e-5 * S + 1e-6)
        assert not bad.any(), \
            f"{name}: {int(bad.sum())} off, max err {err.max().item():.3e}"
