"""The fixed-order fold of (nb, C) fp32 partial rows (`ops/hip/colsum.h`).

`ext.colsum_fold(part, accumulate_into=None, v1=False)` runs the fold the
split-K weight gradient, the geglu / gate column sums, the pair-rep
backward and the fused dQ + dBias kernel finish with.  C % 4 == 0 takes
the 16-byte body (a tall block of 128 row lanes below 32768 columns, a
wide one of 16 row lanes from there on); any other C, and v1=True, takes
the scalar body.

Integer partials must fold exactly.  For random partials every fp32
summation order stays within nb * 2**-24 * sum|part| of the exact sum of
a column, which is the bound used here (the reference is float64).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'

# (nb, C):
# (1, 4)        one row, one quad
# (3, 20)       fewer rows than row lanes
# (64, 16), (65, 260), (256, 1028)   tall body, row tails
# (1030, 36)    tall body through its 8-deep unrolled loop (8 * 128 rows)
# (9, 32772)    wide body, fewer rows than its 16 row lanes, last block ragged
# (131, 32768)  wide body through its unrolled loop (8 * 16 rows) and tail
# (7, 10), (70, 33)   C % 4 != 0: the scalar body
CASES = [(1, 4), (3, 20), (64, 16), (65, 260), (256, 1028), (1030, 36),
         (9, 32772), (131, 32768), (7, 10), (70, 33)]


@pytest.fixture(scope="module")
def ext():
    from alphafold2_amd.ops.dispatch import _load_ext
    e = _load_ext()
    assert e is not None, "extension must load on GPU box"
    return e


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


@pytest.mark.parametrize("v1", [False, True])
@pytest.mark.parametrize("nb,C", CASES)
def test_fold_integers_exact(ext, nb, C, v1):
    part = torch.randint(-8, 9, (nb, C), device=DEV, generator=_gen(1)) \
        .float()
    out = ext.colsum_fold(part, v1=v1)
    assert out.dtype == torch.float32 and out.shape == (C,)
    assert torch.equal(out, part.double().sum(0).float())


@pytest.mark.parametrize("v1", [False, True])
@pytest.mark.parametrize("nb,C", CASES)
def test_fold_random_bound_and_determinism(ext, nb, C, v1):
    part = torch.randn(nb, C, device=DEV, generator=_gen(2))
    out = ext.colsum_fold(part, v1=v1)
    ref = part.double().sum(0)
    bound = nb * 2.0 ** -24 * part.double().abs().sum(0)
    err = (out.double() - ref).abs()
    print(f"EVIDENCE fold[{nb}x{C},v1={int(v1)}] max err/bound "
          f"{(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert (err <= bound).all(), f"max err {err.max().item():.3e}"
    assert torch.equal(out, ext.colsum_fold(part, v1=v1)), \
        "two runs differ"


@pytest.mark.parametrize("v1", [False, True])
@pytest.mark.parametrize("nb,C", CASES)
def test_fold_accumulate_integers(ext, nb, C, v1):
    g = _gen(3)
    part = torch.randint(-8, 9, (nb, C), device=DEV, generator=g).float()
    base = torch.randint(-100, 101, (C,), device=DEV, generator=g).float()
    out = base.clone()
    ret = ext.colsum_fold(part, accumulate_into=out, v1=v1)
    assert ret.data_ptr() == out.data_ptr()
    assert torch.equal(out, ext.colsum_fold(part, v1=v1) + base)
    assert torch.equal(out, (part.double().sum(0) + base.double()).float())


def test_fold_unaligned_rows_take_the_scalar_body(ext):
    """A part whose rows start 4 bytes off a 16-byte boundary (a view
    into a larger buffer) folds exactly: the launcher sees the address."""
    nb, C = 33, 64
    buf = torch.randint(-8, 9, (nb * C + 1,), device=DEV,
                        generator=_gen(4)).float()
    part = buf[1:].view(nb, C)
    assert part.data_ptr() % 16 != 0 and part.is_contiguous()
    assert torch.equal(ext.colsum_fold(part), part.double().sum(0).float())
