"""The streaming split-K weight-gradient kernel (ops/hip/wgrad.hip,
wgrad_stream_kernel) against float64: dW = dY^T X and the column sum of dY
from the same pass, directly and as `hip_linear`'s backward uses them.

The kernel's K step is 32 rows and its block tile 256 x 256 (KS, TM, TN
below); the shapes are chosen around those.

Exact-integer cases: operands are integers in [-2, 2] stored in bf16, so
every product and every fp32 partial sum is an exact integer whatever the
order of the slots and of the fold, and dW and the column sum must be
bit-equal to the float64 result cast to fp32.  The precondition (all sums of
absolute values < 2**24) is asserted on the reference alone.

Random-valued cases use the project's bound for an fp32 accumulation,
|got - ref64| <= 1e-5 * S with S the float64 sum of the absolute values of
the summed terms, and the autograd-level cases the bound of
test_linear_wgrad.py::test_hip_linear_autograd_float64,
2**-7 |ref| + 1e-5 S + 1e-6 (one rounding to bf16 on top).
"""
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF = torch.bfloat16
KS, TM, TN = 32, 256, 256


@pytest.fixture(scope="module")
def ext():
    from alphafold2_amd.ops.dispatch import _load_ext
    e = _load_ext()
    assert e is not None, "extension must load on GPU box"
    return e


def _ints(gen, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(BF).to(DEV)


def _randn(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF).to(DEV)


def _assert_bound(name, got, ref, bound):
    assert got.shape == ref.shape, name
    err = (got.double() - ref).abs()
    bad = err > bound
    assert not bad.any(), (
        f"{name}: {int(bad.sum())} of {bad.numel()} elements off, worst "
        f"err/bound {(err / bound).max().item():.3g}, max err "
        f"{err.max().item():.3e}")


# (1, 8, 8): the smallest legal problem
# (KS-1, 8, TN+8), (KS, TM+8, 8): one K step, short and full; N / M tile
#   tails of 8
# (KS+1, 40, 2*TN+8): one step plus a single-row second step (a second
#   slot); three column tiles
# (1000, 128, 128): 32 slots, K no multiple of KS, a partial tile
# (3000, TM+8, 2*TN+8): 2 x 3 tiles, so the XCD mapping sees more than
#   one tile per K slab
# (70001, 8, 256), (70001, 40, 136): the dispatch class; one tile, hence
#   the largest slot count (244 > 64 partial rows into the fold), the last
#   slot short and odd (17 rows)
EXACT_SHAPES = [(1, 8, 8), (KS - 1, 8, TN + 8), (KS, TM + 8, 8),
                (KS + 1, 40, 2 * TN + 8), (1000, 128, 128),
                (3000, TM + 8, 2 * TN + 8), (70001, 8, 256),
                (70001, 40, 136)]


@pytest.mark.parametrize("K,M,N", EXACT_SHAPES)
def test_stream_exact_integers(ext, K, M, N):
    gen = torch.Generator().manual_seed(K + M)
    dy, x = _ints(gen, -2, 2, K, M), _ints(gen, -2, 2, K, N)
    dy64, x64 = dy.double(), x.double()
    ref, ref_cs = dy64.t() @ x64, dy64.sum(0)
    assert (dy64.abs().t() @ x64.abs()).max().item() < 2 ** 24
    assert dy64.abs().sum(0).max().item() < 2 ** 24

    dw, cs = ext.wgrad_colsum(dy, x)
    assert dw.dtype == torch.float32 and dw.shape == (M, N)
    assert cs.dtype == torch.float32 and cs.shape == (M,)
    assert dw.is_contiguous() and cs.is_contiguous()
    assert torch.equal(dw, ref.float()), (
        f"dW: {int((dw != ref.float()).sum())} elements differ, max |diff| "
        f"{(dw.double() - ref).abs().max().item()}")
    assert torch.equal(cs, ref_cs.float()), (
        f"colsum: {int((cs != ref_cs.float()).sum())} elements differ, max "
        f"|diff| {(cs.double() - ref_cs).abs().max().item()}")
    # the entry point without the column sum
    plain = ext.wgrad(dy, x)
    assert plain.dtype == torch.float32 and plain.shape == (M, N)
    assert torch.equal(plain, ref.float())


@pytest.mark.parametrize("K,M,N", [(1000, 40, 136), (70001, 8, 256)])
def test_stream_random_values(ext, K, M, N):
    gen = torch.Generator().manual_seed(K)
    dy, x = _randn(gen, K, M, scale=0.5), _randn(gen, K, N, scale=0.5)
    dy64, x64 = dy.double(), x.double()
    dw, cs = ext.wgrad_colsum(dy, x)
    _assert_bound("dW", dw, dy64.t() @ x64,
                  1e-5 * (dy64.abs().t() @ x64.abs()))
    _assert_bound("colsum", cs, dy64.sum(0), 1e-5 * dy64.abs().sum(0))
    # fixed slot order and fixed fold order: the same bits on every launch
    dw2, cs2 = ext.wgrad_colsum(dy, x)
    assert torch.equal(dw, dw2) and torch.equal(cs, cs2)
    assert torch.equal(ext.wgrad(dy, x), ext.wgrad(dy, x))


def test_stream_rejects_bad_operands(ext):
    a = torch.zeros(64, 16, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError):
        ext.wgrad_colsum(a, a[:32])                 # K mismatch
    with pytest.raises(RuntimeError):
        ext.wgrad_colsum(a[:, :8], a)               # not contiguous
    with pytest.raises(RuntimeError):
        ext.wgrad_colsum(a.float(), a)              # dtype
    with pytest.raises(RuntimeError):
        ext.wgrad_colsum(torch.zeros(64, 12, dtype=BF, device=DEV), a)
    with pytest.raises(RuntimeError):
        # contiguous but 8 bytes off a 16-byte boundary
        ext.wgrad_colsum(a.view(-1)[4:4 + 32 * 16].view(32, 16), a[:32])


# ---------------------------------------------------------------------------
# autograd level: hip_linear with bias, 70001 rows, 40 -> 136 features

ROWS, FIN, FOUT = 70001, 40, 136


@pytest.fixture(scope="module")
def lin():
    """Operands, float64 references and bounds; shared, never modified."""
    gen = torch.Generator().manual_seed(21)
    x, w = _randn(gen, ROWS, FIN), _randn(gen, FOUT, FIN, scale=0.1)
    b, dy = _randn(gen, FOUT), _randn(gen, ROWS, FOUT, scale=0.5)
    x64, dy64 = x.double(), dy.double()

    def bound(ref, S):
        return 2.0 ** -7 * ref.abs() + 1e-5 * S + 1e-6

    dw_ref, dw_S = dy64.t() @ x64, dy64.abs().t() @ x64.abs()
    db_ref, db_S = dy64.sum(0), dy64.abs().sum(0)
    return dict(x=x, w=w, b=b, dy=dy, dw_ref=dw_ref, db_ref=db_ref,
                dw_bound=bound(dw_ref, dw_S), db_bound=bound(db_ref, db_S))


def _backward(lin, rows=None):
    from alphafold2_amd.ops.hip_autograd import hip_linear
    x, dy = (lin['x'], lin['dy']) if rows is None else \
        (lin['x'][:rows].contiguous(), lin['dy'][:rows].contiguous())
    leaves = [t.clone().requires_grad_(True)
              for t in (x, lin['w'], lin['b'])]
    hip_linear(*leaves).backward(dy)
    return leaves[1].grad, leaves[2].grad


def _spies(ext):
    return (mock.patch.object(ext, 'wgrad_colsum', wraps=ext.wgrad_colsum),
            mock.patch.object(ext, 'wgrad', wraps=ext.wgrad),
            mock.patch.object(ext, 'wgrad_v1', wraps=ext.wgrad_v1))


def test_linear_backward_takes_colsum_kernel(ext, lin):
    """dW and db of one Linear come from ONE launch of the column-sum entry
    point, within the float64 bound."""
    s_cs, s_plain, s_v1 = _spies(ext)
    with s_cs as cs, s_plain as plain, s_v1 as v1:
        dw, db = _backward(lin)
    assert cs.call_count == 1 and plain.call_count == 0
    assert v1.call_count == 0
    _assert_bound("dW", dw, lin['dw_ref'], lin['dw_bound'])
    _assert_bound("db", db, lin['db_ref'], lin['db_bound'])


def test_linear_backward_v1_switch(ext, lin):
    """With the AF2AMD_WGRAD_V1 switch on, the r02 kernel computes dW and a
    separate reduction db."""
    from alphafold2_amd.ops import hip_autograd
    s_cs, s_plain, s_v1 = _spies(ext)
    with mock.patch.object(hip_autograd, '_WGRAD_V1', True), \
            s_cs as cs, s_plain as plain, s_v1 as v1:
        dw, db = _backward(lin)
    assert v1.call_count == 1
    assert cs.call_count == 0 and plain.call_count == 0
    _assert_bound("dW", dw, lin['dw_ref'], lin['dw_bound'])
    _assert_bound("db", db, lin['db_ref'], lin['db_bound'])


def test_linear_backward_small_k_stays_on_library(ext, lin):
    s_cs, s_plain, s_v1 = _spies(ext)
    with s_cs as cs, s_plain as plain, s_v1 as v1:
        dw, db = _backward(lin, rows=200)
    assert cs.call_count == 0 and plain.call_count == 0
    assert v1.call_count == 0
    x64, dy64 = lin['x'][:200].double(), lin['dy'][:200].double()

    def bound(ref, S):
        return 2.0 ** -7 * ref.abs() + 1e-5 * S + 1e-6

    _assert_bound("dW", dw, dy64.t() @ x64,
                  bound(dy64.t() @ x64, dy64.abs().t() @ x64.abs()))
    _assert_bound("db", db, dy64.sum(0),
                  bound(dy64.sum(0), dy64.abs().sum(0)))


def test_linear_backward_graph_capture(ext, lin):
    """The backward captured into a graph on one stream (partials and
    outputs from the torch allocator) and replayed twice equals the eager
    result bit for bit."""
    from alphafold2_amd.ops.hip_autograd import hip_linear
    dw_eager, db_eager = _backward(lin)

    leaves = [t.clone().requires_grad_(True)
              for t in (lin['x'], lin['w'], lin['b'])]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(hip_linear(*leaves), leaves[1:], lin['dy'])
    torch.cuda.current_stream().wait_stream(side)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dw, db = torch.autograd.grad(hip_linear(*leaves), leaves[1:],
                                     lin['dy'])
    for _ in range(2):
        dw.zero_()
        db.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dw, dw_eager)
        assert torch.equal(db, db_eager)
