"""ffgemm.hip (linear_fwd, ff1_geglu_fwd) and wgrad.hip against float64.

Exact-integer cases: operands are small integers stored in bf16, so every
product and every fp32 partial sum is an exact integer in any summation
order (split-K atomics included) and the result must be bit-equal to the
float64 result cast to the output dtype.  The precondition (bf16 outputs
stay <= 256, fp32 sums < 2**24) is asserted on the reference alone.

Random-valued cases use the elementwise bound
    |got - ref64| <= T * |ref64| + c * S + 1e-6
with T the output format's 2**-8 (bf16) / 1e-5 (fp32), S the float64 sum of
the absolute values of the summed terms and c = 1e-5 for their fp32
accumulation.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ext():
    from alphafold2_amd.ops.dispatch import _load_ext
    e = _load_ext()
    assert e is not None, "extension must load on GPU box"
    return e


def _ints(gen, lo, hi, *shape):
    """Integers in [lo, hi] as bf16 on the device (drawn on the CPU so the
    values do not depend on the device generator)."""
    return torch.randint(lo, hi + 1, shape, generator=gen).to(BF).to(DEV)


def _randn(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(BF).to(DEV)


def _gelu64(g):
    return 0.5 * g * (1.0 + torch.erf(g * 0.5 ** 0.5))


def _gelu_grad64(g):
    cdf = 0.5 * (1.0 + torch.erf(g * 0.5 ** 0.5))
    pdf = torch.exp(-0.5 * g * g) * 0.3989422804014327
    return cdf + g * pdf


def _assert_bound(name, got, ref, bound):
    assert got.shape == ref.shape, name
    err = (got.double() - ref).abs()
    bad = err > bound
    assert not bad.any(), (
        f"{name}: {int(bad.sum())} of {bad.numel()} elements off, worst "
        f"err/bound {(err / bound).max().item():.3g}, max err "
        f"{err.max().item():.3e}")


# ---------------------------------------------------------------------------
# linear_fwd

# (130, 72, 136): M tail, K % 64 == 8 (padded staging, short last K step),
#   N % 128 == 8 (second column tile of 8)
# (64, 200, 8):   K = 3 * 64 + 8, a single 8-wide column tile
# (257, 512, 192): three row tiles with a 1-row tail, 8 K steps, N tail 64
# (1, 8, 8):      the smallest legal problem
# (128, 64, 128): exactly one full tile, one K step
LINEAR_SHAPES = [(130, 72, 136), (64, 200, 8), (257, 512, 192), (1, 8, 8),
                 (128, 64, 128)]


@pytest.mark.parametrize("M,K,N", LINEAR_SHAPES)
def test_linear_fwd_exact_integers(ext, M, K, N):
    gen = torch.Generator().manual_seed(M * 1000 + K)
    x, w = _ints(gen, -2, 2, M, K), _ints(gen, -2, 2, N, K)
    b, r = _ints(gen, -4, 4, N), _ints(gen, -8, 8, M, N)
    acc = x.double() @ w.double().t()
    stages = [-1, 0] + ([1] if K % 64 == 0 else [])
    for tag, bias, resid, ref in (
            ("plain", None, None, acc),
            ("bias", b, None, acc + b.double()),
            ("bias+resid", b, r, acc + b.double() + r.double())):
        # integers up to 256 are exact in bf16, also the pre-residual value
        assert ref.abs().max().item() <= 256, tag
        assert (acc + b.double()).abs().max().item() <= 256
        want = ref.to(BF)
        outs = [ext.linear_fwd(x, w, bias, resid, st) for st in stages]
        for st, got in zip(stages, outs):
            assert got.dtype == BF and got.shape == (M, N)
            assert torch.equal(got, want), (
                f"{tag} stage={st}: {int((got != want).sum())} elements "
                f"differ, max |diff| "
                f"{(got.double() - ref).abs().max().item()}")
            assert torch.equal(got, outs[0]), f"{tag}: stage {st} differs"


def test_linear_fwd_random_values(ext):
    M, K, N = 130, 72, 136
    gen = torch.Generator().manual_seed(11)
    x, w = _randn(gen, M, K), _randn(gen, N, K, scale=0.1)
    b = _randn(gen, N)
    ref = x.double() @ w.double().t() + b.double()
    S = x.double().abs() @ w.double().abs().t() + b.double().abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-5 * S + 1e-6
    outs = [ext.linear_fwd(x, w, b, None, st) for st in (-1, 0)]
    for st, got in zip((-1, 0), outs):
        _assert_bound(f"stage={st}", got, ref, bound)
    assert torch.equal(outs[0], outs[1])


def test_forced_dma_stage_needs_k_multiple_of_64(ext):
    """stage=1 reads whole 64-wide K slabs: any other K must be refused
    before a launch, by both entry points."""
    gen = torch.Generator().manual_seed(12)
    x, w = _ints(gen, -2, 2, 16, 72), _ints(gen, -2, 2, 16, 72)
    with pytest.raises(RuntimeError, match="stage"):
        ext.linear_fwd(x, w, None, None, 1)
    with pytest.raises(RuntimeError, match="stage"):
        ext.ff1_geglu_fwd(x, w, None, 1)
    with pytest.raises(RuntimeError, match="stage"):
        ext.ff1_geglu_fwd(x, w, None, 1, False)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# ff1_geglu_fwd

# N/2 = 72: column tail (8) in the second tile; N/2 = 8: in the only tile;
# N/2 = 136: in the third tile.  K = 72 padded staging, K = 64 / 256 DMA.
GEGLU_SHAPES = [(130, 72, 144), (257, 64, 16), (64, 256, 272)]


@pytest.mark.parametrize("M,K,N", GEGLU_SHAPES)
@pytest.mark.parametrize("use_bias", [False, True])
def test_ff1_geglu_fwd_exact_integers(ext, M, K, N, use_bias):
    gen = torch.Generator().manual_seed(M * 1000 + K + 1)
    x, w = _ints(gen, -2, 2, M, K), _ints(gen, -2, 2, N, K)
    b = _ints(gen, -4, 4, N) if use_bias else None
    inter_ref = x.double() @ w.double().t()
    if use_bias:
        inter_ref = inter_ref + b.double()
    assert inter_ref.abs().max().item() <= 256
    val, gate = inter_ref.chunk(2, dim=-1)
    ref = val * _gelu64(gate)
    bound = 2.0 ** -8 * ref.abs() \
        + 1e-6 * val.abs() * (1 + gate.abs()) + 1e-6
    stages = [-1, 0] + ([1] if K % 64 == 0 else [])
    first = None
    for st in stages:
        full = ext.ff1_geglu_fwd(x, w, b, st, True)
        lean = ext.ff1_geglu_fwd(x, w, b, st, False)
        assert len(full) == 2 and len(lean) == 1
        out, inter = full
        assert out.dtype == BF and out.shape == (M, N // 2)
        assert inter.dtype == BF and inter.shape == (M, N)
        assert torch.equal(inter, inter_ref.to(BF)), \
            f"stage={st}: {int((inter != inter_ref.to(BF)).sum())} differ"
        _assert_bound(f"out stage={st}", out, ref, bound)
        assert torch.equal(lean[0], out), f"stage={st}: lean != full"
        first = out if first is None else first
        assert torch.equal(out, first), f"stage {st} differs"


# ---------------------------------------------------------------------------
# wgrad

# (1, 8, 8), (63, 8, 136), (64, 136, 8): K <= 64, one k-slot, the plain
#   store into an uninitialised dW; N / M tile tails of 8
# (65, 40, 264): two k-slots (atomics), second one a single row; three
#   column tiles
# (1000, 128, 128): 16 k-slots, K % 64 != 0, one full tile
# (70001, 40, 136): the K >= 65536 class the autograd wrapper dispatches
WGRAD_SHAPES = [(1, 8, 8), (63, 8, 136), (64, 136, 8), (65, 40, 264),
                (1000, 128, 128), (70001, 40, 136)]


@pytest.mark.parametrize("K,M,N", WGRAD_SHAPES)
def test_wgrad_exact_integers(ext, K, M, N):
    gen = torch.Generator().manual_seed(K)
    dy, x = _ints(gen, -2, 2, K, M), _ints(gen, -2, 2, K, N)
    ref = dy.double().t() @ x.double()
    # every fp32 partial sum is an exact integer
    assert (dy.double().abs().t() @ x.double().abs()).max().item() < 2 ** 24
    got = ext.wgrad(dy, x)
    assert got.dtype == torch.float32 and got.shape == (M, N)
    assert torch.equal(got, ref.float()), (
        f"{int((got != ref.float()).sum())} elements differ, max |diff| "
        f"{(got.double() - ref).abs().max().item()}")


def test_wgrad_random_values(ext):
    K, M, N = 1000, 40, 136
    gen = torch.Generator().manual_seed(13)
    dy, x = _randn(gen, K, M, scale=0.5), _randn(gen, K, N, scale=0.5)
    ref = dy.double().t() @ x.double()
    S = dy.double().abs().t() @ x.double().abs()
    _assert_bound("dW", ext.wgrad(dy, x), ref, 1e-5 * S)


def test_wgrad_autograd_dispatch_is_exact(ext):
    """_wgrad hands K >= 65536 with a small output to the kernel (fp32
    result): exact on integer operands there too."""
    from alphafold2_amd.ops.hip_autograd import _wgrad
    gen = torch.Generator().manual_seed(14)
    dy, x = _ints(gen, -2, 2, 70001, 40), _ints(gen, -2, 2, 70001, 136)
    got = _wgrad(dy, x)
    assert got.dtype == torch.float32
    assert torch.equal(got.double(), dy.double().t() @ x.double())


# ---------------------------------------------------------------------------
# autograd level: every stage against float64 of the tensors it read


@pytest.mark.parametrize("use_bias", [False, True])
def test_hip_linear_autograd_float64(ext, use_bias):
    """y, dx, dW and db are each one GEMM or sum of the bf16 leaves: one
    output rounding, bound 2**-7 |ref| + 1e-5 S."""
    from alphafold2_amd.ops.hip_autograd import hip_linear
    M, K, N = 130, 72, 144
    gen = torch.Generator().manual_seed(15)
    x, w = _randn(gen, M, K), _randn(gen, N, K, scale=0.1)
    b = _randn(gen, N) if use_bias else None
    dy = _randn(gen, M, N)

    leaves = [t.clone().requires_grad_(True) if t is not None else None
              for t in (x, w, b)]
    y = hip_linear(*leaves)
    y.backward(dy)

    x64, w64, dy64 = x.double(), w.double(), dy.double()
    ref = x64 @ w64.t()
    S = x64.abs() @ w64.abs().t()
    if use_bias:
        ref, S = ref + b.double(), S + b.double().abs()

    def bound(ref, S):
        return 2.0 ** -7 * ref.abs() + 1e-5 * S + 1e-6

    _assert_bound("y", y.detach(), ref, bound(ref, S))
    _assert_bound("dx", leaves[0].grad, dy64 @ w64,
                  bound(dy64 @ w64, dy64.abs() @ w64.abs()))
    _assert_bound("dW", leaves[1].grad, dy64.t() @ x64,
                  bound(dy64.t() @ x64, dy64.abs().t() @ x64.abs()))
    if use_bias:
        _assert_bound("db", leaves[2].grad, dy64.sum(0),
                      bound(dy64.sum(0), dy64.abs().sum(0)))


@pytest.mark.parametrize("use_bias", [False, True])
def test_hip_ff1_geglu_autograd_float64(ext, use_bias):
    """The backward has two stages with a bf16 tensor between them: di
    from (dy, inter), then dx / dW / db from di.  Each stage is compared
    with float64 of the rounded tensors it actually read (inter and di as
    the kernels return them), with one output rounding each:
    2**-7 |ref| + 1e-5 S."""
    from alphafold2_amd.ops.hip_autograd import hip_ff1_geglu
    M, K, N = 130, 72, 144
    gen = torch.Generator().manual_seed(16)
    x, w = _randn(gen, M, K), _randn(gen, N, K, scale=0.1)
    b = _randn(gen, N) if use_bias else None
    dy = _randn(gen, M, N // 2)

    leaves = [t.clone().requires_grad_(True) if t is not None else None
              for t in (x, w, b)]
    y = hip_ff1_geglu(*leaves)
    y.backward(dy)

    def bound(ref, S):
        return 2.0 ** -7 * ref.abs() + 1e-5 * S + 1e-6

    # forward: both halves of the pre-activation come from fp32 sums
    x64, w64, dy64 = x.double(), w.double(), dy.double()
    pre = x64 @ w64.t()
    S = x64.abs() @ w64.abs().t()
    if use_bias:
        pre, S = pre + b.double(), S + b.double().abs()
    val, gate = pre.chunk(2, dim=-1)
    Sv, Sg = S.chunk(2, dim=-1)
    ref = val * _gelu64(gate)
    _assert_bound("y", y.detach(), ref, bound(
        ref, Sv * _gelu64(gate).abs() + val.abs() * _gelu_grad64(gate).abs()
        * Sg) + 1e-6 * val.abs() * (1 + gate.abs()))

    # stage 1: the saved pre-activation and the kernel's di
    out, inter = ext.ff1_geglu_fwd(x, w, b)
    assert torch.equal(out, y.detach())
    _assert_bound("inter", inter, pre,
                  2.0 ** -8 * pre.abs() + 1e-5 * S + 1e-6)
    a64, g64 = inter.double().chunk(2, dim=-1)
    di_ref = torch.cat([dy64 * _gelu64(g64),
                        dy64 * a64 * _gelu_grad64(g64)], dim=-1)
    di_S = torch.cat([dy64.abs() * (1 + g64.abs()),
                      (dy64 * a64).abs() * (1 + g64.abs())], dim=-1)
    di = ext.geglu_bwd(dy, inter)
    _assert_bound("di", di, di_ref,
                  2.0 ** -8 * di_ref.abs() + 1e-6 * di_S + 1e-6)
    if use_bias:
        di_cs, colsum = ext.geglu_bwd_colsum(dy, inter)
        assert torch.equal(di_cs, di)
        assert colsum.dtype == torch.float32
        _assert_bound("colsum", colsum, di.float().sum(0).double(),
                      1e-5 * di.double().abs().sum(0))

    # stage 2: GEMMs and the column sum over the rounded di
    di64 = di.double()
    _assert_bound("dx", leaves[0].grad, di64 @ w64,
                  bound(di64 @ w64, di64.abs() @ w64.abs()))
    _assert_bound("dW", leaves[1].grad, di64.t() @ x64,
                  bound(di64.t() @ x64, di64.abs().t() @ x64.abs()))
    if use_bias:
        _assert_bound("db", leaves[2].grad, di64.sum(0),
                      bound(di64.sum(0), di64.abs().sum(0)))
