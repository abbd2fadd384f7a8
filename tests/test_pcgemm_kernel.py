"""Per-channel GEMM kernels (ops/hip/pcgemm.hip), called directly through
`_pcg`, against an fp64 einsum of the same bf16 inputs.

Elementwise bound:  |out - ref| <= 2^-8 |ref| + K 2^-22 |alpha| sum_k |a||b|.
Rounding the fp32 result to bf16 (round to nearest) is 2^-9 relative, so
the first term leaves a factor 2; the second bounds the fp32 accumulation
of K products (K 2^-24 sum|a||b| to first order, a factor 4 left) plus
the alpha multiply.  The bound belongs to neither kernel: run this file
once more with AF2AMD_PCGEMM_V1=1 and the default calls go through the
scatter-staging kernel.

Three kernels: scatter staging (variant 1, what AF2AMD_PCGEMM_V1=1
selects), wide stores (variant 2, same 64x64 tile, off by default) and
the full-line kernel (variant 3, 32x32 tile and all 64 channels of a
line per block; the default wherever D is a multiple of 64).  The
wide-store kernel keeps k ascending in the same 32-wide MFMA steps as
the scatter-staging one, so every case asserts `torch.equal` between
those two.  The full-line kernel sums k in 16-wide MFMA steps and is NOT
bit-equal to them; it is held to the fp64 bound alone.

Shapes are the smallest that can break the staging: sizes that are no
multiple of the 64x64 or the 32x32 tile, K that is no multiple of the
32- or 16-wide k-step nor of a thread's 8-wide k-group, K below one
k-step, one tile and several, one channel chunk, chunk counts that are
no multiple of 8, one and several 64-channel groups, a grid with the
XCD swizzle of the 64x64 kernels on (D = 64, blocks a multiple of 64)
and off, block counts that are and are not a multiple of 8 (the
full-line kernel's block remap), every stride class, and operands that
are channel, row and batch slices of larger tensors.
"""
import functools

import pytest
import torch

gpu = pytest.mark.gpu

# (b, M, N, K, D)
SHAPES = [
    (2, 72, 100, 40, 24),    # M != N != K, 2x2 tiles, 3 chunks
    (2, 40, 24, 8, 8),       # one tile, K below one k-step, one chunk
    (1, 24, 40, 24, 72),     # one tile, K = 24 < 32, 9 chunks
    (1, 136, 8, 100, 24),    # 3x1 tiles, K no multiple of 8
    (1, 100, 136, 136, 136),  # 17 chunks, 4 full k-steps + 8
    (4, 136, 72, 100, 64),   # 6 tiles x 4 x 8 chunks = 192 blocks: swizzle
    # D % 64 == 0: the full-line kernel by default (32x32 tiles)
    (1, 40, 24, 8, 64),      # 2 blocks, K below one 16-wide k-step
    (2, 72, 100, 40, 128),   # 3x4 tiles x 2 x 2 groups = 48 blocks
    (1, 136, 8, 100, 64),    # 5 blocks, K = 6 steps + 4
    (1, 24, 40, 24, 192),    # 6 blocks, 3 groups, K = 1 step + 8
]
AXES = [(1, 2), (2, 1)]
ALPHAS = [1.0, 1.0 / 24]


def _operand(b, rows, k, D, axes, seed, sliced):
    """bf16 (b, ., ., D) operand whose `axes[0]` axis has `rows` entries
    and `axes[1]` axis `k`.  sliced: a channel, row and batch slice of a
    larger tensor, so that no stride is the packed one."""
    g = torch.Generator().manual_seed(seed)
    s1, s2 = (rows, k) if axes == (1, 2) else (k, rows)
    if not sliced:
        return torch.randn(b, s1, s2, D, generator=g).bfloat16().cuda()
    big = torch.randn(2 * b, s1 + 3, s2 + 5, D + 16, generator=g)
    big = big.bfloat16().cuda()
    return big[::2, 1:1 + s1, 2:2 + s2].narrow(-1, 8, D)


@functools.lru_cache(maxsize=None)
def _case(shape, a_axes, b_axes, sliced=False):
    """(A, B, ref, absprod) of a case; ref and absprod are fp64 and for
    alpha = 1.  Computed once and shared; nothing writes to them."""
    b, M, N, K, D = shape
    A = _operand(b, M, K, D, a_axes, 1, sliced)
    B = _operand(b, N, K, D, b_axes, 2, sliced)
    a64 = A.double().permute(0, a_axes[0], a_axes[1], 3)
    b64 = B.double().permute(0, b_axes[0], b_axes[1], 3)
    ref = torch.einsum('bmkd,bnkd->bmnd', a64, b64)
    absprod = torch.einsum('bmkd,bnkd->bmnd', a64.abs(), b64.abs())
    return A, B, ref, absprod


def _check(shape, a_axes, b_axes, alpha, sliced=False):
    from alphafold2_amd.ops.hip_autograd import _pcg
    b, M, N, K, D = shape
    A, B, ref, absprod = _case(shape, a_axes, b_axes, sliced)
    run = lambda v: _pcg(A, B, M, N, K, a_axes[0], a_axes[1],
                         b_axes[0], b_axes[1], alpha=alpha, variant=v)
    out = run(0)
    assert out.shape == (b, M, N, D) and out.is_contiguous()
    ref = ref * alpha
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -22 * abs(alpha) * absprod
    excess = ((out.double() - ref).abs() - bound).max().item()
    print(f"PCG_ERR {shape} a{a_axes} b{b_axes} alpha={alpha:.4f} "
          f"sliced={sliced}: max err "
          f"{(out.double() - ref).abs().max().item():.3e}, max of "
          f"err - bound {excess:.3e}, max |ref| {ref.abs().max().item():.3e}")
    assert excess <= 0
    assert torch.equal(run(1), run(2)), "scatter and wide kernels differ"


@gpu
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("b_axes", AXES)
@pytest.mark.parametrize("a_axes", AXES)
@pytest.mark.parametrize("shape", SHAPES)
def test_pcgemm_against_fp64(shape, a_axes, b_axes, alpha):
    _check(shape, a_axes, b_axes, alpha)


@gpu
@pytest.mark.parametrize("D", [24, 64])
@pytest.mark.parametrize("b_axes", AXES)
@pytest.mark.parametrize("a_axes", AXES)
def test_pcgemm_sliced_operands(a_axes, b_axes, D):
    """narrow(-1, 8, D) of a D + 16 tensor, rows 1.. and 2.. of longer
    axes, every second batch entry: batch, row and k strides all differ
    from the packed ones and the base pointer is offset."""
    _check((2, 72, 100, 40, D), a_axes, b_axes, 1.0 / 24, sliced=True)


@gpu
@pytest.mark.parametrize("d", [24, 64])
@pytest.mark.parametrize("mix", ['outgoing', 'ingoing'])
def test_triangle_mix_autograd(mix, d):
    from alphafold2_amd.ops import eager
    from alphafold2_amd.ops.hip_autograd import hip_triangle_mix
    b, n = 2, 40
    g = torch.Generator().manual_seed(3)
    left, right, w = (torch.randn(b, n, n, d, generator=g).bfloat16().cuda()
                      for _ in range(3))
    l1, r1 = (t.clone().requires_grad_(True) for t in (left, right))
    l2, r2 = (t.float().clone().requires_grad_(True) for t in (left, right))
    out1 = hip_triangle_mix(l1, r1, mix)
    out2 = eager.triangle_mix(l2, r2, mix)
    scale = out2.abs().max().item()
    assert (out1.float() - out2).abs().max().item() < 5e-2 * scale
    out1.backward(w)
    out2.backward(w.float())
    for a1, a2, name in [(l1, l2, 'dL'), (r1, r2, 'dR')]:
        gs = a2.grad.abs().max().item()
        err = (a1.grad.float() - a2.grad).abs().max().item()
        assert err < 5e-2 * gs, f"{mix} {name}: {err} vs scale {gs}"


@gpu
@pytest.mark.parametrize("d", [24, 64])
def test_outer_product_mean_autograd_masked(d):
    from alphafold2_amd.ops import eager
    from alphafold2_amd.ops.hip_autograd import hip_outer_product_mean
    b, m, n = 2, 24, 40
    g = torch.Generator().manual_seed(4)
    left, right = (torch.randn(b, m, n, d, generator=g).bfloat16().cuda()
                   for _ in range(2))
    w = torch.randn(b, n, n, d, generator=g).bfloat16().cuda()
    mask = (torch.rand(b, m, n, generator=g) > 0.2).cuda()
    l1, r1 = (t.clone().requires_grad_(True) for t in (left, right))
    l2, r2 = (t.float().clone().requires_grad_(True) for t in (left, right))
    out1 = hip_outer_product_mean(l1, r1, mask=mask)
    out2 = eager.outer_product_mean(l2, r2, mask=mask)
    scale = out2.abs().max().item()
    assert (out1.float() - out2).abs().max().item() < 5e-2 * scale
    out1.backward(w)
    out2.backward(w.float())
    for a1, a2, name in [(l1, l2, 'dL'), (r1, r2, 'dR')]:
        gs = a2.grad.abs().max().item()
        err = (a1.grad.float() - a2.grad).abs().max().item()
        assert err < 6e-2 * gs, f"{name}: {err} vs scale {gs}"


def _ext_or_skip():
    from alphafold2_amd.ops.dispatch import _load_ext
    ext = _load_ext()
    if ext is None:
        pytest.skip("the extension is not built in this tree")
    return ext


def test_pcgemm_rejects_misaligned_operands():
    """The kernels reinterpret 8 channels as one 16-byte vector: the
    entry refuses strides and base pointers that break that, before it
    touches a device (so CPU tensors do for the test)."""
    ext = _ext_or_skip()
    a = torch.zeros(1, 8, 8, 16, dtype=torch.bfloat16)
    ok = (a.stride(0), a.stride(1), a.stride(2))
    for pos in range(6):
        strides = list(ok + ok)
        strides[pos] += 4
        with pytest.raises(RuntimeError, match="multiple of 8 elements"):
            ext.pcgemm(a, a, 1, 8, 8, 8, 8, *strides, 1.0)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ext.pcgemm(a[..., 4:12], a, 1, 8, 8, 8, 8, *ok, *ok, 1.0)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.pcgemm(a, a, 1, 8, 8, 8, 12, *ok, *ok, 1.0)
    with pytest.raises(RuntimeError, match="fit int"):
        ext.pcgemm(a, a, 1, 2 ** 31, 8, 8, 8, *ok, *ok, 1.0)
    with pytest.raises(RuntimeError, match="D % 64"):
        ext.pcgemm(a, a, 1, 8, 8, 8, 8, *ok, *ok, 1.0, 3)
